"""Rank process of the RCCL fingerprint test (tests/test_cycle_gpu.py).

Started by torch.distributed.run, N processes on ONE GPU, each with its own
NCCL_HOSTID (see tests/mp_rccl_worker.py).  The native RcclTransport then sums
the per-rank fingerprint shares with ncclAllReduce(ncclSum, ncclUint64), modulo
2^64, and every rank checks the whole series it was given, the stand-alone
fingerprint of the final grid and the gathered grid against the fp32 PyTorch
conv2d oracle stepped one generation at a time and the NumPy fingerprint of
tests/cycle_oracle.py.  The byte case runs the byte kernels on a width that is a
multiple of 32, so that the second rank's tile starts on the word grid, at a
non-zero word.

    argv: CASES   comma-separated decomp:layout, e.g. 1x2:bits
"""
import os
import sys

rank = int(os.environ["RANK"])
world = int(os.environ["WORLD_SIZE"])
os.environ["NCCL_HOSTID"] = f"gol-test-rank{rank}"
os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import cycle_oracle as co  # noqa: E402
import gol_amd  # noqa: E402
from gol_amd.ops.life_ops import life_step_torch  # noqa: E402
from gol_amd.parallel.dist import gather_grid  # noqa: E402


def log(*a):
    print(f"[rank {rank}]", *a, file=sys.stderr, flush=True)


def main() -> int:
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    C = gol_amd.native()
    obj = [C.rccl_unique_id() if rank == 0 else None]
    dist.broadcast_object_list(obj, src=0)
    tr = C.rccl_transport(obj[0], rank, world, 0)
    be = C.hip_backend(0)
    failures = []
    for case in sys.argv[1].split(","):
        decomp, layout = case.split(":")
        px, py = (int(v) for v in decomp.split("x"))
        W = 32 * 24 * px
        H = 200 * py + 13
        gens = 70
        g = gol_amd.random_grid(W, H, 17 + px * 10 + py, 0.4)
        cfg = gol_amd.LifeConfig(W, H, gen_limit=gens, check_similarity=False, decomp=decomp, layout=layout, tmax=8,
                                 epoch=16, fingerprint=True, tune={"u8_via_bits": "0"})
        sim = gol_amd.Simulation(cfg, transport=tr, backend=be)
        sim.load(g)
        rep = sim.advance(gens)
        full = gather_grid(sim)
        last = sim.fingerprint()
        x, fps = g, []
        for _ in range(gens):
            x = life_step_torch(x, 1, device="cuda")
            fps.append(co.fingerprint(x))
        ok = (rep.fingerprint.tolist() == fps and last == fps[-1]
              and (rank != 0 or bool(np.array_equal(full, x))))
        log(case, "exact" if ok else "MISMATCH", rep.fingerprint[:4].tolist(), fps[:4])
        if not ok:
            failures.append(case)
        del sim
    res = torch.tensor([len(failures)])
    dist.all_reduce(res, op=dist.ReduceOp.MAX)
    if rank == 0:
        print(f"CYCLE {'PASS' if res.item() == 0 else 'FAIL'} world={world}", flush=True)
    if failures:
        log("failures:", failures)
    del tr
    dist.destroy_process_group()
    return 0 if res.item() == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
