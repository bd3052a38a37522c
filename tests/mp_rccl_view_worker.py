"""Rank process of the RCCL view test (tests/test_view_gpu.py).

Started by torch.distributed.run, N processes on ONE GPU, each with its own
NCCL_HOSTID (see tests/mp_rccl_worker.py).  The native RcclTransport then sums
the ranks' shares of a density map, and their disjoint pieces of a window,
with ncclAllReduce(ncclSum, ncclUint64); every rank checks the complete results
it was given against NumPy on the grid stepped by the fp32 PyTorch oracle, and
the grid after a stamp over the rank boundary and more generations.

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
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import gol_amd  # noqa: E402
from gol_amd.ops.life_ops import life_step_torch  # noqa: E402
from gol_amd.parallel.dist import gather_grid  # noqa: E402

from test_view import GLIDER, density_oracle  # noqa: E402


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
        W = 32 * 24 * px if layout == "bits" else 32 * 24 * px + 7
        H = 100 * py + 13
        gens = 20
        g = gol_amd.random_grid(W, H, 17 + px * 10 + py, 0.4)
        cfg = gol_amd.LifeConfig(W, H, gen_limit=1000, check_similarity=False, decomp=decomp, layout=layout, tmax=8,
                                 epoch=16)
        sim = gol_amd.Simulation(cfg, transport=tr, backend=be)
        sim.load(g)
        sim.advance(gens)
        want = np.array(life_step_torch(g, gens, device="cuda"))
        ok = True
        for by, bx in [(32, 32), (33, 5), (H, W)]:
            ok &= bool(np.array_equal(sim.density((by, bx)), density_oracle(want, by, bx)))
        x, y = W // 2 - 20, H // 2 - 9  # over the boundary of the two ranks, whichever way it runs
        ok &= bool(np.array_equal(sim.window(x, y, 41, 19), want[y:y + 19, x:x + 41]))
        ok &= bool(np.array_equal(sim.window(0, 0, W, H), want))
        sim.place(GLIDER, W // 2 - 1, H // 2 - 1, mode="or")
        want[H // 2 - 1:H // 2 + 2, W // 2 - 1:W // 2 + 2] |= GLIDER
        sim.advance(gens)
        full = gather_grid(sim)
        ok &= rank != 0 or bool(np.array_equal(full, life_step_torch(want, gens, device="cuda")))
        log(case, "exact" if ok else "MISMATCH")
        if not ok:
            failures.append(case)
        del sim
    res = torch.tensor([len(failures)])
    dist.all_reduce(res, op=dist.ReduceOp.MAX)
    if rank == 0:
        print(f"VIEW {'PASS' if res.item() == 0 else 'FAIL'} world={world}", flush=True)
    if failures:
        log("failures:", failures)
    del tr
    dist.destroy_process_group()
    return 0 if res.item() == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
