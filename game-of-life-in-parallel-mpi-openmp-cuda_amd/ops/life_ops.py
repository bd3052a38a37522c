"""Kernel-level ops and independent oracles.

``life_step``       - n generations of the native kernels (HIP or CPU
                      backend) on one periodic grid, no termination logic.
``life_step_torch`` - plain PyTorch fp32 reference: 3x3 ``conv2d`` with
                      circular padding (the oracle SURVEY 4.3 T1 prescribes;
                      runs on CPU or on the GPU).
``life_step_numpy`` - NumPy ``roll``-sum reference.

Every one of them takes ``boundary="torus"`` (default) or ``"dead"``, the
bounded plane whose outside is dead in every generation.
"""
from __future__ import annotations

import numpy as np

from .._native import native


def rule_masks(rule: str = "B3/S23") -> tuple[int, int]:
    """(birth, survive) bit masks of a rule (bit n = at n live neighbours)."""
    b, s = native().parse_rule(str(rule))[1:].split("/S")
    return sum(1 << int(d) for d in b), sum(1 << int(d) for d in s)


def life_step(grid: np.ndarray, gens: int = 1, engine: str = "auto", layout: str = "auto",
              tmax: int = 0, epoch: int = 0, device: int = 0, rule: str = "B3/S23",
              boundary: str = "torus") -> np.ndarray:
    """Advance ``grid`` (H x W, 0/1 uint8) by exactly ``gens`` generations."""
    from ..models.life import LifeConfig, Simulation  # noqa: PLC0415

    g = np.ascontiguousarray(grid, dtype=np.uint8)
    H, W = g.shape
    cfg = LifeConfig(W, H, gen_limit=int(gens), layout=layout, tmax=tmax, epoch=epoch, rule=rule,
                     boundary=boundary)
    sim = Simulation(cfg, engine=engine, device=device)
    sim.load(g)
    sim.advance(int(gens))
    return sim.tile()


def _check_boundary(boundary: str) -> bool:
    """True for the bounded plane."""
    if boundary not in ("torus", "dead"):
        raise ValueError(f"bad boundary {boundary!r} (want torus or dead)")
    return boundary == "dead"


def life_step_numpy(grid: np.ndarray, gens: int = 1, rule: str = "B3/S23", boundary: str = "torus") -> np.ndarray:
    birth, survive = rule_masks(rule)
    dead = _check_boundary(boundary)
    lut = np.array([[(birth >> n) & 1 for n in range(9)], [(survive >> n) & 1 for n in range(9)]], dtype=np.uint8)
    g = (np.asarray(grid) != 0).astype(np.uint8)
    H, W = g.shape
    for _ in range(gens):
        if dead:  # a moat of dead cells, rebuilt every generation: nothing is ever born in it
            p = np.pad(g, 1)
            n = sum(p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                    if (dy, dx) != (0, 0))
        else:
            n = sum(np.roll(np.roll(g, dy, 0), dx, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                    if (dy, dx) != (0, 0))
        g = lut[g, n]
    return g


def _torch_rule(n, t, birth: int, survive: int):
    """Next generation (bool) from fp32 neighbour counts ``n`` (exact: small
    integers) and cells ``t``: the rule's plain definition, count by count."""
    import torch  # noqa: PLC0415

    born = torch.zeros_like(n, dtype=torch.bool)
    stay = torch.zeros_like(n, dtype=torch.bool)
    for k in range(9):
        if (birth >> k) & 1:
            born |= n == k
        if (survive >> k) & 1:
            stay |= n == k
    return torch.where(t == 1, stay, born)


def life_step_torch(grid, gens: int = 1, device: str = "cpu", rule: str = "B3/S23", boundary: str = "torus"):
    """fp32 PyTorch reference of a Life-like rule (default B3/S23) on a torus
    (conv2d, circular pad) or the bounded plane (conv2d on a zero-padded input)."""
    import torch  # noqa: PLC0415
    import torch.nn.functional as F  # noqa: PLC0415

    birth, survive = rule_masks(rule)
    dead = _check_boundary(boundary)

    t = torch.as_tensor(np.asarray(grid) != 0, dtype=torch.float32, device=device)[None, None]
    k = torch.ones(1, 1, 3, 3, dtype=torch.float32, device=device)
    k[0, 0, 1, 1] = 0.0
    for _ in range(gens):
        n = F.conv2d(F.pad(t, (1, 1, 1, 1)) if dead else F.pad(t, (1, 1, 1, 1), mode="circular"), k)
        t = _torch_rule(n, t, birth, survive).to(torch.float32)
    return t[0, 0].to(torch.uint8).cpu().numpy()


def life_step_torch_roll(grid, gens: int = 1, device: str = "cpu", rule: str = "B3/S23", boundary: str = "torus"):
    """fp32 PyTorch reference of a Life-like rule on a torus from elementwise ops only
    (separable neighbour sums of rolled copies, no convolution library): the
    verification oracle for whole-benchmark grids, where a first conv2d call
    spends a minute in kernel selection on a fresh box."""
    import torch  # noqa: PLC0415

    birth, survive = rule_masks(rule)
    dead = _check_boundary(boundary)
    t = torch.as_tensor(np.asarray(grid) != 0, dtype=torch.float32, device=device)

    def shifted(a, s, dim):
        """``a`` rolled by ``s`` along ``dim``; on the bounded plane the row or
        column that rolled in from the other side is dead."""
        r = torch.roll(a, s, dim)
        if dead:
            r.select(dim, 0 if s > 0 else -1).zero_()
        return r

    for _ in range(gens):
        h = t + shifted(t, 1, 1) + shifted(t, -1, 1)
        n = h + shifted(h, 1, 0) + shifted(h, -1, 0) - t
        t = _torch_rule(n, t, birth, survive).to(torch.float32)
        del h, n
    return t.to(torch.uint8).cpu().numpy()


def random_grid(width: int, height: int, seed: int = 1, density: float = 0.5) -> np.ndarray:
    """Host copy of the engine's counter-based RNG grid (same as init_random)."""
    return native().random_grid(int(width), int(height), int(seed), float(density))


def rule_words(*words: int, rule=None) -> int:
    """Host emulation of the bit-sliced rule on one word (for ISA-level tests):
    the B3/S23 form, or with ``rule`` the general form and its tables."""
    w = [int(x) & 0xFFFFFFFF for x in words]
    if rule is None:
        return int(native().rule_words(*w))
    return int(native().rule_words_for(str(rule), *w))
