#!/usr/bin/env python3
"""Regenerate tests/golden/game_c/: what the reference's serial src/game.c
(compiled in a scratch directory, never vendored) prints and writes on every
input test_golden_reference.py feeds it - the GRIDS inputs, the square golden
patterns and the stdout-contract grid - so that the suite compares against
the reference on a box that does not have it.

    python tests/make_game_c_fixtures.py /path/to/reference/src/game.c

generations.json / <N>_<seed>_<density>.out.gz: the GRIDS runs by name.
recorded.json: every run by the sha256 of its input file (conftest.py
RecordedReference replays them).
"""
import gzip
import hashlib
import json
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE))

from gol_amd.utils import io  # noqa: E402
from golden import CASES  # noqa: E402
from test_golden_reference import GRIDS, STDOUT_GRID  # noqa: E402


def main() -> int:
    if len(sys.argv) != 2:
        print(__doc__, file=sys.stderr)
        return 2
    src = Path(sys.argv[1])
    out_dir = HERE / "golden" / "game_c"
    out_dir.mkdir(parents=True, exist_ok=True)
    index, recorded = {}, {}
    with tempfile.TemporaryDirectory() as d:
        d = Path(d)
        exe = d / "game_serial"
        subprocess.run([shutil.which("gcc"), "-std=c99", "-O3", str(src), "-o", str(exe)], check=True)

        def record(key: str, N: int, f: Path) -> str:
            r = subprocess.run([str(exe), str(N), str(N), str(f)], cwd=d, capture_output=True, text=True,
                               check=True)
            data = (d / "game_output.out").read_bytes()
            with gzip.GzipFile(out_dir / f"{key}.out.gz", "wb", mtime=0) as g:
                g.write(data)
            recorded[hashlib.sha256(f.read_bytes()).hexdigest()] = {"name": key, "N": N, "stdout": r.stdout}
            return next(ln for ln in r.stdout.splitlines() if ln.startswith("Generations:"))

        for N, seed, density in [*GRIDS, STDOUT_GRID]:
            key = f"{N}_{seed}_{density}"
            f = d / f"{key}.txt"
            io.generate(str(f), N, N, seed=seed, density=density)
            gens = record(key, N, f)
            if (N, seed, density) in GRIDS:
                index[key] = gens
        for name, grid, _ in CASES:
            if grid.shape[0] == grid.shape[1]:
                f = d / f"pattern_{name}.txt"
                io.write_grid(str(f), np.asarray(grid))
                record(f"pattern_{name}", grid.shape[0], f)
    (out_dir / "generations.json").write_text(json.dumps(index, indent=1) + "\n")
    (out_dir / "recorded.json").write_text(json.dumps(recorded, indent=1, sort_keys=True) + "\n")
    print(f"wrote {len(recorded)} recorded runs to {out_dir}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
