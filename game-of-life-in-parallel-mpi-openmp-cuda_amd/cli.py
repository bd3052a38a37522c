"""Python front end: ``python -m gol_amd W H input_file [options]``.

Same positional contract as the reference (``./a.out <width> <height>
<input_file>``, README.md:50-57) and the native ``bin/gol``; additionally
runs under ``torchrun`` with one process per GPU (the equivalent of
``mpiexec -n P ./a.out``, src/game_mpi.c:2), every rank reading and writing
its own subarray of the text file.

    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 -m gol_amd 32768 32768 in.txt --style mpi
"""
from __future__ import annotations

import argparse
import os
import re
import sys
import time

from .models.life import (DEFAULT_BOUNDARY, DEFAULT_RULE, LifeConfig, Simulation, density_image, make_backend,
                          parse_rule, parse_tune_args, read_rle, reference_run, write_pgm, write_rle)
from .utils.metrics import stdout_lines, write_json


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="gol_amd", description=__doc__.split("\n\n")[0])
    p.add_argument("width", nargs="?", type=int, default=0)
    p.add_argument("height", nargs="?", type=int, default=0)
    p.add_argument("input_file", nargs="?", default=None)
    p.add_argument("--engine", default="auto", choices=["auto", "hip", "cpu", "ref"])
    p.add_argument("--layout", default="auto", choices=["auto", "bits", "u8"])
    p.add_argument("--u8-compute", default="auto", choices=["auto", "bits", "bytes"],
                   help="byte layout: epochs on bit words packed once per epoch (auto: on the GPU) or on the bytes")
    p.add_argument("--rule", default=None, metavar="NAME|B../S..",
                   help="Life-like rule: B<digits>/S<digits> (e.g. B36/S23) or a name (life, highlife, daynight, "
                        "seeds, replicator, lwod, 34life); default B3/S23, no B0; the hip engine runs the named "
                        "ones, the cpu and ref engines any")
    p.add_argument("--boundary", default=None, choices=["torus", "dead"],
                   help="what lies beyond the grid's edge: torus wraps (default); dead = a bounded plane whose "
                        "outside is dead in every generation (hip engine: B3/S23 only, no lds kernels, no graphs)")
    p.add_argument("--census", default=None, metavar="PATH",
                   help="count the live cells of every generation inside the temporal blocks and write "
                        "'generation,population' lines to PATH, one per generation (hip engine: B3/S23 on the torus, "
                        "no lds kernels, no graphs)")
    p.add_argument("--fingerprint", default=None, metavar="PATH",
                   help="accumulate a position-dependent 64-bit fingerprint of every generation inside the temporal "
                        "blocks and write 'generation,fingerprint' lines (16 hex digits) to PATH (hip engine: B3/S23 "
                        "on the torus, no lds kernels, no graphs, no census)")
    p.add_argument("--cycle", type=int, default=None, metavar="P",
                   help="run until the grid repeats with a period <= P (confirmed on the cells) or to the generation "
                        "limit, and print one more line: 'Cycle: period p at generation G (fingerprints repeat from "
                        "E)' or 'Cycle: none within N generations'")
    p.add_argument("--gens", type=int, default=1000, help="GEN_LIMIT")
    p.add_argument("--sim-freq", type=int, default=None, help="SIMILARITY_FREQUENCY (default 3)")
    p.add_argument("--no-similarity", action="store_true")
    p.add_argument("--random", default=None, help="SEED[:DENSITY] random init instead of a file")
    p.add_argument("--output", default=None,
                   help="output path or 'none' (default: the reference build's name for --style)")
    p.add_argument("--decomp", default="auto")
    p.add_argument("--comm", default="auto", choices=["auto", "rccl", "torch"])
    p.add_argument("--tmax", type=int, default=0)
    p.add_argument("--epoch", "--halo-depth", dest="epoch", type=int, default=0,
                   help="generations per halo exchange (deep halo depth)")
    p.add_argument("--poll", "--poll-every", dest="poll", type=int, default=0,
                   help="generations between termination polls")
    p.add_argument("--overlap", default="auto", choices=["auto", "on", "off", "trigger"],
                   help="trigger (= on) = an epoch's boundary rows sent once the groups writing them are done; "
                        "off = no overlap; auto = time plain against trigger epochs on the ranks and keep the "
                        "faster (row strips only)")
    p.add_argument("--graphs", default="off", choices=["auto", "on", "off"],
                   help="replay full epochs as captured HIP graphs")
    p.add_argument("--threads", type=int, default=0)
    p.add_argument("--tune", action="append", default=[], metavar="KEY=VALUE",
                   help="runtime tuning (repeatable; --tune help lists the keys, their GOL_* overrides and defaults)")
    p.add_argument("--style", default="serial", choices=["serial", "mpi", "async", "collective", "openmp", "cuda"])
    p.add_argument("--metrics-json", default=None,
                   help="write run metrics as JSON (per-phase device times with --phase-timing)")
    p.add_argument("--phase-timing", action="store_true",
                   help="time kernels / halos / fills / reductions (adds event pairs inside the timed loop)")
    p.add_argument("--show", action="store_true",
                   help="print the final grid with VT100 escapes (src/game.c:42-58)")
    p.add_argument("--checkpoint-every", type=int, default=0)
    p.add_argument("--checkpoint-dir", default=None)
    p.add_argument("--resume", default=None, help="checkpoint directory to resume from")
    p.add_argument("--place", action="append", default=[], metavar="FILE[@X,Y]",
                   help="stamp the RLE pattern FILE onto the loaded grid (live cells are added), its first cell at "
                        "column X, row Y, or centred; repeatable, in order; with input 'none' the grid starts empty")
    p.add_argument("--density", default=None, metavar="PATH",
                   help="write the block populations of the final grid as a PGM image")
    p.add_argument("--density-block", default=None, metavar="B|BYxBX",
                   help="cells per block (default: the smallest power of two that gives at most 1024 blocks per side)")
    p.add_argument("--density-every", type=int, default=0, metavar="K",
                   help="also one image per generation that is a multiple of K; PATH must contain %%d (any width)")
    p.add_argument("--window", action="append", default=[], metavar="X,Y,W,H:PATH",
                   help="write that rectangle of the final grid: RLE where PATH ends in .rle, else the text format")
    p.add_argument("--batch", type=int, default=None, metavar="N",
                   help="run N independent random universes of width x height cells (width 32 or 64, height 8, 16, "
                        "32 or 64; input 'none', --random SEED[:D]: universe b has seed SEED + b) until each repeats "
                        "or reaches --gens; engines hip and cpu; prints one summary line; not with the "
                        "single-universe outputs and options")
    p.add_argument("--max-period", type=int, default=None, metavar="P",
                   help="--batch: the largest period recognised, 1 to 65536 (default 64)")
    p.add_argument("--batch-csv", default=None, metavar="PATH",
                   help="--batch: write 'universe,seed,generations,stop,period,population' lines, one per universe")
    p.add_argument("--batch-census", default=None, metavar="PATH",
                   help="--batch: find the clusters of every final grid (live cells at most 2 cells apart) and write "
                        "'signature,name,cells,height,width,spanning,count', one line per kind of cluster, the most "
                        "common first")
    p.add_argument("--batch-rules", default=None, metavar="FILE|all",
                   help="--batch with a rule per universe, N = the number of rules R (an explicit --batch N must "
                        "agree): FILE holds one rule per line (# comments and blank lines skipped), all = the 131072 "
                        "Life-like rules without B0; universe b runs rule b on seed SEED + b; any rule on either "
                        "engine; not with --rule; prints a second line 'Rules: R rules x K soups' and adds a 'rule' "
                        "column after 'seed' to --batch-csv")
    p.add_argument("--soups", type=int, default=None, metavar="K",
                   help="--batch-rules: the cross product, N = R * K: universe r*K + j runs rule r on seed SEED + j")
    p.add_argument("--rules-csv", default=None, metavar="PATH",
                   help="--batch-rules: write 'rule,soups,limit,cycle,extinction,mean_generations,max_generations,"
                        "max_period,mean_population' lines, one per rule")
    a = p.parse_args(argv)
    a.output_given = a.output is not None
    a.sim_freq_given = a.sim_freq is not None
    if a.sim_freq is None:
        a.sim_freq = 3
    if a.output is None:  # src/game.c:27, src/game_mpi.c:29, ... src/game_cuda.cu:37
        a.output = f"./{'game' if a.style == 'serial' else a.style}_output.out"
    if a.width <= 0:
        a.width = 30
    if a.height <= 0:
        a.height = 30
    return a


def write_census(path: str, g0: int, population) -> None:
    """``generation,population`` lines, one per generation after ``g0``."""
    with open(path, "w") as f:
        for i, v in enumerate(population):
            f.write(f"{g0 + 1 + i},{int(v)}\n")


def write_fingerprint(path: str, g0: int, fingerprint) -> None:
    """``generation,fingerprint`` lines (16 hex digits), one per generation after ``g0``."""
    with open(path, "w") as f:
        for i, v in enumerate(fingerprint):
            f.write(f"{g0 + 1 + i},{int(v):016x}\n")


def cycle_line(cyc, limit: int) -> str:
    if cyc.period > 0:
        return (f"Cycle: period {cyc.period} at generation {cyc.generation} "
                f"(fingerprints repeat from {cyc.repeats_from})\n")
    return f"Cycle: none within {limit} generations\n"


_FRAME = re.compile(r"%[0-9]*d")


def has_generation_field(path: str) -> bool:
    return path.count("%") == 1 and _FRAME.search(path) is not None


def density_path(path: str, gen: int) -> str:
    return _FRAME.sub(lambda m: m.group(0) % gen, path) if has_generation_field(path) else path


def parse_view_args(a, rule: str):
    """--place / --density* / --window, checked like bin/gol checks them:
    (stamps [(cells, x, y)], (by, bx) or None, windows [(x, y, w, h, path)])."""
    W, H = a.width, a.height
    stamps = []
    for v in a.place:
        file, at, xy = v.rpartition("@")
        m = re.fullmatch(r"(-?\d+),(-?\d+)", xy) if at else None
        if m is None:
            file = v
        try:
            with open(file, "r", encoding="ascii", errors="replace") as f:
                text = f.read()
        except OSError:
            raise SystemExit(f"--place: cannot read '{file}'")
        try:
            cells, prule = read_rle(text + "\n")
        except RuntimeError as e:
            raise SystemExit(f"--place {file}: {e}")
        if prule:
            try:
                prule = parse_rule(prule)
            except RuntimeError as e:
                raise SystemExit(f"--place {file}: {e}")
            if prule != rule:
                raise SystemExit(f"--place {file}: the pattern's rule {prule} is not the engine's {rule}")
        h, w = cells.shape
        x, y = (int(m.group(1)), int(m.group(2))) if m else ((W - w) // 2, (H - h) // 2)
        if x < 0 or y < 0 or w > W - x or h > H - y:
            raise SystemExit(f"--place {file}: rectangle x={x} y={y} w={w} h={h} leaves the grid of {W} x {H} cells "
                             "(patterns do not wrap)")
        stamps.append((cells, x, y))
    block = None
    if a.density_every < 0 or (a.density_every and a.density is None):
        raise SystemExit("--density-every needs K >= 1 and --density PATH")
    if a.density is not None:
        if a.density_every and not has_generation_field(a.density):
            raise SystemExit(f"--density-every: the path '{a.density}' needs one %d (any width) for the generation")
        if not a.density_every and "%" in a.density and not has_generation_field(a.density):
            raise SystemExit(f"--density: the path '{a.density}' may hold one %d (the generation) and no other %")
        if a.density_block is None:
            b = 1
            while -(-max(W, H) // b) > 1024:
                b *= 2
            block = (b, b)
        else:
            m = re.fullmatch(r"(\d+)(?:x(\d+))?", a.density_block)
            if m is None or int(m.group(1)) < 1 or int(m.group(2) or 1) < 1:
                raise SystemExit(f"--density-block: B or BYxBX, got '{a.density_block}'")
            block = (int(m.group(1)), int(m.group(2) or m.group(1)))
    windows = []
    for v in a.window:
        m = re.fullmatch(r"(-?\d+),(-?\d+),(-?\d+),(-?\d+):(.+)", v)
        if m is None:
            raise SystemExit(f"--window: X,Y,W,H:PATH, got '{v}'")
        x, y, w, h = (int(m.group(i)) for i in range(1, 5))
        if w < 1 or h < 1 or x < 0 or y < 0 or w > W - x or h > H - y or w * h > 1 << 26:
            raise SystemExit(f"--window: rectangle x={x} y={y} w={w} h={h} must lie inside the grid of {W} x {H} "
                             "cells and hold at most 2^26 cells")
        windows.append((x, y, w, h, m.group(5)))
    return stamps, block, windows


def write_window_file(path: str, cells, rule: str) -> None:
    if path.endswith(".rle"):
        write_rle(cells, path, rule)
    else:
        from .utils.io import write_grid  # noqa: PLC0415

        write_grid(path, cells)


def print_tuning_keys() -> None:
    from ._native import native  # noqa: PLC0415

    for k in native().tuning_keys():
        print(f"{k['key']:<22} {k['class']:<13} {k['env']:<27} default {k['default'] or repr(''):<6} {k['doc']}")


def batch_summary(n: int, counts: dict, longest: int) -> str:
    return (f"Batch: {n} universes: {counts['limit']} limit, {counts['cycle']} cycle, "
            f"{counts['extinction']} extinction; largest generations {longest}\n")


def load_batch_rules(arg: str) -> list[str]:
    """--batch-rules: the rules of FILE (one per line, # comments and blank
    lines skipped), or all Life-like rules without B0."""
    from .models.batch import life_like_rules  # noqa: PLC0415

    if arg == "all":
        return life_like_rules()
    try:
        with open(arg, "r", encoding="ascii", errors="replace") as f:
            lines = f.read().split("\n")
    except OSError:
        raise SystemExit(f"gol: error: --batch-rules: cannot read '{arg}'")
    rules = []
    for n, line in enumerate(lines, 1):
        text = line.partition("#")[0].strip(" \t\r")
        if not text:
            continue
        try:
            rules.append(parse_rule(text))
        except RuntimeError as e:
            raise SystemExit(f"gol: error: --batch-rules {arg}: line {n}: {e}")
    if not rules:
        raise SystemExit(f"gol: error: --batch-rules {arg}: the file names no rule")
    return rules


def run_batch(a) -> int:
    """--batch: one call of simulate_batch, the CSVs, the metrics and the summary."""
    from .models.batch import simulate_batch  # noqa: PLC0415

    if a.batch_rules is not None and a.rule is not None:
        raise SystemExit("--batch-rules with --rule: the rules come from the list")
    if a.input_file != "none" or a.random is None:
        raise SystemExit("--batch runs random soups: give the input 'none' and --random SEED[:DENSITY]")
    single = {"--output": a.output_given, "--census": a.census is not None,
              "--fingerprint": a.fingerprint is not None, "--cycle": a.cycle is not None,
              "--density": a.density is not None, "--density-block": a.density_block is not None,
              "--density-every": a.density_every != 0, "--window": bool(a.window), "--place": bool(a.place),
              "--checkpoint-every": a.checkpoint_every != 0, "--checkpoint-dir": a.checkpoint_dir is not None,
              "--resume": a.resume is not None, "--decomp": a.decomp != "auto", "--show": a.show}
    for opt, given in single.items():
        if given:
            raise SystemExit(f"--batch with {opt}: a batch has no single grid to write, count, view or checkpoint "
                             "(its results go to --batch-csv and --metrics-json)")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("--batch runs on one device: not under torchrun with more than one process")
    if a.batch is not None and a.batch < 1:
        raise SystemExit("--batch: the number of universes must be at least 1")
    if a.soups is not None and a.soups < 1:
        raise SystemExit("--soups: the number of soups per rule must be at least 1")
    if a.engine == "ref":
        raise SystemExit("--batch runs on --engine hip or cpu, not ref")
    s, _, d = a.random.partition(":")
    seed, density = int(s), float(d) if d else 0.5
    rules, K = None, a.soups or 1
    if a.batch_rules is not None:
        rules = load_batch_rules(a.batch_rules)
        if a.batch is not None and a.batch != len(rules) * K:
            raise SystemExit(f"gol: error: --batch {a.batch}: {len(rules)} rules x {K} soups make {len(rules) * K} "
                             "universes")
        a.batch = len(rules) * K
    try:
        r = simulate_batch(batch=a.batch, rules=rules, soups=a.soups, shape=(a.width, a.height), random=(seed, density), max_gens=a.gens,
                           max_period=64 if a.max_period is None else a.max_period,
                           rule=a.rule if a.rule is not None else DEFAULT_RULE,
                           boundary=a.boundary or DEFAULT_BOUNDARY, engine=a.engine, threads=a.threads,
                           tune=parse_tune_args(a.tune), clusters=a.batch_census is not None)
    except RuntimeError as e:
        raise SystemExit(f"gol: error: {e}")
    names = r.stop_names()
    if a.batch_csv is not None:
        with open(a.batch_csv, "w") as f:
            f.write(f"universe,seed,{'rule,' if rules else ''}generations,stop,period,population\n")
            for b in range(a.batch):
                soup = b % K if a.soups is not None else b
                f.write(f"{b},{(seed + soup) % 2**64},{rules[b // K] + ',' if rules else ''}{int(r.generations[b])},"
                        f"{names[b]},{int(r.period[b])},{int(r.population[b])}\n")
    if a.rules_csv is not None:
        per = r.per_rule()
        with open(a.rules_csv, "w") as f:
            f.write("rule,soups,limit,cycle,extinction,mean_generations,max_generations,max_period,mean_population\n")
            for i, rule in enumerate(rules):
                c = per["counts"][i]
                f.write(f"{rule},{K},{int(c[0])},{int(c[1])},{int(c[2])},{per['mean_generations'][i]:.6f},"
                        f"{int(per['max_generations'][i])},{int(per['max_period'][i])},"
                        f"{per['mean_population'][i]:.6f}\n")
    counts = r.counts()
    longest = int(r.generations.max())
    census = {}
    if a.batch_census is not None:
        kinds = r.cluster_table()
        with open(a.batch_census, "w") as f:
            f.write("signature,name,cells,height,width,spanning,count\n")
            for sig, name, cells, height, width, spanning, count in kinds:
                f.write(f"{sig:016x},{name},{cells},{height},{width},{spanning},{count}\n")
        census = {"batch_clusters": len(r.cluster_records), "batch_cluster_kinds": len(kinds),
                  "batch_clusters_ms": r.clusters_ms}
    write_json(a.metrics_json, {"engine": "cpu" if r.variant.startswith("batch cpu") else "hip", "rule": parse_rule(a.rule) if a.rule is not None else DEFAULT_RULE,
                                "boundary": a.boundary or DEFAULT_BOUNDARY, "width": a.width, "height": a.height,
                                "batch": a.batch, "seed": seed, "density": density, "max_gens": a.gens,
                                "max_period": 64 if a.max_period is None else a.max_period,
                                "batch_kernel_ms": r.kernel_ms, "batch_variant": r.variant, **counts,
                                "max_generations": longest,
                                **({"batch_rules": len(rules), "batch_soups": K} if rules else {}), **census})
    sys.stdout.write(batch_summary(a.batch, counts, longest))
    if rules:
        sys.stdout.write(f"Rules: {len(rules)} rules x {K} soups\n")
    if a.batch_census is not None:
        most = f"; most common {kinds[0][1]} x{kinds[0][6]}" if kinds else ""
        sys.stdout.write(f"Clusters: {len(r.cluster_records)} in {a.batch} universes, {len(kinds)} kinds{most}\n")
    sys.stdout.flush()
    return 0


def main(argv=None) -> int:
    a = parse_args(argv)
    if "help" in a.tune:
        print_tuning_keys()
        return 0
    if a.batch_rules is None and (a.soups is not None or a.rules_csv is not None):
        raise SystemExit("--soups and --rules-csv need --batch-rules FILE|all")
    if a.batch is not None or a.batch_rules is not None:
        return run_batch(a)
    if a.max_period is not None or a.batch_csv is not None:
        raise SystemExit("--max-period and --batch-csv need --batch N")
    if a.batch_census is not None:
        raise SystemExit("--batch-census needs --batch N or --batch-rules FILE|all")
    if a.input_file is None and a.random is None and a.resume is None:
        print("Finished")
        return 0
    try:
        rule = parse_rule(a.rule) if a.rule is not None else DEFAULT_RULE
    except RuntimeError as e:
        raise SystemExit(f"--rule: {e}")
    boundary = a.boundary or DEFAULT_BOUNDARY
    seed, density = 1, 0.5
    if a.random is not None:
        s, _, d = a.random.partition(":")
        seed, density = int(s), float(d) if d else 0.5

    if a.cycle is not None and a.cycle < 1:
        raise SystemExit("--cycle: the largest period must be at least 1")
    if a.cycle is not None and (a.engine == "ref" or a.checkpoint_every > 0):
        raise SystemExit("--cycle runs Simulation.find_cycle: not with --engine ref (the plain serial loop) or "
                         "--checkpoint-every")
    if a.density_every > 0 and (a.engine == "ref" or a.cycle is not None):
        raise SystemExit("--density-every runs the engine in chunks: not with --engine ref (the plain serial loop) or "
                         "--cycle")
    stamps, block, windows = parse_view_args(a, rule)
    # Input 'none' with patterns to place: the grid starts empty.
    empty_start = a.input_file == "none" and a.random is None and a.resume is None and bool(stamps)
    if a.engine == "ref":
        import numpy as np  # noqa: PLC0415

        from .ops.life_ops import random_grid  # noqa: PLC0415
        from .utils.io import read_grid, write_grid  # noqa: PLC0415

        t0 = time.perf_counter()
        if a.random:
            grid = random_grid(a.width, a.height, seed, density)
        elif empty_start:
            grid = np.zeros((a.height, a.width), dtype=np.uint8)
        else:
            grid = read_grid(a.input_file, a.width, a.height)
        if stamps:  # stamped on the host grid before the serial loop
            grid = np.array(grid, dtype=np.uint8)
            grid[grid == ord("1")] = 1
            grid[grid == ord("0")] = 0
            for cells, x, y in stamps:
                grid[y:y + cells.shape[0], x:x + cells.shape[1]] |= cells
        read_ms = (time.perf_counter() - t0) * 1e3
        out, gens, ms, *pop = reference_run(np.asarray(grid), a.gens, not a.no_similarity, a.sim_freq,
                                            max(1, a.threads), rule=rule, boundary=boundary,
                                            census=a.census is not None, fingerprint=a.fingerprint is not None)
        if a.census is not None:
            write_census(a.census, 0, pop[0])
        if a.fingerprint is not None:
            write_fingerprint(a.fingerprint, 0, pop[-1])
        t1 = time.perf_counter()
        if a.output != "none":
            write_grid(a.output, out)
        write_ms = (time.perf_counter() - t1) * 1e3
        if block is not None or windows:
            final = (np.asarray(out) == 1) | (np.asarray(out) == ord("1"))
            final = final.astype(np.uint8)
        if block is not None:
            by, bx = block
            nby, nbx = -(-a.height // by), -(-a.width // bx)
            pad = np.zeros((nby * by, nbx * bx), dtype=np.int64)
            pad[:a.height, :a.width] = final
            counts = pad.reshape(nby, by, nbx, bx).sum((1, 3))
            write_pgm(density_path(a.density, gens), density_image(counts, by, bx, a.height, a.width))
        for x, y, w, h, path in windows:
            write_window_file(path, final[y:y + h, x:x + w], rule)
        sys.stdout.write(stdout_lines(a.style, gens, ms, read_ms, write_ms))
        if a.show:
            from .utils.io import show_text  # noqa: PLC0415

            sys.stdout.write(show_text(out))
            sys.stdout.flush()
        return 0

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", str(rank)))
    tune = parse_tune_args(a.tune)
    backend = make_backend(a.engine, local, a.threads, tune)
    if world > 1:
        from .parallel.dist import init_process_group, make_transport  # noqa: PLC0415

        init_process_group("nccl" if backend.is_device() else "gloo",
                           device=int(backend.device()) if backend.is_device() else None)
        transport = make_transport(a.comm, backend, local, tune=tune)
    else:
        from ._native import native  # noqa: PLC0415

        transport = native().self_transport()

    cfg = LifeConfig(a.width, a.height, gen_limit=a.gens, check_similarity=not a.no_similarity,
                     sim_freq=a.sim_freq, layout=a.layout, decomp=a.decomp, tmax=a.tmax,
                     epoch=a.epoch, poll_gens=a.poll, overlap=a.overlap, graphs=a.graphs,
                     u8_compute=a.u8_compute, tune=tune, rule=rule, boundary=boundary,
                     census=a.census is not None,
                     fingerprint=a.fingerprint is not None or a.cycle is not None)
    src = a.input_file
    if a.resume:
        from .utils.checkpoint import load_checkpoint  # noqa: PLC0415

        cfg, grid_path = load_checkpoint(a.resume, layout=a.layout, decomp=a.decomp, tmax=a.tmax,
                                         epoch=a.epoch, poll_gens=a.poll, gen_limit=a.gens)
        if a.rule is not None and rule != parse_rule(cfg.rule):
            raise SystemExit(f"--resume: checkpoint was taken with --rule {cfg.rule}, not {rule}")
        if a.boundary is not None and a.boundary != cfg.boundary:
            raise SystemExit(f"--resume: checkpoint was taken with --boundary {cfg.boundary}, not {a.boundary}")
        if a.sim_freq_given and not a.no_similarity and a.sim_freq != cfg.sim_freq:
            raise SystemExit(f"--resume: checkpoint was taken with --sim-freq {cfg.sim_freq}; resuming with "
                             f"--sim-freq {a.sim_freq} would shift the similarity checks")
        # A census is per run: --census counts the resumed run whether or not the first one did.
        cfg.census = cfg.census or a.census is not None
        cfg.fingerprint = cfg.fingerprint or a.fingerprint is not None or a.cycle is not None
        src = str(grid_path)
    sim = Simulation(cfg, transport=transport, backend=backend)
    # Opt-in only: the event pairs would sit inside the loop that loop_ms and
    # the reference-style timing line report.
    sim.phase_timing = bool(a.phase_timing)
    g0 = sim.generation
    t0 = time.perf_counter()
    if a.random is not None and not a.resume:
        sim.init_random(seed, density)
    elif empty_start:
        sim.init_random(0, 0.0)  # no cell alive
    else:
        sim.load_text(src)
    for cells, x, y in stamps:
        sim.place(cells, x, y, mode="or")
    transport.barrier()
    read_ms = (time.perf_counter() - t0) * 1e3

    density_ms, density_frames = 0.0, 0

    def write_density(gen: int) -> None:
        """One density image of the current grid (every rank takes part; rank 0 writes it)."""
        nonlocal density_ms, density_frames
        t = time.perf_counter()
        counts = sim.density(block)
        density_ms = (time.perf_counter() - t) * 1e3
        density_frames += 1
        if rank == 0:
            write_pgm(density_path(a.density, gen), density_image(counts, block[0], block[1], a.height, a.width))

    if a.checkpoint_every > 0 or a.density_every > 0:
        from .utils.checkpoint import run_with_checkpoints  # noqa: PLC0415

        rep = run_with_checkpoints(sim, a.checkpoint_every, a.checkpoint_dir, rank == 0, transport.barrier,
                                   frame_every=a.density_every, on_frame=write_density)
    elif a.cycle is not None:
        from .models.life import RunReport  # noqa: PLC0415

        cyc = sim.find_cycle(a.gens, a.cycle)
        rep = RunReport(generations=cyc.generation, executed=cyc.generation - g0, stop_reason=cyc.stop_reason,
                        loop_ms=cyc.loop_ms, extinct=cyc.stop_reason == "extinction", cells=a.width * a.height,
                        fingerprint=cyc.fingerprint)
    else:
        rep = sim.run()

    if block is not None:
        write_density(rep.generations)
    for x, y, w, h, path in windows:
        cells = sim.window(x, y, w, h)
        if rank == 0:
            write_window_file(path, cells, rule)
    write_ms = 0.0
    tiles = None
    if a.show:  # every rank's tile, gathered on rank 0 (the viewer prints the whole grid)
        from .parallel.dist import gather_grid  # noqa: PLC0415

        tiles = gather_grid(sim) if world > 1 else sim.tile()
    if a.output != "none":
        t1 = time.perf_counter()
        if rank == 0:
            from .utils.io import create_text_file  # noqa: PLC0415

            create_text_file(a.output, a.width, a.height)
        transport.barrier()
        sim.write_text(a.output, create=False)
        transport.barrier()
        write_ms = (time.perf_counter() - t1) * 1e3
    if rank == 0:
        sys.stdout.write(stdout_lines(a.style, rep.generations, rep.loop_ms, read_ms, write_ms, world))
        sys.stdout.flush()
        rec = rep.as_dict()
        if cfg.census:
            rec["population"] = [int(v) for v in rep.population]
        if a.census is not None:
            write_census(a.census, g0, rep.population)
        if cfg.fingerprint:
            rec["fingerprints"] = [f"{int(v):016x}" for v in rep.fingerprint]
        if a.fingerprint is not None:
            write_fingerprint(a.fingerprint, g0, rep.fingerprint)
        if a.cycle is not None:
            rec["cycle"] = cyc.as_dict() | {"max_period": a.cycle}
            sys.stdout.write(cycle_line(cyc, a.gens))
            sys.stdout.flush()
        if block is not None:
            rec.update({"density_block": f"{block[0]}x{block[1]}", "density_ms": density_ms,
                        "density_frames": density_frames})
        rec.update(sim.describe())
        rec.update({"read_ms": read_ms, "write_ms": write_ms, "width": a.width, "height": a.height})
        write_json(a.metrics_json, rec)
        if tiles is not None:
            from .utils.io import show_text  # noqa: PLC0415

            sys.stdout.write(show_text(tiles))
            sys.stdout.flush()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
