"""gol-mi355x: an MI355X-native Game of Life stencil engine.

Same capabilities as v-pap/Game-of-Life-in-parallel-MPI-OpenMP-CUDA (serial,
MPI with three I/O strategies, MPI+OpenMP and CUDA programs evolving B3/S23 on
a torus), rebuilt as one engine: CDNA4 HIP kernels (bit-sliced, temporal
blocking in registers), a C++ runtime (epochs, deep halos, lazy exact
termination, parallel text I/O) and RCCL halos over xGMI with one process
per GPU.

Import as ``gol_amd`` (symlink to this directory).
"""
from ._native import hip_available, native
from .models.life import (CycleReport, LifeConfig, RunReport, Simulation, density_image, grid_fingerprint, make_backend,
                          parse_rule, read_rle, reference_run, simulate, write_pgm, write_rle)
from .models.batch import (BATCH_STOP, CLUSTER_RECORD, BatchResult, cluster_name, cluster_signature, cluster_table,
                           find_clusters, life_like_rules, simulate_batch)
from .ops.life_ops import life_step, life_step_numpy, life_step_torch, random_grid

__version__ = "0.1.0"


def __getattr__(name):
    # RULES: the named Life-like rules, name -> canonical B/S text (read from
    # the native module on first use, so importing the package stays cheap).
    if name == "RULES":
        rules = dict(native().rule_names())
        globals()["RULES"] = rules
        return rules
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = ["CycleReport", "grid_fingerprint", "LifeConfig", "RunReport", "Simulation", "make_backend", "reference_run", "simulate",
           "life_step", "life_step_numpy", "life_step_torch", "random_grid", "native",
           "hip_available", "parse_rule", "RULES", "read_rle", "write_rle", "density_image", "write_pgm", "BATCH_STOP", "BatchResult",
           "simulate_batch", "life_like_rules", "find_clusters", "cluster_signature", "cluster_name", "cluster_table",
           "CLUSTER_RECORD", "__version__"]
