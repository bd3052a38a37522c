"""Tile buffers past 2 GiB and 4 GiB on the HIP engine: every kernel family on
a 65536-cell-wide tile whose buffer passes 2^32 bytes by 64 MiB (bits: 533,504
rows, 3.5e10 cells, more than 2^32 live cells in a 0.4 soup; bytes: 67,584
rows, 4.4e9 cells), so a byte offset, cell index or count computed or
truncated in 32 bits is a wrong result here.

The oracle is never a whole-grid tensor (tests/far_oracle.py): islands on an
empty grid, whose windows, count, density map, census and fingerprint series
are the sum of the islands evolved alone in NumPy - the density map watches the
whole buffer for stray writes - then a dense soup checked on windows against
the RNG's definition and their NumPy evolution, with the whole-grid counts
against each other and the RNG's density.  tests/test_far.py shows on the CPU
engine, on a grid a host can hold, that these expectations are a whole-grid
oracle's.

The buffer size is fixed - nothing smaller reaches these offsets; cost is cut
with the generation count (n = 3 T + 1) and the window sizes.  One engine lives
at a time.  On an MI355X the 21 tests take 0.2 to 1.2 s each (the longest: the
deep byte pass, n = 97), 11 to 13 s together.

What the kernels these tests reach keep in 32 bits although it grows with the
tile, its bound and what enforces it (read before the first run; none can
overflow at the two geometries here or at BASELINE.md's largest per-GPU tile,
1,048,576 x 131,072 bytes, so no kernel changed).  Every row address is
base + int64 row * int64 pitch; what is 32-bit lies inside a row or counts
rows, tiles or cells of a bounded piece:

* words and byte offsets in a row (LifeBlockParams::Wp, own_w0/1, wrap_w,
  LaneCols::off, Writer::col * word bytes; Sc1IO's off * 4), the per-row
  buffer resource (num_records = int(pitch)) and the kDrop = 0x40000000
  offset of lanes that store nothing: < pitch < 2^30 and Wp < 2^30, required
  by launch_life_block.
* a folded strip's Writer::roff / nrec and reader offsets, which span the rows
  of several groups in one descriptor: launch_T folds only where
  (out_rows + 2) * pitch < 2^30 (never on a far tile).
* rows per segment, group and wave (seg_rows, seg_rem, grp_q, kend, kmain) and
  group indices (bnd_g, link_prev_nseg): at most the tile's rows, < 2^31 for
  any tile that can be allocated (a pitch is at least 256 bytes).
* waves, tiles and workgroups (ncolw * nseg as int, blockIdx): strips * rows /
  2T, 5.7e5 here and 2.2e6 at BASELINE's tile; launch sizes are computed in 64
  bits.  Not checked; 2^31 would take a buffer of terabytes.
* the plane's grid_row_lo / grid_row_hi and EdgeState::rel: R() < 2^30,
  required.
* census counts per lane and wave (uint32; the slots are 64-bit): blocks of
  fewer than 2^20 rows, required - a wave stays below 2^31.  A tile of
  1,048,576 rows or more is refused, not miscounted.
* the fingerprint's fp_row0, fp_word0, y0, gword: global rows and words below
  2^31, required; the stand-alone kernel's row key is defined on uint32(row).
* the skipping kernel's 20-bit packed counter fields, item numbers and
  n_items * units per item (at most 2^20 * 124): fewer than 2^20 tiles,
  checked where the launch is planned and where its maps are prepared; a
  larger plan runs the dense kernels.  191,488 tiles here.
* the density kernel's LDS bins (uint32): a piece is at most 128 rows by 8192
  cells, 2^20; they are flushed with 64-bit atomics; at most 2^24 blocks and
  2^26 window cells, both checked.
* the LDS-tiled byte kernels: the packed kernel's grid nx * ny < 2^31,
  checked; the single-step and byte multi-generation kernels put rows / tile
  rows in gridDim.y, checked against 2^31 where the device's limit for that
  dimension is 16 bits: a launch error (no wrong result) from about two
  million rows on; 2,112 tile rows here and 4,096 at BASELINE's tile.
* tile_ops.hip, view_ops.hip, the staging and copy paths and the engine's view
  preparation hold every product of rows, pitch and cells in int64 / size_t."""
import gc

import pytest

import far_oracle as fo
from gol_amd import LifeConfig, Simulation

pytestmark = pytest.mark.gpu

# Free device memory the module needs: the heaviest engine's measured peak - free before it minus the least
# free while it lived; 12,684 MiB, the byte-kernel engine with find_cycle's snapshot, a third buffer (the bit
# layout's: 12,520; the byte grid on bit words: 9,570; every other engine 8,344 to 8,876) - plus 25 %.
PEAK_MEASURED = 12684 * 2**20
NEED_FREE = PEAK_MEASURED * 5 // 4  # 15,855 MiB


def _free() -> int:
    import torch  # noqa: PLC0415

    return torch.cuda.mem_get_info()[0]


@pytest.fixture(scope="module", autouse=True)
def room(gpu):
    gc.collect()
    free = _free()
    if free < NEED_FREE:
        pytest.skip(f"far tiles need {NEED_FREE >> 20} MiB of free device memory, {free >> 20} MiB are free")


def far_case(native, layout, phases=2, n=0, **cfg):
    """One engine through phase 1 and (phases == 2) phase 2; what it reported, for the caller's assertions."""
    H = fo.far_height(native, layout)
    gc.collect()
    free0 = _free()
    sim = Simulation(LifeConfig(fo.FAR_W, H, gen_limit=10**9, layout=layout, **cfg), engine="hip")
    try:
        d = sim.describe()
        far = fo.far_rows(sim.native_engine.geom, fo.FAR_W, H)  # asserts bytes() > 2^32 + 2^26
        n = n or 3 * d["tmax"] + 1
        flags = dict(census=bool(cfg.get("census")), fingerprint=bool(cfg.get("fingerprint")))
        rule, boundary = cfg.get("rule", "B3/S23"), cfg.get("boundary", "torus")
        low = _free()
        sp = fo.run_islands(sim, far, n, rule, boundary, **flags)
        assert any(a.y > far.y32 for a in sp.isles)  # a far island lies beyond y32
        out = dict(describe=d, far=far, n=n, islands=sim.describe(), report=sim.last_report)
        low = min(low, _free())
        if phases == 2:
            out["counts"] = fo.run_soup(sim, far, n, rule, boundary, **flags)
            out["soup"], out["report"] = sim.describe(), sim.last_report
            low = min(low, _free())
        out["peak"] = free0 - low
        kind = {k: d[k] for k in ("kernel", "tmax", "row_ring", "drifting", "u8_compute", "halo_rows", "pitch")}
        print(f"\nfar tile: {layout} {cfg} n={n} peak {out['peak'] / 2**20:.0f} MiB {kind} "
              f"launch_paths={out.get('soup', out['islands'])['launch_paths']} counts={out.get('counts')}")
        return out
    finally:
        sim = None
        gc.collect()


def more_than_2_32(out):
    c0, c = out["counts"]
    assert c0 > c > 2**32, (c0, c)  # the three counts that agreed (far_oracle.run_soup) do not fit 32 bits


# ---- the bit layout: 65536 x 533,504 -------------------------------------------------------------------

def test_default_policy(gpu):
    out = far_case(gpu, "bits")
    d, paths = out["describe"], out["soup"]["launch_paths"]
    told = dict(row_ring=d["row_ring"], drifting=d["drifting"], linked=paths["linked"], tmax=d["tmax"], kernel=d["kernel"])
    assert d["layout"] == "bits" and sum(paths.values()) > 0, told
    c0, c = out["counts"]
    assert c0 > c > 2**32, (c0, c, told)


@pytest.mark.parametrize("chain", ["0", "1"])
def test_dpp_window_grouped_without_ring(gpu, chain):
    out = far_case(gpu, "bits", tmax=16, tune={"xlane": "0", "row_ring": "0", "group": "8", "chain": chain})
    d, paths = out["describe"], out["soup"]["launch_paths"]
    assert d["tmax"] == 16 and not d["row_ring"] and not d["drifting"] and d["halo_rows"] >= 16, d
    assert paths["chained" if chain == "1" else "grouped"] > 0 and paths["linked"] == 0, paths
    if chain == "0":
        assert paths["chained"] == 0, paths
    more_than_2_32(out)


def test_adder_window_graph_replay(gpu):
    out = far_case(gpu, "bits", tmax=12, graphs="on", tune={"xlane": "3"})
    d = out["describe"]
    assert d["tmax"] == 12 and d["drifting"] and d["graphs"], d  # the rotate-out kernel ran before every view
    assert out["report"].graph_launches > 0
    more_than_2_32(out)


@pytest.mark.parametrize("cols", ["0", "1"])
def test_skipping_kernel(gpu, cols):
    """The tile list and (cols) the column records: phase 1, whose grid is almost all quiet tiles."""
    tune = {"quiet_skip": "1", "group": "4", "quiet_rows": "96", "quiet_list": "1", "quiet_cols": cols}
    out = far_case(gpu, "bits", phases=1, n=5 * 12 + 1, tune=tune)
    d = out["islands"]
    assert d["tmax"] == 12 and d["quiet_mode"] == "on" and d["quiet_list"] is True, d["quiet_mode"]
    assert d["quiet_blocks"]["skip"] > 0 and d["launch_paths"]["skipping"] > 0, d["quiet_blocks"]
    assert 0 < d["quiet_waves_skipped"] < d["quiet_waves_launched"]
    assert d["quiet_cols"] is (cols == "1")
    if cols == "1":
        assert 0 < d["quiet_cols_computed"] < d["quiet_cols_of_tiles"]


def test_bounded_plane(gpu):
    out = far_case(gpu, "bits", boundary="dead")
    assert out["describe"]["boundary"] == "dead" and out["describe"]["halo_words"] > 0
    more_than_2_32(out)


def test_census(gpu):
    out = far_case(gpu, "bits", census=True)
    assert out["describe"]["census"] and len(out["report"].population) == out["n"]
    more_than_2_32(out)  # the census's last element among them


def test_fingerprint(gpu):
    out = far_case(gpu, "bits", fingerprint=True)
    assert out["describe"]["fingerprint"] and len(out["report"].fingerprint) == out["n"]
    more_than_2_32(out)


@pytest.mark.parametrize("layout", ["bits", "u8"])
def test_cycle_confirmation_beyond_y32(gpu, layout):
    """copy_rows_k and equal_k (find_cycle's snapshot and exact comparison) where only far rows are alive;
    the snapshot is a third buffer of the tile's size."""
    H = fo.far_height(gpu, layout)
    gc.collect()
    free0 = _free()
    sim = Simulation(LifeConfig(fo.FAR_W, H, gen_limit=10**9, layout=layout, fingerprint=True, check_similarity=False,
                                tune={"cycle_match_bits": "0", "u8_via_bits": "0"}), engine="hip")
    try:
        far = fo.far_rows(sim.native_engine.geom, fo.FAR_W, H)
        fo.run_cycle_confirmation(sim, far)
        print(f"\nfar tile: {layout} find_cycle peak {(free0 - _free()) / 2**20:.0f} MiB")
    finally:
        sim = None
        gc.collect()


@pytest.mark.parametrize("xlane,tmax", [(3, 12), (0, 16)])
def test_compiled_rule(gpu, xlane, tmax):
    out = far_case(gpu, "bits", rule="highlife", tmax=tmax, tune={"xlane": str(xlane)})
    d = out["describe"]
    assert d["rule"] == "B36/S23" and d["tmax"] == tmax and d["drifting"] is (xlane == 3), d
    more_than_2_32(out)


# ---- the byte layout: 65536 x 67,584 ---------------------------------------------------------------------

def test_byte_grid_on_bit_words(gpu):
    """The default: the far offsets are in the byte image and the pack / unpack kernels."""
    out = far_case(gpu, "u8")
    assert out["describe"]["u8_compute"] == "bits"
    assert out["counts"][0] > 0.39 * 2**32


@pytest.mark.parametrize("tmax", [16, 32])
def test_byte_kernels(gpu, tmax):
    out = far_case(gpu, "u8", tmax=tmax, tune={"u8_via_bits": "0"})
    d = out["describe"]
    assert d["u8_compute"] == "bytes" and d["tmax"] == tmax, d
    assert out["soup"]["launch_paths"]["lds_tiled"] == 0


@pytest.mark.parametrize("lds_t", [1, 8])
def test_lds_tiled_byte_kernels(gpu, lds_t):
    """The single-step kernel, and the multi-generation kernel on bit words packed in LDS."""
    out = far_case(gpu, "u8", tune={"u8_via_bits": "0", "u8_kernel": "lds", "lds_t": str(lds_t)})
    d = out["describe"]
    assert d["u8_compute"] == "bytes" and d["tmax"] == lds_t and "lds" in d["backend"], d
    if lds_t == 8:
        assert "packed" in d["backend"], d["backend"]
    paths = out["soup"]["launch_paths"]
    assert paths["lds_tiled"] > 0 and paths["lds_tiled"] == sum(paths.values()), paths


@pytest.mark.parametrize("kw", [dict(boundary="dead"), dict(census=True), dict(fingerprint=True)],
                         ids=["plane", "census", "fingerprint"])
def test_byte_kernel_plane_census_fingerprint(gpu, kw):
    out = far_case(gpu, "u8", phases=1, tune={"u8_via_bits": "0"}, **kw)
    d = out["describe"]
    assert d["u8_compute"] == "bytes" and d["tmax"] <= 16, d
    for k, v in kw.items():
        assert d[k] == v
