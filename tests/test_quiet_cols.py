"""Column records of the skipping kernel (csrc/include/gol/quiet.hpp, tuning
quiet_cols): the pure window function and the host model of the column
kernel, against a numpy torus.  A scaled-down plan - 3 strips of 62, 62 and 4
word columns, 4 groups of 40 rows, T = 12 - is stepped block by block; the
records every column would publish are derived from the successive states,
and the model, which recomputes only the windows, must reproduce the words and
records of a full recomputation while every column it leaves alone must
already hold in the destination (the state two blocks back) what the block
would write.

The reference has no counterpart (every generation rewrites every cell,
src/game_cuda.cu:128-148)."""
import numpy as np
import pytest

T = 12
OWN = (62, 62, 4)            # owned word columns per strip
NCOLW, NSEG, ROWS = 3, 4, 40
WORDS = sum(OWN)
W, H = WORDS * 32, NSEG * ROWS
TILES = NCOLW * NSEG
G = 4

BLOCK = ["11", "11"]
BLINKER = ["111"]
GLIDER_SE = [".1.", "..1", "111"]
GLIDER_NW = ["111", "1..", ".1."]
PENTADECATHLON = ["..1....1..", "11.1111.11", "..1....1.."]
PULSAR = ["..111...111..", ".............", "1....1.1....1", "1....1.1....1", "1....1.1....1", "..111...111..",
          ".............", "..111...111..", "1....1.1....1", "1....1.1....1", "1....1.1....1", ".............",
          "..111...111.."]


def put(g, y, x, pat):
    for dy, row in enumerate(pat):
        for dx, c in enumerate(row):
            if c == "1":
                g[(y + dy) % H, (x + dx) % W] = 1


def step(g):
    n = sum(np.roll(np.roll(g, dy, 0), dx, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)) - g
    return ((n == 3) | ((g == 1) & (n == 2))).astype(np.uint8)


def block_states(g):
    s = [g]
    for _ in range(T):
        s.append(step(s[-1]))
    return s


def word0(kcol):
    return sum(OWN[:kcol])


def fresh_records(native, states):
    """tiles x 64 records: what every column publishes if it is computed in this block."""
    rec = np.zeros((TILES, native.QUIET_COL_LANES), np.uint32)
    # Per level, the cells that change, ORed over the 32 cells of each word column.
    chg = [(states[L + 1] ^ states[L]).reshape(H, WORDS, 32).any(2) for L in range(T)]
    dirty = (states[T] ^ states[0]).reshape(H, WORDS, 32).any(2)
    for kcol in range(NCOLW):
        cols = slice(word0(kcol), word0(kcol) + OWN[kcol])
        for grp in range(NSEG):
            t, g0, g1 = kcol * NSEG + grp, grp * ROWS, (grp + 1) * ROWS
            r = np.zeros(OWN[kcol], np.uint32)
            for L in range(T):
                rows = np.arange(g0 - (T - 1 - L), g1 + (T - 1 - L)) % H
                r |= chg[L][rows][:, cols].any(0).astype(np.uint32) << np.uint32(L)
            r |= dirty[g0:g1, cols].any(0).astype(np.uint32) * np.uint32(native.QUIET_DIRTY)
            r |= dirty[g0:g0 + T, cols].any(0).astype(np.uint32) * np.uint32(native.QUIET_TOP)
            r |= dirty[g1 - T:g1, cols].any(0).astype(np.uint32) * np.uint32(native.QUIET_BOT)
            rec[t, 1:1 + OWN[kcol]] = r
    return rec


def full_words(native, rec):
    out = []
    for t in range(TILES):
        own = OWN[t // NSEG]
        w = int(np.bitwise_or.reduce(rec[t, 1:1 + own]))
        if rec[t, 1] & native.QUIET_DIRTY:
            w |= native.QUIET_LEFT
        if rec[t, own] & native.QUIET_DIRTY:
            w |= native.QUIET_RIGHT
        out.append(w)
    return out


def ash(seed=5, still_only=False):
    g = np.zeros((H, W), np.uint8)
    rng = np.random.default_rng(seed)
    for y in range(4, H - 8, 16):
        for x in range(4, W - 8, 16):
            r = rng.integers(0, 6)
            if r == 0:
                put(g, y, x, BLOCK)
            elif r == 1 and not still_only:
                put(g, y, x, BLINKER)
    return g


def clear(g, y0, y1, x0, x1):
    g[np.ix_(np.arange(y0, y1) % H, np.arange(x0, x1) % W)] = 0


def run_model(native, g, blocks, cols_from=2):
    """Steps `blocks` blocks; checks the model against the full recomputation after each.  Returns per block
    the columns computed per tile."""
    m = native.QuietColsModel(NCOLW, NSEG, T, OWN[-1], G)
    hist, before = [], None  # before: the state two blocks back (what the destination holds)
    for b in range(blocks):
        states = block_states(g)
        rec = fresh_records(native, states)
        cols = b >= cols_from
        done = m.block(rec.reshape(-1).tolist(), b > 0, cols)
        hist.append(done)
        words = [w & ~native.QUIET_COLS for w in m.words()]
        assert words == full_words(native, rec), b
        got = np.array(m.records(), np.uint32).reshape(TILES, -1)
        for t in range(TILES):
            own = OWN[t // NSEG]
            if m.valid(t):
                assert np.array_equal(got[t, 1:1 + own], rec[t, 1:1 + own]), (b, t)
            if b > 0 and before is not None:
                # Columns the block leaves alone: the destination already holds them.
                kcol, grp = divmod(t, NSEG)
                for j in range(1, own + 1):
                    if not (done[t] >> j) & 1:
                        c0 = (word0(kcol) + j - 1) * 32
                        rows = slice(grp * ROWS, (grp + 1) * ROWS)
                        assert np.array_equal(states[T][rows, c0:c0 + 32], before[rows, c0:c0 + 32]), (b, t, j)
        before, g = states[0], states[T]
    return m, hist


def test_constants_and_group_helpers(native):
    assert native.QUIET_COLS == 1 << 21 and native.QUIET_COL_LANES == 64
    assert not native.quiet_marks_neighbours(5, 5 | native.QUIET_COLS)  # the bit says nothing about the cells
    assert native.quiet_marks_neighbours(5, 4)
    assert native.quiet_window_spread(1 << 10, 62) == 0b111 << 9
    assert native.quiet_window_spread(1 << 0, 62) == 1 << 1            # the strip to the left: the first column
    assert native.quiet_window_spread(1 << 63, 62) == 1 << 62          # the strip to the right: the last one
    assert native.quiet_window_spread(1 << 5, 4) == 1 << 4             # a narrow strip of 4 columns
    assert native.quiet_window_groups(0b111 << 9, 62, 4) == 1 << 2     # columns 9..11: group 2 (columns 9..12)
    assert native.quiet_window_groups(0b111 << 11, 62, 4) == 0b11 << 2  # columns 11..13: groups 2 and 3
    assert native.quiet_window_groups(0, 62, 4) == 1                    # never no group
    assert native.quiet_group_columns(0b1, 62, 4) == 0b11110
    assert native.quiet_group_columns(1 << 15, 62, 4) == 0b11 << 61      # the last group is cut at the strip's end
    assert native.quiet_group_columns(0b1, 4, 8) == 0b11110


def nine(native, **kw):
    """Nine tiles with valid all-zero records, then rec[i][j] |= bits for kw t<i> = [(j, bits), ...]."""
    rec = [[0] * 64 for _ in range(9)]
    words = [native.QUIET_COLS] * 9
    for k, v in kw.items():
        for j, bits in v:
            rec[int(k[1:])][j] |= bits
            words[int(k[1:])] |= bits
    return rec, words


def test_window_of_a_quiet_neighbourhood_is_empty(native):
    rec, words = nine(native)
    assert native.quiet_window(rec, words, 62, 62, 62) == 0
    # Level flags alone (p2 / p3 ash: flags, never dirty) put nothing in the window.
    rec, words = nine(native, t4=[(7, 0xFFF)], t1=[(8, 0x3)], t3=[(62, 0xFFF)])
    assert native.quiet_window(rec, words, 62, 62, 62) == 0


def test_window_rule_in_the_tile_above_below_beside_and_in_corners(native):
    D, TOP, BOT = native.QUIET_DIRTY, native.QUIET_TOP, native.QUIET_BOT
    w = lambda **kw: native.quiet_window(*nine(native, **kw), 62, 62, 4)  # noqa: E731
    assert w(t4=[(20, D)]) == 0b111 << 19
    assert w(t4=[(1, D)]) == 0b11 << 1 and w(t4=[(62, D)]) == 0b11 << 61
    # The tile above counts through its last T rows, the tile below through its first.
    assert w(t1=[(30, D | BOT)]) == 0b111 << 29 and w(t1=[(30, D | TOP)]) == 0
    assert w(t7=[(30, D | TOP)]) == 0b111 << 29 and w(t7=[(30, D | BOT)]) == 0
    # The strips beside: only their facing column (the last one of the left strip, the first of the right).
    assert w(t3=[(62, D)]) == 1 << 1 and w(t3=[(61, D)]) == 0
    assert w(t5=[(1, D)]) == 1 << 62 and w(t5=[(2, D)]) == 0
    # Corners: the facing column's facing T rows.
    assert w(t0=[(62, D | BOT)]) == 1 << 1 and w(t0=[(62, D | TOP)]) == 0 and w(t0=[(61, D | BOT)]) == 0
    assert w(t2=[(1, D | BOT)]) == 1 << 62 and w(t6=[(62, D | TOP)]) == 1 << 1 and w(t8=[(1, D | TOP)]) == 1 << 62
    # A narrow strip to the left: its last owned column is lane column 4.
    rec, words = nine(native, t3=[(4, D)])
    assert native.quiet_window(rec, words, 4, 62, 62) == 1 << 1
    assert native.quiet_window(rec, words, 62, 62, 62) == 0
    # A narrow centre strip.
    rec, words = nine(native, t5=[(1, D)])
    assert native.quiet_window(rec, words, 62, 4, 62) == 1 << 4


def test_unknown_records_give_full_windows_and_conservative_neighbours(native):
    D, TOP, BOT, COLS = native.QUIET_DIRTY, native.QUIET_TOP, native.QUIET_BOT, native.QUIET_COLS
    every = sum(1 << j for j in range(1, 63))
    rec, words = nine(native)
    words[4] &= ~COLS  # the tile's own records are unknown: every column
    assert native.quiet_window(rec, words, 62, 62, 62) == every
    rec[4] = []
    assert native.quiet_window(rec, [COLS] * 9, 62, 62, 62) == every
    # The tile above without records: every column takes its word's bits.
    rec, words = nine(native)
    words[1] = D | BOT
    assert native.quiet_window(rec, words, 62, 62, 62) == every
    words[1] = D | TOP
    assert native.quiet_window(rec, words, 62, 62, 62) == 0
    # A side tile without records: its facing column takes its word's dirty bit.
    rec, words = nine(native)
    words[3] = D
    assert native.quiet_window(rec, words, 62, 62, 62) == 1 << 1
    assert native.quiet_col_standin(D | TOP | 0xFFF | native.QUIET_LEFT) == D | TOP


def test_still_lifes_and_p2_p3_ash_have_empty_windows(native):
    """The records of a field of blocks, blinkers and a pulsar carry level flags and no dirty bit: no window
    holds a column, and the model's launches end."""
    g = ash()
    clear(g, 40, 100, 1980, 2040)
    put(g, 60, 2000, PULSAR)
    rec = fresh_records(native, block_states(g))
    assert rec.any() and not (rec & native.QUIET_DIRTY).any()
    words = [w | native.QUIET_COLS for w in full_words(native, rec)]
    for t in range(TILES):
        kcol, grp = divmod(t, NSEG)
        nb = [native.quiet_neighbour(kcol, grp, i, NCOLW, NSEG) for i in range(9)]
        win = native.quiet_window([rec[n].tolist() for n in nb], [words[n] for n in nb], OWN[(kcol - 1) % NCOLW],
                                  OWN[kcol], OWN[(kcol + 1) % NCOLW])
        assert win == 0, t
    m, hist = run_model(native, g, 4)
    assert all(d == 0 for d in hist[-1]) and m.candidates() == 0


def test_model_reproduces_the_full_recomputation_with_gliders_and_a_soup(native):
    """Gliders cross the boundary of strips 0 and 1, the column wrap (the narrow strip and strip 0), a group
    boundary and the row seam; a soup evolves over the boundary of strips 1 and 2."""
    g = ash(still_only=True)
    s0 = OWN[0] * 32
    starts = [(50, s0 - 6, GLIDER_SE), (70, s0 + 4, GLIDER_NW), (90, W - 6, GLIDER_SE), (110, 3, GLIDER_NW),
              (ROWS - 6, 1000, GLIDER_SE), (2 * ROWS + 4, 1100, GLIDER_NW), (H - 6, 3000, GLIDER_SE), (3, 3100, GLIDER_NW)]
    for y, x, pat in starts:
        clear(g, y - 45, y + 48, x - 45, x + 48)
        put(g, y, x, pat)
    x1 = (OWN[0] + OWN[1]) * 32
    clear(g, 100, 150, x1 - 40, x1 + 40)
    g[118:130, x1 - 6:x1 + 6] = np.random.default_rng(1).random((12, 12)) < 0.4
    m, hist = run_model(native, g, 14)
    # The windows were narrow and not empty.
    some = [bin(d).count("1") for done in hist[3:] for d in done if d]
    assert some and 2 <= min(some) <= 8 and max(some) <= 62  # (a strip's last group: 2; a tile a glider enters has no records yet: 62)
    assert sum(some) < 62 * len(some) // 2
    assert 0 < m.candidates() <= TILES  # eight gliders and a soup on twelve tiles


def test_alternating_launches_leave_unknown_records_and_stay_exact(native):
    """Whole-tile launches between column launches publish no records: the next column launch computes
    every column of the tiles they computed."""
    g = ash(still_only=True)
    clear(g, 40, 80, 940, 1010)
    put(g, 58, 968, PENTADECATHLON)  # p15, inside one word column and clear of the tile's first and last T rows
    m = native.QuietColsModel(NCOLW, NSEG, T, OWN[-1], G)
    widths = []
    for b in range(10):
        states = block_states(g)
        rec = fresh_records(native, states)
        cols = b >= 2 and b % 3 != 0
        done = m.block(rec.reshape(-1).tolist(), b > 0, cols)
        assert [w & ~native.QUIET_COLS for w in m.words()] == full_words(native, rec), b
        widths.append((cols, sorted(bin(d).count("1") for d in done if d)))
        g = states[T]
    for b in range(3, 10):
        cols, ws = widths[b]
        if cols and not widths[b - 1][0]:
            assert ws == [62], (b, ws)            # records unknown: every column
        elif cols:
            assert ws == [4], (b, ws)             # the oscillator's group alone
