"""Column records of the skipping kernel (csrc/include/gol/quiet.hpp, tuning
quiet_cols): the pure window function and the host model of the column
kernel, against a numpy torus.  A scaled-down plan - 3 strips of 62, 62 and 4
word columns, 4 groups of 40 rows, T = 12 - is stepped block by block; the
records every column would publish are derived from the successive states,
and the model, which recomputes only the windows, must reproduce the words and
records of a full recomputation while every column it leaves alone must
already hold in the destination (the state two blocks back) what the block
would write.

The same on the smallest tile tori (SMALL): one strip, where a tile is its own
left and right neighbour (the window's lane 0 and lane own + 1 read the tile's
own records), one group, where it is its own upper and lower neighbour, two of
either, where both neighbours are the same tile, and last strips of 1, 2 and 3
word columns, narrower than a column group of 2, 4 or 8.

The reference has no counterpart (every generation rewrites every cell,
src/game_cuda.cu:128-148)."""
import dataclasses

import numpy as np
import pytest

T = 12
G = 4


@dataclasses.dataclass(frozen=True)
class Plan:
    """A launch plan: owned word columns per strip, groups of `rows` rows."""
    own: tuple
    nseg: int
    rows: int = 40

    @property
    def ncolw(self):
        return len(self.own)

    @property
    def words(self):
        return sum(self.own)

    @property
    def W(self):
        return self.words * 32

    @property
    def H(self):
        return self.nseg * self.rows

    @property
    def tiles(self):
        return self.ncolw * self.nseg

    def word0(self, kcol):
        return sum(self.own[:kcol])

    def __str__(self):
        return f"{self.ncolw}x{self.nseg}_" + ".".join(map(str, self.own))


BASE = Plan((62, 62, 4), 4)
SMALL = [Plan((32,), 1), Plan((1,), 2), Plan((62, 2), 1), Plan((62, 1), 2), Plan((62, 3), 2)]
small_plans = pytest.mark.parametrize("plan", SMALL, ids=str)
all_plans = pytest.mark.parametrize("plan", [BASE] + SMALL, ids=str)
col_groups = pytest.mark.parametrize("group", [2, 4, 8])

OWN, NCOLW, NSEG, ROWS = BASE.own, BASE.ncolw, BASE.nseg, BASE.rows
WORDS, W, H, TILES = BASE.words, BASE.W, BASE.H, BASE.tiles

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
                g[(y + dy) % g.shape[0], (x + dx) % g.shape[1]] = 1


def step(g):
    n = sum(np.roll(np.roll(g, dy, 0), dx, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)) - g
    return ((n == 3) | ((g == 1) & (n == 2))).astype(np.uint8)


def block_states(g):
    s = [g]
    for _ in range(T):
        s.append(step(s[-1]))
    return s


def fresh_records(native, states, plan=BASE):
    """tiles x 64 records: what every column publishes if it is computed in this block."""
    rec = np.zeros((plan.tiles, native.QUIET_COL_LANES), np.uint32)
    # Per level, the cells that change, ORed over the 32 cells of each word column.
    chg = [(states[L + 1] ^ states[L]).reshape(plan.H, plan.words, 32).any(2) for L in range(T)]
    dirty = (states[T] ^ states[0]).reshape(plan.H, plan.words, 32).any(2)
    for kcol in range(plan.ncolw):
        cols = slice(plan.word0(kcol), plan.word0(kcol) + plan.own[kcol])
        for grp in range(plan.nseg):
            t, g0, g1 = kcol * plan.nseg + grp, grp * plan.rows, (grp + 1) * plan.rows
            r = np.zeros(plan.own[kcol], np.uint32)
            for L in range(T):
                rows = np.arange(g0 - (T - 1 - L), g1 + (T - 1 - L)) % plan.H
                r |= chg[L][rows][:, cols].any(0).astype(np.uint32) << np.uint32(L)
            r |= dirty[g0:g1, cols].any(0).astype(np.uint32) * np.uint32(native.QUIET_DIRTY)
            r |= dirty[g0:g0 + T, cols].any(0).astype(np.uint32) * np.uint32(native.QUIET_TOP)
            r |= dirty[g1 - T:g1, cols].any(0).astype(np.uint32) * np.uint32(native.QUIET_BOT)
            rec[t, 1:1 + plan.own[kcol]] = r
    return rec


def full_words(native, rec, plan=BASE):
    out = []
    for t in range(plan.tiles):
        own = plan.own[t // plan.nseg]
        w = int(np.bitwise_or.reduce(rec[t, 1:1 + own]))
        if rec[t, 1] & native.QUIET_DIRTY:
            w |= native.QUIET_LEFT
        if rec[t, own] & native.QUIET_DIRTY:
            w |= native.QUIET_RIGHT
        out.append(w)
    return out


def ash(seed=5, still_only=False, plan=BASE):
    g = np.zeros((plan.H, plan.W), np.uint8)
    rng = np.random.default_rng(seed)
    for y in range(4, plan.H - 8, 16):
        for x in range(4, plan.W - 8, 16):
            r = rng.integers(0, 6)
            if r == 0:
                put(g, y, x, BLOCK)
            elif r == 1 and not still_only:
                put(g, y, x, BLINKER)
    return g


def clear(g, y0, y1, x0, x1):
    g[np.ix_(np.arange(y0, y1) % g.shape[0], np.arange(x0, x1) % g.shape[1])] = 0


def model_of(native, plan, group=G):
    assert all(o == 62 for o in plan.own[:-1])  # the model's strips but the last are full
    return native.QuietColsModel(plan.ncolw, plan.nseg, T, plan.own[-1], group)


def run_model(native, g, blocks, cols_from=2, plan=BASE, group=G):
    """Steps `blocks` blocks; checks the model against the full recomputation after each.  Returns per block
    the columns computed per tile."""
    m = model_of(native, plan, group)
    hist, before = [], None  # before: the state two blocks back (what the destination holds)
    for b in range(blocks):
        states = block_states(g)
        rec = fresh_records(native, states, plan)
        cols = b >= cols_from
        done = m.block(rec.reshape(-1).tolist(), b > 0, cols)
        hist.append(done)
        words = [w & ~native.QUIET_COLS for w in m.words()]
        assert words == full_words(native, rec, plan), b
        got = np.array(m.records(), np.uint32).reshape(plan.tiles, -1)
        for t in range(plan.tiles):
            own = plan.own[t // plan.nseg]
            if m.valid(t):
                assert np.array_equal(got[t, 1:1 + own], rec[t, 1:1 + own]), (b, t)
            if b > 0 and before is not None:
                # Columns the block leaves alone: the destination already holds them.
                kcol, grp = divmod(t, plan.nseg)
                for j in range(1, own + 1):
                    if not (done[t] >> j) & 1:
                        c0 = (plan.word0(kcol) + j - 1) * 32
                        rows = slice(grp * plan.rows, (grp + 1) * plan.rows)
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


@col_groups
def test_groups_wider_than_the_strip(native, group):
    """Strips of 1, 2 and 3 columns: one group, cut at the strip's end, whatever the window."""
    for own in (1, 2, 3):
        owned = sum(1 << j for j in range(1, own + 1))
        assert native.quiet_window_spread((1 << 64) - 1, own) == owned
        assert native.quiet_window_spread(1 << 0, own) == 0b10                 # from the left: the first column
        assert native.quiet_window_spread(1 << (own + 1), own) == 1 << own     # from the right: the last one
        groups = -(-own // group)
        for win in (0, 0b10, 1 << own, owned):
            hit = native.quiet_window_groups(win, own, group)
            assert 1 <= hit < 1 << groups, (own, win, hit)
            assert native.quiet_group_columns(hit, own, group) & ~owned == 0
            assert win == 0 or native.quiet_group_columns(hit, own, group) & win == win
        assert native.quiet_group_columns((1 << groups) - 1, own, group) == owned


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


def neighbourhood(native, plan, t):
    kcol, grp = divmod(t, plan.nseg)
    return [native.quiet_neighbour(kcol, grp, i, plan.ncolw, plan.nseg) for i in range(9)]


def window_of_records(native, plan, rec, words, t):
    """quiet_window of tile t on the records and words of all tiles, the nine read through the torus of tiles
    (on a degenerate torus several of the nine are the same tile)."""
    kcol = t // plan.nseg
    nb = neighbourhood(native, plan, t)
    return native.quiet_window([rec[n].tolist() for n in nb], [words[n] for n in nb], plan.own[(kcol - 1) % plan.ncolw],
                               plan.own[kcol], plan.own[(kcol + 1) % plan.ncolw])


def window_of_cells(plan, states, t):
    """The window from the cells alone: the owned columns with a word that differs after the block in the
    column itself or the one to its left or right (on the torus of words), in the tile's rows or the T rows
    above or below them (on the torus of rows)."""
    kcol, grp = divmod(t, plan.nseg)
    rows = np.arange(grp * plan.rows - T, (grp + 1) * plan.rows + T) % plan.H
    src = (states[T] ^ states[0]).reshape(plan.H, plan.words, 32).any(2)[rows].any(0)
    win = 0
    for j in range(1, plan.own[kcol] + 1):
        c = plan.word0(kcol) + j - 1
        if src[(c - 1) % plan.words] or src[c] or src[(c + 1) % plan.words]:
            win |= 1 << j
    return win


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


# ---- The smallest tile tori -------------------------------------------------

def small_field(plan):
    """Still-life ash with, scaled to groups of 40 rows and tori from 32 cells wide: a glider over the column
    wrap and the row seam (on one strip and one group: the tile's own edges), one over the boundary of the
    last two strips or in mid-field, and a soup over the last strip's far edge - the column wrap."""
    g = ash(still_only=True, plan=plan)
    last0 = plan.word0(plan.ncolw - 1) * 32  # the last strip's first cell
    gliders = [(plan.H - 8, plan.W - 8, GLIDER_SE), (plan.rows // 2, last0 + 6 if plan.ncolw > 1 else plan.W // 2, GLIDER_NW)]
    for y, x, pat in gliders:
        clear(g, y - 12, y + 16, x - 12, x + 16)
    y0 = plan.H // 2 - 6
    clear(g, y0 - 8, y0 + 20, plan.W - 14, plan.W + 14)
    for y, x, pat in gliders:
        put(g, y, x, pat)
    soup = np.random.default_rng(1).random((12, 12)) < 0.4
    g[np.ix_(np.arange(y0, y0 + 12), np.arange(plan.W - 6, plan.W + 6) % plan.W)] |= soup
    return g


@small_plans
def test_neighbourhoods_of_the_small_tori_repeat_tiles(native, plan):
    for t in range(plan.tiles):
        nb = neighbourhood(native, plan, t)
        assert nb[4] == t and set(nb) == set(range(plan.tiles))  # every tile is a neighbour of every tile
        kcol, grp = divmod(t, plan.nseg)
        if plan.ncolw <= 2:
            assert [nb[3 * r] for r in range(3)] == [nb[3 * r + 2] for r in range(3)]  # left is right
        if plan.nseg <= 2:
            assert nb[0:3] == nb[6:9]  # above is below
        if plan.ncolw == 1:
            assert nb[3] == nb[5] == t
        if plan.nseg == 1:
            assert nb[1] == nb[7] == t


@all_plans
def test_window_is_the_light_cone_of_the_cells_on_the_torus(native, plan):
    """quiet_window on the records of the numpy torus, the nine tiles read through quiet_neighbour, is the
    window the cells themselves give - with one strip through the tile's own first and last column."""
    g = small_field(plan) if plan is not BASE else None
    if g is None:
        g = ash(still_only=True)
        for y, x, pat in [(50, OWN[0] * 32 - 6, GLIDER_SE), (90, W - 6, GLIDER_SE), (110, 3, GLIDER_NW), (H - 6, 3000, GLIDER_SE)]:
            clear(g, y - 12, y + 16, x - 12, x + 16)
            put(g, y, x, pat)
    seen = set()
    for b in range(4):
        states = block_states(g)
        rec = fresh_records(native, states, plan)
        words = [w | native.QUIET_COLS for w in full_words(native, rec, plan)]
        for t in range(plan.tiles):
            win = window_of_records(native, plan, rec, words, t)
            assert win == window_of_cells(plan, states, t), (b, t)
            own = plan.own[t // plan.nseg]
            seen.add("first" if win & 0b10 else "")
            seen.add("last" if win >> own & 1 else "")
            seen.add("inner" if own > 2 and win & ~(0b10 | 1 << own) else "")
            seen.add("empty" if win == 0 else "")
        g = states[T]
    # First and last columns were in a window (through the wrap, which on one strip is the tile itself).
    assert {"first", "last"} <= seen, seen
    assert plan.words == 1 or "inner" in seen or max(plan.own) <= 2, seen


@small_plans
@col_groups
def test_model_reproduces_the_full_recomputation_on_the_small_tori(native, plan, group):
    m, hist = run_model(native, small_field(plan), 14, plan=plan, group=group)
    computed = [bin(d).count("1") for done in hist[3:] for d in done]
    owned = [plan.own[t // plan.nseg] for _ in hist[3:] for t in range(plan.tiles)]
    assert all(c <= o for c, o in zip(computed, owned))
    # Whole groups, cut at the strip's end: where the last strip is narrower than the group, all its columns.
    for c, o in zip(computed, owned):
        assert c == 0 or c == o or c % group == 0 or (c - o % group) % group == 0, (c, o, group)
    # Columns were computed, and fewer than the tiles own.
    assert 0 < sum(computed) < sum(owned), (sum(computed), sum(owned))
    assert 0 <= m.candidates() <= plan.tiles  # (on 32 x 80 cells everything has settled by the end)


@small_plans
@col_groups
def test_alternating_launches_stay_exact_on_the_small_tori(native, plan, group):
    """Whole-tile launches between column launches publish no records: the next column launch computes
    every column of the tiles they computed, and the words stay those of the full recomputation."""
    g = small_field(plan)
    m = model_of(native, plan, group)
    widths = []
    for b in range(10):
        states = block_states(g)
        rec = fresh_records(native, states, plan)
        cols = b >= 2 and b % 3 != 0
        done = m.block(rec.reshape(-1).tolist(), b > 0, cols)
        assert [w & ~native.QUIET_COLS for w in m.words()] == full_words(native, rec, plan), b
        got = np.array(m.records(), np.uint32).reshape(plan.tiles, -1)
        for t in range(plan.tiles):
            own = plan.own[t // plan.nseg]
            if m.valid(t):
                assert np.array_equal(got[t, 1:1 + own], rec[t, 1:1 + own]), (b, t)
        widths.append((cols, [(plan.own[t // plan.nseg], bin(d).count("1")) for t, d in enumerate(done) if d]))
        g = states[T]
    after_whole = [w for b in range(3, 10) if widths[b][0] and not widths[b - 1][0] for w in widths[b][1]]
    assert after_whole and all(c == own for own, c in after_whole), after_whole  # records unknown: every column
