"""The candidate list of the skipping kernel (csrc/include/gol/quiet.hpp, tuning
quiet_list): the pure logic, through the bindings.  A host model keeps the list
as the kernel does - two word maps, launch stamps, flag counts - and must skip
and compute exactly the tiles that evaluating quiet_may_skip on every tile of
every block does, whatever the words: the argument is about words only (a tile
none of whose nine neighbours computed reads the nine words it read before).

The reference has no counterpart (every generation rewrites every cell,
src/game_cuda.cu:128-148)."""
import numpy as np
import pytest

import gol_amd

C = gol_amd.native()
T = 12
DET = [C.QUIET_DIRTY, C.QUIET_TOP, C.QUIET_BOT, C.QUIET_LEFT, C.QUIET_RIGHT]


def neighbours(t, ncolw, nseg):
    return [C.quiet_neighbour(t // nseg, t % nseg, i, ncolw, nseg) for i in range(9)]


def random_words(rng, tiles, p_dirty):
    """Words a computing tile might publish: mostly clean (or nothing would
    ever skip), dirty ones with any mix of edge bits, a few patterns of change
    flags (so that a tile often publishes the word it published before)."""
    out = []
    for _ in range(tiles):
        w = int(rng.choice([0, 0, (1 << T) - 1, 0x555]))
        if rng.random() < p_dirty:
            w |= C.QUIET_DIRTY
            for b in DET[1:]:
                if rng.random() < 0.4:
                    w |= b
        out.append(w)
    return out


def recount(words):
    return [sum((w >> L) & 1 for w in words) for L in range(T)]


def test_neighbourhood_is_symmetric_and_wraps():
    for ncolw, nseg in ((3, 8), (1, 4), (2, 2), (17, 341)):
        tiles = ncolw * nseg
        for t in (0, 1, nseg - 1, tiles - 1, tiles // 2):
            nb = neighbours(t, ncolw, nseg)
            assert nb[4] == t and all(0 <= n < tiles for n in nb)
            for n in set(nb):
                assert t in neighbours(n, ncolw, nseg), (ncolw, nseg, t, n)
    # 3 x 8: nine distinct tiles; 2 x 2: every tile is a neighbour of every tile.
    assert len(set(neighbours(9, 3, 8))) == 9
    assert set(neighbours(0, 2, 2)) == {0, 1, 2, 3}
    assert neighbours(0, 3, 8) == [2 * 8 + 7, 7, 8 + 7, 2 * 8, 0, 8, 2 * 8 + 1, 1, 8 + 1]


def test_flag_counts_pack_and_unpack():
    nw = C.quiet_flag_words(T)
    assert nw == 4 and C.quiet_flag_words(16) == 6
    rng = np.random.default_rng(3)
    words = [0] * 500
    counts = [0] * nw
    for _ in range(4000):  # tiles change their words in any order: the sums stay the counts
        t = int(rng.integers(0, len(words)))
        new = int(rng.integers(0, 1 << T)) | (C.QUIET_DIRTY if rng.random() < 0.5 else 0)
        for w in range(nw):
            counts[w] = (counts[w] + C.quiet_flag_delta(words[t], new, w)) % (1 << 64)
        words[t] = new
    want = recount(words)
    levels = 0
    for w in range(nw):
        levels |= C.quiet_flag_levels(counts[w], w)
        for j in range(3):
            assert (counts[w] >> (21 * j)) & ((1 << 21) - 1) == want[3 * w + j]
    assert levels == sum(1 << L for L in range(T) if want[L])
    assert C.quiet_flag_delta(0x5, 0x5 | C.QUIET_DIRTY, 0) == 0  # detection bits are no flags


def test_neighbourhoods_of_the_smallest_tori_repeat_tiles():
    """One strip: a tile is its own left and right neighbour; one group: its own upper and lower one; two:
    both neighbours are the same tile.  A computing tile then marks a tile several times (the stamps)."""
    assert neighbours(0, 1, 1) == [0] * 9
    assert neighbours(0, 1, 2) == [1, 1, 1, 0, 0, 0, 1, 1, 1] and neighbours(1, 1, 2) == [0, 0, 0, 1, 1, 1, 0, 0, 0]
    assert neighbours(0, 2, 1) == [1, 0, 1] * 3 and neighbours(1, 2, 1) == [0, 1, 0] * 3
    assert neighbours(0, 2, 2) == [3, 1, 3, 2, 0, 2, 3, 1, 3]
    for ncolw, nseg in ((1, 1), (1, 2), (2, 1)):
        for t in range(ncolw * nseg):
            for n in set(neighbours(t, ncolw, nseg)):
                assert t in neighbours(n, ncolw, nseg), (ncolw, nseg, t, n)


@pytest.mark.parametrize("ncolw,nseg", [(3, 8), (1, 4), (2, 2), (1, 1), (1, 2), (2, 1)])
@pytest.mark.parametrize("p_dirty", [0.15, 0.4])
def test_list_computes_what_full_evaluation_computes(ncolw, nseg, p_dirty):
    tiles = ncolw * nseg
    rng = np.random.default_rng(100 * ncolw + nseg + int(100 * p_dirty))
    model = C.QuietListModel(ncolw, nseg, T)
    prev = None  # full evaluation: the map the last block wrote (None: nothing to follow)
    skipped_any = computed_any = short_list = False
    for block in range(50):
        follow = prev is not None and block not in (10, 20, 21, 35, 42)  # invalidations, two in a row
        # Activity dies down in the middle of the chain, so lists get short and tiles leave them.
        p = p_dirty if block % 10 < 6 else 0.0
        if tiles <= 2 and not follow:
            p = 1.0  # one or two tiles: a clean first word would be republished until the next invalidation
        fresh = random_words(rng, tiles, p)
        if follow:
            skip = [C.quiet_may_skip([prev[n] for n in neighbours(t, ncolw, nseg)]) for t in range(tiles)]
        else:
            skip = [False] * tiles
        want = [prev[t] if skip[t] else fresh[t] for t in range(tiles)]
        got_computed = model.block(fresh, follow)
        assert sorted(got_computed) == [t for t in range(tiles) if not skip[t]], block
        assert len(set(got_computed)) == len(got_computed), block
        assert list(model.words()) == want, block
        assert model.flag_counts() == recount(want), block
        assert model.flags() == sum(1 << L for L in range(T) if recount(want)[L]), block
        # What is launched: every tile after an invalidation and in the block after it, else what
        # computed and the neighbourhoods of the words that changed; the next block's candidates likewise.
        if follow:
            cand = set()
            for t in got_computed:  # itself; the tiles that read its word if the word changed
                cand.update(neighbours(t, ncolw, nseg) if want[t] != prev[t] else [t])
            assert model.candidates() == len(cand), block
        else:
            assert model.launched() == tiles and model.candidates() == tiles, block
        skipped_any |= any(skip)
        computed_any |= follow and len(got_computed) > 0
        short_list |= follow and model.launched() < tiles
        prev = want
    assert skipped_any and computed_any and (short_list or tiles == 4), "vacuous"
