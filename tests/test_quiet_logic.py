"""Quiet-tile skipping, host decision logic (csrc/include/gol/quiet.hpp): the
skip rule over the nine tile words, the rule for when a block may read the
previous block's words, and the engine's auto policy are pure functions; the
HIP kernel, the HIP backend and the engine call the same code."""
import itertools

import pytest


def words(native, **at):
    """Nine clean words (3 x 3, row-major: 0 above-left ... 4 own ... 8 below-right) with bits set at names."""
    pos = {"ul": 0, "up": 1, "ur": 2, "left": 3, "own": 4, "right": 5, "dl": 6, "down": 7, "dr": 8}
    nb = [0x0FFF] * 9  # change flags never matter
    for k, v in at.items():
        nb[pos[k]] |= v
    return nb


def test_clean_cone_skips_and_flags_do_not_matter(native):
    assert native.quiet_may_skip([0] * 9)
    assert native.quiet_may_skip(words(native))


def test_every_edge_the_cone_touches_blocks_the_skip(native):
    D, T, B, L, R = (native.QUIET_DIRTY, native.QUIET_TOP, native.QUIET_BOT, native.QUIET_LEFT, native.QUIET_RIGHT)
    # own tile: any change
    for bits in (D, D | T, D | B | L | R):
        assert not native.quiet_may_skip(words(native, own=bits))
    # the facing edge of the four side neighbours blocks; their other edges do not
    facing = {"up": B, "down": T, "left": R, "right": L}
    for side, edge in facing.items():
        assert not native.quiet_may_skip(words(native, **{side: D | edge}))
        # (a change in the facing edge sets that edge's bit whatever else is set)
        assert native.quiet_may_skip(words(native, **{side: D | (T | B | L | R) & ~edge}))
    # corners: only the corner itself is read, dirty only if both of its edges are
    corner = {"ul": (B, R), "ur": (B, L), "dl": (T, R), "dr": (T, L)}
    for c, (a, b) in corner.items():
        assert not native.quiet_may_skip(words(native, **{c: D | a | b}))
        assert native.quiet_may_skip(words(native, **{c: D | a}))
        assert native.quiet_may_skip(words(native, **{c: D | b}))
        assert native.quiet_may_skip(words(native, **{c: D | (T | B | L | R) & ~a}))


def test_skip_rule_is_monotone(native):
    """Setting a bit never turns a refusal into a skip (conservative by construction)."""
    bits = [native.QUIET_DIRTY, native.QUIET_TOP, native.QUIET_BOT, native.QUIET_LEFT, native.QUIET_RIGHT]
    for pos, a, b in itertools.product(range(9), bits, bits):
        nb = [0] * 9
        nb[pos] = a
        if not native.quiet_may_skip(nb):
            nb[pos] |= b
            assert not native.quiet_may_skip(nb)


def test_words_are_read_only_by_the_same_plan_on_swapped_buffers(native):
    L = native.QuietLaunch
    prev = L(0x1000, 0x2000)
    assert native.quiet_may_follow(prev, L(0x2000, 0x1000))
    assert not native.quiet_may_follow(prev, L(0x1000, 0x2000))  # same direction: a rotate or a load in between
    assert not native.quiet_may_follow(prev, L(0x2000, 0x3000))
    assert not native.quiet_may_follow(L(0x1000, 0x2000, T=0), L(0x2000, 0x1000))  # invalidated
    for change in (dict(T=4), dict(row_lo=33), dict(row_hi=801), dict(pitch=1024), dict(ncolw=4), dict(nseg=7),
                   dict(seg_rows=97), dict(seg_rem=1), dict(grp_q=24), dict(wrap_w=161)):
        assert not native.quiet_may_follow(prev, L(0x2000, 0x1000, **change)), change


def run_policy(p, n, quiet_expected=None):
    out = []
    for _ in range(n):
        q = p.next()
        p.ran(q)
        out.append(q)
    return out


def test_policy_off_and_on(native):
    off, on = native.QuietPolicy(mode=0), native.QuietPolicy(mode=1)
    assert run_policy(off, 10) == [False] * 10 and off.name() == "off" and off.blocks_dense == 10
    on.report(100, 0)  # reports never move a forced mode
    assert run_policy(on, 10) == [True] * 10 and on.name() == "on" and on.blocks_skip == 10


def test_policy_auto_scouts_switches_and_falls_back_with_hysteresis(native):
    p = native.QuietPolicy(mode=-1, scout=4, on=60, off=35)
    assert p.name() == "auto:dense"
    assert run_policy(p, 8) == [False, False, False, True] * 2  # every 4th block a scout
    assert (p.blocks_dense, p.blocks_scout, p.blocks_skip) == (6, 2, 0)
    p.report(100, 59)
    assert not p.skipping
    p.report(100, 60)
    assert p.skipping and p.name() == "auto:skipping"
    assert run_policy(p, 5) == [True] * 5 and p.blocks_skip == 5
    p.report(100, 35)  # inside the hysteresis band
    assert p.skipping
    p.report(100, 34)
    assert not p.skipping
    assert run_policy(p, 4) == [False, False, False, True]  # the scout interval restarts
    p.report(0, 0)  # a launch without tiles says nothing
    assert not p.skipping
