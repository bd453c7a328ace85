"""CPU-only: the batch util.full_limit_jobs() builds for tests/test_gpu_full_traceback_routes.py holds what it is built for.  Everything here
comes from the CPU oracle's full-matrix traceback (orc.full_gotoh_traceback) and util.full_route_rule(), the routing of
csrc/gotoh_full_traceback.hip restated from its conditions: no GPU result is needed, and none is used.

One departure from a literal reading, forced by the aligner's own rules and asserted as such: the full matrix charges pat_gap_* for either
gap kind (txt_gap_* only initialise GLOBAL's first column) while G = e2e_gap_bound comes from the cheaper of the two kinds, so under
(0,6,6,-11,-4,-6,-2) a lone gap of L symbols costs 11 + 4 (L - 1) and gives G = 2 L + 1 or more: no traced gap equals G there.  The jobs
on diagonal 0 and W are asserted present and restricted under that scheme, tight under the three others."""
import numpy as np
import pytest

import oracle
from util import (ALN_NO_BAND_ROUTE, ALN_NO_NARROW_TRACEBACK, ALN_NO_UNGAPPED_TRACEBACK, FULL_LIMIT_COLS, FULL_LIMIT_CUT_SCHEME, FULL_LIMIT_READ_LENS,
                  FULL_LIMIT_SHORT_K, LIMIT_GAP_KINDS, LIMIT_SCHEMES, full_gap_bound, full_gap_mins, full_limit_jobs, full_limit_oracle, full_route_rule,
                  limit_select)

SEED = 20262
STRIDE = 16
SG = oracle.SEMI_GLOBAL
NARROW = [s for s in LIMIT_SCHEMES if s[0] != "refused"]


@pytest.fixture(scope="module")
def pool(orc):
    """the generator's jobs but the `cut` ones, and per scheme the oracle's results and the rule's routes; the cut jobs under their scheme"""
    J = full_limit_jobs(SEED)
    main = limit_select(J, np.nonzero(J["kind"] != "cut")[0])
    cut = limit_select(J, np.nonzero(J["kind"] == "cut")[0])
    P = dict(J=main, cut=cut, want={}, rule={})
    for name, sv, with_q in LIMIT_SCHEMES + (FULL_LIMIT_CUT_SCHEME,):
        S = cut if name == "cut" else main
        P["want"][name] = full_limit_oracle(orc, SG, sv, S, with_q, STRIDE)
        P["rule"][name] = full_route_rule(S, with_q, SG, sv, P["want"][name])
    return P


def _forward(cig, ln):
    """a CIGAR row (backtracking order) -> [(op, length)] in read order"""
    els = cig[:int(ln)][::-1].astype(np.int64)
    return [(int(e & 3), int(e >> 2)) for e in els]


def _traced_gap(cig, ln):
    """gap symbols in a CIGAR row"""
    return sum(n for op, n in _forward(cig, ln) if op in (1, 2))


def _first_gap(cig, ln):
    """(the read column the first gap of a CIGAR row starts at, its op), (-1, -1) without a gap"""
    col = 0
    for op, n in _forward(cig, ln):
        if op in (1, 2):
            return col, op
        col += n
    return -1, -1


def _reachable(sv, with_q):
    """the costs the generator's gapped paths can have: one gap of 1..12 symbols, alone, with a substitution or beside a second gap.  The
    aligner charges pat_gap_* for either gap kind"""
    gap = [-(sv[3] + (k - 1) * sv[4]) for k in range(1, 13)]
    mm = range(sv[1], sv[2] + 1) if with_q else (sv[1],)
    return sorted(set(gap) | {g + m for g in gap for m in mm} | {gap[a] + gap[b] for a in range(12) for b in range(12) if a + b + 2 <= 12})


def test_pool_shape(pool):
    """deterministic, a few thousand jobs of at most 65 x 105 cells plus the handful of 252 x 272, every read length and window present"""
    J, C = pool["J"], pool["cut"]
    again = full_limit_jobs(SEED)
    assert all(np.array_equal(a, b) for a, b in zip(again["pats"], list(J["pats"]) + list(C["pats"]))) and 3000 <= len(J["pats"]) <= 8000
    assert max(len(p) for p in J["pats"]) == 65 and max(len(t) for t in J["txts"]) == 104
    assert sorted({len(p) for p in C["pats"]}) == [249, 250, 251, 252] and {len(t) - len(p) for p, t in zip(C["pats"], C["txts"])} == {20}
    assert set(np.unique(J["M"])) >= set(FULL_LIMIT_READ_LENS) and set(np.unique(J["W"])) >= {13, 14, 15, 22, 40, -1, -7, -8, -9}
    for W in (13, 14, 15, 22):
        gaps = np.isin(J["kind"], LIMIT_GAP_KINDS) & (J["W"] == W)
        assert set(J["delta"][gaps]) == set(range(W + 1)), W
    assert set(J["delta"][np.isin(J["kind"], LIMIT_GAP_KINDS) & (J["W"] == 40)]) == set(range(10)) | {19, 20} | set(range(31, 41))
    assert (J["fill"] == 4).sum() >= 10


@pytest.mark.parametrize("scheme", NARROW, ids=lambda s: s[0])
def test_reach(pool, scheme):
    """the conditions of the issue, on the oracle's output and the restated rule alone"""
    name, sv, with_q = scheme
    J, want, (rt, gb) = pool["J"], pool["want"][name], pool["rule"][name]
    go, ge = full_gap_mins(sv)
    n = len(rt)
    a = -want[0].astype(np.int64)
    x, y = want[2][:, 0].astype(np.int64), want[2][:, 1].astype(np.int64)
    delta, W = x - y, J["W"].astype(np.int64)
    G = np.array([full_gap_bound(int(v), sv) for v in a])
    assert (want[4] > 0).all() and (y == J["M"]).all() and set(np.unique(rt)) == {0, 2, 3} and (gb[rt >= 2] == G[rt >= 2]).all() and not gb[rt == 0].any()

    # the cut G = 7 | 8 among the jobs the band route's geometry admits: route 3 below, route 2 above, at the two nearest reachable costs
    geo = (rt > 0) & (W >= 14) & (delta >= 7) & (delta + 7 <= W)
    cut = go + 7 * ge - 1
    sums = _reachable(sv, with_q)
    lo, hi = max(v for v in sums if v <= cut), min(v for v in sums if v > cut)
    assert (rt[geo & (a <= cut)] == 3).all() and (rt[geo & (a > cut)] == 2).all() and (G[a == lo] == 7).all() and (G[a == hi] >= 8).all()
    assert (geo & (a == lo) & (rt == 3)).sum() >= 4 and (geo & (a == hi) & (rt == 2)).sum() >= 4, (name, cut, lo, hi)
    if name in ("equal", "ramp"):
        assert (lo, hi) == (28, 29)
    assert not (rt[~geo] == 3).any()

    # either end of the window: route 3 at delta = 7 and W - 7, route 2 at 6 and W - 6 for want of room alone (G <= 7)
    for w in (15, 22, 40):
        for d, code in ((7, 3), (w - 7, 3), (6, 2), (w - 6, 2)):
            assert ((W == w) & (delta == d) & (rt == code) & (G <= 7)).sum() >= 2, (name, w, d, code)
    # windows of M + 13 | 14 | 15
    assert not (rt[W == 13] == 3).any() and (rt[W == 13] == 2).sum() >= 100
    assert set(delta[(W == 14) & (rt == 3)]) == {7} and ((W == 14) & (rt == 3)).sum() >= 4
    assert set(delta[(W == 15) & (rt == 3)]) == {7, 8} and min(((W == 15) & (rt == 3) & (delta == d)).sum() for d in (7, 8)) >= 4

    # restricted jobs tight against G whose path runs on the first diagonal of the window (a deletion at delta = L) and on the last (an
    # insertion at delta = W - L)
    gaps = np.array([_traced_gap(want[3][j], want[4][j]) for j in range(n)])
    assert (gaps[rt >= 2] <= G[rt >= 2]).all()                                   # (what makes the restricted rows right)
    on_first = (J["kind"] == "del") & (J["delta"] == J["L"]) & (delta == J["delta"]) & (rt == 2)
    on_last = (J["kind"] == "ins") & (J["delta"] == W - J["L"]) & (delta == J["delta"]) & (rt == 2)
    tight = gaps == G
    if name == "cheap_txt":                                                      # (never tight: see the module's docstring)
        assert on_first.sum() >= 20 and on_last.sum() >= 20 and not (tight & (gaps > 0)).any()
    else:
        assert (on_first & tight).sum() >= 20 and (on_last & tight).sum() >= 20
        assert (on_first & tight & (G >= 8)).any() and (on_last & tight & (G >= 8)).any() and (tight & (rt == 3) & (G == 7)).any()
    # the row clamps: the region reaches past row 0, and past the last row
    assert ((rt == 2) & (delta >= 0) & (delta < gb)).sum() >= 100 and ((rt == 2) & (W > 0) & (delta + gb > W)).sum() >= 100
    # short texts: the sink's diagonal is negative
    short = np.char.startswith(J["kind"], "short")
    for k in FULL_LIMIT_SHORT_K + (63,):
        for kind in ("short", "short_lead"):
            sel = (J["kind"] == kind) & (J["L"] == k) & (J["M"] == 64)
            assert sel.sum() >= 4 and (rt[sel] == 2).all() and (x[sel] < y[sel]).all() and (delta[sel] == -k).all(), (name, k, kind)
    assert (x[short] < y[short]).all()
    if name == "equal":                                                          # the bound is tight there: trailing insertions, k of them
        for M, N, k in ((20, 10, 10), (64, 56, 8)):
            sel = np.nonzero((J["kind"] == "short") & (J["M"] == M) & (W == N - M))[0]
            assert len(sel) >= 4
            for j in sel:
                assert oracle.cigar_string(want[3][j, :want[4][j]], reverse=True) == "%dM%dI" % (N, k) and gb[j] == k and a[j] == 5 + 3 * k

    # the shortcut: at least 100 jobs, at every delta of both windows
    assert (rt == 0).sum() >= 100
    for w in (15, 40):
        assert set(delta[(rt == 0) & (W == w) & (J["kind"] == "ungapped")]) == set(range(w + 1)), (name, w)
    # stripe boundaries: per column of the list a traced gap of every kind that starts there
    first = np.array([_first_gap(want[3][j], want[4][j]) for j in range(n)])
    for col in FULL_LIMIT_COLS:
        for kind in LIMIT_GAP_KINDS:
            sel = (J["kind"] == kind) & (J["col"] == col) & (rt >= 2) & (first[:, 0] == col)
            assert sel.sum() >= 4, (name, col, kind)
            if kind.startswith(("del", "ins")):
                assert (first[sel, 1] == (2 if kind.startswith("del") else 1)).all()
        for op in (1, 2):                                                        # an insertion run that spans the boundary; a deletion that sits on it
            assert ((first[:, 0] == col) & (first[:, 1] == op) & (rt == 2) & (gaps >= 2)).any() and ((first[:, 0] == col) & (first[:, 1] == op) & (rt == 3)).any()
    # read lengths
    for M in FULL_LIMIT_READ_LENS:
        sel = J["M"] == M
        assert (sel & (rt == 0)).sum() >= 4 and (sel & (rt >= 2)).sum() >= (4 if M >= 7 else 0), (name, M)     # (one symbol: its diagonal is the optimum)
        if M >= 16:
            assert (sel & (rt == 2) & (gaps > 0)).any() and (sel & (rt == 3) & (gaps > 0)).any(), (name, M)


def test_reach_refused_scheme(pool):
    """under a match bonus neither narrow route takes a job; the batch still holds settled and DP jobs"""
    rt, gb = pool["rule"]["refused"]
    assert set(np.unique(rt)) == {0, 1} and not gb.any() and (rt == 0).sum() >= 300 and (rt == 1).sum() >= 2000


def test_reach_last_cut(pool):
    """G <= 250 | 251 under (0,3,3,-1,-1,-1,-1): a read of M symbols 0 in a window without one is M insertions at -M, G = M: restricted with
    gap_bound 250 at M = 250, over all rows with gap_bound 0 at M = 251"""
    C, want, (rt, gb) = pool["cut"], pool["want"]["cut"], pool["rule"]["cut"]
    for M in (249, 250, 251, 252):
        sel = np.nonzero(C["M"] == M)[0]
        assert len(sel) == 4 and (want[0][sel] == -M).all()
        for j in sel:
            assert oracle.cigar_string(want[3][j, :want[4][j]]) == "%dI" % M
        assert (rt[sel] == (2 if M <= 250 else 1)).all() and (gb[sel] == (M if M <= 250 else 0)).all()
    assert len({tuple(np.unique(t)) for t in C["txts"]}) == 2                    # texts of three letters, and of two


def test_rule_flags(pool):
    """the four switches of the rule: the shortcut off reports (1, 0) throughout, NO_NARROW never 2 or 3, NO_BAND_ROUTE never 3 and 2 in its place"""
    name, sv, with_q = LIMIT_SCHEMES[0]
    J, want, (rt, gb) = pool["J"], pool["want"][name], pool["rule"][name]
    r, g = full_route_rule(J, with_q, SG, sv, want, ALN_NO_UNGAPPED_TRACEBACK)
    assert (r == 1).all() and not g.any()
    r, g = full_route_rule(J, with_q, SG, sv, want, ALN_NO_NARROW_TRACEBACK)
    assert np.array_equal(r, np.minimum(rt, 1)) and not g.any()
    r, g = full_route_rule(J, with_q, SG, sv, want, ALN_NO_BAND_ROUTE)
    assert np.array_equal(r, np.minimum(rt, 2)) and np.array_equal(g, gb)
