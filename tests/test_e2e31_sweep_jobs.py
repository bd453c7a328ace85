"""CPU-only: the pool util.e2e31_sweep_jobs() builds for tests/test_gpu_band31_scheme_sweep.py holds what it is built for.  Everything here is the
oracle and the numpy restatement of the first pass's rule (util.e2e31_first_pass); nothing is measured.

The pool must drive every route of the band-31 end-to-end shortcuts under every regime of the scheme numbers P, go, ge: what a scheme's rule can
flag at all is computed from the rule itself (util.e2e31_possible_flags: one window whose centre diagonal holds 0..M mismatches), and the pool has
to hold at least 5 jobs of each such flag and narrow class.

Two things the rule settles by itself, asserted here so that a change of them is seen:
  * ge = 0: no chance ever applies.  A job that is not settled has U* <= G, so go + g ge = go reaches U* for every g or for none: gmax is 0 or 5,
    never 1..4, and the gap chance asks for ge < 0.  Only flags 0 and 1 occur.
  * |go| < |ge|: `beyond` holds (ge < go), so the third chance flags nothing, and go <= ge fails, so neither does the gap chance; the second
    chance flags the jobs whose U* lies in (max(G - P, 2 G), G] -- under 1 / -2 / -5 the reads with two mismatches."""
import numpy as np

import oracle
from util import (E2E31_CORNERS, E2E31_SWEEP, e2e31_admitted, e2e31_counts, e2e31_first_pass, e2e31_layout, e2e31_possible_flags, e2e31_sweep_jobs)

SEED = 1
DEFAULT = (0, 6, 6, -8, -3, -8, -3)


def _pool():
    J = e2e31_sweep_jobs(SEED)
    return J, J["M"].astype(np.int64), np.array([len(t) for t in J["txts"]], dtype=np.int64), e2e31_counts(J)


def test_the_scheme_lists():
    assert len(E2E31_SWEEP) == 138 and len(set(E2E31_SWEEP)) == 138
    assert all(sv[0] == 0 and sv[1] == sv[2] and sv[3] == sv[5] and sv[4] == sv[6] for sv in E2E31_SWEEP)
    assert {sv[1] for sv in E2E31_SWEEP} == {0, 1, 2, 3, 6, 30} and {-sv[3] for sv in E2E31_SWEEP} == {1, 2, 5, 8, 40}
    names = [c[0] for c in E2E31_CORNERS]
    assert len(set(names)) == len(names) and len({c[1] for c in E2E31_CORNERS}) == len(names)
    corners = {c[1]: c[2] for c in E2E31_CORNERS}
    for sv in ((0, 1, 1, -1, -1, -1, -1), (0, 30, 30, -2, -1, -2, -1), (0, 1, 1, -40, -3, -40, -3), (0, 6, 6, -11, -4, -6, -2), (0, 6, 6, -6, -2, -11, -4),
               (0, 6, 6, -8, -3, -8, -3), (0, 2, 2, -5, -1, -5, -1), (0, 4, 4, -6, -6, -6, -6), (0, 3, 3, -4, -2, -4, -2), (0, 6, 6, -5, -3, -5, -3),
               (0, 3, 3, -3, -3, -9, -1)):
        assert corners[sv] is False
    assert corners[(0, 2, 6, -8, -3, -8, -3)] and corners[(0, 1, 7, -8, -3, -8, -3)] and corners[(0, 3, 10, -8, -3, -8, -3)]
    assert corners[(0, 0, 6, -8, -3, -8, -3)] is False
    regimes = dict(p0=lambda s: s[1] == 0, ge0=lambda s: s[4] == 0, open_below_ext=lambda s: -s[3] < -s[4],
                   linear_below=lambda s: s[3] == s[4] and s[1] < -s[3], linear_above=lambda s: s[3] == s[4] and s[1] > -s[3])
    for name, holds in regimes.items():
        assert any(holds(c[1]) for c in E2E31_CORNERS) and any(holds(sv) for sv in E2E31_SWEEP), name
    # a mismatch that costs nothing is not admitted to the shortcuts; everything else of the two lists is, at both read lengths the GPU test declares
    for sv, q in [(sv, False) for sv in E2E31_SWEEP] + [(c[1], c[2]) for c in E2E31_CORNERS]:
        packed = (162 + 32) * max(abs(v) for v in sv) <= 8000
        assert e2e31_admitted(sv, q, 162) == (sv[1] > 0 and packed) and e2e31_admitted(sv, q, 64) == (sv[1] > 0), sv


def test_the_pool_is_deterministic_and_nothing_is_left_out():
    J, M, N, C = _pool()
    n = len(J["pats"])
    assert 4000 < n < 6000 and all(len(v) == n for v in J.values())
    again = e2e31_sweep_jobs(SEED)
    assert all(np.array_equal(a, b) for key in ("pats", "txts", "quals") for a, b in zip(J[key], again[key]))
    kinds = set(J["kind"])
    assert kinds >= {"del", "ins", "del+sub", "ins+sub", "split", "ungapped", "overhang", "subs", "gap+subs", "gaps2", "gaps3", "longgap", "periodic",
                     "periodic_gap", "n", "near_centre", "many_subs", "allmm"}
    added = ~np.isin(J["kind"], ("del", "ins", "del+sub", "ins+sub", "split", "ungapped", "overhang"))
    assert set(M[added]) == {64, 161} and (J["win"][added] == 31).all()
    assert {int(m) for m in M} == {33, 64, 160, 161, 162} and {int(w) for w in (N - M)[N >= M]} >= {29, 30, 31}
    assert int((N < M).sum()) == 15                                  # windows shorter than their read: nothing is reported
    assert set(J["L"][J["kind"] == "subs"]) == set(range(4, 13)) and set(J["L"][J["kind"] == "longgap"]) == {5, 6, 9}
    assert sum(int((p == 4).sum()) for p in J["pats"]) >= 100
    # every job gets a flag from the rule, under every scheme of both lists
    for sv, q in [(sv, False) for sv in E2E31_SWEEP[::7]] + [(c[1], c[2]) for c in E2E31_CORNERS]:
        flag, cls = e2e31_first_pass(sv, q, M, N, C, weights=e2e31_counts(J, sv) if q else None, max_read_len=162)
        assert len(flag) == n and np.isin(flag, (0, 1, 2, 3, 4)).all() and (cls[flag != 1] == 0).all()


def test_every_route_occurs_under_the_default_scheme():
    J, M, N, C = _pool()
    flag, cls = e2e31_first_pass(DEFAULT, False, M, N, C, max_read_len=162)
    for f in range(5):
        assert int((flag == f).sum()) >= 20, (f, np.bincount(flag))
    assert int((cls == 1).sum()) >= 20 and int((cls == 2).sum()) >= 20, np.bincount(cls)


def test_every_flag_a_corner_scheme_can_give_occurs():
    J, M, N, C = _pool()
    short = M == 64
    plain = (M <= 161) & (N >= M)                                     # (longer reads are the DP's whatever the scheme: flag 1)
    for name, sv, q in E2E31_CORNERS:
        W = e2e31_counts(J, sv) if q else None
        flag, cls = e2e31_first_pass(sv, q, M, N, C, weights=W, max_read_len=162)
        seen = {int(f) for f in flag[plain]} | {10 + int(c) for c in cls if c}
        possible = e2e31_possible_flags(sv, q, 161, 162) | {f for f in e2e31_possible_flags(sv, q, 64, 162) if f < 10}
        assert seen <= possible | {1}, (name, seen, possible)
        for f in possible:
            count = int((flag[plain] == f).sum()) if f < 10 else int((cls == f - 10).sum())
            assert count >= 5, (name, f, count)
        # the M = 64 jobs alone, declared as 64 symbols long: the binary16 DP and its classes wherever the scheme admits them
        flag, cls = e2e31_first_pass(sv, q, M[short], N[short], C[short], weights=W[short] if q else None, max_read_len=64)
        for f in e2e31_possible_flags(sv, q, 64, 64):
            if f >= 10:
                assert int((cls == f - 10).sum()) >= 5, (name, "M = 64", f)


def test_p0_sinks_are_not_the_fewest_mismatch_diagonal(orc):
    """a mismatch that costs nothing: every diagonal scores 0 and BestSink's last maximum is the last reportable column, whatever the diagonals'
    counts -- what the first pass would report is the fewest-mismatch diagonal, so the host must keep such a scheme off the shortcut"""
    J, M, N, C = _pool()
    d = e2e31_layout(orc, J)
    whole = (N >= M + 30)
    best_d = 30 - np.argmin(np.where(C >= 0, C, 1 << 40)[:, ::-1], axis=1)
    for sv in ((0, 0, 0, -5, -3, -5, -3), (0, 0, 6, -8, -3, -8, -3)):
        s, k = orc.banded_gotoh_packed_batch(31, oracle.SEMI_GLOBAL, oracle.Scheme(*sv), d["reads4"], d["roffs"], d["text"], d["wb"], d["we"])
        assert (s[N >= M] == 0).all() and (k[whole, 0] == M[whole] + 30).all()
        differ = int((k[whole, 0].astype(np.int64) - M[whole] != best_d[whole]).sum())
        assert 2 * differ >= int(whole.sum()), (sv, differ, int(whole.sum()))
        assert not e2e31_admitted(sv, False, 162)


def test_zero_extension_and_open_below_extension():
    J, M, N, C = _pool()
    for name, sv, q in E2E31_CORNERS:
        go, ge = sv[3], sv[4]
        if q or sv[1] == 0 or not (ge == 0 or -go < -ge):
            continue
        flag, cls = e2e31_first_pass(sv, q, M, N, C, max_read_len=162)
        assert not (flag == 2).any() and not (flag == 4).any(), name
        if ge == 0:
            assert not (flag == 3).any() and (cls == 0).all(), name
    seconds = [int((e2e31_first_pass(c[1], False, M, N, C)[0] == 3).sum()) for c in E2E31_CORNERS if c[1][1] > 0 and -c[1][3] < -c[1][4]]
    assert len(seconds) >= 3 and max(seconds) >= 50, seconds
    # the grid: the same under every scheme of either regime
    for sv in E2E31_SWEEP:
        if sv[1] > 0 and (sv[4] == 0 or -sv[3] < -sv[4]):
            possible = e2e31_possible_flags(sv, False, 161, 162)
            assert not possible & {2, 4} and (sv[4] != 0 or possible <= {0, 1}), (sv, possible)
