"""CPU: the band-31 DP's narrow classes, restated in numpy (banded_gotoh_band31_pk_kernel with NARROW, the classes of ungapped_e2e31_job).

A job the first pass sends to the DP with a known best diagonal -- U* its score, best_d its column -- gets a class from those two alone: with
r(L) = the largest delta with open + (delta - 1) ext >= L and w = r(U*) + |best_d - 15|, class A (columns 9..21) is w <= 6, class B
(columns 7..23) is w <= 8, anything else keeps the full band.  A class job runs rows 0..23 over the whole band, is qualified at row 24 (every
outer H and F below L = U*, per job; the outer columns then hold the infimum), runs the other rows over its columns only -- column LO takes no E,
column HI no F -- under a monitor (the maximum of what flows outward: max(Hg[LO], F[LO] + ext) of the row before, and E' of column HI), and is
REDONE over the full band unless it qualified and the monitor stayed below L.

Pinned here, against a plain numpy band-31 Gotoh: every job that is not redone has the full band's score and sink, for random reads with 4, 5
and 6 substitutions under five schemes; the random 4- (5-) substitution reads under 0 / -6 / -8 / -3 take class A (B) and are not redone, so
the narrow recurrence is what gets compared; and two decoys are redone -- an outer diagonal (offset 12) that matches the read's first 40 rows,
and the boundary diagonal (offset 6) matching rows 0..59 but for two substitutions.  Both are caught by the qualification: a boundary cell
that can send L outward at row 24 or later (E' = H + open >= L) has sent it into the next column at row 23 already, and a live diagonal left
of the centre feeds column LO - 1 through a pattern gap at every row, so wherever a run of exact rows starts before row 24 the outer cells
hold it at row 24.  The monitor is the guard the proof needs for everything the qualification does not see; a third test drives it alone
(the qualification's share left out of the numpy run) on exact reads, where what flows outward is known in closed form."""
import numpy as np

from util import BAND31, NARROW_HALF_A, NARROW_HALF_B, classes, reach

BAND, FULL_ROWS, HALF_A, HALF_B = BAND31, 24, NARROW_HALF_A, NARROW_HALF_B
NEG = -16384
SCHEMES = ((6, -8, -3), (2, -5, -1), (4, -6, -6), (3, -4, -2), (6, -5, -3))        # (mismatch penalty, gap open, gap extension)


def mismatches(reads, wins):
    """mm[n, i, j]: row i of the read differs from column j of the band in that row (text symbol i + j of the window)"""
    n, M = reads.shape
    idx = np.arange(M)[:, None] + np.arange(BAND)[None, :]
    return reads[:, :, None] != wins[:, idx]


def _row(H, F, mm_i, P, go, ge, lo, hi, mon=None):
    """one row over columns lo..hi, in place; returns the row's E' of column hi"""
    if mon is not None:
        np.maximum(mon, np.maximum(H[:, lo] + go, F[:, lo] + ge), out=mon)       # what the row before sends into column lo - 1
    Hn, Fn = H.copy(), F.copy()
    e = np.full(len(H), NEG)
    for j in range(lo, hi + 1):
        f = np.maximum(F[:, j + 1] + ge, H[:, j + 1] + go) if j < hi else np.full(len(H), NEG)
        d = H[:, j] - P * mm_i[:, j]
        h = np.maximum(np.maximum(f, d), e) if j > lo else np.maximum(f, d)
        e = np.maximum(h + go, e + ge) if j > lo else h + go
        Hn[:, j], Fn[:, j] = h, f
    H[:], F[:] = Hn, Fn
    if mon is not None:
        np.maximum(mon, e, out=mon)                                               # what column hi sends into column hi + 1
    return e


def _report(H):
    score = H.max(axis=1)
    return score, (BAND - 1) - np.argmax(H[:, ::-1] == score[:, None], axis=1)    # the LAST maximum wins


def full_band(mm, P, go, ge):
    n, M, _ = mm.shape
    H, F = np.zeros((n, BAND), dtype=np.int64), np.full((n, BAND), NEG, dtype=np.int64)
    for i in range(M):
        _row(H, F, mm[:, i], P, go, ge, 0, BAND - 1)
    return _report(H)


def narrow_band(mm, P, go, ge, L, half, qualify=True):
    """-> (score, sink column, redone) of class jobs with half-width `half` and bound L per job (qualify = False: the monitor alone decides)"""
    n, M, _ = mm.shape
    lo, hi = 15 - half, 15 + half
    outer = np.array([j < lo or j > hi for j in range(BAND)])
    H, F = np.zeros((n, BAND), dtype=np.int64), np.full((n, BAND), NEG, dtype=np.int64)
    mon = np.full(n, NEG, dtype=np.int64)
    for i in range(M):
        if i < FULL_ROWS:
            _row(H, F, mm[:, i], P, go, ge, 0, BAND - 1)
            continue
        if i == FULL_ROWS:                                                        # the qualification joins the monitor: both are held against L
            if qualify:
                np.maximum(mon, np.maximum(H[:, outer].max(axis=1), F[:, outer].max(axis=1)), out=mon)
            H[:, outer] = NEG; F[:, outer] = NEG
        _row(H, F, mm[:, i], P, go, ge, lo, hi, mon)
    score, col = _report(H)
    return score, col, mon >= L


def _random_jobs(rng, n, M, ks):
    wins = rng.integers(0, 4, (n, M + BAND), dtype=np.uint8)
    reads = wins[:, 15:15 + M].copy()
    for q in range(n):
        k = ks[q % len(ks)]
        pos = rng.choice(M, k, replace=False)
        reads[q, pos] = (reads[q, pos] + 1 + rng.integers(0, 3, k)) % 4
    return reads, wins


def decoy_outer(rng, n, M=150, period=12, rows=40):
    """class A jobs (4 substitutions behind row 60 on the centre diagonal) whose diagonal 15 + period matches rows 0 .. rows - 1 exactly"""
    wins = rng.integers(0, 4, (n, M + BAND), dtype=np.uint8)
    for q in range(n):
        wins[q, 15:15 + rows + period] = np.resize(wins[q, 15:15 + period], rows + period)
    reads = wins[:, 15:15 + M].copy()
    for q in range(n):
        pos = 60 + rng.choice(M - 60, 4, replace=False)
        reads[q, pos] = (reads[q, pos] + 1 + rng.integers(0, 3, 4)) % 4
    return reads, wins


def decoy_boundary(rng, n, M=150, period=6, rows=60):
    """class A jobs whose boundary diagonal 15 + period matches rows 0 .. rows - 1 but for the read's two substitutions there (two more lie
    behind row 70)"""
    wins = rng.integers(0, 4, (n, M + BAND), dtype=np.uint8)
    for q in range(n):
        wins[q, 15:15 + rows + period] = np.resize(wins[q, 15:15 + period], rows + period)
    reads = wins[:, 15:15 + M].copy()
    for q in range(n):
        pos = np.concatenate([24 + rng.choice(rows - 24, 2, replace=False), 70 + rng.choice(M - 70, 2, replace=False)])
        reads[q, pos] = (reads[q, pos] + 1 + rng.integers(0, 3, 4)) % 4
    return reads, wins


def _check(reads, wins, scheme):
    """full band against the narrow run of every class job -> (class, redone) per job"""
    P, go, ge = scheme
    mm = mismatches(reads, wins)
    U, best_d, cls = classes(mm.sum(axis=1), P, go, ge)
    want_s, want_c = full_band(mm, P, go, ge)
    redone = np.zeros(len(reads), dtype=bool)
    for c, half in ((2, HALF_A), (1, HALF_B)):
        sel = np.nonzero(cls == c)[0]
        if len(sel) == 0:
            continue
        s, col, re = narrow_band(mm[sel], P, go, ge, U[sel], half)
        redone[sel] = re
        ok = ~re
        assert (s[ok] == want_s[sel][ok]).all() and (col[ok] == want_c[sel][ok]).all(), (scheme, c, sel[ok][(s[ok] != want_s[sel][ok])][:5])
        assert (want_s[sel] >= U[sel]).all()                                      # L is a lower bound of the optimum
    return cls, redone


def test_reach_and_classes_of_the_default_scheme():
    assert [reach(L, -8, -3) for L in (-7, -8, -10, -11, -23, -24, -25, -26, -30, -31, -32)] == [0, 1, 1, 2, 6, 6, 6, 7, 8, 8, 9]
    cnt = np.full((6, BAND), 40)
    cnt[0, 15] = 4; cnt[1, 15] = 5; cnt[2, 15] = 6; cnt[3, 16] = 4; cnt[4, 18] = 4; cnt[5, 13:16] = 4
    U, best_d, cls = classes(cnt, 6, -8, -3)
    assert list(U) == [-24, -30, -36, -24, -24, -24] and list(best_d) == [15, 15, 15, 16, 18, 15]
    assert list(cls) == [2, 1, 0, 1, 0, 2]
    assert list(classes(cnt[:3], 6, -5, -1)[2]) == [0, 0, 0]                       # cheap gaps: r(-24) = 20, both classes come out empty


def test_narrow_run_equals_the_full_band_unless_redone():
    rng = np.random.default_rng(9)
    for si, scheme in enumerate(SCHEMES):
        reads, wins = _random_jobs(rng, 900, 150, (4, 5, 6))
        cls, redone = _check(reads, wins, scheme)
        if si == 0:
            k = np.arange(900) % 3
            assert (cls[k == 0] == 2).all() and (cls[k == 1] == 1).all() and (cls[k == 2] == 0).all()
            assert not redone.any()
    # shorter and longer reads, the default scheme; rows 23 / 24 / 25 are the switch
    for M in (25, 33, 96, 161):
        reads, wins = _random_jobs(rng, 120, M, (4, 5) if M > 33 else (1, 2))
        _check(reads, wins, SCHEMES[0])


def test_decoys_are_redone():
    rng = np.random.default_rng(10)
    for reads, wins in (decoy_outer(rng, 40), decoy_boundary(rng, 40)):
        cls, redone = _check(reads, wins, SCHEMES[0])
        assert (cls == 2).all() and redone.all()


def test_monitor_alone_on_exact_reads():
    """exact reads as class A: the centre diagonal holds 0 in every row, so column 21 holds open + 5 ext = -23 and sends
    E' = max(-23 + open, -23 + ext) = -26 into column 22, and column 9 holds -23 and sends max(Hg, F + ext) = -26 into column 8: the monitor
    alone refuses exactly the bounds L <= -26 (as does the qualification, which sees the same -26 in columns 8 and 22 at row 24)"""
    rng = np.random.default_rng(11)
    reads, wins = _random_jobs(rng, 20, 150, (0,))
    P, go, ge = SCHEMES[0]
    mm = mismatches(reads, wins)
    for L, want in ((-7, False), (-25, False), (-26, True), (-31, True)):
        for qualify in (False, True):
            s, col, redone = narrow_band(mm, P, go, ge, np.full(20, L), HALF_A, qualify)
            assert (redone == want).all(), (L, qualify, redone)
            assert (s == 0).all() and (col == 15).all()
