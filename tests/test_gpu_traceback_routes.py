"""GPU parity of the banded traceback at the limits of its routes, with the route of every job read from nvbio_banded_gotoh_traceback_routes.

nvbio_banded_gotoh_traceback sends a job down one of five paths (csrc/gotoh_traceback.hip): the ungapped shortcut, scoring the sink's diagonal
by a popcount over bit planes or symbol by symbol, and the direction-vector DP over the full band, over 15 columns or over 7, the narrow bands
at a per-job column offset band_off.  Small integer rules choose: G = e2e_gap_bound(best, go_min, ge_min) with the cuts G <= 3 and G <= 7, the
clamps of band_off (entry - 3 < 24, entry - 7 < 16), the window condition N >= M + 30, sink.y == M, M <= 161 and entry + M <= N for the plane
count, a constant mismatch penalty.  _route_rule() below restates them; util.limit_jobs() builds jobs by construction at every value of each
(every sink diagonal 0..30 x every gap length 1..8 in both directions, with a substitution, split in two; windows of M + 31 | 30 | 29; reads
of 33, 64, 160, 161 | 162 symbols; overhangs past a clipped window's end), under the schemes of util.LIMIT_SCHEMES.

Everything is compared with the oracle (scores, sources, sinks, CIGAR lengths and rows, exactly); the route report with the restated rule, job
by job.  test_reach asserts, on the oracle's output alone, that the batches hold what they are built for -- it needs no GPU result and was
satisfied on the CPU before the first GPU run.

Two departures from the issue's list, both forced by the reference's own rules and asserted as such below:
  * a traced gap can equal G only in a path with ONE gap: two gaps pay two opening penalties, which makes G >= L + 1 under every scheme here;
    so the tight bound is asserted for the kinds del, ins, del+sub and ins+sub, not for split;
  * an overhang of k symbols on diagonal e leaves a window of e + M - k symbols, shorter than the read at e = 0: nothing is reported there.
    The lowest diagonal that holds such a job is e = k, which is added.  An end-to-end sink never lies past the text's end (only columns
    whose last cell is inside the text are searched), so the overhang jobs run LOCAL (sinks past the end, on the sentinel read as 3) and GLOBAL
    (the sink is the band's last cell, column 30, where the sentinel is read as 255 and matches nothing).

That the tests bite was tried with five edits of the rules on a scratch build, one MI355X run each, none committed: G <= 3 -> 4, the band-7 clamp
24 -> 23 and the band-15 offset entry - 7 -> 6 give wrong CIGARs (test_modes and test_chunks, against the oracle and in the report);
N >= M + 30 -> 29 and the shortcut's column-30 compare switched off leave every output right and show in the route report alone (test_modes,
test_chunks, test_overhang)."""
import numpy as np
import pytest

import oracle
from util import LIMIT_GAP_KINDS, LIMIT_SCHEMES, full_layout, limit_jobs, limit_select

pytestmark = pytest.mark.gpu

SEED = 20261
STRIDE = 16
MAX_READ_LEN = 162
SG, LOCAL, GLOBAL = oracle.SEMI_GLOBAL, oracle.LOCAL, oracle.GLOBAL
NO_UNGAPPED, NO_NARROW = 16, 64                                         # NVBIO_ALN_NO_UNGAPPED_TRACEBACK, NVBIO_ALN_NO_NARROW_TRACEBACK


# ---- the rule, restated ---------------------------------------------------------------------------------------------------------------
def _gap_mins(sv):
    """the cheapest gap opening / extension penalty of a scheme"""
    return -max(sv[3], sv[5]), -max(sv[4], sv[6])


def _gap_bound(a, sv):
    go, ge = _gap_mins(sv)
    return 0 if a < go else (a - go) // ge + 1


def _reachable(sv, with_q):
    """the costs the generator's gapped paths can have: one gap of 1..8 symbols, alone, with a substitution or beside a second gap.  The banded
    aligner charges pat_gap_* for either gap kind (txt_gap_* only initialise GLOBAL's first row)"""
    gap = [-(sv[3] + (k - 1) * sv[4]) for k in range(1, 9)]
    mm = range(sv[1], sv[2] + 1) if with_q else (sv[1],)
    return sorted(set(gap) | {g + m for g in gap for m in mm} | {gap[a] + gap[b] for a in range(8) for b in range(8) if a + b + 2 <= 8})


def _narrow_scheme(typ, sv):
    go, ge = _gap_mins(sv)
    return typ == SG and sv[0] == 0 and sv[1] >= 0 and sv[2] >= 0 and ge > 0 and go >= ge


def _diagonal_reaches(pat, q, txt, typ, sv, best, sink, col30=255):
    """does the diagonal that ends in `sink` score `best`?  A symbol past the text's end is the sentinel 255, which columns below 30 read as 3
    and column 30 as `col30`"""
    M, N = len(pat), len(txt)
    x, y = int(sink[0]), int(sink[1])
    entry = x - y
    p = pat[:y].astype(np.int64)
    ti = np.arange(y) + entry
    g = np.where(ti < N, txt[np.minimum(ti, N - 1)], 255 if entry < 30 else col30).astype(np.int64)
    eq = (g == p) if entry == 30 and col30 == 255 else (p < 4) & ((g & 3) == p)
    qq = np.minimum(q[:y].astype(np.int64), 40) if q is not None else np.zeros(y, dtype=np.int64)
    mm = sv[1] + (qq.astype(np.float32) / np.float32(40) * np.float32(sv[2] - sv[1])).astype(np.int64)
    step = np.where(eq, sv[0], -mm)
    if typ == LOCAL:
        return best == 0 or bool((np.cumsum(step[::-1]) == best).any())
    h0 = sv[5] + (entry - 1) * sv[6] if typ == GLOBAL and entry > 0 else 0
    return h0 + int(step.sum()) == best


def _route_rule(J, with_q, typ, sv, want, algo=0, col30=255):
    """(route, band_off) of every job: 0 where nothing is traced or the sink's diagonal reaches the score, else 1, or under an admitted scheme
    with the sink in the last row, a window of M + 30 or more and G from the score: 3 at G <= 3 (band_off = entry - 3 in 0..24), 2 at G <= 7
    (entry - 7 in 0..16)"""
    n = len(J["pats"])
    routes, offs = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    if algo & NO_UNGAPPED:
        return routes + 1, offs
    sc, sk = want[0], want[2].astype(np.int64)
    for j in range(n):
        M, N = len(J["pats"][j]), len(J["txts"][j])
        if want[4][j] == 0 or _diagonal_reaches(J["pats"][j], J["quals"][j] if with_q else None, J["txts"][j], typ, sv, int(sc[j]), sk[j], col30):
            continue
        routes[j] = 1
        entry = int(sk[j, 0] - sk[j, 1])
        if _narrow_scheme(typ, sv) and not algo & NO_NARROW and sk[j, 1] == M and N >= M + 30 and sc[j] <= 0:
            G = _gap_bound(-int(sc[j]), sv)
            if G <= 3:
                routes[j], offs[j] = 3, min(max(entry - 3, 0), 24)
            elif G <= 7:
                routes[j], offs[j] = 2, min(max(entry - 7, 0), 16)
    return routes, offs


def _traced_gap(cig, ln):
    """gap symbols in a CIGAR row"""
    els = cig[:min(int(ln), STRIDE)].astype(np.int64)
    return int((els >> 2)[((els & 3) == 1) | ((els & 3) == 2)].sum())


# ---- batches --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool(orc):
    """the generator's jobs, their layout with and without qualities, and per scheme the oracle's results and the rule's routes"""
    J = limit_jobs(SEED)
    flags = np.random.default_rng(SEED + 1).integers(0, 4, len(J["pats"]))
    P = dict(J=J, flags=flags, L={q: full_layout(J["pats"], J["txts"], J["quals"] if q else None, flags) for q in (False, True)}, want={}, rule={})
    for name, sv, with_q in LIMIT_SCHEMES:
        P["want"][name] = _oracle(orc, SG, sv, P["L"][with_q])
        P["rule"][name] = _route_rule(J, with_q, SG, sv, P["want"][name])
    return P


def _oracle(orc, typ, sv, L):
    return orc.banded_gotoh_traceback_packed_batch(31, typ, oracle.Scheme(*sv), orc.pack4(L["reads"]), L["roffs"], orc.pack2(L["text"]), L["wb"], L["we"],
                                                   STRIDE, flags=L["flags"], quals=L["quals"])


def _gpu(amd, orc, typ, sv, L, algo=0, read_bits=4, planes=False, temp=None, report=True):
    text2 = orc.pack2(L["text"])
    tp = amd.build_text_planes(text2, len(L["text"])) if planes else None
    reads = orc.pack4(L["reads"]) if read_bits == 4 else orc.pack2(L["reads"])
    batch = amd.AlignmentBatch(reads, read_bits, L["roffs"], text2, 2, L["wb"], L["we"], quals=L["quals"], flags=L["flags"], max_read_len=MAX_READ_LEN,
                               algo_flags=algo, text_planes=tp)
    al = amd.make_gotoh_aligner(typ, amd.GotohScheme(*sv))
    if report:
        sc, src, snk, cig, ln, rt, off = amd.banded_gotoh_traceback_routes(31, al, batch, cigar_stride=STRIDE, temp=temp)
        rt, off = rt.cpu().numpy(), off.cpu().numpy()
    else:
        sc, src, snk, cig, ln = amd.BatchedBandedAlignmentTraceback(31, al).enact(batch, cigar_stride=STRIDE, temp=temp)
        rt = off = None
    return (sc.cpu().numpy(), amd.u32(src), amd.u32(snk), cig.cpu().numpy().view(np.uint16), amd.u32(ln)), rt, off


def _check(got, want, what):
    bad = np.zeros(len(want[0]), dtype=bool)
    for g, w in zip(got, want):
        d = g != w
        bad |= d if d.ndim == 1 else d.any(axis=1)
    bad = np.nonzero(bad)[0]
    assert len(bad) == 0, (what, len(bad), bad[:6], [(int(got[0][j]), int(want[0][j]), got[3][j, :6].tolist(), want[3][j, :6].tolist()) for j in bad[:3]])


def _check_routes(rt, off, rule, what):
    bad = np.nonzero((rt != rule[0]) | (off != rule[1]))[0]
    assert len(bad) == 0, (what, len(bad), bad[:6], rt[bad[:6]], rule[0][bad[:6]], off[bad[:6]], rule[1][bad[:6]])


def _subset(P, name, with_q, idx):
    """a batch of the pool's jobs `idx` -> (layout, the oracle's results and the rule's routes for them)"""
    S = limit_select(P["J"], idx)
    L = full_layout(S["pats"], S["txts"], S["quals"] if with_q else None, P["flags"][idx])
    return L, tuple(w[idx] for w in P["want"][name]), tuple(r[idx] for r in P["rule"][name])


NARROW = [s for s in LIMIT_SCHEMES if s[0] != "refused"]


# ---- tests ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", NARROW, ids=lambda s: s[0])
def test_reach(pool, scheme):
    """conditions on the batches, from the oracle's output and the restated rule alone.  With a = -best of the jobs that reach the DP in a
    window the narrow routes admit: jobs at a = go_min + 3 ge_min - 1 and one more (the cut G <= 3 | 4: 16 | 17 under (0,6,6,-8,-3,-8,-3)) and
    at go_min + 7 ge_min - 1 and one more (G <= 7 | 8: 28 | 29); band_off at 0, at its clamp (24 for band 7, 16 for band 15) and strictly
    between, for both bands, with the sink's diagonal on either side of each clamp (3 | 4 and 26 | 27 | 28, 7 | 8 and 22 | 23 | 24); per
    one-gap kind a narrow job whose traced gap equals G (with a substitution only a quality ramp leaves room: 3 L + 7 gives G = L); jobs the
    shortcut settles, windows of M + 29 that the narrow routes refuse next to M + 30 that they take, reads of 161 | 162 symbols settled"""
    name, sv, with_q = scheme
    J, want, (rt, off) = pool["J"], pool["want"][name], pool["rule"][name]
    go, ge = _gap_mins(sv)
    a = -want[0].astype(np.int64)
    entry = want[2][:, 0].astype(np.int64) - want[2][:, 1].astype(np.int64)
    dp = (rt > 0) & (J["win"] >= 30)
    sums = _reachable(sv, with_q)
    for cut, below, above in ((go + 3 * ge - 1, 3, 2), (go + 7 * ge - 1, 2, 1)):
        lo, hi = max(v for v in sums if v <= cut), min(v for v in sums if v > cut)
        assert (rt[dp & (a <= cut)] >= below).all() and (rt[dp & (a > cut)] <= above).all()
        assert (dp & (a == lo) & (rt == below)).sum() >= 4 and (dp & (a == hi) & (rt == above)).sum() >= 4, (name, cut, lo, hi)
        if name in ("equal", "ramp"):
            assert (lo, hi) == (cut, cut + 1) and cut in (16, 28)
    for code, reach, clamp in ((3, 3, 24), (2, 7, 16)):
        o, en = off[rt == code], entry[rt == code]
        assert (o == 0).any() and (o == clamp).any() and ((o > 0) & (o < clamp)).any()
        for v in (reach, reach + 1, clamp + reach - 1, clamp + reach, clamp + reach + 1, 0, 30):
            assert (en == v).any(), (name, code, v)
    gaps = np.array([_traced_gap(want[3][j], want[4][j]) for j in range(len(a))])
    G = np.array([_gap_bound(int(v), sv) for v in a])
    for kind in LIMIT_GAP_KINDS:
        tight = (J["kind"] == kind) & (rt >= 2) & (gaps == G)
        if kind == "split" or (kind.endswith("+sub") and not with_q) or name == "cheap_txt":
            assert ((J["kind"] == kind) & (rt >= 2)).any()                  # (not tight as built, see above)
        else:
            assert (tight & (rt == 3)).any() and (tight & (rt == 2)).any(), (name, kind)
    assert (rt[(J["win"] == 29) & (J["kind"] != "overhang")] < 2).all() and (rt[J["win"] == 29] == 1).sum() >= 100
    assert (rt[J["win"] == 30] >= 2).sum() >= 20
    for M in (161, 162):
        assert ((rt == 0) & (J["M"] == M) & (J["kind"] == "ungapped")).sum() >= 100 and ((rt >= 2) & (J["M"] == M)).sum() >= 20
    assert (J["M"] == 33).sum() >= 100 and ((J["M"] == 33) & (J["L"] == 8) & (rt == 1)).any()


def test_reach_refused_scheme(pool):
    """under a match bonus the narrow routes take nothing; the batch still holds settled and DP jobs"""
    rt, off = pool["rule"]["refused"]
    assert set(np.unique(rt)) == {0, 1} and not off.any() and (rt == 0).sum() >= 300 and (rt == 1).sum() >= 2000


@pytest.mark.parametrize("read_bits", [4, 2])
@pytest.mark.parametrize("scheme", LIMIT_SCHEMES, ids=lambda s: s[0])
def test_modes(amd, orc, pool, scheme, read_bits):
    """every job of the generator under one scheme, end to end: default, the DP for every job, every DP over the full band, each with the
    text as packed words and as bit planes; 4-bit reads and (the jobs without an N) 2-bit reads.  All equal the oracle; the report equals the
    restated rule: all 1 with the shortcut off, never 2 or 3 without the narrow routes or under the scheme they refuse.  The entry point
    without a report gives the same outputs."""
    name, sv, with_q = scheme
    J = pool["J"]
    idx = np.arange(len(J["pats"])) if read_bits == 4 else np.nonzero(J["fill"] != 4)[0]
    L, want, rule = _subset(pool, name, with_q, idx)
    assert amd.ALN_NO_UNGAPPED_TRACEBACK == NO_UNGAPPED and amd.ALN_NO_NARROW_TRACEBACK == NO_NARROW
    for algo in (0, NO_UNGAPPED, NO_NARROW):
        exp = rule if algo == 0 else _route_rule(limit_select(J, idx), with_q, SG, sv, want, algo)
        if algo == NO_UNGAPPED:
            assert (exp[0] == 1).all() and not exp[1].any()
        if algo == NO_NARROW or name == "refused":
            assert exp[0].max() == 1 and not exp[1].any()
        for planes in (False, True):
            got, rt, off = _gpu(amd, orc, SG, sv, L, algo, read_bits, planes)
            _check(got, want, (name, read_bits, algo, planes))
            _check_routes(rt, off, exp, (name, read_bits, algo, planes))
    plain, _, _ = _gpu(amd, orc, SG, sv, L, 0, read_bits, report=False)
    _check(plain, want, (name, read_bits, "no report"))


@pytest.mark.parametrize("side", [0, 1], ids=["last_in_chunk", "first_of_next"])
def test_chunks(amd, orc, pool, side):
    """a caller's temp for exactly 64 full-band jobs holds 128 band-15 jobs: batches whose job lists are 64 | 65 long for the full band and
    128 | 129 for band 15 (counted in the route report), one job either side of a chunk boundary, give what the un-chunked run and the oracle give"""
    import torch
    name, sv, with_q = LIMIT_SCHEMES[0]
    rt = pool["rule"][name][0]
    rng = np.random.default_rng(SEED + 2 + side)
    idx = np.concatenate([rng.permutation(np.nonzero(rt == code)[0])[:count] for code, count in ((1, 64 + side), (2, 128 + side), (3, 70), (0, 50))])
    idx = rng.permutation(idx)
    L, want, rule = _subset(pool, name, with_q, idx)
    temp = torch.empty(64 * MAX_READ_LEN * 16, dtype=torch.uint8, device="cuda:0")
    whole, rt0, off0 = _gpu(amd, orc, SG, sv, L)
    got, rt1, off1 = _gpu(amd, orc, SG, sv, L, temp=temp)
    assert ((rt1 == 1).sum(), (rt1 == 2).sum(), (rt1 == 3).sum()) == (64 + side, 128 + side, 70)
    _check_routes(rt1, off1, rule, side)
    _check_routes(rt0, off0, rule, side)
    _check(got, whole, ("chunked", side))
    _check(got, want, ("oracle", side))


def test_overhang(amd, orc, pool):
    """reads that run k = 1..5 symbols past the end of a clipped window.  LOCAL (match 1): where the overhang is all 3 the alignment runs on
    over the sentinel on every diagonal below 30 -- the shortcut settles such a job (route 0, one CIGAR element, no clip behind it) with a sink
    past the text's end, at e = k, 15 and 29 -- and stops at the text's end on diagonal 30 and wherever the overhang is 0 or N.  GLOBAL: the
    sink is column 30, where the sentinel matches nothing; the shortcut settles the diagonal-30 jobs with their overhang charged as mismatches,
    and would not if column 30 read the sentinel as 3 -- jobs whose route turns on that alone are asserted present.  End to end the jobs are
    ordinary (no sink past the end); at e = 0 the window is shorter than the read and nothing is reported, under every type."""
    J = pool["J"]
    idx = np.nonzero(J["kind"] == "overhang")[0]
    S = limit_select(J, idx)
    e, k, fill = S["e"], S["L"], S["fill"]
    N = np.array([len(t) for t in S["txts"]])
    for typ, (name, sv, with_q) in ((LOCAL, LIMIT_SCHEMES[4]), (GLOBAL, LIMIT_SCHEMES[0]), (GLOBAL, LIMIT_SCHEMES[3]), (SG, LIMIT_SCHEMES[0])):
        L = full_layout(S["pats"], S["txts"], S["quals"] if with_q else None, pool["flags"][idx])
        want = _oracle(orc, typ, sv, L)
        rule = _route_rule(S, with_q, typ, sv, want)
        assert (want[4][e == 0] == 0).all() and (want[0][e == 0] == oracle.SCORE_MIN).all() and (want[4][e > 0] > 0).all()
        if typ == LOCAL:
            past = (want[2][:, 0] > N) & (want[4] > 0)                           # the sink lies past the text's end
            settled = past & (rule[0] == 0) & (want[2][:, 1] == 64) & ((((want[3] & 3) != 3) & (want[3] > 0)).sum(axis=1) == 1)
            for d in (1, 2, 3, 4, 5, 15, 29):
                assert (settled & (e == d) & (fill == 3)).any(), d
            assert not past[(e == 30) | (fill != 3)].any() and (want[2][(e == 30), 1] == 64 - k[e == 30]).all()
        if typ == GLOBAL:
            as3 = _route_rule(S, with_q, typ, sv, want, col30=3)
            turns = (rule[0] == 0) & (as3[0] == 1)
            # (k mismatches on the diagonal against two gap openings and one: at small k the diagonal is the optimum)
            assert turns[(e == 30) & (fill == 3) & (k == 1)].all() and turns.sum() >= 2 and np.array_equal(turns, rule[0] != as3[0])
            assert not turns[(e != 30) | (fill != 3)].any()
        for planes in (False, True):
            got, rt, off = _gpu(amd, orc, typ, sv, L, planes=planes)
            _check(got, want, (typ, name, planes))
            _check_routes(rt, off, rule, (typ, name, planes))
        got, rt, off = _gpu(amd, orc, typ, sv, L, NO_UNGAPPED)
        _check(got, want, (typ, name, "dp"))
        assert (rt == 1).all() and not off.any()
