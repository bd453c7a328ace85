"""GPU parity of the full-matrix Gotoh traceback at the limits of its routes, with the route of every job read from
nvbio_full_gotoh_traceback_routes.

nvbio_full_gotoh_traceback sends a job down one of four paths (csrc/gotoh_full_traceback.hip): the diagonal through the sink without a DP,
the band-15 kernel with the full matrix's tie rule over a window of M + 14 symbols cut around the sink's diagonal, the full-matrix kernel over
the text rows within G diagonals of the sink's, and the same kernel over all rows.  Small integer rules choose: G = e2e_gap_bound(best, go_min,
ge_min) with the cuts G <= 7 and G <= 250, sink.y == M, best <= 0, sink.x >= sink.y, N >= M + 14 and 7 <= delta <= N - M - 7 for the band; the
row window [block + delta - G, block + 7 + delta + G] clamped to the text; the stripe arithmetic of 8 columns.  util.full_route_rule() restates
them; util.full_limit_jobs() builds jobs by construction at every value of each (tests/test_full_traceback_limit_jobs.py asserts on the CPU
that the batch holds them), under the schemes of util.LIMIT_SCHEMES and, for the last cut, (0,3,3,-1,-1,-1,-1).

Everything is compared with the CPU oracle (scores, sources, sinks, CIGAR lengths and rows, exactly, job by job); the route report with the
restated rule, job by job.  Every window lies inside one text with 64 symbols in front of the first and behind the last.

One departure from the issue's list, forced by the reference's own rule and asserted as such in test_min_scores: min_score is tested only
between stripes of 8 pattern columns, so a job whose best path still costs something in its last stripe is traced at best + 1 as well.

That the tests bite was tried with five edits of the rules on a scratch build, one MI355X run each, none committed, none faulted:
  * tb_band_route_kernel `code - 2u <= 7u` -> 8u: wrong scores and CIGARs against the oracle in test_modes (equal, cheap_pat, ramp; under
    cheap_txt, where no path is tight, in the report alone), test_min_scores, test_chunks and test_bounds;
  * `delta >= 7u` -> 6u and `delta + 7u <= N - M` -> `delta + 6u`: the window slides one symbol into the neighbouring text and every output
    stays right; the report shows route 3 where the rule says 2 in test_modes (the four admitted schemes), test_min_scores and test_chunks;
  * rows_of `- band_G` -> `- band_G + 1`: wrong scores and CIGARs for the jobs tight against G in test_modes (equal, cheap_pat, ramp: 513 to
    648 jobs each), test_min_scores, test_chunks and test_bounds; nothing under cheap_txt, where no traced gap reaches G;
  * `G <= 250` -> 251: every output right; the report shows (2, 251) for the reads of 251 symbols in test_modes[cut-*] and test_min_scores."""
import math

import numpy as np
import pytest

import oracle
from util import (ALN_NO_BAND_ROUTE, ALN_NO_NARROW_TRACEBACK, ALN_NO_UNGAPPED_TRACEBACK, FULL_LIMIT_CUT_SCHEME, LIMIT_SCHEMES, flat_scheme,
                  full_limit_jobs, full_limit_layout, full_limit_oracle, full_route_rule, limit_select, limit_thin)

pytestmark = pytest.mark.gpu

SEED = 20262
STRIDE = 16
SG, LOCAL, GLOBAL = oracle.SEMI_GLOBAL, oracle.LOCAL, oracle.GLOBAL
ONES = 0xFFFFFFFF
SCHEMES = LIMIT_SCHEMES + (FULL_LIMIT_CUT_SCHEME,)


# ---- batches --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool(orc):
    """per scheme the jobs it runs (the generator's `cut` jobs under their own scheme, all the others under each of LIMIT_SCHEMES), their
    reverse / complement flags, the oracle's results and the rule's routes"""
    J = full_limit_jobs(SEED)
    flags = np.random.default_rng(SEED + 1).integers(0, 4, len(J["pats"]))
    P = dict(J={}, flags={}, want={}, rule={})
    for name, sv, with_q in SCHEMES:
        idx = np.nonzero((J["kind"] == "cut") == (name == "cut"))[0]
        P["J"][name], P["flags"][name] = limit_select(J, idx), flags[idx]
        P["want"][name] = full_limit_oracle(orc, SG, sv, P["J"][name], with_q, STRIDE)
        P["rule"][name] = full_route_rule(P["J"][name], with_q, SG, sv, P["want"][name])
    return P


def _bounds(S):
    return max(len(p) for p in S["pats"]), max(len(t) for t in S["txts"])


def _gpu(amd, orc, typ, sv, L, bounds, algo=0, read_bits=4, text_bits=2, temp=None, report=True, min_scores=None, given=False, stride=STRIDE):
    """one run of the entry point with the report (or the plain one) -> (scores, sources, sinks, cigars, lens), routes, gap_bound"""
    reads = {4: orc.pack4, 2: orc.pack2, 8: lambda v: v}[read_bits](L["reads"])
    text = orc.pack2(L["text"]) if text_bits == 2 else L["text"]
    batch = amd.AlignmentBatch(reads, read_bits, L["roffs"], text, text_bits, L["wb"], L["we"], quals=L["quals"], flags=L["flags"], algo_flags=algo)
    al = amd.make_gotoh_aligner(typ, amd.GotohScheme(*sv))
    kw = dict(min_scores=min_scores, cigar_stride=stride, temp=temp)
    if given:
        kw["scores"], kw["sinks"] = amd.BatchedAlignmentScore(al, text_blocking=False).enact(batch, bounds[0], bounds[1], min_scores=min_scores)
    if report:
        sc, src, snk, cig, ln, rt, gb = amd.full_gotoh_traceback_routes(al, batch, bounds[0], bounds[1], **kw)
        rt, gb = rt.cpu().numpy(), gb.cpu().numpy()
    else:
        sc, src, snk, cig, ln = amd.BatchedAlignmentTraceback(al).enact(batch, bounds[0], bounds[1], **kw)
        rt = gb = None
    return (sc.cpu().numpy(), amd.u32(src), amd.u32(snk), cig.cpu().numpy().view(np.uint16), amd.u32(ln)), rt, gb


def _check(got, want, what):
    bad = np.zeros(len(want[0]), dtype=bool)
    for g, w in zip(got, want):
        d = g != w
        bad |= d if d.ndim == 1 else d.any(axis=1)
    bad = np.nonzero(bad)[0]
    assert len(bad) == 0, (what, len(bad), bad[:6], [(int(got[0][j]), int(want[0][j]), got[3][j, :6].tolist(), want[3][j, :6].tolist()) for j in bad[:3]])


def _check_routes(rt, gb, rule, what):
    bad = np.nonzero((rt != rule[0]) | (gb != rule[1]))[0]
    assert len(bad) == 0, (what, len(bad), bad[:6], rt[bad[:6]], rule[0][bad[:6]], gb[bad[:6]], rule[1][bad[:6]])


def _subset(P, name, with_q, idx):
    """a batch of the jobs `idx` of a scheme's pool -> (jobs, layout, the oracle's results and the rule's routes for them)"""
    S = limit_select(P["J"][name], idx)
    return S, full_limit_layout(S, with_q, P["flags"][name][idx]), tuple(w[idx] for w in P["want"][name]), tuple(r[idx] for r in P["rule"][name])


# ---- tests ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("read_bits", [4, 2])
@pytest.mark.parametrize("scheme", SCHEMES, ids=lambda s: s[0])
def test_modes(amd, orc, pool, scheme, read_bits):
    """every job of the generator under one scheme, end to end, reads reversed / complemented at random, qualities where the scheme has a
    ramp: default, the DP over all rows for every job, no restricted rows, no band route; 4-bit reads and (the jobs without an N) 2-bit
    reads.  All equal the oracle; the report equals the restated rule: (1, 0) throughout with the shortcut off, never 2 or 3 without the narrow
    routes or under the scheme they refuse, never 3 without the band route.  The entry point without a report gives the same outputs; so does
    a run handed the scores and sinks of the scoring pass; so does a thinned subset as 8-bit reads on 8-bit text."""
    name, sv, with_q = scheme
    J = pool["J"][name]
    idx = np.arange(len(J["pats"])) if read_bits == 4 else np.nonzero(J["fill"] != 4)[0]
    S, L, want, rule = _subset(pool, name, with_q, idx)
    bounds = _bounds(S)
    assert (amd.ALN_NO_UNGAPPED_TRACEBACK, amd.ALN_NO_NARROW_TRACEBACK, amd.ALN_NO_BAND_ROUTE) == (ALN_NO_UNGAPPED_TRACEBACK, ALN_NO_NARROW_TRACEBACK, ALN_NO_BAND_ROUTE)
    for algo in (0, ALN_NO_UNGAPPED_TRACEBACK, ALN_NO_NARROW_TRACEBACK, ALN_NO_BAND_ROUTE):
        exp = rule if algo == 0 else full_route_rule(S, with_q, SG, sv, want, algo)
        if algo == ALN_NO_UNGAPPED_TRACEBACK:
            assert (exp[0] == 1).all() and not exp[1].any()
        if algo == ALN_NO_NARROW_TRACEBACK or name == "refused":
            assert exp[0].max() == 1 and not exp[1].any()
        if algo == ALN_NO_BAND_ROUTE and name != "refused":
            assert exp[0].max() == 2 and np.array_equal(exp[1], rule[1])
        got, rt, gb = _gpu(amd, orc, SG, sv, L, bounds, algo, read_bits)
        _check(got, want, (name, read_bits, algo))
        _check_routes(rt, gb, exp, (name, read_bits, algo))
    plain, _, _ = _gpu(amd, orc, SG, sv, L, bounds, 0, read_bits, report=False)
    _check(plain, want, (name, read_bits, "no report"))
    got, rt, gb = _gpu(amd, orc, SG, sv, L, bounds, 0, read_bits, given=True)
    _check(got, want, (name, read_bits, "scores and sinks given"))
    _check_routes(rt, gb, rule, (name, read_bits, "scores and sinks given"))
    if read_bits == 4:
        thin = limit_thin(J)
        S, L, want, rule = _subset(pool, name, with_q, thin)
        got, rt, gb = _gpu(amd, orc, SG, sv, L, _bounds(S), 0, 8, 8)
        _check(got, want, (name, "8-bit"))
        _check_routes(rt, gb, rule, (name, "8-bit"))


def test_types(amd, orc, pool):
    """a thinned round under LOCAL (a scheme with a match bonus) and GLOBAL: neither reports route 2 or 3; every traced GLOBAL job takes the
    DP over all rows; a traced LOCAL job is settled where the smallest diagonal suffix that scores `best` ends in its sink (or best == 0),
    and takes the DP otherwise"""
    J = pool["J"]["equal"]
    idx = limit_thin(J)
    S = limit_select(J, idx)
    bounds = _bounds(S)
    for typ, (name, sv, with_q) in ((LOCAL, LIMIT_SCHEMES[4]), (GLOBAL, LIMIT_SCHEMES[0]), (GLOBAL, LIMIT_SCHEMES[3])):
        L = full_limit_layout(S, with_q, pool["flags"]["equal"][idx])
        want = full_limit_oracle(orc, typ, sv, S, with_q, STRIDE)
        rule = full_route_rule(S, with_q, typ, sv, want)
        assert rule[0].max() == 1 and not rule[1].any()
        if typ == GLOBAL:
            assert (want[4] > 0).all() and (rule[0] == 1).all()
        else:
            assert sv[0] > 0 and (rule[0][want[4] > 0] == 0).sum() >= 100 and (rule[0] == 1).sum() >= 50
        for algo in (0, ALN_NO_UNGAPPED_TRACEBACK):
            got, rt, gb = _gpu(amd, orc, typ, sv, L, bounds, algo)
            _check(got, want, (typ, name, algo))
            _check_routes(rt, gb, rule if algo == 0 else (np.ones_like(rule[0]), rule[1]), (typ, name, algo))


def test_min_scores(amd, orc, pool):
    """a per-job min_scores equal to the oracle's best traces the job, on every route; one more and the job reports nothing: score
    SCORE_MIN, sink and source all ones, length 0, route 0 -- wherever the reference's own rule drops it.  The reference (and the oracle, and
    the scoring pass) test min_score only between stripes of 8 pattern columns, against the best score of the stripe's last column: a job
    whose best path still costs something in its last stripe is traced at best + 1 as well.  Both kinds are picked on purpose, on every
    route; the reads of the last cut, all insertions, cost 1 in every column and are dropped from best + 9 on, so their limit is best + 16.
    Both halves run in one call, alternating, and are compared with the oracle called with the same min_score"""
    for (name, sv, with_q), codes, step in ((LIMIT_SCHEMES[0], (0, 2, 3), 1), (FULL_LIMIT_CUT_SCHEME, (1, 2), 16)):
        J, rt_all, best = pool["J"][name], pool["rule"][name][0], pool["want"][name][0].astype(np.int64)
        drops = full_limit_oracle(orc, SG, sv, J, with_q, STRIDE, min_scores=best + step)[4] == 0
        rng = np.random.default_rng(SEED + 5)
        idx = np.concatenate([rng.permutation(np.nonzero((rt_all == c) & (drops == d))[0])[:count] for c in codes for d, count in ((True, 30), (False, 10))])
        idx = np.stack([idx, rng.permutation(idx)], axis=1).reshape(-1)          # every job picked once for either half, at random
        S, L, want, rule = _subset(pool, name, with_q, idx)
        above = np.arange(len(idx)) % 2 == 1
        ms = (want[0].astype(np.int64) + step * above).astype(np.int32)
        exp = full_limit_oracle(orc, SG, sv, S, with_q, STRIDE, min_scores=ms)
        dropped = above & drops[idx]
        for k in range(5):
            assert np.array_equal(exp[k][~dropped], want[k][~dropped])
        assert (exp[0][dropped] == oracle.SCORE_MIN).all() and (exp[1][dropped] == ONES).all() and (exp[2][dropped] == ONES).all() and not exp[4][dropped].any()
        assert all((dropped & (rule[0] == c)).sum() >= 4 and (~above & (rule[0] == c)).sum() >= 4 for c in codes)
        if name != "cut":
            assert all((above & ~dropped & (rule[0] == c)).sum() >= 4 for c in codes)
        exp_rule = (np.where(dropped, 0, rule[0]), np.where(dropped, 0, rule[1]))
        for given in (False, True):
            got, rt, gb = _gpu(amd, orc, SG, sv, L, _bounds(S), min_scores=ms, given=given)
            _check(got, exp, (name, given))
            _check_routes(rt, gb, exp_rule, (name, given))


@pytest.mark.parametrize("side", [0, 1], ids=["last_in_chunk", "first_of_next"])
def test_chunks(amd, orc, pool, side):
    """a caller's temp for exactly 64 full-matrix jobs: batches whose full-matrix job list is 64 | 65 long and whose band list is cap | cap + 1
    long, cap = the band-15 jobs that temp holds (both counted in the route report), one job either side of a chunk boundary of each, give
    what the un-chunked run and the oracle give.  A temp one byte short of 64 jobs is refused"""
    import torch
    name, sv, with_q = LIMIT_SCHEMES[0]
    J, rt_all = pool["J"][name], pool["rule"][name][0]
    max_m, max_n = _bounds(J)
    per_job = max_n * 4 * (1 + math.ceil(max_m / 8))
    cap = 64 * per_job // (max_m * 8)
    rng = np.random.default_rng(SEED + 2 + side)
    band = rng.permutation(np.nonzero(rt_all == 3)[0])
    band = np.concatenate([band] * (-(-(cap + 1) // len(band))))[:cap + side]               # (repeated where the pool has fewer)
    idx = rng.permutation(np.concatenate([rng.permutation(np.nonzero((rt_all == 1) | (rt_all == 2))[0])[:64 + side], band,
                                          rng.permutation(np.nonzero(rt_all == 0)[0])[:50]]))
    S, L, want, rule = _subset(pool, name, with_q, idx)
    temp = torch.empty(64 * per_job, dtype=torch.uint8, device="cuda:0")
    whole, rt0, gb0 = _gpu(amd, orc, SG, sv, L, (max_m, max_n))
    got, rt1, gb1 = _gpu(amd, orc, SG, sv, L, (max_m, max_n), temp=temp)
    assert (((rt1 == 1) | (rt1 == 2)).sum(), (rt1 == 3).sum(), (rt1 == 0).sum()) == (64 + side, cap + side, 50)
    _check_routes(rt1, gb1, rule, side)
    _check_routes(rt0, gb0, rule, side)
    _check(got, whole, ("chunked", side))
    _check(got, want, ("oracle", side))
    plain, _, _ = _gpu(amd, orc, SG, sv, L, (max_m, max_n), temp=temp, report=False)
    _check(plain, want, ("chunked, no report", side))
    with pytest.raises(amd.NvbioError):
        _gpu(amd, orc, SG, sv, L, (max_m, max_n), temp=temp[:64 * per_job - 1])


def test_bounds(amd, orc, pool):
    """the declared bounds: a job with M == max_pattern_len and N == max_text_len is traced; the same batch declared one symbol shorter on
    either side skips that job (length 0xFFFFFFFF, source all ones, route 0) and traces the rest.  The int16 admission (max_pattern_len +
    max_text_len + 1) * max_step <= 30000 accepts the largest bounds that satisfy it and refuses the next; at the accepted bound one job of
    all mismatches equals the oracle, with the shortcut and over all rows"""
    name, sv, with_q = LIMIT_SCHEMES[0]
    J = pool["J"][name]
    idx = np.concatenate([np.nonzero(J["M"] == 65)[0][::4], np.nonzero(J["M"] == 33)[0][::8]])
    S, L, want, rule = _subset(pool, name, with_q, idx)
    max_m, max_n = _bounds(S)
    assert (max_m, max_n) == (65, 87) and ((L["M"] == 65) & (L["N"] == 87) & (rule[0] >= 2)).sum() >= 10 and ((L["M"] == 65) & (L["N"] == 80)).sum() >= 4
    got, rt, gb = _gpu(amd, orc, SG, sv, L, (max_m, max_n))
    _check(got, want, "at the bounds")
    _check_routes(rt, gb, rule, "at the bounds")
    for bounds in ((max_m - 1, max_n), (max_m, max_n - 1)):
        over = (L["M"] > bounds[0]) | (L["N"] > bounds[1])
        assert 10 <= over.sum() <= len(idx) - 10
        for algo in (0, ALN_NO_UNGAPPED_TRACEBACK):
            got, rt, gb = _gpu(amd, orc, SG, sv, L, bounds, algo)
            assert (got[4][over] == ONES).all() and (got[1][over] == ONES).all(), (bounds, algo)
            _check(tuple(g[~over] for g in got), tuple(w[~over] for w in want), (bounds, algo))
            if algo == 0:
                _check_routes(rt, gb, (np.where(over, 0, rule[0]), np.where(over, 0, rule[1])), bounds)
    # the int16 admission: a step of 40 admits 750 cells = 64 + 685 + 1
    fv = flat_scheme(0, 40)
    pat = np.zeros(64, dtype=np.uint8)
    txt = np.random.default_rng(SEED + 3).integers(1, 4, 685, dtype=np.uint8)
    A = dict(pats=[pat], txts=[txt], quals=[np.zeros(64, dtype=np.uint8)])
    LA = full_limit_layout(A, False)
    stride = 160
    want = full_limit_oracle(orc, SG, fv, A, False, stride)
    rule = full_route_rule(A, False, SG, fv, want)
    assert 30000 // 40 == 64 + 685 + 1 and want[0][0] == -64 * 40 and want[4][0] <= stride
    for algo in (0, ALN_NO_UNGAPPED_TRACEBACK, ALN_NO_BAND_ROUTE):
        got, rt, gb = _gpu(amd, orc, SG, fv, LA, (64, 685), algo, stride=stride)
        _check(got, want, ("all mismatches", algo))
        _check_routes(rt, gb, rule if algo == 0 else full_route_rule(A, False, SG, fv, want, algo), ("all mismatches", algo))
    for bounds in ((64, 686), (65, 685)):
        with pytest.raises(amd.NvbioError):
            _gpu(amd, orc, SG, fv, LA, bounds, stride=stride)
