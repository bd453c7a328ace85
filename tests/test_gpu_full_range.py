"""GPU parity at the limits of the routes of full-matrix Gotoh scoring.

nvbio_full_gotoh_score picks the kernel of a batch on the host (full_score() and full_packed_ok(), csrc/gotoh_full.hip) from the declared
max_pattern_len = M and max_text_len = N, the number of jobs n, the scheme and the algorithm flags; step = the scheme's largest single term
in absolute value:

  packed (pk, pk16)   two jobs per lane in int16 registers: pattern blocking, 2-bit text and 2- or 4-bit reads, n >= 262,144 or
                      NVBIO_ALN_FORCE_PACKED_DP; every term <= 4096, (M + N) * step <= 12000, LOCAL: match * M <= 2000 (the sink key
                      score << 4 | column fits an int16); only the jobs of shape (M, N)
  cooperative (coop)  L lanes per job, the boundary in int32 registers: GLOBAL, SEMI_GLOBAL outside the end-to-end case, no min_scores,
                      M <= 256, (M + N + 2) * step <= 30000, not the packed route
  narrow              band 31 around the best diagonal, then the run test: the end-to-end shortcut applies, M <= 161, the band-31 int16
                      rule (M + 32) * step <= 8000, pat_ge < 0
  int32 (i32)         everything else: one lane per job with the reference's short2 boundary column, its truncation included

Each rule is a claim that no value leaves what the narrower representation holds exactly.  util.full_route() restates the rules,
util.full_last_admitted() solves them; the tests run the LAST shape a route admits and the FIRST it refuses on inputs that reach the range
(under a flat scheme, every penalty = s: a GLOBAL all-mismatch job scores exactly -N * s, a SEMI_GLOBAL one -M * s, a perfect LOCAL read
match * M, sinks lie at (N, M)); those conditions are asserted on the oracle's output, so no batch can be benign.  Scores and sinks must
equal the oracle's (int32) job by job; the rows of tests/golden/full_range_golden.npz must equal what the reference itself returned.

The packed bound of 12,000 leaves a margin of about 2.7 under int16, the cooperative one of 30,000 a margin of 2,767: the first refused shape
shows that the route chosen instead is exact, not that the bound is tight (test_past_the_edge).

Kernels seen under `rocprofv3 --kernel-trace --stats` on an MI355X, one run per test (template arguments: full_gotoh_pb_pk_kernel<type,
read bits>, full_gotoh_pb_pk16_kernel<read bits>, full_gotoh_coop_kernel<type, L, W, read bits>, full_gotoh_kernel<type, text blocking,
read bits, text bits>; types 0 / 1 / 2 = GLOBAL / LOCAL / SEMI_GLOBAL):

  test_packed_route_edges     full_gotoh_pb_pk_kernel<0|1|2,4|2> and full_gotoh_pb_pk16_kernel<4|2> behind classify_shape_kernel (the
                              admitted side under the forced switches; <2,..> for SEMI_GLOBAL with a match bonus and under PK_STRIPE8);
                              full_gotoh_kernel<0|1|2,false,4|2,2,false,false> (the refused side, the ragged third, NO_PACKED_DP);
                              full_gotoh_coop_kernel<0|2,4,8,4|2> (default flags without min_scores); ungapped_full_e2e_kernel<4|2,0|1>,
                              narrow_jobs_kernel, banded_gotoh_band31_pk_kernel<2,4|2,2,true,false,true>, narrow_check_kernel<4|2>
  test_cooperative_route_edges  full_gotoh_coop_kernel<0,4,8,4>, <2,4,8,4> (8 rows), <0,8,32,4>, <2,8,32,4> (256 rows);
                              full_gotoh_kernel<0|2,false|true,4,2,..> (the refused side, 257 rows, NO_COOPERATIVE_DP)
  test_past_the_edge          full_gotoh_kernel<0|1,false|true,4,2,..>, nothing else
  test_default_switch_at_262144_jobs  at 262,144 jobs full_gotoh_pb_pk_kernel<0,4>, <1,4>, full_gotoh_pb_pk16_kernel<4> behind
                              classify_shape_kernel; below, and under NO_PACKED_DP, full_gotoh_coop_kernel<0,4,8,4> and
                              full_gotoh_kernel<0|1|2,false,4,2,..>; the shortcut and the narrow-route kernels in front of SEMI_GLOBAL
  test_narrow_route_length_edge  narrow_jobs_kernel, banded_gotoh_band31_pk_kernel<2,4,2,true,false,true>, narrow_check_kernel<4> (161 rows);
                              ungapped_full_e2e_kernel<4,0|1>, full_gotoh_pb_pk16_kernel<4>, full_gotoh_kernel<2,false,4,2,..>
  test_int16_column_truncation  full_gotoh_kernel<0|1|2,false|true,4,2,..>; ungapped_full_e2e_kernel<4,0|1> in front of SEMI_GLOBAL
  test_fixture_rows           full_gotoh_pb_pk_kernel<0|1|2,4>, full_gotoh_pb_pk16_kernel<4>, full_gotoh_coop_kernel<0|2,4,8,4>,
                              full_gotoh_kernel<0|1|2,false|true,4,2,..>, the shortcut and the narrow-route kernels
"""
import os

import numpy as np
import pytest

import oracle
from util import (F_FORCE_PACKED, F_NO_COOP, F_NO_NARROW, F_NO_PACKED, F_NO_UNGAPPED, F_PK_STRIPE8, FULL_PK_EDGES, flat_scheme,
                  full_jobs, full_last_admitted, full_layout, full_pk_edge_sides, full_route, full_shapes, full_step)

pytestmark = pytest.mark.gpu

G, L_, SG = oracle.GLOBAL, oracle.LOCAL, oracle.SEMI_GLOBAL
EXTREME = ("allmm", "perfect", "shift")


@pytest.fixture(scope="module")
def full_golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "full_range_golden.npz"), allow_pickle=False)


def test_flag_numbers(amd):
    """util.full_route() reads the algorithm flags by the numbers of the C-ABI"""
    assert (F_NO_UNGAPPED, F_NO_PACKED, F_FORCE_PACKED, F_PK_STRIPE8, F_NO_NARROW, F_NO_COOP) == (
        amd.ALN_NO_UNGAPPED_SCORE, amd.ALN_NO_PACKED_DP, amd.ALN_FORCE_PACKED_DP, amd.ALN_PK_STRIPE8, amd.ALN_NO_NARROW_SCORE,
        amd.ALN_NO_COOPERATIVE_DP)


def _batch(seed, shapes, with_q=False, allow_n=True, first=0, kinds=None):
    """jobs of the given shapes, kinds by util.FULL_KINDS (neighbours differ), reads stored reversed and / or complemented at random;
    all-mismatch reads of a quality scheme carry the quality of the largest penalty"""
    rng = np.random.default_rng(seed)
    pats, txts, names = full_jobs(seed + 1, shapes, first=first, allow_n=allow_n, kinds=kinds)
    quals = None
    if with_q:
        quals = [np.full(len(p), 63, dtype=np.uint8) if k == "allmm" else rng.integers(0, 64, len(p), dtype=np.uint8) for p, k in zip(pats, names)]
    L = full_layout(pats, txts, quals, flags=rng.integers(0, 4, len(pats)))
    L["kinds"] = names
    return L


def _oracle(orc, typ, blocking, sv, L, ms=None):
    """(scores, sinks, ok); with per-job min_scores job by job"""
    if ms is None:
        sc, sk = orc.full_gotoh_batch(typ, blocking, oracle.Scheme(*sv), L["pats"], L["roffs"], L["text"], L["toffs"], quals=L["pquals"])
        return sc, sk, np.ones(len(sc), dtype=bool)
    n = len(ms)
    sc, sk, ok = np.zeros(n, dtype=np.int32), np.zeros((n, 2), dtype=np.uint32), np.zeros(n, dtype=bool)
    s_ = oracle.Scheme(*sv)
    for j in range(n):
        p0, p1, t0, t1 = L["roffs"][j], L["roffs"][j + 1], L["toffs"][j], L["toffs"][j + 1]
        ok[j], sc[j], sk[j] = orc.full_gotoh(typ, blocking, s_, L["pats"][p0:p1], L["text"][t0:t1],
                                             L["pquals"][p0:p1] if L["pquals"] is not None else None, int(ms[j]))
    return sc, sk, ok


def _gpu(amd, orc, typ, blocking, sv, L, M, N, algo, read_bits=4, ms=None, jobs=None):
    key = "_packed%d" % read_bits
    if key not in L:
        L[key] = (orc.pack4(L["reads"]) if read_bits == 4 else orc.pack2(L["reads"]), orc.pack2(L["text"]))
    n = len(L["wb"]) if jobs is None else jobs
    batch = amd.AlignmentBatch(L[key][0], read_bits, L["roffs"][:n + 1], L[key][1], 2, L["wb"][:n], L["we"][:n], quals=L["quals"],
                               flags=L["flags"][:n], algo_flags=algo)
    sc, sk = amd.BatchedAlignmentScore(amd.make_gotoh_aligner(typ, amd.GotohScheme(*sv)), text_blocking=bool(blocking)).enact(batch, M, N, min_scores=ms)
    return sc.cpu().numpy(), amd.u32(sk)


def _check(got, want, what):
    sc, sk = got
    wsc, wsk = want[0][:len(sc)], want[1][:len(sc)]
    bad = np.nonzero((sc != wsc) | (sk != wsk).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:6], sc[bad[:6]], wsc[bad[:6]], sk[bad[:6]].tolist(), wsk[bad[:6]].tolist())


def _assert_reaches_the_range(L, typ, sv, M, N, want, packed=True):
    """the conditions that keep a batch from being benign, on the oracle's output; -> the extreme score of the dominant shape"""
    wsc, wsk = want[0].astype(np.int64), want[1]
    kinds, Ms, Ns = L["kinds"], L["M"], L["N"]
    n = len(kinds)
    assert n % 2 == 1 and (kinds[:-1] != kinds[1:]).all()                       # lane partners differ in kind
    if packed:                                                                  # only the jobs of the dominant shape run packed
        assert ((Ms == M) & (Ns == N)).sum() * 3 >= 2 * n
    if n >= 15:
        assert np.isin(kinds, EXTREME).sum() * 4 >= n and (kinds == "mut").sum() * 4 >= n
    assert ((wsk[:, 0] == N) & (wsk[:, 1] == M)).any()                          # a sink in the matrix' last cell
    nothing = wsc == oracle.SCORE_MIN
    assert nothing.sum() * 10 <= n                                              # jobs that report nothing
    match, s = sv[0], full_step(sv[1:])
    flat = tuple(sv[1:]) == flat_scheme(match, s)[1:]
    am, pf = kinds == "allmm", kinds == "perfect"
    dom_am = am & (Ms == M) & (Ns == N)
    low = wsc[~nothing].min()
    if typ == G and flat:
        assert np.array_equal(wsc[am], -Ns[am] * s) and (not dom_am.any() or low == -N * s)
        return -N * s
    if typ == SG and flat:
        assert np.array_equal(wsc[am], -Ms[am] * s) and (not dom_am.any() or low == -M * s)
        return -M * s
    if typ == L_:
        assert np.array_equal(wsc[pf], Ms[pf] * match) and (wsc[am] == 0).all() and wsc.max() == match * M
        return match * M
    return None


def _min_scores(rng, typ, sv, L, want):
    """per-job limits on both sides of what the jobs reach: at the final score and next to it (the oracle decides whether the stripe test
    sees it), at the level the first stripes reach, beyond every alignment (those jobs leave at the first test), and none"""
    wsc = want[0].astype(np.int64)
    n = len(wsc)
    first_stripes = -full_step(sv) * rng.integers(0, 17, n) if sv[0] == 0 or typ != L_ else sv[0] * rng.integers(1, 1 + np.maximum(L["M"], 1))
    pick = rng.integers(0, 6, n)
    beyond = sv[0] * L["M"] + 1                                                 # more than any alignment scores: out at the first test
    ms = np.select([pick == 0, pick == 1, pick == 2, pick == 3, pick == 4], [wsc - 3, wsc, wsc + 1, first_stripes, beyond], oracle.SCORE_MIN)
    ms[wsc == oracle.SCORE_MIN] = oracle.SCORE_MIN
    return np.clip(ms, oracle.SCORE_MIN, 2 ** 31 - 1).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the packed route
# ---------------------------------------------------------------------------------------------------------------------------------------
# the rules solved by hand: the last max_text_len each edge admits at its max_pattern_len (for LOCAL's key rule: the last max_pattern_len)
PK_TABLE = {"g_flat8_m9": 1491, "g_flat8_m24": 1476, "g_match8_flat8_m24": 1476, "g_flat40_m9": 291, "g_flat1_m9": 11991, "g_flat4096_m1": 1,
            "g_penalty4096_m1": 1, "g_asym8_m24": 1476, "sg_flat8_m24": 1476, "sg_flat8_m9": 1491, "sg_match3_flat8_m9": 1491,
            "sg_ramp8_m24": 1476, "l_flat8_m24": 1476, "l_key_match2": 1000, "l_key_match1": 2000, "l_key_match20": 100,
            "l_key_match5_ramp": 400}


def _pk_switches():
    return (("force", F_FORCE_PACKED), ("force, stripe8", F_FORCE_PACKED | F_PK_STRIPE8), ("force, no_ungapped", F_FORCE_PACKED | F_NO_UNGAPPED),
            ("force, no_narrow", F_FORCE_PACKED | F_NO_NARROW), ("no_packed", F_NO_PACKED), ("no_coop", F_NO_COOP), ("default", 0))


@pytest.mark.parametrize("read_bits", [4, 2], ids=lambda b: "%dbit" % b)
@pytest.mark.parametrize("side", [0, 1], ids=["last_admitted", "first_refused"])
@pytest.mark.parametrize("edge", FULL_PK_EDGES, ids=lambda e: e[0])
def test_packed_route_edges(amd, orc, edge, side, read_bits):
    """both sides of one threshold of full_packed_ok(): the last shape (M, N) the packed kernels admit and the first they refuse (for the
    penalty limit: the next penalty), two thirds of the jobs of that shape, the others ragged.  (M + N) * step = 12000 | 12001 at steps 8, 40,
    1 and 4096 with short patterns, so that a GLOBAL all-mismatch job scores -(12000 - M * step); LOCAL's match * M = 2000 | 2001.  Every
    switch of the route -- forced, 8 columns per stripe, without the shortcut, without the narrow route, refused by flag, without the
    cooperative kernel, default -- gives the oracle's scores and sinks, with and without per-job min_scores (patterns of 1,000 and more
    rows, which take a lane of the int32 kernel a quarter of a second: min_scores where the route is forced, refused, and by default)"""
    name, typ, sv0, M0, with_q = edge
    sides = full_pk_edge_sides(edge)
    # the rules, solved here, give the table's figure; one more symbol (or one more unit of penalty) leaves the route
    assert full_last_admitted("pk", typ, sv0, M0) == PK_TABLE[name] == (sides[0][2] if M0 is not None else sides[0][1])
    for sv, M, N in sides[side:side + 1]:
        n = 15 if M >= 2000 else 61 if M >= 400 else 205 if M * N > 50000 else 307
        route = full_route(typ, sv, 0, M, N, n, F_FORCE_PACKED, read_bits=read_bits, has_quals=with_q)
        assert route.split("+")[-1] == (("pk16" if typ == SG and sv[0] == 0 else "pk") if side == 0 else "i32"), (name, side, route)
        L = _batch(1000 * FULL_PK_EDGES.index(edge) + 10 * side + read_bits, full_shapes(7 + side, M, N, n), with_q=with_q, allow_n=read_bits == 4)
        want = _oracle(orc, typ, 0, sv, L)
        extreme = _assert_reaches_the_range(L, typ, sv, M, N, want)
        if side == 0 and typ == G and extreme is not None:
            assert extreme == -(12000 // full_step(sv) * full_step(sv) - M * full_step(sv))
        if side == 0 and M0 is None:
            assert extreme == 2000 // sv[0] * sv[0]
        ms = _min_scores(np.random.default_rng(5 + side), typ, sv, L, want)
        want_ms = _oracle(orc, typ, 0, sv, L, ms)
        dominant = (L["M"] == M) & (L["N"] == N)
        if M > 8:                                                               # (a pattern of one stripe is never tested)
            assert want_ms[2][dominant].any() and not want_ms[2][dominant].all(), name
        for what, algo in _pk_switches():
            _check(_gpu(amd, orc, typ, 0, sv, L, M, N, algo, read_bits), want, (name, side, what))
            if M < 1000 or what in ("force", "no_packed", "default"):
                _check(_gpu(amd, orc, typ, 0, sv, L, M, N, algo, read_bits, ms), want_ms, (name, side, what, "min_scores"))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cooperative kernel
# ---------------------------------------------------------------------------------------------------------------------------------------
# (name, type, scheme, max_pattern_len or None for the 256 | 257 edge, qualities?) and, solved by hand, the last max_text_len
COOP_EDGES = (("g_flat8_m8", G, flat_scheme(0, 8), 8, False), ("g_flat8_m256", G, flat_scheme(0, 8), 256, False),
              ("sg_match3_flat8_m8", SG, flat_scheme(3, 8), 8, False), ("sg_match3_flat8_m256", SG, flat_scheme(3, 8), 256, False),
              ("g_flat40_m256", G, flat_scheme(0, 40), 256, False), ("g_asym8_ramp_m256", G, (2, 3, 8, -8, -2, -6, -3), 256, True),
              ("g_flat8_rows", G, flat_scheme(0, 8), None, False))
COOP_TABLE = {"g_flat8_m8": 3740, "g_flat8_m256": 3492, "sg_match3_flat8_m8": 3740, "sg_match3_flat8_m256": 3492, "g_flat40_m256": 492,
              "g_asym8_ramp_m256": 3492, "g_flat8_rows": 256}


@pytest.mark.parametrize("edge", COOP_EDGES, ids=lambda e: e[0])
def test_cooperative_route_edges(amd, orc, edge):
    """(M + N + 2) * step = 30000 | 30001 for max_pattern_len 8 (4 lanes per job) and 256 (8 lanes), and max_pattern_len 256 | 257: GLOBAL, and
    SEMI_GLOBAL with a match bonus, both blockings, batches of 1, 3 and 517 jobs of which every eighth has the full shape and the others
    ragged patterns (1 .. M) in windows of 0 .. 300 symbols -- equal to the oracle and to the one-lane-per-job kernel
    (NVBIO_ALN_NO_COOPERATIVE_DP).  At step 8 and M = 8 the GLOBAL all-mismatch jobs score -29,920, 2,848 above int16's floor"""
    name, typ, sv, M0, with_q = edge
    assert full_last_admitted("coop", typ, sv, M0) == COOP_TABLE[name]
    sides = ((M0, COOP_TABLE[name]), (M0, COOP_TABLE[name] + 1)) if M0 is not None else ((256, 300), (257, 300))
    for side, (M, N) in enumerate(sides):
        for n in (1, 3, 517):
            rng = np.random.default_rng(31 * n + side)
            shapes = []
            for j in range(n):                                                  # (every 16th window is shorter than its read, or empty)
                m = int(rng.integers(1, M + 1))
                w = int(rng.integers(m, min(N, m + 300) + 1)) if j % 16 != 5 else int(rng.integers(0, m)) * (j % 32 == 5)
                shapes.append((M, N) if j % 8 == 0 else (m, w))
            L = _batch(4000 + 100 * COOP_EDGES.index(edge) + 10 * side + n, shapes, with_q=with_q)
            for blocking in (0, 1):
                assert full_route(typ, sv, blocking, M, N, n, has_quals=with_q) == ("coop" if side == 0 else "i32")
                assert full_route(typ, sv, blocking, M, N, n, F_NO_COOP, has_quals=with_q) == "i32"
                want = _oracle(orc, typ, blocking, sv, L)
                if blocking == 0:                                               # (text blocking truncates the other column)
                    extreme = _assert_reaches_the_range(L, typ, sv, M, N, want, packed=False)
                    assert name != "g_flat8_m8" or extreme == (-29920, -29928)[side]
                _check(_gpu(amd, orc, typ, blocking, sv, L, M, N, 0), want, (name, side, n, blocking, "default"))
                _check(_gpu(amd, orc, typ, blocking, sv, L, M, N, F_NO_COOP), want, (name, side, n, blocking, "no_coop"))


# ---------------------------------------------------------------------------------------------------------------------------------------
# past the edges
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["local_key_2048", "global_31000"])
def test_past_the_edge(amd, orc, case):
    """the packed bound of 12,000 leaves a margin of about 2.7 under int16, so the first refused shape of test_packed_route_edges can only
    show that the route chosen instead is exact: it cannot show that the bound is tight, and nothing here claims so.  These are two points
    where a narrower type is provably wrong just past its rule, and the route the rules choose must still be exact: LOCAL perfect reads at
    match * M = 2048 (match 2, M = 1024), whose sink key score << 4 reaches 32,768; GLOBAL flat 8 at (M + N) * step = 31,000, exact in
    the reference's int16 column (-30,936) but outside both 16-bit routes"""
    if case == "local_key_2048":
        typ, sv, M, N, n = L_, (2, 3, 3, -5, -2, -5, -2), 1024, 1064, 61
        assert (M + N) * full_step(sv) <= 12000                                 # the sum rule admits it: the key rule alone refuses
        routes = {F_FORCE_PACKED: "i32", 0: "i32"}
    else:
        typ, sv, M, N, n = G, flat_scheme(0, 8), 8, 3867, 205
        assert (M + N) * 8 == 31000
        routes = {F_FORCE_PACKED: "i32", 0: "i32", F_NO_COOP: "i32"}
    L = _batch(8000 + M, full_shapes(3, M, N, n))
    for blocking in (0, 1):
        want = _oracle(orc, typ, blocking, sv, L)
        if blocking == 0:
            assert _assert_reaches_the_range(L, typ, sv, M, N, want) == (2048 if typ == L_ else -30936)
        for algo, route in routes.items():
            assert full_route(typ, sv, blocking, M, N, n, algo) == route
            _check(_gpu(amd, orc, typ, blocking, sv, L, M, N, algo), want, (case, blocking, algo))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the default switch to the packed route
# ---------------------------------------------------------------------------------------------------------------------------------------
def _uniform_batch(seed, n, M, N):
    """n jobs of one shape, vectorised; job j is of kind j % 5: all-mismatch, perfect, shifted to the last diagonal, one substitution,
    random; reads stored reversed and / or complemented at random"""
    rng = np.random.default_rng(seed)
    kind = np.arange(n) % 5
    txt = rng.integers(0, 4, (n, N), dtype=np.uint8)
    d = rng.integers(0, N - M + 1, n); d[kind == 2] = N - M
    pat = np.take_along_axis(txt, d[:, None] + np.arange(M)[None, :], 1)
    rows = np.nonzero(kind == 3)[0]; pos = rng.integers(0, M, len(rows))
    pat[rows, pos] = (pat[rows, pos] + 1 + rng.integers(0, 3, len(rows))) % 4
    rows = np.nonzero(kind == 4)[0]; pat[rows] = rng.integers(0, 4, (len(rows), M), dtype=np.uint8)
    rows = np.nonzero(kind == 0)[0]; a = rng.integers(0, 4, len(rows), dtype=np.uint8)
    pat[rows] = a[:, None]; txt[rows] = (a[:, None] + 1 + rng.integers(0, 3, (len(rows), N))) % 4
    flags = rng.integers(0, 4, n).astype(np.uint8)
    stored = np.where((flags & 2)[:, None] != 0, 3 - pat, pat)
    stored = np.where((flags & 1)[:, None] != 0, stored[:, ::-1], stored).astype(np.uint8)
    roffs = (np.arange(n + 1, dtype=np.uint64) * M).astype(np.uint32); toffs = (np.arange(n + 1, dtype=np.uint64) * N).astype(np.uint32)
    return dict(reads=stored.reshape(-1), pats=pat.reshape(-1), pquals=None, quals=None, roffs=roffs, text=txt.reshape(-1), toffs=toffs,
                wb=toffs[:-1].copy(), we=toffs[1:].copy(), flags=flags, kind=kind)


@pytest.mark.parametrize("shape", [(8, 16), (9, 24)], ids=lambda s: "%dx%d" % s)
def test_default_switch_at_262144_jobs(amd, orc, shape):
    """under default flags a batch of 262,144 jobs is the first that runs two jobs per lane -- and the first the cooperative kernel does not
    get: 262,143 | 262,144 jobs of one shape, the three types, equal to the oracle and to the run with NVBIO_ALN_NO_PACKED_DP"""
    M, N = shape
    n = 262144
    L = _uniform_batch(90 + M, n, M, N)
    for typ, sv, below, at in ((G, (2, 2, 6, -8, -3, -8, -3), "coop", "pk"), (L_, (2, 2, 6, -8, -3, -8, -3), "i32", "pk"),
                               (SG, (0, 6, 6, -8, -3, -8, -3), "narrow+i32", "narrow+pk16")):
        assert full_route(typ, sv, 0, M, N, n - 1) == below and full_route(typ, sv, 0, M, N, n) == at
        assert full_route(typ, sv, 0, M, N, n, F_NO_PACKED) == ("coop" if typ == G else "i32")
        want = orc.full_gotoh_batch(typ, 0, oracle.Scheme(*sv), L["pats"], L["roffs"], L["text"], L["toffs"])
        wsc, wsk = want
        assert ((wsk[:, 0] == N) & (wsk[:, 1] == M)).any() and (wsc > oracle.SCORE_MIN).all()
        if typ == L_:
            assert (wsc[L["kind"] == 1] == 2 * M).all() and (wsc[L["kind"] == 0] == 0).all() and wsc.max() == 2 * M
        if typ == SG:
            assert (wsc[L["kind"] == 1] == 0).all() and (wsc[L["kind"] == 3] >= -6).all() and wsc.min() < -6 * M // 2
        for jobs in (n - 1, n):                                                  # (the smaller batch: the larger one without its last job)
            for algo in (0, F_NO_PACKED):
                _check(_gpu(amd, orc, typ, 0, sv, L, M, N, algo, jobs=jobs), want, (shape, typ, jobs, algo))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the narrow route
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sv,refused", [((0, 6, 6, -8, -3, -8, -3), False), ((0, 6, 6, -8, 0, -8, -3), True)], ids=["e2e", "pat_ge0"])
def test_narrow_route_length_edge(amd, orc, sv, refused):
    """the narrow route takes patterns of up to 161 rows (what the band-31 first pass holds): max_pattern_len 161 | 162, windows from M + 30
    to 528 symbols, with the route, without it (NVBIO_ALN_NO_NARROW_SCORE) and in front of the packed kernels; a scheme with pat_ge == 0 is
    refused at either length"""
    assert full_last_admitted("narrow", SG, sv) == 161
    for M in (161, 162):
        n = 301
        rng = np.random.default_rng(M)
        shapes = [(M if j % 3 != 2 else int(rng.integers(40, M + 1)), int(rng.integers(M + 30, 529))) for j in range(n)]
        shapes[0] = (M, 528)
        L = _batch(6000 + M, shapes)
        want = _oracle(orc, SG, 0, sv, L)
        wsc = want[0]
        kinds = L["kinds"]
        assert (kinds[:-1] != kinds[1:]).all() and (wsc[kinds == "perfect"] == 0).all() and (wsc <= -8).sum() * 2 >= n
        assert ((want[1][:, 0] == L["N"]) & (want[1][:, 1] == L["M"])).any()
        for algo in (0, F_NO_NARROW, F_FORCE_PACKED, F_FORCE_PACKED | F_NO_NARROW):
            route = full_route(SG, sv, 0, M, 528, n, algo)
            assert route.startswith("narrow+") == (M == 161 and not refused and not algo & F_NO_NARROW), (M, algo, route)
            _check(_gpu(amd, orc, SG, 0, sv, L, M, 528, algo), want, (sv, M, algo))


# ---------------------------------------------------------------------------------------------------------------------------------------
# beyond int16
# ---------------------------------------------------------------------------------------------------------------------------------------
TRUNCATION_CASES = (("global_flat8", G, flat_scheme(0, 8), 8, 4200, 205, -33600),
                    ("local_match9", L_, (9, 2, 60, -8, -3, -8, -3), 4000, 4040, 5, 36000),
                    ("semi_global_flat8", SG, flat_scheme(0, 8), 4200, 4230, 5, -33600))


@pytest.mark.parametrize("blocking", [0, 1], ids=["pattern_blocking", "text_blocking"])
@pytest.mark.parametrize("case", TRUNCATION_CASES, ids=lambda c: c[0])
def test_int16_column_truncation(amd, orc, case, blocking):
    """beyond +-32,767 the reference's result is defined by its short2 store of the boundary column, and full_gotoh_kernel reproduces it:
    GLOBAL flat 8 at M = 8, N = 4,200 (-33,600 without the truncation), LOCAL (9, 2, 60, ...) with perfect reads of 4,000 rows (36,000),
    SEMI_GLOBAL flat 8 all-mismatch at M = 4,200 (-33,600).  The oracle's restatement of the truncation is pinned on the reference by the
    rows of full_range_golden.npz (tests/test_oracle_golden.py)"""
    name, typ, sv, M, N, n, untruncated = case
    kinds = None if n > 15 else ["allmm", "perfect", "mut", "shift", "gap"]
    L = _batch(7000 + M, [(M, N)] * n, kinds=kinds)
    assert full_route(typ, sv, blocking, M, N, n) == "i32" and full_route(typ, sv, blocking, M, N, n, F_FORCE_PACKED) == "i32"
    want = _oracle(orc, typ, blocking, sv, L)
    # what the DP gives in int32 is out of int16's range: the column cannot hold it
    assert abs(untruncated) > 32767 and untruncated == {G: -N * 8, L_: 9 * M, SG: -M * 8}[typ] and untruncated not in want[0]
    assert np.abs(want[0].astype(np.int64)).max() > 30000
    for algo in (0, F_FORCE_PACKED, F_NO_COOP):
        _check(_gpu(amd, orc, typ, blocking, sv, L, M, N, algo), want, (name, blocking, algo))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the reference's own results
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ["pk", "coop", "i32"])
def test_fixture_rows(amd, orc, full_golden, group):
    """the rows of full_range_golden.npz whose combination of scheme and shape the rules send to the packed kernels, the cooperative one or
    the int32 one, a batch per combination: what the reference's own host code returned for them, both blockings, under the route
    util.full_route() names for the combination and again with that route switched off (the shapes beyond int16, 4,000 rows in one lane:
    once)"""
    g = full_golden
    checked, routes = 0, set()
    for combo in np.unique(g["combo"]):
        rows = np.nonzero(g["combo"] == combo)[0]
        if not str(g["route"][rows[0]]).split("+")[-1].startswith(group):
            continue
        i0 = rows[0]
        typ, M, N, algo = int(g["typ"][i0]), int(g["max_pattern_len"][i0]), int(g["max_text_len"][i0]), int(g["algo"][i0])
        sv = tuple(int(v) for v in g["schemes"][g["scheme"][i0]])
        has_q = bool(g["has_quals"][i0])
        route = full_route(typ, sv, 0, M, N, len(rows), algo, has_quals=has_q)
        assert route == str(g["route"][i0]), (combo, route)
        routes.add(route)
        pats = [g["pats"][g["pat_off"][i]:g["pat_off"][i + 1]] for i in rows]
        txts = [g["txts"][g["txt_off"][i]:g["txt_off"][i + 1]] for i in rows]
        quals = [g["quals"][g["pat_off"][i]:g["pat_off"][i + 1]] for i in rows] if has_q else None
        L = full_layout(pats, txts, quals, flags=(np.arange(len(rows)) + combo) % 4)
        off = {"pk": F_NO_PACKED, "pk16": F_NO_PACKED, "coop": F_NO_COOP, "i32": F_FORCE_PACKED}[route.split("+")[-1]]
        for blocking in (0, 1):
            ref = g["out"][rows, blocking]
            want = (ref[:, 1].astype(np.int32), ref[:, 2:4].astype(np.uint32))
            assert (ref[:, 0] == 1).all()
            for a in (algo, off, off | F_NO_NARROW) if M * N < 10 ** 6 else (algo,):
                _check(_gpu(amd, orc, typ, blocking, sv, L, M, N, a), want, (int(combo), typ, sv, blocking, a))
        checked += len(rows)
    assert checked >= {"pk": 25, "coop": 4, "i32": 40}[group] and {"pk": {"pk", "narrow+pk16", "pk16"}, "coop": {"coop"}, "i32": {"i32", "narrow+i32"}}[group] <= routes
