"""GPU parity at the numeric limits of band-31 scoring, and on reads far longer than the 161 rows the first pass holds.

nvbio_banded_gotoh_score picks the arithmetic of band 31 on the host (packed_ok() and launch_pk_kernel(), csrc/band31_packed.hip), for 4- or
2-bit reads in a 2-bit text, from the batch's max_read_len = M and the scheme; step = the scheme's largest single penalty:

  binary16 lanes   SEMI_GLOBAL, match == 0, two-wave build, (M + 32) * step <= 2040 (and mm_max <= 400)
  int16 lanes      GLOBAL / SEMI_GLOBAL: (M + 32) * max(step, match) <= 8000 and every penalty <= 4096;
                   LOCAL: match * M <= 1000 and the mismatch and pattern-gap penalties <= 4096
  int32            everything else, M == 0 (no bound declared) and NVBIO_ALN_NO_PACKED_DP

Each rule is a proof that no intermediate value leaves the range the narrower type holds exactly.  util.band31_route() restates the rules,
util.band31_last_admitted() solves them for M; the tests below run the LAST length a route admits and the FIRST it refuses (or, where the
length cannot move, the next penalty), on inputs that reach the range: the all-mismatch jobs of a flat scheme (every penalty = s) score
exactly -M * s (SEMI_GLOBAL) or -(M + 30) * s (GLOBAL), perfect LOCAL reads score match * M, sinks lie at (M + 30, M).  Those conditions are
asserted on the oracle's output, so no batch can be benign.  Scores and sinks must equal the oracle's (int32 throughout) under every switch
that changes the arithmetic; the rows of tests/golden/band31_range_golden.npz must also equal what the reference itself returned.

Kernels seen under `rocprofv3 --kernel-trace --stats` on an MI355X, one run per group of tests (the packed kernel's template arguments
are <type, read bits, waves per SIMD, match == 0, ragged, binary16>, types 0 / 1 / 2 = GLOBAL / LOCAL / SEMI_GLOBAL; the int32 kernel's
<band, type, read bits, text bits, false, false>):

  test_route_edges[f16_*]    banded_gotoh_band31_pk_kernel<2,4,2,true,false,true> and <2,2,2,true,false,true> (binary16: the admitted side);
                             <2,4|2,2,true,false,false> (int16: the refused side and NVBIO_ALN_NO_F16_DP), <2,4|2,3,true,false,false> (three
                             waves); banded_gotoh_kernel<31,2,4|2,2,..>; in front of them ungapped_e2e31_kernel<4|2,0,false>, <4,0,true>
                             (qualities), <4,1,..>, <4,2,..> and chances_e2e31_kernel<4|2>
  test_route_edges[i16_*]    banded_gotoh_band31_pk_kernel<0,4,2|3,false,..>, <0,4|2,2|3,true,..>, <1,4|2,2|3,false,..>, <2,4,2|3,true,..>,
                             <2,4,2|3,false,..>, all with binary16 = false; banded_gotoh_kernel<31,0|1|2,4,2,..> and <31,0|1,2,2,..>
  test_route_edges[i32_*]    banded_gotoh_kernel<31,1,4,2,..> and <31,1,2,2,..>, nothing else
  test_twice_past_the_edge   banded_gotoh_band31_pk_kernel<2,4,2|3,true,false,false>; banded_gotoh_kernel<31,2,4,2,..> and <31,1,4,2,..>
  test_long_ragged_reads     banded_gotoh_band31_pk_kernel<2,4,2,true,true,false> and <2,4,2,true,true,true> (the ragged builds),
                             <2,4,2,true,false,false> and <2,4,2,true,false,true>; job_length_keys_kernel and the radix sort; the first pass
  test_int32_kernel_at_narrow_bands   banded_gotoh_kernel<3|7|15,0|1|2,4,2,..>
  test_fixture_rows          banded_gotoh_band31_pk_kernel<2,4,2,true,false,true>, <0|1|2,4,2,..,false,false>; banded_gotoh_kernel<31,0|1|2,4,2,..>
"""
import os

import numpy as np
import pytest

import oracle
from util import (RANGE_EDGES, band31_last_admitted, band31_route, flat_scheme, range_edge_sides, range_jobs, range_layout,
                  scheme_step)

pytestmark = pytest.mark.gpu

EXTREME = ("allmm", "perfect", "shift")


@pytest.fixture(scope="module")
def range_golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "band31_range_golden.npz"), allow_pickle=False)


def _switches(amd, M):
    """(name, max_read_len, algo flags): everything that changes the arithmetic of a band-31 batch"""
    return (("default", M, 0), ("no_f16", M, amd.ALN_NO_F16_DP), ("no_ungapped", M, amd.ALN_NO_UNGAPPED_SCORE),
            ("three_waves", M, amd.ALN_PK_THREE_WAVES), ("no_packed", M, amd.ALN_NO_PACKED_DP), ("int32", 0, 0))


def _oracle(orc, band, typ, sv, L):
    return orc.banded_gotoh_packed_batch(band, typ, oracle.Scheme(*sv), orc.pack4(L["reads"]), L["roffs"], orc.pack2(L["text"]), L["wb"], L["we"],
                                         flags=L["flags"], quals=L["quals"])


def _gpu(amd, orc, band, typ, sv, L, max_read_len, algo, read_bits=4):
    reads = orc.pack4(L["reads"]) if read_bits == 4 else orc.pack2(L["reads"])
    batch = amd.AlignmentBatch(reads, read_bits, L["roffs"], orc.pack2(L["text"]), 2, L["wb"], L["we"], quals=L["quals"], flags=L["flags"],
                               max_read_len=max_read_len, algo_flags=algo)
    sc, sk = amd.batch_banded_alignment_score(band, amd.make_gotoh_aligner(typ, amd.GotohScheme(*sv)), batch)
    return sc.cpu().numpy(), amd.u32(sk)


def _check(got, want, what):
    sc, sk = got
    wsc, wsk = want
    bad = np.nonzero((sc != wsc) | (sk != wsk).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:6], sc[bad[:6]], wsc[bad[:6]], sk[bad[:6]].tolist(), wsk[bad[:6]].tolist())


def _batch(seed, M, n, band=31, with_q=False, allow_n=True, lens=None, first=0):
    """n jobs (odd), two thirds of them M symbols long and the rest 1..M, kinds by util.RANGE_KINDS (neighbours differ), reads stored
    reversed and / or complemented at random; all-mismatch reads of a quality scheme carry the quality of the largest penalty"""
    rng = np.random.default_rng(seed)
    if lens is None:
        lens = np.where(np.arange(n) % 3 != 2, M, rng.integers(1, M + 1, n))
    pats, txts, kinds = range_jobs(seed + 1, lens, band, first=first, allow_n=allow_n)
    quals = None
    if with_q:
        quals = [np.full(len(p), 63, dtype=np.uint8) if k == "allmm" else rng.integers(0, 64, len(p), dtype=np.uint8) for p, k in zip(pats, kinds)]
    L = range_layout(pats, txts, quals, flags=rng.integers(0, 4, len(pats)))
    L["kinds"], L["lens"] = kinds, np.asarray(lens)
    return L


def _assert_reaches_the_range(L, typ, sv, M, want, band=31):
    """the conditions that make a batch worth running, on the oracle's output"""
    wsc, wsk = want
    kinds, lens = L["kinds"], L["lens"].astype(np.int64)
    n = len(kinds)
    assert n % 2 == 1 and (kinds[:-1] != kinds[1:]).all()                       # lane partners differ in kind
    assert np.isin(kinds, EXTREME).sum() * 4 >= n and (kinds == "mut").sum() * 4 >= n
    assert (lens == M).sum() * 2 >= n
    assert ((wsk[:, 0] == M + band - 1) & (wsk[:, 1] == M)).any()               # a sink in the band's last cell
    match, s = sv[0], scheme_step(sv)
    flat = tuple(sv[1:]) == flat_scheme(match, s)[1:]                           # (where a gap row is cheaper than a mismatch the bound is not met)
    am, pf = kinds == "allmm", kinds == "perfect"
    low = wsc[wsc > oracle.SCORE_MIN].min()                                     # (a window shorter than its read reports nothing)
    assert M < band + 3 or (wsc == oracle.SCORE_MIN).any()
    if typ == oracle.SEMI_GLOBAL and flat:
        assert np.array_equal(wsc[am], -lens[am] * s) and low == -M * s
    if typ == oracle.GLOBAL and flat:
        assert np.array_equal(wsc[am], -(lens[am] + band - 1) * s) and low == -(M + band - 1) * s
    if typ == oracle.LOCAL:
        assert np.array_equal(wsc[pf], lens[pf] * match) and wsc.max() == match * M and (wsc[am] == 0).all()


def _edge_ids():
    # one 2-bit-read variant per route
    return [(e, 4) for e in RANGE_EDGES] + [(e, 2) for e in RANGE_EDGES if e[0] in ("f16_flat8", "i16_g_flat8", "i16_local_match2", "i32_local_match9")]


# the rules solved by hand: the last max_read_len each edge's route admits
TABLE = {"f16_flat8": 223, "f16_flat10": 172, "f16_flat1": 2008, "f16_flat60": 2, "f16_ramp8": 223, "f16_asym8": 223,
         "i16_sg_flat8": 968, "i16_sg_match3_flat8": 968, "i16_g_flat8": 968, "i16_g_match8_flat8": 968, "i16_sg_flat40": 168,
         "i16_g_match40_flat40": 168, "i16_sg_flat1": 7968, "i16_g_flat1": 7968, "i16_g_match1_flat1": 7968, "i16_sg_flat242": 1,
         "i16_g_flat242": 1, "i16_sg_ramp8": 968, "i16_g_asym8": 968, "i16_local_match2": 500, "i16_local_match1": 1000,
         "i16_local_match3": 333, "i16_local_match5_ramp": 200, "i16_local_mm4096": 500, "i16_local_open4096": 500}


@pytest.mark.parametrize("edge,read_bits", _edge_ids(), ids=lambda v: v[0] if isinstance(v, tuple) else "%dbit" % v)
def test_route_edges(amd, orc, edge, read_bits):
    """both sides of one threshold of the table above: max_read_len = the last length the route admits, then the first it refuses (for
    step 242 at M = 1 and for the penalty limit 4096: the next penalty), two thirds of the jobs that long.  Every switch of the arithmetic --
    default, int16 instead of binary16 lanes, the DP for every job, the three-wave build, the int32 kernel by flag and by max_read_len = 0
    -- gives the oracle's scores and sinks.  LOCAL (9, 2, 60, ...) at 5,000 rows has perfect reads scoring 45,000: int32 is 32 bits wide."""
    name, route, typ, sv, with_q = edge
    sides = range_edge_sides(edge)
    if route != "i32":
        # the rules, solved here, give the table's figures; one more row (or one more unit of penalty) leaves the route
        assert sides[0][1] == band31_last_admitted(route, typ, sv) == TABLE[name] and band31_route(typ, sv, TABLE[name]) == route
        assert band31_route(typ, sides[1][0], sides[1][1]) == {"f16": "i16", "i16": "i32"}[route]
    for side, (ssv, M, _) in enumerate(sides):
        n = 307 if M <= 1100 else 205 if M <= 2100 else 131
        L = _batch(100 * RANGE_EDGES.index(edge) + side, M, n, with_q=with_q, allow_n=read_bits == 4)
        want = _oracle(orc, 31, typ, ssv, L)
        _assert_reaches_the_range(L, typ, ssv, M, want)
        if route == "i32":
            assert want[0].max() == 45000
        for what, mrl, algo in _switches(amd, M):
            _check(_gpu(amd, orc, 31, typ, ssv, L, mrl, algo, read_bits), want, (name, M, what))


@pytest.mark.parametrize("case", [("f16", oracle.SEMI_GLOBAL, flat_scheme(0, 1)), ("i16", oracle.SEMI_GLOBAL, flat_scheme(0, 8)),
                                  ("i16", oracle.LOCAL, (2, 6, 6, -8, -3, -8, -3))], ids=lambda c: "%s_type%d" % (c[0], c[1]))
def test_twice_past_the_edge(amd, orc, case):
    """the rules leave a margin (they bound (M + 32) * step where an end-to-end score reaches M * step), so the first refused length
    alone cannot tell a bound that is somewhat too wide.  At TWICE the limit the narrower type is certainly wrong -- odd scores down to
    -4,048 do not exist in binary16, -15,744 is next to int16's stand-in for minus infinity, a LOCAL score of 2,000 needs 11 bits --
    and the route the rules choose instead must still be exact"""
    route, typ, sv = case
    M = 2 * (band31_last_admitted(route, typ, sv) + (32 if typ != oracle.LOCAL else 0)) - (32 if typ != oracle.LOCAL else 0)
    assert band31_route(typ, sv, M) == {"f16": "i16", "i16": "i32"}[route]
    L = _batch(900 + typ + len(route), M, 205)
    want = _oracle(orc, 31, typ, sv, L)
    _assert_reaches_the_range(L, typ, sv, M, want)
    assert M * max(scheme_step(sv) if typ != oracle.LOCAL else 0, sv[0]) in (4048, 15744, 2000)
    for what, mrl, algo in _switches(amd, M):
        _check(_gpu(amd, orc, 31, typ, sv, L, mrl, algo), want, (route, typ, M, what))


@pytest.mark.parametrize("lanes", ["i16", "f16"])
def test_long_ragged_reads(amd, orc, lanes):
    """reads of 1 to 1,000 symbols in one batch, lengths on either side of a plane word (31..33), of the first pass's own limit (M > 161
    goes to the DP: 161, 162, 163), of 256 and 1,000; lane partners (8, 1000), (1000, 8), (161, 162) and (1, 999) in front.  max_read_len
    = 1000 under (0, 6, 6, -7, -3, -7, -3): step 7, because step 8 admits 968 rows only ((1000 + 32) * 8 = 8,256 > 8,000) -- int16 lanes.  The
    binary16 lanes take the same batch cut at their own limit: step 8, max_read_len = 223.  With and without the ragged-batch route, its
    length sort and the first pass."""
    sv, top = ((0, 6, 6, -7, -3, -7, -3), 1000) if lanes == "i16" else ((0, 6, 6, -8, -3, -8, -3), 223)
    assert band31_route(oracle.SEMI_GLOBAL, sv, top) == lanes and band31_route(oracle.SEMI_GLOBAL, (0, 6, 6, -8, -3, -8, -3), 1000) == "i32"
    rng = np.random.default_rng(61)
    pool = np.minimum([1, 7, 8, 9, 31, 32, 33, 161, 162, 163, 255, 256, 257, 999, 1000], top)
    lens = np.concatenate([np.minimum([8, 1000, 1000, 8, 161, 162, 1, 999], top), rng.choice(pool, 293)])
    L = _batch(62, top, len(lens), lens=lens, first=2)
    want = _oracle(orc, 31, oracle.SEMI_GLOBAL, sv, L)
    wsc, wsk = want
    kinds = L["kinds"]                                                          # (an all-mismatch read pays 3 or more on every row)
    assert len(lens) % 2 == 1 and (kinds[:-1] != kinds[1:]).all() and np.isin(kinds, EXTREME).sum() * 4 >= len(lens) and (kinds == "mut").sum() * 4 >= len(lens)
    assert all((lens == v).sum() >= 5 for v in pool) and wsc[wsc > oracle.SCORE_MIN].min() <= -3 * top and ((wsk[:, 0] == top + 30) & (wsk[:, 1] == top)).any()
    for ragged in (0, amd.ALN_RAGGED_READS):
        for sort in (0, amd.ALN_NO_LENGTH_SORT):
            for first_pass in (0, amd.ALN_NO_UNGAPPED_SCORE):
                _check(_gpu(amd, orc, 31, oracle.SEMI_GLOBAL, sv, L, top, ragged | sort | first_pass), want, (lanes, ragged, sort, first_pass))
    _check(_gpu(amd, orc, 31, oracle.SEMI_GLOBAL, sv, L, top, amd.ALN_RAGGED_READS | amd.ALN_NO_F16_DP), want, (lanes, "ragged, no_f16"))


@pytest.mark.parametrize("band", [3, 7, 15])
def test_int32_kernel_at_narrow_bands(amd, orc, band):
    """bands 3, 7 and 15 (one kernel, int32) on 2,000 rows, the same kinds scaled to the band: shifts of band / 2, gaps of 1, band / 2 and
    band - 1 symbols, windows clipped below M + band - 1 and below M; the three types under one scheme each"""
    M = 2000
    L = _batch(700 + band, M, 205, band=band)
    for typ, sv in ((oracle.LOCAL, (2, 2, 6, -8, -3, -8, -3)), (oracle.SEMI_GLOBAL, flat_scheme(0, 6)), (oracle.GLOBAL, flat_scheme(3, 5))):
        want = _oracle(orc, band, typ, sv, L)
        _assert_reaches_the_range(L, typ, sv, M, want, band)
        for mrl in (M, 0):
            _check(_gpu(amd, orc, band, typ, sv, L, mrl, 0), want, (band, typ, mrl))


@pytest.mark.parametrize("route", ["f16", "i16", "i32"])
def test_fixture_rows(amd, orc, range_golden, route):
    """the rows of band31_range_golden.npz whose combination of scheme and length the rules send to `route`, a batch per combination with
    max_read_len = that length: what the reference's own host code returned for them (and the oracle, again), with the declared bound and
    without; reads stored under rotating reverse / complement flags"""
    g = range_golden
    checked = 0
    for combo in np.unique(g["combo"][g["route"] == route]):
        rows = np.nonzero(g["combo"] == combo)[0]
        i0 = rows[0]
        typ, M = int(g["typ"][i0]), int(g["max_read_len"][i0])
        sv = tuple(int(v) for v in g["schemes"][g["scheme"][i0]])
        assert band31_route(typ, sv, M) == route
        pats = [g["pats"][g["pat_off"][i]:g["pat_off"][i + 1]] for i in rows]
        txts = [g["txts"][g["txt_off"][i]:g["txt_off"][i + 1]] for i in rows]
        quals = [g["quals"][g["pat_off"][i]:g["pat_off"][i + 1]] for i in rows] if g["has_quals"][i0] else None
        L = range_layout(pats, txts, quals, flags=(np.arange(len(rows)) + combo) % 4)
        want = _oracle(orc, 31, typ, sv, L)
        ref = g["out"][rows]
        ok = ref[:, 0] == 1
        assert np.array_equal(want[0][ok], ref[ok, 1]) and np.array_equal(want[1][ok], ref[ok, 2:4]), combo
        assert (want[0][~ok] == amd.SCORE_MIN).all()
        for mrl in (M, 0):
            _check(_gpu(amd, orc, 31, typ, sv, L, mrl, 0), want, (int(combo), typ, sv, mrl))
        checked += len(rows)
    assert checked >= 40
