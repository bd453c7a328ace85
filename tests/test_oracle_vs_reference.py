"""Fuzz of the oracle against the reference's own host code: live where oracle/_ref is built (oracle/Makefile, from the
reference sources), elsewhere against what that code returned for the same calls (tests/golden/ref_fuzz_golden.npz, the
fixture `ref`).  Regenerate the recording with tests/golden/make_golden.py whenever these tests change."""
import numpy as np
import pytest

import oracle
from util import (E2E31_CORNERS, E2E31_SWEEP, FULL_KINDS, FULL_LIMIT_CUT_SCHEME, LIMIT_SCHEMES, RANGE_KINDS, e2e31_sweep_jobs, flat_scheme, full_jobs,
                  full_limit_jobs, full_shapes, limit_jobs, limit_thin, range_jobs)

SCHEMES = [oracle.Scheme.simple(2, -1, -1, -1), oracle.Scheme.simple(0, -5, -8, -3),
           oracle.Scheme.simple(2, -1, -2, -1), oracle.Scheme(2, 2, 6, -8, -3, -8, -3),
           oracle.Scheme(0, 2, 6, -8, -3, -8, -3), oracle.Scheme(1, 3, 3, -15, -4, -11, -2)]


def test_fm_index_fuzz(orc, ref):
    rng = np.random.default_rng(7)
    for n in (1, 2, 15, 16, 17, 63, 64, 65, 1000, 4097, 50000):
        text = rng.integers(0, 4, n, dtype=np.uint8)
        if n == 1000:
            text[:] = 0
        if n == 4097:
            text = np.tile(np.array([0, 1, 2, 3, 3, 2], dtype=np.uint8), 700)[:n]
        ri, oi = ref.build_index(text), orc.build_index(text)
        assert np.array_equal(ri.sa[1:], oi.sa[1:])
        assert ri.primary == oi.primary and np.array_equal(ri.L2, oi.L2) and np.array_equal(ri.ssa, oi.ssa)
        ks = list(range(-1, min(n, 200) + 1)) + [int(x) for x in rng.integers(0, n + 1, 100)]
        for k in ks:
            for c in range(4):
                assert ref.rank(ri, k, c) == orc.rank(oi, k, c)
        for _ in range(200):
            l = int(rng.integers(-1, n + 1)); r = int(rng.integers(max(l, 0), n + 1)); c = int(rng.integers(0, 4))
            assert np.array_equal(ref.rank2(ri, l, r, c), orc.rank2(oi, l, r, c))
        Q = 300
        lens = rng.integers(1, 30, Q)
        offs = np.zeros(Q + 1, dtype=np.uint32); offs[1:] = np.cumsum(lens)
        syms = rng.integers(0, 4, int(offs[-1]), dtype=np.uint8)
        for q in range(0, Q, 2):
            if lens[q] <= n:
                p = int(rng.integers(0, n - lens[q] + 1)); syms[offs[q]:offs[q + 1]] = text[p:p + lens[q]]
        syms[rng.integers(0, len(syms), 10)] = 4
        for rev in (False, True):
            assert np.array_equal(ref.match_batch(ri, syms, offs, rev), orc.match_batch(oi, syms, offs, rev))
        rows = rng.integers(0, n + 1, 200).astype(np.uint32)
        assert np.array_equal(ref.locate_batch(ri, rows), orc.locate_batch(oi, rows))
        ref.destroy(ri)


def test_gotoh_fuzz(orc, ref):
    rng = np.random.default_rng(11)
    for it in range(600):
        band = [3, 7, 15, 31][it % 4]
        M = int(rng.integers(1, 160))
        N = int(rng.integers(max(M, band - 1), M + band + 10))
        if it % 7 == 0:
            N = max(band - 1, int(rng.integers(max(1, M - 3), M + 2)))
        txt = rng.integers(0, 4, N, dtype=np.uint8)
        st = int(rng.integers(0, max(1, N - M + 1)))
        pat = txt[st:st + M].copy()
        if len(pat) < M:
            pat = np.concatenate([pat, rng.integers(0, 4, M - len(pat), dtype=np.uint8)])
        mut = rng.random(M) < 0.08
        pat[mut] = rng.integers(0, 5, int(mut.sum()))
        quals = rng.integers(0, 60, M, dtype=np.uint8) if it % 2 else None
        sc = SCHEMES[it % len(SCHEMES)]
        for typ in range(3):
            assert ref.banded_gotoh(band, typ, sc, pat, txt, quals) == orc.banded_gotoh(band, typ, sc, pat, txt, quals)
            if quals is None:   # edit distance == Gotoh(0, -1, -1, -1) (ed/ed_banded_inl.h:37-69 -> sw/sw_banded_inl.h)
                assert ref.banded_ed(band, typ, pat, txt) == orc.banded_gotoh(band, typ, oracle.Scheme(*oracle.ED_SCHEME), pat, txt)
            # traceback: Alignment {score, source, sink}, the op string and the clips (banded_inl.h:354-417)
            r, rs, rsrc, rsnk, rops, rclips = ref.banded_gotoh_traceback(band, typ, sc, pat, txt, quals)
            ok, s, src, snk, cig, ops = orc.banded_gotoh_traceback(band, typ, sc, pat, txt, quals)
            assert (ok, s, src, snk) == (1 if r == 2 else 0, rs, rsrc, rsnk), (it, typ)
            assert np.array_equal(ops, rops), (it, typ)
            assert np.array_equal(cig, oracle.cigar_from_ops(rops, *rclips) if r == 2 else np.zeros(0, dtype=np.uint16)), (it, typ)
            ms = oracle.SCORE_MIN if it % 3 else int(rng.integers(-50, 200))
            # full-matrix traceback (alignment_inl.h:355-455)
            r, rs, rsrc, rsnk, rops, rclips = ref.full_gotoh_traceback(typ, sc, pat, txt, quals, ms)
            ok, s, src, snk, cig = orc.full_gotoh_traceback(typ, sc, pat, txt, quals, ms)
            assert (ok, s, src, snk) == (1 if r == 2 else 0, rs, rsrc, rsnk), (it, typ)
            assert np.array_equal(cig, oracle.cigar_from_ops(rops, *rclips) if r == 2 else np.zeros(0, dtype=np.uint16)), (it, typ)
            for blk in range(2):
                assert ref.full_gotoh(typ, blk, sc, pat, txt, quals, ms) == orc.full_gotoh(typ, blk, sc, pat, txt, quals, ms)


def test_gotoh_long_fuzz(orc, ref):
    """band 31 on patterns of 200 to 8,000 symbols, the lengths at which the library changes its arithmetic among them: one round of
    the kinds of tests/util.py (all-mismatch, perfect, shifted to the band's rim, one gap of up to 30 symbols, mutated, N's, random,
    clipped windows) per length, schemes whose scores run to -8,000, to 45,000 and past the reference's int16 stand-in for minus
    infinity, qualities on every other job"""
    schemes = SCHEMES[3:] + [oracle.Scheme(*flat_scheme(0, 8)), oracle.Scheme(*flat_scheme(0, 1)), oracle.Scheme(*flat_scheme(1, 1)),
                             oracle.Scheme(9, 2, 60, -8, -3, -8, -3), oracle.Scheme(0, 2, 8, -8, -3, -8, -3)]
    rng = np.random.default_rng(13)
    for li, M in enumerate((200, 223, 224, 500, 968, 969, 1000, 2009, 3000, 5000, 7968, 8000)):
        jobs = len(RANGE_KINDS) if M <= 1000 else 6
        pats, txts, kinds = range_jobs(300 + li, [M] * jobs, 31, first=5 * li)
        for j in range(jobs):
            quals = rng.integers(0, 64, M, dtype=np.uint8) if j % 2 else None
            sc = schemes[(li + j) % len(schemes)]
            for typ in range(3):
                assert ref.banded_gotoh(31, typ, sc, pats[j], txts[j], quals) == orc.banded_gotoh(31, typ, sc, pats[j], txts[j], quals), (M, kinds[j], typ)


def test_traceback_limit_fuzz(orc, ref):
    """the banded traceback on a thinned round of the generator of tests/test_gpu_traceback_routes.py: one job of every kind, read length,
    window length and overhang (fill and diagonal) under every scheme of util.LIMIT_SCHEMES, end to end; the overhang jobs, where the
    reference reads the sentinel past a clipped window's end, under LOCAL and GLOBAL as well"""
    J = limit_jobs(20261)
    idx = limit_thin(J)
    kinds = set(J["kind"][idx])
    assert kinds == set(J["kind"]) and len(idx) >= 60 and {(int(m), int(w)) for m, w in zip(J["M"][idx], J["win"][idx])} >= {
        (33, 31), (64, 31), (64, 30), (64, 29), (160, 31), (161, 31), (162, 31)}
    traced_past_end = 0
    for name, sv, with_q in LIMIT_SCHEMES:
        sc = oracle.Scheme(*sv)
        for j in idx:
            pat, txt, quals = J["pats"][j], J["txts"][j], J["quals"][j] if with_q else None
            for typ in ((oracle.SEMI_GLOBAL, oracle.LOCAL, oracle.GLOBAL) if J["kind"][j] == "overhang" else (oracle.SEMI_GLOBAL,)):
                r, rs, rsrc, rsnk, rops, rclips = ref.banded_gotoh_traceback(31, typ, sc, pat, txt, quals)
                ok, s, src, snk, cig, ops = orc.banded_gotoh_traceback(31, typ, sc, pat, txt, quals)
                assert (ok, s, src, snk) == (1 if r == 2 else 0, rs, rsrc, rsnk), (name, j, typ)
                assert np.array_equal(ops, rops), (name, j, typ)
                assert np.array_equal(cig, oracle.cigar_from_ops(rops, *rclips) if r == 2 else np.zeros(0, dtype=np.uint16)), (name, j, typ)
                traced_past_end += int(ok and snk[0] > len(txt))
    assert traced_past_end >= 5                                                 # LOCAL sinks on the sentinel, read as 3


def test_e2e31_scheme_sweep(orc, ref):
    """band 31, SEMI_GLOBAL, under every scheme of the sweep of tests/test_gpu_band31_scheme_sweep.py -- the 138 of util.E2E31_SWEEP and the
    corners of util.E2E31_CORNERS, the ramps with the pool's qualities -- on every 40th job of its pool: a mismatch that costs nothing, a gap
    extension that costs nothing, an opening cheaper than an extension, P = 30 against gaps of 2 and 1.  ok, score and sink are equal"""
    J = e2e31_sweep_jobs(1)
    idx = range(0, len(J["pats"]), 40)
    assert len(idx) >= 100 and len(set(J["kind"][list(idx)])) >= 12
    cases = 0
    for sv, with_q in [(sv, False) for sv in E2E31_SWEEP] + [(c[1], c[2]) for c in E2E31_CORNERS]:
        sc = oracle.Scheme(*sv)
        for j in idx:
            pat, txt, quals = J["pats"][j], J["txts"][j], J["quals"][j] if with_q else None
            assert ref.banded_gotoh(31, oracle.SEMI_GLOBAL, sc, pat, txt, quals) == orc.banded_gotoh(31, oracle.SEMI_GLOBAL, sc, pat, txt, quals), (sv, j)
            cases += 1
    assert cases >= 138 * 100


def test_full_traceback_limit_fuzz(orc, _live_ref):
    """the full-matrix traceback on a thinned round of the generator of tests/test_gpu_full_traceback_routes.py: one job of every kind, read
    length, window length and gap column, every short-text job and the reads of 249..252 symbols at the G <= 250 cut, end to end under every
    scheme of util.LIMIT_SCHEMES (the last under their own as well); the short texts, where the implicit first row and column supply the
    alignment's ends, under LOCAL and GLOBAL too.  Live only: it pins the oracle that the GPU tests compare with"""
    if _live_ref is None:
        pytest.skip("needs the reference's own host code (oracle/_ref)")
    J = full_limit_jobs(20262)
    short, cut = np.char.startswith(J["kind"], "short"), J["kind"] == "cut"
    idx = sorted(set(limit_thin(J).tolist()) | set(np.nonzero(short | cut)[0].tolist()))
    assert set(J["kind"][idx]) == set(J["kind"]) and len(idx) >= 250 and max(len(J["pats"][j]) for j in idx) <= 256
    assert {(int(m), int(w)) for m, w in zip(J["M"][idx], J["W"][idx])} >= {(64, 13), (64, 14), (64, 15), (64, 22), (64, 40), (1, 15), (7, 15), (8, 22),
                                                                           (9, 15), (65, 22), (64, -1), (64, -9), (20, -10), (64, -63), (250, 20), (251, 20)}
    checked = sink_above = 0
    for name, sv, with_q in LIMIT_SCHEMES + (FULL_LIMIT_CUT_SCHEME,):
        sc = oracle.Scheme(*sv)
        for j in (idx if name != "cut" else np.nonzero(cut)[0]):
            pat, txt, quals = J["pats"][j], J["txts"][j], J["quals"][j] if with_q else None
            for typ in ((oracle.SEMI_GLOBAL, oracle.LOCAL, oracle.GLOBAL) if short[j] else (oracle.SEMI_GLOBAL,)):
                r, rs, rsrc, rsnk, rops, rclips = _live_ref.full_gotoh_traceback(typ, sc, pat, txt, quals)
                ok, s, src, snk, cig = orc.full_gotoh_traceback(typ, sc, pat, txt, quals)
                assert (ok, s, src, snk) == (1 if r == 2 else 0, rs, rsrc, rsnk), (name, j, typ)
                assert np.array_equal(cig, oracle.cigar_from_ops(rops, *rclips) if r == 2 else np.zeros(0, dtype=np.uint16)), (name, j, typ)
                ops = np.concatenate([np.full(int(c) >> 2, int(c) & 3, dtype=np.uint8) for c in cig if int(c) & 3 != 3] + [np.zeros(0, dtype=np.uint8)])
                assert np.array_equal(ops, rops), (name, j, typ)
                checked += 1; sink_above += int(ok and snk[0] < snk[1])
    assert checked >= 1500 and sink_above >= 300                                # (sinks with x < y: the short texts)


def test_full_gotoh_range_fuzz(orc, _live_ref):
    """full-matrix Gotoh, both blockings, on the generator of tests/test_gpu_full_range.py: a round of its kinds at either side of the packed
    and the cooperative bounds, past them and beyond int16, where the result is what the short2 boundary column leaves of it.  Live only:
    patterns of 4,000 rows make too large a recording"""
    if _live_ref is None:
        pytest.skip("needs the reference's own host code (oracle/_ref)")
    G, L, SG = oracle.GLOBAL, oracle.LOCAL, oracle.SEMI_GLOBAL
    shapes = ((G, flat_scheme(0, 8), 9, 1491), (G, flat_scheme(0, 8), 24, 1477), (G, flat_scheme(8, 8), 24, 1476), (G, flat_scheme(0, 1), 9, 11992),
              (SG, flat_scheme(0, 8), 24, 1476), (SG, flat_scheme(3, 8), 9, 1492), (L, (2, 3, 3, -5, -2, -5, -2), 1001, 1041),
              (L, (20, 6, 6, -8, -3, -8, -3), 100, 140), (G, flat_scheme(0, 8), 8, 3740), (G, flat_scheme(0, 8), 256, 3493),
              (SG, flat_scheme(3, 8), 256, 3492), (G, flat_scheme(0, 8), 8, 3867), (L, (2, 3, 3, -5, -2, -5, -2), 1024, 1064),
              (G, flat_scheme(0, 8), 8, 4200), (G, flat_scheme(0, 8), 8, 4500), (L, (9, 2, 60, -8, -3, -8, -3), 4000, 4040),
              (SG, flat_scheme(0, 8), 4200, 4230), (G, (2, 2, 6, -8, -3, -8, -3), 3000, 6000))
    rng = np.random.default_rng(17)
    beyond = 0
    for si, (typ, sv, M, N) in enumerate(shapes):
        jobs = len(FULL_KINDS) if M * N <= 400000 else 5
        pats, txts, kinds = full_jobs(500 + si, full_shapes(si, M, N, jobs), first=3 * si)
        for j in range(jobs):
            quals = rng.integers(0, 64, len(pats[j]), dtype=np.uint8) if j % 2 else None
            ms = oracle.SCORE_MIN if j % 3 else int(rng.integers(-200, 200))
            for blk in range(2):
                got = orc.full_gotoh(typ, blk, oracle.Scheme(*sv), pats[j], txts[j], quals, ms)
                assert _live_ref.full_gotoh(typ, blk, oracle.Scheme(*sv), pats[j], txts[j], quals, ms) == got, (typ, sv, M, N, kinds[j], blk)
                beyond += int(abs(got[1]) > 30000 and got[1] != oracle.SCORE_MIN)
    assert beyond >= 20


def test_whole_path_oracle_equals_reference_code(orc, ref):
    """the CPU composition used as bench.py's baseline: the oracle's functions and the reference's own
    host templates (on an adopted index) give the same best alignment for every read"""
    from oracle import cpu_pipeline
    rng = np.random.default_rng(3)
    G = 300000
    text = rng.integers(0, 4, G, dtype=np.uint8)
    text[1000:1500] = text[200000:200500]
    hidx = orc.build_index(text)
    ridx = ref.adopt_index(oracle.HostIndex(hidx.n, hidx.primary, hidx.L2, hidx.bwt_occ, hidx.ssa))
    R, M = 2000, 150
    starts = rng.integers(0, G - M, R)
    starts[:40] = rng.integers(1000, 1300, 40)
    reads = np.stack([text[s:s + M] for s in starts]).copy()
    reads[rng.random(reads.shape) < 0.02] = 2
    rc = rng.random(R) < 0.5
    reads[rc] = 3 - reads[rc][:, ::-1]
    a = cpu_pipeline.seed_and_extend_cpu(orc, hidx, text, G, reads)
    b = cpu_pipeline.seed_and_extend_ref(ref, orc, ridx, orc.pack2(text), G, reads)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    assert a[3] == b[3]
    ref.destroy(ridx)


def test_seed_hit_deque_fuzz(orc, ref):
    """live: the oracle's interval heap against the reference's priority_deque on fresh random operation sequences"""
    rng = np.random.default_rng(77)
    for t in range(1500):
        n = int(rng.integers(1, 120)); mh = int(rng.integers(1, 40))
        ops = rng.choice([0, 0, 0, 1, 2, 3, 3], n).astype(np.uint32)
        begins = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        sizes = rng.choice([1, 1, 1, 2, 7, 300], n).astype(np.uint32)
        bits = (sizes | (rng.integers(0, 1024, n).astype(np.uint32) << 20)).astype(np.uint32)
        h1, r1 = orc.hit_deque_run(ops, begins, bits, mh)
        h2, r2 = ref.hit_deque_run(ops, begins, bits, mh)
        assert np.array_equal(h1, h2) and np.array_equal(r1, r2), t
