"""GPU: the reference kept as bit planes, one 128-byte line per window (nvbio_text_planes_build, nvbio_fm_index_text_planes,
nvbio_alignment_batch::text_planes_dev; NVBIO_ALN_NO_TEXT_PLANES switches the loader off).

The builder is compared line by line, padding included, with the numpy restatement of the layout in tests/test_text_planes_layout.py; the
handle's copy with the standalone builder's.  Band-31 end-to-end scoring is run three ways on the same batches -- with the planes, with the
planes and the flag, without planes -- and every way must equal the oracle.  The batches place a window at every tb mod 256 (every unit slot,
shift 0 and 63, the second half of a line), at tb = 0 and at the text's end (clipped: N < M + 30, N = M, N < M), and hold what each call site
of the loader takes: reads with 0-3 substitutions (first pass, second chance, the gap chance's third-chance join) and reads with one indel of
1-5 symbols as two neighbouring windows (the gap chance's pair walk) or as one window (its single walk).

The DP must not do the work: the routes of the run with planes (and of the run without) are read back, at least half of every batch's jobs
-- all of them, indel reads included; the batch of the quality route, where the gap chance does not run, is composed for that -- are
settled before the DP, and under 0 / -6 / -8 / -3 at least one job of each kind -- told apart on the CPU, from the mismatch counts of a
job's 31 diagonals and the oracle's score -- is settled: best diagonal with <= 1 mismatch (the first pass settles it: U* > G = -8), with 2
(second chance), with 3 (third-chance join, the single walk), every diagonal above the first pass's cap of 5 and the score in the gap chance's
class {-8, -11, -14, -17, -20}: with a partner in the same state (the pair walk; nvbio_banded_gap_pairs says who may pair) or without one
(the single walk)."""
import importlib

import numpy as np
import pytest

import oracle
from test_text_planes_layout import n_lines, planes_reference

pytestmark = pytest.mark.gpu

SCHEMES = ((0, 6, 6, -8, -3, -8, -3), (0, 2, 2, -5, -1, -5, -1), (0, 3, 3, -4, -2, -4, -2))
IN_CLASS = (-8, -11, -14, -17, -20)                                 # SCHEMES[0]: one gap of g <= 5 and e <= 2 mismatches below c_unk = 22
LENGTHS = (20, 100, 150, 161)
N_MAIN = 70001
SETTLED = 0


def _stored(read, fl):
    """the read as stored when the job's flags (bit 0 reverse, bit 1 complement) turn it back into `read`"""
    r = read[::-1] if fl & 1 else read
    return ((3 - r) if fl & 2 else r).astype(np.uint8)


def _batch(orc, text, M, seed, indel_every=1, more_subst=()):
    """jobs over `text`: per residue r of tb mod 256 two substitution reads, an indel read with its two windows (every 8th: one window only);
    then windows at tb = 0 and windows clipped by the text's end.  indel_every: the indel read at every so-manieth residue only; more_subst:
    per residue one more read with that many substitutions for every entry"""
    rng = np.random.default_rng(seed)
    n = len(text)
    reads, jobs, kind = [], [], []                                  # job = (read index, win_begin, win_end, flags); kind: 's' substitutions, 'i' indel

    def add(read, fl, windows, k):
        reads.append(_stored(read, fl))
        for wb, we in windows:
            jobs.append((len(reads) - 1, wb, we, fl)); kind.append(k)

    def subst(p0, k):
        r = text[p0:p0 + M].copy()
        pos = rng.choice(M, k, replace=False)
        r[pos] = (r[pos] + 1 + rng.integers(0, 3, k)) % 4
        return r

    def indel(p0, g, ins, k):
        at = int(rng.integers(M // 4, M - M // 4))
        src = text[p0:p0 + M + 8]
        r = np.concatenate([src[:at], rng.integers(0, 4, g, dtype=np.uint8), src[at:]]) if ins else np.concatenate([src[:at], src[at + g:]])
        r = r[:M].copy()
        if k:
            r[5] = (r[5] + 1) % 4
        return r, min(p0, p0 - g if ins else p0 + g), max(p0, p0 - g if ins else p0 + g)

    full = lambda wb: (wb, wb + M + 31)
    for r in range(256):
        wb = 20 + 257 * r                                           # tb mod 256 = 20 + r: every residue once
        fl = (r // 4) % 4
        add(subst(wb + 15, r % 4), fl, [full(wb)], "s")
        add(subst(wb + 15, (r // 16) % 4), (fl + 1) % 4, [full(wb)], "s")
        for k in more_subst:
            add(subst(wb + 15, k), (fl + 3) % 4, [full(wb)], "s")
        if r % indel_every:
            continue
        g = 1 + r % 5
        read, lo, hi = indel(wb + 15, g, bool((r // 5) % 2), 1 if r % 4 == 3 else 0)
        w = [full(lo - 15), full(hi - 15)]
        add(read, (fl + 2) % 4, w[:1] if r % 8 == 7 else (w if (r // 3) % 2 else w[::-1]), "i")
    # tb = 0
    add(subst(15, 1), 0, [full(0)], "s")
    add(subst(0, 0), 3, [full(0)], "s")
    read, lo, hi = indel(15, 2, False, 0)
    add(read, 0, [full(0), full(hi - 15)], "i")
    # the text's end: N = M + 10 (diagonals 0 .. 10 reportable), N = M (diagonal 0 alone), N = M - 3 (nothing reported)
    add(subst(n - M - 5, 1), 0, [(n - M - 10, n)], "s")
    add(subst(n - M - 10, 2), 2, [(n - M - 10, n)], "s")
    add(subst(n - M, 0), 1, [(n - M, n)], "s")
    add(subst(n - M, 3), 0, [(n - M, n)], "s")
    add(subst(n - M, 0)[:M], 0, [(n - M + 3, n)], "s")
    read, lo, hi = indel(n - M - 10, 3, True, 0)                    # both windows of the pair clipped
    add(read, 0, [(lo - 15, min(lo - 15 + M + 31, n)), (hi - 15, min(hi - 15 + M + 31, n))], "i")
    sym = np.concatenate(reads)
    roffs = (np.arange(len(reads) + 1) * M).astype(np.uint32)
    rid, wb, we, fl = (np.array([j[c] for j in jobs], dtype=t) for c, t in ((0, np.uint32), (1, np.uint32), (2, np.uint32), (3, np.uint8)))
    return dict(reads4=orc.pack4(sym), reads2=orc.pack2(sym), roffs=roffs, rid=rid, wb=wb, we=we, fl=fl, n=len(jobs), M=M, kind=np.array(kind),
                read_syms=reads)


def _diagonal_counts(text, d):
    """[jobs, 31] mismatches of every diagonal of the unclipped jobs (-1 in every column of a clipped one)"""
    M = d["M"]
    out = np.full((d["n"], 31), -1, dtype=np.int64)
    whole = np.nonzero(d["we"] - d["wb"] == M + 31)[0]
    for j in whole:
        r = d["read_syms"][d["rid"][j]]
        r = r[::-1] if d["fl"][j] & 1 else r
        r = 3 - r if d["fl"][j] & 2 else r
        win = text[int(d["wb"][j]):int(d["wb"][j]) + M + 31]
        out[j] = [(win[k:k + M] != r).sum() for k in range(31)]
    return out


@pytest.fixture(scope="module")
def main_text():
    return np.random.default_rng(12).integers(0, 4, N_MAIN, dtype=np.uint8)


def _planes_host(t):
    return t.cpu().numpy().view("<u8").reshape(-1, 8, 2)


class _DeviceBytes:
    """a device address as something torch.as_tensor can read (the CUDA array interface)"""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def test_builder_equals_the_layout_definition(amd, orc):
    import torch
    rng = np.random.default_rng(3)
    for n in (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 70001):
        sym = rng.integers(0, 4, n, dtype=np.uint8)
        want = planes_reference(sym)
        assert amd.text_planes_bytes(n) == n_lines(n) * 128 == want.nbytes
        words = torch.from_numpy(orc.pack2(sym).view(np.int32)[:(n + 15) // 16].copy()).cuda()      # exactly the words the text has
        out = torch.full((want.nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
        got = _planes_host(amd.build_text_planes(words, n, out=out))
        bad = np.nonzero((got != want).any(axis=(1, 2)))[0]
        assert len(bad) == 0, (n, bad[:5], got[bad[:1]], want[bad[:1]])
        if n >= 255:
            # the handle's copy (a handle that keeps the text: sa_int = 1), and the opt-out
            fmi = amd.FMIndex.build(words, n, kmer_len=0, sa_int=1)
            ptr, length = fmi.text_planes()
            assert length == n and ptr % 128 == 0
            mine = torch.as_tensor(_DeviceBytes(ptr, want.nbytes), device="cuda").clone()
            assert np.array_equal(_planes_host(mine), want), n
            assert fmi.text_planes_of(words, n) == ptr and fmi.text_planes_of(words.clone(), n) is None and fmi.text_planes_of(words, n - 1) is None
            with_planes = fmi.device_bytes()
            fmi.close()
            bare = amd.FMIndex.build(words, n, kmer_len=0, sa_int=1, table_flags=amd.FM_TABLE_NO_TEXT_PLANES)
            assert bare.text_planes() is None and with_planes - bare.device_bytes() == want.nbytes
            bare.close()
            sampled = amd.FMIndex.build(words, n, kmer_len=0, sa_int=16)                             # keeps no text: no planes
            assert sampled.text_planes() is None
            sampled.close()
    # a buffer that is not 128-byte aligned is refused
    buf = torch.zeros(amd.text_planes_bytes(1000) + 128, dtype=torch.uint8, device="cuda")
    sym = rng.integers(0, 4, 1000, dtype=np.uint8)
    with pytest.raises(amd.NvbioError, match="128-byte aligned"):
        amd.build_text_planes(orc.pack2(sym), 1000, out=buf[64:])
    with pytest.raises(amd.NvbioError, match="128-byte aligned"):
        amd.batch_banded_alignment_score(31, amd.make_gotoh_aligner(oracle.SEMI_GLOBAL, amd.GotohScheme(*SCHEMES[0])),
                                         amd.AlignmentBatch(orc.pack4(sym[:150]), 4, np.array([0, 150], dtype=np.uint32), orc.pack2(sym), 2,
                                                            np.array([10], dtype=np.uint32), np.array([191], dtype=np.uint32), max_read_len=150,
                                                            text_planes=buf[64:]))


def _three_ways(amd, d, text2, planes, rbits, quals=None):
    mk = lambda tp, algo: amd.AlignmentBatch(d["reads4"] if rbits == 4 else d["reads2"], rbits, d["roffs"], text2, 2, d["wb"], d["we"], read_id=d["rid"],
                                             flags=d["fl"], max_read_len=d["M"], algo_flags=algo, text_planes=tp, quals=quals)
    return (("planes", mk(planes, 0)), ("flagged", mk(planes, amd.ALN_NO_TEXT_PLANES)), ("no planes", mk(None, 0)))


def _check_scores(amd, tag, d, ways, sv, want):
    """every way equals the oracle; returns {way: routes}"""
    routes = {}
    for way, batch in ways:
        sc, sk, rt = amd.banded_gotoh_score_routes(31, amd.make_gotoh_aligner(oracle.SEMI_GLOBAL, amd.GotohScheme(*sv)), batch)
        sc, sk, routes[way] = sc.cpu().numpy(), amd.u32(sk), rt.cpu().numpy()
        bad = np.nonzero((sc != want[0]) | (sk != want[1]).any(axis=1))[0]
        assert len(bad) == 0, (tag, sv, way, len(bad), bad[:5], d["wb"][bad[:5]], d["we"][bad[:5]], sc[bad[:5]], want[0][bad[:5]], sk[bad[:5]], want[1][bad[:5]])
    return routes


def test_band31_scoring_with_planes_equals_the_oracle_three_ways(amd, orc, main_text):
    import torch
    assert amd.ALN_NO_TEXT_PLANES == 1048576
    # the whole grid on the 70 001-symbol text; texts that end 0, 1 and 255 symbols into a line: M = 150, 4-bit reads, the first scheme
    texts = [(N_MAIN, LENGTHS, (4, 2), SCHEMES)] + [(n, (150,), (4,), SCHEMES[:1]) for n in (69888, 69889, 69887)]
    for n, lengths, bits, schemes in texts:
        text = main_text[:n]
        assert n % 256 == {N_MAIN: N_MAIN % 256, 69888: 0, 69889: 1, 69887: 255}[n]
        text2 = torch.from_numpy(orc.pack2(text).view(np.int32)).cuda()
        planes = amd.build_text_planes(text2, n)
        for M in lengths:
            d = _batch(orc, text, M, 100 + M)
            N = d["we"] - d["wb"]
            assert set((d["wb"] % 256).tolist()) == set(range(256)) and (d["wb"] == 0).sum() >= 3
            assert ((N < M + 30) & (N > M)).any() and (N == M).any() and (N < M).any() and (d["we"] == n).sum() >= 6
            cnt = _diagonal_counts(text, d)
            best = np.where(cnt[:, 0] >= 0, cnt.min(axis=1), -1)
            for sv in schemes:
                want = orc.banded_gotoh_packed_batch(31, oracle.SEMI_GLOBAL, oracle.Scheme(*sv), d["reads4"], d["roffs"], orc.pack2(text), d["wb"], d["we"],
                                                     read_id=d["rid"], flags=d["fl"])
                for rbits in bits:
                    tag = "n %d M %d bits %d" % (n, M, rbits)
                    ways = _three_ways(amd, d, text2, planes, rbits)
                    routes = _check_scores(amd, tag, d, ways, sv, want)
                    for way in ("planes", "no planes"):
                        settled = routes[way] == SETTLED
                        print(tag, sv, way, "jobs", d["n"], "settled before the DP", int(settled.sum()))
                        assert 2 * int(settled.sum()) >= d["n"], (tag, sv, way, int(settled.sum()), d["n"])
                        if sv != SCHEMES[0]:
                            continue
                        partner = amd.u32(amd.banded_gap_pairs(ways[0][1]))
                        far = (best > 5) & np.isin(want[0], IN_CLASS)                    # flagged for the gap chance, and inside its class
                        has = partner != amd.NO_PARTNER
                        paired = far & has & far[np.where(has, partner, 0)]
                        kinds = {"first pass": (best >= 0) & (best <= 1), "second chance": (best == 2) & (want[0] == -12),
                                 "third-chance join": (best == 3) & (want[0] == -18), "gap chance, single": far & ~has, "gap chance, pair": paired}
                        for name, sel in kinds.items():
                            print("   ", name, int(sel.sum()), "settled", int((sel & settled).sum()))
                            assert (sel & settled).any(), (tag, way, name, int(sel.sum()))


def test_band31_scoring_with_planes_under_a_quality_ramp(amd, orc, main_text):
    import torch
    text, M = main_text, 150
    # Under a ramp the gap chance does not run, so an indel read cannot be settled before the DP: this batch has the indel read (its two
    # windows) at every 4th residue only and, per residue, two more substitution reads with 0 and 1 substitutions.
    d = _batch(orc, text, M, 77, indel_every=4, more_subst=(0, 1))
    assert set((d["wb"] % 256).tolist()) == set(range(256)) and (d["kind"] == "i").sum() >= 100
    quals = np.random.default_rng(78).integers(0, 45, len(d["read_syms"]) * M).astype(np.uint8)
    sv = (0, 2, 6, -5, -3, -5, -3)                                  # nvBowtie's ramp: the penalty of a mismatch depends on the base quality
    # told on the CPU: a job one of whose diagonals costs less than a gap (U* > G = -5: no, one cheap or two cheapest mismatches) is settled
    # by the first pass itself; the inputs are chosen so that these alone are half of the batch
    pen = np.array([-orc.mismatch(oracle.Scheme(*sv), q) for q in range(64)])
    sure = np.zeros(d["n"], dtype=bool)
    for j in np.nonzero(d["we"] - d["wb"] == M + 31)[0]:
        r, q = d["read_syms"][d["rid"][j]], quals[int(d["rid"][j]) * M:int(d["rid"][j]) * M + M]
        r, q = (r[::-1], q[::-1]) if d["fl"][j] & 1 else (r, q)
        r = 3 - r if d["fl"][j] & 2 else r
        win = text[int(d["wb"][j]):int(d["wb"][j]) + M + 31]
        sure[j] = min(int(pen[q[win[k:k + M] != r]].sum()) for k in range(31)) < 5
    print("qualities: jobs", d["n"], "substitution jobs", int((d["kind"] == "s").sum()), "settled by the first pass for sure", int(sure.sum()))
    assert 2 * int(sure.sum()) >= d["n"]
    text2 = torch.from_numpy(orc.pack2(text).view(np.int32)).cuda()
    planes = amd.build_text_planes(text2, len(text))
    want = orc.banded_gotoh_packed_batch(31, oracle.SEMI_GLOBAL, oracle.Scheme(*sv), d["reads4"], d["roffs"], orc.pack2(text), d["wb"], d["we"],
                                         read_id=d["rid"], flags=d["fl"], quals=quals)
    routes = _check_scores(amd, "qualities", d, _three_ways(amd, d, text2, planes, 4, quals=quals), sv, want)
    for way in ("planes", "no planes"):
        settled = routes[way] == SETTLED
        print("qualities", way, "jobs", d["n"], "settled before the DP", int(settled.sum()), "of the sure ones", int((sure & settled).sum()))
        assert 2 * int(settled.sum()) >= d["n"], (way, int(settled.sum()), d["n"])


def test_band31_scoring_reads_the_planes_it_is_given(amd, orc, main_text):
    """The three ways above would agree even if the planes were never read.  Here the batch carries the packed words of one text and the
    planes of ANOTHER (every 160th symbol changed: one more mismatch on nearly every diagonal of 150 rows): whatever is settled before the DP has looked at the
    planes alone and must score as the oracle does on the other text, which differs from the score on the first; under the flag the planes
    are not looked at and every score is the first text's."""
    import torch
    text, M, sv = main_text, 150, SCHEMES[0]
    other = text.copy()
    other[50::160] = (other[50::160] + 1) % 4
    d = _batch(orc, text, M, 500)
    text2 = torch.from_numpy(orc.pack2(text).view(np.int32)).cuda()
    planes_other = amd.build_text_planes(torch.from_numpy(orc.pack2(other).view(np.int32)).cuda(), len(other))
    want, want_other = (orc.banded_gotoh_packed_batch(31, oracle.SEMI_GLOBAL, oracle.Scheme(*sv), d["reads4"], d["roffs"], orc.pack2(t), d["wb"], d["we"],
                                                      read_id=d["rid"], flags=d["fl"]) for t in (text, other))
    aligner = amd.make_gotoh_aligner(oracle.SEMI_GLOBAL, amd.GotohScheme(*sv))
    (_, mixed), (_, flagged), _ = _three_ways(amd, d, text2, planes_other, 4)
    sc, sk, rt = amd.banded_gotoh_score_routes(31, aligner, mixed)
    sc, sk, settled = sc.cpu().numpy(), amd.u32(sk), rt.cpu().numpy() == SETTLED
    # told on the CPU: a job whose best diagonal on the other text has at most one mismatch is settled by the first pass (U* > G = -8); the
    # exact reads are such jobs, with one mismatch there and none on the batch's text
    cnt = _diagonal_counts(other, d)
    sure = (cnt[:, 0] >= 0) & (cnt.min(axis=1) <= 1) & (want[0] != want_other[0])
    differ = settled & (want[0] != want_other[0])
    print("planes of another text: jobs", d["n"], "settled", int(settled.sum()), "of them with another score than on the batch's text", int(differ.sum()),
          "sure", int(sure.sum()))
    assert sure.sum() >= 50 and settled[sure].all()
    bad = np.nonzero(settled & ((sc != want_other[0]) | (sk != want_other[1]).any(axis=1)))[0]
    assert len(bad) == 0, (len(bad), bad[:5], sc[bad[:5]], want_other[0][bad[:5]], want[0][bad[:5]])
    sc, sk, _ = amd.banded_gotoh_score_routes(31, aligner, flagged)
    assert np.array_equal(sc.cpu().numpy(), want[0]) and np.array_equal(amd.u32(sk), want[1])


def test_band31_traceback_with_and_without_planes(amd, orc, main_text):
    import torch
    text = main_text
    text2 = torch.from_numpy(orc.pack2(text).view(np.int32)).cuda()
    planes = amd.build_text_planes(text2, len(text))
    sv = SCHEMES[0]
    aligner = amd.make_gotoh_aligner(oracle.SEMI_GLOBAL, amd.GotohScheme(*sv))
    for M in LENGTHS:
        d = _batch(orc, text, M, 300 + M)
        want = orc.banded_gotoh_packed_batch(31, oracle.SEMI_GLOBAL, oracle.Scheme(*sv), d["reads4"], d["roffs"], orc.pack2(text), d["wb"], d["we"],
                                             read_id=d["rid"], flags=d["fl"])
        for rbits in (4, 2):
            outs = [amd.BatchedBandedAlignmentTraceback(31, aligner).enact(batch, cigar_stride=32) for _, batch in _three_ways(amd, d, text2, planes, rbits)]
            assert np.array_equal(outs[0][0].cpu().numpy(), want[0]), (M, rbits)
            lens = outs[0][4].cpu().numpy().view(np.uint32)
            ungapped = int((lens == 1).sum())                       # one CIGAR element: a diagonal, written by the ungapped traceback
            print("traceback M", M, "bits", rbits, "jobs", d["n"], "one-element CIGARs", ungapped)
            assert 3 * ungapped >= d["n"]
            for other in outs[1:]:
                for a, b, what in zip(outs[0], other, ("score", "source", "sink", "cigar", "cigar_len")):
                    assert torch.equal(a, b), (M, rbits, what)


def test_seed_and_extend_uses_the_handles_planes_only_with_its_own_text(amd, orc):
    import torch
    pipeline = importlib.import_module("nvbio_gpl_amd.pipeline")
    rng = np.random.default_rng(41)
    G, R, M = 300_000, 3000, 150
    text = rng.integers(0, 4, G, dtype=np.uint8)
    starts = rng.integers(0, G - M - 8, R)
    reads = np.empty((R, M), dtype=np.uint8)
    for i, s in enumerate(starts):
        w = text[s:s + M + 8].copy()
        mut = rng.random(M + 8) < 0.01
        w[mut] = (w[mut] + 1 + rng.integers(0, 3, int(mut.sum()))) % 4
        if i % 5 == 0:
            p = int(rng.integers(30, 120))
            w = np.delete(w, p) if i % 10 == 0 else np.insert(w, p, rng.integers(0, 4))
        reads[i] = w[:M]
    rcm = rng.random(R) < 0.5
    reads[rcm] = 3 - reads[rcm][:, ::-1]
    g_dev = torch.from_numpy(orc.pack2(text).view(np.int32)).cuda()
    fmi = amd.FMIndex.build(g_dev, G, kmer_len=11, sa_int=1, table_flags=amd.FM_TABLE_CANONICAL_WIDE)
    assert fmi.text_planes() is not None
    rb = pipeline.ReadBatch(torch.from_numpy(orc.pack4(reads.reshape(-1)).view(np.int32)).cuda(), R, M)

    def run(genome, algo):
        params = pipeline.SeedExtendParams.end_to_end(seed_len=16)
        params.mapq, params.algo_flags = True, algo
        extras, seen = {}, []

        class Recorded(amd.AlignmentBatch):                         # what the extension's batches were given
            def __init__(self, *a, **kw):
                seen.append(kw.get("text_planes"))
                super().__init__(*a, **kw)

        real, pipeline.AlignmentBatch = pipeline.AlignmentBatch, Recorded
        try:
            out = pipeline.seed_and_extend(fmi, genome, G, rb, params, return_windows=True, extras=extras)
        finally:
            pipeline.AlignmentBatch = real
        amd.FinishStatus.of(g_dev.device).check(wait=True)
        assert len(seen) >= 1 and len(set(seen)) == 1 and "text_planes" not in extras
        used = seen[0]
        assert used == fmi.text_planes_of(genome, G)
        tb = pipeline.traceback_best_all(genome, G, rb, params, extras["best_keys"], out[4], text_planes=used)
        return out, extras, used, tb

    with_planes, flagged, elsewhere = run(g_dev, 0), run(g_dev, amd.ALN_NO_TEXT_PLANES), run(g_dev.clone(), 0)
    assert with_planes[2] == fmi.text_planes()[0] and flagged[2] == with_planes[2]
    assert elsewhere[2] is None                                     # a clone at another address: not the text the handle was built from
    assert with_planes[0][3] > 0 and int((with_planes[0][0] > amd.SCORE_MIN).sum()) > R // 2
    for other in (flagged, elsewhere):
        assert with_planes[0][3] == other[0][3]
        for a, b in zip(with_planes[0][:3] + with_planes[0][4:], other[0][:3] + other[0][4:]):
            assert torch.equal(a, b)
        assert set(with_planes[1]) == set(other[1]) and {"mapq", "second_score", "second", "best_keys"} <= set(other[1])
        for k in with_planes[1]:
            assert torch.equal(with_planes[1][k], other[1][k]), k
        for a, b in zip(with_planes[3], other[3]):
            assert torch.equal(a, b)
    fmi.close()
