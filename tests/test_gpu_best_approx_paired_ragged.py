"""GPU parity of nvBowtie's PAIRED best-approx loop over mates of DIFFERENT lengths (pipeline.nvbowtie_best_approx_paired_host over ReadBatches with
offsets; nvbio_pe_*_ragged, host/nvbio_amd/best_approx.hpp: best_approx_paired_ragged) against the pass-by-pass restatement
(tests/best_approx_paired_ragged_cpu.py, pinned without a GPU by tests/test_best_approx_paired_ragged_oracle.py).  The shared pairs hold mates below
min_read_len and below seed_len (filtered as anchors, aligned as opposite mates), with exactly one seed, at the 10-bit position limit (1023: the
unpaired fallback and a window shorter than the pattern), inside a 12-copy repeat, at both genome ends, with the second mate elsewhere, and unalignable
ones."""
import importlib

import numpy as np
import pytest

import oracle
from best_approx_paired_ragged_cpu import KW, MODES, PLAIN, SETTINGS, genome_and_index, long_input, make_pairs, pe_kw, restatement, shared_input, stored_stream

pytestmark = pytest.mark.gpu

OSC = oracle.Scheme(0, 6, 6, -8, -3, -8, -3)


@pytest.fixture(scope="module")
def device_genome(amd, orc):
    import torch
    pipeline = importlib.import_module("nvbio_gpl_amd.pipeline")
    text, _ = genome_and_index(orc)
    genome2 = orc.pack2(text)
    fmi = amd.FMIndex.build(genome2, len(text), kmer_len=8, sa_int=16)
    g_dev = torch.from_numpy(genome2.view(np.int32)).cuda()
    yield pipeline, fmi, g_dev, len(text)
    fmi.close()


def ragged_batch(pipeline, orc, reads):
    import torch
    syms, off = stored_stream(reads)
    return pipeline.ReadBatch(torch.from_numpy(orc.pack4(syms).view(np.int32)).cuda(), len(reads), max(len(r) for r in reads),
                              offsets=torch.from_numpy(off.astype(np.int32)).cuda())


def uniform_batch(pipeline, orc, reads):
    import torch
    m = np.stack(reads)
    return pipeline.ReadBatch(torch.from_numpy(orc.pack4(np.ascontiguousarray(m[:, ::-1]).reshape(-1)).view(np.int32)).cuda(), m.shape[0], m.shape[1])


def pe_params(amd, pipeline, mode, max_frag=500):
    k = pe_kw(mode, max_frag)
    return pipeline.PairedEndParams(policy=amd.PE_POLICY_FF if k["policy"] == 0 else amd.PE_POLICY_FR, min_frag_len=k["min_frag"], max_frag_len=k["max_frag"],
                                    overlap=k["overlap"]), k["unpaired"]


def same(got, want, what):
    for k in ("best_a", "best_o"):
        g = got[k].cpu().numpy().astype(np.int64)
        w = want[k]
        assert np.array_equal(g[..., 0], w[..., 0]), what + (k, "score")
        assert np.array_equal(g[..., 1] & 0xFFFFFFFF, w[..., 1]), what + (k, "pos")
        assert np.array_equal(g[..., 2] & 0xFFFFFFFF, w[..., 2]), what + (k, "sink")
        assert np.array_equal(g[..., 3], w[..., 3] | (w[..., 4] << 1) | (w[..., 5] << 2)), what + (k, "flags")
    for k in ("n_extensions", "n_opposite", "passes"):
        assert got[k] == want[k], what + (k, got[k], want[k])


def oriented(read, rc):
    return (np.where(read[::-1] < 4, 3 - read[::-1], read[::-1]) if rc else read).astype(np.uint8)


@pytest.mark.parametrize("mode", MODES)
def test_ragged_pairs_equal_the_restatement(amd, orc, device_genome, mode):
    """best_a / best_o of every pair -- score, position, sink, flags -- and the three counters at the three (batch_size, multi_hit) settings; then the
    traceback stage over the ragged mates: CIGARs and alignment begins equal the oracle's tracebacks of the same strings, for every pair found"""
    pipeline, fmi, g_dev, G = device_genome
    text, _, m1, m2 = shared_input(orc, mode == "no_unpaired_ff")
    rb = [ragged_batch(pipeline, orc, m) for m in (m1, m2)]
    params = pipeline.SeedExtendParams.end_to_end()
    pe, unpaired = pe_params(amd, pipeline, mode)
    for bs, multi in SETTINGS:
        got = pipeline.nvbowtie_best_approx_paired_host(fmi, g_dev, G, rb[0], rb[1], params, pipeline.NvBowtieParams(**KW[mode]), pe, unpaired=unpaired, batch_size=bs,
                                                        multi_hit=multi)
        same(got, restatement(orc, mode, bs, multi), (mode, bs, multi))
        assert (got["multi_passes"] > 0) == multi
    tb = pipeline.nvbowtie_paired_traceback(g_dev, G, rb[0], rb[1], params, got, pipeline.NvBowtieParams(**KW[mode]), cigar_stride=32)
    ba = got["best_a"].cpu().numpy().astype(np.int64); bo = got["best_o"].cpu().numpy().astype(np.int64)
    is_pair = tb["paired"].cpu().numpy()
    assert np.array_equal(is_pair, (((ba[:, 0, 3] >> 2) & 1) == 1) & (ba[:, 0, 1] != -1)) and is_pair.sum() > 150
    mates = (m1, m2)
    tbh = {k: v.cpu().numpy() for k, v in tb.items()}
    for r in np.nonzero(is_pair)[0]:
        am = int((ba[r, 0, 3] >> 1) & 1); a_rc = int(ba[r, 0, 3] & 1); o_rc = int(bo[r, 0, 3] & 1)
        Ma = len(mates[am][r])
        gpos = int(ba[r, 0, 1] & 0xFFFFFFFF)
        wb = gpos - 15 if gpos > 15 else 0; we = min(wb + 31 + Ma, G)
        ok, sc_, src_, snk_, cig_, _ = orc.banded_gotoh_traceback(31, oracle.SEMI_GLOBAL, OSC, oriented(mates[am][r], a_rc), text[wb:we])
        k = am + 1
        assert sc_ == ba[r, 0, 0] and int(tbh["score%d" % k][r]) == sc_, (mode, r, "anchor score")
        assert int(tbh["begin%d" % k][r]) == wb + src_[0] and int(tbh["rc%d" % k][r]) == a_rc, (mode, r, "anchor begin")
        n = int(tbh["cigar_lens%d" % k][r])
        assert n == len(cig_) and np.array_equal(tbh["cigars%d" % k][r, :n].view(np.uint16), cig_), (mode, r, "anchor cigar")
        ob = int(bo[r, 0, 1] & 0xFFFFFFFF); osx = int(bo[r, 0, 2] & 0xFFFFFFFF)
        ok, sc_, src_, snk_, cig_ = orc.full_gotoh_traceback(oracle.SEMI_GLOBAL, OSC, oriented(mates[1 - am][r], o_rc), text[ob:ob + osx])
        k = 2 - am
        assert sc_ == bo[r, 0, 0], (mode, r, "opposite score")
        assert int(tbh["begin%d" % k][r]) == ob + src_[0] and int(tbh["rc%d" % k][r]) == o_rc, (mode, r, "opposite begin")
        n = int(tbh["cigar_lens%d" % k][r])
        assert n == len(cig_) and np.array_equal(tbh["cigars%d" % k][r, :n].view(np.uint16), cig_), (mode, r, "opposite cigar")


def test_ragged_pairs_in_local_mode_equal_the_restatement(amd, orc, device_genome):
    """nvBowtie's local mode -- match 2, LOCAL alignment, thresholds int( 10 ln M ) -- over 60 ragged pairs: the perfect-score terms (match * o_len in
    both targets, `min_score > o_opt`, max_text_gaps' start) are live; the same arrays and counters as the end-to-end test"""
    pipeline, fmi, g_dev, G = device_genome
    pairs = slice(PLAIN.start, PLAIN.start + 60)
    _, _, m1, m2 = shared_input(orc, False)
    rb = [ragged_batch(pipeline, orc, m[pairs]) for m in (m1, m2)]
    params = pipeline.SeedExtendParams()
    assert params.scheme.c.match == 2 and params.aln_type == amd.LOCAL and params.min_score_for(100) == 46
    pe, unpaired = pe_params(amd, pipeline, "default")
    got = pipeline.nvbowtie_best_approx_paired_host(fmi, g_dev, G, rb[0], rb[1], params, pipeline.NvBowtieParams(**KW["default"]), pe, unpaired=unpaired)
    want = restatement(orc, "default", 0, True, local=True, pairs=pairs)
    same(got, want, ("local",))
    a = want["best_a"]
    assert ((a[:, 0, 5] == 1) & (a[:, 0, 1] != 0xFFFFFFFF)).sum() > 40 and (a[:, 0, 0] > 0).all()


def test_long_mates_pair_under_a_longer_fragment_limit(amd, orc, device_genome):
    """max_frag_len = 1500: the 1023-symbol mates of the four-pair set are placed as opposite mates, as the restatement places them"""
    pipeline, fmi, g_dev, G = device_genome
    text, _, m1, m2 = long_input(orc)
    rb = [ragged_batch(pipeline, orc, m) for m in (m1, m2)]
    pe, unpaired = pe_params(amd, pipeline, "default", 1500)
    got = pipeline.nvbowtie_best_approx_paired_host(fmi, g_dev, G, rb[0], rb[1], pipeline.SeedExtendParams.end_to_end(), pipeline.NvBowtieParams(**KW["default"]), pe,
                                                    unpaired=unpaired)
    same(got, restatement(orc, "default", 0, True, which="long", max_frag=1500), ("long",))
    a = got["best_a"].cpu().numpy()
    assert (((a[:, 0, 3] >> 2) & 1) == 1).all() and (a[:, 0, 1] != -1).all()


@pytest.mark.parametrize("mode", MODES)
def test_uniform_batch_through_offsets_equals_the_uniform_entry(amd, orc, device_genome, mode):
    """mates of 100 / 120 symbols expressed through offsets -- on both mates, or on one only -- take the ragged route and give the arrays and counters of
    the uniform entry point, bit for bit"""
    import torch
    pipeline, fmi, g_dev, G = device_genome
    text, _ = genome_and_index(orc)
    rng = np.random.default_rng(6)
    R = 200
    starts = rng.integers(0, G - 600, R)
    starts[:50] = 40000 + 5000 * rng.integers(0, 12, 50) + rng.integers(0, 100, 50)
    m1, m2 = make_pairs(rng, text, starts, rng.integers(230, 480, R), np.full(R, 100), np.full(R, 120), mode == "no_unpaired_ff", exact=set(),
                        elsewhere=set(range(60, 80)), random2=set(range(R - 8, R)))
    uni = [uniform_batch(pipeline, orc, m) for m in (m1, m2)]
    rag = [pipeline.ReadBatch(u.reads4, R, u.read_len, offsets=(torch.arange(R + 1, dtype=torch.int32) * u.read_len).cuda()) for u in uni]
    params = pipeline.SeedExtendParams.end_to_end()
    pe, unpaired = pe_params(amd, pipeline, mode)
    run = lambda a, b, multi: pipeline.nvbowtie_best_approx_paired_host(fmi, g_dev, G, a, b, params, pipeline.NvBowtieParams(**KW[mode]), pe, unpaired=unpaired,
                                                                        multi_hit=multi)
    for multi in (False, True):
        want = run(uni[0], uni[1], multi)
        for a, b in ((rag[0], rag[1]), (rag[0], uni[1]), (uni[0], rag[1])):
            got = run(a, b, multi)
            assert torch.equal(got["best_a"], want["best_a"]) and torch.equal(got["best_o"], want["best_o"]), (mode, multi)
            for k in ("n_extensions", "n_opposite", "passes", "multi_passes"):
                assert got[k] == want[k], (mode, multi, k)
    a = want["best_a"].cpu().numpy()
    assert ((((a[:, 0, 3] >> 2) & 1) == 1) & (a[:, 0, 1] != -1)).mean() > 0.7


@pytest.mark.parametrize("long_mate", [1, 2])
def test_a_1024_symbol_mate_is_rejected_and_nothing_is_written(amd, orc, device_genome, long_mate):
    """SeedHit keeps the seed position in 10 bits: a batch holding a mate of 1024 symbols, in either batch, is refused before any launch -- the result
    arrays keep what they held -- and 1023 is served"""
    import torch
    pipeline, fmi, g_dev, G = device_genome
    text, _ = genome_and_index(orc)
    short = [text[1000 * (k + 1):1000 * (k + 1) + M].copy() for k, M in enumerate((100, 110, 120))]
    # FR pairs: mate 2 reverse-complemented, downstream of mate 1; the long one ends 1200 symbols after its partner starts
    ends = [1000 * (k + 1) + 1200 for k in range(3)]
    params = pipeline.SeedExtendParams.end_to_end()
    pe = pipeline.PairedEndParams(max_frag_len=1500)

    def batches(long_len):
        lens = (130, long_len, 140)
        other = [(3 - text[e - M:e][::-1]).astype(np.uint8) for e, M in zip(ends, lens)]
        pair = (short, other) if long_mate == 2 else (other, short)
        return [ragged_batch(pipeline, orc, m) for m in pair]

    rb = batches(1024)
    out = (torch.full((3, 2, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0"), torch.full((3, 2, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0"))
    with pytest.raises(RuntimeError, match="1024"):
        pipeline.nvbowtie_best_approx_paired_host(fmi, g_dev, G, rb[0], rb[1], params, pe=pe, out=out)
    torch.cuda.synchronize()
    assert all(bool((t == 0x5A5A5A5A).all()) for t in out)
    rb = batches(1023)
    got = pipeline.nvbowtie_best_approx_paired_host(fmi, g_dev, G, rb[0], rb[1], params, pe=pe)
    a = got["best_a"].cpu().numpy(); o = got["best_o"].cpu().numpy()
    assert (((a[:, 0, 3] >> 2) & 1) == 1).all() and a[:, 0, 0].tolist() == [0, 0, 0] and o[:, 0, 0].tolist() == [0, 0, 0]


def test_the_ragged_init_call_writes_every_pairs_own_thresholds(amd):
    """nvbio_pe_init_ragged through its binding: unaligned at the mate's own min score, `mate` in the rc slot of best_o as the uniform call keeps it"""
    import torch
    w1 = torch.tensor([-7, -61, -90], dtype=torch.int32, device="cuda:0"); w2 = torch.tensor([-13, -19, -614], dtype=torch.int32, device="cuda:0")
    best_a = torch.zeros((3, 2, 4), dtype=torch.int32, device="cuda:0"); best_o = torch.zeros_like(best_a)
    amd.pe_init_ragged(amd.PeRagged(None, None, w1, w2), best_a, best_o)
    for best, w, flags in ((best_a, w1, 0), (best_o, w2, 1)):
        b = best.cpu().numpy()
        assert np.array_equal(b[..., 0], np.repeat(w.cpu().numpy()[:, None], 2, axis=1)) and (b[..., 1] == -1).all() and (b[..., 2] == 255).all() and (b[..., 3] == flags).all()
