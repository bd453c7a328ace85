"""GPU parity of nvBowtie's best-approx loop over reads of DIFFERENT lengths (pipeline.nvbowtie_best_approx[_host] over a ReadBatch with offsets;
nvbio_*_ragged, host/nvbio_amd/best_approx.hpp: best_approx_ragged) against the oracle: one hit per read and pass against the oracle's per-read loop
called at every read's own length, the several-hits-per-read phase against the pass-by-pass restatement (tests/best_approx_ragged_cpu.py, pinned
without a GPU by tests/test_best_approx_ragged_oracle.py).  The shared input holds reads below min_read_len and below seed_len (filtered), with
exactly one seed, at steps of the seed interval and of its third, with a seed in pass 0 but none later, at the 10-bit position limit (1023), inside
a 30-copy repeat, at both genome ends, and unalignable ones."""
import importlib

import numpy as np
import pytest

from best_approx_ragged_cpu import KW, N_RANDOM, references, shared_input, stored_stream

pytestmark = pytest.mark.gpu

FIELDS = ("best_score", "best_loc", "best_rc", "second_score", "second_loc", "second_rc")


@pytest.fixture(scope="module")
def device_input(amd, orc):
    import torch
    pipeline = importlib.import_module("nvbio_gpl_amd.pipeline")
    text, reads = shared_input()
    G = len(text)
    genome2 = orc.pack2(text)
    fmi = amd.FMIndex.build(genome2, G, kmer_len=8, sa_int=16)
    g_dev = torch.from_numpy(genome2.view(np.int32)).cuda()
    syms, off = stored_stream(reads)
    rb = pipeline.ReadBatch(torch.from_numpy(orc.pack4(syms).view(np.int32)).cuda(), len(reads), max(len(r) for r in reads),
                            offsets=torch.from_numpy(off.astype(np.int32)).cuda())
    yield pipeline, fmi, g_dev, G, rb
    fmi.close()


def same(got, want, what):
    for k in FIELDS:
        assert np.array_equal(got[k].cpu().numpy().astype(np.int64), want[k].astype(np.int64)), what + (k,)


@pytest.mark.parametrize("mode", ["default", "tight"])
def test_one_hit_per_pass_equals_the_per_read_oracle(orc, device_input, mode):
    """the Python composition and the C++ loop with multi_hit off: best / second score, locus and strand of every read and the number of
    extensions equal nvbowtie_best_approx_cpu called once per read at that read's length"""
    pipeline, fmi, g_dev, G, rb = device_input
    want = references(orc, mode)["per_read"]
    params = pipeline.SeedExtendParams.end_to_end()
    got = pipeline.nvbowtie_best_approx(fmi, g_dev, G, rb, params, pipeline.NvBowtieParams(**KW[mode]))
    same(got, want, (mode, "composition"))
    assert got["n_extensions"] == want["n_extensions"]
    host = pipeline.nvbowtie_best_approx_host(fmi, g_dev, G, rb, params, pipeline.NvBowtieParams(**KW[mode]), multi_hit=False)
    same(host, want, (mode, "host"))
    assert host["n_extensions"] == want["n_extensions"] and host["multi_passes"] == 0
    aligned = host["best_loc"].cpu().numpy() >= 0
    assert not aligned[-N_RANDOM:].any() and not aligned[references(orc, mode)["filtered"]].any()


@pytest.mark.parametrize("mode", ["default", "tight"])
def test_several_hits_per_read_equal_the_restatement(orc, device_input, mode):
    """the C++ loop with the reference's several-hits-per-read phase at two batch sizes: the arrays and the counters equal the restatement's"""
    pipeline, fmi, g_dev, G, rb = device_input
    params = pipeline.SeedExtendParams.end_to_end()
    for bs, want in references(orc, mode)["multi"].items():
        got = pipeline.nvbowtie_best_approx_host(fmi, g_dev, G, rb, params, pipeline.NvBowtieParams(**KW[mode]), batch_size=bs, multi_hit=True)
        same(got, want, (mode, "multi", bs))
        assert got["n_extensions"] == want["n_extensions"] and got["passes"] == want["passes"] and got["multi_passes"] == want["multi_passes"], (mode, bs)
        assert got["multi_passes"] > 0


@pytest.mark.parametrize("mode", ["default", "tight"])
def test_uniform_batch_through_offsets_equals_the_uniform_entry(amd, orc, device_input, mode):
    """150 bp reads expressed through offsets take the ragged route and give the arrays and counters of the existing uniform entry point"""
    import torch
    from util import mutate_reads
    pipeline, fmi, g_dev, G, _ = device_input
    text, _ = shared_input()
    rng = np.random.default_rng(5)
    R, M = 300, 150
    starts = rng.integers(0, G - M - 8, R)
    starts[:100] = 50000 + 4000 * rng.integers(0, 30, 100) + rng.integers(0, 90, 100)
    reads = mutate_reads(rng, text, starts, M, sub=0.03)
    rcm = rng.random(R) < 0.5
    reads[rcm] = 3 - reads[rcm][:, ::-1]
    reads[-8:] = rng.integers(0, 4, (8, M))
    packed = torch.from_numpy(orc.pack4(np.ascontiguousarray(reads[:, ::-1]).reshape(-1)).view(np.int32)).cuda()
    uniform = pipeline.ReadBatch(packed, R, M)
    ragged = pipeline.ReadBatch(packed, R, M, offsets=(torch.arange(R + 1, dtype=torch.int32) * M).cuda())
    params = pipeline.SeedExtendParams.end_to_end()
    for multi in (False, True):
        a = pipeline.nvbowtie_best_approx_host(fmi, g_dev, G, uniform, params, pipeline.NvBowtieParams(**KW[mode]), multi_hit=multi)
        b = pipeline.nvbowtie_best_approx_host(fmi, g_dev, G, ragged, params, pipeline.NvBowtieParams(**KW[mode]), multi_hit=multi)
        for k in FIELDS:
            assert torch.equal(a[k], b[k]), (mode, multi, k)
        for k in ("n_extensions", "passes", "multi_passes", "seeding_passes"):
            assert a[k] == b[k], (mode, multi, k)
    c = pipeline.nvbowtie_best_approx(fmi, g_dev, G, uniform, params, pipeline.NvBowtieParams(**KW[mode]))
    d = pipeline.nvbowtie_best_approx(fmi, g_dev, G, ragged, params, pipeline.NvBowtieParams(**KW[mode]))
    for k in FIELDS:
        assert torch.equal(c[k], d[k]), (mode, "composition", k)
    assert c["n_extensions"] == d["n_extensions"] and c["passes"] == d["passes"]
    assert (b["best_loc"] >= 0).float().mean() > 0.9


def test_a_1024_symbol_read_is_rejected_and_nothing_is_written(amd, orc, device_input):
    """SeedHit keeps the seed position in 10 bits: a batch holding a read of 1024 symbols is refused by both loops, before any launch -- the
    result arrays keep what they held"""
    import torch
    pipeline, fmi, g_dev, G, _ = device_input
    text, _ = shared_input()
    lens = [100, 1024, 120]
    reads = [text[1000 * (k + 1):1000 * (k + 1) + M].copy() for k, M in enumerate(lens)]
    syms, off = stored_stream(reads)
    rb = pipeline.ReadBatch(torch.from_numpy(orc.pack4(syms).view(np.int32)).cuda(), 3, 1024, offsets=torch.from_numpy(off.astype(np.int32)).cuda())
    params = pipeline.SeedExtendParams.end_to_end()
    best = torch.full((3, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    best_rc = torch.full((3,), 0xA5, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(RuntimeError, match="1024"):
        pipeline.host_best_approx_ragged_into(fmi, g_dev, G, rb, params, pipeline.NvBowtieParams(), 0, True, best, best_rc)
    torch.cuda.synchronize()
    assert bool((best == 0x5A5A5A5A).all()) and bool((best_rc == 0xA5).all())
    with pytest.raises(RuntimeError, match="1024"):
        pipeline.nvbowtie_best_approx_host(fmi, g_dev, G, rb, params)
    with pytest.raises(ValueError, match="1024"):
        pipeline.nvbowtie_best_approx(fmi, g_dev, G, rb, params)
    # ... and 1023 is served (the shared input holds four such reads; here: the same three reads with the long one a symbol shorter)
    reads[1] = reads[1][:1023]
    syms, off = stored_stream(reads)
    ok = pipeline.ReadBatch(torch.from_numpy(orc.pack4(syms).view(np.int32)).cuda(), 3, 1023, offsets=torch.from_numpy(off.astype(np.int32)).cuda())
    got = pipeline.nvbowtie_best_approx_host(fmi, g_dev, G, ok, params)
    assert got["best_loc"].cpu().numpy().tolist() == [1000, 2000, 3000] and got["best_score"].cpu().numpy().tolist() == [0, 0, 0]
