"""CPU-only: the pass-by-pass restatement of the ragged best-approx loop (tests/best_approx_ragged_cpu.py) that the GPU tests compare against is
pinned before any GPU is involved -- on a uniform batch it is the oracle's batch loop field for field, with one hit per read and pass it is the
oracle's per-read loop called at every read's own length -- and the shared ragged input exercises what it should; the mode's symbols are
declared and exported."""
import math

import numpy as np
import pytest

import __graft_entry__ as ge
import oracle
from best_approx_ragged_cpu import (FIXED_LENGTHS, KW, N_RANDOM, best_approx_ragged_cpu, min_score_e2e, references, repeat_genome, seed_freq_of,
                                    seed_tables, shared_input)
from oracle import cpu_pipeline
from util import mutate_reads

FIELDS = ("best_score", "best_loc", "best_rc", "second_score", "second_loc", "second_rc")


@pytest.mark.parametrize("mode", ["default", "tight"])
def test_uniform_batch_equals_the_batch_oracle(orc, mode):
    """every read the same length: the restatement is nvbowtie_best_approx_batch_cpu, counters included, at two batch sizes"""
    rng = np.random.default_rng(77)
    text = repeat_genome(rng, 200_000)
    G, R, M = len(text), 90, 100
    starts = rng.integers(0, G - M - 8, R)
    starts[:40] = 50000 + 4000 * rng.integers(0, 15, 40) + rng.integers(0, 140, 40)
    reads = mutate_reads(rng, text, starts, M, sub=0.03)
    rcm = rng.random(R) < 0.5
    reads[rcm] = 3 - reads[rcm][:, ::-1]
    reads[-5:] = rng.integers(0, 4, (5, M))
    hidx = orc.build_index(text)
    osc = oracle.Scheme(0, 6, 6, -8, -3, -8, -3)
    S, first, filtered = seed_tables(np.full(R, M))
    assert not filtered.any()
    multi = 0
    for bs in (0, 3 * R):
        want = cpu_pipeline.nvbowtie_best_approx_batch_cpu(orc, hidx, text, G, reads, osc, oracle.SEMI_GLOBAL, min_score_e2e(M), batch_size=bs or None, **KW[mode])
        got = best_approx_ragged_cpu(orc, hidx, text, G, list(reads), osc, oracle.SEMI_GLOBAL, S, first, filtered, np.full(R, min_score_e2e(M)),
                                     batch_size=bs or None, **KW[mode])
        for k in FIELDS:
            assert np.array_equal(got[k].astype(np.int64), want[k].astype(np.int64)), (mode, bs, k)
        for k in ("n_extensions", "passes", "multi_passes"):
            assert got[k] == want[k], (mode, bs, k)
        multi += got["multi_passes"]
    assert multi > 0


@pytest.mark.parametrize("mode", ["default", "tight"])
def test_one_hit_per_pass_equals_the_per_read_oracle(orc, mode):
    """multi_hit off, on the shared ragged input: nvbowtie_best_approx_cpu once per read at that read's own length and worst score (filtered
    reads, which the oracle would seed with the whole read, stay unaligned by the contract)"""
    text, reads = shared_input()
    ref = references(orc, mode)
    osc = oracle.Scheme(0, 6, 6, -8, -3, -8, -3)
    got = best_approx_ragged_cpu(orc, ref["hidx"], text, len(text), reads, osc, oracle.SEMI_GLOBAL, ref["S"], ref["first"], ref["filtered"], ref["min_scores"],
                                 multi_hit=False, **KW[mode])
    want = ref["per_read"]
    for k in FIELDS:
        assert np.array_equal(got[k].astype(np.int64), want[k].astype(np.int64)), (mode, k)
    assert got["n_extensions"] == want["n_extensions"] and got["multi_passes"] == 0


def test_seed_tables_are_the_contract():
    lens = np.array(sorted(set(FIXED_LENGTHS) | set(range(100, 151))))
    S, first, filtered = seed_tables(lens)
    # the float32 evaluation agrees with the oracle's (double) one at every length in use
    assert [int(s) for s in S] == [int(1 + 1.15 * math.sqrt(M)) for M in lens]
    at = {int(M): k for k, M in enumerate(lens)}
    assert filtered[at[11]] and filtered[at[21]] and not filtered[at[22]]                      # below min_read_len, below seed_len, exactly one seed
    assert S[at[22]] == 6 and first[1][at[22]] == 2                                            # 22 < 22 + 2: a seed in pass 0, none in pass 1 or 2
    assert S[at[23]] == 6 and 23 < 22 + first[1][at[23]]
    assert first[2][at[30]] + 22 <= 30                                                         # ... and 30 keeps a seed in every pass
    assert (S[at[49]], S[at[50]]) == (9, 9) and (S[at[99]], S[at[100]], S[at[101]]) == (12, 12, 12)
    assert (S[at[149]], S[at[150]], S[at[151]]) == (15, 15, 15) and S[at[250]] == 19 and S[at[1023]] == 37
    steps = {int(M) for M in lens[1:] if seed_freq_of([M])[0] != seed_freq_of([M - 1])[0]}
    assert steps & set(range(100, 151)), "the 100..150 reads cross a step of int( 1 + 1.15 sqrt( M ) )"
    thirds = {int(s) // 3 for s in S}
    assert len(thirds) >= 5, "S_r / 3 takes several values"
    assert max(lens) == 1023                                                                   # the 10-bit position limit


@pytest.mark.parametrize("mode", ["default", "tight"])
def test_shared_input_meets_the_input_conditions(orc, mode):
    """conditions on the inputs the GPU test relies on, asserted on the restatement itself"""
    text, reads = shared_input()
    ref = references(orc, mode)
    lens = np.array([len(r) for r in reads])
    R = len(reads)
    assert R == 600 and all((lens == M).sum() >= 4 for M in FIXED_LENGTHS)
    random = np.arange(R) >= R - N_RANDOM
    for bs, got in ref["multi"].items():
        aligned = got["best_loc"] >= 0
        real = (lens >= 50) & ~random
        assert aligned[real].mean() >= 0.95, (mode, bs, aligned[real].mean())
        assert ref["filtered"].sum() >= 8 and not aligned[ref["filtered"]].any() and not aligned[random].any()
        assert got["multi_passes"] > 0
        unaligned = ref["filtered"] | random
        assert np.array_equal(got["best_score"][unaligned], ref["min_scores"][unaligned])
    if mode == "default":
        assert aligned[lens == 1023].all() and aligned[lens == 22].any()


NEW_SYMBOLS = ("nvbio_seed_hits_map_ragged", "nvbio_read_queue_begin_ragged", "nvbio_best_approx_init_ragged", "nvbio_score_reduce_effort_ragged",
               "nvbio_score_reduce_effort_multi_ragged")


def test_symbols_are_declared_and_exported():
    amd = ge.load_package()
    declared = amd.abi.Header(amd.HEADER_PATH).prototypes
    L = amd.lib()
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(L, s), s
    from importlib import import_module
    pipeline = import_module("nvbio_gpl_amd.pipeline")
    assert hasattr(pipeline._host_lib(), "nvbio_host_best_approx_ragged")
    assert callable(amd.seed_hits_map_ragged) and callable(amd.read_queue_begin_ragged) and callable(amd.best_approx_init_ragged)
    assert callable(amd.score_reduce_effort_ragged) and callable(amd.score_reduce_effort_multi_ragged)
    assert pipeline.NvBowtieParams().min_read_len == 12


def test_ragged_map_fails_without_a_gpu():
    import ctypes
    import torch
    if torch.cuda.is_available():
        return                                          # with a GPU the call would run: nothing to refuse
    amd = ge.load_package()
    buf = np.zeros(64, dtype=np.uint64)
    at = lambda k: ctypes.c_void_p(buf.ctypes.data + 64 * k)
    lay = amd._RaggedSeedLayout(at(0), at(1), 1, 0, 2, 22, 12)
    st = amd.lib().nvbio_seed_hits_map_ragged(0, at(2), at(3), None, ctypes.c_uint32(1), ctypes.byref(lay), ctypes.c_uint32(100), ctypes.c_uint32(1000),
                                              at(4), at(5), None, None)
    assert st == 5, st                                  # NVBIO_ERR_NO_DEVICE
