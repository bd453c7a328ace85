"""CPU-only: the pass-by-pass restatement of the ragged PAIRED best-approx loop (tests/best_approx_paired_ragged_cpu.py) that the GPU tests compare
against is pinned before any GPU is involved -- on a uniform batch it is the oracle's paired loop field for field, with one hit per read and pass it
is that oracle called once per pair at the pair's own two lengths -- and the shared ragged pairs exercise what they should; the route's symbols are
declared and exported, and the host entry refuses what the contract refuses before it touches the device."""
import ctypes
from importlib import import_module

import numpy as np
import pytest

import __graft_entry__ as ge
import oracle
from best_approx_paired_ragged_cpu import (ELSEWHERE, FIXED, FIXED_PAIRS, KW, MODES, N_PAIRS, N_RANDOM, N_REPEAT, PLAIN, SETTINGS, best_approx_paired_ragged_cpu,
                                           make_pairs, paired_genome, pe_kw, restatement, shared_input, tables_of)
from best_approx_ragged_cpu import min_score_e2e
from oracle import cpu_pipeline

OSC = oracle.Scheme(0, 6, 6, -8, -3, -8, -3)


def is_paired(best_a):
    return (best_a[:, 0, 5] == 1) & (best_a[:, 0, 1] != 0xFFFFFFFF)


@pytest.mark.parametrize("mode", MODES)
def test_uniform_batch_equals_the_paired_oracle(orc, mode):
    """mates of lengths 100 / 120: the restatement is nvbowtie_best_approx_paired_cpu, counters included, at the three (batch_size, multi_hit) settings"""
    rng = np.random.default_rng(78)
    text = paired_genome(rng, 200_000)
    G, R = len(text), 90
    hidx = orc.build_index(text)
    starts = rng.integers(0, G - 600, R)
    starts[:25] = 40000 + 5000 * rng.integers(0, 12, 25) + rng.integers(0, 100, 25)
    m1, m2 = make_pairs(rng, text, starts, rng.integers(230, 480, R), np.full(R, 100), np.full(R, 120), mode == "no_unpaired_ff", exact=set(),
                        elsewhere=set(range(30, 40)), random2=set(range(R - 5, R)))
    tables, min_scores = tables_of(m1, m2)
    assert not tables[0][2].any() and not tables[1][2].any()
    for bs, multi in ((0, False), (0, True), (3 * R, True)):
        kw = dict(batch_size=bs or None, multi_hit=multi, **pe_kw(mode), **KW[mode])
        want = cpu_pipeline.nvbowtie_best_approx_paired_cpu(orc, hidx, text, G, np.stack(m1), np.stack(m2), OSC, oracle.SEMI_GLOBAL, min_score_e2e, **kw)
        got = best_approx_paired_ragged_cpu(orc, hidx, text, G, m1, m2, OSC, oracle.SEMI_GLOBAL, tables, min_scores, **kw)
        for k in ("best_a", "best_o"):
            assert np.array_equal(got[k], want[k]), (mode, bs, multi, k)
        for k in ("n_extensions", "n_opposite", "passes"):
            assert got[k] == want[k], (mode, bs, multi, k)
        assert (got["multi_passes"] > 0) == multi


@pytest.mark.parametrize("mode", MODES)
def test_one_hit_per_pass_equals_the_per_pair_oracle(orc, mode):
    """multi_hit off, on the shared ragged pairs: every pair with neither mate filtered equals nvbowtie_best_approx_paired_cpu called for that pair alone
    at its own two lengths and thresholds; a pair with one filtered mate holds only results whose anchor is the other mate; a pair with both filtered
    equals its initial state"""
    text, hidx, m1, m2 = shared_input(orc, mode == "no_unpaired_ff")
    tables, min_scores = tables_of(m1, m2)
    got = restatement(orc, mode, 0, False)
    assert got["multi_passes"] == 0
    filt = (tables[0][2], tables[1][2])
    n_ext = n_opp = 0
    seen = {"none": 0, "one": 0, "both": 0}
    for r in range(N_PAIRS):
        if filt[0][r] and filt[1][r]:
            seen["both"] += 1
            for k, m in (("best_a", 0), ("best_o", 1)):
                assert np.array_equal(got[k][r], [[min_scores[m][r], 0xFFFFFFFF, 255, m, 0, 0]] * 2), (mode, r, k)
        elif filt[0][r] or filt[1][r]:
            seen["one"] += 1
            anchor = 1 if filt[0][r] else 0                                   # the mate that was seeded
            a1, o1 = got["best_a"][r, 0], got["best_o"][r, 0]
            if a1[5] == 1 and a1[1] != 0xFFFFFFFF:
                assert a1[4] == anchor and o1[4] == 1 - anchor, (mode, r)
            # the unpaired fallback writes the anchor mate's own array only: the filtered mate's stays as initialised
            k, m = ("best_a", 0) if anchor == 1 else ("best_o", 1)
            if not (a1[5] == 1 and a1[1] != 0xFFFFFFFF):
                assert np.array_equal(got[k][r], [[min_scores[m][r], 0xFFFFFFFF, 255, m, 0, 0]] * 2), (mode, r, k)
        else:
            seen["none"] += 1
            one = cpu_pipeline.nvbowtie_best_approx_paired_cpu(orc, hidx, text, len(text), m1[r][None, :], m2[r][None, :], OSC, oracle.SEMI_GLOBAL, min_score_e2e,
                                                               multi_hit=False, **pe_kw(mode), **KW[mode])
            for k in ("best_a", "best_o"):
                assert np.array_equal(got[k][r], one[k][0]), (mode, r, k, len(m1[r]), len(m2[r]))
            n_ext += one["n_extensions"]; n_opp += one["n_opposite"]
    assert seen["both"] >= 2 and seen["one"] >= 4 and seen["none"] >= 280, seen
    # the pairs with a filtered mate add extensions of their own
    assert got["n_extensions"] >= n_ext and got["n_opposite"] >= n_opp


# the share of PLAIN pairs with both mates >= 50 found as pairs by the restatement.  default: the bar the issue sets.  tight / no_unpaired_ff: observed on
# this input 0.910 .. 0.917 / 0.924 over the three settings (default: 0.910 .. 0.917), less a margin of 0.03, and not below the 0.75 of the uniform test
FOUND_BAR = {"default": 0.9, "tight": 0.88, "no_unpaired_ff": 0.89}


@pytest.mark.parametrize("mode", MODES)
def test_shared_input_meets_the_input_conditions(orc, mode):
    """conditions on the inputs the GPU test relies on, asserted on the restatement itself"""
    text, hidx, m1, m2 = shared_input(orc, mode == "no_unpaired_ff")
    l1, l2 = np.array([len(r) for r in m1]), np.array([len(r) for r in m2])
    assert len(m1) == N_PAIRS and [(int(a), int(b)) for a, b in zip(l1[FIXED][::2], l2[FIXED][::2])] == list(FIXED_PAIRS)
    assert l1.min() == 11 and l1.max() == 1023 and l2.max() == 1023
    real = np.zeros(N_PAIRS, dtype=bool); real[PLAIN] = True
    real &= (l1 >= 50) & (l2 >= 50)
    assert real.sum() >= 100
    multi_passes = 0
    for bs, multi in SETTINGS:
        got = restatement(orc, mode, bs, multi)
        paired = is_paired(got["best_a"])
        found = paired[real].mean()
        print(mode, bs, multi, "found", round(float(found), 3), "passes", got["passes"], "ext", got["n_extensions"], "opp", got["n_opposite"])
        assert found >= FOUND_BAR[mode], (mode, bs, multi, found)
        assert not paired[N_PAIRS - N_RANDOM:].any()                          # no unalignable pair is paired
        assert not paired[ELSEWHERE].any() and paired[:N_REPEAT].any()
        # a 1023-symbol mate cannot be placed as the opposite mate under max_frag_len = 500: those pairs stay unpaired
        assert not paired[(l1 == 1023) | (l2 == 1023)].any()
        multi_passes += got["multi_passes"]
    assert multi_passes > 0                                                   # a multi-hit pass occurs
    if mode != "no_unpaired_ff":                                              # ... and end in the unpaired fallback: the exact 1023-symbol mate is held
        got = restatement(orc, mode, 0, True)
        k = FIXED.start + 2 * FIXED_PAIRS.index((1023, 100))
        assert got["best_a"][k, 0, 1] != 0xFFFFFFFF and got["best_a"][k, 0, 0] == 0 and got["best_a"][k, 0, 5] == 0


def test_long_mates_pair_under_a_longer_fragment_limit(orc):
    """the four-pair set with max_frag_len = 1500: its 1023-symbol mates are placed as opposite mates"""
    got = restatement(orc, "default", 0, True, which="long", max_frag=1500)
    assert is_paired(got["best_a"]).all()


NEW_SYMBOLS = ("nvbio_pe_init_ragged", "nvbio_pe_anchor_flatten_ragged", "nvbio_pe_opposite_flatten_ragged", "nvbio_pe_score_reduce_ragged")


def test_symbols_are_declared_and_exported():
    amd = ge.load_package()
    header = amd.abi.Header(amd.HEADER_PATH)
    declared = header.prototypes
    L = amd.lib()
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(L, s), s
    assert "nvbio_pe_ragged" in header.structs
    pipeline = import_module("nvbio_gpl_amd.pipeline")
    assert hasattr(pipeline._host_lib(), "nvbio_host_best_approx_paired_ragged")
    for f in ("pe_init_ragged", "pe_anchor_flatten_ragged", "pe_opposite_flatten_ragged", "pe_score_reduce_ragged"):
        assert callable(getattr(amd, f)), f


def test_ragged_paired_init_fails_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        return                                          # with a GPU the call would run: nothing to refuse
    amd = ge.load_package()
    buf = np.zeros(64, dtype=np.uint64)
    at = lambda k: ctypes.c_void_p(buf.ctypes.data + 64 * k)
    rg = amd._PeRagged(at(0), at(1), at(2), at(3))
    st = amd.lib().nvbio_pe_init_ragged(0, ctypes.c_uint32(1), ctypes.byref(rg), at(4), at(5), None)
    assert st == 5, st                                  # NVBIO_ERR_NO_DEVICE


def _refuse(offsets1, offsets2, min1=True, min2=True):
    """nvbio_host_best_approx_paired_ragged with null device pointers: a refusal comes before any HIP or library call -> the message"""
    amd = ge.load_package()
    pipeline = import_module("nvbio_gpl_amd.pipeline")
    host = pipeline._host_lib()
    scheme = amd.GotohScheme(0, 6, 6, -8, -3, -8, -3)
    p = pipeline._host_params(pipeline.NvBowtieParams(), 0, 0, True)
    pe = pipeline._HostPairedParams(1, 0, 500, 1, 1)
    st = pipeline._HostPairedStats()
    off = [None if o is None else np.ascontiguousarray(np.array(o, dtype=np.uint32)) for o in (offsets1, offsets2)]
    R = len(offsets2) - 1
    worst = [np.full(R, -30, dtype=np.int32) if m else None for m in (min1, min2)]
    hp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    rc = host.nvbio_host_best_approx_paired_ragged(0, None, None, ctypes.c_uint32(1000), None, None, None, None, ctypes.c_uint32(R), hp(off[0]), hp(off[1]), 1,
                                                   ctypes.byref(scheme.c), hp(worst[0]), hp(worst[1]), ctypes.c_uint32(12), ctypes.byref(p), ctypes.byref(pe), None, None, None,
                                                   ctypes.byref(st))
    assert rc == 1
    return host.nvbio_host_last_error().decode()


def test_the_host_entry_refuses_before_it_touches_the_device():
    ok = [0, 100, 200, 300]
    assert "1024" in _refuse([0, 100, 1124, 1224], ok)                        # a mate of 1024 symbols, in either batch
    assert "1024" in _refuse(ok, [0, 1024, 1124, 1224])
    assert "decrease" in _refuse([0, 100, 50, 300], ok) and "decrease" in _refuse(ok, [0, 100, 50, 300])
    assert "empty mate" in _refuse([0, 100, 100, 300], ok) and "empty mate" in _refuse(ok, [0, 0, 100, 300])
    assert "required" in _refuse(None, ok) and "required" in _refuse(ok, ok, min2=False) and "required" in _refuse(ok, ok, min1=False)
