"""GPU: the oracle-parity cases once more under the library's scratch check mode (nvbio_amd_set_scratch_check), with three fills.

In check mode every scratch block is a fresh exact-size allocation between two 4 KiB guard bands, a layout leaves 256 bytes before each
sub-array and after the last, and all of it (a caller's temp included) holds the fill before any work of the call.  A kernel or hipcub call
that writes past a sub-array damages a band or gap (the report says where); one that reads scratch it never wrote reads the fill instead of
the previous call's right answer, and its results stop equalling the oracle.  The fills: 0x00 (a fresh block), 0xFF (every flag "needs work",
every count huge), 0x02 (every unwritten need_dp flag a third-chance job).  Every case runs with the library's own scratch (temp=None) and,
where the entry point takes one, with a caller temp (the MEM and q-gram filters take only a caller temp).  The cases are the other
modules' tests, called through their modules."""
import ctypes

import numpy as np
import pytest

import oracle
import test_gpu_fm as fm
import test_gpu_gotoh as g
import test_gpu_gotoh_full as gf
import test_gpu_mem as mem
import test_gpu_pipeline as pl
import test_gpu_qgram as qg
import test_gpu_rank_dictionary as rd
import test_gpu_seed_hits as sh
import test_gpu_seed_pass as sp
import test_gpu_traceback as tb
from test_mem_oracle import NaiveIndex, make_reads, make_text
from test_scratch_sites import SCRATCH_TAGS

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xFF, 0x02)
_SEEN = {f: {} for f in FILLS}                  # fill -> tag -> blocks checked, over the whole module

fills = pytest.mark.parametrize("fill", FILLS, ids=["fill00", "fillFF", "fill02"])


@pytest.fixture
def checked(amd, fill):
    """check mode with `fill` for the test; afterwards (always) off again, and no scratch block of the test may have been damaged"""
    amd.set_scratch_check(True, fill)
    try:
        yield
    finally:
        report = amd.scratch_check_report()
        amd.set_scratch_check(False)
    damaged = {t: r for t, r in report.items() if r[1]}
    assert not damaged, damaged
    for t, r in report.items():
        _SEEN[fill][t] = _SEEN[fill].get(t, 0) + r[0]


class _NoSeedTemp:
    """the library as the package sees it, except that the seed-pass temp queries answer 0 bytes: the wrappers then hand the seed passes
    an empty tensor (a null temp) and the library takes its own scratch"""
    _NAMES = ("nvbio_fm_match_seed_diagonals_temp_bytes", "nvbio_fm_match_seed_diagonals_both_temp_bytes")

    def __init__(self, L):
        self._L = L

    def __getattr__(self, name):
        if name in self._NAMES:
            return lambda *a: 0
        return getattr(self._L, name)


@pytest.fixture(params=["caller", "library"])
def temp_owner(request, amd, monkeypatch):
    """'caller': the wrappers' own scratch tensors as temp_dev; 'library': a null temp_dev for the DP and seed-pass entry points"""
    if request.param == "library":
        torch = amd._torch()
        monkeypatch.setattr(amd, "_scratch", lambda device, nbytes, cap=0: torch.empty(0, dtype=torch.uint8, device=device))
        monkeypatch.setattr(amd, "lib", lambda L=amd.lib(): _NoSeedTemp(L))
    return request.param


@pytest.fixture(scope="module")
def big(orc):
    """test_gpu_fm's 1 Mbp text with a repeat"""
    rng = np.random.default_rng(42)
    text = rng.integers(0, 4, 1 << 20, dtype=np.uint8)
    text[5000:9000] = np.tile(np.array([2, 3, 2, 2, 0], dtype=np.uint8), 800)
    return rng, text, orc.build_index(text)


# ---- banded e2e scorer: need_dp, the three-way partition, second / third / gap chance, the length sort ---------------------------------
@fills
def test_banded_gap_chance(amd, orc, fill, checked):
    g.test_gap_chance_on_reads_with_indels(amd, orc)
    g.test_gap_chance_on_ragged_reversed_reads(amd, orc)


@fills
def test_banded_shortcut_with_qualities(amd, orc, fill, checked):
    g.test_end_to_end_shortcut_with_qualities_reversed_reads(amd, orc)
    g.test_best2_sink_golden(amd, g_golden("dp_golden"), g_golden("best2_golden"))


@fills
@pytest.mark.parametrize("flags", [0, 1, 2 | 128, 1 | 32])
def test_banded_low_complexity(amd, orc, fill, checked, flags, monkeypatch):
    g.test_end_to_end_banded_scoring_on_low_complexity_text(amd, orc, flags, monkeypatch)


# ---- tracebacks ------------------------------------------------------------------------------------------------------------------------
@fills
@pytest.mark.parametrize("typ", ["LOCAL", "SEMI_GLOBAL"])
def test_tracebacks(amd, orc, fill, checked, temp_owner, typ):
    tb.test_traceback_packed_batch_vs_oracle(amd, orc, typ, "shortcut")
    tb.test_full_traceback_opposite_mate_shape(amd, orc, typ, "shortcut")


# ---- full Gotoh ------------------------------------------------------------------------------------------------------------------------
@fills
def test_full_gotoh(amd, orc, fill, checked, temp_owner, monkeypatch):
    for max_m in (32, 152, 256):
        gf.test_cooperative_kernel_equals_the_oracle(amd, orc, max_m)
    gf.test_opposite_mate_shape(amd, orc)
    gf.test_end_to_end_full_dp_with_ungapped_shortcut(amd, orc, True, monkeypatch)


# ---- seed passes -----------------------------------------------------------------------------------------------------------------------
@fills
def test_seed_passes(amd, orc, fill, checked, temp_owner):
    sp.test_seed_pass_equals_the_operators(amd, orc, 9, 0)
    sp.test_two_strand_pass_equals_the_per_strand_operators(amd, orc, 9, False)
    sp.test_two_strand_pass_with_deferred_heavy_searches(amd, orc, 9)
    sp.test_two_strand_pass_over_ragged_reads(amd, orc)


# ---- FM index, rank dictionary, seed hits ----------------------------------------------------------------------------------------------
@fills
def test_fm_and_rank_dictionary(amd, orc, fill, checked, big):
    fm.test_filter_rank_locate(amd, orc, big)
    fm.test_seed_enumeration_and_diagonal_helpers(amd, orc, big)
    fm.test_hamming_backtrack(amd, orc, g_golden("fm_golden"), g_golden("bt_golden"))
    rd.test_generic_rank_golden(amd, g_golden("rankdict_golden"))
    rd.test_generic_rank_other_shapes_equal_the_oracle(amd, orc, 32, 128, 64)


@fills
def test_sort_unique_keys(amd, fill, checked):
    """nvbio_sort_unique_keys with its own scratch and with a caller temp (sized by the query made in check mode) == numpy's unique"""
    torch = amd._torch()
    rng = np.random.default_rng(77)
    for n in (1, 255, 4097, 200003):
        keys = rng.integers(0, max(2, n // 3), n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) >> np.uint64(1)
        want = np.unique(keys)
        nb = ctypes.c_uint64(0)
        amd._check(amd.lib().nvbio_sort_unique_keys_temp_bytes(ctypes.c_uint64(n), ctypes.byref(nb)))
        for temp in (None, torch.empty(nb.value + 3, dtype=torch.uint8, device="cuda")[3:]):      # (a caller temp off a 256-byte boundary)
            d = torch.from_numpy(keys.view(np.int64).copy()).cuda()
            n_out = torch.zeros(1, dtype=torch.int32, device="cuda")
            amd._check(amd.lib().nvbio_sort_unique_keys(
                0, amd._ptr(d), ctypes.c_uint64(n), amd._ptr(n_out), amd._ptr(temp), ctypes.c_uint64(0 if temp is None else temp.numel()),
                amd._stream_ptr(0)))
            m = int(n_out.item())
            assert m == len(want)
            assert np.array_equal(d[:m].cpu().numpy().view(np.uint64), want)


# ---- MEM filter and q-gram filter: the caller's temp only -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mem_texts(amd, orc):
    """test_gpu_mem's 60 kbp workload, and a 4 kbp text over two symbols whose split entries outnumber the reads' symbols several times"""
    out = []
    rng = np.random.default_rng(2)
    text = make_text(rng, 60_000)
    text[30_000:31_200] = np.tile(text[500:560], 20)
    reads = make_reads(rng, text, 150, [1, 30, 100, 150, 300])
    out.append((NaiveIndex(text), *mem._indices(amd, orc, text), reads))
    rng = np.random.default_rng(7)
    text = rng.integers(0, 2, 4000, dtype=np.uint8)
    reads = [text[p:p + 150].copy() for p in rng.integers(0, 4000 - 150, 40)] + [rng.integers(0, 2, 150, dtype=np.uint8) for _ in range(10)]
    out.append((NaiveIndex(text), *mem._indices(amd, orc, text), reads))
    yield out
    for _, f, r, _ in out:
        f.close(); r.close()


@fills
def test_mem_filter(amd, orc, fill, checked, mem_texts):
    """ragged and fixed-length sets, with and without split.  The binary text's split arena outgrows the candidate regions: the first
    attempt fails naming the temp it needs, the second moves the arena within the grown caller temp and fails on max_ranges, the third
    succeeds"""
    (idx, f, r, reads), (bidx, bf, br, breads) = mem_texts
    for params in (dict(min_intv=1), dict(min_intv=2, max_intv=20, split_len=28, split_width=10)):
        mem._check(amd, orc, idx, f, r, reads, 4, **params)
        mem._check(amd, orc, idx, f, r, [x for x in reads if len(x) == 150], 8, fixed=True, **params)
    mf, _, _ = mem._check(amd, orc, bidx, bf, br, breads, 2, min_intv=2, split_len=8, split_width=1000)
    assert mf.attempts == 3


@fills
def test_qgram_filter(amd, orc, fill, checked):
    qg.test_string_index_and_filter(amd, orc, 4, 2, True, 12, 8)
    qg.test_set_index_and_filter(amd, orc, "ragged", 3, 4, 2, 5, 1)
    qg.test_generate_qgrams(amd, orc, 4, 2, 12)
    qg.test_merge_wrapped_diagonals(amd)


# ---- whole pipeline (read_queue_filter and select_flagged_indices are the C++ host loop's) -------------------------------------------
@fills
def test_pipelines(amd, orc, fill, checked):
    pl.test_pipeline_equals_cpu_path(amd, orc, "e2e")
    pl.test_pipeline_ragged_reads_with_qualities_and_a_repeat_family(amd, orc)
    pl.test_paired_end_equals_cpu_path(amd, orc)
    sh.test_best_approx_loop_equals_the_oracle(amd, orc, "default")
    sh.test_paired_best_approx_loop_equals_the_oracle(amd, orc, "default")


# ---- the scorers' first-pass stash lives in the caller's scores / sinks -----------------------------------------------------------------
def _e2e_batch(amd, orc, seed, R, indel_every, M=150):
    """R end-to-end jobs: reads from a random genome with 0-3 substitutions, a 1-4 bp indel in every `indel_every`-th read and some
    far-off reads; band-31 windows around the true locus"""
    rng = np.random.default_rng(seed)
    G = 200000
    text = rng.integers(0, 4, G, dtype=np.uint8)
    text[3000:3600] = np.tile(text[3000:3012], 50)
    reads, wbs = [], []
    for j in range(R):
        p = int(rng.integers(64, G - M - 64)) if j % 13 else int(rng.integers(3000, 3400))
        src = text[p:p + M + 8].copy()
        if indel_every and j % indel_every == 0:
            at, gl = int(rng.integers(2, M - 6)), int(rng.integers(1, 5))
            src = np.concatenate([src[:at], src[at + gl:]]) if j % 2 else np.concatenate([src[:at], rng.integers(0, 4, gl, dtype=np.uint8), src[at:]])
        r = src[:M].copy()
        k = int(rng.integers(0, 4))
        if k:
            pos = rng.integers(0, M, k); r[pos] = (r[pos] + 1 + rng.integers(0, 3, k)) % 4
        if j % 17 == 5:
            r = rng.integers(0, 4, M, dtype=np.uint8)
        reads.append(r.astype(np.uint8)); wbs.append(p - 15)
    flat = np.concatenate(reads)
    roffs = (np.arange(R + 1) * M).astype(np.uint32)
    wb = np.array(wbs, dtype=np.uint32); we = (wb + M + 31).astype(np.uint32)
    return text, reads, flat, roffs, wb, we


SV = (0, 6, 6, -8, -3, -8, -3)


@fills
def test_stale_scores_and_sinks_do_not_leak_into_results(amd, orc, fill, checked):
    """the banded and full scorers stash their first pass in the caller's scores / sinks: what those held before the call must not matter"""
    torch = amd._torch()
    text, reads, flat, roffs, wb, we = _e2e_batch(amd, orc, 5, 3000, 4)
    R = len(reads)
    wsc, wsk = orc.banded_gotoh_packed_batch(31, oracle.SEMI_GLOBAL, oracle.Scheme(*SV), orc.pack4(flat), roffs, orc.pack2(text), wb, we)
    batch = amd.AlignmentBatch(orc.pack4(flat), 4, roffs, orc.pack2(text), 2, wb, we, max_read_len=150)
    aligner = amd.make_gotoh_aligner(oracle.SEMI_GLOBAL, g._scheme(amd, SV))
    fr = slice(0, R, 7)                                             # the full scorer on a sub-sample (its oracle is per job)
    fwant = [orc.full_gotoh(oracle.SEMI_GLOBAL, 0, oracle.Scheme(*SV), reads[j], text[wb[j]:we[j]]) for j in range(R)[fr]]
    fidx = np.arange(R)[fr]
    fbatch = amd.AlignmentBatch(orc.pack4(np.concatenate([reads[j] for j in fidx])), 4, (np.arange(len(fidx) + 1) * 150).astype(np.uint32),
                                orc.pack2(text), 2, wb[fidx], we[fidx])
    got = []
    for pattern in (0x7FFFFFFF, -1, 0):
        sc = torch.full((R,), pattern, dtype=torch.int32, device="cuda")
        sk = torch.full((R, 2), pattern, dtype=torch.int32, device="cuda")
        amd.BatchedBandedAlignmentScore(31, aligner).enact(batch, scores=sc, sinks=sk)
        s_, k_ = sc.cpu().numpy(), amd.u32(sk)
        assert np.array_equal(s_, wsc) and np.array_equal(k_, wsk), (pattern, np.nonzero(s_ != wsc)[0][:5])
        fsc = torch.full((len(fidx),), pattern, dtype=torch.int32, device="cuda")
        fsk = torch.full((len(fidx), 2), pattern, dtype=torch.int32, device="cuda")
        amd.BatchedAlignmentScore(aligner, text_blocking=False).enact(fbatch, 150, 181, scores=fsc, sinks=fsk)
        fs_, fk_ = fsc.cpu().numpy(), amd.u32(fsk)
        for i, (ok, ws, wk) in enumerate(fwant):
            assert fs_[i] == ws and tuple(fk_[i]) == wk, (pattern, i)
        got.append((s_, k_, fs_, fk_))
    for a in got[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(a, got[0]))
    assert len(np.unique(wsc)) > 10


def test_repeat_calls_on_the_cached_block(amd, orc):
    """check mode off (the production allocator): batch X, then batch Y of the same size with another mix of need_dp flags, then X again,
    on one stream -- Y's block still holds X's flags, and the second X's still holds Y's; each result equals the oracle"""
    aligner = amd.make_gotoh_aligner(oracle.SEMI_GLOBAL, g._scheme(amd, SV))
    R = 4000
    cases = {"X": _e2e_batch(amd, orc, 11, R, 0), "Y": _e2e_batch(amd, orc, 12, R, 2)}
    for name in ("X", "Y", "X"):
        text, reads, flat, roffs, wb, we = cases[name]
        wsc, wsk = orc.banded_gotoh_packed_batch(31, oracle.SEMI_GLOBAL, oracle.Scheme(*SV), orc.pack4(flat), roffs, orc.pack2(text), wb, we)
        batch = amd.AlignmentBatch(orc.pack4(flat), 4, roffs, orc.pack2(text), 2, wb, we, max_read_len=150)
        sc, sk = amd.batch_banded_alignment_score(31, aligner, batch)
        assert np.array_equal(sc.cpu().numpy(), wsc) and np.array_equal(amd.u32(sk), wsk), name


# ---- every site was checked under every fill ------------------------------------------------------------------------------------------
def test_every_site_was_checked_under_every_fill():
    for fill in FILLS:
        missing = [t for t in SCRATCH_TAGS if not _SEEN[fill].get(t)]
        assert not missing, (hex(fill), missing, _SEEN[fill])
    print("\nscratch check: blocks checked per site and fill (none damaged)")
    for t in SCRATCH_TAGS:
        print("  %-24s %s" % (t, "  ".join("%02X:%d" % (f, _SEEN[f][t]) for f in FILLS)))


_GOLDEN = {}


def g_golden(name):
    """the golden vectors conftest's session fixtures load, for cases called with them directly"""
    import os
    if name not in _GOLDEN:
        _GOLDEN[name] = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"), allow_pickle=False)
    return _GOLDEN[name]
