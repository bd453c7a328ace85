"""GPU: the MEM filter (nvbio_mem_filter_rank / _locate through amd.MEMFilter) against the restatement of tests/test_mem_oracle.py --
ranges, their order and flags, first ranges, slots and the MEM count, then every located hit -- and, on a 16 Mbp text, against
FMIndex.match and the text itself."""
import numpy as np
import pytest

from test_mem_oracle import NaiveIndex, UNLIMITED, locate, make_reads, make_text, mem_filter

pytestmark = pytest.mark.gpu


def _indices(amd, orc, text, sa_int=4):
    n = len(text)
    f = amd.FMIndex.build(orc.pack2(text), n, kmer_len=0, sa_int=sa_int)
    r = amd.FMIndex.build(orc.pack2(text[::-1].copy()), n, kmer_len=0, sa_int=sa_int)
    return f, r


def _string_set(amd, orc, reads, bits, fixed=False):
    syms = np.concatenate(reads) if reads else np.zeros(0, np.uint8)
    packed = orc.pack2(syms) if bits == 2 else orc.pack4(syms) if bits == 4 else np.concatenate([syms, np.zeros(16, np.uint8)])
    if fixed:
        return amd.PackedStringSet(packed, bits, len(reads), fixed_len=len(reads[0]))
    offs = np.zeros(len(reads) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return amd.PackedStringSet(packed, bits, len(reads), offsets=offs, ranges=True)


def _check(amd, orc, idx, f, r, reads, bits, fixed=False, ss=None, **params):
    want_r, want_first, want_slots = mem_filter(idx, reads, **params)
    mf = amd.MEMFilter()
    n_mems = mf.rank(f, r, ss if ss is not None else _string_set(amd, orc, reads, bits, fixed), **params)
    got = amd.u32(mf.ranges()).reshape(-1, 4)
    assert mf.n_ranges == len(want_r)
    assert np.array_equal(got, want_r)
    assert np.array_equal(amd.u32(mf.first_ranges()), want_first)
    assert np.array_equal(mf.slots().cpu().numpy().astype(np.uint64), want_slots)
    assert n_mems == (int(want_slots[-1]) if len(want_slots) else 0)
    if n_mems:
        hits = amd.u32(mf.locate(0, n_mems)).reshape(-1, 4)
        assert np.array_equal(hits, locate(idx, want_r, want_slots, 0, n_mems))
    for sid in (0, len(reads) // 2, len(reads)):
        want = (int(want_slots[want_first[sid] - 1]) if want_first[sid] else 0) if sid < len(reads) else n_mems
        assert mf.first_hit(sid) == want
    return mf, want_r, want_slots


_PARAMS = [
    dict(min_intv=1),
    dict(min_intv=2, max_intv=UNLIMITED, min_span=19),
    dict(min_intv=5, max_intv=40),
    dict(min_intv=1, max_intv=3, min_span=19),
    dict(min_intv=1, min_span=19, split_len=28, split_width=10),
    dict(min_intv=2, max_intv=20, split_len=28, split_width=10),
    dict(min_intv=5, split_len=28, split_width=10),
]


@pytest.fixture(scope="module")
def workloads(amd, orc):
    out = {}
    for seed, n in ((1, 10_000), (2, 60_000), (3, 200_000)):
        rng = np.random.default_rng(seed)
        text = make_text(rng, n)
        text[n // 2:n // 2 + 1200] = np.tile(text[500:560], 20)     # a repeat: split candidates with a few occurrences
        reads = make_reads(rng, text, 150, [1, 30, 100, 150, 300])
        reads[3] = np.full(40, 4, np.uint8)
        reads[4] = text[-90:].copy()                                  # ends where the text ends
        f, r = _indices(amd, orc, text)
        out[n] = (NaiveIndex(text), f, r, reads)
    yield out
    for _, f, r, _ in out.values():
        f.close(); r.close()


@pytest.mark.parametrize("n", [10_000, 60_000, 200_000])
@pytest.mark.parametrize("bits", [2, 4, 8])
@pytest.mark.parametrize("pi", range(len(_PARAMS)))
def test_rank_and_locate_equal_the_restatement(amd, orc, workloads, n, bits, pi):
    idx, f, r, reads = workloads[n]
    if bits == 2:
        reads = [np.where(x > 3, 0, x).astype(np.uint8) for x in reads]
    _check(amd, orc, idx, f, r, reads, bits, **_PARAMS[pi])


def test_fixed_length_set(amd, orc, workloads):
    idx, f, r, _ = workloads[60_000]
    rng = np.random.default_rng(21)
    reads = make_reads(rng, idx.text, 200, [150])
    _check(amd, orc, idx, f, r, reads, 4, fixed=True, min_intv=2, split_len=28, split_width=10)


def test_ragged_set_whose_offsets_do_not_start_at_zero(amd, orc, workloads):
    """offsets[0] > 0: the candidate regions are laid out from offsets[0] (read_bounds' begin - offsets[0])"""
    idx, f, r, reads = workloads[60_000]
    rng = np.random.default_rng(23)
    lead = rng.integers(0, 5, 37).astype(np.uint8)                  # symbols before the first read, N's among them
    syms = np.concatenate([lead] + reads + [np.zeros(16, np.uint8)])
    offs = (37 + np.concatenate([[0], np.cumsum([len(x) for x in reads])])).astype(np.uint32)
    for bits in (4, 8):
        packed = orc.pack4(syms) if bits == 4 else syms
        ss = amd.PackedStringSet(packed, bits, len(reads), offsets=offs, ranges=True)
        _check(amd, orc, idx, f, r, reads, bits, ss=ss, min_intv=2, split_len=28, split_width=10)


def test_fixed_length_set_with_start_offsets(amd, orc, workloads):
    """n start offsets and fixed_len (reads scattered through a buffer, out of order, with gaps): regions are i x fixed_len"""
    idx, f, r, _ = workloads[60_000]
    rng = np.random.default_rng(24)
    R, M = 120, 100
    reads = make_reads(rng, idx.text, R, [M])
    slot = rng.permutation(R)
    buf = rng.integers(0, 5, R * (M + 13) + 16).astype(np.uint8)
    starts = (slot * (M + 13) + 5).astype(np.uint32)
    for i in range(R):
        buf[starts[i]:starts[i] + M] = reads[i]
    ss = amd.PackedStringSet(orc.pack4(buf), 4, R, offsets=starts, fixed_len=M)
    _check(amd, orc, idx, f, r, reads, 4, ss=ss, min_intv=1)
    _check(amd, orc, idx, f, r, reads, 4, ss=ss, min_intv=2, max_intv=20, split_len=28, split_width=10)


def test_edge_reads(amd, orc, workloads):
    """length 1, all N, a read of 700 symbols (spans past 255), and the empty set"""
    idx, f, r, _ = workloads[200_000]
    t = idx.text
    reads = [t[5:6].copy(), np.full(3, 4, np.uint8), np.concatenate([t[1000:1400], np.full(2, 4, np.uint8), t[150000:150298]])]
    mf, want, _ = _check(amd, orc, idx, f, r, reads, 8)
    assert any((int(w[3]) & 0xFFFF) >= 256 for w in want)
    mf = amd.MEMFilter()
    assert mf.rank(f, r, _string_set(amd, orc, [], 8)) == 0 and mf.n_ranges == 0
    assert amd.u32(mf.first_ranges())[0] == 0


def test_locate_sub_ranges(amd, orc, workloads):
    idx, f, r, reads = workloads[60_000]
    mf, want_r, want_slots = _check(amd, orc, idx, f, r, reads, 8, min_intv=2)
    n = int(want_slots[-1])
    rng = np.random.default_rng(5)
    for b, e in [(0, 1), (n - 1, n), (n // 3, n // 2), (7, 7 + 3000)] + [tuple(sorted(rng.integers(0, n + 1, 2))) for _ in range(5)]:
        e = min(e, n)
        got = amd.u32(mf.locate(int(b), int(e))).reshape(-1, 4)
        assert np.array_equal(got, locate(idx, want_r, want_slots, int(b), int(e)))
    with pytest.raises(amd.NvbioError):
        mf.locate(0, n + 1)


def test_capacity_error_names_the_size_and_a_rerun_at_it_succeeds(amd, orc, workloads):
    import re
    idx, f, r, reads = workloads[10_000]
    ss = _string_set(amd, orc, reads, 8)
    want_r, _, want_slots = mem_filter(idx, reads, min_intv=1)
    mf = amd.MEMFilter()
    with pytest.raises(amd.NvbioError) as e:
        mf.rank(f, r, ss, max_ranges=3)
    assert e.value.status == 1
    need = int(re.search(r"has (\d+) MEM ranges", str(e.value)).group(1))
    assert need == len(want_r)
    assert mf.rank(f, r, ss, max_ranges=need) == int(want_slots[-1])
    assert np.array_equal(amd.u32(mf.ranges()).reshape(-1, 4), want_r)


def test_buffers_are_sized_so_that_passes_are_not_repeated(amd, orc, workloads):
    """without split the first call fits (the symbol total bounds the ranges); a reused filter keeps what a split call needed"""
    idx, f, r, reads = workloads[200_000]
    ss = _string_set(amd, orc, reads, 8)
    mf = amd.MEMFilter()
    for params in (dict(min_intv=1), dict(min_intv=2, min_span=19)):
        mf.rank(f, r, ss, **params)
        assert mf.attempts == 1
    split = dict(min_intv=1, split_len=28, split_width=10)
    n1 = mf.rank(f, r, ss, **split)
    n2 = mf.rank(f, r, ss, **split)
    assert n1 == n2 and mf.attempts == 1


def test_mismatched_reverse_index_is_rejected(amd, orc, workloads):
    idx, f, _, reads = workloads[10_000]
    rng = np.random.default_rng(9)
    other = rng.integers(0, 4, 9_000, dtype=np.uint8)
    r2 = amd.FMIndex.build(orc.pack2(other), len(other), kmer_len=0, sa_int=4)
    try:
        with pytest.raises(amd.NvbioError) as e:
            amd.MEMFilter().rank(f, r2, _string_set(amd, orc, reads, 8))
        assert e.value.status == 1
    finally:
        r2.close()
    seeds = amd.PackedStringSet(np.zeros(64, np.uint8), 8, 4, fixed_len=10, stride=40, seeds_per_string=2, seed_interval=5)
    with pytest.raises(amd.NvbioError) as e:
        amd.MEMFilter().rank(f, workloads[10_000][2], seeds)
    assert e.value.status == 1


def test_large_self_consistency(amd, orc):
    """16 Mbp text, 200 k reads of 150: every range equals FMIndex.match of its span, is left-maximal, and every sampled hit's
    text equals the read span"""
    import torch
    rng = np.random.default_rng(42)
    G, R, M = 16_000_000, 200_000, 150
    text = rng.integers(0, 4, G, dtype=np.uint8)
    for _ in range(200):
        L = int(rng.integers(200, 2000)); s = int(rng.integers(0, G - L)); d = int(rng.integers(0, G - L))
        text[d:d + L] = text[s:s + L]
    f, r = _indices(amd, orc, text, sa_int=16)
    starts = rng.integers(0, G - M, R)
    reads = text[starts[:, None] + np.arange(M)].copy()
    m = rng.random(reads.shape) < 0.01
    reads[m] = rng.integers(0, 5, int(m.sum()))
    ss = amd.PackedStringSet(orc.pack4(reads.reshape(-1)), 4, R, fixed_len=M)
    mf = amd.MEMFilter()
    n_mems = mf.rank(f, r, ss, min_intv=1)
    assert mf.attempts == 1                                           # the default call never reruns its passes
    rg = amd.u32(mf.ranges()).reshape(-1, 4)
    first = amd.u32(mf.first_ranges())
    assert mf.n_ranges > R // 2 and first[-1] == mf.n_ranges
    sid = rg[:, 2] & 0x7FFFFFFF
    b, e = (rg[:, 3] & 0xFFFF).astype(np.int64), (rg[:, 3] >> 16).astype(np.int64)
    assert np.all(sid == np.repeat(np.arange(R), np.diff(first.astype(np.int64))))
    flat = reads.reshape(-1)

    def spans(bb, ee):
        lens = ee - bb
        offs = np.zeros(len(bb) + 1, np.uint32); offs[1:] = np.cumsum(lens)
        idx = np.repeat(sid.astype(np.int64) * M + bb - offs[:-1], lens) + np.arange(int(offs[-1]))
        return amd.PackedStringSet(flat[idx], 8, len(bb), offsets=offs, ranges=True)

    got = amd.u32(f.match(spans(b, e)))
    assert np.array_equal(got, rg[:, :2])
    left = b > 0
    prev = np.where(left, flat[sid.astype(np.int64) * M + np.maximum(b - 1, 0)], 4)
    ext = left & (prev <= 3)
    ext_r = amd.u32(f.match(spans(b - ext, e)))
    assert np.all((ext_r[ext, 1].astype(np.int64) - ext_r[ext, 0] + 1) < 1)
    # the longest range of each right-pass group carries the flag (every group keeps it here: min_span 1, no max_intv, no split):
    # one more symbol on the right falls below min_intv, unless it is an N or the read end
    flagged = (rg[:, 2] & 0x80000000) != 0
    nxt = np.where(e < M, flat[sid.astype(np.int64) * M + np.minimum(e, M - 1)], 4)
    ext = flagged & (nxt <= 3)
    assert flagged.sum() >= R // 2 and ext.sum() > 1000
    ext_r = amd.u32(f.match(spans(b, e + ext)))
    assert np.all((ext_r[ext, 1].astype(np.int64) - ext_r[ext, 0] + 1) < 1)
    k = min(n_mems, 2_000_000)
    hits = amd.u32(mf.locate(0, k)).reshape(-1, 4)
    pick = rng.integers(0, k, 20_000)
    for h in hits[pick]:
        p, s, hb, he = (int(v) for v in h)
        assert bytes(text[p:p + he - hb]) == bytes(reads[s, hb:he])
    f.close(); r.close(); torch.cuda.synchronize()
