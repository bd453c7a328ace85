"""GPU: the q-group index in its string and set form (nvbio_qgroup_* through amd.QGroupIndex / QGroupSetIndex) against the
restatement of tests/test_qgroup_oracle.py and against the library's own sorted index of the same input: the exported I, S, SS and
P, nvbio_qgram_ranges, the q-gram filter's rank / locate / merge over it, slot order under contention, ragged and empty inputs,
byte-equal rebuilds, every limit, and one 100 Mbp text at Q = 16."""
import ctypes

import numpy as np
import pytest

import test_qgram_oracle as O
import test_qgroup_oracle as G
from test_gpu_qgram import _set_strings, _string_set, check_filter, pack, text_of, u64

pytestmark = pytest.mark.gpu


def check_group(amd, gidx, want, dense=True):
    """the exported arrays and the view against the restatement `want` (G.group_of)"""
    import torch
    a = gidx.arrays()
    v = gidx.view()
    assert v.n_qgrams == want["n_qgrams"] and v.n_unique == want["n_unique"] and v.n_words == want["n_words"]
    assert v.q == want["q"] and v.symbol_size == want["ss"] and v.is_set == (1 if want["P"].ndim == 2 else 0)
    assert a["I"].numel() == want["n_words"] and a["S"].numel() == want["n_words"]
    assert np.array_equal(amd.u32(a["SS"]), want["SS"])
    assert np.array_equal(amd.u32(a["P"]).reshape(want["P"].shape), want["P"])
    if dense:
        assert np.array_equal(amd.u32(a["I"]), want["I"]) and np.array_equal(amd.u32(a["S"]), want["S"])
        return
    # a table too large for a dense host copy: the set bits as a list, and S as the running popcount
    at = torch.nonzero(a["I"]).view(-1)
    words = amd.u32(a["I"][at]).astype(np.uint64)
    base = at.cpu().numpy().astype(np.uint64) << np.uint64(5)
    got = np.concatenate([base[k] + np.nonzero((words[k] >> np.arange(32, dtype=np.uint64)) & np.uint64(1))[0].astype(np.uint64)
                          for k in range(len(words))]) if len(words) else np.zeros(0, np.uint64)
    assert np.array_equal(got, want["qgrams"])
    assert int(a["I"][-1]) == 0                                       # A^q is a multiple of 32: word W holds no bit
    step = a["S"][1:] - a["S"][:-1]                                   # popc( I[i] ): 0 off the set words
    assert np.array_equal(amd.u32(step[at]), G.popc(words.astype(np.uint32)))
    step[at] = 0
    assert not bool(step.any()) and int(a["S"][0]) == 0 and int(a["S"][-1]) == want["n_unique"]


def filter_outputs(amd, idx, queries, indices, interval):
    """ranges, slots, hits, merged diagonals and counts of the q-gram filter over idx"""
    import torch
    qf = amd.QGramFilter()
    n = qf.rank(idx, torch.from_numpy(queries.view(np.int64)).cuda(), torch.from_numpy(indices.view(np.int32)).cuda())
    out = [amd.u32(qf.ranges()).copy(), u64(qf.slots()).copy()]
    if n:
        hits = qf.locate(0, n)
        cut = qf.locate(n // 3, n - n // 4)
        m, c = qf.merge(interval, hits)
        out += [amd.u32(hits).copy(), amd.u32(cut).copy(), amd.u32(m).copy(), amd.u32(c).copy()]
    return n, out


def check_both(amd, grp_idx, srt_idx, want, queries, indices, interval, cuts=()):
    """the filter over the q-group index equals the restatement and the filter over the sorted index; the two indices hold the same
    slots and occurrences"""
    a, b = grp_idx.arrays(), srt_idx.arrays()
    assert np.array_equal(amd.u32(a["SS"]), amd.u32(b["slots"])) and np.array_equal(amd.u32(a["P"]), amd.u32(b["index"]))
    nh = check_filter(amd, grp_idx, want, queries, indices, interval, cuts)
    n1, o1 = filter_outputs(amd, grp_idx, queries, indices, interval)
    n2, o2 = filter_outputs(amd, srt_idx, queries, indices, interval)
    assert n1 == n2 == nh and len(o1) == len(o2) and all(np.array_equal(x, y) for x, y in zip(o1, o2))
    return nh


def string_queries(rng, s, q, ss, n_from_text=3000):
    n = len(s)
    allg = O.qgrams_at(s, 0, n, np.arange(n), q, ss)
    top = np.uint64(1 << (q * ss))
    queries = np.concatenate([allg[rng.integers(0, n, n_from_text)], rng.integers(0, 1 << 62, 300, dtype=np.uint64) % top, allg[-q:],
                              np.array([0, top - np.uint64(1)], np.uint64),
                              top + np.array([0, 1, 31, 32, 1 << 40], np.uint64), np.array([(1 << 64) - 1], np.uint64)])   # >= A^q: misses
    return np.sort(queries)


STRING_CASES = [(2, 2, 1), (2, 2, 2), (2, 2, 5), (2, 2, 12), (4, 2, 3), (4, 2, 8), (4, 4, 1), (4, 4, 3), (4, 4, 6), (8, 2, 10), (8, 4, 5),
                (8, 2, 12), (8, 8, 2), (8, 8, 3)]                 # q * ss = 2, 4, 10, 24, 6, 16, 4, 12, 24, 20, 20, 24, 16, 24


@pytest.mark.parametrize("bits,ss,q", STRING_CASES)
def test_string_index_and_filter(amd, orc, bits, ss, q):
    rng = np.random.default_rng(bits * 1000 + ss * 100 + q)
    n = 6000
    s = text_of(rng, n, bits, with_n=True)
    s[100:400] = s[3000:3300]                                        # a planted repeat
    want = O.string_index(s, q, ss)
    packed = pack(orc, s, bits)
    gidx = amd.QGroupIndex.build(packed, bits, n, q, ss)
    sidx = amd.QGramIndex.build(packed, bits, n, q, ss, min(q, 8 // ss))
    check_group(amd, gidx, G.group_of(want))
    assert gidx.device_bytes() == 8 * G.n_words(q, ss) + 4 * (gidx.n_unique + 1) + 4 * n
    queries = string_queries(rng, s, q, ss)
    indices = rng.integers(0, 1 << 32, len(queries), dtype=np.uint64).astype(np.uint32)
    assert check_both(amd, gidx, sidx, want, queries, indices, 7, cuts=((0, 1), (5, 333), (1000, 4097), (2047, 2049))) > 0
    # the common view of a q-group handle, and the sorted index's export refused
    v = amd._QGramView()
    assert amd.lib().nvbio_qgram_index_get_view(gidx._h, ctypes.byref(v)) == 0
    gv = gidx.view()
    assert (v.q, v.symbol_size, v.qlut, v.is_set, v.n_qgrams, v.n_unique, v.lut_size) == (q, ss, 0, 0, n, gidx.n_unique, 0)
    assert v.slots_dev == gv.ss_dev and v.index_dev == gv.p_dev and not v.qgrams_dev and not v.lut_dev
    assert amd.lib().nvbio_qgram_index_export(gidx._h, None, None, None, None, None) == 1
    assert amd.lib().nvbio_qgroup_index_get_view(sidx._h, ctypes.byref(amd._QGroupView())) == 1
    assert amd.lib().nvbio_qgroup_index_export(sidx._h, None, None, None, None, None) == 1
    gidx.close(); sidx.close()


def test_q_times_ss_32_through_the_set_bit_list(amd, orc):
    rng = np.random.default_rng(32)
    n = 200_000
    s = text_of(rng, n, 2)
    s[5000:9000] = s[100_000:104_000]
    want = O.string_index(s, 16, 2)
    gidx = amd.QGroupIndex.build(orc.pack2(s), 2, n, 16, 2)
    check_group(amd, gidx, G.group_of(want, dense=False), dense=False)
    queries = string_queries(rng, s, 16, 2)
    check_filter(amd, gidx, want, queries, np.arange(len(queries), dtype=np.uint32), 16, cuts=((3, 1000),))
    gidx.close()


def _contended(amd, orc, s, q, n_queries):
    want = O.string_index(s, q, 2)
    packed = orc.pack2(s)
    gidx = amd.QGroupIndex.build(packed, 2, len(s), q, 2)
    again = amd.QGroupIndex.build(packed, 2, len(s), q, 2)
    sidx = amd.QGramIndex.build(packed, 2, len(s), q, 2, 8)
    check_group(amd, gidx, G.group_of(want))
    a, b = gidx.arrays(), again.arrays()
    assert all(bool((a[k] == b[k]).all()) for k in a)                # two builds are byte-equal
    queries = np.sort(O.qgrams_at(s, 0, len(s), np.arange(n_queries), q, 2))
    nh = check_both(amd, gidx, sidx, want, queries, np.arange(n_queries, dtype=np.uint32), 16, cuts=((12345, 200_000), (99_990, 100_010)))
    gidx.close(); again.close(); sidx.close()
    return nh


def test_all_a_text_is_one_ordered_slot(amd, orc):
    n = 100_000
    assert _contended(amd, orc, np.zeros(n, np.uint8), 12, 3) == 3 * n


def test_all_a_text_above_the_huge_slot_class(amd, orc):
    """a slot of 2^18 entries or more takes the device-wide sort"""
    import torch
    n = 600_000
    s = np.zeros(n, np.uint8)
    gidx = amd.QGroupIndex.build(orc.pack2(s), 2, n, 12, 2)
    a = gidx.arrays()
    assert amd.u32(a["SS"]).tolist() == [0, n] and bool((a["P"] == torch.arange(n, dtype=torch.int32, device="cuda")).all())
    gidx.close()


def test_period_three_tandem_repeat(amd, orc):
    s = np.tile(np.array([0, 1, 2], np.uint8), 40_000)                # three slots of 40,000 (and the padded tail's)
    assert _contended(amd, orc, s, 12, 30) >= 30 * 39_990


def test_ten_thousand_copy_repeat(amd, orc):
    rng = np.random.default_rng(7)
    unit = rng.integers(0, 4, 50, dtype=np.uint8)
    s = np.concatenate([rng.integers(0, 4, 1000, dtype=np.uint8), np.tile(unit, 10_000), rng.integers(0, 4, 1000, dtype=np.uint8)])
    want = O.string_index(s, 12, 2)
    gidx = amd.QGroupIndex.build(orc.pack2(s), 2, len(s), 12, 2)
    check_group(amd, gidx, G.group_of(want))
    gidx.close()


@pytest.mark.parametrize("n,q", [(1, 5), (3, 5), (4, 12), (11, 12), (12, 12), (64, 3), (65, 3)])
def test_short_texts(amd, orc, n, q):
    rng = np.random.default_rng(n + q)
    s = text_of(rng, n, 2)
    want = O.string_index(s, q, 2)
    gidx = amd.QGroupIndex.build(pack(orc, s, 2), 2, n, q, 2)
    check_group(amd, gidx, G.group_of(want))
    queries = np.sort(np.concatenate([want["qgrams"], np.array([1, 12345, 1 << 50], np.uint64)]))
    check_filter(amd, gidx, want, queries, np.arange(len(queries), dtype=np.uint32), 3)
    gidx.close()


@pytest.mark.parametrize("layout", ["fixed", "ragged", "offset"])
@pytest.mark.parametrize("interval", [1, 3, 10])
@pytest.mark.parametrize("bits,ss,q", [(2, 2, 12), (4, 2, 5), (4, 4, 5), (8, 2, 2)])
def test_set_index_and_filter(amd, orc, layout, interval, bits, ss, q):
    rng = np.random.default_rng(interval * 7 + q + bits)
    strings = _set_strings(rng, layout, bits)                          # ragged: empty and shorter-than-q strings among them
    if layout != "fixed":
        strings[5] = strings[9][:len(strings[5])]                       # equal seeds in several strings
        strings += [np.zeros(70, np.uint8)] * 3                         # a homopolymer in three strings: one contended slot
    want = O.set_index(strings, q, ss, interval)
    sset = _string_set(amd, orc, strings, bits, layout)
    gidx = amd.QGroupSetIndex.build(sset, q, ss, interval)
    again = amd.QGroupSetIndex.build(sset, q, ss, interval)
    sidx = amd.QGramSetIndex.build(sset, q, ss, interval, min(q, 4))
    check_group(amd, gidx, G.group_of(want))
    a, b = gidx.arrays(), again.arrays()
    assert all(bool((a[k] == b[k]).all()) for k in a)
    assert gidx.device_bytes() == 8 * G.n_words(q, ss) + 4 * (gidx.n_unique + 1) + 8 * gidx.n_qgrams
    text = np.concatenate([s[:40] for s in strings if len(s)] + [text_of(rng, 500, bits)])
    qg, pos = O.generate(text, len(text), q, ss, 0, len(text), True)
    qg = np.concatenate([qg, np.array([1 << (q * ss), (1 << 64) - 1], np.uint64)])     # out of range: misses
    pos = np.concatenate([pos, np.array([7, 8], np.uint32)])
    check_both(amd, gidx, sidx, want, qg, pos, 16, cuts=((3, 100), (50, 51)))
    check_filter(amd, gidx, want, qg[:300], np.zeros(300, np.uint32), 5)               # wrapped diagonals
    gidx.close(); again.close(); sidx.close()


def test_set_with_a_large_slot(amd, orc):
    """2,000 equal reads: every seed's slot holds 2,000 coordinates, string-major"""
    rng = np.random.default_rng(11)
    read = rng.integers(0, 4, 100, dtype=np.uint8)
    strings = [read.copy() for _ in range(2000)]
    want = O.set_index(strings, 12, 2, 10)
    gidx = amd.QGroupSetIndex.build(_string_set(amd, orc, strings, 2, "fixed"), 12, 2, 10)
    check_group(amd, gidx, G.group_of(want))
    gidx.close()


def test_empty_text_and_empty_set(amd, orc):
    import torch
    z64, z32 = torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    gidx = amd.QGroupIndex.build(np.zeros(16, np.uint32), 2, 0, 5, 2)
    check_group(amd, gidx, G.group_of(O.string_index(np.zeros(0, np.uint8), 5, 2)))
    sset = amd.PackedStringSet(np.zeros(16, np.uint8), 8, 0, offsets=np.zeros(1, np.uint32), ranges=True)
    gset = amd.QGroupSetIndex.build(sset, 5, 2, 3)
    check_group(amd, gset, G.group_of(O.set_index([], 5, 2, 3)))
    for idx in (gidx, gset):
        assert idx.n_unique == 0 and amd.u32(idx.arrays()["SS"]).tolist() == [0]
        qf = amd.QGramFilter()
        assert qf.rank(idx, z64, z32) == 0 and qf.rank(idx, z64[:0], z32[:0]) == 0
        assert not bool(idx.ranges(z64).any())
        idx.close()


def test_invalid_arguments(amd, orc):
    import torch
    L = amd.lib()
    text = torch.from_numpy(pack(orc, np.zeros(100, np.uint8), 2).view(np.int32)).cuda()
    h = ctypes.c_void_p()
    stream = amd._stream_ptr("cuda:0")

    def build(bits=2, length=100, q=5, ss=2, t=text, out=True):
        return L.nvbio_qgroup_index_build(0, amd._ptr(t), bits, length, q, ss, ctypes.byref(h) if out else None, stream)

    def refused(status):
        assert status == 1 and b"invalid argument" in L.nvbio_amd_last_error()

    assert build() == 0 and L.nvbio_qgram_index_destroy(h) == 0
    for kw in (dict(bits=3), dict(ss=0), dict(ss=9), dict(q=0), dict(q=19), dict(q=37, ss=1), dict(q=10, ss=4), dict(q=5, ss=8), dict(t=None),
               dict(out=False), dict(length=0xFFFFFFFF)):
        refused(build(**kw))
    strings = [np.zeros(30, np.uint8)] * 4
    ss = _string_set(amd, orc, strings, 8, "fixed")
    sb = L.nvbio_qgroup_set_index_build
    c = ss.c_struct()
    refused(sb(0, ctypes.byref(c), 5, 2, 0, ctypes.byref(h), stream))                                            # interval 0
    seeded = amd.PackedStringSet(ss.symbols, 8, 4, fixed_len=5, stride=30, seeds_per_string=1, seed_interval=1)
    refused(sb(0, ctypes.byref(seeded.c_struct()), 5, 2, 1, ctypes.byref(h), stream))                            # a seed enumeration
    c.offsets_are_ranges = 1
    refused(sb(0, ctypes.byref(c), 5, 2, 1, ctypes.byref(h), stream))                                            # ranges without offsets
    c2 = ss.c_struct(); c2.symbols_dev = None
    refused(sb(0, ctypes.byref(c2), 5, 2, 1, ctypes.byref(h), stream))
    c3 = ss.c_struct(); c3.symbol_bits = 3
    refused(sb(0, ctypes.byref(c3), 5, 2, 1, ctypes.byref(h), stream))
    refused(sb(0, ctypes.byref(ss.c_struct()), 19, 2, 1, ctypes.byref(h), stream))                               # q * ss = 38
    refused(sb(0, None, 5, 2, 1, ctypes.byref(h), stream))
    refused(sb(0, ctypes.byref(ss.c_struct()), 5, 2, 1, None, stream))
    refused(L.nvbio_qgroup_index_get_view(None, None))
    refused(L.nvbio_qgroup_index_export(None, None, None, None, None, stream))


@pytest.mark.timeout(1500)
def test_100_mbp_text_at_q16(amd, orc):
    """a seeded 100 Mbp text at Q = 16, two bits: SS and P equal the sorted index's arrays on the device, the popcount total is
    n_unique, and the ranges of 16 M sorted genome q-grams are equal through both indices"""
    import torch
    rng = np.random.default_rng(100)
    n = 100_000_000
    s = rng.integers(0, 4, n, dtype=np.uint8)
    for k in range(200):                                                # some repeats
        a, b = rng.integers(0, n - 500, 2)
        s[b:b + 500] = s[a:a + 500]
    s[50_000_000:50_300_000] = 0                                        # a homopolymer: one slot of 300,000
    packed = torch.from_numpy(orc.pack2(s).view(np.int32)).cuda()
    del s
    q = 16
    gidx = amd.QGroupIndex.build(packed, 2, n, q, 2)
    sidx = amd.QGramIndex.build(packed, 2, n, q, 2, 12)
    assert gidx.n_qgrams == n and gidx.n_unique == sidx.n_unique
    a, b = gidx.arrays(), sidx.arrays()
    assert torch.equal(a["SS"], b["slots"]) and torch.equal(a["P"], b["index"])
    b = None
    total = 0
    for part in a["I"].split(1 << 24):                                  # popcount by bit tricks, in slices
        x = part.to(torch.int64) & 0xFFFFFFFF
        x = x - ((x >> 1) & 0x55555555)
        x = (x & 0x33333333) + ((x >> 2) & 0x33333333)
        x = (x + (x >> 4)) & 0x0F0F0F0F
        total += int((((x * 0x01010101) >> 24) & 0xFF).sum())
    assert total == gidx.n_unique and int(a["S"][-1]) == gidx.n_unique and int(a["I"][-1]) == 0
    # the set bits are the sorted index's q-grams
    v = sidx.view()
    a = x = part = None
    g, _ = amd.generate_qgrams(q, 2, packed, 2, n, 40_000_000, 16 << 20, sort=True)
    r1, r2 = gidx.ranges(g), sidx.ranges(g)
    assert torch.equal(r1, r2) and int((r1[:, 1] - r1[:, 0]).min()) >= 1 and v.n_qgrams == n
    gidx.close(); sidx.close()
    del r1, r2, g, packed
    torch.cuda.empty_cache()
