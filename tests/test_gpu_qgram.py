"""GPU: the q-gram index, set index and filter (nvbio_qgram_*, nvbio_generate_qgrams through amd.QGramIndex / QGramSetIndex /
QGramFilter / generate_qgrams) against the restatement of tests/test_qgram_oracle.py: the index arrays (qgrams, slots, index, lut),
ranges, slots, the hit count, located hits over whole and cut sub-ranges, and merged diagonals; every invalid-argument status; and
on a 64 Mbp text, that every located hit's text holds its query q-gram."""
import ctypes

import numpy as np
import pytest

import test_qgram_oracle as O

pytestmark = pytest.mark.gpu


def pack(orc, syms, bits):
    syms = np.asarray(syms, np.uint8)
    if bits == 2:
        return orc.pack2(syms)
    if bits == 4:
        return orc.pack4(syms)
    return np.concatenate([syms, np.zeros(16, np.uint8)])


def text_of(rng, n, bits, with_n=False):
    hi = 4 if bits == 2 else 16 if bits == 4 else 256
    s = rng.integers(0, min(hi, 4), n, dtype=np.uint8)
    if with_n and n and bits > 2:                                    # a 2-bit text has no N
        s[rng.random(n) < 0.05] = 4 if bits == 4 else rng.integers(4, hi)
    return s


def u64(t):
    return t.detach().cpu().numpy().view(np.uint64)


def check_index(amd, gidx, want):
    a = gidx.arrays()
    assert gidx.n_qgrams == want["n_qgrams"] and gidx.n_unique == len(want["qgrams"])
    assert np.array_equal(u64(a["qgrams"]), want["qgrams"])
    assert np.array_equal(amd.u32(a["slots"]), want["slots"])
    assert np.array_equal(amd.u32(a["index"]).reshape(want["index"].shape), want["index"])
    if want["lut"] is None:
        assert a["lut"] is None
    else:
        assert np.array_equal(amd.u32(a["lut"]), want["lut"])


def check_filter(amd, gidx, want, queries, indices, interval, cuts=()):
    """rank, ranges, slots, locate (whole and sub-ranges) and merge against the restatement; returns n_hits"""
    import torch
    qf = amd.QGramFilter()
    n_hits = qf.rank(gidx, torch.from_numpy(queries.view(np.int64)).cuda(), torch.from_numpy(indices.view(np.int32)).cuda())
    r, slots, wn = O.rank(want, queries)
    assert n_hits == wn
    assert np.array_equal(amd.u32(qf.ranges()).reshape(-1, 2), r)
    assert np.array_equal(u64(qf.slots()), slots)
    assert np.array_equal(amd.u32(gidx.ranges(torch.from_numpy(queries.view(np.int64)).cuda())).reshape(-1, 2), r)
    if n_hits == 0:
        return 0
    hits = qf.locate(0, n_hits)
    wh = O.locate(want, r, slots, indices, 0, n_hits)
    assert np.array_equal(amd.u32(hits).reshape(wh.shape), wh)
    for b, e in cuts:
        b, e = min(b, n_hits), min(e, n_hits)
        assert np.array_equal(amd.u32(qf.locate(b, e)).reshape(-1, wh.shape[1]), wh[b:e])
    m, c = qf.merge(interval, hits)
    wm, wc = O.merge(wh, interval)
    assert np.array_equal(amd.u32(m).reshape(wm.shape), wm) and np.array_equal(amd.u32(c), wc)
    return n_hits


def _string_cases():
    out = []
    for bits, ss, with_n in ((2, 2, False), (4, 2, True), (4, 4, True), (8, 2, False), (8, 8, True)):
        for q in (1, 5, 12, 20, 31, 32):
            if q * ss > 64:
                continue
            for qlut in (0, 1, 8, q):
                if qlut <= q and qlut * ss <= 24:
                    out.append((bits, ss, with_n, q, qlut))
    return sorted(set(out))


@pytest.mark.parametrize("bits,ss,with_n,q,qlut", _string_cases())
def test_string_index_and_filter(amd, orc, bits, ss, with_n, q, qlut):
    rng = np.random.default_rng(bits * 1000 + ss * 100 + q * 10 + qlut)
    n = 6000
    s = text_of(rng, n, bits, with_n)
    s[100:400] = s[3000:3300]                                        # a repeat
    want = O.string_index(s, q, ss, qlut)
    gidx = amd.QGramIndex.build(pack(orc, s, bits), bits, n, q, ss, qlut)
    check_index(amd, gidx, want)
    allg = O.qgrams_at(s, 0, n, np.arange(n), q, ss)
    top = np.uint64((1 << (q * ss)) - 1) if q * ss < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
    queries = np.concatenate([allg[rng.integers(0, n, 3000)], rng.integers(0, 1 << 62, 300, dtype=np.uint64) & top,
                              allg[-q:], np.array([0], np.uint64)])
    if q * ss < 64:
        queries = np.concatenate([queries, np.array([top + np.uint64(1)], np.uint64)])       # bits above q * ss: a miss
    queries = np.sort(queries)
    indices = rng.integers(0, 1 << 32, len(queries), dtype=np.uint64).astype(np.uint32)
    nh = check_filter(amd, gidx, want, queries, indices, 7, cuts=((0, 1), (5, 333), (1000, 4097), (2047, 2049)))
    assert nh > 0
    gidx.close()


@pytest.mark.parametrize("n,q,qlut", [(1, 5, 0), (1, 5, 3), (3, 5, 2), (4, 20, 12), (19, 20, 0), (20, 20, 8)])
def test_short_texts(amd, orc, n, q, qlut):
    rng = np.random.default_rng(n + q)
    s = text_of(rng, n, 2)
    want = O.string_index(s, q, 2, qlut)
    gidx = amd.QGramIndex.build(pack(orc, s, 2), 2, n, q, 2, qlut)
    check_index(amd, gidx, want)
    queries = np.sort(np.concatenate([want["qgrams"], np.array([1, 12345], np.uint64)]))
    check_filter(amd, gidx, want, queries, np.arange(len(queries), dtype=np.uint32), 3)


def test_all_a_text(amd, orc):
    s = np.zeros(5000, np.uint8)
    want = O.string_index(s, 12, 2, 8)
    gidx = amd.QGramIndex.build(pack(orc, s, 2), 2, len(s), 12, 2, 8)
    check_index(amd, gidx, want)
    assert gidx.n_unique == 1
    q = np.zeros(3, np.uint64)
    check_filter(amd, gidx, want, q, np.array([0, 7, 4999], np.uint32), 16, cuts=((4999, 5001), (10, 12000)))


def test_ten_thousand_copy_repeat(amd, orc):
    rng = np.random.default_rng(7)
    unit = rng.integers(0, 4, 50, dtype=np.uint8)
    s = np.concatenate([rng.integers(0, 4, 1000, dtype=np.uint8), np.tile(unit, 10_000), rng.integers(0, 4, 1000, dtype=np.uint8)])
    q, qlut = 20, 8
    want = O.string_index(s, q, 2, qlut)
    gidx = amd.QGramIndex.build(pack(orc, s, 2), 2, len(s), q, 2, qlut)
    check_index(amd, gidx, want)
    queries = np.sort(O.qgrams_at(s, 0, len(s), np.arange(1000, 1050), q, 2))
    nh = check_filter(amd, gidx, want, queries, np.arange(1000, 1050, dtype=np.uint32), 16, cuts=((12345, 200_000), (499_990, 500_010)))
    assert nh >= 50 * 9_999


def _set_strings(rng, layout, bits):
    lens = [150] * 40 if layout == "fixed" else list(rng.integers(0, 80, 60)) + [3, 4, 5, 19, 20, 21]
    strings = [text_of(rng, int(L), bits, with_n=True) for L in lens]
    return strings


def _string_set(amd, orc, strings, bits, layout):
    syms = np.concatenate(strings) if strings else np.zeros(0, np.uint8)
    if layout == "fixed":
        return amd.PackedStringSet(pack(orc, syms, bits), bits, len(strings), fixed_len=len(strings[0]))
    lead = 37 if layout == "offset" else 0                              # offsets not starting at 0
    syms = np.concatenate([np.full(lead, 3, np.uint8), syms])
    offs = np.zeros(len(strings) + 1, np.uint32)
    offs[1:] = np.cumsum([len(s) for s in strings])
    return amd.PackedStringSet(pack(orc, syms, bits), bits, len(strings), offsets=offs + lead, ranges=True)


@pytest.mark.parametrize("layout", ["fixed", "ragged", "offset"])
@pytest.mark.parametrize("interval", [1, 3, 10])
@pytest.mark.parametrize("bits,ss,q,qlut", [(2, 2, 20, 12), (4, 2, 5, 1), (4, 4, 5, 5), (8, 2, 12, 0)])
def test_set_index_and_filter(amd, orc, layout, interval, bits, ss, q, qlut):
    rng = np.random.default_rng(interval * 7 + q + bits)
    strings = _set_strings(rng, layout, bits)
    want = O.set_index(strings, q, ss, interval, qlut)
    gidx = amd.QGramSetIndex.build(_string_set(amd, orc, strings, bits, layout), q, ss, interval, qlut)
    check_index(amd, gidx, want)
    # a text made of pieces of the strings, its q-grams streamed as qmap does (sorted, coordinates = positions)
    text = np.concatenate([s[:40] for s in strings if len(s)] + [text_of(rng, 500, bits)])
    qg, pos = O.generate(text, len(text), q, ss, 0, len(text), True)
    check_filter(amd, gidx, want, qg, pos, 16, cuts=((3, 100), (50, 51)))
    # non-power-of-two interval with wrapped diagonals (text positions below string positions)
    check_filter(amd, gidx, want, qg[:300], np.zeros(300, np.uint32), 5)
    gidx.close()


def test_empty_set(amd, orc):
    ss = amd.PackedStringSet(np.zeros(16, np.uint8), 8, 0, offsets=np.zeros(1, np.uint32), ranges=True)
    gidx = amd.QGramSetIndex.build(ss, 5, 2, 3, 2)
    want = O.set_index([], 5, 2, 3, 2)
    check_index(amd, gidx, want)
    import torch
    qf = amd.QGramFilter()
    assert qf.rank(gidx, torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")) == 0
    assert qf.rank(gidx, torch.zeros(0, dtype=torch.int64, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda")) == 0


def test_merge_wrapped_diagonals(amd):
    import torch
    rng = np.random.default_rng(3)
    h2 = rng.integers(0, 1 << 32, (5000, 2), dtype=np.uint64).astype(np.uint32)
    h2[:2000, 1] = h2[:2000, 0] - rng.integers(0, 40, 2000).astype(np.uint32)
    h2[2000:2100] = [0, 0xFFFFFFFD]
    h4 = np.zeros((5000, 4), np.uint32)
    h4[:, 0] = rng.integers(0, 50, 5000)
    h4[:, 1] = rng.integers(0, 150, 5000)
    h4[:, 2] = rng.integers(0, 300, 5000)
    qf = amd.QGramFilter()
    for interval in (1, 7, 16, 1000, 0x80000001):
        for h in (h2, h4):
            m, c = qf.merge(interval, torch.from_numpy(h.view(np.int32)).cuda())
            wm, wc = O.merge(h, interval)
            assert np.array_equal(amd.u32(m).reshape(wm.shape), wm) and np.array_equal(amd.u32(c), wc)
    m, c = qf.merge(16, torch.from_numpy(np.array([[0, 0xFFFFFFFD]], np.uint32).view(np.int32)).cuda())
    assert amd.u32(m).tolist() == [0] and amd.u32(c).tolist() == [1]          # -3 snaps to 0


@pytest.mark.parametrize("bits,ss,q", [(2, 2, 20), (4, 2, 12), (4, 4, 5), (8, 8, 8)])
def test_generate_qgrams(amd, orc, bits, ss, q):
    rng = np.random.default_rng(q)
    s = text_of(rng, 20000, bits, with_n=True)
    s[:5000] = 0                                                       # many equal q-grams: stability shows
    for first, n, sort in ((0, 20000, True), (123, 5000, False), (19000, 2000, True), (0, 1, True)):
        g, p = amd.generate_qgrams(q, ss, pack(orc, s, bits), bits, len(s), first, n, sort=sort)
        wg, wp = O.generate(s, len(s), q, ss, first, n, sort)
        assert np.array_equal(u64(g), wg) and np.array_equal(amd.u32(p), wp)


def test_invalid_arguments(amd, orc):
    import torch
    L = amd.lib()
    text = torch.from_numpy(pack(orc, np.zeros(100, np.uint8), 2).view(np.int32)).cuda()
    h = ctypes.c_void_p()
    stream = amd._stream_ptr("cuda:0")

    def build(bits=2, length=100, q=5, ss=2, qlut=0, t=text, out=True):
        return L.nvbio_qgram_index_build(0, amd._ptr(t), bits, length, q, ss, qlut, ctypes.byref(h) if out else None, stream)

    assert build() == 0
    good = amd.QGramIndex(ctypes.c_void_p(h.value), "cuda:0")
    for kw in (dict(bits=3), dict(ss=0), dict(ss=9), dict(q=0), dict(q=33), dict(q=5, qlut=6), dict(q=20, qlut=15), dict(t=None),
               dict(out=False), dict(length=0xFFFFFFFF), dict(q=9, ss=8)):
        assert build(**kw) == 1, kw
    assert build(q=32, ss=2, qlut=14) == 0 and L.nvbio_qgram_index_destroy(h) == 0      # the limits themselves
    assert build(q=64, ss=1, qlut=28) == 0 and L.nvbio_qgram_index_destroy(h) == 0

    strings = [np.zeros(30, np.uint8)] * 4
    ss = _string_set(amd, orc, strings, 8, "fixed")
    c = ss.c_struct()
    assert L.nvbio_qgram_set_index_build(0, ctypes.byref(c), 5, 2, 0, 0, ctypes.byref(h), stream) == 1           # interval 0
    seeded = amd.PackedStringSet(ss.symbols, 8, 4, fixed_len=5, stride=30, seeds_per_string=1, seed_interval=1)
    cs = seeded.c_struct()
    assert L.nvbio_qgram_set_index_build(0, ctypes.byref(cs), 5, 2, 1, 0, ctypes.byref(h), stream) == 1          # seed enumeration
    c.offsets_are_ranges = 1
    assert L.nvbio_qgram_set_index_build(0, ctypes.byref(c), 5, 2, 1, 0, ctypes.byref(h), stream) == 1           # ranges without offsets
    c2 = ss.c_struct(); c2.symbols_dev = None
    assert L.nvbio_qgram_set_index_build(0, ctypes.byref(c2), 5, 2, 1, 0, ctypes.byref(h), stream) == 1          # no symbols
    c3 = ss.c_struct(); c3.symbol_bits = 3
    assert L.nvbio_qgram_set_index_build(0, ctypes.byref(c3), 5, 2, 1, 0, ctypes.byref(h), stream) == 1
    assert L.nvbio_qgram_set_index_build(0, ctypes.byref(ss.c_struct()), 5, 2, 1, 6, ctypes.byref(h), stream) == 1   # qlut > q
    assert L.nvbio_qgram_set_index_build(0, None, 5, 2, 1, 0, ctypes.byref(h), stream) == 1

    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = amd._ptr(buf)
    gen = L.nvbio_generate_qgrams
    assert gen(0, 5, 2, amd._ptr(text), 2, 100, 0, 10, p, p, 1, None, ctypes.c_uint64(0), stream) == 1          # sorted without temp
    assert gen(0, 5, 2, amd._ptr(text), 2, 100, 0xFFFFFFF0, 0x20, p, p, 0, None, ctypes.c_uint64(0), stream) == 1  # first + n wraps
    assert gen(0, 5, 2, amd._ptr(text), 2, 100, 0, 10, p, p, 1, p, ctypes.c_uint64(16), stream) == 1             # temp too small
    assert gen(0, 5, 2, amd._ptr(text), 5, 100, 0, 10, p, None, 0, None, ctypes.c_uint64(0), stream) == 1         # text bits
    assert gen(0, 40, 2, amd._ptr(text), 2, 100, 0, 10, p, None, 0, None, ctypes.c_uint64(0), stream) == 1        # q * ss > 64
    assert gen(0, 5, 2, amd._ptr(text), 2, 100, 0, 10, None, None, 0, None, ctypes.c_uint64(0), stream) == 1      # no output

    nh = ctypes.c_uint64(0)
    rk = L.nvbio_qgram_filter_rank
    assert rk(good._h, p, 10, p, p, p, ctypes.c_uint64(8), ctypes.byref(nh), stream) == 1                         # temp too small
    assert rk(good._h, p, 10, p, p, p, ctypes.c_uint64(1 << 16), None, stream) == 1                                # no n_hits
    assert rk(good._h, None, 10, p, p, p, ctypes.c_uint64(1 << 16), ctypes.byref(nh), stream) == 1
    assert rk(None, p, 10, p, p, p, ctypes.c_uint64(1 << 16), ctypes.byref(nh), stream) == 1

    qf = amd.QGramFilter()
    n = qf.rank(good, torch.zeros(3, dtype=torch.int64, device="cuda"), torch.zeros(3, dtype=torch.int32, device="cuda"))
    assert n == 300
    with pytest.raises(amd.NvbioError):
        qf.locate(0, n + 1)                                                                                    # past the last hit
    lo = L.nvbio_qgram_filter_locate
    assert lo(good._h, amd._ptr(qf._ranges), amd._ptr(qf._slots), None, 3, ctypes.c_uint64(0), ctypes.c_uint64(5), p, stream) == 1
    assert lo(good._h, amd._ptr(qf._ranges), amd._ptr(qf._slots), amd._ptr(qf._indices), 0, ctypes.c_uint64(0), ctypes.c_uint64(5), p,
              stream) == 1
    nm = ctypes.c_uint32(0)
    mg = L.nvbio_qgram_filter_merge
    assert mg(0, 0, 0, p, 10, p, p, ctypes.byref(nm), p, ctypes.c_uint64(1 << 16), stream) == 1                  # interval 0
    assert mg(0, 1, 16, p, 1000, p, p, ctypes.byref(nm), p, ctypes.c_uint64(64), stream) == 1                     # temp too small
    assert mg(0, 0, 16, p, 10, None, p, ctypes.byref(nm), p, ctypes.c_uint64(1 << 16), stream) == 1
    assert mg(0, 0, 16, p, 10, p, p, None, p, ctypes.c_uint64(1 << 16), stream) == 1
    assert L.nvbio_qgram_index_get_view(None, None) == 1 and L.nvbio_qgram_index_device_bytes(good._h, None) == 1
    good.close()


def test_64_mbp_text(amd, orc):
    """Q = 20, LUT 12 over 64 Mbp: every located hit's text holds the query q-gram, and every query's hit count is its q-gram's
    number of occurrences in the text"""
    import torch
    rng = np.random.default_rng(64)
    n = 64 << 20
    s = rng.integers(0, 4, n, dtype=np.uint8)
    for k in range(200):                                                # some repeats
        a, b = rng.integers(0, n - 500, 2)
        s[b:b + 500] = s[a:a + 500]
    q, qlut = 20, 12
    packed = orc.pack2(s)
    gidx = amd.QGramIndex.build(packed, 2, n, q, 2, qlut)
    assert gidx.n_qgrams == n
    first = 12_345_678
    g, p = amd.generate_qgrams(q, 2, packed, 2, n, first, 1 << 20, sort=True)
    qf = amd.QGramFilter()
    n_hits = qf.rank(gidx, g, p)
    assert n_hits >= 1 << 20
    hits = amd.u32(qf.locate(0, n_hits)).reshape(-1, 2)
    want_g = O.qgrams_at(s, 0, n, hits[:, 1].astype(np.int64), q, 2)
    got_g = O.qgrams_at(s, 0, n, hits[:, 0].astype(np.int64), q, 2)
    assert np.array_equal(want_g, got_g)
    sizes = np.diff(np.concatenate([[0], u64(qf.slots()).astype(np.int64)]))
    allg = np.sort(O.qgrams_at(s, 0, n, np.arange(n), q, 2))
    gq = u64(g)
    cnt = np.searchsorted(allg, gq, "right") - np.searchsorted(allg, gq, "left")
    assert np.array_equal(sizes, cnt)
    gidx.close()
