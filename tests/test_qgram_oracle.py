"""CPU-only: a numpy restatement of the q-gram index, set index and filter (nvbio/qgram/qgram.h, qgram_inl.h, filter_inl.h) with the
library's departures (include/nvbio_amd.h), checked here against brute-force definitions.  tests/test_gpu_qgram*.py compare the
library with it.  A self-check of the oracle: it does not touch the library."""
import numpy as np
import pytest

M32 = np.uint64(0xFFFFFFFF)


# ---- packing (string_qgram_functor / string_set_qgram_functor, qgram.h:793-886) ---------------------------------------------------
def qgrams_at(syms, begin, length, pos, q, ss):
    """the q-gram of q symbols at string positions pos (array) of a string at `begin` of `length` symbols: the first symbol in the
    least significant bits, (s & mask) << j * ss, 0 past the end"""
    syms = np.asarray(syms, np.uint8)
    pos = np.asarray(pos, np.int64)
    mask = np.uint64((1 << ss) - 1)
    g = np.zeros(pos.shape, np.uint64)
    for j in range(q):
        p = pos + j
        ok = p < length
        s = np.zeros(pos.shape, np.uint64)
        if ok.any():
            s[ok] = syms[begin + p[ok]].astype(np.uint64) & mask
        g |= s << np.uint64(j * ss)
    return g


def lut_of(qgrams, q, ss, qlut):
    """lut[k] = lower_bound( qgrams, k << QLS ) for k < A^QL, lut[A^QL] = n_unique (qgram_inl.h:122-140); None without a LUT"""
    if qlut == 0:
        return None
    qls = (q - qlut) * ss
    keys = np.arange(1 << (qlut * ss), dtype=np.uint64) << np.uint64(qls)
    return np.concatenate([np.searchsorted(qgrams, keys, "left"), [len(qgrams)]]).astype(np.uint32)


def _finish(g, coords, q, ss, qlut):
    order = np.argsort(g, kind="stable")                      # the stable radix sort over [0, q * ss)
    sg = g[order]
    qgrams, counts = np.unique(sg, return_counts=True)
    slots = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    return dict(q=q, ss=ss, qlut=qlut, qgrams=qgrams.astype(np.uint64), slots=slots, index=coords[order], lut=lut_of(qgrams, q, ss, qlut),
                n_qgrams=len(g))


def string_index(syms, q, ss, qlut=0):
    """QGramIndexDevice::build: every position, padded; index = uint32 positions"""
    n = len(syms)
    g = qgrams_at(syms, 0, n, np.arange(n), q, ss)
    return _finish(g, np.arange(n, dtype=np.uint32), q, ss, qlut)


def seed_coords(lengths, q, interval):
    """uniform_seeds_functor( q, interval ) over a set: (string_id, pos) for pos = k * interval, pos + q <= len, string-major"""
    out = [np.stack([np.full(len(range(0, L - q + 1, interval)), i, np.uint32), np.arange(0, L - q + 1, interval, dtype=np.uint32)], 1)
           for i, L in enumerate(lengths) if L >= q]
    return np.concatenate(out) if out else np.zeros((0, 2), np.uint32)


def set_index(strings, q, ss, interval, qlut=0):
    """QGramSetIndexDevice::build over a list of symbol arrays; index = (string_id, string_pos) pairs"""
    coords = seed_coords([len(s) for s in strings], q, interval)
    g = np.array([qgrams_at(strings[i], 0, len(strings[i]), [p], q, ss)[0] for i, p in coords], np.uint64) if len(coords) else \
        np.zeros(0, np.uint64)
    return _finish(g, coords, q, ss, qlut)


# ---- search and filter (qgram.h:451-475, filter_inl.h:336-410) --------------------------------------------------------------------
def ranges_of(idx, g):
    """range(g): lower_bound inside the LUT bucket (everything without one); half-open [slots[i], slots[i+1]), (0, 0) on a miss"""
    g = np.asarray(g, np.uint64)
    qg, n_unique = idx["qgrams"], len(idx["qgrams"])
    lo, hi = np.zeros(len(g), np.int64), np.full(len(g), n_unique, np.int64)
    valid = np.ones(len(g), bool)
    if idx["lut"] is not None:
        lut = idx["lut"]
        k = g >> np.uint64((idx["q"] - idx["qlut"]) * idx["ss"])
        valid = k < np.uint64(len(lut) - 1)
        kk = np.where(valid, k, 0).astype(np.int64)
        lo, hi = lut[kk].astype(np.int64), lut[kk + 1].astype(np.int64)
    i = np.clip(np.searchsorted(qg, g, "left"), lo, hi)
    hit = valid & (i < n_unique)
    hit[hit] = qg[i[hit]] == g[hit]
    out = np.zeros((len(g), 2), np.uint32)
    out[hit, 0] = idx["slots"][i[hit]]
    out[hit, 1] = idx["slots"][i[hit] + 1]
    return out


def rank(idx, g):
    """ranges, slots (inclusive uint64 scan of the sizes), n_hits (0 without queries)"""
    r = ranges_of(idx, g)
    slots = np.cumsum((r[:, 1].astype(np.int64) - r[:, 0].astype(np.int64))).astype(np.uint64)
    return r, slots, int(slots[-1]) if len(slots) else 0


def locate(idx, r, slots, indices, begin, end):
    """outputs [begin, end): output o belongs to query i = upper_bound( o, slots ); uint2 (index position, indices[i]) or uint4
    (string_id, string_pos, indices[i], 0)"""
    o = np.arange(begin, end, dtype=np.uint64)
    i = np.searchsorted(slots, o, "right")
    base = np.where(i > 0, slots[np.maximum(i - 1, 0)], 0).astype(np.uint64)
    at = (r[i, 0].astype(np.uint64) + o - base).astype(np.int64)
    ix = np.asarray(indices, np.uint32)[i]
    if idx["index"].ndim == 2:
        c = idx["index"][at]
        return np.stack([c[:, 0], c[:, 1], ix, np.zeros(len(o), np.uint32)], 1).astype(np.uint32)
    return np.stack([idx["index"][at], ix], 1).astype(np.uint32)


def snap(d, interval):
    """the closest multiple of interval to the uint32 diagonal d, ties down, mod 2^32 (the departure from util::round's r + 1)"""
    d = np.asarray(d, np.uint64) & M32
    iv = np.uint64(interval)
    r = (d // iv) * iv
    x = d - r
    return np.where(x > iv - x, (r + iv) & M32, r).astype(np.uint64)


def reference_round(d, interval):
    """util::round as the reference writes it (numbers.h:149-153): r + 1 where it means r + interval"""
    d = np.asarray(d, np.uint64) & M32
    iv = np.uint64(interval)
    r = (d // iv) * iv
    return np.where(((d - r) * np.uint64(2)) & M32 > iv, r + np.uint64(1), r).astype(np.uint64)


def merge(hits, interval):
    """(merged, counts): string hits (index_pos, text_pos) -> uint32 diagonals; set hits (string_id, string_pos, text_pos, 0) ->
    (diagonal, string_id) ordered by string id, then diagonal; counts uint32"""
    h = np.asarray(hits, np.uint64)
    if h.shape[1] == 2:
        key = snap((h[:, 1] - h[:, 0]) & M32, interval)
        u, c = np.unique(key, return_counts=True)
        return u.astype(np.uint32), c.astype(np.uint32)
    key = snap((h[:, 2] - h[:, 1]) & M32, interval) | (h[:, 0] << np.uint64(32))
    u, c = np.unique(key, return_counts=True)
    return np.stack([(u & M32).astype(np.uint32), (u >> np.uint64(32)).astype(np.uint32)], 1), c.astype(np.uint32)


def generate(syms, text_len, q, ss, first, n, sort):
    """qmap's build_qgrams: the q-grams at [first, first + n), padded past text_len; sort: stably by q-gram"""
    pos = np.arange(first, first + n, dtype=np.int64)
    g = qgrams_at(syms, 0, text_len, pos, q, ss)
    if sort:
        o = np.argsort(g, kind="stable")
        return g[o], pos[o].astype(np.uint32)
    return g, pos.astype(np.uint32)


# ---- self-checks against brute-force definitions ------------------------------------------------------------------------------
def _brute_qgram(s, p, q, ss):
    return sum(((int(s[p + j]) if p + j < len(s) else 0) & ((1 << ss) - 1)) << (j * ss) for j in range(q))


@pytest.mark.parametrize("q,ss", [(1, 2), (5, 2), (12, 2), (20, 2), (31, 2), (32, 2), (5, 4), (16, 4), (8, 8), (64, 1)])
def test_packing_first_symbol_lowest(q, ss):
    rng = np.random.default_rng(q * 10 + ss)
    s = rng.integers(0, 1 << min(ss, 3), 50, dtype=np.uint8)
    g = qgrams_at(s, 0, len(s), np.arange(len(s)), q, ss)
    assert [int(x) for x in g] == [_brute_qgram(s, p, q, ss) for p in range(len(s))]


def test_n_becomes_a_with_two_bit_symbols():
    s = np.array([4, 1, 4, 2], np.uint8)                       # DNA_N's N = 4
    assert int(qgrams_at(s, 0, 4, [0], 4, 2)[0]) == (0 | 1 << 2 | 0 << 4 | 2 << 6)
    assert int(qgrams_at(s, 0, 4, [0], 4, 4)[0]) == (4 | 1 << 4 | 4 << 8 | 2 << 12)


def test_numeric_order_is_not_lexicographic():
    a, b = np.array([0, 1], np.uint8), np.array([1, 0], np.uint8)   # "AC" < "CA" lexicographically
    assert int(qgrams_at(a, 0, 2, [0], 2, 2)[0]) > int(qgrams_at(b, 0, 2, [0], 2, 2)[0])


@pytest.mark.parametrize("n,q,qlut", [(1, 5, 0), (3, 5, 1), (500, 5, 2), (2000, 8, 8), (2000, 12, 8), (700, 20, 0), (700, 1, 1)])
def test_string_index_against_definitions(n, q, qlut):
    rng = np.random.default_rng(n + q)
    s = rng.integers(0, 4, n, dtype=np.uint8)
    idx = string_index(s, q, 2, qlut)
    assert idx["n_qgrams"] == n and idx["slots"][-1] == n
    allg = [_brute_qgram(s, p, q, 2) for p in range(n)]
    assert [int(x) for x in idx["qgrams"]] == sorted(set(allg))
    for u, g in enumerate(idx["qgrams"]):
        occ = idx["index"][idx["slots"][u]:idx["slots"][u + 1]]
        assert list(occ) == [p for p in range(n) if allg[p] == int(g)]         # ascending position order
    if qlut:
        qls = (q - qlut) * 2
        for k in range(0, len(idx["lut"]) - 1, max(1, (len(idx["lut"]) - 1) // 97)):
            assert idx["lut"][k] == sum(1 for g in idx["qgrams"] if int(g) < (k << qls))
        assert idx["lut"][-1] == len(idx["qgrams"])


def test_all_a_text_padded_tail_collides():
    idx = string_index(np.zeros(10, np.uint8), 5, 2, 2)
    assert list(idx["qgrams"]) == [0] and list(idx["slots"]) == [0, 10] and list(idx["index"]) == list(range(10))


@pytest.mark.parametrize("interval", [1, 3, 10])
def test_set_index_seeds(interval):
    rng = np.random.default_rng(interval)
    strings = [rng.integers(0, 4, L, dtype=np.uint8) for L in (0, 3, 5, 6, 17, 40, 41)]
    q = 5
    idx = set_index(strings, q, 2, interval, 2)
    want = [(i, p) for i, s in enumerate(strings) for p in range(0, len(s) - q + 1, interval)]
    assert idx["n_qgrams"] == len(want)
    for u, g in enumerate(idx["qgrams"]):
        occ = [tuple(c) for c in idx["index"][idx["slots"][u]:idx["slots"][u + 1]]]
        assert occ == [c for c in want if _brute_qgram(strings[c[0]], c[1], q, 2) == int(g)]   # string-major, then position


def test_empty_set():
    idx = set_index([], 5, 2, 3, 2)
    assert idx["n_qgrams"] == 0 and list(idx["slots"]) == [0] and len(idx["qgrams"]) == 0 and np.all(idx["lut"] == 0)


@pytest.mark.parametrize("qlut", [0, 1, 4, 6])
def test_rank_locate_equal_brute_force(qlut):
    rng = np.random.default_rng(qlut)
    s = rng.integers(0, 4, 3000, dtype=np.uint8)
    s[1000:1100] = s[2000:2100]                                  # a repeat
    q = 6
    idx = string_index(s, q, 2, qlut)
    allg = qgrams_at(s, 0, len(s), np.arange(len(s)), q, 2)
    queries = np.concatenate([allg[rng.integers(0, len(s), 200)], rng.integers(0, 1 << 12, 50).astype(np.uint64),
                              np.array([1 << 40], np.uint64)])   # bits above q * ss: a miss
    indices = rng.integers(0, 1 << 31, len(queries)).astype(np.uint32)
    r, slots, n_hits = rank(idx, queries)
    assert n_hits == sum(int((allg == g).sum()) for g in queries)
    hits = locate(idx, r, slots, indices, 0, n_hits)
    o = 0
    for i, g in enumerate(queries):
        want = np.nonzero(allg == g)[0]
        got = hits[o:o + len(want)]
        assert list(got[:, 0]) == list(want) and np.all(got[:, 1] == indices[i])
        o += len(want)
    # a sub-range cutting through queries
    assert np.array_equal(locate(idx, r, slots, indices, 7, n_hits - 5), hits[7:n_hits - 5])


def test_no_queries_is_zero_hits():
    idx = string_index(np.zeros(4, np.uint8), 2, 2)
    assert rank(idx, np.zeros(0, np.uint64))[2] == 0


def test_set_locate_equal_brute_force():
    rng = np.random.default_rng(5)
    strings = [rng.integers(0, 4, L, dtype=np.uint8) for L in rng.integers(5, 60, 40)]
    q = 4
    idx = set_index(strings, q, 2, 3)
    text = rng.integers(0, 4, 500, dtype=np.uint8)
    g = qgrams_at(text, 0, len(text), np.arange(len(text)), q, 2)
    r, slots, n_hits = rank(idx, g)
    hits = locate(idx, r, slots, np.arange(len(text), dtype=np.uint32), 0, n_hits)
    seeds = seed_coords([len(s) for s in strings], q, 3)
    want = sorted((int(i), int(p), t) for t in range(len(text)) for i, p in seeds
                  if _brute_qgram(strings[i], p, q, 2) == int(g[t]))
    assert sorted(map(tuple, hits[:, :3].tolist())) == want and np.all(hits[:, 3] == 0)


@pytest.mark.parametrize("interval", [1, 2, 3, 7, 16, 1000, 0x80000001])
def test_snap_is_nearest_multiple(interval):
    rng = np.random.default_rng(interval % 1000)
    d = np.concatenate([rng.integers(0, 1 << 32, 2000, dtype=np.uint64),
                        np.array([0, 1, 2, 3, interval // 2, interval // 2 + 1, (1 << 32) - 1, (1 << 32) - 3, (1 << 32) - interval], np.uint64)])
    got = snap(d, interval)
    for x, y in zip(d.tolist(), got.tolist()):
        r = (x // interval) * interval
        best = r if (x - r) * 2 <= interval else r + interval        # nearest, ties down, as integers
        assert y == best % (1 << 32)
        assert y % interval == 0 or best >= 1 << 32               # a multiple (unless it wrapped past 2^32)


def test_snap_minus_three_is_zero_and_reference_round_is_not():
    d = np.array([(1 << 32) - 3], np.uint64)                      # diagonal -3
    assert int(snap(d, 16)[0]) == 0
    assert int(reference_round(d, 16)[0]) == (1 << 32) - 16 + 1   # r + 1: not a multiple, 15 from the truth


@pytest.mark.parametrize("interval", [1, 5, 16])
def test_merge_counts_sum_to_hits(interval):
    rng = np.random.default_rng(interval)
    h2 = rng.integers(0, 1 << 32, (500, 2), dtype=np.uint64).astype(np.uint32)
    h2[:100, 1] = h2[:100, 0] - rng.integers(0, 5, 100).astype(np.uint32)   # negative diagonals: wrap
    m, c = merge(h2, interval)
    assert c.sum() == len(h2) and np.all(np.diff(m.astype(np.int64)) > 0)
    d = snap((h2[:, 1].astype(np.uint64) - h2[:, 0]) & M32, interval)
    for x, k in zip(m, c):
        assert (d == x).sum() == k
    h4 = np.zeros((500, 4), np.uint32)
    h4[:, 0] = rng.integers(0, 7, 500)
    h4[:, 1] = rng.integers(0, 200, 500)
    h4[:, 2] = rng.integers(0, 300, 500)
    m4, c4 = merge(h4, interval)
    assert c4.sum() == 500
    key = m4[:, 1].astype(np.uint64) << np.uint64(32) | m4[:, 0]
    assert np.all(np.diff(key.astype(np.float64)) > 0)            # by string id, then diagonal


def test_generate_sorted_is_stable():
    s = np.zeros(40, np.uint8)
    s[5] = 1
    g, p = generate(s, 30, 3, 2, 2, 30, True)
    assert np.all(np.diff(g.astype(np.float64)) >= 0)
    for v in np.unique(g):
        assert np.all(np.diff(p[g == v].astype(np.int64)) > 0)
