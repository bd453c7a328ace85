"""CPU-only: a numpy restatement of the q-group index (nvbio/qgram/qgroup.h, qgroup_inl.h) with the library's departures
(include/nvbio_amd.h), derived from the pinned restatement of the sorted q-gram index in tests/test_qgram_oracle.py and checked
here against brute-force definitions.  tests/test_gpu_qgroup*.py compare the library with it.  A self-check of the oracle: it
does not touch the library."""
import numpy as np
import pytest

import test_qgram_oracle as O


def popc(x):
    """the number of set bits of every uint32"""
    x = np.asarray(x, np.uint32).astype(np.uint64)
    x = x - ((x >> np.uint64(1)) & np.uint64(0x55555555))
    x = (x & np.uint64(0x33333333)) + ((x >> np.uint64(2)) & np.uint64(0x33333333))
    x = (x + (x >> np.uint64(4))) & np.uint64(0x0F0F0F0F)
    return ((x * np.uint64(0x01010101)) >> np.uint64(24)).astype(np.uint32) & np.uint32(0xFF)


def n_words(q, ss):
    """W + 1 with W = A^q / 32 (integer division)"""
    return (1 << (q * ss)) // 32 + 1


def group_of(idx, dense=True):
    """I, S, SS, P of the q-group index that holds what the sorted index `idx` (O.string_index / O.set_index) holds.  The defined
    slot order makes SS = slots and P = index; the set bits of I are the unique q-grams.  dense=False leaves I and S out (a table
    too large for the host) and keeps the set-bit list `qgrams`."""
    q, ss, g = idx["q"], idx["ss"], idx["qgrams"]
    out = dict(q=q, ss=ss, n_words=n_words(q, ss), SS=idx["slots"], P=idx["index"], n_unique=len(g), n_qgrams=idx["n_qgrams"], qgrams=g)
    if dense:
        I = np.zeros(out["n_words"], np.uint32)
        np.bitwise_or.at(I, (g >> np.uint64(5)).astype(np.int64), np.uint32(1) << (g & np.uint64(31)).astype(np.uint32))
        out["I"] = I
        out["S"] = np.concatenate([[0], np.cumsum(popc(I).astype(np.uint64))[:-1]]).astype(np.uint32)
    return out


def ranges_of(grp, g):
    """range(g) (qgroup.h:112-130): (0, 0) if g >= A^q or its bit is clear, else (SS[S[i] + j'], SS[S[i] + j' + 1])"""
    g = np.asarray(g, np.uint64)
    valid = g < np.uint64(1 << (grp["q"] * grp["ss"]))
    i = np.where(valid, g >> np.uint64(5), 0).astype(np.int64)
    j = (g & np.uint64(31)).astype(np.uint32)
    w = grp["I"][i]
    hit = valid & (((w >> j) & np.uint32(1)) == 1)
    r = (grp["S"][i] + popc(w & ((np.uint32(1) << j) - np.uint32(1)))).astype(np.int64)
    out = np.zeros((len(g), 2), np.uint32)
    out[hit, 0] = grp["SS"][r[hit]]
    out[hit, 1] = grp["SS"][r[hit] + 1]
    return out


# ---- self-checks ----------------------------------------------------------------------------------------------------------------
def test_popc():
    x = np.array([0, 1, 0x80000000, 0xFFFFFFFF, 0x12345678], np.uint32)
    assert popc(x).tolist() == [bin(int(v)).count("1") for v in x]


@pytest.mark.parametrize("q,ss", [(1, 2), (2, 2), (1, 4), (4, 1), (3, 2), (5, 2), (3, 4), (8, 2), (2, 8), (12, 2)])
def test_word_counts_and_ranks(q, ss):
    rng = np.random.default_rng(q * 10 + ss)
    s = rng.integers(0, 1 << min(ss, 3), 3000, dtype=np.uint8)
    idx = O.string_index(s, q, ss)
    grp = group_of(idx)
    W = (1 << (q * ss)) // 32
    assert len(grp["I"]) == W + 1 and len(grp["S"]) == W + 1 and grp["n_words"] == W + 1
    if q * ss < 5:
        assert W == 0 and grp["S"][0] == 0                     # the one word holds every bit: the reference's n_unique = S[W] is 0 here
    else:
        assert grp["S"][W] == grp["n_unique"] and grp["I"][W] == 0
    assert int(grp["S"][W]) + int(popc(grp["I"][W:])[0]) == grp["n_unique"]     # the library's n_unique, for every q * ss
    assert int(popc(grp["I"]).sum()) == grp["n_unique"]
    # the bits, by brute force
    allg = {O._brute_qgram(s, p, q, ss) for p in range(len(s))}
    bits = {(i << 5) | j for i, w in enumerate(grp["I"].tolist()) for j in range(32) if (w >> j) & 1}
    assert bits == allg
    assert len(grp["SS"]) == grp["n_unique"] + 1 and grp["SS"][-1] == grp["n_qgrams"] == len(grp["P"])


@pytest.mark.parametrize("q,ss", [(1, 2), (2, 2), (6, 2), (3, 4), (10, 2)])
def test_range_equals_the_sorted_index(q, ss):
    rng = np.random.default_rng(q + ss)
    s = rng.integers(0, 4, 2000, dtype=np.uint8)
    s[100:200] = s[1000:1100]
    idx = O.string_index(s, q, ss)
    grp = group_of(idx)
    top = 1 << (q * ss)
    queries = np.concatenate([idx["qgrams"], np.arange(min(top, 5000), dtype=np.uint64),                 # occurring and absent
                              rng.integers(0, top, 500, dtype=np.uint64),
                              np.array([top, top + 1, top + 31, top + 32, 1 << 40, (1 << 64) - 1], np.uint64)])   # >= A^q: misses
    got = ranges_of(grp, queries)
    assert np.array_equal(got, O.ranges_of(idx, queries))
    assert np.all(got[queries >= np.uint64(top)] == 0)
    # and by brute force
    allg = O.qgrams_at(s, 0, len(s), np.arange(len(s)), q, ss)
    for g, (b, e) in zip(queries[::37].tolist(), got[::37].tolist()):
        assert list(grp["P"][b:e]) == [p for p in range(len(s)) if int(allg[p]) == g]


def test_all_a_text_is_one_slot():
    n = 1000
    grp = group_of(O.string_index(np.zeros(n, np.uint8), 12, 2))
    assert grp["n_unique"] == 1 and grp["I"][0] == 1 and not grp["I"][1:].any()
    assert list(grp["SS"]) == [0, n] and np.array_equal(grp["P"], np.arange(n, dtype=np.uint32))
    assert ranges_of(grp, np.array([0, 1], np.uint64)).tolist() == [[0, n], [0, 0]]


def test_set_form_orders_string_major_then_position():
    rng = np.random.default_rng(2)
    strings = [rng.integers(0, 2, L, dtype=np.uint8) for L in (0, 3, 30, 4, 31, 5)]
    idx = O.set_index(strings, 4, 2, 3)
    grp = group_of(idx)
    for u in range(grp["n_unique"]):
        occ = [tuple(c) for c in grp["P"][grp["SS"][u]:grp["SS"][u + 1]]]
        assert occ == sorted(occ)
    assert np.array_equal(ranges_of(grp, idx["qgrams"]), O.ranges_of(idx, idx["qgrams"]))


def test_empty_input():
    for idx in (O.string_index(np.zeros(0, np.uint8), 5, 2), O.set_index([], 5, 2, 3)):
        grp = group_of(idx)
        assert grp["n_unique"] == 0 and list(grp["SS"]) == [0] and len(grp["P"]) == 0 and not grp["I"].any() and not grp["S"].any()
        assert np.all(ranges_of(grp, np.array([0, 5], np.uint64)) == 0)
