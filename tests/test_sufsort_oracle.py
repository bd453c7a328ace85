"""CPU-only: a brute-force restatement of the sufsort module's semantics (include/nvbio_amd.h, "sufsort"), the reference of
tests/test_gpu_sufsort.py, and its self-checks on cases written out by hand.

A suffix is (pos, string_id), 0 <= pos <= len; it compares by its symbols, a proper prefix first, then by string_id.  Python's bytes
order is exactly that: symbol by symbol, the shorter of two that agree first."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NO_EMPTY = 1                                                         # NVBIO_SUFSORT_NO_EMPTY_SUFFIXES


def set_suffix_sort(strings, no_empty=False):
    """strings: a list of uint8 symbol arrays.  -> (suffixes uint32 [n, 2] = (pos, string_id), global uint32 [n], bwt uint8 [n])"""
    extra = 0 if no_empty else 1
    items, base, g = [], [], 0
    for sid, s in enumerate(strings):
        b = np.asarray(s, np.uint8).tobytes()
        base.append(g)
        g += len(b) + extra
        for pos in range(len(b) + extra):
            items.append((b[pos:], sid, pos))
    items.sort(key=lambda t: (t[0], t[1]))
    n = len(items)
    suf = np.zeros((n, 2), np.uint32)
    glb = np.zeros(n, np.uint32)
    bwt = np.zeros(n, np.uint8)
    for r, (_, sid, pos) in enumerate(items):
        suf[r] = (pos, sid)
        glb[r] = base[sid] + pos
        bwt[r] = strings[sid][pos - 1] if pos else 255
    return suf, glb, bwt


def suffix_array(text):
    """the suffix array of one string in the convention of nvbio/fmindex/bwt.h:28-37: n + 1 rows, row 0 = the empty suffix (SA[0] = n)"""
    b = np.asarray(text, np.uint8).tobytes()
    return np.array(sorted(range(len(b) + 1), key=lambda i: b[i:]), np.uint32)


def bwt_of(text, sa):
    """gen_bwt_from_sa (bwt.h:41-53): the BWT symbols with the primary row squeezed out, and primary"""
    n = len(text)
    primary = int(np.nonzero(sa == 0)[0][0])
    rows = np.concatenate([sa[:primary], sa[primary + 1:]]).astype(np.int64)
    return np.asarray(text, np.uint8)[rows - 1][:n], primary


def pack2_words(syms):
    """2-bit big-endian words, 16 symbols each"""
    syms = np.asarray(syms, np.uint32)
    pad = np.concatenate([syms, np.zeros((-len(syms)) % 16, np.uint32)]).reshape(-1, 16)
    return (pad << (30 - 2 * np.arange(16, dtype=np.uint32))).sum(axis=1).astype(np.uint32)


A, C, G, T = 0, 1, 2, 3


def _s(*x):
    return np.array(x, np.uint8)


def test_hand_written_set():
    strings = [_s(A, C, A), _s(A), _s(), _s(A, C, A)]
    suf, glb, bwt = set_suffix_sort(strings)
    # the four empty suffixes in string order; then "A" of strings 0, 1, 3 (ended-and-equal: by string id); "ACA" of 0 and 3; "CA" of both
    want = [(3, 0), (1, 1), (0, 2), (3, 3), (2, 0), (0, 1), (2, 3), (0, 0), (0, 3), (1, 0), (1, 3)]
    assert [tuple(int(v) for v in x) for x in suf] == want
    # global index: the strings start at 0, 4, 6, 7 (len + 1 each)
    assert glb.tolist() == [3, 5, 6, 10, 2, 4, 9, 0, 7, 1, 8]
    assert bwt.tolist() == [A, A, 255, A, C, 255, C, 255, 255, A, A]

    suf, glb, bwt = set_suffix_sort(strings, no_empty=True)
    want = [(2, 0), (0, 1), (2, 3), (0, 0), (0, 3), (1, 0), (1, 3)]
    assert [tuple(int(v) for v in x) for x in suf] == want
    assert glb.tolist() == [2, 3, 6, 0, 4, 1, 5]                     # the strings start at 0, 3, 4, 4 (len each)
    assert bwt.tolist() == [C, 255, C, 255, 255, A, A]


def test_prefix_sorts_before_symbol_zero():
    """the implicit '$' is below symbol 0: "A" < "AA" < "AAC" whatever the string ids; the two "A" by string id"""
    suf, _, _ = set_suffix_sort([_s(A, A, C), _s(A, A), _s(A)], no_empty=True)
    assert [tuple(int(v) for v in x) for x in suf] == [(1, 1), (0, 2), (0, 1), (0, 0), (1, 0), (2, 0)]


def test_empty_set_and_empty_strings():
    suf, glb, bwt = set_suffix_sort([])
    assert suf.shape == (0, 2) and len(glb) == 0 and len(bwt) == 0
    suf, glb, bwt = set_suffix_sort([_s(), _s()])
    assert suf.tolist() == [[0, 0], [0, 1]] and glb.tolist() == [0, 1] and bwt.tolist() == [255, 255]
    assert len(set_suffix_sort([_s(), _s()], no_empty=True)[1]) == 0


def test_banana():
    b, a, n = 1, 0, 2
    text = _s(b, a, n, a, n, a)
    sa = suffix_array(text)
    assert sa.tolist() == [6, 5, 3, 1, 0, 4, 2]                      # $, a, ana, anana, banana, na, nana
    bwt, primary = bwt_of(text, sa)
    assert primary == 4 and bwt.tolist() == [a, n, n, b, a, a]      # "annb$aa" without the '$' of row 4


def test_convention_of_the_fm_golden():
    """rows 1..n of fm_golden.npz's suffix array are the sorted suffixes and its row 0 is the empty suffix, which the golden (the
    FM-index's sampled-SA view of it) writes as -1 and bwt.h's gen_sa as n; primary is the row of suffix 0"""
    z = np.load(os.path.join(GOLDEN, "fm_golden.npz"), allow_pickle=False)
    text, gsa = z["text"], z["sa"]
    sa = suffix_array(text)
    assert len(sa) == len(gsa) == len(text) + 1
    assert np.array_equal(sa[1:], gsa[1:])
    assert sa[0] == len(text) and gsa[0] in (len(text), 0xFFFFFFFF)
    bwt, primary = bwt_of(text, sa)
    assert primary == int(z["primary"])
    words = z["bwt_occ"].reshape(-1, 8)[:, :4].reshape(-1)[:(len(text) + 15) // 16]
    assert np.array_equal(pack2_words(bwt), words)
