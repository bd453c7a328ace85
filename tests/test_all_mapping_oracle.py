"""CPU-only: the restatement of nvBowtie's all-mapping mode (tests/all_mapping_cpu.py) that the GPU tests compare against is sane and its
shared input exercises what it should; the mode's symbols are declared, exported, and refuse to run without a GPU."""
import ctypes

import numpy as np
import pytest

import __graft_entry__ as ge
import oracle
from all_mapping_cpu import all_mapping_cpu, band_length, revcomp, shared_input

MAX_DIST = 15


@pytest.fixture(scope="module")
def restated(orc):
    text, reads, planted = shared_input()
    hidx = orc.build_index(text)
    rec, det = all_mapping_cpu(orc, hidx, text, len(text), reads, oracle.SEMI_GLOBAL, MAX_DIST, want_cigars=True)
    return text, reads, planted, rec, det


def semi_global_edit_distance(pat, txt):
    """plain numpy: the least number of edits that turn `pat` into some substring of `txt` (the text's ends are free)"""
    prev = np.zeros(len(txt) + 1, dtype=np.int64)
    for i, c in enumerate(pat, 1):
        sub = prev[:-1] + ((txt != c) | (c > 3))
        cur = np.minimum(sub, prev[1:] + 1)
        cur = np.concatenate([[i], cur])
        cur = np.minimum.accumulate(cur - np.arange(len(cur))) + np.arange(len(cur))     # insertions of text symbols, left to right
        prev = cur
    return int(prev.min())


def test_band_length_is_the_reference_function():
    assert band_length(15) == 31 and band_length(3) == 7 and band_length(0) == 3 and band_length(16) == 63


def test_scores_are_bounded_by_an_independent_edit_distance(restated):
    text, reads, _, rec, _ = restated
    band, M, n = band_length(MAX_DIST), reads.shape[1], len(text)
    for r, rc, loc, score in rec:
        assert -MAX_DIST <= score <= 0
        begin = loc - band // 2 if loc > band // 2 else 0
        end = min(begin + band + M, n)
        pat = revcomp(reads[r]) if rc else reads[r]
        assert semi_global_edit_distance(pat, text[begin:end]) <= -score, (r, rc, loc, score)


def test_planted_exact_copies_are_found_with_score_zero(restated):
    _, _, planted, rec, _ = restated
    zero = {(r, rc, loc) for r, rc, loc, s in rec if s == 0}
    assert len(planted) >= 8
    for p in planted:
        assert p in zero, p


def test_shared_input_is_not_vacuous(restated):
    _, reads, _, rec, det = restated
    a = np.array(rec, dtype=np.int64)
    per_read = np.bincount(a[:, 0], minlength=len(reads))
    assert len(rec) >= 2000
    assert int((per_read > 10).sum()) >= 20
    assert int((per_read == 0).sum()) >= 10
    assert int((a[:, 3] < 0).sum()) * 5 >= len(rec)
    assert len(set(rec)) * 2 <= len(rec)
    assert any(any((int(c) & 3) == 1 for c in d[3]) for d in det) and any(any((int(c) & 3) == 2 for c in d[3]) for d in det)
    # at 100 bp: S = 12, max_seeds = 8, first offset 8, so seed indices 6 and 7 have no seed
    assert 100 // 12 == 8 and 8 + 5 * 12 + 22 <= 100 < 8 + 6 * 12 + 22


NEW_SYMBOLS = ("nvbio_all_hits_scan_temp_bytes", "nvbio_all_hits_scan", "nvbio_all_hits_select", "nvbio_all_hits_unique_temp_bytes",
               "nvbio_all_hits_unique", "nvbio_all_score_output_temp_bytes", "nvbio_all_score_output", "nvbio_all_traceback_flatten")


def test_symbols_are_declared_and_exported():
    amd = ge.load_package()
    declared = amd.abi.Header(amd.HEADER_PATH).prototypes
    L = amd.lib()
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(L, s), s
    from importlib import import_module
    host = import_module("nvbio_gpl_amd.pipeline")._host_lib()
    assert hasattr(host, "nvbio_host_all_mapping")
    assert callable(amd.all_mapping) and callable(amd.all_hits_scan) and callable(amd.all_hits_select) and callable(amd.all_hits_unique)
    assert callable(amd.all_score_output) and callable(amd.all_traceback_flatten)


def test_scan_fails_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    amd = ge.load_package()
    buf = np.zeros(64, dtype=np.uint64)
    p = amd._AllHitsParams(1, 8, 12, 22, 100)
    at = lambda k: ctypes.c_void_p(buf.ctypes.data + 64 * k)
    st = amd.lib().nvbio_all_hits_scan(0, at(0), at(1), ctypes.c_uint32(1), ctypes.byref(p), at(2), at(3), at(4), ctypes.c_uint64(256), None)
    assert st == 5, st                                  # NVBIO_ERR_NO_DEVICE
