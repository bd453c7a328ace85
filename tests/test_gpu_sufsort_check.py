"""GPU: the set suffix sort and the set BWT under the scratch check mode (amd.set_scratch_check) for fills 0x00, 0xFF and 0x02.  The
calls' own buffers (BuildBuffers) are filled by the library before any work, so a key, a segment or a list entry the sorter does
not write itself shows as a result that differs from the restatement of tests/test_sufsort_oracle.py; the output tensors are
filled here with the same byte.  The sorter has no ScratchBlock site, so the report must stay free of damage."""
import numpy as np
import pytest

import test_sufsort_oracle as S
from test_gpu_qgram import text_of
from test_gpu_sufsort import check_set, ragged_set

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[0x00, 0xFF, 0x02])
def fill(amd, request):
    amd.set_scratch_check(True, request.param)
    yield request.param
    report = amd.scratch_check_report()
    amd.set_scratch_check(False)
    assert not {t: r for t, r in report.items() if r[1]}, report


@pytest.mark.parametrize("bits", [2, 4, 8])
def test_set_sort_and_bwt_under_check(amd, orc, fill, bits):
    rng = np.random.default_rng(bits)
    genome = rng.integers(0, 4, 1500, dtype=np.uint8)
    lens = rng.integers(0, 120, 200)
    strings = [genome[s:s + L].copy() for s, L in zip(rng.integers(0, 1380, 200), lens)]
    strings += [np.zeros(90, np.uint8)] * 3 + [text_of(rng, 50, bits, with_n=True)]
    sset = ragged_set(amd, orc, strings, bits, lead=3)
    check_set(amd, sset, strings, bits)


def test_outputs_are_written_whole(amd, orc, fill):
    """output tensors prefilled with the fill byte: every entry up to the count is overwritten, none behind it"""
    import ctypes
    import torch
    rng = np.random.default_rng(7)
    strings = [text_of(rng, int(L), 2) for L in rng.integers(0, 70, 100)]
    sset = ragged_set(amd, orc, strings, 2)
    want_suf, want_glb, want_bwt = S.set_suffix_sort(strings)
    n = len(want_glb)
    cap = n + 64
    suf = torch.full((cap, 2), fill * 0x01010101 - (1 << 32 if fill >= 0x80 else 0), dtype=torch.int32, device="cuda:0")
    glb = suf[:, 0].clone()
    bwt = torch.full((cap,), fill, dtype=torch.uint8, device="cuda:0")
    cnt, ss = ctypes.c_uint32(0), sset.c_struct()
    L = amd.lib()
    amd._check(L.nvbio_set_suffix_sort(0, ctypes.byref(ss), 0, amd._ptr(suf), amd._ptr(glb), ctypes.c_uint64(cap), ctypes.byref(cnt), None,
                                       amd._stream_ptr("cuda:0")))
    assert cnt.value == n
    assert np.array_equal(amd.u32(suf[:n]).reshape(-1, 2), want_suf) and np.array_equal(amd.u32(glb[:n]), want_glb)
    assert bool((amd_bytes(suf[n:]) == fill).all()) and bool((amd_bytes(glb[n:]) == fill).all())
    amd._check(L.nvbio_set_bwt(0, ctypes.byref(ss), 0, amd._ptr(bwt), None, ctypes.c_uint64(cap), ctypes.byref(cnt), None,
                               amd._stream_ptr("cuda:0")))
    assert cnt.value == n and np.array_equal(bwt[:n].cpu().numpy(), want_bwt) and bool((bwt[n:] == fill).all())


def amd_bytes(t):
    import torch
    return t.contiguous().view(torch.uint8)


def test_empty_inputs_under_check(amd, orc, fill):
    e = np.zeros(0, np.uint8)
    check_set(amd, ragged_set(amd, orc, [e, e], 4), [e, e], 4)
    check_set(amd, amd.PackedStringSet(np.zeros(16, np.uint8), 8, 0, offsets=np.zeros(1, np.uint32), ranges=True), [], 8)
