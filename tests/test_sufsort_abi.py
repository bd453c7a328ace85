"""CPU-only: the sufsort entry points are declared in include/nvbio_amd.h and exported by the library, the Python mirror has its
functions, invalid arguments are named before the device is looked for, and without a GPU every compute entry fails loudly with
NVBIO_ERR_NO_DEVICE."""
import ctypes

import numpy as np

import __graft_entry__ as ge

SYMBOLS = ("nvbio_set_suffix_count", "nvbio_set_suffix_sort", "nvbio_set_suffix_sort_flat", "nvbio_set_bwt", "nvbio_suffix_sort", "nvbio_bwt")


def _set(amd, buf, bits=2, n=4, fixed_len=10, **kw):
    s = amd._StringSet(ctypes.c_void_p(buf.ctypes.data), bits, None, 0, fixed_len, fixed_len, n, 0, 0, None)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_symbols_are_declared_and_exported():
    amd = ge.load_package()
    header = amd.abi.Header(amd.HEADER_PATH)
    L = amd.lib()
    for name in SYMBOLS:
        assert name in header.prototypes, name + " is not declared"
        assert hasattr(L, name), name + " is not exported"
    assert "nvbio_sufsort_stats" in header.structs and "NVBIO_SUFSORT_NO_EMPTY_SUFFIXES" in open(amd.HEADER_PATH).read()
    assert L.nvbio_amd_version() == 100


def test_python_mirror_has_the_functions():
    amd = ge.load_package()
    for name in ("set_suffix_count", "set_suffix_sort", "set_bwt", "suffix_sort", "bwt"):
        assert callable(getattr(amd, name))
    assert amd.SUFSORT_NO_EMPTY_SUFFIXES == 1
    assert ctypes.sizeof(amd._SufsortStats) == 88                   # 19 uint32, padding, one uint64


def test_arguments_are_checked_before_the_device():
    amd = ge.load_package()
    L = amd.lib()
    buf = np.zeros(64, np.uint32)
    out = ctypes.c_void_p(buf.ctypes.data)
    n = ctypes.c_uint32(7)
    bad = [_set(amd, buf, bits=3), _set(amd, buf, bits=1), _set(amd, buf, seeds_per_string=2), _set(amd, buf, seed_intervals_dev=buf.ctypes.data),
           _set(amd, buf, offsets_are_ranges=1), _set(amd, buf, symbols_dev=None), _set(amd, buf, n=0xFFFFFFFF)]
    for s in bad:
        assert L.nvbio_set_suffix_count(0, ctypes.byref(s), 0, ctypes.byref(n), None) == 1
        assert b"invalid argument" in L.nvbio_amd_last_error()
        assert L.nvbio_set_suffix_sort(0, ctypes.byref(s), 0, out, None, ctypes.c_uint64(64), ctypes.byref(n), None, None) == 1
        assert L.nvbio_set_bwt(0, ctypes.byref(s), 0, out, None, ctypes.c_uint64(64), ctypes.byref(n), None, None) == 1
        assert L.nvbio_set_suffix_sort_flat(0, ctypes.byref(s), 0, out, None, None, ctypes.c_uint64(64), ctypes.byref(n), None, None) == 1
        assert n.value == 0
    ok = _set(amd, buf)
    assert L.nvbio_set_suffix_count(0, ctypes.byref(ok), 2, ctypes.byref(n), None) == 1               # an unknown flag
    assert L.nvbio_set_suffix_count(0, None, 0, ctypes.byref(n), None) == 1
    assert L.nvbio_set_suffix_count(0, ctypes.byref(ok), 0, None, None) == 1
    assert L.nvbio_set_suffix_sort(0, ctypes.byref(ok), 0, out, None, ctypes.c_uint64(64), None, None, None) == 1
    assert L.nvbio_set_suffix_sort(0, ctypes.byref(ok), 0, None, None, ctypes.c_uint64(64), ctypes.byref(n), None, None) == 1
    assert L.nvbio_set_bwt(0, ctypes.byref(ok), 0, None, out, ctypes.c_uint64(64), ctypes.byref(n), None, None) == 1
    assert L.nvbio_suffix_sort(None, 100, 0, out, None) == 1 and L.nvbio_suffix_sort(out, 100, 0, None, None) == 1
    assert L.nvbio_suffix_sort(out, 0, 0, out, None) == 1
    assert L.nvbio_bwt(out, 100, 0, out, None, None) == 1 and L.nvbio_bwt(out, 0, 0, out, ctypes.byref(n), None) == 1


def test_no_device_no_sort():
    import torch
    amd = ge.load_package()
    L = amd.lib()
    if torch.cuda.is_available():
        return                                                       # tests/test_gpu_sufsort.py covers the calls on a GPU
    buf = np.zeros(64, np.uint32)
    out = ctypes.c_void_p(buf.ctypes.data)
    n = ctypes.c_uint32(0)
    s = _set(amd, buf)
    assert L.nvbio_set_suffix_count(0, ctypes.byref(s), 0, ctypes.byref(n), None) == 5               # NVBIO_ERR_NO_DEVICE: no CPU fallback
    assert L.nvbio_set_suffix_sort(0, ctypes.byref(s), 0, out, None, ctypes.c_uint64(64), ctypes.byref(n), None, None) == 5
    assert L.nvbio_set_bwt(0, ctypes.byref(s), 1, out, None, ctypes.c_uint64(64), ctypes.byref(n), None, None) == 5
    assert L.nvbio_set_suffix_sort_flat(0, ctypes.byref(s), 0, out, out, None, ctypes.c_uint64(64), ctypes.byref(n), None, None) == 5
    assert L.nvbio_suffix_sort(out, 100, 0, out, None) == 5
    assert L.nvbio_bwt(out, 100, 0, out, ctypes.byref(n), None) == 5
    assert n.value == 0
