"""CPU-only: the four q-group entry points are declared in include/nvbio_amd.h and exported by the library, the Python mirror has
its classes, and without a GPU the build fails loudly with NVBIO_ERR_NO_DEVICE (invalid arguments are still named first)."""
import ctypes

import numpy as np

import __graft_entry__ as ge

SYMBOLS = ("nvbio_qgroup_index_build", "nvbio_qgroup_set_index_build", "nvbio_qgroup_index_get_view", "nvbio_qgroup_index_export")


def test_symbols_are_declared_and_exported():
    amd = ge.load_package()
    header = amd.abi.Header(amd.HEADER_PATH)
    L = amd.lib()
    for name in SYMBOLS:
        assert name in header.prototypes, name + " is not declared"
        assert hasattr(L, name), name + " is not exported"
    assert "nvbio_qgroup_index_view" in header.structs
    assert L.nvbio_amd_version() == 100


def test_python_mirror_has_the_classes():
    amd = ge.load_package()
    for cls in (amd.QGroupIndex, amd.QGroupSetIndex):
        assert issubclass(cls, amd.QGramIndex)
        for name in ("build", "view", "arrays", "close", "device_bytes", "ranges"):
            assert hasattr(cls, name)
    assert amd.QGroupSetIndex.IS_SET and not amd.QGroupIndex.IS_SET


def test_arguments_are_checked_before_the_device():
    amd = ge.load_package()
    L = amd.lib()
    buf = np.zeros(64, np.uint32)
    h = ctypes.c_void_p()
    build = L.nvbio_qgroup_index_build
    for bits, q, ss in ((3, 5, 2), (2, 0, 2), (2, 5, 0), (2, 5, 9), (2, 19, 2), (2, 37, 1), (8, 5, 8)):
        assert build(0, ctypes.c_void_p(buf.ctypes.data), bits, 100, q, ss, ctypes.byref(h), None) == 1, (bits, q, ss)
        assert b"invalid argument" in L.nvbio_amd_last_error()
    assert build(0, ctypes.c_void_p(buf.ctypes.data), 2, 0xFFFFFFFF, 5, 2, ctypes.byref(h), None) == 1
    assert build(0, None, 2, 100, 5, 2, ctypes.byref(h), None) == 1
    assert build(0, ctypes.c_void_p(buf.ctypes.data), 2, 100, 5, 2, None, None) == 1
    assert L.nvbio_qgroup_set_index_build(0, None, 5, 2, 1, ctypes.byref(h), None) == 1
    assert L.nvbio_qgroup_index_get_view(None, None) == 1 and L.nvbio_qgroup_index_export(None, None, None, None, None, None) == 1


def test_no_device_no_build():
    import torch
    amd = ge.load_package()
    L = amd.lib()
    if torch.cuda.is_available():
        return                                                   # tests/test_gpu_qgroup.py covers the build on a GPU
    buf = np.zeros(64, np.uint32)
    h = ctypes.c_void_p()
    st = L.nvbio_qgroup_index_build(0, ctypes.c_void_p(buf.ctypes.data), 2, 100, 5, 2, ctypes.byref(h), None)
    assert st == 5, st                                           # NVBIO_ERR_NO_DEVICE: no CPU fallback
    assert not h.value
