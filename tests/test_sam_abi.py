"""CPU-only: the SAM entry points are declared in include/nvbio_amd.h and exported by the library, the Python mirror has its
functions, invalid arguments and a record bound beyond the LDS budget are named before the device is looked for, and without a GPU the
calls fail loudly with NVBIO_ERR_NO_DEVICE."""
import ctypes
import io

import numpy as np

import __graft_entry__ as ge

SYMBOLS = ("nvbio_sam_format_temp_bytes", "nvbio_sam_record_offsets", "nvbio_sam_format")


def _structs(amd, buf, n=4, **kw):
    p = buf.ctypes.data
    refs = amd._SamRefs(2, 4, p, p, p)
    rec = amd._SamRecords(n, 40, 150, 1, p, p, p, p, None, p, p, p, None, p, p, p, p, p, p, None, 32, 64)
    for k, v in kw.items():
        setattr(refs if k.startswith("refs_") else rec, k[5:] if k.startswith("refs_") else k, v)
    return refs, rec


def test_symbols_are_declared_and_exported():
    amd = ge.load_package()
    header = amd.abi.Header(amd.HEADER_PATH)
    L = amd.lib()
    for name in SYMBOLS:
        assert name in header.prototypes, name + " is not declared"
        assert hasattr(L, name), name + " is not exported"
    assert "nvbio_sam_refs" in header.structs and "nvbio_sam_records" in header.structs
    src = open(amd.HEADER_PATH).read()
    assert all(s in src for s in ("NVBIO_SAM_STATUS_CAPACITY", "NVBIO_SAM_STATUS_OFFSETS", "NVBIO_SAM_STATUS_TOO_LONG", "output_sam.cpp:182-544"))
    assert ctypes.sizeof(amd._SamRefs) == 32 and ctypes.sizeof(amd._SamRecords) == 16 + 16 * 8 + 8


def test_python_mirror_has_the_functions():
    from importlib import import_module
    amd = ge.load_package()
    pipeline = import_module("nvbio_gpl_amd.pipeline")
    for name in ("sam_records", "sam_record_offsets", "sam_format", "SamRefs", "SamRecords"):
        assert callable(getattr(amd, name))
    for name in ("sam_header", "write_sam", "align_to_sam"):
        assert callable(getattr(pipeline, name))
    assert (amd.SAM_STATUS_CAPACITY, amd.SAM_STATUS_OFFSETS, amd.SAM_STATUS_TOO_LONG) == (1, 2, 4)
    header = pipeline.sam_header(["chr1", b"chrB"], [1000, 500])
    assert header == b"@HD\tVN:1.3\n@PG\tID:nvBowtie\tPN:nvBowtie\tVN:0.5.1\n@SQ\tSN:chr1\tLN:1000\n@SQ\tSN:chrB\tLN:500\n"
    assert pipeline.sam_header([], [], pg_id="x", pg_name="y", pg_version="1") == b"@HD\tVN:1.3\n@PG\tID:x\tPN:y\tVN:1\n"
    f = io.BytesIO()
    pipeline.write_sam(f, header, b"r0\t4\n")
    assert f.getvalue() == header + b"r0\t4\n"


def test_arguments_are_checked_before_the_device():
    amd = ge.load_package()
    L = amd.lib()
    buf = np.zeros(64, np.uint64)
    out = ctypes.c_void_p(buf.ctypes.data)
    nb = ctypes.c_uint64(0)
    assert L.nvbio_sam_format_temp_bytes(4, None) == 1 and L.nvbio_sam_format_temp_bytes(0x7FFFFFFF, ctypes.byref(nb)) == 1
    refs, rec = _structs(amd, buf)
    offsets = lambda r, c, flags=0, o=out, t=out, tb=1 << 20: L.nvbio_sam_record_offsets(0, r, c, flags, o, t, tb, None)
    fmt = lambda r, c, flags=0, o=out, text=out, cap=64, sk=out, st=out: L.nvbio_sam_format(0, r, c, flags, o, text, cap, sk, st, None)
    R, C = ctypes.byref(refs), ctypes.byref(rec)
    assert offsets(None, C) == 1 and offsets(R, None) == 1 and fmt(None, C) == 1 and fmt(R, None) == 1
    assert offsets(R, C, flags=2) == 1 and fmt(R, C, flags=1) == 1                                    # unknown flags; LENGTHS_ONLY is the offsets call's alone
    assert offsets(R, C, o=None) == 1 and offsets(R, C, t=None) == 1
    import torch
    if torch.cuda.is_available():                                    # rocPRIM sizes the scan's temp for the device it runs on
        assert offsets(R, C, tb=8) == 1 and b"temp_bytes too small" in L.nvbio_amd_last_error()
    assert fmt(R, C, o=None) == 1 and fmt(R, C, text=None) == 1 and fmt(R, C, sk=None) == 1 and fmt(R, C, st=None) == 1
    assert fmt(R, C, text=ctypes.c_void_p(buf.ctypes.data + 8)) == 1 and b"16-byte aligned" in L.nvbio_amd_last_error()
    for field in ("names_dev", "name_index_dev", "reads4_dev", "read_index_dev", "state_dev", "pos_dev", "score_dev", "ed_dev", "mapq_dev", "cigars_dev",
                  "cigar_lens_dev", "mds_lens_dev", "refs_sequence_index_dev", "refs_names_dev", "refs_names_index_dev"):
        r, c = _structs(amd, buf, **{field: None})
        assert offsets(ctypes.byref(r), ctypes.byref(c)) == 1 and fmt(ctypes.byref(r), ctypes.byref(c)) == 1, field
        assert b"invalid argument" in L.nvbio_amd_last_error()
    for kw in (dict(max_read_len=1024), dict(mds_stride=1), dict(refs_n_seqs=0), dict(n=0x7FFFFFFF)):
        r, c = _structs(amd, buf, **kw)
        assert offsets(ctypes.byref(r), ctypes.byref(c)) == 1 and fmt(ctypes.byref(r), ctypes.byref(c)) == 1, kw


def test_a_record_bound_beyond_the_lds_budget_is_unsupported():
    """before any launch, so also without a device: a wave's LDS holds 16384 bytes"""
    amd = ge.load_package()
    L = amd.lib()
    buf = np.zeros(64, np.uint64)
    out = ctypes.c_void_p(buf.ctypes.data)
    for kw in (dict(cigar_stride=4096), dict(mds_stride=8192), dict(max_name_len=20000), dict(refs_max_name_len=9000)):
        r, c = _structs(amd, buf, **kw)
        assert L.nvbio_sam_record_offsets(0, ctypes.byref(r), ctypes.byref(c), 0, out, out, 1 << 20, None) == 4, kw
        msg = L.nvbio_amd_last_error()
        assert b"LDS" in msg and b"16384" in msg
        assert L.nvbio_sam_format(0, ctypes.byref(r), ctypes.byref(c), 0, out, out, 64, out, out, None) == 4, kw
    # the largest shape that fits: 40 + 2 x 4 + 2 x 1023 + 6 x 2048 + (2 x 64 + 16) + 192 = 14734 text bytes, + 16 + 64 <= 16384
    import torch
    if not torch.cuda.is_available():                                # (with a device the call would go on to launch over these host pointers)
        r, c = _structs(amd, buf, cigar_stride=2048, max_read_len=1023)
        assert L.nvbio_sam_record_offsets(0, ctypes.byref(r), ctypes.byref(c), 0, out, out, 1 << 20, None) == 5


def test_no_device_no_text():
    import torch
    if torch.cuda.is_available():
        return                                                       # tests/test_gpu_sam.py covers the calls on a GPU
    amd = ge.load_package()
    L = amd.lib()
    buf = np.zeros(64, np.uint64)
    out = ctypes.c_void_p(buf.ctypes.data)
    refs, rec = _structs(amd, buf)
    assert L.nvbio_sam_record_offsets(0, ctypes.byref(refs), ctypes.byref(rec), 0, out, out, 1 << 20, None) == 5      # NVBIO_ERR_NO_DEVICE: no CPU fallback
    assert L.nvbio_sam_format(0, ctypes.byref(refs), ctypes.byref(rec), 0, out, out, 64, out, out, None) == 5
