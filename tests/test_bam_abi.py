"""CPU-only: the BAM and BGZF entry points are declared in include/nvbio_amd.h and exported by the library, the Python mirror has its
functions and constants, bam_header and write_bam give the bytes the format asks for, every refusal the header lists happens before the
device is looked for, and without a GPU the calls fail loudly with NVBIO_ERR_NO_DEVICE."""
import ctypes
import gzip
import io
import os
import struct
import subprocess

import numpy as np

import __graft_entry__ as ge

SYMBOLS = ("nvbio_bam_format_temp_bytes", "nvbio_bam_record_offsets", "nvbio_bam_format", "nvbio_bgzf_framed_bytes", "nvbio_bgzf_frame")


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
    src = open(amd.HEADER_PATH).read()
    assert all(s in src for s in ("NVBIO_BAM_LENGTHS_ONLY 1u", "NVBIO_BAM_REG2BIN      2u", "NVBIO_BAM_STATUS_CAPACITY 1u", "NVBIO_BAM_STATUS_OFFSETS  2u",
                                  "NVBIO_BAM_STATUS_TOO_LONG 4u", "NVBIO_BGZF_BLOCK_BYTES 65280u", "NVBIO_BGZF_OVERHEAD    31u", "output_bam.cpp:227-544",
                                  "output_gzip.cpp:29-42,118-134"))
    assert L.nvbio_amd_version() == 100


def test_python_mirror_has_the_functions_and_constants():
    from importlib import import_module
    amd = ge.load_package()
    pipeline = import_module("nvbio_gpl_amd.pipeline")
    for name in ("bam_records", "bam_record_offsets", "bam_format", "bgzf_frame", "bgzf_framed_bytes"):
        assert callable(getattr(amd, name))
    for name in ("bam_header", "write_bam", "align_to_bam", "fastq_to_bam", "align_to_sam", "fastq_to_sam"):
        assert callable(getattr(pipeline, name))
    assert (amd.BAM_STATUS_CAPACITY, amd.BAM_STATUS_OFFSETS, amd.BAM_STATUS_TOO_LONG) == (1, 2, 4)
    assert (amd.BAM_LENGTHS_ONLY, amd.BAM_REG2BIN, amd.BGZF_BLOCK_BYTES, amd.BGZF_OVERHEAD) == (1, 2, 65280, 31)
    assert amd.BGZF_EOF == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000") and gzip.decompress(amd.BGZF_EOF) == b""
    for n, want in ((0, 0), (1, 32), (65280, 65311), (65281, 65343), (5 * 65280 + 33, 5 * 65280 + 33 + 6 * 31)):
        assert amd.bgzf_framed_bytes(n) == want


def test_bam_header_bytes_for_two_sequences():
    from importlib import import_module
    ge.load_package()
    pipeline = import_module("nvbio_gpl_amd.pipeline")
    text = b"@HD\tVN:1.3\n@PG\tID:nvBowtie\tPN:nvBowtie\tVN:0.5.1\n"
    want = (b"BAM\x01" + struct.pack("<I", len(text)) + text + struct.pack("<I", 2) + struct.pack("<I", 5) + b"chr1\0" + struct.pack("<I", 1000) +
            struct.pack("<I", 5) + b"chrB\0" + struct.pack("<I", 500))
    assert pipeline.bam_header(["chr1", b"chrB"], [1000, 500]) == want
    full = pipeline.sam_header(["chr1", b"chrB"], [1000, 500])
    got = pipeline.bam_header(["chr1", b"chrB"], [1000, 500], text=full)
    assert got[:8] == b"BAM\x01" + struct.pack("<I", len(full)) and got[8:8 + len(full)] == full and got[8 + len(full):] == want[8 + len(text):]
    assert pipeline.bam_header([], []) == b"BAM\x01" + struct.pack("<I", len(text)) + text + struct.pack("<I", 0)


def test_write_bam_from_bytes_inflates_to_header_and_data():
    from importlib import import_module
    amd = ge.load_package()
    pipeline = import_module("nvbio_gpl_amd.pipeline")
    header = pipeline.bam_header(["chr1"], [1000])
    data = np.random.default_rng(5).integers(0, 256, 65280 + 100, dtype=np.uint8).tobytes()
    f = io.BytesIO()
    pipeline.write_bam(f, header, data)
    got = f.getvalue()
    assert gzip.decompress(got) == header + data and got.endswith(amd.BGZF_EOF)
    assert len(got) == len(header) + 31 + len(data) + 2 * 31 + 28       # the header is a block sequence of its own
    assert struct.unpack_from("<H", got, 16)[0] == len(header) + 30


def test_arguments_are_checked_before_the_device():
    amd = ge.load_package()
    L = amd.lib()
    buf = np.zeros(64, np.uint64)
    out = ctypes.c_void_p(buf.ctypes.data)
    nb = ctypes.c_uint64(0)
    assert L.nvbio_bam_format_temp_bytes(4, None) == 1 and L.nvbio_bam_format_temp_bytes(0x7FFFFFFF, ctypes.byref(nb)) == 1
    assert L.nvbio_bam_format_temp_bytes(4, ctypes.byref(nb)) == 0 and nb.value >= 16      # a host formula: known without a device
    refs, rec = _structs(amd, buf)
    offsets = lambda r, c, flags=0, o=out, t=out, tb=1 << 20: L.nvbio_bam_record_offsets(0, r, c, flags, o, t, tb, None)
    fmt = lambda r, c, flags=0, o=out, data=out, cap=64, sk=out, st=out: L.nvbio_bam_format(0, r, c, flags, o, data, cap, sk, st, None)
    R, C = ctypes.byref(refs), ctypes.byref(rec)
    assert offsets(None, C) == 1 and offsets(R, None) == 1 and fmt(None, C) == 1 and fmt(R, None) == 1
    assert offsets(R, C, flags=4) == 1 and b"unknown flags" in L.nvbio_amd_last_error()
    assert fmt(R, C, flags=1) == 1 and b"unknown flags" in L.nvbio_amd_last_error()                # LENGTHS_ONLY is the offsets call's alone
    assert fmt(R, C, flags=4) == 1
    assert offsets(R, C, o=None) == 1 and offsets(R, C, t=None) == 1
    assert offsets(R, C, tb=8) == 1 and b"temp_bytes too small" in L.nvbio_amd_last_error()
    assert fmt(R, C, o=None) == 1 and fmt(R, C, data=None) == 1 and fmt(R, C, sk=None) == 1 and fmt(R, C, st=None) == 1
    assert fmt(R, C, data=ctypes.c_void_p(buf.ctypes.data + 8)) == 1 and b"16-byte aligned" in L.nvbio_amd_last_error()
    for field in ("names_dev", "name_index_dev", "reads4_dev", "read_index_dev", "state_dev", "pos_dev", "score_dev", "ed_dev", "mapq_dev", "cigars_dev",
                  "cigar_lens_dev", "mds_lens_dev", "refs_sequence_index_dev", "refs_names_dev", "refs_names_index_dev"):
        r, c = _structs(amd, buf, **{field: None})
        assert offsets(ctypes.byref(r), ctypes.byref(c)) == 1 and fmt(ctypes.byref(r), ctypes.byref(c)) == 1, field
        assert b"invalid argument" in L.nvbio_amd_last_error()
    for kw in (dict(max_read_len=1024), dict(mds_stride=1), dict(refs_n_seqs=0), dict(n=0x7FFFFFFF)):
        r, c = _structs(amd, buf, **kw)
        assert offsets(ctypes.byref(r), ctypes.byref(c)) == 1 and fmt(ctypes.byref(r), ctypes.byref(c)) == 1, kw

    # the framing call
    fb = ctypes.c_uint64(0)
    assert L.nvbio_bgzf_framed_bytes(10, None) == 1
    assert L.nvbio_bgzf_framed_bytes(65281, ctypes.byref(fb)) == 0 and fb.value == 65281 + 62
    frame = lambda d=out, n=100, o=out, cap=131: L.nvbio_bgzf_frame(0, d, n, o, cap, None)
    assert frame(cap=130) == 1 and b"out_capacity" in L.nvbio_amd_last_error()                      # one byte short
    assert frame(d=None) == 1 and frame(o=None) == 1
    assert frame(d=ctypes.c_void_p(buf.ctypes.data + 8)) == 1 and b"16-byte aligned" in L.nvbio_amd_last_error()
    assert frame(o=ctypes.c_void_p(buf.ctypes.data + 4)) == 1 and b"16-byte aligned" in L.nvbio_amd_last_error()


def test_record_bounds_that_do_not_fit_are_unsupported():
    """before any launch, so also without a device: l_read_name is one byte, n_cigar_op 16 bits, a group's LDS holds 16384 bytes"""
    amd = ge.load_package()
    L = amd.lib()
    buf = np.zeros(64, np.uint64)
    out = ctypes.c_void_p(buf.ctypes.data)
    both = lambda r, c: (L.nvbio_bam_record_offsets(0, ctypes.byref(r), ctypes.byref(c), 0, out, out, 1 << 20, None),
                         L.nvbio_bam_format(0, ctypes.byref(r), ctypes.byref(c), 0, out, out, 64, out, out, None))
    r, c = _structs(amd, buf, max_name_len=255)
    assert both(r, c) == (4, 4) and b"l_read_name" in L.nvbio_amd_last_error()
    r, c = _structs(amd, buf, cigar_stride=65536)
    assert both(r, c) == (4, 4) and b"n_cigar_op" in L.nvbio_amd_last_error()
    for kw in (dict(cigar_stride=4096), dict(mds_stride=8192)):
        r, c = _structs(amd, buf, **kw)
        assert both(r, c) == (4, 4), kw
        msg = L.nvbio_amd_last_error()
        assert b"LDS" in msg and b"16384" in msg
    # the largest cigar_stride that fits: 40 + 4 x 3955 + 150 + 75 + (2 x 64 + 16) + 72 = 16301 bytes of record, + 16 + 64 = 16381 <= 16384;
    # one element more gives 16385
    import torch
    if not torch.cuda.is_available():                                # (with a device the call would go on to launch over these host pointers)
        r, c = _structs(amd, buf, cigar_stride=3955)
        assert both(r, c) == (5, 5)
    r, c = _structs(amd, buf, cigar_stride=3956)
    assert both(r, c) == (4, 4)


def test_no_device_no_bytes():
    import torch
    if torch.cuda.is_available():
        return                                                       # tests/test_gpu_bam.py covers the calls on a GPU
    amd = ge.load_package()
    L = amd.lib()
    buf = np.zeros(64, np.uint64)
    out = ctypes.c_void_p(buf.ctypes.data)
    refs, rec = _structs(amd, buf)
    assert L.nvbio_bam_record_offsets(0, ctypes.byref(refs), ctypes.byref(rec), 0, out, out, 1 << 20, None) == 5      # NVBIO_ERR_NO_DEVICE: no CPU fallback
    assert L.nvbio_bam_format(0, ctypes.byref(refs), ctypes.byref(rec), 0, out, out, 64, out, out, None) == 5
    assert L.nvbio_bgzf_frame(0, out, 100, out, 131, None) == 5


def test_the_cpp_program_exists_and_prints_usage():
    path = os.path.join(ge.PKG_DIR, "lib", "bam_format_amd")
    assert os.path.exists(path), "lib/bam_format_amd is missing: build()"
    p = subprocess.run([path], capture_output=True)
    assert p.returncode == 2 and b"usage" in p.stderr
