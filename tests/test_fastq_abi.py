"""CPU-only: the FASTQ entry points are declared in include/nvbio_amd.h and exported by the library, the Python mirror has its classes and
functions, the struct mirrors have the header's size, and the queries that need no device answer."""
import ctypes
import importlib

import __graft_entry__ as ge


def test_fastq_symbols_are_declared_and_exported():
    amd = ge.load_package()
    header = amd.abi.Header(amd.HEADER_PATH)
    for name in ("nvbio_fastq_temp_bytes", "nvbio_fastq_scan", "nvbio_fastq_encode"):
        assert name in header.prototypes and hasattr(amd.lib(), name), name
    assert [f for f, _ in header.structs["nvbio_fastq_params"]] == ["quality_encoding", "strand_op", "truncate_len", "max_records"]
    assert tuple(f for f, _ in header.structs["nvbio_fastq_summary"]) == amd.FASTQ_SUMMARY_FIELDS
    assert ctypes.sizeof(amd._FastqParams) == 16 and ctypes.sizeof(amd._FastqSummary) == 40
    assert len(header.prototypes["nvbio_fastq_scan"][1]) == 8 and len(header.prototypes["nvbio_fastq_encode"][1]) == 15


def test_python_mirror_has_the_functions():
    amd = ge.load_package()
    pipeline = importlib.import_module("nvbio_gpl_amd.pipeline")
    for name in ("parse_fastq", "read_fastq", "FastqBatch", "fastq_scan", "fastq_encode", "fastq_summary"):
        assert hasattr(amd, name), name
    assert hasattr(pipeline, "fastq_to_sam")
    assert (amd.FASTQ_PHRED, amd.FASTQ_PHRED33, amd.FASTQ_PHRED64, amd.FASTQ_SOLEXA) == (0, 1, 2, 3)
    assert (amd.FASTQ_NO_OP, amd.FASTQ_REVERSE_OP, amd.FASTQ_COMPLEMENT_OP, amd.FASTQ_REVERSE_COMPLEMENT_OP) == (0, 1, 2, 3)


def test_a_text_of_4_gib_is_refused_without_a_device():
    """the refusal comes before anything that needs a device (the size itself is the rocPRIM scan's and is asked on the GPU: tests/test_gpu_fastq.py)"""
    amd = ge.load_package()
    L = amd.lib()
    b = ctypes.c_uint64(0)
    assert L.nvbio_fastq_temp_bytes(1 << 32, 1, ctypes.byref(b)) == 4 and b"4 GiB" in L.nvbio_amd_last_error()
    assert L.nvbio_fastq_temp_bytes(1 << 40, 0xFFFFFFFF, ctypes.byref(b)) == 4
    assert L.nvbio_fastq_temp_bytes(16, 1, None) == 1
