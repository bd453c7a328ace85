"""CPU-only: the FASTA entry points are declared in include/nvbio_amd.h and exported by the library, the Python mirror has its classes and
functions, the struct mirrors have the header's fields, sizes and offsets, and the queries that need no device answer."""
import ctypes
import importlib

import __graft_entry__ as ge

FUNCTIONS = {"nvbio_fasta_state_init": 4, "nvbio_fasta_temp_bytes": 2, "nvbio_fasta_scan": 8, "nvbio_fasta_encode": 19, "nvbio_fasta_finish": 11}


def test_fasta_symbols_are_declared_and_exported():
    amd = ge.load_package()
    header = amd.abi.Header(amd.HEADER_PATH)
    for name, n_args in FUNCTIONS.items():
        assert name in header.prototypes and hasattr(amd.lib(), name), name
        assert len(header.prototypes[name][1]) == n_args, name
    for c_name, mirror, size in (("nvbio_fasta_state", amd._FastaState, 64), ("nvbio_fasta_summary", amd._FastaSummary, 32)):
        fields = header.structs[c_name]
        assert [f for f, _ in fields] == [f for f, _ in mirror._fields_], c_name
        assert ctypes.sizeof(mirror) == size == sum(ctypes.sizeof(t) for _, t in fields), c_name
        at = 0
        for f, t in fields:
            assert getattr(mirror, f).offset == at and getattr(mirror, f).size == ctypes.sizeof(t), (c_name, f)
            at += ctypes.sizeof(t)
    assert tuple(f for f, _ in header.structs["nvbio_fasta_summary"]) == amd.FASTA_SUMMARY_FIELDS
    assert tuple(f for f, _ in header.structs["nvbio_fasta_state"])[:8] == amd.FASTA_STATE_FIELDS
    assert amd._MIRRORS["nvbio_fasta_state"] is amd._FastaState and amd._MIRRORS["nvbio_fasta_summary"] is amd._FastaSummary


def test_python_mirror_has_the_functions():
    amd = ge.load_package()
    pipeline = importlib.import_module("nvbio_gpl_amd.pipeline")
    for name in ("parse_fasta", "read_fasta", "FastaReference", "fasta_state_init", "fasta_scan", "fasta_encode", "fasta_finish", "fasta_summary", "fasta_state"):
        assert hasattr(amd, name), name
    assert hasattr(pipeline, "reference_from_fasta")
    for name in ("sam_refs", "build_index", "save", "names", "holes"):
        assert hasattr(amd.FastaReference, name), name
    assert (amd.FASTA_PRE, amd.FASTA_ID, amd.FASTA_REST, amd.FASTA_BODY, amd.FASTA_END) == (0, 1, 2, 3, 4)
    assert (amd.FASTA_STATUS_INCOMPLETE, amd.FASTA_STATUS_END_BYTE, amd.FASTA_STATUS_OVERFLOW_32, amd.FASTA_STATUS_CAPACITY) == (1, 2, 4, 8)


def test_the_header_states_the_constants_the_mirror_uses():
    amd = ge.load_package()
    text = open(amd.HEADER_PATH).read()
    for name, value in (("NVBIO_FASTA_PRE", 0), ("NVBIO_FASTA_ID", 1), ("NVBIO_FASTA_REST", 2), ("NVBIO_FASTA_BODY", 3), ("NVBIO_FASTA_END", 4),
                        ("NVBIO_FASTA_STATUS_INCOMPLETE", 1), ("NVBIO_FASTA_STATUS_END_BYTE", 2), ("NVBIO_FASTA_STATUS_OVERFLOW_32", 4),
                        ("NVBIO_FASTA_STATUS_CAPACITY", 8)):
        assert any(line.split()[:2] == ["#define", name] and line.split()[2] == "%du" % value for line in text.split("\n")), name


def test_a_text_of_4_gib_is_refused_without_a_device():
    amd = ge.load_package()
    L = amd.lib()
    b = ctypes.c_uint64(0)
    assert L.nvbio_fasta_temp_bytes(1 << 32, ctypes.byref(b)) == 4 and b"4 GiB" in L.nvbio_amd_last_error()
    assert L.nvbio_fasta_temp_bytes(16, None) == 1
    assert L.nvbio_fasta_temp_bytes(1 << 30, ctypes.byref(b)) == 0 and 36 * (1 << 18) <= b.value < 37 * (1 << 18) + 4096
