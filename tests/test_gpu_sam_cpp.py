"""SAM output used from C++ (tests/cpp/test_sam_format.cpp over nvbio_amd/sam.hpp, built by the library's Makefile as lib/sam_format_amd):
the program formats the 257-record fixture of tests/test_gpu_sam.py, whose arrays this test writes to a temp dir, through SamFormatter,
and its stdout is the header plus the restatement's text."""
import os
import subprocess

import numpy as np
import pytest

import sam_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "nvbio-gpl_amd", "lib", "sam_format_amd")


def test_the_program_is_built_and_names_its_usage():
    assert os.path.exists(EXE), "lib/sam_format_amd is missing: __graft_entry__.build() makes it"
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "usage" in out.stderr


def write_arrays(d, refs, rec):
    """one file per array of nvbio_sam_refs / nvbio_sam_records, and meta.u32"""
    names, ref_names = rec["names"], refs["names"]
    lens = np.diff(rec["read_index"].astype(np.int64))
    index = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.uint32)
    has = lambda k: 0 if rec.get(k) is None else 1
    files = {"meta.u32": np.array([len(names), len(ref_names), max(len(x) for x in names), max(len(x) for x in ref_names), int(lens.max()),
                                   1 if rec["reads_reversed"] else 0, rec["cigars"].shape[1], rec["mds"].shape[1] if has("mds") else 0, has("quals"),
                                   has("second_score"), has("mds"), has("mate_of")], np.uint32),
             "seq_index.u32": refs["sequence_index"].astype(np.uint32), "ref_names.u8": np.frombuffer(b"".join(ref_names), np.uint8),
             "ref_names_index.u32": index(ref_names), "names.u8": np.frombuffer(b"".join(names), np.uint8), "name_index.u32": index(names),
             "reads4.u32": sam_cpu.pack4(rec["reads"]), "read_index.u32": rec["read_index"].astype(np.uint32), "state.u8": rec["state"],
             "pos.u32": rec["pos"], "score.i32": rec["score"], "ed.u32": rec["ed"], "mapq.u8": rec["mapq"], "cigars.u16": rec["cigars"],
             "cigar_lens.u32": rec["cigar_lens"]}
    for key, name in (("quals", "quals.u8"), ("second_score", "second.i32"), ("mds", "mds.u8"), ("mds_lens", "mds_lens.u32"), ("mate_of", "mate_of.u32")):
        if has(key):
            files[name] = rec[key]
    for name, a in files.items():
        np.ascontiguousarray(a).tofile(os.path.join(d, name))


@pytest.mark.gpu
def test_sam_formatter_equals_the_restatement(tmp_path):
    refs = sam_cpu.random_refs()
    rec = sam_cpu.random_records(np.random.default_rng(20240611), 257, refs)
    write_arrays(str(tmp_path), refs, rec)
    want_text, _, want_skipped = sam_cpu.sam_records(refs, rec)
    header = sam_cpu.sam_header(refs["names"], np.diff(refs["sequence_index"].astype(np.int64)))
    out = subprocess.run([EXE, str(tmp_path)], capture_output=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout == header + want_text
    assert out.stderr.decode().strip() == "sam ok: 257 records, %d bytes, %d skipped" % (len(want_text), want_skipped)
