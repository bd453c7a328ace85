"""BAM output used from C++ (tests/cpp/test_bam_format.cpp over nvbio_amd/bam.hpp, built by the library's Makefile as lib/bam_format_amd):
the program makes a complete BAM file of the 257-record fixture of tests/test_gpu_sam.py, whose arrays this test writes to a temp dir
(tests/test_gpu_sam_cpp.py::write_arrays), through BamFormatter; its stdout inflates to the header plus the restatement's records."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import bam_cpu
import sam_cpu
from test_gpu_sam_cpp import write_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "nvbio-gpl_amd", "lib", "bam_format_amd")


@pytest.mark.gpu
def test_bam_formatter_writes_a_complete_file(tmp_path):
    refs = sam_cpu.random_refs()
    rec = sam_cpu.random_records(np.random.default_rng(20240611), 257, refs)
    write_arrays(str(tmp_path), refs, rec)
    want_data, _, want_skipped = bam_cpu.bam_records(refs, rec)
    header = bam_cpu.bam_header(refs["names"], np.diff(refs["sequence_index"].astype(np.int64)))
    out = subprocess.run([EXE, str(tmp_path)], capture_output=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.endswith(bam_cpu.BGZF_EOF)
    assert gzip.decompress(out.stdout) == header + want_data
    assert out.stdout == bam_cpu.bgzf_frame(header) + bam_cpu.bgzf_frame(want_data) + bam_cpu.BGZF_EOF      # the header in blocks of its own
    assert out.stderr.decode().strip() == "bam ok: 257 records, %d bytes, %d skipped" % (len(want_data), want_skipped)
