"""FASTQ input used from C++ (tests/cpp/test_fastq_parse.cpp over nvbio_amd/fastq.hpp, built by the library's Makefile as lib/fastq_parse_amd):
the program reads the known file through FastqFile at chunk sizes 64, 1000 and the whole file; what it prints is the same each time and
is the restatement's batch (tests/fastq_cpu.py), and the file's unfinished last record is reported as the reference's "incomplete read"."""
import os
import subprocess

import numpy as np
import pytest

import fastq_cpu as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "nvbio-gpl_amd", "lib", "fastq_parse_amd")
KNOWN = os.path.join(ROOT, "tests", "golden", "fastq_known.fq")


def test_the_program_is_built_and_names_its_usage():
    assert os.path.exists(EXE), "lib/fastq_parse_amd is missing: __graft_entry__.build() makes it"
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "usage" in out.stderr


def printed(batch):
    """the program's output for a restatement Batch"""
    lines = []
    for i in range(batch.n):
        lines.append(b"%s\t%s\t%s\n" % (batch.name(i).hex().encode(), bytes(b"ACGTN-"[s] for s in batch.symbols(i)), batch.qualities(i).tobytes().hex().encode()))
    return b"".join(lines)


@pytest.mark.gpu
def test_fastq_file_equals_the_restatement_at_every_chunk_size(tmp_path):
    text = open(KNOWN, "rb").read()
    want = printed(fc.parse(text))
    for chunk in (64, 1000, len(text)):
        out = subprocess.run([EXE, KNOWN, str(chunk)], capture_output=True, timeout=120)
        assert out.returncode == 3 and b"incomplete read" in out.stderr and b"after 19 reads" in out.stderr, (chunk, out.stderr)
        assert out.stdout == want, chunk
    whole = tmp_path / "whole.fq"                                     # the same file with its last record ended, stored reversed as nvBowtie loads it
    whole.write_bytes(text + b"\n")
    want = printed(fc.parse(text + b"\n", fc.PHRED64, fc.REVERSE_OP))
    for chunk, batch in ((64, 1), (1000, 7), (1 << 20, 1000)):
        out = subprocess.run([EXE, str(whole), str(chunk), str(batch), "1", "2"], capture_output=True, timeout=120)
        assert out.returncode == 0 and out.stderr.startswith(b"fastq ok: 20 reads"), (chunk, out.stderr)
        assert out.stdout == want, chunk
