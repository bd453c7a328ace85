"""FASTA input used from C++ (tests/cpp/test_fasta_parse.cpp over nvbio_amd/fasta.hpp, built by the library's Makefile as lib/fasta_parse_amd):
the program reads files through FastaFile at several chunk sizes; what it prints is the same each time and is the restatement's reference
(tests/fasta_cpu.py), and input that ends inside a header line is reported."""
import os
import subprocess

import numpy as np
import pytest

import fasta_cpu as fa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "nvbio-gpl_amd", "lib", "fasta_parse_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_the_program_is_built_and_names_its_usage():
    assert os.path.exists(EXE), "lib/fasta_parse_amd is missing: __graft_entry__.build() makes it"
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "usage" in out.stderr


def printed(r):
    """the program's output for a restatement Reference"""
    lines = [b"total\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (r.length, r.n_seqs, r.n_holes, *[int(v) for v in r.freq], r.max_name_len)]
    for i, name in enumerate(r.name_list()):
        lines.append(b"seq\t%s\t%d\t%d\t%d\n" % (name.hex().encode(), r.seq_offset[i], r.seq_offset[i + 1] - r.seq_offset[i], r.seq_n_ambs[i]))
    lines += [b"hole\t%d\t%d\t%d\n" % (o, l, a) for o, l, a in zip(r.hole_offset, r.hole_len, r.hole_amb)]
    h = 0xcbf29ce484222325
    for b in r.text2.astype("<u4").tobytes():
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    lines.append(b"text2\t%016x\n" % h)
    return b"".join(lines)


@pytest.mark.gpu
def test_fasta_file_equals_the_restatement_at_every_chunk_size(tmp_path):
    rng = np.random.default_rng(21)
    known = open(os.path.join(GOLDEN, "fasta_known.fa"), "rb").read()
    letters = np.frombuffer(b"ACGTN", dtype=np.uint8)
    body = letters[rng.choice(5, 9000, p=[0.24, 0.24, 0.24, 0.24, 0.04])].tobytes()
    second = b">extra one\n" + b"\n".join(body[i:i + 70] for i in range(0, len(body), 70)) + b"\n"
    a, b = tmp_path / "a.fa", tmp_path / "b.fa"
    a.write_bytes(known + b"\n")
    b.write_bytes(second)
    want = printed(fa.parse(known + b"\n" + second))
    for chunk in (1000, 4096, 1 << 20):
        out = subprocess.run([EXE, str(chunk), str(a), str(b)], capture_output=True, timeout=120)
        assert out.returncode == 0, (chunk, out.stderr)
        assert out.stdout == want, chunk
    out = subprocess.run([EXE, "1000", os.path.join(GOLDEN, "fasta_cut.fa")], capture_output=True, timeout=120)
    assert out.returncode == 3 and b"inside a header line" in out.stderr
