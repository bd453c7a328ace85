"""The C++ host loop of the all-mapping mode used from C++ (tests/cpp/test_all_mapping.cpp over nvbio_amd/all_mapping.hpp): it builds
against the headers, and on a GPU gives the records, CIGARs and edit distances of the oracle's restatement -- in several chunks, with the
per-chunk callback seeing every record exactly once."""
import os
import subprocess

import numpy as np
import pytest

import oracle
from all_mapping_cpu import all_mapping_cpu, shared_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(out):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "nvbio-gpl_amd", "host"), "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "test_all_mapping.cpp"),
                           "-L" + os.path.join(ROOT, "nvbio-gpl_amd", "lib"), "-lnvbio_amd", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "nvbio-gpl_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib", "-o", out])


def test_all_mapping_program_compiles(tmp_path):
    _build(str(tmp_path / "test_all_mapping"))


@pytest.mark.gpu
def test_all_mapping_program_equals_the_restatement(orc, tmp_path):
    exe = str(tmp_path / "test_all_mapping")
    _build(exe)
    text, reads, _ = shared_input()
    R, M = reads.shape
    hidx = orc.build_index(text)
    want, det = all_mapping_cpu(orc, hidx, text, len(text), reads, oracle.SEMI_GLOBAL, 15, want_cigars=True)
    text.tofile(str(tmp_path / "text.u8")); np.ascontiguousarray(reads[:, ::-1]).tofile(str(tmp_path / "stored.u8"))
    hits_per_batch = 1031                                            # about a seventh of the hits, not a divisor
    out = subprocess.run([exe, str(tmp_path), str(R), str(M), str(oracle.SEMI_GLOBAL), "15", str(hits_per_batch), "0", "0", "20000"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all mapping ok" in out.stdout
    ld = lambda name, dt: np.fromfile(str(tmp_path / name), dt)
    n_hits, n_scored, n_aln, chunks = (int(v) for v in ld("stats.u64", np.uint64))
    rec = ld("records.u32", np.uint32).reshape(-1, 4).astype(np.int64)
    rec[:, 3] = np.where(rec[:, 3] >= 1 << 31, rec[:, 3] - (1 << 32), rec[:, 3])          # scores are int32
    dt = ld("details.u32", np.uint32).reshape(-1, 5).astype(np.int64)
    cig = ld("cigars.u16", np.uint16).reshape(-1, 64); lens = ld("cigar_lens.u32", np.uint32)
    assert n_aln == len(want) == len(rec) and n_scored == n_hits and chunks == -(-n_hits // hits_per_batch) and chunks >= 5
    assert (np.diff(rec[:, 0]) >= 0).all()
    go = sorted(range(len(rec)), key=lambda k: (tuple(rec[k]), int(dt[k, 0])))
    wo = sorted(range(len(want)), key=lambda k: (tuple(want[k]), det[k][0][0]))
    for g, w in zip(go, wo):
        src, snk, ed, wc = det[w]
        assert tuple(rec[g]) == tuple(want[w]) and tuple(dt[g]) == src + snk + (ed,), (g, w)
        assert lens[g] == len(wc) and np.array_equal(cig[g, :lens[g]], wc), (g, w)
    # the callback saw every record exactly once, chunk by chunk, in order
    cb = ld("cb_records.u32", np.uint32).reshape(-1, 5).astype(np.int64)
    first = ld("cb_first.u64", np.uint64).reshape(-1, 2).astype(np.int64)
    assert np.array_equal(first[:, 0], np.concatenate([[0], np.cumsum(first[:, 1])[:-1]])) and int(first[:, 1].sum()) == n_aln
    assert np.array_equal(cb[:, :3], rec[:, :3]) and np.array_equal(cb[:, 3].astype(np.uint32), rec[:, 3].astype(np.uint32)) and np.array_equal(cb[:, 4], dt[:, 4])
