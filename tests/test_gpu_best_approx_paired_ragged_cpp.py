"""The C++ host loop of the ragged PAIRED best-approx mode used from C++ (tests/cpp/test_best_approx_paired_ragged.cpp over nvbio_amd/best_approx.hpp): it
builds against the headers, and on a GPU gives the arrays and counters of the restatement in `tight` mode with several hits per read, and refuses a
batch with a 1024-symbol mate with exit status 3, without touching the result arrays."""
import os
import subprocess

import numpy as np
import pytest

import oracle
from best_approx_paired_ragged_cpu import N_PAIRS, restatement, shared_input, stored_stream, tables_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(out):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "nvbio-gpl_amd", "host"), "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "test_best_approx_paired_ragged.cpp"),
                           "-L" + os.path.join(ROOT, "nvbio-gpl_amd", "lib"), "-lnvbio_amd", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "nvbio-gpl_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib", "-o", out])


def _write(tmp_path, text, mates, min_scores):
    text.tofile(str(tmp_path / "text.u8"))
    for m in (0, 1):
        syms, off = stored_stream(mates[m])
        syms.tofile(str(tmp_path / ("stored%d.u8" % (m + 1)))); off.tofile(str(tmp_path / ("offsets%d.u32" % (m + 1))))
        np.asarray(min_scores[m], dtype=np.int32).tofile(str(tmp_path / ("min_scores%d.i32" % (m + 1))))


def test_best_approx_paired_ragged_program_compiles(tmp_path):
    _build(str(tmp_path / "test_best_approx_paired_ragged"))


@pytest.mark.gpu
def test_best_approx_paired_ragged_program_equals_the_restatement(orc, tmp_path):
    exe = str(tmp_path / "test_best_approx_paired_ragged")
    _build(exe)
    text, _, m1, m2 = shared_input(orc, False)
    R, bs = N_PAIRS, 3 * N_PAIRS
    _write(tmp_path, text, (m1, m2), tables_of(m1, m2)[1])
    out = subprocess.run([exe, str(tmp_path), str(R), str(oracle.SEMI_GLOBAL), str(bs), "1", "1"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "best approx paired ragged ok" in out.stdout
    want = restatement(orc, "tight", bs, True)
    for k in ("best_a", "best_o"):
        g = np.fromfile(str(tmp_path / (k + ".i32")), np.int32).reshape(R, 2, 4).astype(np.int64)
        w = want[k]
        assert np.array_equal(g[..., 0], w[..., 0]) and np.array_equal(g[..., 1] & 0xFFFFFFFF, w[..., 1]) and np.array_equal(g[..., 2] & 0xFFFFFFFF, w[..., 2]), k
        assert np.array_equal(g[..., 3], w[..., 3] | (w[..., 4] << 1) | (w[..., 5] << 2)), k
    n_ext, n_opp, passes, multi = (int(v) for v in np.fromfile(str(tmp_path / "stats.u64"), np.uint64))
    assert (n_ext, n_opp, passes, multi) == (want["n_extensions"], want["n_opposite"], want["passes"], want["multi_passes"]) and multi > 0
    # a mate of 1024 symbols: refused, nothing written
    a = [text[1000 * (k + 1):1000 * (k + 1) + M].copy() for k, M in enumerate((100, 110, 120))]
    b = [text[1300 * (k + 1):1300 * (k + 1) + M].copy() for k, M in enumerate((100, 1024, 120))]
    _write(tmp_path, text, (a, b), (np.full(3, -60), np.full(3, -60)))
    out = subprocess.run([exe, str(tmp_path), "3", str(oracle.SEMI_GLOBAL), "0", "1", "0"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 3 and "refused" in out.stdout and "1024" in out.stdout, out.stdout + out.stderr
    assert (np.fromfile(str(tmp_path / "best_a.i32"), np.int32) == 0x5A5A5A5A).all() and (np.fromfile(str(tmp_path / "best_o.i32"), np.int32) == 0x5A5A5A5A).all()
