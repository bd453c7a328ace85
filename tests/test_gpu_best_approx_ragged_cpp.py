"""The C++ host loop of the ragged best-approx mode used from C++ (tests/cpp/test_best_approx_ragged.cpp over nvbio_amd/best_approx.hpp): it builds
against the headers, and on a GPU gives the arrays and counters of the restatement with the several-hits-per-read phase, and refuses a batch with a
1024-symbol read without touching the result arrays."""
import os
import subprocess

import numpy as np
import pytest

import oracle
from best_approx_ragged_cpu import references, shared_input, stored_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(out):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "nvbio-gpl_amd", "host"), "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "test_best_approx_ragged.cpp"),
                           "-L" + os.path.join(ROOT, "nvbio-gpl_amd", "lib"), "-lnvbio_amd", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "nvbio-gpl_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib", "-o", out])


def test_best_approx_ragged_program_compiles(tmp_path):
    _build(str(tmp_path / "test_best_approx_ragged"))


@pytest.mark.gpu
def test_best_approx_ragged_program_equals_the_restatement(orc, tmp_path):
    exe = str(tmp_path / "test_best_approx_ragged")
    _build(exe)
    text, reads = shared_input()
    ref = references(orc, "tight")
    R = len(reads)
    syms, off = stored_stream(reads)
    text.tofile(str(tmp_path / "text.u8")); syms.tofile(str(tmp_path / "stored.u8")); off.tofile(str(tmp_path / "offsets.u32"))
    ref["min_scores"].astype(np.int32).tofile(str(tmp_path / "min_scores.i32"))
    bs = 3 * R
    out = subprocess.run([exe, str(tmp_path), str(R), str(oracle.SEMI_GLOBAL), str(bs), "1", "1"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "best approx ragged ok" in out.stdout
    want = ref["multi"][bs]
    best = np.fromfile(str(tmp_path / "best.i32"), np.int32).reshape(R, 4).astype(np.int64)
    rc = np.fromfile(str(tmp_path / "best_rc.u8"), np.uint8)
    n_ext, passes, multi, seeding = (int(v) for v in np.fromfile(str(tmp_path / "stats.u64"), np.uint64))
    loc = lambda c: np.where(best[:, c] == -1, -1, best[:, c] & 0xFFFFFFFF)
    assert np.array_equal(best[:, 0], want["best_score"]) and np.array_equal(best[:, 2], want["second_score"])
    assert np.array_equal(loc(1), want["best_loc"]) and np.array_equal(loc(3), want["second_loc"])
    assert np.array_equal(rc & 1, want["best_rc"]) and np.array_equal((rc >> 1) & 1, want["second_rc"])
    assert (n_ext, passes, multi) == (want["n_extensions"], want["passes"], want["multi_passes"]) and multi > 0 and seeding == 3
    # a read of 1024 symbols: refused, nothing written
    lens = [100, 1024, 120]
    short = [text[1000 * (k + 1):1000 * (k + 1) + M].copy() for k, M in enumerate(lens)]
    syms, off = stored_stream(short)
    syms.tofile(str(tmp_path / "stored.u8")); off.tofile(str(tmp_path / "offsets.u32")); np.full(3, -60, np.int32).tofile(str(tmp_path / "min_scores.i32"))
    out = subprocess.run([exe, str(tmp_path), "3", str(oracle.SEMI_GLOBAL), "0", "1", "0"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 3 and "refused" in out.stdout and "1024" in out.stdout, out.stdout + out.stderr
    assert (np.fromfile(str(tmp_path / "best.i32"), np.int32) == 0x5A5A5A5A).all() and (np.fromfile(str(tmp_path / "best_rc.u8"), np.uint8) == 0xA5).all()
