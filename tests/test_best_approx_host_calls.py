"""CPU-only: the host loops of host/nvbio_amd/best_approx.hpp call the library exactly as they did before they were written once, and the uniform
routes refuse a batch whose read index would not fit 32 bits before they touch the device.

The call sequence.  tests/cpp/test_best_approx_calls.cpp runs best_approx, best_approx_ragged and best_approx_paired over doubles of the HIP runtime
and of the nvbio_* entry points (no library, no GPU) and prints one line per call.  tests/golden/best_approx_host_calls.txt is that trace recorded
once from the same program compiled against best_approx.hpp as it stood BEFORE the three loops became one (the parent of the commit that added this
test; the public signatures did not change, so the program builds against both headers):

    g++ -std=c++17 -O1 -D__HIP_PLATFORM_AMD__ -Iinclude -Invbio-gpl_amd/host -I/opt/rocm/include tests/cpp/test_best_approx_calls.cpp -o calls
    ./calls > tests/golden/best_approx_host_calls.txt

The trace of the one loop equals it line for line: allocations and their sizes, every nvbio_* call with its scalar arguments and the buffers it is
handed, every hipMemsetAsync / hipMemcpyAsync, every host synchronisation.  The one difference the rewrite was allowed -- a stream synchronise on the
uniform route's `no seed fits` return -- does not exist: with seed_len clamped to the read length that return could never be taken, and it is gone.
The second parametrisation builds the same stand-alone program with AddressSanitizer and UBSan and asks for a clean run with the same trace."""
import ctypes
import os
import subprocess
from types import SimpleNamespace

import pytest

import __graft_entry__ as ge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "best_approx_host_calls.txt")
HOST_LIB = os.path.join(ROOT, "nvbio-gpl_amd", "lib", "libnvbio_amd_host.so")

# 28,633,116 reads of 150 bp = 4,294,967,400 symbols: the smallest such batch past 2^32
BIG_R, BIG_M = 28633116, 150


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_the_loops_call_the_library_as_before(tmp_path, sanitize):
    exe = str(tmp_path / "test_best_approx_calls")
    # the sanitizers' runtimes linked into the program itself: a stand-alone program, nothing is preloaded into it
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "nvbio-gpl_amd", "host"), "-I/opt/rocm/include"] + extra +
                          [os.path.join(ROOT, "tests", "cpp", "test_best_approx_calls.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-4000:]
    got, want = out.stdout.splitlines(), open(GOLDEN).read().splitlines()
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "line %d differs:\n  got  %s\n  want %s" % (k + 1, g, w)
    assert len(got) == len(want)
    # the trace is not vacuous: three seeding passes each, the several-hits-per-read phase, the paired route's third counter, the refused batch
    text = out.stdout
    assert text.count("nvbio_read_queue_filter") == 3 + 3 + 6 and "nvbio_read_queue_begin_ragged" in text and "nvbio_pe_opposite_output" in text
    assert "stats 434 13 11 3" in text and "invalid_argument best_approx_ragged: a read of 1024 symbols" in text


def _host():
    if not os.path.exists(HOST_LIB):
        pytest.skip("nvbio-gpl_amd/lib/libnvbio_amd_host.so has not been built")
    amd = ge.load_package()
    from importlib import import_module
    pipeline = import_module("nvbio_gpl_amd.pipeline")
    return amd, pipeline, pipeline._host_lib()


def _refused(host, rc):
    assert rc == 1
    msg = host.nvbio_host_last_error().decode()
    assert "2^32" in msg, msg


def test_best_approx_refuses_a_batch_of_2_to_the_32_symbols():
    """null device pointers: the refusal comes before any HIP or library call"""
    amd, pipeline, host = _host()
    assert BIG_R * BIG_M >= 2 ** 32 > (BIG_R - 1) * BIG_M
    scheme = amd.GotohScheme(2, 2, 6, -5, -3, -5, -3)
    p = pipeline._host_params(pipeline.NvBowtieParams(), 0, 0, True)
    st = pipeline._HostStats()
    u32, i32 = ctypes.c_uint32, ctypes.c_int32
    rc = host.nvbio_host_best_approx(0, None, None, u32(1000), None, None, u32(BIG_R), u32(BIG_M), 1, ctypes.byref(scheme.c), i32(0), ctypes.byref(p), None, None, None,
                                     ctypes.byref(st))
    _refused(host, rc)


@pytest.mark.parametrize("long_mate", [1, 2])
def test_best_approx_paired_refuses_either_mate_of_2_to_the_32_symbols(long_mate):
    amd, pipeline, host = _host()
    scheme = amd.GotohScheme(2, 2, 6, -5, -3, -5, -3)
    p = pipeline._host_params(pipeline.NvBowtieParams(), 0, 0, True)
    pe = pipeline._HostPairedParams(0, 0, 500, 1, 1)                      # nvbio_host_paired_params: policy, min / max fragment, overlap, unpaired
    st = pipeline._HostPairedStats()
    u32, i32 = ctypes.c_uint32, ctypes.c_int32
    lens = (BIG_M, 100) if long_mate == 1 else (100, BIG_M)
    rc = host.nvbio_host_best_approx_paired(0, None, None, u32(1000), None, None, None, None, u32(BIG_R), u32(lens[0]), u32(lens[1]), 1, ctypes.byref(scheme.c), i32(0),
                                            i32(0), ctypes.byref(p), ctypes.byref(pe), None, None, None, ctypes.byref(st))
    _refused(host, rc)


def test_all_mapping_refuses_a_batch_of_2_to_the_32_symbols():
    amd, pipeline, host = _host()
    scheme = amd._SWScheme(0, -1, -1, -1)                                 # nvbio_sw_scheme: edit distance
    p = amd._AllMappingParams(22, 0, 2, 15, 0, 2, 0, 0, 0, 0)
    out = amd._AllMappingOutput()
    st = amd._AllMappingStats()
    u32 = ctypes.c_uint32
    rc = host.nvbio_host_all_mapping(0, None, None, u32(1000), None, u32(BIG_R), u32(BIG_M), ctypes.byref(scheme), ctypes.c_int32(-15), ctypes.byref(p), ctypes.byref(out), None,
                                     ctypes.byref(st))
    _refused(host, rc)


def test_the_python_loop_refuses_a_batch_of_2_to_the_32_symbols():
    """before it touches the device: the index and the genome are None, the batch a stub"""
    amd, pipeline, _ = _host()
    batch = SimpleNamespace(n=BIG_R, read_len=BIG_M, offsets=None)
    with pytest.raises(ValueError, match=r"2\^32"):
        pipeline.nvbowtie_best_approx(None, None, 1000, batch, pipeline.SeedExtendParams.end_to_end())
    # one read fewer is below the limit and gets past the guard (to the missing index)
    batch.n = BIG_R - 1
    with pytest.raises(AttributeError):
        pipeline.nvbowtie_best_approx(None, None, 1000, batch, pipeline.SeedExtendParams.end_to_end())
