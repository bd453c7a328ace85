"""The C++ mirror MEMFilter<amd_device_tag> (tests/cpp/test_mem_filter.cpp): it builds against the header, and on a GPU gives the
same ranges, first ranges, slots and hits as the Python path (amd.MEMFilter) over the same text and reads."""
import os
import subprocess

import numpy as np
import pytest

from test_mem_oracle import UNLIMITED, make_reads, make_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(out):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "nvbio-gpl_amd", "host"), "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "test_mem_filter.cpp"),
                           "-L" + os.path.join(ROOT, "nvbio-gpl_amd", "lib"), "-lnvbio_amd", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "nvbio-gpl_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib", "-o", out])


def test_mem_filter_mirror_compiles(tmp_path):
    _build(str(tmp_path / "test_mem_filter"))


@pytest.mark.gpu
@pytest.mark.parametrize("params", [(1, UNLIMITED, 1, UNLIMITED, UNLIMITED), (2, 30, 19, 28, 10)])
def test_mem_filter_mirror_equals_python(amd, orc, tmp_path, params):
    exe = str(tmp_path / "test_mem_filter")
    _build(exe)
    rng = np.random.default_rng(31)
    text = make_text(rng, 50_000)
    reads = make_reads(rng, text, 300, [40, 150, 400])
    offs = np.zeros(len(reads) + 1, np.uint32)
    offs[1:] = np.cumsum([len(r) for r in reads])
    syms = np.concatenate(reads)
    text.tofile(str(tmp_path / "text.u8")); syms.tofile(str(tmp_path / "reads.u8")); offs.tofile(str(tmp_path / "offsets.u32"))
    out = subprocess.run([exe, str(tmp_path)] + [str(p) for p in params], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mem filter ok" in out.stdout

    f = amd.FMIndex.build(orc.pack2(text), len(text), kmer_len=0, sa_int=4)
    r = amd.FMIndex.build(orc.pack2(text[::-1].copy()), len(text), kmer_len=0, sa_int=4)
    mf = amd.MEMFilter()
    ss = amd.PackedStringSet(np.concatenate([syms, np.zeros(16, np.uint8)]), 8, len(reads), offsets=offs, ranges=True)
    n = mf.rank(f, r, ss, *params)
    assert np.array_equal(np.fromfile(str(tmp_path / "ranges.u32"), np.uint32).reshape(-1, 4), amd.u32(mf.ranges()).reshape(-1, 4))
    assert np.array_equal(np.fromfile(str(tmp_path / "first.u32"), np.uint32), amd.u32(mf.first_ranges()))
    assert np.array_equal(np.fromfile(str(tmp_path / "slots.u64"), np.uint64), mf.slots().cpu().numpy().astype(np.uint64))
    assert np.array_equal(np.fromfile(str(tmp_path / "hits.u32"), np.uint32).reshape(-1, 4), amd.u32(mf.locate(0, n)).reshape(-1, 4))
    f.close(); r.close()
