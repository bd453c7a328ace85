"""The C++ mirror QGroupIndexDevice / QGroupSetIndexDevice under QGramFilterDevice (tests/cpp/test_qgroup_filter.cpp): it builds
against the header, and on a GPU gives the same ranges, slots, hits, merged diagonals and counts as the Python path
(amd.QGramFilter over amd.QGroupIndex / QGroupSetIndex) over the same text and reads, for both forms."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(out):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "nvbio-gpl_amd", "host"), "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "test_qgroup_filter.cpp"),
                           "-L" + os.path.join(ROOT, "nvbio-gpl_amd", "lib"), "-lnvbio_amd", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "nvbio-gpl_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib", "-o", out])


def test_qgroup_filter_mirror_compiles(tmp_path):
    _build(str(tmp_path / "test_qgroup_filter"))


@pytest.mark.gpu
@pytest.mark.parametrize("q,seed_interval,merge_interval", [(12, 10, 16), (8, 3, 5)])
def test_qgroup_filter_mirror_equals_python(amd, tmp_path, q, seed_interval, merge_interval):
    import torch
    exe = str(tmp_path / "test_qgroup_filter")
    _build(exe)
    rng = np.random.default_rng(q)
    text = rng.integers(0, 4, 40_000, dtype=np.uint8)
    text[20_000:20_500] = 0                                                   # a contended slot
    starts = rng.integers(0, len(text) - 200, 300)
    lens = rng.integers(30, 200, 300)
    reads = [text[s:s + L].copy() for s, L in zip(starts, lens)]
    for r in reads[::5]:
        r[rng.integers(0, len(r))] = 4                                        # an N
    offs = np.zeros(len(reads) + 1, np.uint32)
    offs[1:] = np.cumsum(lens)
    syms = np.concatenate(reads)
    text.tofile(str(tmp_path / "text.u8")); syms.tofile(str(tmp_path / "reads.u8")); offs.tofile(str(tmp_path / "offsets.u32"))
    out = subprocess.run([exe, str(tmp_path), str(q), str(seed_interval), str(merge_interval)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "qgroup filter ok" in out.stdout

    tpad = np.concatenate([text, np.zeros(16, np.uint8)])
    g, p = amd.generate_qgrams(q, 2, tpad, 8, len(text), 0, len(text), sort=True)
    ss = amd.PackedStringSet(np.concatenate([syms, np.zeros(16, np.uint8)]), 8, len(reads), offsets=offs, ranges=True)
    for kind, index in (("string", amd.QGroupIndex.build(tpad, 8, len(text), q, 2)), ("set", amd.QGroupSetIndex.build(ss, q, 2, seed_interval))):
        qf = amd.QGramFilter()
        n = qf.rank(index, g, p)
        hits = qf.locate(0, n)
        m, c = qf.merge(merge_interval, hits)
        ld = lambda name, dt: np.fromfile(str(tmp_path / ("%s_%s" % (kind, name))), dt)  # noqa: E731
        assert np.array_equal(ld("ranges.u32", np.uint32), amd.u32(qf.ranges()).reshape(-1))
        assert np.array_equal(ld("slots.u64", np.uint64), qf.slots().cpu().numpy().view(np.uint64))
        assert np.array_equal(ld("hits.u32", np.uint32), amd.u32(hits).reshape(-1))
        assert np.array_equal(ld("merged.u32", np.uint32), amd.u32(m).reshape(-1))
        assert np.array_equal(ld("counts.u32", np.uint32), amd.u32(c))
        assert np.array_equal(ld("ss.u32", np.uint32), amd.u32(index.arrays()["SS"]))
        assert n > 0 and len(c) > 0
        index.close()
    torch.cuda.synchronize()
