"""The C++ mirror of the sufsort module (cuda::suffix_sort / cuda::bwt / cuda::find_primary of nvbio_amd.hpp, driven by
tests/cpp/test_sufsort.cpp): it builds against the header, and on a GPU its handlers receive what the Python mirror returns for
the same set and text."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(out):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "nvbio-gpl_amd", "host"), "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "test_sufsort.cpp"),
                           "-L" + os.path.join(ROOT, "nvbio-gpl_amd", "lib"), "-lnvbio_amd", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "nvbio-gpl_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib", "-o", out])


def test_sufsort_mirror_compiles(tmp_path):
    _build(str(tmp_path / "test_sufsort"))


@pytest.mark.gpu
@pytest.mark.parametrize("bits,flags", [(2, 0), (4, 1), (8, 0)])
def test_sufsort_mirror_equals_python(amd, orc, tmp_path, bits, flags):
    import torch
    from test_gpu_qgram import pack
    exe = str(tmp_path / "test_sufsort")
    _build(exe)
    rng = np.random.default_rng(bits)
    genome = rng.integers(0, 4, 2000, dtype=np.uint8)
    lens = rng.integers(0, 90, 300)
    lens[[3, 100, 299]] = 0
    reads = [genome[s:s + L].copy() for s, L in zip(rng.integers(0, 1900, 300), lens)]
    offs = np.zeros(len(reads) + 1, np.uint32)
    offs[1:] = np.cumsum(lens)
    packed = pack(orc, np.concatenate(reads), bits)
    text = rng.integers(0, 4, 5000, dtype=np.uint8)
    text[1000:1300] = text[3000:3300]
    text2 = orc.pack2(text)
    packed.tofile(str(tmp_path / "symbols.bin")); offs.tofile(str(tmp_path / "offsets.u32"))
    text2.tofile(str(tmp_path / "text2.u32")); np.array([len(text)], np.uint32).tofile(str(tmp_path / "text_len.u32"))
    out = subprocess.run([exe, str(tmp_path), str(bits), str(flags)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "sufsort ok" in out.stdout

    sset = amd.PackedStringSet(packed, bits, len(reads), offsets=offs, ranges=True)
    suf, glb, st = amd.set_suffix_sort(sset, flags)
    bwt, suf2, _ = amd.set_bwt(sset, flags)
    suf, glb = amd.u32(suf).reshape(-1, 2), amd.u32(glb)
    ld = lambda name, dt: np.fromfile(str(tmp_path / name), dt)  # noqa: E731
    assert st["n_suffixes"] == len(glb) > 0
    assert np.array_equal(ld("sort_global.u32", np.uint32), glb)
    assert np.array_equal(ld("sort_ids.u32", np.uint32), suf[:, 1])
    assert np.array_equal(ld("sort_cum.u32", np.uint32), np.cumsum(lens + (0 if flags else 1)).astype(np.uint32))
    for name in ("bwt_host.u8", "bwt_dev.u8"):
        assert np.array_equal(ld(name, np.uint8), bwt.cpu().numpy())
    for name in ("suf_host.u32", "suf_dev.u32"):
        assert np.array_equal(ld(name, np.uint32).reshape(-1, 2), suf)
    assert np.array_equal(amd.u32(suf2).reshape(-1, 2), suf)
    assert np.array_equal(ld("sa.u32", np.uint32), amd.u32(amd.suffix_sort(text2, len(text))))
    words, primary = amd.bwt(text2, len(text))
    assert np.array_equal(ld("bwt.u32", np.uint32), amd.u32(words)) and int(ld("primary.u32", np.uint32)[0]) == primary
    torch.cuda.synchronize()
