"""GPU: the q-group build in its string and set form, and rank, locate and merge over it, under the scratch check mode
(amd.set_scratch_check) for fills 0x00, 0xFF and 0x02.  The builds' own buffers are filled by the library before any work, so a
table, an SS or a cursor the build does not initialise itself shows as a result that differs from the restatement of
tests/test_qgroup_oracle.py; the caller's temp and output buffers are filled here with the same byte."""
import numpy as np
import pytest

import test_qgram_oracle as O
import test_qgroup_oracle as G
from test_gpu_qgram import pack, text_of, u64
from test_gpu_qgram_check import _run
from test_gpu_qgroup import check_group

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[0x00, 0xFF, 0x02])
def fill(amd, request):
    amd.set_scratch_check(True, request.param)
    yield request.param
    amd.set_scratch_check(False)


@pytest.mark.parametrize("bits,ss,q", [(2, 2, 12), (4, 2, 5), (8, 2, 2), (4, 4, 5)])
def test_string_index_under_check(amd, orc, fill, bits, ss, q):
    import torch
    rng = np.random.default_rng(q + bits)
    s = text_of(rng, 5000, bits, with_n=True)
    s[:200] = s[2000:2200]
    s[3000:3400] = 0                                                  # a contended slot that takes the segmented sort
    want = O.string_index(s, q, ss)
    gidx = amd.QGroupIndex.build(pack(orc, s, bits), bits, len(s), q, ss)
    check_group(amd, gidx, G.group_of(want))
    allg = O.qgrams_at(s, 0, len(s), np.arange(len(s)), q, ss)
    queries = np.sort(np.concatenate([allg[rng.integers(0, len(s), 2000)], np.array([1, 2, 3, 1 << 40], np.uint64)]))
    _run(amd, torch, gidx, want, queries, rng.integers(0, 1 << 32, len(queries), dtype=np.uint64).astype(np.uint32), 7, fill)
    gidx.close()


@pytest.mark.parametrize("interval", [1, 10])
def test_set_index_under_check(amd, orc, fill, interval):
    import torch
    rng = np.random.default_rng(interval)
    strings = [text_of(rng, int(L), 4, with_n=True) for L in rng.integers(0, 120, 80)] + [np.zeros(100, np.uint8)] * 5
    syms = np.concatenate(strings)
    offs = np.zeros(len(strings) + 1, np.uint32)
    offs[1:] = np.cumsum([len(x) for x in strings])
    ss = amd.PackedStringSet(orc.pack4(syms), 4, len(strings), offsets=offs, ranges=True)
    want = O.set_index(strings, 12, 2, interval)
    gidx = amd.QGroupSetIndex.build(ss, 12, 2, interval)
    check_group(amd, gidx, G.group_of(want))
    text = np.concatenate([x[:50] for x in strings])
    qg, pos = O.generate(text, len(text), 12, 2, 0, len(text), True)
    g, p = amd.generate_qgrams(12, 2, orc.pack4(text), 4, len(text), 0, len(text), sort=True)
    assert np.array_equal(u64(g), qg) and np.array_equal(amd.u32(p), pos)
    _run(amd, torch, gidx, want, qg, pos, 16, fill)
    gidx.close()


def test_empty_inputs_under_check(amd, fill):
    gidx = amd.QGroupIndex.build(np.zeros(16, np.uint32), 2, 0, 5, 2)
    check_group(amd, gidx, G.group_of(O.string_index(np.zeros(0, np.uint8), 5, 2)))
    sset = amd.PackedStringSet(np.zeros(16, np.uint8), 8, 0, offsets=np.zeros(1, np.uint32), ranges=True)
    gset = amd.QGroupSetIndex.build(sset, 5, 2, 3)
    check_group(amd, gset, G.group_of(O.set_index([], 5, 2, 3)))
    gidx.close(); gset.close()
