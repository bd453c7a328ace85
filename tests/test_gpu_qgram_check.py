"""GPU: the q-gram build, rank, locate and merge cases under the scratch check mode (amd.set_scratch_check) for fills 0x00, 0xFF and
0x02.  The builds' own buffers are filled by the library; the caller's temp and output buffers are filled here with the same byte.
Results must equal the restatement of tests/test_qgram_oracle.py, which catches reads of build buffers or temp never written."""
import numpy as np
import pytest

import test_qgram_oracle as O
from test_gpu_qgram import check_index, pack, text_of, u64

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[0x00, 0xFF, 0x02])
def fill(amd, request):
    amd.set_scratch_check(True, request.param)
    yield request.param
    amd.set_scratch_check(False)


def _filled(torch, shape, dtype, fill):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(fill)
    return t


def _run(amd, torch, gidx, want, queries, indices, interval, fill):
    qf = amd.QGramFilter()
    n = len(queries)
    qf._ranges = _filled(torch, (n, 2), torch.int32, fill)
    qf._slots = _filled(torch, n, torch.int64, fill)
    qf._temp = _filled(torch, 1 << 22, torch.uint8, fill)
    n_hits = qf.rank(gidx, torch.from_numpy(queries.view(np.int64)).cuda(), torch.from_numpy(indices.view(np.int32)).cuda())
    r, slots, wn = O.rank(want, queries)
    assert n_hits == wn and n_hits > 0
    assert np.array_equal(amd.u32(qf.ranges()).reshape(-1, 2), r) and np.array_equal(u64(qf.slots()), slots)
    wh = O.locate(want, r, slots, indices, 0, n_hits)
    hits = _filled(torch, wh.shape, torch.int32, fill)
    qf.locate(0, n_hits, hits)
    assert np.array_equal(amd.u32(hits).reshape(wh.shape), wh)
    b, e = n_hits // 3, n_hits // 3 + 77
    sub = _filled(torch, (e - b, wh.shape[1]), torch.int32, fill)
    qf.locate(b, e, sub)
    assert np.array_equal(amd.u32(sub).reshape(-1, wh.shape[1]), wh[b:e])
    qf._temp = _filled(torch, 1 << 24, torch.uint8, fill)
    qf._merged = _filled(torch, (n_hits, 2), torch.int32, fill)
    qf._counts = _filled(torch, n_hits, torch.int32, fill)
    m, c = qf.merge(interval, hits)
    wm, wc = O.merge(wh, interval)
    assert np.array_equal(amd.u32(m).reshape(wm.shape), wm) and np.array_equal(amd.u32(c), wc)


@pytest.mark.parametrize("bits,ss,q,qlut", [(2, 2, 20, 8), (4, 2, 5, 1), (8, 2, 12, 0), (4, 4, 5, 5)])
def test_string_index_under_check(amd, orc, fill, bits, ss, q, qlut):
    import torch
    rng = np.random.default_rng(q + bits)
    s = text_of(rng, 5000, bits, with_n=True)
    s[:200] = s[2000:2200]
    want = O.string_index(s, q, ss, qlut)
    gidx = amd.QGramIndex.build(pack(orc, s, bits), bits, len(s), q, ss, qlut)
    check_index(amd, gidx, want)
    allg = O.qgrams_at(s, 0, len(s), np.arange(len(s)), q, ss)
    queries = np.sort(np.concatenate([allg[rng.integers(0, len(s), 2000)], np.array([1, 2, 3], np.uint64)]))
    _run(amd, torch, gidx, want, queries, rng.integers(0, 1 << 32, len(queries), dtype=np.uint64).astype(np.uint32), 7, fill)
    gidx.close()


@pytest.mark.parametrize("interval", [1, 10])
def test_set_index_under_check(amd, orc, fill, interval):
    import torch
    rng = np.random.default_rng(interval)
    strings = [text_of(rng, int(L), 4, with_n=True) for L in rng.integers(0, 120, 80)]
    syms = np.concatenate(strings)
    offs = np.zeros(len(strings) + 1, np.uint32)
    offs[1:] = np.cumsum([len(x) for x in strings])
    ss = amd.PackedStringSet(orc.pack4(syms), 4, len(strings), offsets=offs, ranges=True)
    want = O.set_index(strings, 12, 2, interval, 8)
    gidx = amd.QGramSetIndex.build(ss, 12, 2, interval, 8)
    check_index(amd, gidx, want)
    text = np.concatenate([x[:50] for x in strings])
    qg, pos = O.generate(text, len(text), 12, 2, 0, len(text), True)
    g, p = amd.generate_qgrams(12, 2, orc.pack4(text), 4, len(text), 0, len(text), sort=True)
    assert np.array_equal(u64(g), qg) and np.array_equal(amd.u32(p), pos)
    _run(amd, torch, gidx, want, qg, pos, 16, fill)
    gidx.close()
