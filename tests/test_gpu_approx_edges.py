"""GPU: fm_hamming_backtrack_kernel and fm_map_approx_kernel (csrc/fm_index.hip) on the named cases of approx_cases.py, against both references:
the oracle hit for hit -- ranges in delegate order, deques in heap order -- and the text scans of approx_cpu.py, which know nothing about FM indices
(test_approx_oracle.py proves the cases are what they say): counts, numbers of ranges, sets of ranges, multisets of hits, reseed bits.  2-, 4- and
8-bit symbols wherever a case holds no N.  Every output lies between poisoned guard bands that must survive, and every slot a call is not to write
must keep its poison.  Exact: no tolerance anywhere.  One index per text and module."""
import ctypes

import numpy as np
import pytest

import approx_cases as cases
import approx_cpu as ap

pytestmark = pytest.mark.gpu

GUARD = 64
POISON = cases.POISON
POISON8 = 0xEE
ERR_UNSUPPORTED = 4

BT_CASES = list(cases.backtrack_cases())
MP_CASES = list(cases.mapper_cases())


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def indices(amd, orc):
    """(oracle index, device index) of a named text or its reverse, built once; the device index wraps the oracle's arrays"""
    made = {}

    def get(name, reverse=False):
        if (name, reverse) not in made:
            t = cases.text(name)
            h = orc.build_index(t[::-1].copy() if reverse else t)
            made[name, reverse] = (h, amd.FMIndex.from_arrays(h.n, h.primary, h.L2, h.bwt_occ, h.ssa, kmer_len=0))
        return made[name, reverse]
    yield get
    for _, f in made.values():
        f.close()


class Out:
    """an int32 or uint8 output array between two guard bands, all poisoned"""

    def __init__(self, torch, n, u8=False):
        self.n, self.u8 = n, u8
        fill = POISON8 if u8 else int(np.uint32(POISON).view(np.int32))
        self.buf = torch.full((n + 2 * GUARD,), fill, dtype=torch.uint8 if u8 else torch.int32, device="cuda:0")
        self.t = self.buf[GUARD:GUARD + n]

    def get(self):
        a = self.buf.cpu().numpy()
        a = a if self.u8 else a.view(np.uint32)
        fill = POISON8 if self.u8 else POISON
        assert (a[:GUARD] == fill).all() and (a[GUARD + self.n:] == fill).all(), "guard band overwritten"
        return a[GUARD:GUARD + self.n].astype(np.int64)


def packed(orc, torch, symbols, bits):
    symbols = np.ascontiguousarray(symbols, dtype=np.uint8)
    if bits == 8:
        return torch.from_numpy(np.concatenate([symbols, np.zeros(16, np.uint8)])).cuda()
    return torch.from_numpy((orc.pack2(symbols) if bits == 2 else orc.pack4(symbols)).view(np.int32)).cuda()


def run_backtrack(amd, torch, fmi, qs, seed, mm, quirks, max_ranges):
    """nvbio_fm_hamming_backtrack into poisoned buffers -> (counts [Q], n_ranges [Q], ranges [Q, max_ranges, 2])"""
    cnt, nr, rg = Out(torch, qs.n), Out(torch, qs.n), Out(torch, qs.n * max_ranges * 2)
    s = qs.c_struct()
    amd._check(amd.lib().nvbio_fm_hamming_backtrack(fmi._h, ctypes.byref(s), seed, mm, amd.BACKTRACK_REFERENCE_QUIRKS if quirks else 0, amd._ptr(cnt.t),
                                                    amd._ptr(nr.t), amd._ptr(rg.t), max_ranges, amd._stream_ptr("cuda:0")))
    return cnt.get(), nr.get(), rg.get().reshape(qs.n, max_ranges, 2)


_BT_WANT = {}


def backtrack_want(orc, hidx, case):
    """per query: the oracle's (count, n, ranges in delegate order) and, in default mode, the scan's (count, n, set of ranges); computed once"""
    if case.name not in _BT_WANT:
        stream, offs = cases.stream_of(case)
        st = cases.scan_text(case.text)
        o = [orc.hamming_backtrack(hidx, stream, int(offs[i]), len(q), case.seed, case.mm, quirks=case.quirks, cap=2048) for i, q in enumerate(case.queries)]
        s = None if case.quirks else [ap.backtrack_scan(st, q, case.seed, case.mm) for q in case.queries]
        _BT_WANT[case.name] = (o, s)
    return _BT_WANT[case.name]


# ---- hamming_backtrack ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BT_CASES, ids=[c.name for c in BT_CASES])
def test_backtrack_case(amd, orc, indices, case):
    import torch
    hidx, fmi = indices(case.text)
    stream, offs = cases.stream_of(case)
    Q = len(case.queries)
    want_o, want_s = backtrack_want(orc, hidx, case)
    most = max(w[1] for w in want_o)
    max_ranges = {"one": 1, "most-1": most - 1}.get(case.max_ranges, case.max_ranges)
    assert max_ranges >= 1
    if case.family == "truncated":
        assert max_ranges < most
    for bits in cases.widths_of(stream):
        qs = amd.PackedStringSet(packed(orc, torch, stream, bits), bits, Q, offsets=offs, ranges=True)
        cnt, nr, rg = run_backtrack(amd, torch, fmi, qs, case.seed, case.mm, case.quirks, max_ranges)
        for i in range(Q):
            c, n, ranges = want_o[i]
            assert (cnt[i], nr[i]) == (c, n), (case.name, bits, i, "oracle")
            k = min(n, max_ranges)
            assert np.array_equal(rg[i, :k], ranges[:k]), (case.name, bits, i, "delegate order")
            assert (rg[i, k:] == POISON).all(), (case.name, bits, i, "written at or beyond max_ranges / n_ranges")
            if want_s is not None:
                sc, sn, sset = want_s[i]
                assert (cnt[i], nr[i]) == (sc, sn), (case.name, bits, i, "scan")
                if n <= max_ranges:
                    assert set(map(tuple, rg[i, :n].tolist())) == sset, (case.name, bits, i, "scan ranges")
                else:
                    assert set(map(tuple, rg[i, :k].tolist())) < sset, (case.name, bits, i, "scan ranges, truncated")


def test_backtrack_stack_overflow_is_an_error_and_the_handle_lives(amd, orc, indices):
    """d = 128: one branch finds the 128-entry stack full; the call returns NVBIO_ERR_UNSUPPORTED, the library's guarded error (the entry is dropped,
    nothing is written past the stack), and the next call on the same handle answers the d = 127 query"""
    import torch
    _, fmi = indices("poly_t")
    over = cases.overflow_case()
    stream, offs = cases.stream_of(over)
    qs = amd.PackedStringSet(packed(orc, torch, stream, 2), 2, 1, offsets=offs, ranges=True)
    with pytest.raises(amd.NvbioError) as e:
        fmi.hamming_backtrack(qs, over.seed, over.mm, max_ranges=8)
    assert e.value.status == ERR_UNSUPPORTED and "128-entry stack" in str(e.value)
    full = cases.poly_t_query(127)
    qs = amd.PackedStringSet(packed(orc, torch, full, 2), 2, 1, offsets=np.array([0, len(full)], dtype=np.uint32), ranges=True)
    cnt, nr, rg = run_backtrack(amd, torch, fmi, qs, cases.STACK_SEED, 1, False, 8)
    count, n, ranges = ap.backtrack_scan(cases.scan_text("poly_t"), full, cases.STACK_SEED, 1)
    assert (count, n) == (59, 2) and (cnt[0], nr[0]) == (59, 2) and set(map(tuple, rg[0, :2].tolist())) == ranges


# ---- the approximate seed mapper --------------------------------------------------------------------------------------------------
_MP_WANT = {}


def mapper_want(orc, indices, case):
    """per read: the oracle's (deque in heap order, reseed) and the scan's (sorted hits, range_count, reseed); computed once"""
    if case.name not in _MP_WANT:
        hidx, ridx = indices(case.text)[0], indices(case.text, True)[0]
        fwd, rev = cases.scan_text(case.text), cases.scan_text(case.text, True)
        p = case.p
        seed_off = p["first_offset"] + np.arange(p["seeds_per_read"]) * p["seed_interval"]
        o = [orc.map_approx_read(hidx, ridx, s, seed_off, p["seed_len"], case.max_hits, p["rep_seeds"]) for s in case.reads]
        s = [ap.map_approx_scan(fwd, rev, s, p) for s in case.reads]
        _MP_WANT[case.name] = (o, [(x[0], x[2], x[3]) for x in s])
    return _MP_WANT[case.name]


@pytest.mark.parametrize("case", MP_CASES, ids=[c.name for c in MP_CASES])
def test_map_approx_case(amd, orc, indices, case):
    import torch
    fmi, rfmi = indices(case.text)[1], indices(case.text, True)[1]
    want_o, want_s = mapper_want(orc, indices, case)
    p = case.p
    R = len(case.reads)
    sp = amd.SeedHitsParams(p["seeds_per_read"], p["seed_interval"], p["seed_len"], p["read_len"], first_offset=p["first_offset"], max_hits=case.max_hits,
                            rep_seeds=p["rep_seeds"])
    cap = amd.seed_hits_approx_capacity(sp)
    assert cap == min(cases.worst_hits(p["seeds_per_read"], p["seed_len"]), case.max_hits) + 1
    mapped = set(range(R)) if case.queue is None else set(case.queue.tolist())
    queue = None if case.queue is None else torch.from_numpy(case.queue.view(np.int32)).cuda()
    flat = case.reads.reshape(-1)
    seen = {}
    for bits in cases.widths_of(flat):
        deques, sizes, reseed = Out(torch, R * cap * 2), Out(torch, R), Out(torch, R, u8=True)
        amd.seed_hits_map_approx(fmi, rfmi, packed(orc, torch, flat, bits), bits, sp, len(mapped), deques.t, sizes.t, reseed.t, read_queue=queue)
        d, n, rs = deques.get().reshape(R, cap, 2), sizes.get(), reseed.get()
        for r in range(R):
            if r not in mapped:
                assert (d[r] == POISON).all() and n[r] == POISON and rs[r] == POISON8, (case.name, bits, r, "a read outside the queue was written")
                continue
            deque, o_reseed = want_o[r]
            hits, count, s_reseed = want_s[r]
            assert n[r] == len(deque) and np.array_equal(d[r, :n[r]], deque), (case.name, bits, r, "oracle, heap order")
            assert rs[r] == int(o_reseed) == int(s_reseed), (case.name, bits, r, "reseed")
            if case.max_hits >= count:
                assert sorted(map(tuple, d[r, :n[r]].tolist())) == hits, (case.name, bits, r, "scan")
            else:
                assert n[r] == case.max_hits, (case.name, bits, r, "scan, capped")
        valid = np.arange(cap)[None, :, None] < np.where(n == POISON, 0, n)[:, None, None]
        seen[bits] = (np.where(valid, d, 0), n, rs)
    for bits in seen:                                               # the symbol widths agree byte for byte
        assert all(np.array_equal(a, b) for a, b in zip(seen[bits], seen[8])), (case.name, bits)
    if case.family == "full":
        assert (seen[8][1] == 20 * p["seeds_per_read"]).all()
