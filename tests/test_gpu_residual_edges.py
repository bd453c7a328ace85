"""GPU: the two routes that turn residual seeds into diagonal keys -- nvbio_fm_residual_diagonals (radix sort + residual_locate_kernel) and
nvbio_fm_filter_scan + nvbio_fm_filter_locate_diagonals[_ragged] (fm_filter_locate_kernel over locate_ranges), csrc/fm_index.hip -- on the
named cases of residual_cases.py, key for key against the restatement of residual_cpu.py, which knows a plain suffix array and the key rule
and no FM index (test_residual_oracle.py pins it and proves the cases are what they say).  The one-call route: the number of keys and their
sorted multiset (the order between workgroups is not defined), the same on a second run, and its set against the two-call route on the capped
ranges.  The two-call route: the scan's sums, then every window in order.  Calls go through ctypes into poisoned buffers between poisoned
guard bands: every slot a call is not to write keeps its poison.  Exact: no tolerance anywhere.  One index per sampling interval and module."""
import ctypes

import numpy as np
import pytest

import residual_cases as cases
import residual_cpu as rc

pytestmark = pytest.mark.gpu

GUARD = 64
POISON = cases.POISON
POISON64 = (POISON << 32) | POISON
ERR_INVALID, ERR_UNSUPPORTED = 1, 4

OC_CASES = list(cases.one_call_cases())
TC_CASES = list(cases.two_call_cases())


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def indices(amd, orc):
    """the device index of the cases' text with the full (sa_int = 1) or a sampled (sa_int = 16) suffix array, built once"""
    made = {}

    def get(sa_int):
        if sa_int not in made:
            made[sa_int] = amd.FMIndex.build(orc.pack2(cases.text()), cases.N_TEXT, kmer_len=0, sa_int=sa_int)
        return made[sa_int]
    yield get
    for f in made.values():
        f.close()


class Out:
    """a uint32 or uint64 output array between two guard bands, all poisoned"""

    def __init__(self, torch, n, wide=False):
        self.n, self.wide = n, wide
        self.fill = POISON64 if wide else POISON
        signed = int(np.array([self.fill], dtype=np.uint64 if wide else np.uint32).view(np.int64 if wide else np.int32)[0])
        self.buf = torch.full((n + 2 * GUARD,), signed, dtype=torch.int64 if wide else torch.int32, device="cuda:0")
        self.t = self.buf[GUARD:GUARD + n]

    def get(self):
        a = self.buf.cpu().numpy().view(np.uint64 if self.wide else np.uint32)
        assert (a[:GUARD] == self.fill).all() and (a[GUARD + self.n:] == self.fill).all(), "guard band overwritten"
        return a[GUARD:GUARD + self.n]

    def untouched(self):
        return bool((self.get() == self.fill).all())


def dev(torch, values, width=32):
    """a device tensor with the bit patterns of unsigned values (None stays None)"""
    if values is None:
        return None
    a = np.ascontiguousarray(values, dtype=np.uint64 if width == 64 else np.uint32)
    return torch.from_numpy(a.view(np.int64 if width == 64 else np.int32)).cuda()


def ptr(amd, t):
    return None if t is None or t.numel() == 0 else amd._ptr(t)


def residual_diagonals(amd, torch, fmi, x, y, ids, cap, g, keys=None, n=None, read_offsets="g", intervals="g"):
    """nvbio_fm_residual_diagonals into poisoned buffers -> (status, the keys' Out, n_keys' Out)"""
    n = len(ids) if n is None else n
    ranges = dev(torch, np.stack([np.asarray(x, dtype=np.uint32), np.asarray(y, dtype=np.uint32)], axis=1).reshape(-1))
    ids_d = dev(torch, ids)
    ro = dev(torch, g.read_offsets if read_offsets == "g" else read_offsets)
    iv = dev(torch, g.intervals if intervals == "g" else intervals)
    keys = Out(torch, n * cap, wide=True) if keys is None else keys
    nk = Out(torch, 1)
    status = amd.lib().nvbio_fm_residual_diagonals(fmi._h, ptr(amd, ranges), ptr(amd, ids_d), n, cap, g.spr, g.interval or 0, g.seed_len, g.read_len or 0,
                                                   ptr(amd, ro), ptr(amd, iv), amd._ptr(keys.t), amd._ptr(nk.t), amd._stream_ptr("cuda:0"))
    torch.cuda.synchronize()
    return status, keys, nk


def filter_scan(amd, torch, fmi, ranges):
    """nvbio_fm_filter_scan into a poisoned buffer -> (ranges on the device, the slots' Out, total)"""
    r = dev(torch, np.asarray(ranges, dtype=np.uint32).reshape(-1))
    slots = Out(torch, len(ranges), wide=True)
    total = ctypes.c_uint64(POISON64)
    amd._check(amd.lib().nvbio_fm_filter_scan(fmi._h, ptr(amd, r), len(ranges), amd._ptr(slots.t), ctypes.byref(total), amd._stream_ptr("cuda:0")))
    return r, slots, int(total.value)


def locate_diagonals(amd, torch, fmi, r, slots, n, begin, end, g, strand, ids=None, direct=None, room=None):
    """nvbio_fm_filter_locate_diagonals, or its ragged form where the geometry is ragged, into a poisoned buffer -> (status, the keys' Out)"""
    keys = Out(torch, max(end - begin, 0) if room is None else room, wide=True)
    L, s = amd.lib(), amd._stream_ptr("cuda:0")
    if g.read_offsets is None:
        status = L.nvbio_fm_filter_locate_diagonals(fmi._h, ptr(amd, r), amd._ptr(slots.t), ptr(amd, direct), n, begin, end, g.spr, g.interval, g.seed_len,
                                                    g.read_len, strand, ptr(amd, ids), amd._ptr(keys.t), s)
    else:
        ro, iv = dev(torch, g.read_offsets), dev(torch, g.intervals)
        status = L.nvbio_fm_filter_locate_diagonals_ragged(fmi._h, ptr(amd, r), amd._ptr(slots.t), ptr(amd, direct), n, begin, end, g.spr, g.seed_len,
                                                           amd._ptr(ro), amd._ptr(iv), strand, ptr(amd, ids), amd._ptr(keys.t), s)
    torch.cuda.synchronize()
    return status, keys


_ONE = {}


def one_call_want(case):
    """(sorted keys, number dropped) of a one-call case by the restatement; computed once"""
    if case.name not in _ONE:
        kept, dropped = rc.one_call_keys(cases.scan_text(), case.entries, case.cap, case.g)
        _ONE[case.name] = (np.array(sorted(kept.elements()), dtype=np.uint64), dropped)
    return _ONE[case.name]


def two_call_set(amd, torch, fmi, x, y, ids, cap, g):
    """the distinct keys of the two-call route over the ranges cut to their first cap rows, the ids as query_ids"""
    x, y = np.asarray(x, dtype=np.int64), np.asarray(y, dtype=np.int64)
    cut = np.stack([x, np.where(y >= x, np.minimum(y, x + cap - 1), y)], axis=1)
    r, slots, total = filter_scan(amd, torch, fmi, cut)
    if total == 0:
        return np.zeros(0, np.uint64)
    status, keys = locate_diagonals(amd, torch, fmi, r, slots, len(ids), 0, total, g, 0, ids=dev(torch, ids))
    assert status == 0
    return np.unique(keys.get())


def check_one_call(amd, torch, fmi, x, y, ids, cap, g, want, name):
    seen = []
    for run in range(2):                                            # a second run gives the same multiset
        status, keys, nk = residual_diagonals(amd, torch, fmi, x, y, ids, cap, g)
        assert status == 0, (name, amd.lib().nvbio_amd_last_error())
        n_keys, k = int(nk.get()[0]), keys.get()
        assert n_keys == len(want), (name, run, "n_keys", n_keys, len(want))
        assert (k[n_keys:] == POISON64).all(), (name, run, "a slot from n_keys to n * cap was written")
        got = np.sort(k[:n_keys])
        assert np.array_equal(got, want), (name, run, "keys")
        seen.append(got)
    assert np.array_equal(seen[0], seen[1])
    assert np.array_equal(np.unique(seen[0]), two_call_set(amd, torch, fmi, x, y, ids, cap, g)), (name, "the two-call route's set")


# ---- the one-call route -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", OC_CASES, ids=[c.name for c in OC_CASES])
def test_one_call_case(amd, indices, case):
    import torch
    e = np.array(case.entries, dtype=np.int64).reshape(-1, 3)
    want, _ = one_call_want(case)
    check_one_call(amd, torch, indices(1), e[:, 0], e[:, 1], e[:, 2], case.cap, case.g, want, case.name)


def test_one_call_large(amd, indices):
    """8,192 x 256 + 300 entries, cap = 1: the loop over workgroups wraps at the cap of the grid; chains of duplicates, some broken by an empty range"""
    import torch
    x, y, ids = cases.large_case()
    want, dropped = rc.one_call_keys_cap1(cases.scan_text(), x, y, ids, cases.G_LARGE)
    assert dropped > 0
    check_one_call(amd, torch, indices(1), x, y, ids, 1, cases.G_LARGE, want, "large")


def test_one_call_without_entries_writes_nothing(amd, indices):
    import torch
    keys = Out(torch, 8, wide=True)
    status, keys, nk = residual_diagonals(amd, torch, indices(1), [], [], [], 4, cases.G8, keys=keys)
    assert status == 0 and int(nk.get()[0]) == 0 and keys.untouched()


# ---- the two-call route -----------------------------------------------------------------------------------------------------------
_TWO = {}


def two_call_want(case, k):
    if (case.name, k) not in _TWO:
        _TWO[case.name, k] = np.array(rc.two_call_keys(cases.scan_text(), list(case.ranges), case.ids, case.direct, case.strand, case.geoms[k]), dtype=np.uint64)
    return _TWO[case.name, k]


@pytest.mark.parametrize("sa_int", [1, 16])
@pytest.mark.parametrize("case", TC_CASES, ids=[c.name for c in TC_CASES])
def test_two_call_case(amd, indices, case, sa_int):
    import torch
    fmi = indices(sa_int)
    n = len(case.ranges)
    sums = rc.inclusive_sizes(cases.plain_of(case))                 # (a range that holds a position is one row: the sizes are those of the plain ranges)
    r, slots, total = filter_scan(amd, torch, fmi, case.ranges)
    assert total == int(sums[-1]) and np.array_equal(slots.get(), sums), (case.name, "scan")
    ids, direct = dev(torch, case.ids), None if case.direct is None else torch.tensor(case.direct, dtype=torch.uint8, device="cuda:0")
    for k, g in enumerate(case.geoms):
        want = two_call_want(case, k)
        assert len(want) == total
        for b, e in case.windows:
            status, keys = locate_diagonals(amd, torch, fmi, r, slots, n, b, e, g, case.strand, ids=ids, direct=direct)
            assert status == 0, (case.name, k, b, e, amd.lib().nvbio_amd_last_error())
            assert np.array_equal(keys.get(), want[b:e]), (case.name, "ragged" if k else "fixed", sa_int, b, e)
    assert np.array_equal(slots.get(), sums)                        # the slots are read only


@pytest.mark.parametrize("sa_int", [1, 16])
def test_two_call_empty_window_writes_nothing(amd, indices, sa_int):
    import torch
    case = TC_CASES[0]
    fmi = indices(sa_int)
    r, slots, total = filter_scan(amd, torch, fmi, case.ranges)
    for g in case.geoms:
        for b, e in ((5, 5), (7, 3), (total, total), (total, 0)):
            status, keys = locate_diagonals(amd, torch, fmi, r, slots, len(case.ranges), b, e, g, 0, room=16)
            assert status == 0 and keys.untouched(), (b, e)


# ---- argument checks --------------------------------------------------------------------------------------------------------------
def test_one_call_refuses_bad_arguments_and_writes_nothing(amd, indices):
    """a refused call returns NVBIO_ERR_INVALID or NVBIO_ERR_UNSUPPORTED and leaves the keys, n_keys and the guard bands as they were"""
    import torch
    case = next(c for c in OC_CASES if c.name == "family_12")
    e = np.array(case.entries, dtype=np.int64).reshape(-1, 3)
    x, y, ids, g = e[:, 0], e[:, 1], e[:, 2], case.g
    gr = next(c for c in OC_CASES if c.name == "ragged").g

    def refused(want, fmi, cap, geometry=g, **kw):
        keys = Out(torch, 64 * len(ids), wide=True)
        status, keys, nk = residual_diagonals(amd, torch, fmi, x, y, ids, cap, geometry, keys=keys, **kw)
        assert status == want, (status, kw)
        assert keys.untouched() and nk.untouched(), kw

    refused(ERR_INVALID, indices(1), 0)
    refused(ERR_INVALID, indices(1), 65)
    # n * cap = 2^31 through the argument check alone: the call returns before it reads an entry or writes a key
    refused(ERR_INVALID, indices(1), 64, n=1 << 25)
    refused(ERR_INVALID, indices(1), 1, n=1 << 31)
    refused(ERR_UNSUPPORTED, indices(16), 4)
    refused(ERR_INVALID, indices(1), 4, geometry=gr, intervals=None)
    refused(ERR_INVALID, indices(1), 4, geometry=gr, read_offsets=None)
    status, keys, nk = residual_diagonals(amd, torch, indices(1), x, y, ids, 4, g)      # ... and the handle still answers
    assert status == 0 and int(nk.get()[0]) == len(one_call_want(case._replace(name="family_12_cap_4", cap=4))[0])
