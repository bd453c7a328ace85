"""CPU-only: a restatement of MEMFilter<device_tag>::rank (the MEM filter of include/nvbio_amd.h, csrc/mem.hip) over a naive index,
checked against the definitions.  tests/test_gpu_mem.py uses it as the oracle of the GPU path.

The naive index is a suffix array of the text (numpy prefix doubling; the suffix "$" sorts first, row 0) and SA intervals found by
bisection over it: every range here is the exact interval of its pattern, not the result of a chain of rank steps.  The passes are
written from the algorithm (see the header of csrc/mem.hip):
  right    from x, extend one symbol at a time while the interval keeps >= min_intv rows and no N is met; every length at which
           the interval size changes closes the range of the previous length (not the empty one), and the longest one closes the
           group -- if at least one range was closed before it (the reference records nothing otherwise).  The group is emitted
           longest first, the first one flagged; the next x is max(longest end, x + 1).
  left     extend every range to the left while it keeps >= min_intv rows and no N is met.
  discard  per group (a flagged entry starts one), in entry order: keep iff begin < the left-most begin kept so far in the group,
           length >= min_span and occurrences <= max_intv; the first kept entry of a group gets the flag.
  split    a kept MEM with length >= split_len and occurrences <= split_width becomes the right group from its midpoint with
           min_intv = occurrences + 1; then left and discard again.
  output   per read, ascending (begin, end), stable.
"""
import numpy as np
import pytest

FLAG = 1 << 31
UNLIMITED = 0xFFFFFFFF


def suffix_array(text):
    """rows 0..n of the suffix array of text + '$' ('$' smallest): prefix doubling"""
    n = len(text)
    N = n + 1
    rank = np.append(np.asarray(text, dtype=np.int64) + 1, 0)
    idx = np.arange(N)
    k = 1
    while True:
        r2 = np.where(idx + k < N, rank[np.minimum(idx + k, N - 1)], -1)
        sa = np.lexsort((r2, rank))
        key = rank[sa] * (N + 2) + (r2[sa] + 1)
        new = np.empty(N, dtype=np.int64)
        new[sa] = np.concatenate([[0], np.cumsum(key[1:] != key[:-1])])
        rank = new
        if rank.max() == N - 1:
            return sa
        k *= 2


class NaiveIndex:
    """the suffix array of a text over {0,1,2,3} and the SA interval (x, y) (inclusive; empty: y = x - 1) of any pattern"""

    def __init__(self, text):
        self.text = np.asarray(text, dtype=np.uint8)
        self.t = bytes(self.text)
        self.n = len(self.text)
        self.sa = suffix_array(self.text)
        self._memo = {}

    def _bound(self, p, strict):
        lo, hi, m = 0, self.n + 1, len(p)
        while lo < hi:
            mid = (lo + hi) // 2
            s = self.sa[mid]
            pre = self.t[s:s + m]
            if pre < p or (strict and pre == p):
                lo = mid + 1
            else:
                hi = mid
        return lo

    def interval(self, p):
        p = bytes(p)
        r = self._memo.get(p)
        if r is None:
            r = self._memo[p] = (self._bound(p, False), self._bound(p, True) - 1)
        return r

    def positions(self, x, y):
        return self.sa[x:y + 1]


def _size(r):
    return r[1] - r[0] + 1


def right_group(idx, read, sid, x, min_intv):
    """the ranges right_kmems pushes from x, in emit order (longest first, flagged), and the next x"""
    L = len(read)
    prev = (0, idx.n)
    closed = []
    i = x
    while i < L and read[i] <= 3:
        cur = idx.interval(read[x:i + 1])
        if _size(cur) < min_intv:
            break
        if _size(cur) != _size(prev):
            if i > x:
                closed.append([prev[0], prev[1], sid, False, x, i])
            prev = cur
        i += 1
    if closed:
        closed.append([prev[0], prev[1], sid, False, x, i])
    group = closed[::-1]
    if group:
        group[0][3] = True
    return group, (max(group[0][5], x + 1) if group else x + 1)


def left_extend(idx, read, m, min_intv):
    x, y, sid, flag, b, e = m
    while b > 0 and read[b - 1] <= 3:
        r = idx.interval(read[b - 1:e])
        if _size(r) < min_intv:
            break
        (x, y), b = r, b - 1
    return [x, y, sid, flag, b, e]


def discard(entries, max_intv, min_span, host=False):
    """host=True: the host find_kmems rule, whose left-most marker moves also for a MEM dropped only for max_intv"""
    out, leftmost = [], None
    for m in entries:
        x, y, sid, flag, b, e = m
        if flag:
            leftmost = None
        inside = leftmost is not None and b >= leftmost
        if not inside and e - b >= min_span and _size((x, y)) <= max_intv:
            out.append([x, y, sid, flag or leftmost is None, b, e])
            leftmost = b
        elif host and not inside and e - b >= min_span:
            leftmost = b
    return out


def mem_read(idx, read, sid, min_intv=1, max_intv=UNLIMITED, min_span=1, split_len=UNLIMITED, split_width=UNLIMITED, host=False):
    """the kept MEMs of one read, [x, y, string id, flag, begin, end], in output order"""
    read = bytes(np.asarray(read, dtype=np.uint8))
    cands, x = [], 0
    while x < len(read):
        g, x = right_group(idx, read, sid, x, min_intv)
        cands += g
    kept = discard([left_extend(idx, read, m, min_intv) for m in cands], max_intv, min_span, host)
    if split_len != UNLIMITED:
        assert not host
        new = []
        for m in kept:
            occ = _size((m[0], m[1]))
            if m[5] - m[4] >= split_len and occ <= split_width:
                new += right_group(idx, read, sid, (m[4] + m[5]) // 2, occ + 1)[0]
            else:
                new.append(m)
        kept = discard([left_extend(idx, read, m, min_intv) for m in new], max_intv, min_span)
    return sorted(kept, key=lambda m: (m[4], m[5]))


def mem_filter(idx, reads, **params):
    """(ranges [n_ranges, 4] uint32 as the C ABI's nvbio_mem_range, first_range [n + 1], slots uint64 [n_ranges])"""
    rows, first = [], [0]
    for sid, r in enumerate(reads):
        for x, y, s, flag, b, e in mem_read(idx, r, sid, **params):
            rows.append((x, y, s | (FLAG if flag else 0), b | (e << 16)))
        first.append(len(rows))
    ranges = np.array(rows, dtype=np.uint32).reshape(-1, 4)
    sizes = ranges[:, 1].astype(np.int64) - ranges[:, 0] + 1
    return ranges, np.array(first, dtype=np.uint32), np.cumsum(sizes).astype(np.uint64)


def locate(idx, ranges, slots, begin, end):
    """hits [end - begin, 4]: (text position, string id, span begin, span end) of the MEM occurrences [begin, end)"""
    out = np.zeros((max(end - begin, 0), 4), dtype=np.uint32)
    for h in range(begin, end):
        k = int(np.searchsorted(slots, h, side="right"))
        base = int(slots[k - 1]) if k else 0
        x, _, s, sp = (int(v) for v in ranges[k])
        out[h - begin] = (idx.sa[x + h - base], s & ~FLAG, sp & 0xFFFF, sp >> 16)
    return out


# ---- workloads ----------------------------------------------------------------------------------
def make_text(rng, n):
    t = rng.integers(0, 4, n, dtype=np.uint8)
    for _ in range(max(1, n // 2000)):                       # planted repeats: copies with a few differences
        L = int(rng.integers(30, 300)); s = int(rng.integers(0, n - L)); d = int(rng.integers(0, n - L))
        t[d:d + L] = t[s:s + L]
        m = rng.random(L) < 0.02
        t[d:d + L][m] = rng.integers(0, 4, int(m.sum()))
    return t


def make_reads(rng, text, R, lens, sub=0.02, indel=0.2, n_rate=0.005):
    """reads drawn from the text (one in eight random), with substitutions, indels and N's (4)"""
    n, reads = len(text), []
    for _ in range(R):
        L = int(rng.choice(lens))
        if rng.random() < 0.125 or L + 8 > n:
            reads.append(rng.integers(0, 4, L, dtype=np.uint8)); continue
        s = int(rng.integers(0, n - L - 4 + 1)) if rng.random() > 0.05 else n - L   # a few at the very end of the text
        r = text[s:s + L + 4].copy()
        if rng.random() < indel and L > 12:
            p = int(rng.integers(3, L - 3)); g = int(rng.integers(1, 4))
            r = np.concatenate([r[:p], r[p + g:]]) if rng.random() < 0.5 else np.concatenate([r[:p], rng.integers(0, 4, g, dtype=np.uint8), r[p:]])
        r = r[:L].copy()
        if len(r) < L:
            r = np.concatenate([r, rng.integers(0, 4, L - len(r), dtype=np.uint8)])
        m = rng.random(L) < sub
        r[m] = rng.integers(0, 4, int(m.sum()))
        r[rng.random(L) < n_rate] = 4
        reads.append(r)
    return reads


# ---- the restatement against the definitions ----------------------------------------------------
def _check_definitions(idx, read, mems, min_intv, max_intv, min_span, split):
    read = bytes(read)
    L = len(read)
    for x, y, _, flag, b, e in mems:
        assert 0 <= b < e <= L and all(c <= 3 for c in read[b:e])
        assert (x, y) == idx.interval(read[b:e]), "range is not the exact SA interval of its span"
        assert min_intv <= y - x + 1 <= max_intv and e - b >= min_span
        occ = sorted(idx.positions(x, y))
        assert all(idx.t[p:p + e - b] == read[b:e] for p in occ)
        # left-maximal: one more symbol on the left falls below min_intv, or hits an N or the read start
        assert b == 0 or read[b - 1] > 3 or _size(idx.interval(read[b - 1:e])) < min_intv
        # the longest range of a group (flagged; every group keeps it without split and limits) is right-maximal
        if flag and not split and min_span == 1 and max_intv == UNLIMITED:
            assert e == L or read[e] > 3 or _size(idx.interval(read[b:e + 1])) < min_intv
    if not split:
        for i, m in enumerate(mems):                            # no two kept MEMs nested
            for o in mems[i + 1:]:
                assert not (m[4] <= o[4] and o[5] <= m[5]) and not (o[4] <= m[4] and m[5] <= o[5]), (m, o)
    assert [(m[4], m[5]) for m in mems] == sorted((m[4], m[5]) for m in mems)


@pytest.mark.parametrize("seed,n", [(1, 1000), (2, 5000), (3, 20000)])
@pytest.mark.parametrize("min_intv,max_intv,min_span", [(1, UNLIMITED, 1), (2, UNLIMITED, 1), (5, 40, 1), (1, 3, 19), (2, UNLIMITED, 19)])
def test_restatement_meets_the_definitions(seed, n, min_intv, max_intv, min_span):
    rng = np.random.default_rng(seed)
    text = make_text(rng, n)
    idx = NaiveIndex(text)
    reads = make_reads(rng, text, 40, [1, 7, 30, 100])
    reads[0] = np.full(20, 4, np.uint8)                         # all N
    for sid, r in enumerate(reads):
        mems = mem_read(idx, r, sid, min_intv, max_intv, min_span)
        _check_definitions(idx, r, mems, min_intv, max_intv, min_span, False)
        if min_intv == 1 and max_intv == UNLIMITED and min_span == 1 and all(c <= 3 for c in r) and len(r) > 1:
            assert mems, "a read over {0..3} has at least one MEM at min_intv 1"
    assert not mem_read(idx, reads[0], 0)


@pytest.mark.parametrize("seed", [4, 5])
def test_split_restatement_meets_the_definitions(seed):
    """BWA's defaults: split_len 28, split_width 10"""
    rng = np.random.default_rng(seed)
    text = make_text(rng, 8000)
    text[4000:4600] = np.tile(text[100:160], 10)                # many copies of 60 symbols: split candidates with a few occurrences
    idx = NaiveIndex(text)
    reads = make_reads(rng, text, 40, [60, 150], sub=0.005)
    n_split = 0
    for sid, r in enumerate(reads):
        plain = mem_read(idx, r, sid, 1, UNLIMITED, 19)
        mems = mem_read(idx, r, sid, 1, UNLIMITED, 19, 28, 10)
        _check_definitions(idx, r, mems, 1, UNLIMITED, 19, True)
        n_split += plain != mems
    assert n_split > 5


def test_reads_from_the_end_of_the_text_get_exact_ranges():
    """the suffix P$ is part of P's interval: a read that ends where the text ends (the reference's extend_forward leaves it out)"""
    rng = np.random.default_rng(6)
    text = rng.integers(0, 4, 3000, dtype=np.uint8)
    idx = NaiveIndex(text)
    r = text[-50:].copy()
    mems = mem_read(idx, r, 0)
    assert [(m[4], m[5]) for m in mems] == [(0, 50)]
    assert list(idx.positions(mems[0][0], mems[0][1])) == [3000 - 50]


def test_spans_beyond_256_symbols():
    """spans begin past 255: the reference's 8-bit mask of the span begin is not reproduced"""
    rng = np.random.default_rng(7)
    text = rng.integers(0, 4, 20000, dtype=np.uint8)
    idx = NaiveIndex(text)
    r = np.concatenate([text[1000:1300], rng.integers(0, 4, 5, dtype=np.uint8), text[9000:9400]])
    r[300:305] = 4                                               # an N run between the two pieces
    mems = mem_read(idx, r, 0)
    assert [(m[4], m[5]) for m in mems] == [(0, 300), (305, 705)]
    ranges, first, slots = mem_filter(idx, [r])
    assert int(ranges[1, 3]) & 0xFFFF == 305 and int(ranges[1, 3]) >> 16 == 705
    hits = locate(idx, ranges, slots, 0, int(slots[-1]))
    assert [tuple(h) for h in hits] == [(1000, 0, 0, 300), (9000, 0, 305, 705)]


@pytest.mark.parametrize("seed", [8, 9, 10])
def test_host_and_device_discard_agree_for_finite_max_intv(seed):
    """Recorded finding: the host find_kmems moves its left-most marker also for a MEM it then drops for max_intv; the device
    discard_ranges_kernel moves it only for MEMs it keeps.  The kept sets are nevertheless EQUAL (without split): inside a group
    the begins do not increase, and a MEM that begins where a MEM dropped for max_intv begins is a prefix of it, so it has no fewer
    occurrences and is dropped as well.  The restatement pins the device rule; this test shows the two rules agree."""
    rng = np.random.default_rng(seed)
    text = make_text(rng, 6000)
    text[2000:2600] = np.tile(text[10:40], 20)
    idx = NaiveIndex(text)
    reads = make_reads(rng, text, 60, [40, 120], sub=0.01)
    differ = dropped = 0
    for max_intv in (1, 2, 3, 7):
        for sid, r in enumerate(reads):
            dev = mem_read(idx, r, sid, 1, max_intv, 1)
            host = mem_read(idx, r, sid, 1, max_intv, 1, host=True)
            differ += [m[:3] + m[4:] for m in dev] != [m[:3] + m[4:] for m in host]
            dropped += len(mem_read(idx, r, sid)) != len(dev)
    assert dropped > 10                                          # max_intv did drop MEMs
    assert differ == 0


def test_flags_and_order_of_the_output():
    rng = np.random.default_rng(11)
    text = make_text(rng, 4000)
    idx = NaiveIndex(text)
    reads = make_reads(rng, text, 30, [80])
    ranges, first, slots = mem_filter(idx, reads, min_intv=2)
    assert first[0] == 0 and first[-1] == len(ranges) and np.all(np.diff(first.astype(np.int64)) >= 0)
    for sid in range(len(reads)):
        part = ranges[first[sid]:first[sid + 1]]
        assert np.all(part[:, 2] & ~np.uint32(FLAG) == sid)
        if len(part):
            assert np.any(part[:, 2] & np.uint32(FLAG))
    assert slots[-1] == np.sum(ranges[:, 1].astype(np.int64) - ranges[:, 0] + 1)


def test_abi_surface():
    """the library exports the three calls and the Python mirror's parameter struct has the header's layout (5 x uint32, defaults
    of the reference in MEMFilter.rank)"""
    import ctypes
    import inspect

    import __graft_entry__ as ge
    amd = ge.load_package()
    L = amd.lib()
    for name in ("nvbio_mem_filter_temp_bytes", "nvbio_mem_filter_rank", "nvbio_mem_filter_locate"):
        assert hasattr(L, name)
    assert ctypes.sizeof(amd._MemParams) == 20
    d = {k: v.default for k, v in inspect.signature(amd.MEMFilter.rank).parameters.items() if v.default is not inspect.Parameter.empty}
    assert (d["min_intv"], d["max_intv"], d["min_span"], d["split_len"], d["split_width"]) == (1, UNLIMITED, 1, UNLIMITED, UNLIMITED)
