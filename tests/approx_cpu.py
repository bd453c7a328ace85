"""Plain references for the two approximate FM-index searches (nvbio_fm_hamming_backtrack and nvbio_seed_hits_map_approx) that know nothing
about FM indices: no BWT, no rank, no backward-search recurrence.  A string is found by scanning the text; a suffix array made by plain prefix
doubling turns the places where it occurs into rows.  Row 0 is the empty suffix, so the rows of a string w are the ranks (1-based) of the
suffixes that start with w, and because the suffixes are sorted they form one interval.  NumPy only.

The only thing taken from the searches themselves is their specification: which strings a search accepts (backtrack.h:51-157,
mapping_inl.h:114-184), the four searches of a seed with their len1 and flags (mapping_inl.h:325-345), and that a backward search over
query[0], query[1], ... finds the text string query[len-1] ... query[1] query[0]."""
import numpy as np

STACK_ENTRIES = 128                       # count_core's stack (nvbio-test/fmindex_test.cu:757), BACKTRACK_STACK in csrc/fm_index.hip


# ---- strings to rows --------------------------------------------------------------------------------------------------------------
def suffix_array(text):
    """rows of the sorted suffixes of text, the empty suffix first: sa[0] = n -> uint32 [n + 1].  Prefix doubling over plain ranks."""
    text = np.asarray(text, dtype=np.int64)
    n = len(text)
    if n == 0:
        return np.zeros(1, dtype=np.uint32)
    rank = np.concatenate([text + 1, [0]])                          # the empty suffix sorts below every symbol
    k = 1
    while True:
        nxt = np.zeros(n + 1, dtype=np.int64)
        if k <= n:
            nxt[:n + 1 - k] = rank[k:] + 1                          # suffixes shorter than k keep 0, below every rank + 1
        order = np.lexsort((nxt, rank))
        key = rank[order] * (n + 8) + nxt[order]
        new = np.zeros(n + 1, dtype=np.int64)
        new[order] = np.concatenate([[0], np.cumsum(key[1:] != key[:-1])])
        rank = new
        if rank.max() == n:
            return np.argsort(rank).astype(np.uint32)
        k *= 2


class Text:
    """a text, its suffix array and the row of every suffix; interval tables per string length, made on demand"""

    def __init__(self, text):
        self.text = np.ascontiguousarray(text, dtype=np.uint8)
        assert self.text.size == 0 or self.text.max() < 4
        self.n = len(self.text)
        self.sa = suffix_array(self.text)
        self.row = np.empty(self.n + 1, dtype=np.int64)             # row[p] = the row of the suffix that starts at p
        self.row[self.sa] = np.arange(self.n + 1)
        self._tables = {}

    def windows(self, m):
        """every length-m window of the text, [n - m + 1, m] (none if m > n)"""
        if m > self.n:
            return np.zeros((0, m), dtype=np.uint8)
        if m == 0:
            return np.zeros((self.n + 1, 0), dtype=np.uint8)
        return np.lib.stride_tricks.sliding_window_view(self.text, m)

    def intervals_of(self, positions, m):
        """the places `positions` where length-m strings occur, grouped by string -> [(lo, hi)] one SA interval per distinct string.
        Checks that each string's rows are a full interval (all its occurrences were given)."""
        positions = np.asarray(positions, dtype=np.int64)
        if len(positions) == 0:
            return []
        if m == 0:
            return [(0, self.n)]
        w = self.windows(m)[positions]
        _, inv = np.unique(w, axis=0, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        rows = self.row[positions]
        out = []
        for g in range(int(inv.max()) + 1):
            r = rows[inv == g]
            lo, hi = int(r.min()), int(r.max())
            assert hi - lo + 1 == len(r), "the rows of one string are not an interval"
            out.append((lo, hi))
        return out

    def table(self, m):
        """every distinct length-m string of the text (1 <= m <= 32) as a 2-bit big-endian key -> (sorted keys uint64, lo, hi)"""
        if m not in self._tables:
            assert 1 <= m <= 32
            w = self.windows(m).astype(np.uint64)
            key = np.zeros(len(w), dtype=np.uint64)
            for j in range(m):
                key = (key << np.uint64(2)) | w[:, j]
            keys, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
            inv = np.asarray(inv).reshape(-1)
            rows = self.row[:len(w)]
            lo = np.full(len(keys), self.n + 1, dtype=np.int64)
            hi = np.full(len(keys), -1, dtype=np.int64)
            np.minimum.at(lo, inv, rows)
            np.maximum.at(hi, inv, rows)
            assert np.array_equal(hi - lo + 1, cnt), "the rows of one string are not an interval"
            self._tables[m] = (keys, lo, hi)
        return self._tables[m]

    def interval(self, string):
        """(lo, hi) of one string of symbols 0..3 (1..32 of them), or None if the text does not hold it"""
        keys, lo, hi = self.table(len(string))
        k = 0
        for c in string:
            k = (k << 2) | int(c)
        i = int(np.searchsorted(keys, np.uint64(k)))
        if i < len(keys) and int(keys[i]) == k:
            return int(lo[i]), int(hi[i])
        return None


# ---- hamming_backtrack ------------------------------------------------------------------------------------------------------------
def backtrack_scan(text, query, seed, mismatches):
    """every place of the text where `query` occurs with its last min(seed, len) symbols exact and at most `mismatches` mismatches in
    all; a query symbol above 3 mismatches every text symbol; mismatches == 0 or seed >= len: exact.
    text: a Text -> (count, n_ranges, set of (lo, hi)): count = the places, one range per distinct matching string."""
    query = np.asarray(query, dtype=np.uint8)
    m = len(query)
    if m == 0:
        return text.n + 1, 1, {(0, text.n)}                         # the empty string starts every suffix, the empty one included
    seed = min(seed, m)
    if mismatches == 0 or seed == m:
        seed, mismatches = m, 0
    w = text.windows(m)
    if len(w) == 0:
        return 0, 0, set()
    diff = w != query[None, :]                                      # (a symbol above 3 differs from every text symbol)
    ok = diff.sum(axis=1) <= mismatches
    if seed:
        ok &= ~diff[:, m - seed:].any(axis=1)
    pos = np.nonzero(ok)[0]
    ranges = text.intervals_of(pos, m)
    assert sum(hi - lo + 1 for lo, hi in ranges) == len(pos)
    rs = set(ranges)
    assert len(rs) == len(ranges)
    return len(pos), len(ranges), rs


def backtrack_stack_peak(text, query, seed, mismatches):
    """a model of hamming_backtrack's walk (backtrack.h:78-157, default mode) that keeps strings where the walk keeps ranges: the node of
    a string exists iff the text holds the string.  -> the highest number of entries the stack would hold if it had no bound (an entry
    counts from its push), or 0 where the walk never starts.  text: uint8 symbols."""
    tb = bytes(np.asarray(text, dtype=np.uint8))
    q = [int(c) for c in query]
    m = len(q)
    seed = min(seed, m)
    if mismatches == 0 or seed == m:
        return 0
    root = bytes(q[m - seed:])
    if any(c > 3 for c in root) or root not in tb:
        return 0
    stack, peak = [], 0

    def push_children(s, cost, l):
        nonlocal peak
        for c in range(4):
            child = bytes([c]) + s
            if child in tb:
                stack.append((child, cost + (0 if c == q[l - 1] else 1), l - 1))
                peak = max(peak, len(stack))
    push_children(root, 0, m - seed)
    while stack:
        s, cost, l = stack.pop()
        if l == 0:
            continue
        if cost < mismatches:
            push_children(s, cost, l)
    return peak


# ---- seed_mapper<APPROX_MAPPING> --------------------------------------------------------------------------------------------------
def seed_searches(stored, read_len, pos, seed_len):
    """the four searches of the seed at `pos` of a stored read (mapping_inl.h:325-345)
    -> [(reversed text?, query, len1, check exact?, flags)]; flags = position:10 << 20 | complement << 30 | reverse index << 31"""
    fq = [int(c) for c in stored[pos:pos + seed_len]]
    rq = fq[::-1]
    comp = lambda q: [3 - c if c < 4 else c for c in q]
    half, half_up = seed_len // 2, (seed_len + 1) // 2
    F = lambda p, rc, rev: ((p & 0x3FF) << 20) | (rc << 30) | (rev << 31)
    return [(False, fq, half, True, F(read_len - pos - seed_len, 0, 0)),
            (True, rq, half_up, False, F(read_len - pos - 1, 0, 1)),
            (True, comp(fq), half, True, F(pos + seed_len - 1, 1, 1)),
            (False, comp(rq), half_up, False, F(pos, 1, 0))]


def search_hits(text, query, len1, check_exact, flags):
    """one search: every string that differs from the query in exactly one position, that position in [len1, len), and the query itself
    where check_exact; each string the text holds gives one hit (range begin, size | flags).  The backward search turns the query round,
    so the text is asked for the reversed string.  -> (hits, sum of sizes)"""
    L = len(query)
    cands = []
    for j in range(len1, L):
        for sub in range(4):
            if sub != query[j]:
                cands.append(query[:j] + [sub] + query[j + 1:])
    if check_exact:
        cands.append(list(query))
    hits, total = [], 0
    for s in cands:
        if max(s) > 3:
            continue
        iv = text.interval(s[::-1])
        if iv is not None:
            size = iv[1] - iv[0] + 1
            assert size < (1 << 20)
            hits.append((iv[0], size | flags))
            total += size
    return hits, total


def map_approx_scan(fwd, rev, stored_read, params):
    """one read: fwd / rev = the Text of the text and of the reversed text; stored_read = the read as nvBowtie stores it (reversed);
    params = dict(seeds_per_read, first_offset, seed_interval, seed_len, read_len, rep_seeds)
    -> (sorted list of (range begin, size | flags) over the four searches of every seed, range_sum, range_count, reseed)"""
    hits, range_sum = [], 0
    for j in range(params["seeds_per_read"]):
        pos = params["first_offset"] + j * params["seed_interval"]
        assert pos + params["seed_len"] <= params["read_len"]
        for reverse, query, len1, exact, flags in seed_searches(stored_read, params["read_len"], pos, params["seed_len"]):
            h, s = search_hits(rev if reverse else fwd, query, len1, exact, flags)
            hits += h
            range_sum += s
    range_count = len(hits)
    reseed = range_count == 0 or (range_sum & 0xFFFFFFFF) >= ((params["rep_seeds"] * range_count) & 0xFFFFFFFF)
    return sorted(hits), range_sum, range_count, reseed
