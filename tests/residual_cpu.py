"""A plain restatement of the two routes that turn residual seeds -- searches that end on several suffix-array rows -- into diagonal keys:
the two-call route (nvbio_fm_filter_scan + nvbio_fm_filter_locate_diagonals[_ragged]) and the one-call route (nvbio_fm_residual_diagonals).
It knows the text, a plain suffix array (approx_cpu.Text: prefix doubling, row 0 the empty suffix) and the key rule
(selection_cpu.hit_to_diagonal); it knows no FM index: no BWT, no rank, no LF walk, no sampled suffix array.  A seed's rows are found by
scanning the text.  Both routes are written from their rules in include/nvbio_amd.h, not from the kernels.

A geometry says how a seed id becomes a read and an offset: seeds_per_read and seed_len for every read, one seed_interval and read_len
(fixed) or every read's own length and interval (ragged: read_offsets [R + 1] and intervals [R]).  An entry is (x, y, id): the closed
row range [x, y] (empty when y = x - 1) and the 32-bit seed id, bit 31 = the other strand."""
from collections import Counter, namedtuple

import numpy as np

import selection_cpu as sel

Geometry = namedtuple("Geometry", "spr interval seed_len read_len read_offsets intervals")
STRAND_BIT = 1 << 31
EMPTY = (1, 0)                                                      # what a search that finds nothing leaves


def fixed(spr, interval, seed_len, read_len):
    assert (spr - 1) * interval + seed_len <= read_len and read_len - seed_len <= sel.MAX_SEED_OFFSET
    return Geometry(spr, interval, seed_len, read_len, None, None)


def ragged(spr, seed_len, lengths, intervals):
    lengths, intervals = [int(v) for v in lengths], [int(v) for v in intervals]
    assert len(lengths) == len(intervals)
    assert all((spr - 1) * s + seed_len <= m and m - seed_len <= sel.MAX_SEED_OFFSET for m, s in zip(lengths, intervals))
    return Geometry(spr, None, seed_len, None, np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32), np.asarray(intervals, dtype=np.uint32))


def read_shape(g, rid):
    """(seed interval, length) of read rid"""
    if g.read_offsets is None:
        return g.interval, g.read_len
    return int(g.intervals[rid]), int(g.read_offsets[rid + 1]) - int(g.read_offsets[rid])


def key_of(pos, id32, g, strand=0):
    """the diagonal key of a hit at text position pos of the seed with the 32-bit id: bit 31 flips `strand`"""
    sid = id32 & (STRAND_BIT - 1)
    s, m = read_shape(g, sid // g.spr)
    return sel.hit_to_diagonal(int(pos), sid, g.spr, s, g.seed_len, m, (strand ^ (id32 >> 31)) & 1)


def size_of(x, y):
    return (1 + y - x) & 0xFFFFFFFF


# ---- seeds to rows ----------------------------------------------------------------------------------------------------------------
def rows_of(text, string):
    """the closed interval of rows whose suffixes start with `string`, found by comparing it with every window of the text; EMPTY if none"""
    string = np.asarray(string, dtype=np.uint8)
    w = text.windows(len(string))
    at = np.nonzero((w == string[None, :]).all(axis=1))[0] if len(w) else np.zeros(0, np.int64)
    if len(at) == 0:
        return EMPTY
    r = text.row[at]
    lo, hi = int(r.min()), int(r.max())
    assert hi - lo + 1 == len(at), "the rows of one string are not an interval"
    return lo, hi


def seed_entries(text, reads, g, strands=(0, 1)):
    """(x, y, id) of every seed of every read, strand by strand: strand 0 asks the text for the seed, strand 1 for its reverse complement
    (id | bit 31).  reads: one array of symbols per read, as long as the geometry says."""
    out = []
    for strand in strands:
        for rid, read in enumerate(reads):
            s, m = read_shape(g, rid)
            assert len(read) == m
            for j in range(g.spr):
                seed = np.asarray(read[j * s:j * s + g.seed_len], dtype=np.uint8)
                x, y = rows_of(text, (3 - seed[::-1]) if strand else seed)
                out.append((x, y, (rid * g.spr + j) | (STRAND_BIT if strand else 0)))
    return out


# ---- the two-call route -----------------------------------------------------------------------------------------------------------
def inclusive_sizes(ranges):
    """nvbio_fm_filter_scan: the running sums of the range sizes"""
    return np.cumsum([size_of(x, y) for x, y in ranges], dtype=np.uint64) if len(ranges) else np.zeros(0, np.uint64)


def two_call_keys(text, ranges, ids, direct, strand, g):
    """every output of the two-call route, in order: output h belongs to range i = upper_bound(inclusive sizes, h), its row is
    x_i + (h - the outputs before range i), its position sa[row] -- or x_i itself where direct[i] is set (a one-row range that already
    holds its text position) -- and its seed id ids[i] (i where ids is None); bit 31 of the id flips `strand`."""
    slots = [int(v) for v in inclusive_sizes(ranges)]
    out = []
    for h in range(slots[-1] if slots else 0):
        i = 0
        while slots[i] <= h:                                        # upper_bound, the slow way
            i += 1
        base = slots[i - 1] if i else 0
        row = ranges[i][0] + (h - base)
        pos = row if (direct is not None and direct[i]) else int(text.sa[row])
        out.append(key_of(pos, i if ids is None else int(ids[i]), g, strand))
    return out


def capped(entries, cap):
    """the ranges with at most their first cap rows"""
    return [(x, min(y, x + cap - 1)) if size_of(x, y) else (x, y) for x, y, _ in entries]


# ---- the one-call route -----------------------------------------------------------------------------------------------------------
def one_call_keys(text, entries, cap, g):
    """nvbio_fm_residual_diagonals by its rule: the entries in ascending order of the 32-bit id (strand bit included), the first
    min(size, cap) rows of each range, and a key dropped iff the previous entry belongs to the same read and strand, has a row t, and
    leaves the same key there.  -> (Counter of the keys written, number dropped)"""
    assert 1 <= cap <= 64
    order = sorted(entries, key=lambda e: e[2])                     # (stable, like the radix sort)
    kept, dropped = Counter(), 0
    prev = None                                                     # (read, strand, keys row by row) of the previous entry
    for x, y, id32 in order:
        rows = min(size_of(x, y), cap)
        keys = [key_of(text.sa[x + t], id32, g) for t in range(rows)]
        who = ((id32 & (STRAND_BIT - 1)) // g.spr, id32 >> 31)
        for t, k in enumerate(keys):
            if prev is not None and prev[:2] == who and t < len(prev[2]) and prev[2][t] == k:
                dropped += 1
            else:
                kept[k] += 1
        prev = who + (keys,)
    return kept, dropped


def one_call_keys_cap1(text, x, y, ids, g):
    """one_call_keys for cap = 1 and a fixed geometry over arrays (x, y, ids: one entry each) -> (sorted uint64 keys, number dropped)"""
    assert g.read_offsets is None
    x, y, ids = (np.asarray(a, dtype=np.int64) for a in (x, y, ids))
    order = np.argsort(ids, kind="stable")
    x, y, ids = x[order], y[order], ids[order]
    has = y >= x                                                    # one row, row 0 of the range, where the range is not empty
    sid, strand = ids & (STRAND_BIT - 1), ids >> 31
    rid = sid // g.spr
    off = (sid % g.spr) * g.interval
    off = np.where(strand == 1, g.read_len - off - g.seed_len, off)
    field = text.sa[np.where(has, x, 0)].astype(np.int64) - off + sel.BIAS
    assert ((field >= 0) & (field <= sel.FIELD))[has].all()
    key = (rid.astype(np.uint64) << np.uint64(34)) | (strand.astype(np.uint64) << np.uint64(33)) | field.astype(np.uint64)
    dup = np.zeros(len(ids), dtype=bool)
    dup[1:] = has[1:] & has[:-1] & (rid[1:] == rid[:-1]) & (strand[1:] == strand[:-1]) & (key[1:] == key[:-1])
    return np.sort(key[has & ~dup]), int(dup.sum())
