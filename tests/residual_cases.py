"""The named cases the residual-key tests share (test_residual_oracle.py pins the restatement of residual_cpu.py on them and proves that
they are what their names say; test_gpu_residual_edges.py runs nvbio_fm_residual_diagonals and nvbio_fm_filter_scan +
nvbio_fm_filter_locate_diagonals[_ragged] on them): built once from seeded generators, never modified.  Every case carries one line that
says why it is there.

One text of 20,000 symbols: random, with a family of 12 copies of a 200-symbol unit, a family of 70 copies of a 110-symbol unit, and a
period-2 and a period-5 stretch of 400 symbols each.  To the one-call route the ranges are data -- it never looks at the text -- so where a
case needs a range of an exact size, or two seeds with equal diagonals, it writes the range from Text.row or cuts it out of a real one.
Every range keeps x >= 1: row 0, the empty suffix, is outside the contract."""
import functools
from collections import namedtuple

import numpy as np

import approx_cpu as ap
import residual_cpu as rc

POISON = 0xDEADBEEF
N_TEXT = 20000
FAM12, FAM12_UNIT, FAM12_STEP = 1000, 200, 400                      # copies at 1000, 1400, ... 5400
FAM70, FAM70_UNIT, FAM70_STEP = 6000, 110, 150                      # copies at 6000, 6150, ... 16350
PERIOD2, PERIOD5, PERIODIC_LEN = 17000, 17600, 400
SEED = 22
S_BIT = rc.STRAND_BIT

# one call of nvbio_fm_residual_diagonals: entries = ((x, y, id), ...) in the order they are handed over; tags = what the case must show
OC = namedtuple("OC", "name reason entries cap g tags")
# one list of ranges for the two-call route: ids / direct = None or one per range; geoms = (fixed, ragged); windows = ((begin, end), ...)
TC = namedtuple("TC", "name reason ranges ids direct strand geoms windows")

G8 = rc.fixed(8, 10, SEED, 100)                                     # seeds at 0, 10, ... 70
G6 = rc.fixed(6, 15, SEED, 100)                                     # 6 seeds per read: 256 is no multiple of it
G7 = rc.fixed(7, 13, SEED, 100)                                     # an interval that is no multiple of 2 or 5
G1 = rc.fixed(1, 7, SEED, 100)
G_LONG = rc.fixed(9, 128, SEED, 1046)                               # the longest read: the last seed lies 1,024 symbols in


# ---- the text ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def text():
    rng = np.random.default_rng(9100)
    t = rng.integers(0, 4, N_TEXT, dtype=np.uint8)
    unit = rng.integers(0, 4, FAM12_UNIT, dtype=np.uint8)
    for c in range(12):
        t[FAM12 + FAM12_STEP * c:FAM12 + FAM12_STEP * c + FAM12_UNIT] = unit
    unit = rng.integers(0, 4, FAM70_UNIT, dtype=np.uint8)
    for c in range(70):
        t[FAM70 + FAM70_STEP * c:FAM70 + FAM70_STEP * c + FAM70_UNIT] = unit
    t[PERIOD2:PERIOD2 + PERIODIC_LEN] = np.tile(np.array([0, 1], dtype=np.uint8), PERIODIC_LEN // 2)
    t[PERIOD5:PERIOD5 + PERIODIC_LEN] = np.tile(np.array([2, 3, 2, 2, 0], dtype=np.uint8), PERIODIC_LEN // 5)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def scan_text():
    return ap.Text(text())


def copy(d, m, rc_=False):
    """the read that lies at text position d (its reverse complement: it is found on strand 1)"""
    r = text()[d:d + m].copy()
    assert len(r) == m
    return (3 - r[::-1]).astype(np.uint8) if rc_ else r


def junk(rng, m):
    return rng.integers(0, 4, m, dtype=np.uint8)


def in_fam12(c, at=0):
    return FAM12 + FAM12_STEP * c + at


def in_fam70(c, at=0):
    return FAM70 + FAM70_STEP * c + at


def row_at(pos):
    """the one-row range of the suffix that starts at pos"""
    r = int(scan_text().row[pos])
    assert r >= 1
    return r, r


def sized(entry, size):
    """the first `size` rows of an entry's range (none: the empty range at the same x)"""
    x, y, i = entry
    assert size <= rc.size_of(x, y)
    return x, x + size - 1, i


def _unique_places(rng, k, m):
    """k places of m symbols in plain random text (they may overlap each other)"""
    free = np.concatenate([np.arange(0, FAM12 - m, 20), np.arange(16500, PERIOD2 - m, 20), np.arange(18100, N_TEXT - m, 20)])
    return [int(v) for v in rng.permutation(free)[:k]]


# ---- one-call cases ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def one_call_cases():
    rng = np.random.default_rng(9200)
    T = scan_text()
    cs = []

    def add(name, reason, entries, cap, g, *tags):
        cs.append(OC(name, reason, tuple((int(x), int(y), int(i)) for x, y, i in entries), cap, g, frozenset(tags)))

    # -- the cap against ranges below, at and above it
    reads = [copy(in_fam12(3, 20), 100), copy(in_fam70(5, 4), 100), copy(300, 100), junk(rng, 100), copy(in_fam12(7, 50), 100, True),
             copy(in_fam70(9, 2), 100, True)]
    base = rc.seed_entries(T, reads, G8)
    for cap in (1, 2, 4, 63, 64):
        e = list(base)
        for j, size in ((2, cap - 1), (4, cap), (6, cap + 1)):      # three seeds of the read in the 70-copy family, cut to size
            e[1 * 8 + j] = sized(e[1 * 8 + j], size)
        add("cap_%d" % cap, "cap = %d against ranges of 0, 1, 12 and 70 rows and of exactly cap - 1, cap and cap + 1 rows" % cap, e, cap, G8, "cap", "drops")

    # -- empty ranges
    fam = rc.seed_entries(T, [copy(in_fam12(0, 30), 100)], G8, strands=(0,))
    add("empty_alone", "one empty range (x, x - 1) and nothing else: no key, no previous entry", [(fam[0][0], fam[0][0] - 1, 0)], 4, G8, "no_drops", "no_keys")
    add("empty_previous", "an empty range as the previous entry of a seed of the same read: it has no row to compare with, nothing is dropped",
        [sized(fam[3], 0), fam[4]], 4, G8, "no_drops")
    add("short_previous", "the previous entry has 2 rows, this one 12 and cap = 8: rows 0 and 1 are dropped, rows t >= 2 have nothing to compare with",
        [sized(fam[3], 2), fam[4]], 8, G8, "drops", "short_previous")

    # -- the number of entries against the workgroup of 256: entries 255 and 256 are seeds 3 and 4 of read 42, which lies in the 12-copy family
    places = _unique_places(rng, 86, 100)
    reads = []
    for r, d in enumerate(places):
        read = copy(in_fam12(5, 40), 100) if r == 42 else copy(d, 100)
        if r % 2 and r != 42:                                       # every other read with substitutions: some seeds find nothing
            m = rng.random(100) < 0.02
            read[m] = (read[m] + 1 + rng.integers(0, 3, int(m.sum()))) % 4
        reads.append(read)
    many = rc.seed_entries(T, reads, G6, strands=(0,))
    assert len(many) == 516
    add("n_1", "a single entry: no previous entry at all", many[:1], 4, G6, "no_drops")
    add("n_255", "255 entries: one workgroup, its last lane idle", many[:255], 4, G6, "drops")
    add("n_256", "256 entries: exactly one workgroup", many[:256], 4, G6, "drops")
    add("n_257", "257 entries: entry 256 opens the second workgroup and is a duplicate of entry 255 in the first", many[:257], 4, G6, "drops", "block_boundary")
    add("n_513", "513 entries: three workgroups, the duplicate of entry 256 has its source in the previous one", many[:513], 4, G6, "drops", "block_boundary")
    add("ids_permuted", "the 513 entries handed over in a random order: the call sorts them by id itself", [many[i] for i in rng.permutation(513)], 4, G6,
        "drops", "block_boundary", "permuted")

    # -- strands
    d = 16600
    hand = [row_at(d + 10 * j) + (2 * 8 + j,) for j in range(8)] + [row_at(d + 100 - 10 * j - SEED) + ((2 * 8 + j) | S_BIT,) for j in range(8)]
    both = rc.seed_entries(T, [copy(in_fam12(2, 10), 100), copy(in_fam70(30, 3), 100, True)], G8) + hand
    add("both_strands", "both strands in one call: reads found forwards and backwards, and a read whose two strands lie on one diagonal; its entries with "
        "and without bit 31 sort far apart and are never compared", [both[i] for i in rng.permutation(len(both))], 4, G8, "drops", "both_strands")
    one = [row_at(d + 10 * j) + (j,) for j in range(8)] + [row_at(d + 100 - 10 * j - SEED) + (j | S_BIT,) for j in range(8)]
    add("one_read_both_strands", "one read alone, both strands on one diagonal: its last forward seed and its first reverse seed are neighbours with equal "
        "diagonal fields, and differ in the strand only", one, 4, G8, "drops", "strand_neighbours")
    add("read_boundary", "the last seed of read 0 and the first seed of read 1 have equal diagonal fields: another read, nothing is dropped",
        [row_at(d + 70) + (7,), row_at(d) + (8,)], 4, G8, "no_drops", "equal_fields")
    same = [copy(in_fam12(4, 60), 100)] * 6 + [copy(500, 100)] * 3
    add("one_seed_per_read", "seeds_per_read = 1 over identical reads: every previous entry is another read, nothing is ever dropped",
        rc.seed_entries(T, same, G1), 4, G1, "no_drops")

    # -- repeats
    add("family_12", "a read inside the dispersed 12-copy family, cap = 12: every seed lists the copies in one order, chains of duplicates, one key per row",
        rc.seed_entries(T, [copy(in_fam12(6, 30), 100)], G8, strands=(0,)), 12, G8, "drops", "one_per_row")
    add("family_12_cap_64", "the same with cap = 64 above every range", rc.seed_entries(T, [copy(in_fam12(6, 30), 100)], G8, strands=(0,)), 64, G8,
        "drops", "one_per_row")
    add("family_70", "a read inside the 70-copy family on the reverse strand, cap = 64 below the ranges: one key per row of the cap",
        rc.seed_entries(T, [copy(in_fam70(33, 5), 100, True)], G8, strands=(1,)), 64, G8, "drops", "one_per_row")
    add("period_2", "a read in period-2 text with seeds every 13 symbols: neighbouring seeds list the copies shifted, duplicates survive",
        rc.seed_entries(T, [copy(PERIOD2 + 101, 100)], G7, strands=(0,)), 64, G7, "periodic")
    add("period_5", "a read in period-5 text with seeds every 13 symbols: the same with five phases",
        rc.seed_entries(T, [copy(PERIOD5 + 52, 100), copy(PERIOD5 + 131, 100, True)], G7), 64, G7, "periodic")

    # -- the ends of the text
    over = [np.concatenate([junk(rng, k), copy(0, 100 - k)]) for k in (5, 37)]       # reads that hang 5 and 37 symbols over the text start
    ends = rc.seed_entries(T, over + [copy(N_TEXT - 100, 100)], G8) + [row_at(N_TEXT - 1) + (3 * 8 + 2,), row_at(0) + (3 * 8 + 5,)]
    add("text_ends", "hits within the seed's offset of the text start (the field falls below the bias of 1,024), a read at the text's end, and one-row "
        "ranges that hold the first and the last text position", ends, 4, G8, "drops", "text_start")
    add("long_read", "reads of 1,046 symbols, the last seed 1,024 symbols in: a read at position 0 (every field exactly the bias) and one on strand 1",
        rc.seed_entries(T, [copy(0, 1046), copy(2000, 1046, True)], G_LONG), 4, G_LONG, "drops", "field_at_bias")

    # -- ragged reads
    lengths = [30, 31, 57, 100, 200, 64, 199, 30]
    gr = rc.ragged(4, SEED, lengths, [2, 3, 11, 26, 59, 14, 50, 1])
    where = [in_fam12(1, 9), 700, in_fam70(2, 11), in_fam70(3, 1), in_fam12(8, 0), 16700, 18200, in_fam12(9, 150)]
    reads = [copy(p, m, r % 2 == 1) for r, (p, m) in enumerate(zip(where, lengths))]
    rag = rc.seed_entries(T, reads, gr)
    add("ragged", "reads of 30 to 200 symbols with their own seed intervals: reverse-strand offsets come from each read's own length",
        [rag[i] for i in rng.permutation(len(rag))], 4, gr, "drops", "ragged")
    return tuple(cs)


# ---- the large one-call case ------------------------------------------------------------------------------------------------------
G_LARGE = rc.fixed(4, 20, SEED, 100)
LARGE_N = 8192 * 256 + 300                                          # the launch is capped at 8,192 workgroups: the loop over entries wraps


@functools.lru_cache(maxsize=None)
def large_case():
    """8,192 x 256 + 300 entries, cap = 1, four seeds per read on one-row ranges: most reads lie on one diagonal (a chain of three
    duplicates), every eleventh on four unrelated rows, every fifth read is a reverse-strand one, and every 37th entry is emptied, which
    breaks its chain.  -> (x, y, ids) as handed over: permuted"""
    T, g = scan_text(), G_LARGE
    assert LARGE_N % g.spr == 0
    sid = np.arange(LARGE_N, dtype=np.int64)
    rid, j = sid // g.spr, sid % g.spr
    strand = (rid % 5 == 0).astype(np.int64)
    off = np.where(strand == 1, g.read_len - j * g.interval - g.seed_len, j * g.interval)
    pos = (rid * 7919) % (N_TEXT - 100) + off
    stray = rid % 11 == 3
    pos = np.where(stray, (rid * 104729 + 4001 * j * j + 17 * j) % (N_TEXT - 1), pos)
    x = T.row[pos]
    assert x.min() >= 1
    y = np.where(sid % 37 == 5, x - 1, x)
    ids = sid | (strand << 31)
    p = np.random.default_rng(9300).permutation(LARGE_N)
    return x[p], y[p], ids[p]


# ---- two-call cases ---------------------------------------------------------------------------------------------------------------
TILE = 2048                                                         # outputs per tile of the expansion


def _windows(total):
    w = [(0, total), (0, 1), (total - 1, total)]
    for b in (0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1):       # windows that start and end one before, on and one after multiples of 2,048
        for e in (TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, b + TILE - 1, b + TILE, b + TILE + 1, 3 * TILE - 1, 3 * TILE, 3 * TILE + 1):
            if b < e <= total:
                w.append((b, e))
    return tuple(sorted(set(w)))


@functools.lru_cache(maxsize=None)
def two_call_cases():
    rng = np.random.default_rng(9400)
    T = scan_text()
    strip = lambda es: [(x, y) for x, y, _ in es]
    fam12 = strip(rc.seed_entries(T, [copy(in_fam12(2, 10), 100)], G8, strands=(0,)))
    fam70 = strip(rc.seed_entries(T, [copy(in_fam70(c, 3), 100) for c in (4, 40, 66)], G8, strands=(0,)))
    uniq = strip(rc.seed_entries(T, [copy(d, 100) for d in _unique_places(rng, 5, 100)], G8, strands=(0,)))
    assert all(y - x == 11 for x, y in fam12) and all(y - x == 69 for x, y in fam70) and all(x == y for x, y in uniq)
    ranges = [rc.EMPTY] * 3 + fam12 + [(100, 5099)] + [(7, 6)] * 5                  # empty ranges in front; a range of 5,000 rows over three tiles
    for k in range(3):                                              # one-row ranges between walked ones, in the same tile
        ranges += fam70[8 * k:8 * k + 8] + uniq[13 * k:13 * k + 13] + [rc.EMPTY]
    ranges += uniq[39:] + [rc.EMPTY] * 4                            # ... and empty ranges at the end
    n = len(ranges)
    total = int(rc.inclusive_sizes(ranges)[-1])
    assert total > 3 * TILE + 1
    reads = 40                                                      # seed ids of the compacted cases reach up to 40 reads

    def geoms():
        lengths = rng.integers(92, 201, reads)
        return (G8, rc.ragged(8, SEED, lengths, (lengths - SEED) // 7 - rng.integers(0, 3, reads)))

    cs = []

    def add(name, reason, rg, ids, direct, strand, windows):
        cs.append(TC(name, reason, tuple(rg), None if ids is None else tuple(int(i) for i in ids), None if direct is None else tuple(direct), strand, geoms(),
                     windows))

    add("plain", "range i is seed i, strand 0: the whole list, single outputs, windows around multiples of 2,048, a range over three tiles, runs of empty "
        "ranges at the front, in the middle and at the end", ranges, None, None, 0, _windows(total))
    add("plain_strand_1", "the same on strand 1: every offset is taken from the read's end", ranges, None, None, 1, ((0, total), (TILE - 1, 2 * TILE + 1)))
    ids = np.sort(rng.permutation(reads * 8)[:n]) | (rng.integers(0, 2, n) << 31)
    assert len(set((ids >> 31).tolist())) == 2
    add("ids_strand_0", "query_ids as a compacted subset of the seeds, bit 31 set on about half of them, base strand 0", ranges, ids, None, 0,
        ((0, total), (1, TILE + 1), (TILE, 3 * TILE)))
    add("ids_strand_1", "the same ids with base strand 1: bit 31 flips it back to 0", ranges, ids, None, 1, ((0, total), (TILE + 1, 2 * TILE - 1)))
    one_row = [i for i, (x, y) in enumerate(ranges) if x == y]
    direct = [0] * n
    with_pos = list(ranges)
    for i in one_row[::2]:                                          # every other one-row range holds its text position instead of its row
        direct[i] = 1
        with_pos[i] = (int(T.sa[ranges[i][0]]),) * 2
    add("direct", "direct flags on every other one-row range, between walked ranges in the same tile: such a range holds a text position", with_pos, None,
        direct, 0, ((0, total), (3 * TILE - 1, total), (TILE + 1, 3 * TILE + 1)))
    add("direct_ids", "direct flags and compacted ids with both strands in one call", with_pos, ids, direct, 1, ((0, total), (TILE, 2 * TILE)))
    add("single_output", "one one-row range: a single output", [row_at(12345)], None, None, 0, ((0, 1),))
    return tuple(cs)


def plain_of(case):
    """the ranges of a case with direct flags as plain rows"""
    T = scan_text()
    return tuple((int(T.row[x]),) * 2 if (case.direct is not None and case.direct[i]) else (x, y) for i, (x, y) in enumerate(case.ranges))
