"""The named cases the approximate-search tests share (test_approx_oracle.py pins the oracle on them against the text scans of approx_cpu.py,
test_gpu_approx_edges.py runs the kernels on them): built once from seeded generators, never modified.  Every case carries one line that says why
it is there.

Every text is far below 2^20 symbols, so no range reaches the 20-bit size field of a seed hit (seed_hit.h:217): the largest has 60,000."""
import functools
from collections import namedtuple

import numpy as np

import approx_cpu as ap

T_, A_, C_, N_ = 3, 0, 1, 4
STACK_SEED = 16
POISON = 0xDEADBEEF

# one hamming_backtrack call: queries = the strings, laid out back to back after `lead` symbols of lead-in; max_ranges: a number, "one" or
# "most-1" (one below the largest n_ranges of the set)
BT = namedtuple("BT", "name reason text queries seed mm lead quirks max_ranges family")
# one map_approx call: reads = the stored (reversed) reads [R, read_len]; p = the seed parameters; queue = None or the read ids to map
MP = namedtuple("MP", "name reason text reads p max_hits queue family")


# ---- texts ------------------------------------------------------------------------------------------------------------------------
def de_bruijn(k):
    """a text of 4^k + k - 1 symbols that holds every k-mer once"""
    a, seq = [0] * (4 * k), []

    def db(t, p):
        if t > k:
            if k % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, 4):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return np.array(seq + seq[:k - 1], dtype=np.uint8)


def _poly_t(d_run=200):
    rng = np.random.default_rng(7001)
    return np.concatenate([rng.integers(0, 4, 1500), [A_], [T_] * d_run, [C_], rng.integers(0, 4, 1500)]).astype(np.uint8)


def _tandem(period, seed):
    rng = np.random.default_rng(seed)
    unit = rng.permutation(4)[:period]
    pure = np.tile(unit, 120 // period + 1)[:120]
    worn = np.tile(unit, 240 // period + 1)[:240]                  # the same repeat with a substitution every 5 to 13 symbols: sibling strings
    at = np.cumsum(rng.integers(5, 14, 40))
    at = at[at < 240]
    worn[at] = (worn[at] + 1 + rng.integers(0, 3, len(at))) % 4
    return np.concatenate([pure, worn]).astype(np.uint8)


def _with_repeat(n, seed):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 4, n, dtype=np.uint8)
    t[1000:1400] = np.tile(t[1000:1010], 40)                       # a period-10 tandem repeat
    t[1200] = (t[1200] + 1) % 4                                    # ... with one copy that differs
    return t


@functools.lru_cache(maxsize=None)
def text(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "poly_t":
        return _poly_t()
    if name.startswith("rand"):
        return rng.integers(0, 4, int(name[4:]), dtype=np.uint8)
    if name.startswith("period"):
        return _tandem(int(name[6:]), 7100 + int(name[6:]))
    if name == "two_letter":
        return (rng.integers(0, 2, 300) * 2 + 1).astype(np.uint8)     # C and T only
    if name == "m3k":
        return _with_repeat(3000, 7200)
    if name == "m60k":
        return _with_repeat(60000, 7201)
    if name == "every4mer":
        return de_bruijn(4)                                         # 259 symbols
    if name == "t70":
        return np.concatenate([de_bruijn(3), rng.integers(0, 4, 4)]).astype(np.uint8)      # 70 symbols, every 3-mer
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def scan_text(name, reverse=False):
    t = text(name)
    return ap.Text(t[::-1].copy() if reverse else t)


# ---- backtrack cases --------------------------------------------------------------------------------------------------------------
def _copies(rng, t, n, length, sub, keep_last=0, ends=True):
    """n queries copied from t, substitutions at rate `sub` outside their last keep_last symbols; the first two from both ends of the text"""
    out = []
    for i in range(n):
        s = int(rng.integers(0, len(t) - length + 1))
        if ends and i == 0:
            s = 0
        if ends and i == 1:
            s = len(t) - length
        q = t[s:s + length].copy()
        m = rng.random(length) < sub
        m[length - keep_last:] = False
        q[m] = (q[m] + 1 + rng.integers(0, 3, int(m.sum()))) % 4
        out.append(q.astype(np.uint8))
    return out


def poly_t_query(d):
    return np.full(STACK_SEED + d, T_, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def backtrack_cases():
    rng = np.random.default_rng(7300)
    cs = []

    def add(name, reason, text_name, queries, seed, mm, lead=0, quirks=False, max_ranges=64, family="limits"):
        cs.append(BT(name, reason, text_name, tuple(np.asarray(q, dtype=np.uint8) for q in queries), seed, mm, lead, quirks, max_ranges, family))

    add("stack_full", "poly-T query of 16 + 127 in a T^200 run: the stack peaks at exactly 128 entries and nothing overflows",
        "poly_t", [poly_t_query(127), poly_t_query(4), poly_t_query(100), poly_t_query(126)], STACK_SEED, 1, family="stack")
    r3 = text("rand3000")
    add("seed_len_minus_1", "seed = len - 1: one position may differ, the root is the stack's only level", "rand3000", _copies(rng, r3, 40, 24, 0.04, 0), 23, 2)
    add("seed_0", "seed = 0: the walk starts from the whole index, rank4 at row -1", "rand3000",
        _copies(rng, r3, 30, 12, 0.05) + _copies(rng, r3, 30, 5, 0.1) + _copies(rng, r3, 10, 7, 0.1), 0, 1)
    add("seed_0_mm2", "seed = 0 with two mismatches on short strings: many ranges from the whole index", "rand3000", _copies(rng, r3, 30, 6, 0.1), 0, 2,
        max_ranges=160)
    add("seed_above_len", "seed > len: the search is exact", "rand3000", _copies(rng, r3, 40, 24, 0.02), 40, 2)
    add("mismatches_0", "mismatches = 0: the search is exact whatever the seed", "rand3000", _copies(rng, r3, 40, 24, 0.02), 8, 0)
    for length in (4, 5):
        for mm in (length, length + 1):
            add("all_%dmers_mm%d" % (length, mm), "mismatches >= len with seed = 0: every %d-mer of the text, count n - len + 1" % length, "rand3000",
                _copies(rng, r3, 3, length, 0.5), 0, mm, max_ranges=1024, family="all_lenmers")
    add("short_queries", "queries of length 0, 1 and 2: the exact route for the empty string, a walk of one and two levels", "rand3000",
        [[], [0], [3], [1, 2], [3, 3], [], [2]], 0, 1, max_ranges=16)
    add("short_queries_seed1", "lengths 0, 1, 2 with seed 1: length 1 is all seed, length 2 leaves one free symbol", "rand3000",
        [[], [0], [3], [1, 2], [3, 3], [], [2]], 1, 1, max_ranges=16)
    base = _copies(rng, r3, 12, 20, 0.0)
    def with_n(qs, where):
        out = []
        for q in qs:
            q = q.copy()
            q[where] = N_
            out.append(q)
        return out
    add("n_in_seed", "an N in the seed part: nothing matches", "rand3000", with_n(base, [15]) + with_n(base, [19]) + base[:2], 8, 2, family="n")
    add("n_outside_seed", "an N outside the seed costs one mismatch: four strings per N", "rand3000",
        with_n(base, [3]) + with_n(base, [0]) + with_n(base, [11]) + with_n(base, [2, 9]) + with_n(base, [1, 5, 7]), 8, 2, family="n")
    add("all_n", "a query of N's only: nothing with a seed, every string with seed = 0 and mismatches = len", "rand3000",
        [np.full(4, N_), np.full(3, N_), np.full(1, N_)], 0, 4, max_ranges=300, family="n")
    add("all_n_seeded", "a query of N's only, with a seed: nothing", "rand3000", [np.full(6, N_), np.full(2, N_)], 2, 3, family="n")
    for name in ("period1", "period2", "period3", "period4", "two_letter"):
        t = text(name)
        for mm in (2, 3):
            add("%s_mm%d" % (name, mm), "low-complexity text, %d mismatches: many sibling ranges, deep ties" % mm, name, _copies(rng, t, 16, 14, 0.12, 4), 4, mm,
                max_ranges=512, family="low_complexity")
    for n in (63, 64, 65, 4097):
        t = text("rand%d" % n)
        qs = _copies(rng, t, 12, 10, 0.1, 3)
        qs[0], qs[1] = t[:10].copy(), t[n - 10:].copy()            # position 0 and the text's last 10 symbols, one substitution each
        qs[0][1] = (qs[0][1] + 1) % 4
        qs[1][1] = (qs[1][1] + 2) % 4
        add("ends_%d" % n, "occurrences at text position 0 and ending at n, a text of %d symbols" % n, "rand%d" % n, qs, 3, 2, max_ranges=128, family="ends")
    ragged = [q for L in (1, 3, 7, 9, 15, 17, 23, 31, 33) for q in _copies(rng, r3, 4, L, 0.05, 0, ends=False)]
    add("mid_word", "ragged packed queries behind 5 symbols of lead-in: every begin falls mid-word", "rand3000", ragged, 6, 1, lead=5, family="mid_word")
    add("mid_word_seed0", "the same ragged set from the whole index", "rand3000", ragged, 0, 1, lead=5, family="mid_word")
    tl = text("two_letter")
    many = _copies(rng, tl, 10, 12, 0.1, 3) + [[0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 3, 1]] + _copies(rng, tl, 5, 12, 0.1, 3)
    add("truncated_1", "max_ranges = 1 below n_ranges: only the first range of a query is written", "two_letter", many, 3, 2, max_ranges="one", family="truncated")
    add("truncated_most", "max_ranges = n_ranges - 1 of the widest query: the last range is not written", "two_letter", many, 3, 2, max_ranges="most-1",
        family="truncated")
    r4 = text("rand4097")
    for seed, mm in ((16, 1), (14, 2)):
        add("quirks_seed%d_mm%d" % (seed, mm), "the reference's walk past the start of the query, on random text behind 64 symbols of lead-in", "rand4097",
            _copies(rng, r4, 120, 32, 0.03), seed, mm, lead=64, quirks=True, family="quirks")
    return tuple(cs)


def overflow_case():
    """the d = 128 query: one branch finds the stack full"""
    return BT("stack_overflow", "poly-T query of 16 + 128: one push beyond the 128-entry stack", "poly_t", (poly_t_query(128),), STACK_SEED, 1, 0, False, 64, "stack")


def stream_of(case):
    """(symbol stream uint8, offsets uint32 [Q + 1]) of a backtrack case; the lead-in is seeded by the case's name"""
    lead = np.random.default_rng(sum(map(ord, case.name))).integers(0, 4, case.lead, dtype=np.uint8)
    stream = np.concatenate([lead] + [q for q in case.queries]).astype(np.uint8) if (case.lead or case.queries) else np.zeros(0, np.uint8)
    offs = case.lead + np.concatenate([[0], np.cumsum([len(q) for q in case.queries])])
    return stream, offs.astype(np.uint32)


def widths_of(symbols):
    """the symbol widths a stream may be packed in"""
    return (2, 4, 8) if (len(symbols) == 0 or int(np.max(symbols)) < 4) else (4, 8)


# ---- approximate mapper cases -----------------------------------------------------------------------------------------------------
def worst_hits(spr, seed_len):
    """the total nvbio_seed_hits_approx_capacity caps: up to 3 (len2 - len1) + 1 hits per search, four searches per seed"""
    return 4 * spr * (3 * ((seed_len + 1) // 2) + 1)


def seed_params(spr, interval, seed_len, read_len, first_offset=0, rep_seeds=1000):
    assert first_offset + (spr - 1) * interval + seed_len <= read_len < 1024
    return dict(seeds_per_read=spr, first_offset=first_offset, seed_interval=interval, seed_len=seed_len, read_len=read_len, rep_seeds=rep_seeds)


def _reads(rng, t, n, length, sub=0.03, inside=None):
    """n stored reads: copies of the text (from `inside` = (lo, hi) for the first half of them), substitutions, half of them reverse-complemented,
    then reversed as nvBowtie stores them"""
    out = np.zeros((n, length), dtype=np.uint8)
    for i in range(n):
        lo, hi = (inside if inside is not None and i < (n + 1) // 2 else (0, len(t) - length))
        s = int(rng.integers(lo, min(hi, len(t) - length) + 1))
        r = t[s:s + length].copy()
        m = rng.random(length) < sub
        r[m] = (r[m] + 1 + rng.integers(0, 3, int(m.sum()))) % 4
        if rng.random() < 0.5:
            r = 3 - r[::-1]
        out[i] = r[::-1]
    return out


@functools.lru_cache(maxsize=None)
def mapper_cases():
    rng = np.random.default_rng(7400)
    cs = []
    m3k = text("m3k")

    def add(name, reason, text_name, reads, p, max_hits=None, queue=None, family="shapes"):
        if max_hits is None:
            max_hits = worst_hits(p["seeds_per_read"], p["seed_len"])
        cs.append(MP(name, reason, text_name, np.ascontiguousarray(reads, dtype=np.uint8), dict(p), max_hits,
                     None if queue is None else np.asarray(queue, dtype=np.uint32), family))

    for L in (1, 2, 3, 5, 12, 21, 31, 32):
        M = 40
        spr = 3 if L > 12 else 4
        why = "len1 = 0, the first rank4 at row -1 of the whole index" if L == 1 else ("odd: the four searches split at different len1" if L % 2 else "even")
        add("seed_len_%d" % L, "seed length %d: %s" % (L, why), "m3k", _reads(rng, m3k, 24, M, inside=(990, 1360)), seed_params(spr, (M - L) // (spr - 1), L, M),
            family="seed_len")
    add("every_4mer", "a text that holds every 4-mer, seed_len 3: exactly 7 + 3 + 7 + 3 = 20 hits per seed", "every4mer",
        _reads(rng, text("every4mer"), 16, 12, sub=0.2), seed_params(4, 3, 3, 12), family="full")
    add("every_3mer_70", "a 70-symbol text that holds every 3-mer, seed_len 3: 20 hits per seed", "t70",
        _reads(rng, text("t70"), 16, 12, sub=0.2), seed_params(4, 3, 3, 12), family="full")
    add("one_seed", "seeds_per_read = 1", "m3k", _reads(rng, m3k, 24, 40, inside=(990, 1360)), seed_params(1, 13, 15, 40), family="placement")
    add("first_offset", "first_offset != 0", "m3k", _reads(rng, m3k, 24, 40, inside=(990, 1360)), seed_params(3, 9, 13, 40, first_offset=7), family="placement")
    add("overlapping_seeds", "seed_interval < seed_len: the seeds overlap", "m3k", _reads(rng, m3k, 24, 40, inside=(990, 1360)), seed_params(6, 4, 15, 40),
        family="placement")
    add("last_seed_at_end", "the last seed ends exactly at the read's end", "m3k", _reads(rng, m3k, 24, 41, inside=(990, 1360)), seed_params(3, 13, 15, 41),
        family="placement")
    add("read_len_1023", "read length 1023: seed positions fill the top of the 10-bit position field", "m3k",
        _reads(rng, m3k, 6, 1023, sub=0.01), seed_params(2, 1002, 21, 1023), family="read_len")
    for M in (7, 9, 17):
        add("read_len_%d" % M, "read length %d: r * read_len starts mid-word for 2- and 4-bit reads" % M, "m3k",
            _reads(rng, m3k, 40, M, inside=(990, 1360)), seed_params(2, M - 5, 5, M), family="read_len")
    # N's: seed length 11 (len1 = 5 for the searches that check the exact match, 6 for the others), one seed at offset 3 of a 20-symbol read
    clean = _reads(rng, m3k, 8, 20, sub=0.0, inside=(990, 1360))
    for name, where, why in (("n_before_len1", [2], "an N before len1: the exact half fails"), ("n_at_len1", [5], "an N at len1 = 5 (and before len1 = 6)"),
                             ("n_at_len1_up", [6], "an N at len1 = 6 (and after len1 = 5)"), ("n_after_len1", [8], "an N after len1: four substitutions there"),
                             ("n_last", [10], "an N in the seed's last position"), ("two_n", [6, 9], "two N's in one seed: nothing past the first")):
        r = np.concatenate([clean, clean[:2]])
        r[:8, [3 + w for w in where]] = N_
        add(name, why, "m3k", r, seed_params(1, 1, 11, 20, first_offset=3), family="n")
    rep = _reads(rng, m3k, 24, 60, sub=0.01, inside=(1000, 1330))
    for mh in (1, 2, 3):
        add("max_hits_%d" % mh, "max_hits = %d: the interval heap's pop_bottom on a heap of %d" % (mh, mh), "m3k", rep, seed_params(5, 12, 12, 60), max_hits=mh,
            family="max_hits")
    e4 = _reads(rng, text("every4mer"), 12, 12, sub=0.2)
    w = worst_hits(4, 3)
    add("max_hits_worst", "max_hits = the worst-case total: the capacity's two bounds meet", "every4mer", e4, seed_params(4, 3, 3, 12), max_hits=w, family="capacity")
    add("max_hits_worst_minus_1", "max_hits one below the worst-case total", "every4mer", e4, seed_params(4, 3, 3, 12), max_hits=w - 1, family="capacity")
    # the reseed rule at its boundary: rep_seeds = range_sum / range_count of one read exactly, and one more
    rs_reads = np.concatenate([_reads(rng, m3k, 24, 40, inside=(990, 1360)), np.zeros((1, 40), dtype=np.uint8)])
    rs_reads[-1] = rs_reads[0]
    rs_reads[-1, [1, 2, 14, 15, 27, 28]] = N_                       # every seed holds two early N's: before len1 read forwards, both past it
                                                                    # read backwards, where the second ends what the first began: range_count == 0
    p = seed_params(3, 13, 13, 40)
    fwd, rev = scan_text("m3k"), scan_text("m3k", True)
    ratio = None
    for r in rs_reads[:-1]:
        _, s, c, _ = ap.map_approx_scan(fwd, rev, r, p)
        if c and s % c == 0 and s // c >= 2:
            ratio = s // c
            break
    assert ratio is not None, "no read with range_sum a multiple (>= 2) of range_count: change the generator's seed"
    add("reseed_at_boundary", "rep_seeds with range_sum == rep_seeds * range_count for one read: it reseeds; a read with no range at all reseeds", "m3k",
        rs_reads, dict(p, rep_seeds=ratio), family="reseed")
    add("reseed_above_boundary", "rep_seeds one more: that read does not reseed", "m3k", rs_reads, dict(p, rep_seeds=ratio + 1), family="reseed")
    qr = _reads(rng, m3k, 40, 40, inside=(990, 1360))
    add("read_queue", "a permuted read_queue naming a strict subset of the reads: the other rows keep their fill", "m3k", qr, seed_params(3, 13, 13, 40),
        queue=np.random.default_rng(7401).permutation(40)[:23], family="queue")
    add("read_queue_bitten", "the same queue with max_hits biting", "m3k", qr, seed_params(3, 13, 13, 40), max_hits=3,
        queue=np.random.default_rng(7402).permutation(40)[:17], family="queue")
    add("tandem", "reads inside a tandem repeat: large sub-ranges that tie", "m3k", _reads(rng, m3k, 32, 50, sub=0.01, inside=(1000, 1340))[:16],
        seed_params(4, 10, 14, 50), family="tandem")
    add("tandem_60k", "the same in a text of 60,000 symbols", "m60k", _reads(rng, text("m60k"), 32, 50, sub=0.02, inside=(1000, 1340)), seed_params(4, 10, 16, 50),
        family="tandem")
    add("tandem_60k_bitten", "... with max_hits = 7 biting", "m60k", _reads(rng, text("m60k"), 32, 50, sub=0.02, inside=(1000, 1340)), seed_params(4, 10, 16, 50),
        max_hits=7, family="tandem")
    return tuple(cs)
