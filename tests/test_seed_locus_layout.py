"""The seed locus lines on paper (include/nvbio_amd.h: nvbio_seed_locus_build; csrc/bitplanes.h): a numpy restatement of the layout, the
claim that ONE line holds every seed window of a read of up to 193 symbols wherever the read begins, and the brute-force meaning of the
uniqueness plane u.  The GPU tests (test_gpu_seed_locus.py) compare the library's lines with locus_lines() word for word."""
import numpy as np

LINE_WORDS = 16            # a line: 128 bytes, 16 uint64
UNIT_WORDS = 3             # a unit: lo64, hi64, u64 of 64 symbols
UNITS = 5                  # units per line: symbols 128 L .. 128 L + 319, then one zero word
MAX_READ = 193


def n_lines(n):
    return (n >> 7) + 1


def _planes(bits):
    """bits [units * 64] of 0/1 -> uint64 [units], bit j of word u = bits[64 u + j]"""
    w = np.uint64(1) << np.arange(64, dtype=np.uint64)
    return (bits.reshape(-1, 64).astype(np.uint64) * w).sum(axis=1, dtype=np.uint64)


def locus_lines(text, u):
    """the lines of a text (symbols 0..3) and its uniqueness plane as uint64 [n_lines, 16]"""
    n = len(text)
    L = n_lines(n)
    units = 2 * (L - 1) + UNITS
    sym = np.zeros(units * 64, dtype=np.uint8); sym[:n] = text
    ub = np.zeros(units * 64, dtype=np.uint8); ub[:n] = u
    lo, hi, uu = _planes(sym & 1), _planes((sym >> 1) & 1), _planes(ub)
    lines = np.zeros((L, LINE_WORDS), dtype=np.uint64)
    for s in range(UNITS):
        idx = 2 * np.arange(L) + s
        lines[:, UNIT_WORDS * s], lines[:, UNIT_WORDS * s + 1], lines[:, UNIT_WORDS * s + 2] = lo[idx], hi[idx], uu[idx]
    return lines


def window_from_line(lines, base, x, length):
    """what a lane of the seed pass reads: the `length` symbols from x on and u[x], out of the ONE line base >> 7 of the read that begins
    at `base` -- the unit that holds x and the planes of the next one (load_locus_units / locus_answers)"""
    line = lines[base >> 7]
    off = x - ((base >> 7) << 7)
    unit, s = off >> 6, off & 63
    assert 0 <= off and unit < UNITS
    nxt = min(unit + 1, UNITS - 1)
    assert s + length <= 64 or unit + 1 < UNITS                 # a window that crosses into the next unit has one
    lo = (int(line[3 * unit]) >> s) | (int(line[3 * nxt]) << (64 - s))
    hi = (int(line[3 * unit + 1]) >> s) | (int(line[3 * nxt + 1]) << (64 - s))
    syms = np.array([((lo >> t) & 1) | (((hi >> t) & 1) << 1) for t in range(length)], dtype=np.uint8)
    return syms, (int(line[3 * unit + 2]) >> s) & 1


def window_codes(text, length):
    """(code of text[x, x + length), code of its reverse complement) for every x in [0, n - length]; symbol t at bits [2 t, +2)"""
    n = len(text)
    m = n - length + 1
    if m <= 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    t = text.astype(np.int64)
    fw = np.zeros(m, dtype=np.int64); rc = np.zeros(m, dtype=np.int64)
    for i in range(length):
        fw |= t[i:i + m] << (2 * i)
        rc |= (3 - t[i:i + m]) << (2 * (length - 1 - i))
    return fw, rc


def occurrences(text, length):
    """occ[x] = occurrences of text[x, x + length) plus those of its reverse complement, over the whole text; int64 [n], 0 past n - length"""
    n = len(text)
    fw, rc = window_codes(text, length)
    vals, cnt = np.unique(fw, return_counts=True)

    def count(codes):
        i = np.searchsorted(vals, codes)
        i = np.minimum(i, len(vals) - 1)
        return np.where(vals[i] == codes, cnt[i], 0)
    occ = np.zeros(n, dtype=np.int64)
    occ[:len(fw)] = count(fw) + count(rc)
    return occ


def brute_unique(text, length):
    """u by its meaning: text[x, x + length) occurs once and its reverse complement nowhere (a window that is its own reverse complement
    counts twice); 0 in the last length - 1 positions"""
    return (occurrences(text, length) == 1).astype(np.uint8)


def table_unique(text, length, k, rows_max=8):
    """u as the builder defines it: brute_unique, and neither the window's last k symbols nor its first k symbols form a k-mer with more
    than rows_max occurrences over both strands (such a k-mer has no rows in the canonical table)"""
    n = len(text)
    u = brute_unique(text, length)
    kocc = occurrences(text, k)
    m = n - length + 1
    if m > 0:
        u[:m] &= (kocc[:m] <= rows_max) & (kocc[length - k:length - k + m] <= rows_max)
    return u


def test_layout_restated():
    rng = np.random.default_rng(1)
    for n in (1, 63, 64, 127, 128, 129, 300, 1000, 1024 + 127):
        text = rng.integers(0, 4, n, dtype=np.uint8)
        u = rng.integers(0, 2, n, dtype=np.uint8)
        lines = locus_lines(text, u)
        assert lines.shape == ((n >> 7) + 1, 16) and lines.nbytes == ((n >> 7) + 1) * 128
        assert (lines[:, 15] == 0).all()                                       # the 8 pad bytes
        for L in range(lines.shape[0]):
            for s in range(UNITS):
                lo, hi, ub = (int(v) for v in lines[L, 3 * s:3 * s + 3])
                for j in (0, 1, 31, 62, 63):
                    x = 128 * L + 64 * s + j
                    want = (int(text[x]), int(u[x])) if x < n else (0, 0)       # every bit at or beyond n is zero
                    assert (((lo >> j) & 1) | (((hi >> j) & 1) << 1), (ub >> j) & 1) == want
        # consecutive lines overlap: units 2, 3, 4 of line L are units 0, 1, 2 of line L + 1
        assert np.array_equal(lines[:-1, 6:15], lines[1:, 0:9])


def test_one_line_holds_a_read_of_193_symbols():
    rng = np.random.default_rng(2)
    n = 2000
    text = rng.integers(0, 4, n, dtype=np.uint8)
    u = rng.integers(0, 2, n, dtype=np.uint8)
    lines = locus_lines(text, u)
    length = 22
    for p in range(128):                                                       # every P0 mod 128
        for M in range(1, MAX_READ + 1):
            assert (p + M - 1) <= 64 * UNITS - 1                                # the read's last symbol lies in the line of its first
            assert ((p & 127) >> 6) <= 1
    for p in range(128):
        base = 512 + p
        for M in (length, 100, MAX_READ):
            for x in (base, base + 1, base + (M - length) // 2, base + M - length):
                syms, ub = window_from_line(lines, base, x, length)
                assert np.array_equal(syms, text[x:x + length]) and ub == u[x]
    # one symbol more can overflow the line
    assert 127 + (MAX_READ + 1) - 1 > 64 * UNITS - 1


def test_brute_force_u():
    def sym(s):
        return np.array(["ACGT".index(c) for c in s], dtype=np.uint8)
    # every 4-mer of this text is unique over both strands except ...
    text = sym("AACCAGGATTTGCA")
    u = brute_unique(text, 4)
    fw, rc = window_codes(text, 4)
    for x in range(len(text) - 3):
        w = text[x:x + 4]
        r = (3 - w)[::-1]
        occ = sum(np.array_equal(text[y:y + 4], w) for y in range(len(text) - 3)) + sum(np.array_equal(text[y:y + 4], r) for y in range(len(text) - 3))
        assert u[x] == (occ == 1)
    assert (u[-3:] == 0).all()
    assert u[len("AACCAGGATT")] == 0                                            # TGCA is its own reverse complement: two hits at one place
    assert u[0] == 1
    # a repeat and a reverse-complement copy switch u off on both copies
    rng = np.random.default_rng(3)
    t = rng.integers(0, 4, 600, dtype=np.uint8)
    t[300:340] = t[100:140]
    t[500:540] = (3 - t[200:240])[::-1]
    u = brute_unique(t, 12)
    assert not u[100:129].any() and not u[300:329].any() and not u[200:229].any() and not u[500:529].any()
    assert u[:80].all()
    # heavy k-mers at either end of the window switch it off in the builder's form
    t2 = rng.integers(0, 4, 3000, dtype=np.uint8)
    for c in range(12):
        t2[200 * c + 50:200 * c + 57] = t2[50:57]
    ut, ub = table_unique(t2, 12, 5), brute_unique(t2, 12)
    assert (ut <= ub).all() and (ut < ub).any()
