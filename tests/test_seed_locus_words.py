"""The seed pass's read of a locus line on paper (csrc/bitplanes.h: load_locus_words, locus_answers; csrc/fm_canon_inl.h: the locus stage
of fm_seed_locus_loop): a lane reads five 32-bit words -- of each symbol plane the word that holds x and the word behind it, and the word
of u that holds x -- funnels each plane by x & 31, and compares with its seed's planes; a lane on the reverse strand mirrors and inverts
its planes instead of taking the reverse complement of its seed.  Restated in numpy against the 64-bit unit form of
test_seed_locus_layout.py (window_from_line), for every place of a read in its line and every seed length a 32-bit word holds."""
import numpy as np

from test_seed_locus_layout import MAX_READ, UNITS, locus_lines, window_from_line

M32 = 0xFFFFFFFF


def words_from_line(lines, base, x):
    """load_locus_words: (lo0, lo1, hi0, hi1, u) of the window at x, out of line base >> 7; as 32-bit words a unit is lo, lo', hi, hi', u, u'"""
    w32 = lines[base >> 7].view("<u4")
    off = x - ((base >> 7) << 7)
    unit, w = off >> 6, (off >> 5) & 1
    assert 0 <= off and unit < UNITS
    p = 6 * unit
    w1 = (6 if unit + 1 < UNITS else 0) if w else 1           # behind a unit's second word: the first word of the next unit, if there is one
    assert max(p + w1, p + 2 + w1, p + 4 + w) < 32             # every word read lies inside the line
    return tuple(int(w32[i]) for i in (p + w, p + w1, p + 2 + w, p + 2 + w1, p + 4 + w))


def alignbit(hi, lo, s):
    return (((hi << 32) | lo) >> (s & 31)) & M32


def locus_answers(lw, x, length, tlo, thi):
    lo0, lo1, hi0, hi1, u = lw
    s = x & 31
    lo, hi = alignbit(lo1, lo0, s), alignbit(hi1, hi0, s)
    mask = M32 if length >= 32 else (1 << length) - 1
    return (((lo ^ tlo) | (hi ^ thi)) & mask) == 0 and ((u >> s) & 1) == 1


def squeeze2(v):
    """every 2nd bit of a 32-bit word (positions 0, 2, .., 30) squeezed into 16 bits"""
    return sum(((v >> (2 * i)) & 1) << i for i in range(16))


def seed_planes(syms, strand):
    """the planes the locus stage makes of a seed's bits V (symbol t at bits [2 t, 2 t + 2)): squeezed in 32-bit halves; on the reverse
    strand mirrored and inverted -- bits from the seed's length on are ones there, and ignored"""
    length = len(syms)
    V = sum(int(c) << (2 * t) for t, c in enumerate(syms))
    vl, vh = V & M32, V >> 32
    plo, phi = squeeze2(vl) | (squeeze2(vh) << 16), squeeze2(vl >> 1) | (squeeze2(vh >> 1) << 16)
    if strand:
        brev = lambda v: int(format(v, "032b")[::-1], 2)
        plo, phi = ~(brev(plo) >> (32 - length)) & M32, ~(brev(phi) >> (32 - length)) & M32
    return plo, phi


def test_five_words_hold_the_window_wherever_the_read_begins():
    rng = np.random.default_rng(11)
    n = 2000
    text = rng.integers(0, 4, n, dtype=np.uint8)
    u = rng.integers(0, 2, n, dtype=np.uint8)
    lines = locus_lines(text, u)
    for p in range(128):                                                        # every place of the read's first symbol in its line
        base = 640 + p
        for length in (1, 14, 22, 31, 32):
            for x in {base, base + 1, base + 31 - (p & 31), base + 32 - (p & 31), base + (MAX_READ - length) // 2, base + MAX_READ - length}:
                lo0, lo1, hi0, hi1, uw = words_from_line(lines, base, x)
                s = x & 31
                lo, hi = alignbit(lo1, lo0, s), alignbit(hi1, hi0, s)
                syms = np.array([((lo >> t) & 1) | (((hi >> t) & 1) << 1) for t in range(length)], dtype=np.uint8)
                want, want_u = window_from_line(lines, base, x, length)
                assert np.array_equal(syms, want) and np.array_equal(syms, text[x:x + length]) and (uw >> s) & 1 == want_u == u[x]


def test_the_last_word_of_a_line_has_nothing_behind_it():
    """the window in the second word of the line's last unit: the word read in place of the one behind it is not looked at"""
    rng = np.random.default_rng(12)
    text = rng.integers(0, 4, 1000, dtype=np.uint8)
    lines = locus_lines(text, np.ones(1000, dtype=np.uint8))
    base = 128 + 127                                                            # the read begins at the end of its line's first 128 symbols
    for length in (1, 14, 22, 32):
        x = base + MAX_READ - length                                            # its last window ends on the line's last symbol
        assert x + length - 1 - 128 == 64 * UNITS - 1
        for strand in (0, 1):
            w = text[x:x + length]
            seed = (3 - w)[::-1] if strand else w
            assert locus_answers(words_from_line(lines, base, x), x, length, *seed_planes(seed, strand))


def test_a_window_is_answered_iff_it_equals_the_seed_and_is_unique():
    rng = np.random.default_rng(13)
    n = 3000
    text = rng.integers(0, 4, n, dtype=np.uint8)
    u = rng.integers(0, 2, n, dtype=np.uint8)
    lines = locus_lines(text, u)
    seen = [0, 0, 0]
    for _ in range(3000):
        length = int(rng.integers(1, 33))
        base = int(rng.integers(0, n - MAX_READ))
        x = base + int(rng.integers(0, MAX_READ - length + 1))
        strand = int(rng.integers(0, 2))
        w = text[x:x + length].copy()
        differs = rng.random() < 0.4
        if differs:
            w[rng.integers(0, length)] ^= int(rng.integers(1, 4))
        seed = (3 - w)[::-1] if strand else w                                   # a lane on the reverse strand holds the reverse complement
        got = locus_answers(words_from_line(lines, base, x), x, length, *seed_planes(seed, strand))
        assert got == (not differs and u[x] == 1), (length, base, x, strand, differs)
        seen[0 if differs else 1 + int(u[x])] += 1
    assert min(seen) > 300
