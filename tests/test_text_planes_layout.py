"""CPU: the text kept as bit planes (include/nvbio_amd.h: nvbio_text_planes_build; csrc/bitplanes.h: load_text_units, text_planes_units), restated in numpy.

A unit is 16 bytes, (lo64, hi64) of 64 consecutive text symbols: bit j of lo64 / hi64 = the low / high bit of symbol 64 u + j.  Line L (128 bytes)
holds units 4 L .. 4 L + 7, i.e. symbols 256 L .. 256 L + 511; there are ((n + 255) >> 8) + 1 lines and every bit at or beyond n is zero.

planes_reference() is that definition, and what tests/test_gpu_text_planes.py compares the builder with.  window_from_line() is the loader's
arithmetic: the window that begins at symbol tb is taken from the ONE line tb >> 8, from unit (tb & 255) >> 6 on, shifted by tb & 63.  The
extent argument next to the loader -- a single job looks at up to 192 symbols through 4 units, a gap-chance pair at up to 197 through 5, and
the last unit's index never exceeds 7 -- is checked for every tb mod 256 and every extent."""
import numpy as np

LINE_SYMBOLS, UNIT_SYMBOLS, UNITS_PER_LINE = 256, 64, 8
SINGLE_EXTENT, PAIR_EXTENT = 192, 197                               # 161 + 31, 161 + 31 + 5 (the pair's largest shift)


def n_lines(n):
    return ((n + 255) >> 8) + 1


def planes_reference(sym):
    """uint64 [lines, 8, 2]: (lo64, hi64) of every unit of every line of the text `sym` (one symbol 0..3 per entry)"""
    n, nl = len(sym), n_lines(len(sym))
    n_units = 4 * (nl - 1) + UNITS_PER_LINE
    bits = np.zeros((2, n_units * UNIT_SYMBOLS), dtype=np.uint8)
    bits[0, :n], bits[1, :n] = sym & 1, (sym >> 1) & 1
    words = np.packbits(bits, axis=1, bitorder="little").view("<u8")                 # [2, n_units]: bit j of word u = symbol 64 u + j
    units = np.stack([words[0], words[1]], axis=1)                                   # [n_units, 2]
    return np.stack([units[4 * L:4 * L + UNITS_PER_LINE] for L in range(nl)])


def last_unit(tb, extent):
    """index, within line tb >> 8, of the unit that holds the window's last symbol"""
    return ((tb & 255) >> 6) + (((tb & 63) + extent - 1) >> 6)


def window_from_line(planes, tb, extent, units):
    """the `extent` symbols from tb on, read as load_text_units<units> and text_planes_units<units> read them"""
    line, u0, s = planes[tb >> 8], (tb & 255) >> 6, tb & 63
    assert u0 + units - 1 < UNITS_PER_LINE
    lo = np.unpackbits(line[u0:u0 + units, 0].copy().view(np.uint8), bitorder="little")
    hi = np.unpackbits(line[u0:u0 + units, 1].copy().view(np.uint8), bitorder="little")
    assert s + extent <= units * UNIT_SYMBOLS
    return lo[s:s + extent] | (hi[s:s + extent] << 1)


def test_every_window_ends_inside_its_line():
    for tbm in range(LINE_SYMBOLS):
        for extent in range(1, PAIR_EXTENT + 1):
            lu = last_unit(tbm, extent)
            assert lu <= 7, (tbm, extent, lu)
            n_units = lu - ((tbm & 255) >> 6) + 1
            assert n_units <= (4 if extent <= SINGLE_EXTENT else 5), (tbm, extent, n_units)
    # and the bounds are tight: one symbol more does not fit
    assert max(last_unit(t, SINGLE_EXTENT) - (t >> 6) + 1 for t in range(LINE_SYMBOLS)) == 4
    assert max(last_unit(t, PAIR_EXTENT) - (t >> 6) + 1 for t in range(LINE_SYMBOLS)) == 5
    assert max(last_unit(t, PAIR_EXTENT) for t in range(LINE_SYMBOLS)) == 7
    assert max(last_unit(t, SINGLE_EXTENT + 2) - (t >> 6) + 1 for t in range(LINE_SYMBOLS)) == 5
    assert max(last_unit(t, PAIR_EXTENT + 61) for t in range(LINE_SYMBOLS)) == 8


def test_layout_size_and_padding():
    rng = np.random.default_rng(5)
    for n in (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 70001):
        sym = rng.integers(0, 4, n, dtype=np.uint8)
        p = planes_reference(sym)
        assert p.shape == (n_lines(n), 8, 2) and p.nbytes == n_lines(n) * 128
        assert (n - 1) >> 8 < n_lines(n)                            # the line of the text's last symbol exists
        # the two halves of neighbouring lines are the same units
        assert np.array_equal(p[:-1, 4:], p[1:, :4])
        # every symbol where the definition puts it, zeros beyond n
        flat = np.concatenate([p[:, :4].reshape(-1, 2), p[-1, 4:]])                    # units 0, 1, 2, ... in order
        lo = np.unpackbits(flat[:, 0].copy().view(np.uint8), bitorder="little")
        hi = np.unpackbits(flat[:, 1].copy().view(np.uint8), bitorder="little")
        assert np.array_equal((lo | (hi << 1))[:n], sym) and not lo[n:].any() and not hi[n:].any()


def test_a_window_is_read_from_one_line():
    rng = np.random.default_rng(6)
    n = 3000
    sym = rng.integers(0, 4, n, dtype=np.uint8)
    p = planes_reference(sym)
    padded = np.concatenate([sym, np.zeros(600, dtype=np.uint8)])
    for tb in list(range(0, 520)) + list(range(n - 300, n)):
        for extent, units in ((SINGLE_EXTENT, 4), (PAIR_EXTENT, 5), (1, 4), (64 - (tb & 63), 4)):
            got = window_from_line(p, tb, extent, units)
            assert np.array_equal(got, padded[tb:tb + extent]), (tb, extent)
