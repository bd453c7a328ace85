"""The one-pass emission of a common tile (csrc/fm_canon_inl.h: resolve_tile) restated in numpy against the two-pass rule it replaces.

A common tile: every lane holds at most one (strand, position).  The two-pass rule (emit_seed_results, once per strand): the strand's keys
in lane order, a key dropped iff it EQUALS the key of the nearest lower lane with a key on that strand; forward keys first.  The one-pass
rule: the predecessor is found the same way, but the test is "the predecessor lies in this lane's read AND its diagonal's low word equals
mine" -- no 64-bit key is shipped between lanes.  The two agree because the strand bit is equal by construction, the read id sits in bits
34 and up, and the diagonal (position + 1024 - offset, 0 <= it < 2^32: a text has at most 2^32 - 8193 symbols, an offset is at most 1024)
never reaches them.  The random tiles draw diagonals from a handful of values at both ends of that range, so that equal diagonals in
neighbouring reads -- the boundary at which key equality and the restated test could part -- occur in nearly every tile."""
import numpy as np
import pytest

MAX_TEXT = (1 << 32) - 8193


def _key(rid, strand, diag):
    return (np.uint64(rid) << np.uint64(34)) | (np.uint64(strand) << np.uint64(33)) | np.uint64(diag)


def two_pass(spr, rid0, has, strand, diag):
    """emit_seed_results twice: per strand, the keys in lane order with a key equal to its predecessor's dropped"""
    out, counts = [], []
    for s in (0, 1):
        last, n = None, 0
        for lane in range(64):
            if not has[lane] or strand[lane] != s:
                continue
            key = _key(rid0 + lane // spr, s, diag[lane])
            if last is None or key != last:
                out.append(key); n += 1
            last = key
        counts.append(n)
    return np.array(out, dtype=np.uint64), counts


def one_pass(spr, rid0, has, strand, diag):
    """the merged emission, lane by lane as the kernel computes it: masks, the predecessor's lane, one 32-bit compare, slots"""
    lanes = range(64)
    strand = [int(v) for v in strand]
    m = [sum(1 << l for l in lanes if has[l] and strand[l] == s) for s in (0, 1)]
    keep = np.zeros(64, dtype=bool)
    for lane in lanes:
        if not has[lane]:
            continue
        prev_mask = m[strand[lane]] & ((1 << lane) - 1)
        dup = False
        if prev_mask:
            prev_lane = prev_mask.bit_length() - 1
            first = lane - lane % spr                                          # lane - j: the lane of this read's first seed
            dup = prev_lane >= first and (int(diag[prev_lane]) & 0xFFFFFFFF) == (int(diag[lane]) & 0xFFFFFFFF)
        keep[lane] = not dup
    k = [sum(1 << l for l in lanes if keep[l] and strand[l] == s) for s in (0, 1)]
    n0, n1 = bin(k[0]).count("1"), bin(k[1]).count("1")
    slots = np.zeros(n0 + n1, dtype=np.uint64)
    written = np.zeros(n0 + n1, dtype=bool)
    for lane in lanes:
        if keep[lane]:
            s = strand[lane]
            at = (n0 if s else 0) + bin(k[s] & ((1 << lane) - 1)).count("1")
            assert not written[at]
            slots[at], written[at] = _key(rid0 + lane // spr, s, diag[lane]), True
    assert written.all()
    return slots, [n0, n1]


@pytest.mark.parametrize("spr", [1, 2, 9, 64])
def test_merged_emission_equals_the_two_pass_rule(spr):
    rng = np.random.default_rng(1600 + spr)
    rpt = 64 // spr
    pool = np.array([0, 1, 1023, 1024, 1025, MAX_TEXT + 1023, MAX_TEXT + 1022, (1 << 32) - 1, (1 << 31), 77777], dtype=np.int64)
    dropped = kept_across_reads = both = 0
    for trial in range(400):
        rid0 = int(rng.choice([0, 7, (1 << 30) - 64, 123456]))
        density = rng.choice([0.2, 0.6, 1.0])
        has = rng.random(64) < density
        has[rpt * spr:] = False                                                # lanes behind the tile's last read hold no seed
        if trial % 5 == 0:
            has[rng.integers(0, rpt) * spr:] = False                           # a partial last tile
        strand = np.repeat(rng.integers(0, 2, rpt + 1), spr)[:64]              # a read lies on one strand ...
        flip = rng.random(64) < 0.1
        strand = np.where(flip, 1 - strand, strand)                            # ... but a seed may hit the other one
        diag = np.repeat(rng.choice(pool[:4 + trial % 7], rpt + 1), spr)[:64]  # a read's seeds share a diagonal; neighbouring reads often do
        off = rng.random(64) < 0.15
        diag = np.where(off, rng.choice(pool, 64), diag)                       # an indel: another diagonal in the same read
        a, ca = two_pass(spr, rid0, has, strand, diag)
        b, cb = one_pass(spr, rid0, has, strand, diag)
        assert ca == cb and np.array_equal(a, b), (spr, trial)
        dropped += int(has.sum()) - len(a)
        both += ca[0] > 0 and ca[1] > 0
        for lane in range(spr, 64, spr):                                       # a read's first key equal in diagonal and strand to the previous read's last
            if has[lane] and has[lane - 1] and strand[lane] == strand[lane - 1] and diag[lane] == diag[lane - 1]:
                kept_across_reads += 1
    assert both > 100 and (kept_across_reads > 20 or spr == 64)                # (64 seeds per read: a tile is one read)
    assert dropped > 100 or spr == 1                                           # (one seed per read: nothing to drop)


def test_the_diagonal_is_its_low_word():
    """the bounds the equivalence rests on: position + 1024 - offset stays inside [0, 2^32) for every text the index accepts"""
    for pos in (0, 1, MAX_TEXT - 14, MAX_TEXT):
        for off in (0, 1, 1024):
            d = pos + 1024 - off
            assert 0 <= d < (1 << 32) and (d & 0xFFFFFFFF) == d
            assert int(_key(5, 1, d)) >> 34 == 5 and (int(_key(5, 1, d)) >> 33) & 1 == 1
