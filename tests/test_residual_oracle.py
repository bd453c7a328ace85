"""CPU: the restatement of the two residual-key routes (residual_cpu.py) pinned on the oracle -- its seed ranges against match() on the oracle's
FM index of the same text, its two-call keys against the oracle's FMIndexFilter::locate put through hit_to_diagonal -- and on itself: the set
of keys of the one-call rule equals that of the two-call form over the capped ranges, the vectorised cap = 1 form equals the scalar one.
Then the proofs that the cases of residual_cases.py are what their names say: keys are dropped where a case says so and nowhere where it says
not, the periodic cases keep duplicates, the cap cases hold a range below, at and above the cap, the large case passes 8,192 x 256 entries."""
from collections import Counter

import numpy as np
import pytest

import residual_cases as cases
import residual_cpu as rc
import selection_cpu as sel

OC_CASES = list(cases.one_call_cases())
TC_CASES = list(cases.two_call_cases())
_ONE, _IDX = {}, {}


def _index(orc):
    if "idx" not in _IDX:
        _IDX["idx"] = orc.build_index(cases.text())
    return _IDX["idx"]


def _one(case):
    if case.name not in _ONE:
        _ONE[case.name] = rc.one_call_keys(cases.scan_text(), case.entries, case.cap, case.g)
    return _ONE[case.name]


def _field(key):
    return key & sel.FIELD


def _who(id32, g):
    return (id32 & (rc.STRAND_BIT - 1)) // g.spr, id32 >> 31


def test_every_case_has_a_name_and_a_reason():
    assert len(cases.text()) <= 20000
    for cs in (OC_CASES, TC_CASES):
        names = [c.name for c in cs]
        assert len(set(names)) == len(names)
        assert all(len(c.reason) > 10 and "\n" not in c.reason for c in cs)
    for c in OC_CASES:
        assert all(x >= 1 for x, _, _ in c.entries), c.name         # row 0 is outside the contract
        assert c.tags & {"drops", "no_drops", "periodic"}, c.name
        lengths = [c.g.read_len] if c.g.read_offsets is None else np.diff(c.g.read_offsets.astype(np.int64)).tolist()
        assert 30 <= min(lengths) and max(lengths) <= 1046, c.name
    assert {c.cap for c in OC_CASES if "cap" in c.tags} == {1, 2, 4, 63, 64}
    assert {len(c.entries) for c in OC_CASES} >= {1, 255, 256, 257, 513}
    assert max(c.g.read_len for c in OC_CASES if c.g.read_offsets is None) == 1046
    for c in TC_CASES:
        assert all(x >= 1 for i, (x, _) in enumerate(c.ranges) if not (c.direct and c.direct[i])), c.name


# ---- the restatement against the oracle -------------------------------------------------------------------------------------------
def test_seed_entries_equal_the_oracles_match(orc):
    """the rows the text scan finds for a seed are the range match() ends on; a seed the text does not hold ends on some empty range"""
    hidx, T = _index(orc), cases.scan_text()
    rng = np.random.default_rng(9500)
    fixed_reads = [cases.copy(cases.in_fam12(3, 20), 100), cases.copy(cases.in_fam70(5, 4), 100, True), cases.copy(300, 100), cases.junk(rng, 100),
                   cases.copy(cases.PERIOD2 + 7, 100), cases.copy(cases.PERIOD5 + 3, 100, True), np.concatenate([cases.junk(rng, 5), cases.copy(0, 95)]),
                   cases.copy(cases.N_TEXT - 100, 100)]
    lengths = [30, 57, 200, 64]
    gr = rc.ragged(4, cases.SEED, lengths, [2, 11, 59, 14])
    ragged_reads = [cases.copy(p, m, r % 2 == 1) for r, (p, m) in enumerate(zip([cases.in_fam12(1, 9), cases.in_fam70(2, 11), cases.in_fam12(8, 0), 16700], lengths))]
    nonempty = 0
    for g, reads in ((cases.G8, fixed_reads), (cases.G7, fixed_reads), (gr, ragged_reads)):
        got = rc.seed_entries(T, reads, g)
        n = len(reads) * g.spr
        assert len(got) == 2 * n
        seeds = []
        for rid, read in enumerate(reads):
            s, _ = rc.read_shape(g, rid)
            seeds += [read[j * s:j * s + g.seed_len] for j in range(g.spr)]
        flat = np.concatenate(seeds).astype(np.uint8)
        offs = (np.arange(n + 1) * g.seed_len).astype(np.uint32)
        want = np.concatenate([orc.match_batch(hidx, flat, offs), orc.match_batch(hidx, (3 - flat).astype(np.uint8), offs, reverse=True)]).astype(np.int64)
        for e, ((x, y, id32), (wx, wy)) in enumerate(zip(got, want)):
            assert id32 == (e % n) | (rc.STRAND_BIT if e >= n else 0)
            if wx <= wy:
                assert (x, y) == (wx, wy), (e, "range")
                nonempty += 1
            else:
                assert (x, y) == rc.EMPTY, (e, "empty")
    assert nonempty > 60


@pytest.mark.parametrize("case", TC_CASES, ids=[c.name for c in TC_CASES])
def test_two_call_keys_equal_the_oracles_filter_locate(orc, case):
    """every output: the oracle's FMIndexFilter::locate over the plain ranges gives (position, range), hit_to_diagonal the key"""
    hidx, T = _index(orc), cases.scan_text()
    plain = np.array(cases.plain_of(case), dtype=np.uint32).reshape(-1, 2)
    slots = rc.inclusive_sizes(plain.tolist())
    total = int(slots[-1])
    hits = orc.filter_locate(hidx, plain, slots, 0, total)
    for g in case.geoms:
        want = [rc.key_of(int(pos), int(q) if case.ids is None else case.ids[int(q)], g, case.strand) for pos, q in hits]
        assert rc.two_call_keys(T, list(case.ranges), case.ids, case.direct, case.strand, g) == want
    assert all(0 <= b < e <= total for b, e in case.windows)


@pytest.mark.parametrize("case", OC_CASES, ids=[c.name for c in OC_CASES])
def test_one_call_set_equals_the_capped_two_call_set(case):
    """what the header promises: dropping a key that the previous entry leaves at the same row never loses a key"""
    T = cases.scan_text()
    kept, dropped = _one(case)
    two = rc.two_call_keys(T, rc.capped(case.entries, case.cap), [i for _, _, i in case.entries], None, 0, case.g)
    assert set(kept) == set(two)
    assert sum(kept.values()) + dropped == len(two)
    assert not kept - Counter(two)                                  # (no key written more often than the two-call form lists it)


def test_vectorised_cap_1_equals_the_scalar_rule():
    T = cases.scan_text()
    x, y, ids = cases.large_case()
    first = (ids & (rc.STRAND_BIT - 1)) < 6000                      # the first 1,500 reads of the large case, in the order handed over
    entries = list(zip(x[first].tolist(), y[first].tolist(), ids[first].tolist()))
    assert len(entries) == 6000
    kept, dropped = rc.one_call_keys(T, entries, 1, cases.G_LARGE)
    keys, n_dropped = rc.one_call_keys_cap1(T, x[first], y[first], ids[first], cases.G_LARGE)
    assert sorted(kept.elements()) == keys.tolist() and n_dropped == dropped and dropped > 1000 and len(keys) > 1000
    for c in OC_CASES:                                              # ... and every fixed-length case, its cap set to 1
        if c.g.read_offsets is None:
            kept, dropped = rc.one_call_keys(T, c.entries, 1, c.g)
            e = np.array(c.entries, dtype=np.int64).reshape(-1, 3)
            keys, n_dropped = rc.one_call_keys_cap1(T, e[:, 0], e[:, 1], e[:, 2], c.g)
            assert sorted(kept.elements()) == keys.tolist() and n_dropped == dropped, c.name


# ---- the cases are what they say --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", OC_CASES, ids=[c.name for c in OC_CASES])
def test_one_call_case_is_not_vacuous(case):
    T, g = cases.scan_text(), case.g
    kept, dropped = _one(case)
    n_keys = sum(kept.values())
    sizes = [rc.size_of(x, y) for x, y, _ in case.entries]
    order = sorted(case.entries, key=lambda e: e[2])
    if "drops" in case.tags:
        assert dropped > 0 and n_keys > 0
    if "no_drops" in case.tags:
        assert dropped == 0 and n_keys == sum(min(s, case.cap) for s in sizes)
    if "no_keys" in case.tags:
        assert n_keys == 0 and sizes == [0]
    if "periodic" in case.tags:
        assert n_keys > len(kept) and dropped < sum(min(s, case.cap) for s in sizes) - len(kept)     # duplicates survive
    if "cap" in case.tags:
        assert any(s > case.cap for s in sizes) and any(s == case.cap for s in sizes) and any(s < case.cap for s in sizes)
        assert {0, 1, 12, 70, case.cap - 1, case.cap, case.cap + 1} <= set(sizes)
    if "block_boundary" in case.tags:                               # entry 256 is dropped for what entry 255, in the workgroup before, leaves at row 0
        (xa, ya, ia), (xb, yb, ib) = order[255], order[256]
        assert _who(ia, g) == _who(ib, g) and ya >= xa and yb >= xb
        assert rc.key_of(T.sa[xa], ia, g) == rc.key_of(T.sa[xb], ib, g)
    if "permuted" in case.tags:
        assert [e[2] for e in case.entries] != [e[2] for e in order]
    if "one_per_row" in case.tags:
        assert len(set(sizes)) == 1 and len(kept) == n_keys == min(sizes[0], case.cap) and dropped == (len(sizes) - 1) * n_keys
    if "both_strands" in case.tags:
        fw = {_who(i, g)[0] for (x, y, i), s in zip(case.entries, sizes) if s and not i >> 31}
        assert fw & {_who(i, g)[0] for (x, y, i), s in zip(case.entries, sizes) if s and i >> 31}
        assert {sel.key_strand(k) for k in kept} == {0, 1}
    if "strand_neighbours" in case.tags:
        (xa, _, ia), (xb, _, ib) = order[7], order[8]
        assert _who(ia, g)[0] == _who(ib, g)[0] and (ia >> 31, ib >> 31) == (0, 1)
        assert _field(rc.key_of(T.sa[xa], ia, g)) == _field(rc.key_of(T.sa[xb], ib, g))
        assert n_keys == 2 and dropped == 14
    if "equal_fields" in case.tags:
        assert len(kept) == 2 and len({_field(k) for k in kept}) == 1 and len({sel.key_read(k) for k in kept}) == 2
    if "short_previous" in case.tags:
        assert sizes == [2, 12] and dropped == 2 and n_keys == 2 + 6
    if "text_start" in case.tags:
        assert sum(1 for k in kept if _field(k) < sel.BIAS) >= 2
        assert {0, cases.N_TEXT - 1} <= {int(T.sa[x]) for x, y, _ in case.entries if x == y}
    if "field_at_bias" in case.tags:
        assert any(_field(k) == sel.BIAS for k in kept) and g.read_len - g.seed_len == sel.MAX_SEED_OFFSET
        assert {sel.key_strand(k) for k in kept} == {0, 1}
    if "ragged" in case.tags:
        lengths = np.diff(g.read_offsets.astype(np.int64))
        assert lengths.min() == 30 and lengths.max() == 200 and len(set(g.intervals.tolist())) > 4
        assert {sel.key_strand(k) for k in kept} == {0, 1}


def test_large_case_is_not_vacuous():
    T = cases.scan_text()
    x, y, ids = cases.large_case()
    assert len(ids) == cases.LARGE_N > 8192 * 256 and len(set(ids.tolist())) == len(ids)
    assert (np.diff(ids) < 0).any()                                 # handed over unsorted
    keys, dropped = rc.one_call_keys_cap1(T, x, y, ids, cases.G_LARGE)
    emptied = int((y < x).sum())
    assert emptied > 50000 and dropped > 1000000 and len(keys) + dropped + emptied == cases.LARGE_N
    # a chain that an emptied range breaks: more keys survive than one per read on a diagonal
    reads = cases.LARGE_N // cases.G_LARGE.spr
    assert len(keys) > reads + emptied // 2
    assert {int(k >> 33) & 1 for k in keys[:: 997]} == {0, 1}


def test_two_call_cases_are_not_vacuous():
    T = cases.scan_text()
    by = {c.name: c for c in TC_CASES}
    plain = by["plain"]
    slots = [int(v) for v in rc.inclusive_sizes(plain.ranges)]
    total = slots[-1]
    sizes = [rc.size_of(x, y) for x, y in plain.ranges]
    big = sizes.index(5000)
    assert (slots[big] - 5000) // cases.TILE == 0 and (slots[big] - 1) // cases.TILE == 2         # the large range spans three tiles
    assert sizes[:3] == [0, 0, 0] and sizes[-4:] == [0, 0, 0, 0] and any(sizes[i:i + 5] == [0] * 5 for i in range(4, len(sizes) - 9))
    w = set(plain.windows)
    assert (0, total) in w and (0, 1) in w and (total - 1, total) in w
    for m in (cases.TILE, 2 * cases.TILE):
        assert {m - 1, m, m + 1} <= {b for b, _ in w} | {0} and {m - 1, m, m + 1} <= {e for _, e in w}
    assert {cases.TILE - 1, cases.TILE, cases.TILE + 1} <= {b for b, _ in w}
    for name in ("ids_strand_0", "ids_strand_1", "direct_ids"):
        c = by[name]
        assert list(c.ids) != list(range(len(c.ids))) and {i >> 31 for i in c.ids} == {0, 1}
        assert {sel.key_strand(k) for k in rc.two_call_keys(T, list(c.ranges), c.ids, c.direct, c.strand, c.geoms[0])} == {0, 1}
    assert by["ids_strand_0"].strand == 0 and by["ids_strand_1"].strand == 1
    for name, twin in (("direct", "plain"), ("direct_ids", "ids_strand_1")):
        c = by[name]
        assert 10 < sum(c.direct) < sum(1 for x, y in c.ranges if x == y)
        assert c.ranges != by[twin].ranges and cases.plain_of(c) == by[twin].ranges
        for g in c.geoms:                                           # a range that holds its position gives the key its row gives
            assert rc.two_call_keys(T, list(c.ranges), c.ids, c.direct, c.strand, g) == rc.two_call_keys(T, list(by[twin].ranges), c.ids, None, c.strand, g)
        flagged = [i for i, d in enumerate(c.direct) if d]
        walked = [i for i, s in enumerate(sizes) if s > 1]
        assert any(a < i < b and slots[b] // cases.TILE == slots[a] // cases.TILE for i in flagged for a in walked for b in walked)
    assert rc.inclusive_sizes(by["single_output"].ranges).tolist() == [1]
    for c in TC_CASES:
        assert c.geoms[0].read_offsets is None and c.geoms[1].read_offsets is not None
