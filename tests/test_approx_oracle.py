"""CPU: the oracle's hamming_backtrack and its restated approximate seed mapper (orc_map_approx_read, restated from device-only mapping_inl.h)
against the text scans of approx_cpu.py, which know nothing about FM indices, on every case of approx_cases.py.  Exact: counts, numbers of
ranges, sets of ranges, multisets of hits and reseed bits.  Then the proofs that the cases are what their names say: the stack cases peak at 128
and 129 entries, every family reports several ranges somewhere, max_hits bites where a case says so."""
import numpy as np
import pytest

import approx_cases as cases
import approx_cpu as ap

_IDX = {}


def _index(orc, name, reverse=False):
    if (name, reverse) not in _IDX:
        t = cases.text(name)
        _IDX[name, reverse] = orc.build_index(t[::-1].copy() if reverse else t)
    return _IDX[name, reverse]


BT_CASES = [c for c in cases.backtrack_cases() if not c.quirks]
MP_CASES = list(cases.mapper_cases())
_BT_SEEN, _MP_SEEN = {}, {}


def test_suffix_array_is_the_sorted_suffixes():
    """the scans' own footing: the prefix-doubling suffix array equals a sort of the suffixes as Python tuples"""
    for name in ("rand65", "period2", "two_letter", "t70"):
        t = cases.text(name)
        want = sorted(range(len(t) + 1), key=lambda p: tuple(t[p:]))
        assert np.array_equal(ap.suffix_array(t), want), name
    assert np.array_equal(ap.suffix_array(np.zeros(0, np.uint8)), [0])


def test_every_case_has_a_name_and_a_reason():
    for cs in (cases.backtrack_cases() + (cases.overflow_case(),), cases.mapper_cases()):
        names = [c.name for c in cs]
        assert len(set(names)) == len(names)
        assert all(len(c.reason) > 10 and "\n" not in c.reason for c in cs)
    assert all(len(cases.text(c.text)) < (1 << 20) for c in cases.backtrack_cases() + cases.mapper_cases())
    assert all(c.lead >= 64 for c in cases.backtrack_cases() if c.quirks)           # quirks mode never starts at the stream's beginning


@pytest.mark.parametrize("case", BT_CASES, ids=[c.name for c in BT_CASES])
def test_backtrack_oracle_equals_the_scan(orc, case):
    hidx, st = _index(orc, case.text), cases.scan_text(case.text)
    stream, offs = cases.stream_of(case)
    most = 0
    for i, q in enumerate(case.queries):
        count, n, ranges = ap.backtrack_scan(st, q, case.seed, case.mm)
        c, k, rg = orc.hamming_backtrack(hidx, stream, int(offs[i]), len(q), case.seed, case.mm, cap=2048)
        assert (c, k) == (count, n), (case.name, i)
        assert k <= 2048 and set(map(tuple, rg.tolist())) == ranges and len(rg) == len(ranges), (case.name, i)
        assert ap.backtrack_stack_peak(cases.text(case.text), q, case.seed, case.mm) <= ap.STACK_ENTRIES, (case.name, i)
        most = max(most, n)
    _BT_SEEN[case.name] = most


def test_backtrack_cases_are_not_vacuous(orc):
    t = cases.text("poly_t")
    # the stack exactly full, and one entry more: re-derived from the model of the walk, and what the full case must find
    assert ap.backtrack_stack_peak(t, cases.poly_t_query(127), cases.STACK_SEED, 1) == 128
    assert ap.backtrack_stack_peak(t, cases.poly_t_query(128), cases.STACK_SEED, 1) == 129
    st = cases.scan_text("poly_t")
    count, n, _ = ap.backtrack_scan(st, cases.poly_t_query(127), cases.STACK_SEED, 1)
    assert (count, n) == (59, 2)
    over = cases.overflow_case()
    assert ap.backtrack_stack_peak(t, over.queries[0], over.seed, over.mm) == ap.STACK_ENTRIES + 1
    # every family reports more than one range for some query
    fam = {}
    for c in BT_CASES:
        if c.name not in _BT_SEEN:
            _BT_SEEN[c.name] = max(ap.backtrack_scan(cases.scan_text(c.text), q, c.seed, c.mm)[1] for q in c.queries)
        fam[c.family] = max(fam.get(c.family, 0), _BT_SEEN[c.name])
    assert all(v > 1 for v in fam.values()), fam
    # mismatches >= len from the whole index: every len-mer of the text, every place
    for c in BT_CASES:
        if c.family == "all_lenmers":
            st = cases.scan_text(c.text)
            for q in c.queries:
                count, n, _ = ap.backtrack_scan(st, q, c.seed, c.mm)
                assert count == st.n - len(q) + 1 and n == len(np.unique(st.windows(len(q)), axis=0))
    # the ends: the first query sits at position 0, the second ends at n
    for c in BT_CASES:
        if c.family == "ends":
            st = cases.scan_text(c.text)
            for q, p in ((c.queries[0], 0), (c.queries[1], st.n - len(c.queries[1]))):
                _, _, ranges = ap.backtrack_scan(st, q, c.seed, c.mm)
                assert any(lo <= st.row[p] <= hi for lo, hi in ranges), c.name
    # the truncated cases cut something: the widest query has at least 3 ranges, and a query without ranges follows one with several
    for c in BT_CASES:
        if c.family == "truncated":
            ns = [ap.backtrack_scan(cases.scan_text(c.text), q, c.seed, c.mm)[1] for q in c.queries]
            assert max(ns) >= 3 and any(a > 1 and b == 0 for a, b in zip(ns, ns[1:])), ns


def test_quirks_walks_stay_in_the_lead_in():
    """quirks mode walks on past the start of a query through the symbols before it.  A branch gets k symbols past the start only if the query with
    those k symbols in front occurs in the text within the mismatch bound; none does with k = 24, so no walk leaves the 64 symbols of lead-in"""
    qc = [c for c in cases.backtrack_cases() if c.quirks]
    assert qc
    for c in qc:
        st = cases.scan_text(c.text)
        stream, offs = cases.stream_of(c)
        for i, q in enumerate(c.queries):
            b = int(offs[i])
            assert b >= 64 and ap.backtrack_scan(st, stream[b - 24:b + len(q)], c.seed, c.mm)[0] == 0, (c.name, i)


@pytest.mark.parametrize("case", MP_CASES, ids=[c.name for c in MP_CASES])
def test_map_approx_oracle_equals_the_scan(orc, case):
    hidx, ridx = _index(orc, case.text), _index(orc, case.text, True)
    fwd, rev = cases.scan_text(case.text), cases.scan_text(case.text, True)
    p = case.p
    seed_off = p["first_offset"] + np.arange(p["seeds_per_read"]) * p["seed_interval"]
    totals, reseeds = [], []
    for r, stored in enumerate(case.reads):
        hits, rsum, rcount, reseed = ap.map_approx_scan(fwd, rev, stored, p)
        assert rcount <= cases.worst_hits(p["seeds_per_read"], p["seed_len"])
        deque, got_reseed = orc.map_approx_read(hidx, ridx, stored, seed_off, p["seed_len"], case.max_hits, p["rep_seeds"])
        assert got_reseed == reseed, (case.name, r)
        if case.max_hits >= rcount:
            assert sorted(map(tuple, deque.tolist())) == hits, (case.name, r)
        else:
            assert len(deque) == case.max_hits, (case.name, r)      # which hits survive is the deque's business
        totals.append(rcount)
        reseeds.append(reseed)
    _MP_SEEN[case.name] = (totals, reseeds)


def _seen(case):
    if case.name not in _MP_SEEN:
        fwd, rev = cases.scan_text(case.text), cases.scan_text(case.text, True)
        res = [ap.map_approx_scan(fwd, rev, s, case.p) for s in case.reads]
        _MP_SEEN[case.name] = ([x[2] for x in res], [x[3] for x in res])
    return _MP_SEEN[case.name]


def test_mapper_cases_are_not_vacuous():
    by = {c.name: c for c in MP_CASES}
    for c in MP_CASES:
        totals, reseeds = _seen(c)
        bites = c.max_hits < cases.worst_hits(c.p["seeds_per_read"], c.p["seed_len"]) - 1
        if bites:
            assert max(totals) > c.max_hits, c.name                 # some deque is offered more than it may hold
        else:
            assert max(totals) <= c.max_hits and max(totals) > 0, c.name
        if c.family == "full":
            assert all(t == 20 * c.p["seeds_per_read"] for t in totals), c.name
    # an N kills exactly the searches it should: the clean copies (rows 8, 9 = rows 0, 1 without the N) find more
    for name in ("n_before_len1", "n_at_len1", "n_at_len1_up", "two_n"):
        totals, _ = _seen(by[name])
        assert totals[0] < totals[8] and totals[1] < totals[9], name
    assert all(t == 0 for t in _seen(by["two_n"])[0][:8])
    assert any(t > 0 for t in _seen(by["n_before_len1"])[0][:8]) and any(t > 0 for t in _seen(by["n_last"])[0][:8])
    # the reseed rule: one read sits exactly on the boundary and flips with rep_seeds + 1; the read of N's has no range and reseeds
    at, above = by["reseed_at_boundary"], by["reseed_above_boundary"]
    fwd, rev = cases.scan_text(at.text), cases.scan_text(at.text, True)
    exact = [r for r, s in enumerate(at.reads) if (lambda x: x[2] and x[1] == at.p["rep_seeds"] * x[2])(ap.map_approx_scan(fwd, rev, s, at.p))]
    assert exact and all(_seen(at)[1][r] and not _seen(above)[1][r] for r in exact)
    assert _seen(at)[0][-1] == 0 and _seen(at)[1][-1] and _seen(above)[1][-1]
    assert not all(_seen(at)[1]) and not all(_seen(above)[1])
    # the queue names a strict subset, out of order
    for c in MP_CASES:
        if c.queue is not None:
            assert len(set(c.queue.tolist())) == len(c.queue) < len(c.reads) and not np.array_equal(c.queue, np.sort(c.queue))
    # odd seed lengths are there, and the position field is filled to its top
    assert {c.p["seed_len"] for c in MP_CASES if c.family == "seed_len"} == {1, 2, 3, 5, 12, 21, 31, 32}
    c = by["read_len_1023"]
    flags = [f for pos in (0, 1002) for *_, f in ap.seed_searches(c.reads[0], 1023, pos, 21)]
    assert max((f >> 20) & 0x3FF for f in flags) == 1022
