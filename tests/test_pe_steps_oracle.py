"""CPU: pins the restatement of the paired-end loop's steps (pe_steps_cpu.py) without a GPU.  On every input a real genome produces it is tied to the
oracle through the loop built from it (best_approx_paired_ragged_cpu.py, pinned by test_best_approx_paired_ragged_oracle.py); here: hand-worked answers
for the inputs that loop cannot reach, agreement of the opposite window with selection_cpu.opposite_window where both are defined, and the proof that
the fixed lists of pe_steps_cases.py reach every branch of the reduce and every reason an opposite job does not run -- the condition that keeps
test_gpu_pe_steps.py from testing nothing."""
import itertools

import pe_steps_cases as cases
import pe_steps_cpu as pe
import selection_cpu as sel

U32 = 0xFFFFFFFF
E2E = pe.Params(0, pe.SCORE_MIN, pe.WORST_SCORE, 0, -8, -3, 31, U32, pe.FR, 0, 500, 1, 1, 15, 30, 400)


def test_init_puts_mate_in_the_rc_slot_of_best_o():
    a, o = pe.init(-61, -19)
    assert a == ((-61, U32, 255, 0, 0, 0),) * 2 and o == ((-19, U32, 255, 1, 0, 0),) * 2
    assert pe.flags_word(a[0]) == 0 and pe.flags_word(o[0]) == 1


def test_target_score_truncates_toward_zero():
    # alignment_utils.h:100-101: second + delta * 3 / 4 in int32: 3/4 = 0, 6/4 = 1, 9/4 = 2, 15/4 = 3, -3/4 = 0 (not -1), -15/4 = -3 (not -4)
    for delta, want in ((1, 0), (2, 1), (3, 2), (5, 3), (-1, 0), (-5, -3)):
        a1, o1 = pe.aln(-10, 100, 99, 0, 0, True), pe.aln(-20, 300, 99, 1, 1, True)
        a2, o2 = pe.aln(-10 - delta, 900, 99, 0, 0, True), pe.aln(-20, 1100, 99, 1, 1, True)
        assert pe.target_score([a1, a2, o1, o2], -60, -90) == (-30 - delta) + want
    # :96-97 no second PAIR: the two worst scores; an unpaired second alignment is no pair
    assert pe.target_score([a1, pe.aln(-12, 900, 99, 0, 0, False), o1, o2], -60, -90) == -150
    assert pe.target_score([a1, pe.aln(-12, U32, 99, 0, 0, True), o1, o2], -60, -90) == -150


def test_frame_of_every_policy():
    # alignment_utils.h:61-87, (anchor, anchor_fw) -> (left, fw)
    want = {pe.FF: {(0, 1): (0, 1), (0, 0): (1, 0), (1, 1): (1, 1), (1, 0): (0, 0)},
            pe.RR: {(0, 1): (1, 1), (0, 0): (0, 0), (1, 1): (0, 1), (1, 0): (1, 0)},
            pe.FR: {(0, 1): (0, 0), (0, 0): (1, 1), (1, 1): (0, 0), (1, 0): (1, 1)},
            pe.RF: {(0, 1): (1, 0), (0, 0): (0, 1), (1, 1): (1, 0), (1, 0): (0, 1)}}
    for policy, table in want.items():
        for (anchor, fw), (left, ofw) in table.items():
            assert pe.frame(policy, anchor, bool(fw)) == (bool(left), bool(ofw)), (policy, anchor, fw)


def test_max_text_gaps_by_hand():
    # utils_inl.h:150-166, match 2, open -8, extension -3, pattern 11: perfect 22
    assert pe.max_text_gaps(2, -8, -3, 23, 11) == 0                   # 22 < 23: return 0
    assert pe.max_text_gaps(2, -8, -3, 22, 11) == -1                  # 22 - 8 = 14 < 22: the loop does not turn, n - 1 = uint32( -1 ) -> int32 -1
    assert pe.max_text_gaps(2, -8, -3, 15, 11) == -1
    assert pe.max_text_gaps(2, -8, -3, 14, 11) == 0                   # 14 >= 14: one turn (11), n = 1
    assert pe.max_text_gaps(2, -8, -3, 5, 11) == 3                    # 14, 11, 8, 5 >= 5: four turns
    assert pe.max_text_gaps(2, -8, -3, -100, 11) == 10                # bounded by n < pattern_len: o_len - 1
    assert pe.max_text_gaps(0, -8, -3, -59, 100) == 17                # end to end, min_score( 100 ) + 1: -8 - 3 * 17 = -59 >= -59 eighteen turns
    # o_gapped_len = o_len + max_ref_gaps in uint32: -1 makes it o_len - 1
    assert pe.u32(11 + pe.max_text_gaps(2, -8, -3, 22, 11)) == 10


def test_opposite_window_near_2_32_and_near_zero_by_hand():
    # score_inl.h:410-413 right side, g = 0xFFFFFFF0, max_frag 500: end = uint32( g + 500 ) = 0x1E4 = 484; begin = g (overlap) -- min_begin = g + 0 - 110
    # is smaller -- so end < begin: the library's "not run"
    assert pe.opposite_frame_window(0xFFFFFFF0, False, 100, 110, 0, 500, 1, U32) == (0xFFFFFFF0, 484)
    assert pe.opposite_frame_window(0xFFFFFFF0, False, 100, 110, 0, 500, 0, U32) == (0xFFFFFFF0 - 110, 484)      # g + a_len wraps to 84, but min_begin = g - 110 is larger
    best = list(pe.init(-60, -90)[0] + pe.init(-60, -90)[1])
    row = pe.opposite_flatten(E2E, best, 0, 0xFFFFFFF0, -10, 100, 150, -60, -90, 0)      # FR, anchor forward: the opposite mate to the right, reverse
    assert row == (pe.READ_COMPLEMENT, 0, 0, -89, "wrapped")          # target_pair -150, less the anchor's -10: -140 -> max( -140, -90 ) + 1
    # :403-408 left side, g = 3, a_len 100, max_frag 500, min_frag 150, o_gapped 110: reach = 3 + 100 + 110 = 213 > 150 -> max_end = 63;
    # begin = 103 > 500 ? ... : 0; end = min( 103, 63 ) with overlap, min( 3, 63 ) without
    assert pe.opposite_frame_window(3, True, 100, 110, 150, 500, 1, U32) == (0, 63)
    assert pe.opposite_frame_window(3, True, 100, 110, 150, 500, 0, U32) == (0, 3)
    assert pe.opposite_frame_window(3, True, 100, 40, 150, 500, 1, U32) == (0, 0)         # reach 143 <= min_frag: max_end = 0, the empty window
    p = E2E._replace(min_frag=150)
    assert pe.opposite_flatten(p, best, 1, 3, -10, 100, 40, -60, -24, 0)[1:] == (0, 0, -23, "empty")        # ms -23: -8 - 3 * 5 = -23, six turns: gaps 5, 45 + 103 < 150
    assert pe.opposite_flatten(p, best, 1, 3, -10, 100, 100, -60, -60, 0)[:3] == (pe.READ_REVERSE, 0, 70)   # ms -59: gaps 17: reach 220 - 150 = 70; min( 103, 70 )


def test_anchor_window_and_output_by_hand():
    # score_inl.h:238-239: g = 0xFFFFFFF0, band 31: begin = g - 15; end = uint32( begin + 31 + 100 ) wraps to 0x64: a window that ends before it begins
    assert pe.anchor_window(0xFFFFFFF0, 31, 100, U32) == (0xFFFFFFE1, 0x64)
    best = list(pe.init(-60, -90)[0] + pe.init(-60, -90)[1])
    assert pe.anchor_flatten(E2E, best, 1, 0xFFFFFFF0, 100, -60, -90, 0) == (pe.READ_COMPLEMENT, 0, 0, -59)
    assert pe.anchor_flatten(E2E, best, 0, 15, 100, -60, -90, 0) == (pe.READ_REVERSE, 0, 131, -59)
    assert pe.anchor_flatten(E2E, best, 0, 16, 100, -60, -90, 0)[1:3] == (1, 132)
    assert pe.anchor_flatten(E2E._replace(genome_len=1000), best, 0, 1015, 100, -60, -90, 0)[1:3] == (0, 0)       # begins at genome_len
    assert pe.anchor_flatten(E2E._replace(genome_len=1000), best, 0, 1014, 100, -60, -90, 0)[1:3] == (999, 1000)
    # local: match 2: target_mate = max( (46 + 50) - 2 * 150, 46 ) = 46: the perfect score of the OPPOSITE mate is what is subtracted
    assert pe.anchor_flatten(E2E._replace(match=2, score_limit=0), best, 0, 500, 100, 46, 50, 300)[3] == 47
    assert pe.anchor_flatten(E2E._replace(match=2, score_limit=0), best, 0, 500, 100, -400, 50, 300)[3] == 0      # max( -400 + 1, score_limit )
    held = [pe.aln(-5, 500, 99, 0, 0, True)] + best[1:]
    assert pe.anchor_flatten(E2E, held, 0, 500, 100, -60, -90, 0) == (pe.READ_REVERSE, 0, 0, pe.INT32_MAX)       # a locus already held
    assert pe.anchor_flatten(E2E, held, 1, 500, 100, -60, -90, 0)[3] == -59
    # output: passed = score >= min_score; valid needs a score other than worst_score as well
    assert pe.anchor_output(-59, 7, 100, -59, -65536) == (-59, 107, -65536, 1)
    assert pe.anchor_output(-60, 7, 100, -59, -65536) == (-65536, 107, -65536, 0)
    assert pe.anchor_output(-65536, 7, U32, -65536, -65536) == (-65536, 6, -65536, 0)
    assert pe.anchor_output(0, U32, 0, pe.INT32_MAX, -65536) == (-65536, U32, -65536, 0)
    assert pe.opposite_output(-3, U32, 500, 900, -10, -65536) == (-3, 500, 500)
    assert pe.opposite_output(-3, 7, 0, 0, -10, -65536) == (-65536, 0, 7)         # a job that did not run: worst_score whatever its slot holds
    assert pe.opposite_output(-3, 7, 900, 100, -10, -65536) == (-65536, 900, 907)


def test_distinct_at_its_distance_by_hand():
    # alignments_inl.h:33-37: pos1 in [pos2 - min( pos2, dist ), pos2 + dist] is NOT distinct
    assert not pe.distinct(0, 0, 10, 0, 50) and not pe.distinct(60, 0, 10, 0, 50) and pe.distinct(61, 0, 10, 0, 50)        # pos2 < dist: clamped at 0
    assert not pe.distinct(950, 0, 1000, 0, 50) and pe.distinct(949, 0, 1000, 0, 50)                                         # exactly dist, dist + 1
    assert not pe.distinct(1050, 0, 1000, 0, 50) and pe.distinct(1051, 0, 1000, 0, 50)
    assert pe.distinct(1000, 1, 1000, 0, 50)
    # uint32: pos2 + dist wraps to 39 while pos2 - dist stays large, so NOTHING is near such a position, not even itself
    assert pe.distinct(U32 - 10, 0, U32 - 10, 0, 50) and pe.distinct(3, 0, U32 - 10, 0, 50) and not pe.distinct(U32 - 60, 0, U32 - 50, 0, 50)
    a, o = pe.aln(-5, 1000, 99, 0, 0, True), pe.aln(-6, 1300, 149, 1, 1, True)
    for da, do, want in ((50, 0, False), (51, 0, True), (-50, -50, False), (0, -51, True), (0, 0, False)):
        a2, o2 = pe.aln(-9, 1000 + da, 99, 0, 0, True), pe.aln(-9, 1300 + do, 149, 1, 1, True)
        assert pe.pairs_distinct(a, o, a2, o2, 50) == want and pe.pairs_distinct(a, o, a2, o2) == ((da, do) != (0, 0))
    # compared by MATE, not by role: the same pair found from the other anchor is the same pair
    assert not pe.pairs_distinct(a, o, pe.aln(-6, 1300, 149, 1, 1, True), pe.aln(-5, 1000, 99, 0, 0, True))


def test_reduce_keeps_the_reference_quirk_by_hand():
    # reduce_inl.h:262-273: an unpaired update writes memory, not the local best_pairs
    ia, io = pe.init(-60, -90)
    up = lambda pos, s: (pos, pos + 100, s, -65536, 0, 0, 0, 0)
    ba, bo, trys, erased, br = pe.reduce_read(E2E, list(ia + io), 2, [up(1000, -10), up(9000, -30)], 100, 0)
    assert br == ["unpaired-best", "unpaired-best"]                  # -30 > the LOCAL copy's -60
    assert ba == ((-30, 9000, 100, 0, 0, 0), ia[0]) and bo == io and trys == 2 and not erased
    ba, bo, trys, erased, br = pe.reduce_read(E2E, list(ia + io), 2, [up(1000, -10), (9000, 9100, -20, -30, 9300, 9450, 0, 0)], 100, 0)
    assert br == ["unpaired-best", "best"] and trys == 15
    assert ba == ((-20, 9000, 100, 0, 0, 1), ia[0]) and bo == ((-30, 9300, 150, 1, 1, 1), io[0])     # the unpaired write is overwritten
    # the failure counter (reduce.h:82-92): counted from min_ext on for hits without the top flag; max_ext stops whatever the flag says
    low = up(5000, -70)
    run = lambda ext, top, trys: pe.reduce_read(E2E._replace(min_ext=30, max_ext=40), list(ia + io), trys, [low[:7] + (top,)], 100, ext)[2:]
    assert run(29, 0, 2) == (2, False, ["unpaired-keep"]) and run(30, 0, 2) == (1, False, ["unpaired-keep"]) and run(30, 0, 1) == (0, True, ["unpaired-fail"])
    assert run(30, 1, 1) == (1, False, ["unpaired-keep"]) and run(40, 1, 1) == (1, True, ["unpaired-fail"]) and run(40, 0, 0) == (0, False, ["unpaired-keep"])
    assert run(40, 0, 2) == (1, True, ["unpaired-fail"]) and run(39, 1, 3) == (3, False, ["unpaired-keep"])


def test_opposite_window_agrees_with_the_selection_restatement():
    """the same g, a_len, o_gapped, policy, anchor, overlap and fragment limits, no threshold or visited test: wherever none of the reference's
    uint32 sums wraps (selection_cpu computes them unbounded) the two restatements give the same window -- over test_selection_oracle.py's product"""
    same = skipped = 0
    for G in (1_000_000, U32):
        gs = [0, 1, 99, 100, 101, 499, 500, 501, 5000, G - 1, G - 100, G - 501] + ([U32 - 300, U32 - 1] if G == U32 else [G, G + 7])
        for policy, anchor, rc, overlap, g in itertools.product(range(4), (0, 1), (0, 1), (False, True), gs):
            for a_len, o_len, lo, hi in ((100, 110, 0, 500), (100, 110, 0, 50), (100, 110, 400, 500), (150, 160, 2000, 3000), (1, 1, 0, 1)):
                if g + a_len + o_len > U32 or g + hi > U32 or g + lo > U32:
                    skipped += 1
                    continue
                left, fw = pe.frame(policy, anchor, rc == 0)
                begin, end = pe.opposite_frame_window(g, left, a_len, o_len, lo, hi, 1 if overlap else 0, G)
                ok = begin < G and begin < end
                want = sel.opposite_window(g, rc, a_len, o_len, anchor, policy, lo, hi, overlap, G)
                assert ((begin, end) if ok else (0, 0), 0 if fw else 3, 1 if ok else 0) == (want[:2], want[2], want[3]), (G, policy, anchor, rc, overlap, g, a_len)
                same += 1
    assert same > 3800 and 0 < skipped < same // 5


# ---- the lists prove their own coverage ---------------------------------------------------------------------------------------------
def test_flatten_lists_reach_every_reason_for_every_policy_and_anchor():
    configs = cases.flatten_configs()
    assert len(configs) == 144 and sum(1 for c in configs if c.scheme == "local") * 2 >= len(configs)            # the match * len terms are live in half
    assert {(c.policy, c.anchor, c.overlap, c.min_frag, c.max_frag) for c in configs} == set(itertools.product(range(4), (0, 1), (0, 1), cases.MIN_FRAGS, cases.MAX_FRAGS))
    for form in ("uniform", "ragged"):
        seen, gaps, anchors, thresholds = set(), set(), set(), set()
        for cfg in configs:
            L = cases.flatten_list(cfg, form)
            assert len(L["queue"]) % 64 != 0 and len(set(L["queue"])) == len(L["queue"]) < len(L["rid"]) and list(L["queue"]) != sorted(L["queue"])
            assert all(m1 != m2 for m1, m2 in zip(L["min1"], L["min2"]))
            if form == "ragged":
                assert sum(1 for a, o in zip(L["a_len"], L["o_len"]) if a != o) * 4 > 3 * len(L["a_len"]) and set(L["a_len"]) == set(cases.LENGTHS) == set(L["o_len"])
            else:
                assert len(set(L["a_len"])) == len(set(L["o_len"])) == len(set(L["min1"])) == len(set(L["min2"])) == 1
            for row in cases.want_opposite_flatten(L):
                r, flags, wb, we, ms, reason, g = row
                seen.add((reason, cfg.policy, cfg.anchor, flags))
                o_opt = L["p"].match * L["o_len"][r]
                thresholds.add((cfg.scheme, ms - o_opt) if abs(ms - o_opt) <= 1 else None)
                if reason is None:
                    gaps.add((cfg.scheme, "cap" if g == L["o_len"][r] - 1 and g > 3 else g if g in (-1, 0, 3) else None))
                    assert wb < we <= cfg.genome_len
                else:
                    assert (wb, we) == (0, 0)
            for r, flags, wb, we, ms in cases.want_anchor_flatten(L):
                anchors.add((cfg.anchor, "skip" if ms == pe.INT32_MAX else "empty" if (wb, we) == (0, 0) else "clamped" if we == cfg.genome_len else "plain", flags))
                assert (wb, we) == (0, 0) or wb < we <= cfg.genome_len
        for reason in (None,) + pe.REASONS:
            for policy, anchor in itertools.product(range(4), (0, 1)):
                assert {f for (w, p, a, f) in seen if (w, p, a) == (reason, policy, anchor)} == {pe.READ_REVERSE, pe.READ_COMPLEMENT}, (form, reason, policy, anchor)
        for scheme in ("e2e", "local"):
            assert {(scheme, d) for d in (-1, 0, 1)} <= thresholds, (form, scheme)
            # (o_len - 1 gaps need a threshold below perfect - 8 - 3 (o_len - 1) < 0: score_limit = 0 keeps the local lists above it)
            assert {(scheme, g) for g in (-1, 0, 3) + (("cap",) if scheme == "e2e" else ())} <= gaps, (form, scheme)
        assert anchors == set(itertools.product((0, 1), ("skip", "empty", "clamped", "plain"), (pe.READ_REVERSE, pe.READ_COMPLEMENT))), form


def test_reduce_lists_reach_every_branch_for_every_policy_and_anchor():
    configs = cases.reduce_configs()
    assert {(c.policy, c.anchor, c.unpaired, c.ext) for c in configs} == set(itertools.product(range(4), (0, 1), (0, 1), cases.EXTS))
    for form in ("uniform", "ragged"):
        seen, orders, erased_at = set(), set(), set()
        for cfg in configs:
            L = cases.reduce_list(cfg, form)
            assert {c for c in L["count"]} >= set(cases.HIT_COUNTS) and any(a >> 31 for a in L["active"]) and len(L["active"]) < len(L["best"])
            firsts = sorted(zip(L["first"], L["count"]))
            assert list(L["first"]) != sorted(L["first"]) and any(f + c < g for (f, c), (g, _) in zip(firsts, firsts[1:]))       # not contiguous
            want, branches = cases.want_reduce(L)
            for t, br in enumerate(branches):
                r = L["active"][t] & 0x7FFFFFFF
                seen.update((b, cfg.policy, cfg.anchor) for b in br)
                orders.update(zip(br, br[1:]))
                if want[r][3]:
                    erased_at.add((cfg.ext, L["trys"][r]))
        for branch, policy, anchor in itertools.product(pe.BRANCHES, range(4), (0, 1)):
            assert (branch, policy, anchor) in seen, (form, branch, policy, anchor)
        assert {("unpaired-best", "unpaired-best"), ("unpaired-best", "best"), ("best", "unpaired-keep"), ("second", "best")} <= orders | {(a, "unpaired-keep") for a, b in orders if b == "keep"}, form
        assert {e for e, _ in erased_at} >= {cases.MIN_EXT, cases.MAX_EXT - 1, cases.MAX_EXT} and {t for _, t in erased_at} >= {1, 2, cases.MAX_EFFORT}
