"""GPU: the band-31 end-to-end shortcuts -- the ungapped first pass, the second, third and gap chance, the DP's narrow classes and their redo list
(csrc/band31_*.hip) -- over the space of the three scheme numbers their arguments rest on: P, the smallest mismatch penalty, and the gap's
opening and extension terms go and ge.

Every check is integer equality: scores and sinks against the oracle (the reference algorithm, band 31, SEMI_GLOBAL: orc.banded_gotoh_packed_batch,
itself pinned on the reference's host code under every scheme used here by tests/test_oracle_vs_reference.py::test_e2e31_scheme_sweep), and the
route report of nvbio_banded_gotoh_score_routes against util.e2e31_first_pass, the first pass's rule restated in numpy as the code has it:
a job the rule flags 0 is reported ROUTE_SETTLED, a job it flags 1 is reported on the DP route of the rule's class (ROUTE_REDONE may be added to a
class), and a job it hands to a chance (flags 2, 3, 4) may end either way.  Whether a chance's argument is RIGHT under a scheme is what the
comparison with the oracle decides; the report makes sure the comparison is of the route meant, and that a scheme the host keeps off the
shortcuts (P = 0; a step too large for the int16 lanes) is reported as the DP's throughout.

The jobs are util.e2e31_sweep_jobs(): tests/test_e2e31_sweep_jobs.py asserts on the CPU that they reach every flag and class a scheme's rule can
give.  The schemes are the 138 of util.E2E31_SWEEP (test_grid) and the corners of util.E2E31_CORNERS (every other test).

What the sweep found: under P = 0 the first pass settled every job on its fewest-mismatch diagonal while the reference's sink is the last
reportable column (3,950 of 4,701 jobs wrong); ungapped_ok() now keeps mm_min = 0 off the shortcuts, which test_grid[0], test_corners[p0*] and
test_qualities[ramp_0_6] hold it to.

Five one-scalar edits of the rule, each run once on a scratch build: `gmax <= 4` -> 5: wrong results under ge = 0 (test_grid, test_corners[ge0]) and
the report elsewhere (test_corners[ge0_p1]); `ge < go` dropped from `beyond`: the report alone (test_grid[1, 2, 3, 6], test_corners[open_below_ext_p1]);
`2 G < U` -> <=: the report alone (test_grid[2], test_corners[two_gaps_tie]); `cap` + 1 and GAP_CHANCE_GA = 6 in gap_chance_unknown_cost: not
seen -- the first changes no result and only moves a chance's job to the DP, the second needs a six-symbol gap that ties an evaluated member of
cost Cg(6) .. Cg(7) - 1, which the pool does not hold."""
import numpy as np
import pytest

import oracle
from util import (ALN_NO_F16_DP, ALN_NO_GAP_CHANCE, ALN_NO_NARROW_DP, ALN_NO_PAIRED_GAP_CHANCE, ALN_NO_QUALITY_SHORTCUT, ALN_NO_SECOND_CHANCE,
                  ALN_NO_THIRD_CHANCE, ALN_NO_UNGAPPED_SCORE, ALN_PK_THREE_WAVES, ALN_SPLIT_CHANCES, E2E31_CORNERS, E2E31_SWEEP, e2e31_admitted, e2e31_counts,
                  e2e31_first_pass, e2e31_layout, e2e31_possible_flags, e2e31_sweep_jobs)

pytestmark = pytest.mark.gpu

SEED = 1
SETTLED, FULL, CLASS_A, CLASS_B, REDONE = 0, 1, 2, 3, 8
CLASS_ROUTE = np.array([FULL, CLASS_B, CLASS_A])                     # the rule's class (0 none, 1 = B, 2 = A) -> the route's low bits
# switch -> the rule's flags whose jobs may be settled under default flags and the DP's under the switch
SWITCHES = (("default", 0, ()), ("no_second", ALN_NO_SECOND_CHANCE, (3,)), ("no_third", ALN_NO_THIRD_CHANCE, (2,)), ("no_gap", ALN_NO_GAP_CHANCE, (2, 4)),
            ("no_paired_gap", ALN_NO_PAIRED_GAP_CHANCE, (4,)), ("split", ALN_SPLIT_CHANCES, ()), ("no_narrow", ALN_NO_NARROW_DP, ()),
            ("no_f16", ALN_NO_F16_DP, ()), ("three_waves", ALN_PK_THREE_WAVES, ()))


class _Pool:
    """the jobs, their layouts (all jobs declared as 162 symbols long; the M = 64 jobs alone, declared as 64), and what is computed once and
    shared: the diagonals' counts, the oracle's results per scheme, the device batches per switch"""

    def __init__(self, orc):
        self.orc = orc
        self.J = J = e2e31_sweep_jobs(SEED)
        self.M = J["M"].astype(np.int64)
        self.N = np.array([len(t) for t in J["txts"]], dtype=np.int64)
        self.C = e2e31_counts(J)
        self.idx = {"all": np.arange(len(self.M)), "m64": np.nonzero(self.M == 64)[0],
                    "acgt": np.nonzero([not (p == 4).any() for p in J["pats"]])[0]}
        self._layouts, self._wants, self._weights, self._batches = {}, {}, {}, {}

    def layout(self, which, with_q=False, bits=4):
        key = (which, with_q, bits)
        if key not in self._layouts:
            self._layouts[key] = e2e31_layout(self.orc, self.J, self.idx[which], with_q, bits)
        return self._layouts[key]

    def want(self, sv, which, with_q=False):
        key = (tuple(sv), which, with_q)
        if key not in self._wants:
            d = self.layout(which, with_q)
            self._wants[key] = self.orc.banded_gotoh_packed_batch(31, oracle.SEMI_GLOBAL, oracle.Scheme(*sv), d["reads4"], d["roffs"], d["text"], d["wb"],
                                                                  d["we"], quals=d["quals"])
        return self._wants[key]

    def rule(self, sv, which, with_q, algo):
        """(flag, class, admitted) per job of the layout under a switch"""
        d = self.layout(which, with_q)
        i = d["idx"]
        if with_q and tuple(sv) not in self._weights:
            self._weights[tuple(sv)] = e2e31_counts(self.J, sv)
        W = self._weights[tuple(sv)][i] if with_q else None
        flag, cls = e2e31_first_pass(sv, with_q, self.M[i], self.N[i], self.C[i], weights=W, max_read_len=d["max_len"], algo=algo)
        return flag, cls, e2e31_admitted(sv, with_q, d["max_len"], algo)

    def batch(self, amd, which, with_q, algo, bits=4):
        key = (which, with_q, algo, bits)
        if key not in self._batches:
            d = self.layout(which, with_q, bits)
            self._batches[key] = amd.AlignmentBatch(d["reads"], bits, d["roffs"], d["text"], 2, d["wb"], d["we"], quals=d["quals"], max_read_len=d["max_len"],
                                                    algo_flags=algo)
        return self._batches[key]

    def run(self, amd, sv, which, with_q, algo, bits=4):
        """scores and sinks equal the oracle's -> the route report"""
        sc, sk, rt = amd.banded_gotoh_score_routes(31, amd.make_gotoh_aligner(oracle.SEMI_GLOBAL, amd.GotohScheme(*sv)), self.batch(amd, which, with_q, algo, bits))
        sc, sk, rt = sc.cpu().numpy(), amd.u32(sk), rt.cpu().numpy()
        want_s, want_k = self.want(sv, which, with_q)
        bad = np.nonzero((sc != want_s) | (sk != want_k).any(axis=1))[0]
        i = self.layout(which, with_q, bits)["idx"][bad[:5]]
        assert len(bad) == 0, (sv, which, with_q, algo, len(bad), i, self.J["kind"][i], self.M[i], rt[bad[:5]], sc[bad[:5]], want_s[bad[:5]], sk[bad[:5]],
                               want_k[bad[:5]])
        return rt

    def check_routes(self, sv, which, with_q, algo, rt):
        """the report against the rule -> the rule's flags"""
        flag, cls, admitted = self.rule(sv, which, with_q, algo)
        if not admitted:
            assert (rt == FULL).all(), (sv, which, algo, np.bincount(rt, minlength=12))
            return flag
        assert (rt[flag == 0] == SETTLED).all(), (sv, which, algo, np.bincount(rt[flag == 0], minlength=12))
        dp = flag == 1
        assert ((rt[dp] & 7) == CLASS_ROUTE[cls[dp]]).all() and not (rt[dp & (cls == 0)] & REDONE).any(), (sv, which, algo, np.bincount(rt[dp], minlength=12), np.bincount(cls[dp]))
        assert np.isin(rt[flag >= 2], (SETTLED, FULL)).all(), (sv, which, algo)
        if algo & ALN_NO_THIRD_CHANCE:
            assert (rt[flag == 2] == FULL).all(), (sv, which, algo)  # flag 2 has no launch to go to
        return flag


@pytest.fixture(scope="module")
def pool(orc):
    return _Pool(orc)


@pytest.mark.parametrize("P", sorted({sv[1] for sv in E2E31_SWEEP}))
def test_grid(amd, pool, P):
    """the 23 (go, ge) of the grid under one mismatch penalty: default flags and the DP alone"""
    schemes = [sv for sv in E2E31_SWEEP if sv[1] == P]
    assert len(schemes) == 23
    settled = dp_class = 0
    for sv in schemes:
        rt = pool.run(amd, sv, "all", False, 0)
        flag = pool.check_routes(sv, "all", False, 0, rt)
        settled += int((rt == SETTLED).sum()); dp_class += int(np.isin(rt & 7, (CLASS_A, CLASS_B)).sum())
        off = pool.run(amd, sv, "all", False, ALN_NO_UNGAPPED_SCORE)
        assert (off == FULL).all()
    print("P", P, "settled", settled, "class jobs", dp_class, "of", 23 * len(pool.M))
    assert (settled > 0) == (P > 0)                                   # a mismatch that costs nothing is kept off the shortcuts


@pytest.mark.parametrize("name,sv,with_q", E2E31_CORNERS, ids=[c[0] for c in E2E31_CORNERS])
def test_corners(amd, pool, name, sv, with_q):
    """a corner scheme under every switch of the stage, on the whole pool declared as 162 symbols and on its M = 64 jobs declared as 64 (the binary16
    DP and the classes wherever the scheme admits them)"""
    for which in ("all", "m64"):
        base_rt = base_flag = None
        for switch, algo, lost_flags in SWITCHES:
            rt = pool.run(amd, sv, which, with_q, algo)
            flag = pool.check_routes(sv, which, with_q, algo, rt)
            if switch == "default":
                base_rt, base_flag = rt, flag
                print("%-22s %-4s jobs per flag %s settled per flag %s routes %s" % (name, which, np.bincount(flag, minlength=5),
                                                                                  np.bincount(flag[rt == SETTLED], minlength=5), np.bincount(rt, minlength=12)))
                continue
            lost = (base_rt == SETTLED) & (rt != SETTLED)
            assert np.isin(base_flag[lost], lost_flags).all(), (name, which, switch, np.bincount(base_flag[lost], minlength=5))


RAMPS = [c for c in E2E31_CORNERS if c[2]]


@pytest.mark.parametrize("name,sv", [(c[0], c[1]) for c in RAMPS] + [("ramp_0_6", (0, 0, 6, -8, -3, -8, -3))])
def test_qualities(amd, pool, name, sv):
    """quality ramps on the pool's qualities: the first pass sums the candidate diagonals' rows from the quality bytes.  The ramp 0..6 is run
    without qualities (every mismatch costs 0) and with them (a smallest penalty of 0: kept off the shortcut)"""
    assert len(RAMPS) == 3
    for with_q in ((False, True) if sv[1] == 0 else (True,)):
        for algo in (0, ALN_NO_QUALITY_SHORTCUT, ALN_NO_GAP_CHANCE):
            rt = pool.run(amd, sv, "all", with_q, algo)
            flag = pool.check_routes(sv, "all", with_q, algo, rt)
            if sv[1] == 0 or algo & ALN_NO_QUALITY_SHORTCUT:
                assert (rt == FULL).all()
            else:
                assert int((rt == SETTLED).sum()) >= 100 and int(((flag == 2) | (flag == 3)).sum()) >= 20 and not (flag == 4).any()


LINEAR = [(P, g) for P in (1, 2, 5) for g in (1, 2, 5)]


@pytest.mark.parametrize("P,g", LINEAR + [(None, None)], ids=["sw_%d_%d" % pg for pg in LINEAR] + ["edit_distance"])
def test_linear_gap_entry_points(amd, orc, pool, P, g):
    """nvbio_banded_sw_score with deletion == insertion, and the edit-distance aligner, take the shortcuts as Gotoh( open = extension ): every job
    against orc.banded_sw, 4-bit reads and (the jobs without an N) 2-bit reads; the route report of the equal Gotoh scheme shows which jobs the
    shortcuts settled"""
    sw = (0, -1, -1, -1) if P is None else (0, -P, -g, -g)
    aligner = amd.make_edit_distance_aligner(oracle.SEMI_GLOBAL) if P is None else amd.make_smith_waterman_aligner(oracle.SEMI_GLOBAL, amd.SimpleSmithWatermanScheme(*sw))
    sv = (0, -sw[1], -sw[1], sw[2], sw[2], sw[2], sw[2])
    J = pool.J
    want = np.array([[s, k[0], k[1]] for ok, s, k in (orc.banded_sw(31, oracle.SEMI_GLOBAL, sw, J["pats"][j], J["txts"][j]) for j in range(len(pool.M)))], dtype=np.int64)
    for which, bits in (("all", 4), ("acgt", 2)) if (P, g) in ((None, None), (2, 5)) else (("all", 4),):
        i = pool.idx[which]
        sc, sk = amd.batch_banded_alignment_score(31, aligner, pool.batch(amd, which, False, 0, bits))
        got = np.concatenate([sc.cpu().numpy().astype(np.int64)[:, None], amd.u32(sk).astype(np.int64)], axis=1)
        bad = np.nonzero((got != want[i]).any(axis=1))[0]
        assert len(bad) == 0, (sw, which, len(bad), i[bad[:5]], J["kind"][i[bad[:5]]], got[bad[:5]], want[i[bad[:5]]])
        rt = pool.run(amd, sv, which, False, 0, bits) if which == "all" else None
        if rt is not None:
            flag = pool.check_routes(sv, "all", False, 0, rt)
            chances = int(((rt == SETTLED) & (flag >= 2)).sum())
            print("sw", sw, "settled", int((rt == SETTLED).sum()), "of them by a chance", chances, "routes", np.bincount(rt, minlength=12))
            assert int((rt == SETTLED).sum()) >= 100 and chances >= 20


def test_pairs(amd, orc):
    """one indel grid of tests/test_gpu_band31_paired_gap_chance.py -- two windows per read, a pair for the gap chance -- under every corner scheme
    whose rule admits the gap chance: paired, unpaired and the DP alone equal the oracle"""
    from test_gpu_band31_paired_gap_chance import _grid
    d = _grid(orc, 81, 1280)
    schemes = [(c[0], c[1]) for c in E2E31_CORNERS if not c[2] and 4 in e2e31_possible_flags(c[1], False, 150, 150)]
    assert len(schemes) >= 10 and {"edit_distance", "p30_cheap_gaps", "linear_p_above", "linear_p_below", "cheap_txt", "cheap_pat"} <= {s[0] for s in schemes}
    mk = lambda algo: amd.AlignmentBatch(d["reads"], 4, d["roffs"], d["text"], 2, d["wb"], d["we"], read_id=d["rid"], flags=d["fl"], max_read_len=d["max_len"],
                                         algo_flags=algo)
    batches = [(way, mk(algo)) for way, algo in (("paired", 0), ("unpaired", ALN_NO_PAIRED_GAP_CHANCE), ("dp_only", ALN_NO_UNGAPPED_SCORE))]
    for name, sv in schemes:
        want_s, want_k = orc.banded_gotoh_packed_batch(31, oracle.SEMI_GLOBAL, oracle.Scheme(*sv), d["reads"], d["roffs"], d["text"], d["wb"], d["we"],
                                                       read_id=d["rid"], flags=d["fl"])
        settled = {}
        for way, batch in batches:
            sc, sk, rt = amd.banded_gotoh_score_routes(31, amd.make_gotoh_aligner(oracle.SEMI_GLOBAL, amd.GotohScheme(*sv)), batch)
            sc, sk, settled[way] = sc.cpu().numpy(), amd.u32(sk), int((rt.cpu().numpy() == SETTLED).sum())
            bad = np.nonzero((sc != want_s) | (sk != want_k).any(axis=1))[0]
            assert len(bad) == 0, (name, sv, way, len(bad), bad[:5], sc[bad[:5]], want_s[bad[:5]], sk[bad[:5]], want_k[bad[:5]])
        print("%-22s settled of %d: %s" % (name, d["n"], settled))
        assert settled["dp_only"] == 0 and settled["paired"] > 0
