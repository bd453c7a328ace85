"""GPU: the band-31 DP's narrow classes (banded_gotoh_band31_pk_kernel with NARROW; NVBIO_ALN_NO_NARROW_DP switches them off).

Every job's (score, sink) must equal the oracle's band-31 SEMI_GLOBAL scoring and the same call with ALN_NO_NARROW_DP set; which body a job
went through is read from nvbio_banded_gotoh_score_routes (0 settled before the DP, 1 full band, 2 class A, 3 class B, +8 redone), without
which none of this could tell whether a narrow row ever ran.  The rule itself is pinned in numpy by tests/test_narrow_dp_rule.py, whose job
builders (random substitutions, the two decoys) are used here.

Batches (reads of 96, 100, 150 and 161 symbols, 4-bit and 2-bit, forward and reverse-complemented):
  a  exactly 4, exactly 5 and 6-8 substitutions at random rows: >= 95 % of the 4s take class A, >= 95 % of the 5s class B, none of either redone
  b  substitutions only in rows 0..23, only in the last 8 rows, and at rows 23 / 24 / 25 (the switch from the full to the narrow body)
  c  decoy 1: diagonal 27 matches the read's first 40 rows exactly -- every job carries the redo bit
  d  decoy 2: the boundary diagonal 21 matches rows 0..59 but for two substitutions -- every job carries the redo bit, results equal
  e  optima that are gapped and above U*: four substitutions clustered beside a one-symbol indel-like repeat, and tandem repeats of period 1-7
  f  windows off centre by 1, 2 and 3 columns (class B, class B, full band at 0 / -6 / -8 / -3: w = 6 + offset), and clipped windows (full band)
  g  class lists of 0, 1, 127, 128, 129 and 257 jobs, each class empty in turn
  h  five schemes, among them one with gaps so cheap that class A comes out empty"""
import numpy as np
import pytest

import oracle
from test_narrow_dp_rule import decoy_boundary, decoy_outer

pytestmark = pytest.mark.gpu

SCHEMES = ((0, 6, 6, -8, -3, -8, -3), (0, 6, 6, -5, -1, -5, -1), (0, 4, 4, -6, -6, -6, -6), (0, 3, 3, -4, -2, -4, -2), (0, 6, 6, -5, -3, -5, -3))
SETTLED, FULL, CLASS_A, CLASS_B, REDONE = 0, 1, 2, 3, 8
SPACING = 256


class _Jobs:
    """one job per read over one random text; read q's source starts at text symbol 100 + q * SPACING"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.reads, self.wins, self.offs, self.flags, self.kind = [], [], [], [], []

    def add(self, read, win, off=0, flags=0, kind=0):
        """read against the window's symbols `win` (len(read) + 31 + slack of them, the band's column 15 + off on the read's own diagonal)"""
        self.reads.append(np.asarray(read, dtype=np.uint8)); self.wins.append(np.asarray(win, dtype=np.uint8))
        self.offs.append(off); self.flags.append(flags); self.kind.append(kind)

    def add_subs(self, M, rows, off=0, flags=0, kind=0, win=None):
        """a read with substitutions at `rows` (win: the window's symbols, random if not given)"""
        if win is None:
            win = self.rng.integers(0, 4, M + 40, dtype=np.uint8)
        read = win[15:15 + M].copy()
        rows = np.asarray(rows, dtype=np.int64)
        read[rows] = (read[rows] + 1 + self.rng.integers(0, 3, len(rows))) % 4
        self.add(read, win, off, flags, kind)

    def finish(self, orc, read_bits=4, clip=None):
        n = len(self.reads)
        text = self.rng.integers(0, 4, 100 + n * SPACING + 64, dtype=np.uint8)
        lens = np.array([len(r) for r in self.reads])
        wb = np.zeros(n, dtype=np.uint32)
        stored = []
        for q in range(n):
            p0 = 100 + q * SPACING
            text[p0 - 15:p0 - 15 + len(self.wins[q])] = self.wins[q]
            wb[q] = p0 - 15 - self.offs[q]
            r = self.reads[q]
            if self.flags[q] & 1: r = r[::-1]
            if self.flags[q] & 2: r = 3 - r
            stored.append(r.astype(np.uint8))
        we = (wb + lens + 31).astype(np.uint32)
        if clip is not None:                                                   # those windows end `clip` symbols early
            we[-clip[0]:] -= clip[1]
        flat = np.concatenate(stored)
        roffs = np.zeros(n + 1, dtype=np.uint32); roffs[1:] = np.cumsum(lens)
        return dict(reads4=orc.pack4(flat), reads=orc.pack4(flat) if read_bits == 4 else orc.pack2(flat), bits=read_bits, roffs=roffs,
                    text=orc.pack2(text), wb=wb, we=we, fl=np.array(self.flags, dtype=np.uint8), n=n, max_len=int(lens.max()),
                    kind=np.array(self.kind))


def _run(amd, orc, d, scheme=SCHEMES[0]):
    """oracle == default == ALN_NO_NARROW_DP for every job; -> the default call's routes"""
    want_s, want_k = orc.banded_gotoh_packed_batch(31, oracle.SEMI_GLOBAL, oracle.Scheme(*scheme), d["reads4"], d["roffs"], d["text"], d["wb"], d["we"],
                                                   flags=d["fl"])
    aligner = amd.make_gotoh_aligner(2, amd.GotohScheme(*scheme))
    routes = {}
    for algo in (0, amd.ALN_NO_NARROW_DP):
        batch = amd.AlignmentBatch(d["reads"], d["bits"], d["roffs"], d["text"], 2, d["wb"], d["we"], flags=d["fl"], max_read_len=d["max_len"], algo_flags=algo)
        sc, sk, rt = amd.banded_gotoh_score_routes(31, aligner, batch)
        sc, sk, routes[algo] = sc.cpu().numpy(), amd.u32(sk), rt.cpu().numpy()
        bad = np.nonzero((sc != want_s) | (sk != want_k).any(axis=1))[0]
        assert len(bad) == 0, (scheme, algo, d["n"], bad[:5], routes[algo][bad[:5]], sc[bad[:5]], want_s[bad[:5]], sk[bad[:5]], want_k[bad[:5]])
        sc2, sk2 = amd.batch_banded_alignment_score(31, aligner, batch)                     # the plain call: the same results
        assert (sc2.cpu().numpy() == sc).all() and (amd.u32(sk2) == sk).all()
    off = routes[amd.ALN_NO_NARROW_DP]
    assert np.isin(off, (SETTLED, FULL)).all()                                           # with the flag set no class is formed
    return routes[0]


def _share(routes, sel, value):
    return float((routes[sel] == value).mean())


def test_substitution_reads_take_their_classes(amd, orc):
    """a: by length, read width and strand"""
    assert amd.ALN_NO_NARROW_DP == 524288
    for M, bits, seed in ((150, 4, 1), (150, 2, 2), (96, 4, 3), (100, 2, 4), (161, 4, 5)):
        b = _Jobs(seed)
        for q in range(1536):
            k = (4, 5, int(b.rng.integers(6, 9)))[q % 3]
            b.add_subs(M, b.rng.choice(M, k, replace=False), flags=(0, 3)[(q // 3) % 2], kind=q % 3)
        d = b.finish(orc, bits)
        rt = _run(amd, orc, d)
        a, bb = _share(rt, d["kind"] == 0, CLASS_A), _share(rt, d["kind"] == 1, CLASS_B)
        print("length", M, "bits", bits, "class A of the 4s", a, "class B of the 5s", bb, "routes", np.bincount(rt, minlength=12))
        assert a >= 0.95 and bb >= 0.95, (M, bits, a, bb)
        assert not (rt[d["kind"] < 2] & REDONE).any()


def test_substitutions_around_the_switch_rows(amd, orc):
    """b"""
    b = _Jobs(6)
    for q in range(768):
        k, where = 4 + q % 2, q % 3
        if where == 0:   rows = b.rng.choice(24, k, replace=False)
        elif where == 1: rows = 150 - 8 + b.rng.choice(8, k, replace=False)
        else:            rows = np.concatenate([[23, 24, 25], 26 + b.rng.choice(120, k - 3, replace=False)])
        b.add_subs(150, rows, flags=(0, 3)[(q // 6) % 2], kind=k)
    d = b.finish(orc)
    rt = _run(amd, orc, d)
    assert _share(rt, d["kind"] == 4, CLASS_A) >= 0.95 and _share(rt, d["kind"] == 5, CLASS_B) >= 0.95 and not (rt & REDONE).any()


def test_decoys_are_redone(amd, orc):
    """c, d"""
    for builder, seed in ((decoy_outer, 7), (decoy_boundary, 8)):
        b = _Jobs(seed)
        reads, wins = builder(b.rng, 300)
        for q in range(300):
            b.add(reads[q], wins[q])
        rt = _run(amd, orc, b.finish(orc))
        assert (rt == (CLASS_A | REDONE)).all(), np.bincount(rt, minlength=12)


def test_gapped_optima_above_the_bound(amd, orc):
    """e: class jobs whose optimum is a gapped alignment ABOVE the bound L = U* (L is only a lower bound), and tandem repeats, where many
    placements tie.  Odd jobs: the read's last (first) four rows lie on the next (previous) diagonal and all four differ on the centre one --
    an indel-like shift of one symbol that the best diagonal pays with four mismatches, U* = -24, and the DP with one gap, -8"""
    b = _Jobs(9)
    M = 150
    for q in range(800):
        win = b.rng.integers(0, 4, M + 40, dtype=np.uint8)
        at = int(b.rng.integers(30, 110))
        run = int(b.rng.integers(8, 24))
        win[15 + at:15 + at + run] = np.resize(b.rng.integers(0, 4, 1 + q % 7, dtype=np.uint8), run)      # a tandem repeat of period 1-7
        if q % 2 == 0:
            b.add_subs(M, b.rng.choice(M, 4 + (q // 2) % 2, replace=False), kind=0, win=win)
            continue
        ramp = (np.arange(8) + int(b.rng.integers(0, 4))) % 4                        # neighbours differ
        if q % 4 == 1:
            win[15 + M - 6:15 + M + 2] = ramp
            read = win[15:15 + M].copy(); read[M - 4:] = win[15 + M - 3:15 + M + 1]
        else:
            win[15 - 2:15 + 6] = ramp
            read = win[15:15 + M].copy(); read[:4] = win[14:18]
        b.add(read, win, flags=(0, 3)[(q // 4) % 2], kind=1)
    d = b.finish(orc)
    rt = _run(amd, orc, d)
    want_s, _ = orc.banded_gotoh_packed_batch(31, oracle.SEMI_GLOBAL, oracle.Scheme(*SCHEMES[0]), d["reads4"], d["roffs"], d["text"], d["wb"], d["we"], flags=d["fl"])
    print("gapped optima: routes", np.bincount(rt, minlength=12), "scores of the shifted reads", np.unique(want_s[d["kind"] == 1]))
    shifted = d["kind"] == 1
    assert (want_s[shifted] > -24).mean() >= 0.9 and _share(rt, shifted, CLASS_A) >= 0.9 and not (rt[shifted] & REDONE).any()


def test_off_centre_and_clipped_windows(amd, orc):
    """f"""
    b = _Jobs(10)
    for q in range(512):
        b.add_subs(150, b.rng.choice(150, 4, replace=False), off=(1, -1, 2, -2, 3, -3, 0, 0)[q % 8], kind=q % 8)
    d = b.finish(orc)
    rt = _run(amd, orc, d)
    assert _share(rt, d["kind"] < 4, CLASS_B) >= 0.95                               # w = 7, 8
    assert (rt[(d["kind"] == 4) | (d["kind"] == 5)] == FULL).all()                  # w = 9
    assert _share(rt, d["kind"] >= 6, CLASS_A) >= 0.95
    b = _Jobs(11)
    for q in range(256):
        b.add_subs(150, b.rng.choice(150, 4 + q % 2, replace=False))
    d = b.finish(orc, clip=(128, 3))
    rt = _run(amd, orc, d)
    assert (rt[-128:] == FULL).all() and np.isin(rt[:128], (CLASS_A, CLASS_B)).mean() >= 0.95


@pytest.mark.parametrize("n_a,n_b", [(0, 0), (1, 0), (0, 1), (127, 129), (128, 128), (129, 127), (257, 0), (0, 257), (257, 1)])
def test_class_list_lengths(amd, orc, n_a, n_b):
    """g: the lists' ends inside, at and behind a workgroup's 256 jobs (two per lane); 40 other jobs around them"""
    b = _Jobs(100 + 3 * n_a + n_b)
    ks = [4] * n_a + [5] * n_b + [0, 2, 9, 12] * 10
    for k in b.rng.permutation(ks):
        b.add_subs(150, b.rng.choice(150, int(k), replace=False), kind=int(k))
    d = b.finish(orc)
    rt = _run(amd, orc, d)
    assert int((rt == CLASS_A).sum()) == n_a and int((rt == CLASS_B).sum()) == n_b, np.bincount(rt, minlength=12)


def test_five_schemes(amd, orc):
    """h"""
    b = _Jobs(12)
    for q in range(1024):
        b.add_subs(150, b.rng.choice(150, 1 + q % 8, replace=False), flags=(0, 3)[(q // 8) % 2])
    d = b.finish(orc)
    for scheme in SCHEMES:
        rt = _run(amd, orc, d, scheme)
        print("scheme", scheme, "routes", np.bincount(rt, minlength=12))
        if scheme == SCHEMES[1]:
            assert not ((rt & 7) == CLASS_A).any() and (rt == CLASS_B).sum() >= 100     # thresholds -10 / -12: one mismatch goes to the second chance, two reach class B
        if scheme == SCHEMES[0]:
            assert (rt == CLASS_A).sum() >= 100 and (rt == CLASS_B).sum() >= 100
