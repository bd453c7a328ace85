"""GPU: the two windows of an indel read as ONE gap-chance job (gap_chance_e2e31_pair; NVBIO_ALN_NO_PAIRED_GAP_CHANCE switches it off).

A read with an indel of g symbols reaches the band-31 end-to-end scorer as two candidates whose windows are centred on its two diagonals, g
columns apart.  The batches here are built that way directly -- two adjacent jobs per read, sharing a read id -- and every job's score and sink
must equal the oracle's (the reference algorithm, band 31, SEMI_GLOBAL) four ways: default flags, ALN_NO_PAIRED_GAP_CHANCE, ALN_SPLIT_CHANCES
and ALN_NO_UNGAPPED_SCORE (the DP alone).  Which jobs the library may pair is pinned, on every batch, to the numpy restatement of the rule in
tests/test_paired_gap_chance_rule.py through nvbio_banded_gap_pairs.

What an indel batch holds is checked on the CPU, from the oracle's scores under 0 / -6 / -8 / -3, before the GPU is asked.  Under that scheme
the gap chance's class (one gap of g <= 5 symbols and e <= 2 mismatches, below the cheapest class it cannot see, c_unk = 22) is exactly the
costs 8 + 3 (g - 1) + 6 e < 22 = {8, 11, 14, 17, 20}; no other combination of gaps (16, 19, 22, ...) and mismatches (6, 12, 18, ...) gives one
of these, so a job's optimum lies in the class iff its score is the negative of one of them.  Per indel batch at least a third of the pairs
have BOTH jobs' optimum in the class and at least a tenth have AT LEAST ONE job's optimum outside it (`one outside` below counts those), decided
under that one scheme; the other schemes score the same batches.

The pair and the single job share one walk (gap_chance_e2e31_walk), so the pair also runs at the read lengths where the plane words end
differently from M = 150 (PAIR_LENGTHS, one small indel grid each).  A pair takes the paired route only if the first pass flags BOTH jobs 4:
with penalty 6 it keeps counts up to 5 exact, so both need more than 5 mismatches on every one of their 31 diagonals.  Per such batch at least
two fifths of the pairs are of that kind, and at least one eighth of the pairs are of that kind with both optima in the class.

What this test cannot see is whether a pair went through gap_chance_e2e31_pair or through two single jobs: the results are the same by design
and the lists' lengths stay on the device.  It pins which jobs MAY pair (nvbio_banded_gap_pairs) and that every way of scoring agrees with the
oracle; that the paired route runs is seen in the step's time with and without ALN_NO_PAIRED_GAP_CHANCE (profiles/r08_ab_bench.json)."""
import numpy as np
import pytest

import oracle
from test_paired_gap_chance_rule import MAX_SHIFT, NO_PARTNER, gap_pairs

pytestmark = pytest.mark.gpu

SCHEMES = ((0, 6, 6, -8, -3, -8, -3), (0, 2, 2, -5, -1, -5, -1), (0, 4, 4, -6, -6, -6, -6), (0, 3, 3, -4, -2, -4, -2), (0, 6, 6, -5, -3, -5, -3))
IN_CLASS = (-8, -11, -14, -17, -20)                                 # under SCHEMES[0], see above
ROWS = (5, 31, 32, 33, 75, 117, 118, 144)                           # edges of the first / last 32-row words and of the hot halves (M = 150)
SPACING = 400
# read lengths at which the pair's plane words end differently from M = 150: the edges of the 32-row words, of base = M - 32, of the `mid` rule at
# 96 and of the second 64-bit plane
PAIR_LENGTHS = (20, 31, 32, 33, 63, 64, 65, 95, 97, 127, 128, 129)


def _subst(rng, r, k):
    if k:
        pos = rng.choice(len(r), k, replace=False); r[pos] = (r[pos] + 1 + rng.integers(0, 3, k)) % 4
    return r


def _indel_read(rng, text, p0, M, at, g, ins, nsub):
    """the read and its two diagonals (text offsets of row 0 before / after the indel)"""
    src = text[p0:p0 + M + 16]
    r = np.concatenate([src[:at], rng.integers(0, 4, g, dtype=np.uint8), src[at:]]) if ins else np.concatenate([src[:at], src[at + g:]])
    return _subst(rng, r[:M].copy(), nsub).astype(np.uint8), p0, (p0 - g if ins else p0 + g)


class _Jobs:
    """reads (each with any number of jobs) over one random text; a job = (read, win_begin, flags)"""

    def __init__(self, seed, n_reads_hint):
        self.rng = np.random.default_rng(seed)
        self.G = (n_reads_hint + 2) * SPACING
        self.text = self.rng.integers(0, 4, self.G, dtype=np.uint8)
        self.reads, self.jobs = [], []

    def slot(self):
        return len(self.reads) * SPACING + 100                      # where the next read's source starts

    def add(self, read, windows, flags=0):
        self.reads.append(read)
        for w in windows:
            self.jobs.append((len(self.reads) - 1, int(w), flags))

    def finish(self, orc, clip_last=False):
        jobs = self.jobs
        lens = np.array([len(r) for r in self.reads])
        roffs = np.zeros(len(lens) + 1, dtype=np.uint32); roffs[1:] = np.cumsum(lens)
        rid = np.array([j[0] for j in jobs], dtype=np.uint32); wb = np.array([j[1] for j in jobs], dtype=np.uint32)
        fl = np.array([j[2] for j in jobs], dtype=np.uint8)
        we = (wb + lens[rid] + 31).astype(np.uint32)
        text = self.text
        if clip_last:                                               # the text ends one symbol short of the last job's window
            text = text[:int(we[-1]) - 1]; we[-1] = len(text)
        return dict(reads=orc.pack4(np.concatenate(self.reads)), roffs=roffs, text=orc.pack2(text), wb=wb, we=we, rid=rid, fl=fl, n=len(jobs),
                    max_len=int(lens.max()), read_syms=self.reads, text_syms=text)


def _grid(orc, seed, R, M=150, gs=range(1, 8), lead=0, edge=False, repeats=False):
    """R reads with one indel each -- size, kind, row and 0-3 substitutions cycle through every combination -- and the two windows centred on
    their two diagonals (shift = the indel's size), the upper window first for half of the reads.  lead: single jobs of other reads in front (moves the pairs against the waves of 64 jobs).
    edge: the windows are placed so that one of the two diagonals is the first (last) diagonal of one band and outside the other.
    repeats: the indel lies inside a homopolymer or a 2- / 3-periodic repeat (several placements tie)."""
    b = _Jobs(seed, R + lead)
    rng = b.rng
    rows = [min(r, M - 6) for r in ROWS]
    gs = list(gs)                                                   # (5 or 7 sizes: coprime to the 64 combinations of the rest)
    for _ in range(lead):
        p0 = b.slot(); b.add(_subst(rng, b.text[p0:p0 + M].copy(), 7), [p0 - 15])
    for j in range(R):
        g, at, ns, ins = gs[j % len(gs)], rows[j % 8], (j // 8) % 4, bool((j // 32) % 2)
        p0 = b.slot()
        if repeats:
            unit = rng.integers(0, 4, 1 + j % 3).astype(np.uint8); L = int(rng.integers(8, 30))
            a0 = p0 + at - int(rng.integers(0, L)); b.text[max(a0, p0):a0 + L] = np.resize(unit, L)[max(a0, p0) - a0:]
        read, d1, d2 = _indel_read(rng, b.text, p0, M, at, g, ins, ns)
        lo, hi = min(d1, d2), max(d1, d2)
        if not edge:
            w = [lo - 15, hi - 15]
        else:
            s = int(rng.integers(1, min(g, MAX_SHIFT) + 1))
            w = [lo, lo + s] if j % 2 else [hi - 30 - s, hi - 30]
        b.add(read, w if (j // 3) % 2 else w[::-1])                 # (candidates come in seed order: either window may be first)
    return b.finish(orc)


def _geometry(orc, seed):
    """what the pairing rule must tell apart, around reads with an indel of 1-3 symbols: partners of which only one goes to the gap chance,
    opposite strands, a read id that comes back at a non-adjacent index, three candidates in a row, a window clipped at the text's end"""
    M, R = 150, 6 * 120
    b = _Jobs(seed, R)
    rng = b.rng
    for j in range(R):
        p0 = b.slot(); g = 1 + j % 3; kind = j % 6
        read, d1, d2 = _indel_read(rng, b.text, p0, M, int(rng.integers(8, M - 16)), g, bool(rng.integers(0, 2)), int(rng.integers(0, 2)))
        lo, hi = min(d1, d2), max(d1, d2)
        s = 1 + (j // 6) % MAX_SHIFT
        near = _subst(rng, b.text[p0:p0 + M].copy(), (0, 2, 3)[(j // 30) % 3]).astype(np.uint8)      # lies on the diagonal p0
        if kind == 0:        # a diagonal that only the LOWER window holds (its diagonal 0 .. s - 1): the upper job has none in reach, the lower is
            w = p0 - int(rng.integers(0, s))       # settled by the first pass (0 substitutions) or goes to the second (2) or third (3) chance
            b.add(near, [w, w + s])
        elif kind == 1:      # ... that only the UPPER window holds (its diagonal 30 - s + 1 .. 30)
            w = p0 - 30 + int(rng.integers(0, s))
            b.add(near, [w - s, w])
        elif kind == 2:      # the two windows on opposite strands
            b.add(read, [lo - 15, hi - 15]); b.jobs[-1] = (b.jobs[-1][0], b.jobs[-1][1], 3)
        elif kind == 3:      # both on the reverse strand (the read is stored reverse-complemented)
            b.add((3 - read[::-1]).astype(np.uint8), [lo - 15, hi - 15], flags=3)
        elif kind == 4:      # three candidates in a row
            b.add(read, [lo - 15 - 2, lo - 15, hi - 15])
        else:                # (its two jobs are moved apart below)
            b.add(read, [lo - 15, hi - 15])
    # kind 5: swap the upper job with the job that follows it (another read's), so that the read's two jobs are not adjacent
    jobs, i = b.jobs, 0
    while i + 2 < len(jobs):
        if jobs[i][0] % 6 == 5 and jobs[i + 1][0] == jobs[i][0] and jobs[i + 2][0] != jobs[i][0]:
            jobs[i + 1], jobs[i + 2] = jobs[i + 2], jobs[i + 1]; i += 3
        else:
            i += 1
    # the last read: a pair whose upper window the text's end clips
    p0 = b.slot()
    read, d1, d2 = _indel_read(rng, b.text, p0, M, 60, 2, False, 0)
    b.add(read, [d1 - 15, d2 - 15])
    return b.finish(orc, clip_last=True)


def _singles(orc, seed, R, M=150):
    b = _Jobs(seed, R)
    for j in range(R):
        p0 = b.slot()
        read, d1, d2 = _indel_read(b.rng, b.text, p0, M, int(b.rng.integers(8, M - 16)), 1 + j % 5, bool(j & 1), j % 3)
        b.add(read, [(d1 if j % 4 < 2 else d2) - 15])
    return b.finish(orc)


def _every_diagonal_above(d, M, cnt):
    """per job of a _grid batch (forward reads of one length M): all 31 diagonals of its window hold more than cnt mismatches"""
    win = d["text_syms"][d["wb"][:, None].astype(np.int64) + np.arange(M + 30)]
    reads = np.stack(d["read_syms"])[d["rid"]]
    return np.all([(win[:, k:k + M] != reads).sum(axis=1) > cnt for k in range(31)], axis=0)


def _cases(orc):
    # (batch, schemes, an indel batch whose mix is checked)
    edges = {"pair_length_%d" % M: (_grid(orc, 900 + M, 640, M=M), SCHEMES[:1], False) for M in PAIR_LENGTHS}
    return {
        **edges,
        "indel_grid": (_grid(orc, 81, 3000), SCHEMES, True),
        "every_job_a_pair_member": (_grid(orc, 82, 3008, gs=range(1, 6)), SCHEMES[:1], True),
        "wave_boundary_inside_a_pair": (_grid(orc, 83, 130, lead=1), SCHEMES[:2], True),
        "transition_in_one_band_only": (_grid(orc, 84, 3000, edge=True), SCHEMES[:2], False),
        "indels_inside_repeats": (_grid(orc, 85, 3000, repeats=True), SCHEMES[:2], False),
        "geometry": (_geometry(orc, 86), SCHEMES[:2], False),
        "no_pairs": (_singles(orc, 87, 1500), SCHEMES[:1], False),
        "length_96": (_grid(orc, 88, 700, M=96), SCHEMES[:2], False),
        "length_100": (_grid(orc, 89, 700, M=100), SCHEMES[:1], False),
        "length_161": (_grid(orc, 90, 700, M=161), SCHEMES[:2], False),
    }


def _ways(amd):
    return (("paired", 0), ("unpaired", amd.ALN_NO_PAIRED_GAP_CHANCE), ("split", amd.ALN_SPLIT_CHANCES), ("dp_only", amd.ALN_NO_UNGAPPED_SCORE))


def test_paired_gap_chance_equals_the_oracle_four_ways(amd, orc):
    assert amd.ALN_NO_PAIRED_GAP_CHANCE == 2 * amd.ALN_SPLIT_CHANCES and amd.GAP_PAIR_MAX_SHIFT == MAX_SHIFT
    for name, (d, schemes, indel_batch) in _cases(orc).items():
        want_p = gap_pairs(d["roffs"], d["wb"], d["we"], d["rid"], d["fl"])
        lower = np.nonzero((want_p != NO_PARTNER) & (want_p > np.arange(d["n"])))[0]
        wants = [orc.banded_gotoh_packed_batch(31, oracle.SEMI_GLOBAL, oracle.Scheme(*sv), d["reads"], d["roffs"], d["text"], d["wb"], d["we"],
                                               read_id=d["rid"], flags=d["fl"]) for sv in schemes]
        # what the batch holds, before the GPU is asked
        s0 = wants[0][0]
        both_in = int((np.isin(s0[lower], IN_CLASS) & np.isin(s0[lower + 1], IN_CLASS)).sum())
        one_out = int((~np.isin(s0[lower], IN_CLASS) | ~np.isin(s0[lower + 1], IN_CLASS)).sum())
        print(name, "jobs", d["n"], "pairs", len(lower), "both in the class", both_in, "one outside", one_out)
        if indel_batch:
            assert 3 * both_in >= len(lower) and 10 * one_out >= len(lower), (name, len(lower), both_in, one_out)
        if name.startswith("pair_length_"):
            # the pairs that take the paired route: under SCHEMES[0] (penalty 6) the first pass keeps counts up to 5 exact and flags 4 only above
            # that, so BOTH jobs need more than 5 mismatches on every one of their 31 diagonals
            far = _every_diagonal_above(d, int(name[len("pair_length_"):]), 5)
            routed = far[lower] & far[lower + 1]
            routed_in = int((routed & np.isin(s0[lower], IN_CLASS) & np.isin(s0[lower + 1], IN_CLASS)).sum())
            print(name, "pairs with both jobs flagged 4", int(routed.sum()), "of them both optima in the class", routed_in)
            assert 5 * int(routed.sum()) >= 2 * len(lower) and 8 * routed_in >= len(lower), (name, len(lower), int(routed.sum()), routed_in)
        if name == "every_job_a_pair_member":
            assert 2 * len(lower) == d["n"]
        if name == "no_pairs":
            assert len(lower) == 0
        if name == "wave_boundary_inside_a_pair":
            assert want_p[63] == NO_PARTNER and want_p[64] == NO_PARTNER and d["rid"][63] == d["rid"][64] and want_p[65] == 66
        if indel_batch:
            down = int((d["wb"][lower + 1] < d["wb"][lower]).sum())
            assert 3 * down >= len(lower) and 3 * (len(lower) - down) >= len(lower), (name, down)      # both orders of the two windows
        if name == "transition_in_one_band_only":
            assert int((s0[lower] != s0[lower + 1]).sum()) >= len(lower) // 2            # the two jobs of a pair do NOT see the same alignments
        if name == "geometry":
            assert d["we"][-1] - d["wb"][-1] < 150 + 31 and want_p[-1] == NO_PARTNER and len(lower) >= d["n"] // 8
        mk = lambda algo: amd.AlignmentBatch(d["reads"], 4, d["roffs"], d["text"], 2, d["wb"], d["we"], read_id=d["rid"], flags=d["fl"],
                                             max_read_len=d["max_len"], algo_flags=algo)
        got_p = amd.u32(amd.banded_gap_pairs(mk(0)))
        assert np.array_equal(got_p, want_p), (name, np.nonzero(got_p != want_p)[0][:8])
        for sv, (want_s, want_k) in zip(schemes, wants):
            for way, algo in _ways(amd):
                sc, sk = amd.batch_banded_alignment_score(31, amd.make_gotoh_aligner(oracle.SEMI_GLOBAL, amd.GotohScheme(*sv)), mk(algo))
                sc, sk = sc.cpu().numpy(), amd.u32(sk)
                bad = np.nonzero((sc != want_s) | (sk != want_k).any(axis=1))[0]
                assert len(bad) == 0, (name, sv, way, len(bad), bad[:5], d["wb"][bad[:5]], sc[bad[:5]], want_s[bad[:5]], sk[bad[:5]], want_k[bad[:5]])
