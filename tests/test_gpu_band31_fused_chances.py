"""GPU: the band-31 end-to-end scorer's two chances in ONE launch (chances_e2e31_kernel: second-chance and gap-chance workgroups interleaved)
and the trimmed gap chance (ladder from the host, two-gap tests gated per wave).

Every batch is scored five ways -- the fused launch (default), the two launches apart (ALN_SPLIT_CHANCES), without the gap chance
(ALN_NO_GAP_CHANCE), without the second chance (ALN_NO_SECOND_CHANCE) and by the DP alone (ALN_NO_UNGAPPED_SCORE) -- and every job's score and
sink must equal the oracle's (the reference algorithm) in all five.  Which list a job lands on follows from how its read is made, under the
scheme 0 / -6 / -8 / -3 on a random text: exactly 2 substitutions -> flag 3, list `second`; 3 substitutions (flag 2), one indel or 5 and more
substitutions (flag 4: no diagonal in reach) -> list `third`; 0 or 1 substitution -> settled by the first pass.  The batches: substitutions
only, one indel of 1-7 symbols with 0-3 substitutions, two indels, low-complexity text (tandem repeats of period 1-7), a ragged batch (with and
without the ALN_RAGGED_READS hint), a batch with nothing for list `second`, one with nothing for list `third`, and one with
3 x 256 x 4 + 17 jobs for each list (4 = the largest JOB_LIST_CHUNKS the library can be built with; it is built with 1): several workgroups
per role and a partial last chunk for either."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

SCHEMES = ((0, 6, 6, -8, -3, -8, -3), (0, 3, 3, -4, -2, -4, -2))
PER_LIST = 3 * 256 * 4 + 17


def _subst(rng, r, k):
    if k:
        pos = rng.choice(len(r), k, replace=False); r[pos] = (r[pos] + 1 + rng.integers(0, 3, k)) % 4
    return r


def _indel(rng, src, at, g, ins):
    return np.concatenate([src[:at], rng.integers(0, 4, g, dtype=np.uint8), src[at:]]) if ins else np.concatenate([src[:at], src[at + g:]])


def _read(rng, text, p0, L, kind):
    src = text[p0:p0 + L + 32].copy()
    if kind[0] == "subs":                                           # ("subs", lo, hi): lo..hi substitutions
        return _subst(rng, src[:L].copy(), int(rng.integers(kind[1], kind[2] + 1)))
    if kind[0] == "indel":                                          # one indel of 1-7 symbols, 0-3 substitutions
        r = _indel(rng, src, int(rng.integers(1, L - 8)), int(rng.integers(1, 8)), rng.random() < 0.5)[:L].copy()
        return _subst(rng, r, int(rng.integers(0, 4)))
    if kind[0] == "clean_indel":                                    # one indel of 1-3 symbols, nothing else
        return _indel(rng, src, int(rng.integers(8, L - 16)), int(rng.integers(1, 4)), rng.random() < 0.5)[:L].copy()
    assert kind[0] == "two_indels"
    a1, a2 = sorted(rng.integers(2, L - 6, 2))
    r = _indel(rng, _indel(rng, src, int(a2), int(rng.integers(1, 3)), rng.random() < 0.5), int(a1), int(rng.integers(1, 3)), rng.random() < 0.5)[:L].copy()
    return _subst(rng, r, int(rng.integers(0, 2)))


def _batch(orc, seed, kinds, ragged=False, low_complexity=False):
    """one read per entry of `kinds` over a random text (low_complexity: tandem repeats of period 1-7 with a few mutations, two-letter
    stretches, as tests/test_gpu_gotoh.py builds them, laid under two reads of three)"""
    rng = np.random.default_rng(seed)
    R = len(kinds)
    G = R * 300 + 1000
    text = rng.integers(0, 4, G, dtype=np.uint8)
    lens = rng.integers(40, 162, R) if ragged else np.full(R, 150)
    reads, wbs = [], []
    for j in range(R):
        base = j * 300 + 60
        if low_complexity and j % 3 == 0:
            unit = rng.integers(0, 4, int(rng.integers(1, 8))).astype(np.uint8)
            L = int(rng.integers(60, 230)); a0 = base - 30 + int(rng.integers(0, 60))
            rep = np.resize(unit, L).copy(); mut = rng.random(L) < 0.02; rep[mut] = rng.integers(0, 4, int(mut.sum()))
            text[a0:a0 + L] = rep
        elif low_complexity and j % 3 == 1:
            L = int(rng.integers(40, 200)); a0 = base - 20 + int(rng.integers(0, 60))
            text[a0:a0 + L] = rng.integers(0, 2, L) * int(rng.integers(1, 4))
        reads.append(_read(rng, text, base, int(lens[j]), kinds[j]).astype(np.uint8))
        wbs.append(base - 15 + int(rng.integers(-4, 5)))
    flat = np.concatenate(reads)
    roffs = np.zeros(R + 1, dtype=np.uint32); roffs[1:] = np.cumsum(lens)
    wb = np.array(wbs, dtype=np.uint32); we = (wb + lens + 31).astype(np.uint32)
    return dict(reads=orc.pack4(flat), roffs=roffs, text=orc.pack2(text), wb=wb, we=we, n=R, max_len=int(lens.max()))


def _cycle(R, *kinds):
    return [kinds[j % len(kinds)] for j in range(R)]


def _cases(orc):
    S = lambda lo, hi: ("subs", lo, hi)
    return {
        "substitutions_0_to_5": (_batch(orc, 21, _cycle(4 * 256 + 37, S(0, 5))), False),
        "one_indel": (_batch(orc, 22, _cycle(4 * 256 + 91, ("indel",), S(2, 2), ("indel",), S(0, 0))), False),
        "two_indels": (_batch(orc, 23, _cycle(3 * 256 + 5, ("two_indels",), S(2, 2), ("two_indels",), ("indel",))), False),
        "low_complexity": (_batch(orc, 24, _cycle(5 * 256 + 11, S(0, 5), ("indel",), S(2, 3), ("clean_indel",), ("two_indels",)), low_complexity=True), False),
        "ragged": (_batch(orc, 25, _cycle(4 * 256 + 63, S(0, 5), ("indel",), S(2, 2), ("two_indels",)), ragged=True), True),
        "second_empty": (_batch(orc, 26, _cycle(3 * 256 + 17, ("clean_indel",), S(0, 1), S(3, 3), S(5, 9))), False),
        "third_empty": (_batch(orc, 27, _cycle(3 * 256 + 17, S(2, 2), S(0, 1), S(2, 2))), False),
        "several_workgroups_per_role": (_batch(orc, 28, [("subs", 2, 2)] * PER_LIST + [("clean_indel",)] * PER_LIST + [("subs", 0, 0)] * 300), False),
    }


def _five_ways(amd):
    return (("fused", 0), ("split", amd.ALN_SPLIT_CHANCES), ("no_gap_chance", amd.ALN_NO_GAP_CHANCE),
            ("no_second_chance", amd.ALN_NO_SECOND_CHANCE), ("dp_only", amd.ALN_NO_UNGAPPED_SCORE))


def test_fused_chances_equal_the_oracle_five_ways(amd, orc):
    assert amd.ALN_SPLIT_CHANCES == 131072
    for name, (d, ragged) in _cases(orc).items():
        for sv in SCHEMES:
            want_s, want_k = orc.banded_gotoh_packed_batch(31, oracle.SEMI_GLOBAL, oracle.Scheme(*sv), d["reads"], d["roffs"], d["text"], d["wb"], d["we"])
            for hint in ((0, amd.ALN_RAGGED_READS) if ragged else (0,)):
                for way, algo in _five_ways(amd):
                    batch = amd.AlignmentBatch(d["reads"], 4, d["roffs"], d["text"], 2, d["wb"], d["we"], max_read_len=d["max_len"], algo_flags=algo | hint)
                    sc, sk = amd.batch_banded_alignment_score(31, amd.make_gotoh_aligner(oracle.SEMI_GLOBAL, amd.GotohScheme(*sv)), batch)
                    sc, sk = sc.cpu().numpy(), amd.u32(sk)
                    bad = np.nonzero((sc != want_s) | (sk != want_k).any(axis=1))[0]          # every job of the batch
                    assert len(bad) == 0, (name, sv, way, hint, len(bad), bad[:5], sc[bad[:5]], want_s[bad[:5]], sk[bad[:5]], want_k[bad[:5]])
            if sv == SCHEMES[0]:
                # the batch is what its name says (scores under 0 / -6 / -8 / -3): jobs for list `second` score -12, an indel costs 8 + 3 (g - 1)
                two = int((want_s == -12).sum()); gapped = int(((want_s <= -8) & (want_s % 6 != 0)).sum())
                if name == "second_empty":
                    assert two == 0 and gapped >= d["n"] // 8, (two, gapped)
                if name == "third_empty":
                    assert two >= d["n"] // 2 and (want_s >= -12).all(), (two, want_s.min())
                if name == "several_workgroups_per_role":
                    # (a handful of the 2-substitution jobs END gapped -- both substitutions in the read's last rows, which then match a
                    # neighbouring diagonal -- and count as gapped here; the first pass puts them on list `second` all the same)
                    assert two >= PER_LIST - PER_LIST // 100 and gapped >= PER_LIST * 9 // 10, (two, gapped)
