"""GPU: the band-31 end-to-end scorer's job lists, which the first pass and the chances build themselves (no partition / select pass).

The lists are unordered and their counters are reserved with atomics, so what is pinned here is what must not depend on that: for a batch
with jobs on every route (exact reads -> settled by the first pass; 2-4 substitutions -> second / third chance; one indel -> gap chance;
5 or more substitutions -> straight to the DP), `batch_banded_alignment_score(31, ...)` gives bit-equal scores and sinks to the plain DP of
every job (ALN_NO_UNGAPPED_SCORE) under every combination of the flags that decide which launch follows the first pass -- a job parked on a
list that no launch walks would never reach the DP --, under a quality ramp (the QUAL first pass, no gap chance), for ragged batches with
and without the length sort of the DP's list, for a job count that is not a multiple of the workgroup's 256, for n = 1, and for a batch
where no job needs the DP; twice in a row (the counters are zeroed by every call), and once more under the scratch check mode, whose fills
poison the counters and whose report must show no damaged block."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEMI_GLOBAL = 2
SCHEME = (0, 6, 6, -8, -3, -8, -3)              # one mismatch penalty: first pass, three chances and the gap chance
RAMP = (0, 2, 6, -8, -3, -8, -3)                # penalties 2..6 by base quality: the QUAL first pass


def _make_batch(orc, seed, R, kinds, ragged=False):
    """R reads over a random text; read k is of kind kinds[k % len(kinds)]: 'exact', 'subs' (2-4 substitutions), 'indel' (one indel of
    1-4 symbols and 0-1 substitutions), 'many' (5-11 substitutions)"""
    rng = np.random.default_rng(seed)
    G = 300000
    text = rng.integers(0, 4, G, dtype=np.uint8)
    lens = rng.integers(40, 162, R) if ragged else np.full(R, 150)
    starts = rng.integers(60, G - 400, R)
    reads = []
    for k in range(R):
        L = int(lens[k]); src = text[starts[k]:starts[k] + L + 8].copy()
        kind = kinds[k % len(kinds)]
        nm = 0
        if kind == "indel":
            g = int(rng.integers(1, 5)); at = int(rng.integers(4, L - 8))
            r = (np.concatenate([src[:at], rng.integers(0, 4, g, dtype=np.uint8), src[at:]]) if rng.random() < 0.5
                 else np.concatenate([src[:at], src[at + g:]]))[:L].copy()
            nm = int(rng.integers(0, 2))
        else:
            r = src[:L].copy()
            nm = {"exact": 0, "subs": int(rng.integers(2, 5)), "many": int(rng.integers(5, 12))}[kind]
        if nm:
            pos = rng.choice(L, nm, replace=False); r[pos] = (r[pos] + 1 + rng.integers(0, 3, nm)) % 4
        reads.append(r.astype(np.uint8))
    flat = np.concatenate(reads)
    roffs = np.zeros(R + 1, dtype=np.uint32); roffs[1:] = np.cumsum(lens)
    wb = (starts - 15 + rng.integers(-3, 4, R)).astype(np.uint32)
    we = (wb + lens + 31).astype(np.uint32)
    quals = rng.integers(0, 64, len(flat), dtype=np.uint8)
    return dict(reads=orc.pack4(flat), roffs=roffs, text=orc.pack2(text), wb=wb, we=we, quals=quals, n=R, max_len=int(lens.max()))


def _score(amd, d, scheme, algo, quals=False):
    batch = amd.AlignmentBatch(d["reads"], 4, d["roffs"], d["text"], 2, d["wb"], d["we"], quals=d["quals"] if quals else None,
                               max_read_len=d["max_len"], algo_flags=algo)
    sc, sk = amd.batch_banded_alignment_score(31, amd.make_gotoh_aligner(SEMI_GLOBAL, amd.GotohScheme(*scheme)), batch)
    return sc.cpu().numpy(), amd.u32(sk)


def _flag_sets(amd):
    s, t, g = amd.ALN_NO_SECOND_CHANCE, amd.ALN_NO_THIRD_CHANCE, amd.ALN_NO_GAP_CHANCE
    return (0, s, t, g, s | t, s | t | g)


def _check_batch(amd, d, ragged=False):
    for scheme, quals in ((SCHEME, False), (RAMP, True)):
        want_s, want_k = _score(amd, d, scheme, amd.ALN_NO_UNGAPPED_SCORE, quals)          # the plain DP of every job
        algos = list(_flag_sets(amd))
        if ragged:
            algos += [a | amd.ALN_RAGGED_READS for a in _flag_sets(amd)] + [a | amd.ALN_RAGGED_READS | amd.ALN_NO_LENGTH_SORT for a in _flag_sets(amd)]
        else:
            algos += [amd.ALN_RAGGED_READS, amd.ALN_RAGGED_READS | amd.ALN_NO_LENGTH_SORT]
        for algo in algos:
            for call in range(2):                                                          # the second call: counters zeroed again
                sc, sk = _score(amd, d, scheme, algo, quals)
                bad = np.nonzero((sc != want_s) | (sk != want_k).any(axis=1))[0]
                assert len(bad) == 0, (scheme, quals, algo, call, d["n"], bad[:5], sc[bad[:5]], want_s[bad[:5]], sk[bad[:5]], want_k[bad[:5]])
    return want_s


def _cases(orc):
    every = ("exact", "subs", "indel", "many", "subs", "exact", "indel")
    return {
        "every_route": (_make_batch(orc, 11, 5 * 256 + 37, every), False),
        "every_route_ragged": (_make_batch(orc, 12, 3 * 256 + 101, every, ragged=True), True),
        "one_job_exact": (_make_batch(orc, 13, 1, ("exact",)), False),
        "one_job_dp": (_make_batch(orc, 14, 1, ("many",)), False),
        "no_job_needs_dp": (_make_batch(orc, 15, 2 * 256 + 5, ("exact",)), False),
    }


def test_job_lists_give_the_plain_dp_results(amd, orc):
    cases = _cases(orc)
    for name, (d, ragged) in cases.items():
        want = _check_batch(amd, d, ragged)
        if name == "every_route":
            # the batch really has jobs for every route: exact reads, few mismatches, gapped optima, poor ones
            assert (want == 0).sum() >= d["n"] // 8 and ((want <= -12) & (want >= -24)).sum() >= d["n"] // 8 and (want < -30).sum() >= d["n"] // 16
        if name == "no_job_needs_dp":
            assert (want == 0).all()


@pytest.mark.parametrize("fill", [0x00, 0xFF, 0x02], ids=["fill00", "fillFF", "fill02"])
def test_job_lists_under_scratch_check(amd, orc, fill):
    cases = _cases(orc)
    amd.set_scratch_check(True, fill)
    try:
        for name, (d, ragged) in cases.items():
            _check_batch(amd, d, ragged)
    finally:
        report = amd.scratch_check_report()
        amd.set_scratch_check(False)
    assert report.get("banded_job_list", (0,))[0] > 0, report
    damaged = {t: r for t, r in report.items() if r[1]}
    assert not damaged, damaged
