"""nvBowtie's all-mapping mode (Aligner::all + score_all, nvBowtie/bowtie2/cuda/aligner_all.h:29-485) restated on the oracle, one read and
one seed pass at a time, and the shared input of its tests.  A helper, not a test; test infrastructure, parity unpinned beyond the pieces
that are pinned on their own (match / locate / the deque container / the banded DP and its traceback / finish_alignment)."""
import functools
import math

import numpy as np

import oracle
from util import mutate_reads

READ_LEN, N_TEXT = 100, 30000
UNIT, COPIES, DIVERGENCE = 300, 40, 0.02


def band_length(max_dist):
    """Aligner::band_length (aligner.h:149-158)"""
    band_len = 4
    while band_len - 1 < max_dist * 2 + 1:
        band_len *= 2
    return band_len - 1


def revcomp(a):
    a = a[::-1]
    return np.where(a < 4, 3 - a, a).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def shared_input():
    """-> (text uint8 [N_TEXT], reads uint8 [R, 100] in their original orientation, planted: list of (read, rc, loc) exact copies)"""
    rng = np.random.default_rng(20240611)
    M = READ_LEN
    text = rng.integers(0, 4, N_TEXT, dtype=np.uint8)
    unit = rng.integers(0, 4, UNIT, dtype=np.uint8)
    fam = [600 + 700 * k for k in range(COPIES)]                     # the family: 40 copies of a 300 bp unit, 2 % apart
    for p in fam:
        c = unit.copy()
        m = rng.random(UNIT) < DIVERGENCE
        c[m] = (c[m] + 1 + rng.integers(0, 3, int(m.sum()))) % 4
        text[p:p + UNIT] = c
    reads, planted = [], []
    fam_starts = np.array([fam[int(rng.integers(0, COPIES))] + int(rng.integers(0, UNIT - M - 8)) for _ in range(80)])
    reads.append(mutate_reads(rng, text, fam_starts, M, sub=0.01, indel=0.25))
    uniq_starts = np.array([fam[k] + UNIT + 40 + int(rng.integers(0, 200)) for k in rng.integers(0, COPIES - 1, 60)])
    reads.append(mutate_reads(rng, text, uniq_starts, M, sub=0.02, indel=0.25))
    reads = np.concatenate(reads)
    reads[1::2] = np.stack([revcomp(r) for r in reads[1::2]])       # both strands
    extra = []
    for s, rc in ((fam[3] + 17, 0), (fam[20] + 150, 1), (5000 - 250, 0), (12345 - 45, 1), (fam[7] + UNIT + 100, 0), (fam[30] + 60, 1)):
        r = text[s:s + M].copy()                                     # exact copies
        planted.append((len(reads) + len(extra), rc, s))
        extra.append(revcomp(r) if rc else r)
    S = int(1 + 1.15 * math.sqrt(M)); first = 2 * (S // 3)
    for k, s in enumerate((fam[5] + 30, fam[9] + UNIT + 70, fam[12] + 100)):
        r = text[s:s + M].copy(); r[M - 1 - (first + k * S + 5)] = 4   # an N inside seed k (seeds lie on the stored = reversed read)
        extra.append(r)
    for s in (fam[15] + 50, fam[16] + UNIT + 90):
        r = text[s:s + M].copy(); r[M - 1 - 3] = 4                   # an N before the first seed: outside every seed
        extra.append(r)
    planted.append((len(reads) + len(extra), 0, 0)); extra.append(text[:M].copy())                       # window clamps at both ends
    planted.append((len(reads) + len(extra), 0, N_TEXT - M)); extra.append(text[N_TEXT - M:].copy())
    over = np.concatenate([rng.integers(0, 4, 30, dtype=np.uint8), text[:M - 30]])                        # overhangs the start: loc wraps
    extra.append(over)
    for _ in range(45):
        extra.append(rng.integers(0, 4, M, dtype=np.uint8))          # map nowhere
    reads = np.concatenate([reads, np.stack(extra)])
    return text, reads, planted


def all_mapping_cpu(O, hidx, text, genome_len, reads, aln_type, max_dist, seed_len=22, seed_freq=None, max_reseed=2, band=None,
                    rep_seeds=1000, want_cigars=False):
    """reads: uint8 [R, M] in their ORIGINAL orientation (nvBowtie stores them reversed and seeds the stored stream).
    -> list of (read_id, rc, loc, score) in the order seed pass, read, deque entry, SA row; with want_cigars a second list of
    (source, sink, ed, cigar uint16[]) per record"""
    R, M = reads.shape
    L = min(seed_len, M)
    S = seed_freq or int(1 + 1.15 * math.sqrt(M))
    retry_stride = S // (max_reseed + 1)
    band = band or band_length(max_dist)
    min_score = -max_dist                                                                # scoring.h:165,181
    max_seeds = M // S                                                                   # aligner_all.h:72-74
    stored = reads[:, ::-1]
    records, details = [], []
    for seed in range(max_seeds):                                                        # aligner_all.h:76
        for r in range(R):
            deque = np.zeros((0, 2), dtype=np.uint32)                                    # hit_deques.clear_deques()
            for retry in range(max_reseed + 1):                                          # map_kernel, mapping_inl.h:600-633
                offs = []
                for i in range(seed, seed + 1):
                    pos = retry * retry_stride + i * S
                    if pos + L > M:
                        break
                    offs.append(pos)
                seeds = np.concatenate([stored[r, o:o + L] for o in offs]).astype(np.uint8) if offs else np.zeros(0, np.uint8)
                so = (np.arange(len(offs) + 1) * L).astype(np.uint32)
                fw = O.match_batch(hidx, seeds, so, reverse=True) if offs else np.zeros((0, 2), np.uint32)
                comp = np.where(seeds < 4, 3 - seeds, seeds).astype(np.uint8)
                rc = O.match_batch(hidx, comp, so) if offs else np.zeros((0, 2), np.uint32)
                heap, _ = O.map_exact_read(fw, rc, np.array(offs, dtype=np.uint32), M, L, 100, rep_seeds)
                range_count = len(heap)
                range_sum = int((heap[:, 1] & 0xFFFFF).sum()) & 0xFFFFFFFF
                if retry == max_reseed or range_count == 0 and range_sum < ((rep_seeds * range_count) & 0xFFFFFFFF):      # :627
                    deque = heap
                    break
            for begin_row, bits in deque:                                                # select_all: every row of every range
                size = int(bits) & 0xFFFFF; pos_in_read = (int(bits) >> 20) & 0x3FF; read_rc = (int(bits) >> 30) & 1
                if size == 0:
                    continue
                rows = (int(begin_row) + np.arange(size)).astype(np.uint32)
                pat = revcomp(reads[r]) if read_rc else reads[r]
                for p in O.locate_batch(hidx, rows):
                    loc = (int(p) - pos_in_read) & 0xFFFFFFFF                            # locate_inl.h:133
                    begin = loc - band // 2 if loc > band // 2 else 0                    # AllScoreStream::init_context
                    end = min((begin + band + M) & 0xFFFFFFFF, genome_len)
                    if begin >= genome_len or end < begin:
                        continue                                                         # the empty window of a wrapped locus: nothing reported
                    txt = text[begin:end]
                    _, score, _ = O.banded_sw(band, aln_type, oracle.ED_SW, pat, txt)
                    if score < min_score:                                                # AllScoreStream::output
                        continue
                    records.append((r, read_rc, loc, score))
                    if want_cigars:                                                      # AllTracebackStream + finish_alignment
                        ok, _, src, snk, cig = O.banded_sw_traceback(band, aln_type, oracle.ED_SW, pat, txt)
                        ed, _ = O.finish_alignment(pat, txt, cig, src[0]) if ok else (0, None)
                        details.append((src, snk, ed, cig))
    return (records, details) if want_cigars else records
