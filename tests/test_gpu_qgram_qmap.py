"""GPU: the reference's qmap example (examples/qmap/qmap.cu map()) composed over the C ABI on a small genome: a q-gram set index over
the reads and their reverse complements (Q = 20, seed interval 10, LUT 12), the genome's q-grams streamed in batches through rank /
locate / merge (interval 16), windows by qmap's genome_infixes<31> rule (examples/qmap/alignment.h:60-90), the band-31 SEMI_GLOBAL
Myers aligner, and the best score per read (string id / 2 merges the strands).

min_score is -32768: the Myers aligner truncates min_score to an int16 as the reference's code does, so the default
(Field_traits<int32>::min()) would become 0 and only distance-0 columns would be reported (see nvbio_banded_myers_score)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BAND = 31


def test_qmap_composition(amd, orc):
    import torch
    rng = np.random.default_rng(2024)
    G, R, L = 300_000, 400, 150
    genome = rng.integers(0, 4, G, dtype=np.uint8)
    starts = rng.integers(0, G - L, R)
    edits = rng.integers(0, 4, R)                                      # 0..3 substitutions
    edits[::4] = 0
    reverse = rng.random(R) < 0.5
    reads = []
    for s, k, rv in zip(starts, edits, reverse):
        r = genome[s:s + L].copy()
        for p in rng.choice(L, k, replace=False):
            r[p] = (r[p] + rng.integers(1, 4)) % 4
        reads.append((3 - r[::-1]).astype(np.uint8) if rv else r)
    both = [x for r in reads for x in (r, (3 - r[::-1]).astype(np.uint8))]          # string 2i = read i, 2i + 1 = its reverse complement
    offs = np.zeros(len(both) + 1, np.uint32)
    offs[1:] = np.cumsum([len(x) for x in both])
    packed_reads = orc.pack4(np.concatenate(both))
    rset = amd.PackedStringSet(packed_reads, 4, len(both), offsets=offs, ranges=True)
    index = amd.QGramSetIndex.build(rset, 20, 2, 10, 12)
    gpacked = orc.pack2(genome)
    qf = amd.QGramFilter()
    best = np.full(R, -(1 << 20), np.int64)
    batch = 1 << 16
    for b in range(0, G, batch):
        n = min(batch, G - b)
        g, p = amd.generate_qgrams(20, 2, gpacked, 2, G, b, n, sort=True)
        n_hits = qf.rank(index, g, p)
        if n_hits == 0:
            continue
        hits = qf.locate(0, n_hits)
        merged, counts = qf.merge(16, hits)
        m = amd.u32(merged).reshape(-1, 2)
        assert int(amd.u32(counts).astype(np.int64).sum()) == n_hits
        diag, sid = m[:, 0].astype(np.int64), m[:, 1].astype(np.int64)
        read_len = (offs[sid + 1] - offs[sid]).astype(np.int64)
        wb = np.where(diag > BAND // 2, diag - BAND // 2, 0)
        we = np.minimum(wb + read_len + BAND, G)
        ok = we > wb                                                   # a wrapped diagonal gives no window
        aln = amd.AlignmentBatch(packed_reads, 4, offs, gpacked, 2, wb[ok].astype(np.uint32), we[ok].astype(np.uint32),
                                 read_id=sid[ok].astype(np.uint32), max_read_len=L)
        scores, _ = amd.batch_banded_myers_score(BAND, amd.SEMI_GLOBAL, aln, min_score=-32768)
        sc = scores.cpu().numpy().astype(np.int64)
        np.maximum.at(best, sid[ok] // 2, sc)
    torch.cuda.synchronize()
    exact = edits == 0
    assert exact.sum() > 0 and np.all(best[exact] == 0)
    assert np.all(best >= -edits), [(i, int(best[i]), int(edits[i])) for i in np.nonzero(best < -edits)[0][:10]]
    index.close()
