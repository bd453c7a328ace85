"""Time the q-gram index and filter (nvbio_qgram_*, nvbio_generate_qgrams) on one GPU, at two shapes:
  qmap    a set index over 1 M x 150 bp reads (1% substitutions) and their reverse complements, Q = 20, seed interval 10, LUT 12; a
          seeded 100 Mbp genome streamed through it in batches of 16 M q-grams: per batch extract+sort, rank, locate, merge (interval 16)
  string  a string index over the 100 Mbp genome, Q = 20, LUT 12; rank of 16 M of its q-grams (sorted, as qmap feeds them)
Device events around each call after warm-up.  Also: the q-gram entries each rank query loads (the bucket's lower_bound steps plus
the final compare, from the LUT bucket sizes of the queries -- the LUT's two words and the two slots of a hit come on top), and the
resulting random loads/s, to set against the ~47 G random lines/s the seed pass measured.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402


def entries_per_query(amd, index, queries):
    """mean q-gram entries one range lookup loads: the lower_bound steps over its LUT bucket (ceil(log2(size + 1))) + the compare"""
    a = index.arrays()
    v = index.view()
    lut = amd.u32(a["lut"]).astype(np.int64)
    k = (queries.cpu().numpy().view(np.uint64) >> np.uint64((v.q - v.qlut) * v.symbol_size)).astype(np.int64)
    b = lut[k + 1] - lut[k]
    return float(np.mean(np.ceil(np.log2(b + 1)) + 1)), float(np.mean(b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=100_000_000)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--batch", type=int, default=16 << 20)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    import torch
    import oracle
    amd = ge.load_package()
    orc = oracle.Oracle()
    rng = np.random.default_rng(2024)
    G = a.genome
    genome = rng.integers(0, 4, G, dtype=np.uint8)
    gpacked = torch.from_numpy(orc.pack2(genome).view(np.int32)).cuda()
    starts = rng.integers(0, G - a.len, a.reads)
    reads = genome[starts[:, None] + np.arange(a.len)]
    m = rng.random(reads.shape) < 0.01
    reads[m] = rng.integers(0, 4, int(m.sum()))
    both = np.empty((2 * a.reads, a.len), np.uint8)
    both[0::2] = reads
    both[1::2] = 3 - reads[:, ::-1]
    del reads, m
    rset = amd.PackedStringSet(orc.pack4(both.reshape(-1)), 4, 2 * a.reads, fixed_len=a.len)
    del both, genome
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731

    def timed(f):
        e0, e1 = ev(), ev()
        e0.record()
        r = f()
        e1.record()
        torch.cuda.synchronize()
        return r, e0.elapsed_time(e1)

    out = dict(workload="qgram", genome=G, reads=a.reads, read_len=a.len, q=20, qlut=12, batch=a.batch)
    # ---- qmap: set index over reads + reverse complements, the genome streamed in batches ----
    t_build = []
    for step in range(a.warmup + a.steps):
        idx, t = timed(lambda: amd.QGramSetIndex.build(rset, 20, 2, 10, 12))
        if step >= a.warmup:
            t_build.append(t)
        if step + 1 < a.warmup + a.steps:
            idx.close()
    out.update(set_n_qgrams=idx.n_qgrams, set_n_unique=idx.n_unique, set_build_ms=float(np.median(t_build)),
               set_build_mqgrams_per_s=idx.n_qgrams / (np.median(t_build) * 1e-3) / 1e6, set_index_bytes=idx.device_bytes())
    qf = amd.QGramFilter()
    per = dict(extract_sort=[], rank=[], locate=[], merge=[])
    hits_total = merged_total = 0
    ent = None
    for step in range(a.warmup + a.steps):
        tot = dict(extract_sort=0.0, rank=0.0, locate=0.0, merge=0.0)
        h_tot = m_tot = 0
        for b in range(0, G, a.batch):
            n = min(a.batch, G - b)
            (g, p), t0 = timed(lambda: amd.generate_qgrams(20, 2, gpacked, 2, G, b, n, sort=True))
            nh, t1 = timed(lambda: qf.rank(idx, g, p))
            hits, t2 = timed(lambda: qf.locate(0, nh))
            (mg, _), t3 = timed(lambda: qf.merge(16, hits))
            tot["extract_sort"] += t0; tot["rank"] += t1; tot["locate"] += t2; tot["merge"] += t3
            h_tot += nh; m_tot += mg.shape[0]
            if ent is None:
                ent = entries_per_query(amd, idx, g)
            del hits, mg
        if step >= a.warmup:
            for k in per:
                per[k].append(tot[k])
        hits_total, merged_total = h_tot, m_tot
    n_batches = (G + a.batch - 1) // a.batch
    rk = float(np.median(per["rank"]))
    out.update(qmap_batches=n_batches, qmap_ms_total={k: float(np.median(v)) for k, v in per.items()},
               qmap_ms_per_batch={k: float(np.median(v)) / n_batches for k, v in per.items()},
               qmap_rank_qgrams_per_s=G / (rk * 1e-3), qmap_hits=hits_total, qmap_merged=merged_total,
               qmap_entries_per_query=ent[0], qmap_mean_bucket=ent[1],
               qmap_rank_entry_loads_per_s=G * ent[0] / (rk * 1e-3))
    idx.close()
    # ---- string index over the genome ----
    t_build = []
    for step in range(a.warmup + a.steps):
        sidx, t = timed(lambda: amd.QGramIndex.build(gpacked, 2, G, 20, 2, 12))
        if step >= a.warmup:
            t_build.append(t)
        if step + 1 < a.warmup + a.steps:
            sidx.close()
    g, p = amd.generate_qgrams(20, 2, gpacked, 2, G, 0, a.batch, sort=True)
    t_rank = []
    for step in range(a.warmup + a.steps):
        nh, t = timed(lambda: qf.rank(sidx, g, p))
        if step >= a.warmup:
            t_rank.append(t)
    ent = entries_per_query(amd, sidx, g)
    rk = float(np.median(t_rank))
    out.update(string_build_ms=float(np.median(t_build)), string_build_mqgrams_per_s=G / (np.median(t_build) * 1e-3) / 1e6,
               string_n_unique=sidx.n_unique, string_rank_ms=rk, string_rank_qgrams_per_s=a.batch / (rk * 1e-3), string_rank_hits=nh,
               string_entries_per_query=ent[0], string_mean_bucket=ent[1], string_rank_entry_loads_per_s=a.batch * ent[0] / (rk * 1e-3))
    sidx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
