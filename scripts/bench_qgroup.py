"""Time the q-group index (nvbio_qgroup_*) against the sorted q-gram index of the same data on one GPU, in the same run:
  string  an index over a seeded 100 Mbp genome; rank, locate and merge (interval 16) of 16 M of its q-grams (sorted, as qmap feeds
          them)
  set     an index over 1 M x 150 bp reads (1% substitutions) and their reverse complements, seed interval 10; rank, locate and
          merge of the genome's first 16 M q-grams (sorted)
  all-A   the build of a 10 Mbp all-A text: every position goes to one bit, one counter and one cursor
Q = 16, two bits (the reference's own test value, qgram_test.cu:687; qmap's Q = 20 needs a 2^40-bit table and is outside the q-group
limit); the sorted index at Q = 16 with LUT 12.  Device events around each call after warm-up; medians.  Also the dependent loads
of one range lookup: the q-group index's two (the (bits, rank) pair, then the SS pair), and the sorted index's LUT pair + the
lower_bound steps over its LUT bucket + the compare + the slots pair.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
from bench_qgram import entries_per_query  # noqa: E402

Q, SS, QLUT = 16, 2, 12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=100_000_000)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--batch", type=int, default=16 << 20)
    ap.add_argument("--all-a", type=int, default=10_000_000)
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
    apacked = torch.zeros(a.all_a // 16 + 16, dtype=torch.int32, device="cuda")
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731

    def timed(f):
        e0, e1 = ev(), ev()
        e0.record()
        r = f()
        e1.record()
        torch.cuda.synchronize()
        return r, e0.elapsed_time(e1)

    def median_of(f, keep=False):
        """the median time of f over the steps after the warm-up; the last result when keep, else every result is closed"""
        ts, r = [], None
        for step in range(a.warmup + a.steps):
            r, t = timed(f)
            if step >= a.warmup:
                ts.append(t)
            if not keep or step + 1 < a.warmup + a.steps:
                if hasattr(r, "close"):
                    r.close()
        return r, float(np.median(ts))

    builders = dict(
        qgroup=dict(string=lambda t, n: amd.QGroupIndex.build(t, 2, n, Q, SS), set=lambda: amd.QGroupSetIndex.build(rset, Q, SS, 10)),
        qgram=dict(string=lambda t, n: amd.QGramIndex.build(t, 2, n, Q, SS, QLUT), set=lambda: amd.QGramSetIndex.build(rset, Q, SS, 10, QLUT)))
    g, p = amd.generate_qgrams(Q, SS, gpacked, 2, G, 0, a.batch, sort=True)
    out = dict(workload="qgroup", genome=G, reads=a.reads, read_len=a.len, q=Q, symbol_size=SS, qgram_qlut=QLUT, batch=a.batch, all_a=a.all_a)
    qf = amd.QGramFilter()
    for kind, b in builders.items():
        for form, build in (("string", lambda: b["string"](gpacked, G)), ("set", b["set"])):
            idx, t_build = median_of(build, keep=True)
            r = dict(build_ms=t_build, build_mqgrams_per_s=idx.n_qgrams / (t_build * 1e-3) / 1e6, n_qgrams=idx.n_qgrams, n_unique=idx.n_unique,
                     index_bytes=idx.device_bytes())
            nh, t_rank = median_of(lambda: qf.rank(idx, g, p))
            hits, t_locate = median_of(lambda: qf.locate(0, nh))
            mg, t_merge = median_of(lambda: qf.merge(16, hits))
            r.update(rank_ms=t_rank, rank_qgrams_per_s=a.batch / (t_rank * 1e-3), hits=nh, locate_ms=t_locate,
                     locate_hits_per_s=nh / (t_locate * 1e-3), merge_ms=t_merge, merged=int(mg[0].shape[0]))
            if kind == "qgram":
                ent = entries_per_query(amd, idx, g)
                r.update(dependent_loads_per_query=1 + ent[0] + 1, lower_bound_entries=ent[0], mean_bucket=ent[1])
            else:
                r.update(dependent_loads_per_query=2)
            out["%s_%s" % (kind, form)] = r
            del hits, mg
            idx.close()
        _, t = median_of(lambda: b["string"](apacked, a.all_a))
        out["%s_all_a_build_ms" % kind] = t
    print(json.dumps(out))


if __name__ == "__main__":
    main()
