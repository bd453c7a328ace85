"""Time the MEM filter (nvbio_mem_filter_rank / _locate) on one GPU: 1 M seeded reads of 150 bp (1% substitutions) against a seeded
100 Mbp text, forward and reverse indices built on the GPU, default parameters.  Device events around each call after warm-up.
Each timed rank must be one library call (rank_library_calls: a call that had to grow a buffer repeats every pass).
Prints one JSON line: ms, MEMs/s and reads/s of rank and locate, and the bwt_occ records the passes gathered (per read and as
records/s -- each is one random 32-byte line)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=100_000_000)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    import torch
    import oracle
    amd = ge.load_package()
    orc = oracle.Oracle()
    rng = np.random.default_rng(2024)
    text = rng.integers(0, 4, a.genome, dtype=np.uint8)
    f = amd.FMIndex.build(orc.pack2(text), a.genome, kmer_len=0, sa_int=16)
    r = amd.FMIndex.build(orc.pack2(text[::-1].copy()), a.genome, kmer_len=0, sa_int=16)
    starts = rng.integers(0, a.genome - a.len, a.reads)
    reads = text[starts[:, None] + np.arange(a.len)]
    m = rng.random(reads.shape) < 0.01
    reads[m] = rng.integers(0, 4, int(m.sum()))
    ss = amd.PackedStringSet(orc.pack4(reads.reshape(-1)), 4, a.reads, fixed_len=a.len)
    del reads, text
    mf = amd.MEMFilter()
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    t_rank, t_loc, attempts = [], [], []
    for step in range(a.warmup + a.steps):
        e0, e1, e2 = ev(), ev(), ev()
        e0.record()
        n_mems = mf.rank(f, r, ss)
        e1.record()
        hits = mf.locate(0, n_mems)
        e2.record()
        torch.cuda.synchronize()
        if step >= a.warmup:
            t_rank.append(e0.elapsed_time(e1)); t_loc.append(e1.elapsed_time(e2)); attempts.append(mf.attempts)
    rk, lc = float(np.median(t_rank)), float(np.median(t_loc))
    out = dict(workload="mem_filter", genome=a.genome, reads=a.reads, read_len=a.len, n_ranges=mf.n_ranges, n_mems=n_mems,
               rank_ms=rk, locate_ms=lc, rank_library_calls=attempts, rank_ms_all=t_rank, locate_ms_all=t_loc,
               rank_mems_per_s=n_mems / (rk * 1e-3), rank_reads_per_s=a.reads / (rk * 1e-3),
               locate_mems_per_s=n_mems / (lc * 1e-3),
               records=mf.records, records_per_read=mf.records / a.reads, rank_records_per_s=mf.records / (rk * 1e-3))
    print(json.dumps(out))
    del hits
    f.close(); r.close()


if __name__ == "__main__":
    main()
