"""Time the all-mapping mode (amd.all_mapping -> nvbio_host_all_mapping) on one GPU: 1 M seeded reads of 100 bp against a seeded 100 Mbp text
with a planted repeat family (100 copies of a 500 bp unit, 2 % apart; 5 % of the reads come from it), 1.5 % substitutions, default
parameters (seed 22, max_dist 15, band 31, end-to-end edit distance), scores only.  Wall-clock around the whole call (the loop reads
counters back per chunk, so device events would miss its host time), after warm-up; median and spread of --steps repeats for
  one pass over all seed indices        (the default)
  one pass per seed index               (per_seed_passes = 1, the reference's schedule)
  one pass, duplicates removed          (unique = 1)
Prints one JSON line; --out also writes it to a file.  A measurement, not a gate: no threshold."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=100_000_000)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=100)
    ap.add_argument("--copies", type=int, default=100)
    ap.add_argument("--family-reads", type=float, default=0.05)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import oracle
    amd = ge.load_package()
    orc = oracle.Oracle()
    rng = np.random.default_rng(2025)
    G, R, M, U = a.genome, a.reads, a.len, 500
    text = rng.integers(0, 4, G, dtype=np.uint8)
    unit = rng.integers(0, 4, U, dtype=np.uint8)
    fam = rng.choice(G // 1000 - 2, a.copies, replace=False) * 1000 + 200
    for p in fam:
        c = unit.copy()
        m = rng.random(U) < 0.02
        c[m] = rng.integers(0, 4, int(m.sum()))
        text[p:p + U] = c
    starts = rng.integers(0, G - M, R)
    n_fam = int(R * a.family_reads)
    starts[:n_fam] = fam[rng.integers(0, a.copies, n_fam)] + rng.integers(0, U - M, n_fam)
    reads = text[starts[:, None] + np.arange(M)]
    m = rng.random(reads.shape) < 0.015
    reads[m] = rng.integers(0, 4, int(m.sum()))
    rcm = rng.random(R) < 0.5
    reads[rcm] = 3 - reads[rcm][:, ::-1]
    genome2 = orc.pack2(text)
    fmi = amd.FMIndex.build(genome2, G, kmer_len=8, sa_int=16)
    g_dev = torch.from_numpy(genome2.view(np.int32)).cuda()
    r_dev = torch.from_numpy(orc.pack4(np.ascontiguousarray(reads[:, ::-1]).reshape(-1)).view(np.int32)).cuda()
    del reads, text

    def run(**kw):
        times, res = [], None
        for step in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = amd.all_mapping(fmi, g_dev, G, r_dev, R, M, amd.AllMappingParams(**kw), capacity=1 << 20)
            torch.cuda.synchronize()
            if step >= a.warmup:
                times.append((time.perf_counter() - t0) * 1e3)
        med = float(np.median(times))
        return dict(ms=med, ms_min=float(min(times)), ms_max=float(max(times)), ms_all=times, n_hits=res["n_hits"], n_scored=res["n_scored"],
                    n_alignments=res["n_alignments"], chunks=res["chunks"], hits_per_s=res["n_hits"] / (med * 1e-3),
                    alignments_per_s=res["n_alignments"] / (med * 1e-3), scored_over_hits=res["n_scored"] / max(res["n_hits"], 1))

    try:
        commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=os.path.dirname(os.path.abspath(__file__)), text=True).strip()
    except Exception:
        commit = None
    out = dict(workload="all_mapping", genome=G, reads=R, read_len=M, copies=a.copies, family_reads=a.family_reads, warmup=a.warmup, steps=a.steps,
               commit=commit, one_pass=run(), per_seed_passes=run(per_seed_passes=True), unique=run(unique=True))
    out["per_seed_over_one_pass"] = out["per_seed_passes"]["ms"] / out["one_pass"]["ms"]
    out["unique_over_one_pass"] = out["unique"]["ms"] / out["one_pass"]["ms"]
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    fmi.close()


if __name__ == "__main__":
    main()
