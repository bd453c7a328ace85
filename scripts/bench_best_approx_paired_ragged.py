"""Cost of the ragged route of nvBowtie's PAIRED best-approx loop (nvbio_host_best_approx_paired_ragged) next to the uniform one, on one MI355X:
  (a) the uniform entry point (nvbio_host_best_approx_paired: the uniform instantiations of the nvbio_pe_* kernels, the code path of the commit before
      the ragged route existed) on --pairs pairs of 2 x 150 bp, FR, insert N(350, 50) -- the shape of bench.py's paired_end_1M.nvbowtie_loop;
  (b) the ragged entry point on the same pairs expressed through offsets;
  (c) the ragged entry point on the same pairs with every mate cut to a length uniform in 100..150.
(a) and (b) alternate --runs times (DESIGN section 5's A/B); (c) runs --runs times.  Writes one JSON document (default
profiles/best_approx_paired_ragged_bench.json): the three times, the ratio b / a of the medians, the run-to-run spread of each and the pass / extension
counters.  There is no threshold: parity of the results is the gate (tests/test_gpu_best_approx_paired_ragged.py), and (a) == (b) array for array is
asserted here as well.

    python scripts/bench_best_approx_paired_ragged.py [--ref-len 3e8] [--pairs 1e6] [--runs 3] [--commit ID] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COUNTERS = ("n_extensions", "n_opposite", "passes", "multi_passes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-len", type=float, default=3e8)
    ap.add_argument("--pairs", type=float, default=1e6)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--kmer", type=int, default=12)
    ap.add_argument("--commit", default="", help="the commit the numbers are taken on (recorded as given)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "best_approx_paired_ragged_bench.json"))
    args = ap.parse_args()
    import importlib

    import torch

    import __graft_entry__ as ge
    import bench
    amd = ge.load_package()
    pipeline = importlib.import_module("nvbio_gpl_amd.pipeline")
    dev = "cuda:0"
    n, P, M = int(args.ref_len), int(args.pairs), args.read_len
    genome = bench.make_reference(n, dev, 1)
    t0 = time.perf_counter()
    fmi = amd.FMIndex.build(genome, n, kmer_len=args.kmer, sa_int=1)
    torch.cuda.synchronize(); build_s = time.perf_counter() - t0
    # the pairs of bench.py's paired_end_1M: mate 1 forward at the fragment's start, mate 2 reverse-complemented at its end, half of the pairs swapped
    g = torch.Generator(device=dev); g.manual_seed(77)
    ins = torch.clamp((torch.randn(P, device=dev, generator=g) * 50 + 350).round().to(torch.int64), 160, 500)
    left = torch.randint(0, n - 520, (P,), device=dev, generator=g, dtype=torch.int64)
    j = torch.arange(M, device=dev, dtype=torch.int64)[None, :]

    def mate(posv, seed):
        gg = torch.Generator(device=dev); gg.manual_seed(seed)
        symv = bench.genome_symbols(genome, posv[:, None] + j)
        rndv = torch.randint(0, 4, (P, M), device=dev, generator=gg, dtype=torch.uint8)
        sub = torch.rand(P, M, device=dev, generator=gg) < 0.01
        return torch.where(sub, (symv + 1 + rndv % 3) % 4, symv)

    m1 = mate(left, 1); m2 = 3 - mate(left + ins - M, 2).flip(1)
    swap = torch.rand(P, device=dev, generator=g) < 0.5
    stored = [torch.where(swap[:, None], m2, m1).flip(1).contiguous(), torch.where(swap[:, None], m1, m2).flip(1).contiguous()]     # nvBowtie stores reads reversed
    packed = [bench.pack4(s.reshape(-1)) for s in stored]
    uniform = [pipeline.ReadBatch(p, P, M) for p in packed]
    as_offsets = [pipeline.ReadBatch(p, P, M, offsets=(torch.arange(P + 1, device=dev, dtype=torch.int64) * M).to(torch.int32)) for p in packed]
    ragged = []
    for k, s in enumerate(stored):
        flat, offs, _, lens = bench.make_ragged(s, 100, dev, 3 + k)
        ragged.append(pipeline.ReadBatch(bench.pack4(flat), P, int(lens.max()), offsets=offs))
    params = pipeline.SeedExtendParams.end_to_end()

    def run(batches):
        torch.cuda.synchronize(); t = time.perf_counter()
        out = pipeline.nvbowtie_best_approx_paired_host(fmi, genome, n, batches[0], batches[1], params)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    _, ua = run(uniform); _, ub = run(as_offsets); _, uc = run(ragged)           # warm, at full size: scratch blocks are cached per stream by size
    for k in ("best_a", "best_o"):
        assert torch.equal(ua[k], ub[k]), k
    for k in COUNTERS:
        assert ua[k] == ub[k], k
    a, b, c = [], [], []
    for _ in range(args.runs):
        a.append(run(uniform)[0]); b.append(run(as_offsets)[0])
    for _ in range(args.runs):
        c.append(run(ragged)[0])
    med = lambda v: sorted(v)[len(v) // 2]
    spread = lambda v: (max(v) - min(v)) / med(v)
    paired = lambda o: float(((((o["best_a"][:, 0, 3] >> 2) & 1) == 1) & (o["best_a"][:, 0, 1] != -1)).float().mean())
    doc = {"what": "nvBowtie paired best-approx C++ host loop, uniform entry (a) vs ragged entry on the same pairs through offsets (b) vs ragged entry on mate "
                   "lengths 100..150 (c)",
           "commit": args.commit, "device": torch.cuda.get_device_name(0), "ref_len": n, "pairs": P, "read_len": M, "kmer": args.kmer, "index_build_s": build_s,
           "a_uniform_ms": a, "b_ragged_same_pairs_ms": b, "c_ragged_100_150_ms": c,
           "a_median_ms": med(a), "b_median_ms": med(b), "c_median_ms": med(c), "b_over_a": med(b) / med(a),
           "a_spread": spread(a), "b_spread": spread(b), "c_spread": spread(c), "a_equals_b": True,
           "counters": {"a": {k: ua[k] for k in COUNTERS}, "c": {k: uc[k] for k in COUNTERS}},
           "paired_fraction": {"a": paired(ua), "c": paired(uc)}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    fmi.close()


if __name__ == "__main__":
    main()
