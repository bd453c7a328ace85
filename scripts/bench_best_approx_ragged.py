"""Cost of the ragged route of nvBowtie's best-approx loop (nvbio_host_best_approx_ragged) next to the uniform one, on one MI355X:
  (a) the uniform entry point (nvbio_host_best_approx: the uniform instantiations of the seed-hit kernels, the code path of the commit before the
      ragged route existed) on --reads x 150 bp reads -- the nvbowtie_mode inputs of bench.py at a tenth of their size by default;
  (b) the ragged entry point on the same reads expressed through offsets;
  (c) the ragged entry point on the same reads cut to lengths uniform in 100..150.
(a) and (b) alternate --runs times (DESIGN section 5's A/B); (c) runs --runs times.  Writes one JSON document (default
profiles/best_approx_ragged_bench.json): the times, the ratio b / a of the medians and the run-to-run spread of each.  There is no threshold: parity
of the results is the gate (tests/test_gpu_best_approx_ragged.py), and (a) == (b) array for array is asserted here as well.

    python scripts/bench_best_approx_ragged.py [--ref-len 3e8] [--reads 1e6] [--runs 3] [--commit ID] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-len", type=float, default=3e8)
    ap.add_argument("--reads", type=float, default=1e6)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--kmer", type=int, default=12)
    ap.add_argument("--commit", default="", help="the commit the numbers are taken on (recorded as given)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "best_approx_ragged_bench.json"))
    args = ap.parse_args()
    import importlib

    import torch

    import __graft_entry__ as ge
    import bench
    amd = ge.load_package()
    pipeline = importlib.import_module("nvbio_gpl_amd.pipeline")
    dev = "cuda:0"
    n, R, M = int(args.ref_len), int(args.reads), args.read_len
    genome = bench.make_reference(n, dev, 1)
    reads_sym, _, _ = bench.make_reads(genome, n, R, M, dev, 2)
    t0 = time.perf_counter()
    fmi = amd.FMIndex.build(genome, n, kmer_len=args.kmer, sa_int=1)
    torch.cuda.synchronize(); build_s = time.perf_counter() - t0
    params = pipeline.SeedExtendParams.end_to_end()
    stored = reads_sym.flip(1).contiguous()                                    # nvBowtie stores reads reversed (io::REVERSE)
    stored4 = bench.pack4(stored.reshape(-1))
    uniform = pipeline.ReadBatch(stored4, R, M)
    as_offsets = pipeline.ReadBatch(stored4, R, M, offsets=(torch.arange(R + 1, device=dev, dtype=torch.int64) * M).to(torch.int32))
    flat, offs, _, lens = bench.make_ragged(stored, 100, dev, 3)
    ragged = pipeline.ReadBatch(bench.pack4(flat), R, int(lens.max()), offsets=offs)

    def run(batch):
        torch.cuda.synchronize(); t = time.perf_counter()
        out = pipeline.nvbowtie_best_approx_host(fmi, genome, n, batch, params)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    _, ua = run(uniform); _, ub = run(as_offsets); _, uc = run(ragged)           # warm, at full size: scratch blocks are cached per stream by size
    for k in ("best_score", "best_loc", "best_rc", "second_score", "second_loc", "second_rc"):
        assert torch.equal(ua[k], ub[k]), k
    for k in ("n_extensions", "passes", "multi_passes", "seeding_passes"):
        assert ua[k] == ub[k], k
    a, b, c = [], [], []
    for _ in range(args.runs):
        a.append(run(uniform)[0]); b.append(run(as_offsets)[0])
    for _ in range(args.runs):
        c.append(run(ragged)[0])
    med = lambda v: sorted(v)[len(v) // 2]
    spread = lambda v: (max(v) - min(v)) / med(v)
    doc = {"what": "nvBowtie best-approx C++ host loop, uniform entry (a) vs ragged entry on the same reads through offsets (b) vs ragged entry on lengths 100..150 (c)",
           "commit": args.commit, "device": torch.cuda.get_device_name(0), "ref_len": n, "reads": R, "read_len": M, "kmer": args.kmer, "index_build_s": build_s,
           "a_uniform_ms": a, "b_ragged_same_reads_ms": b, "c_ragged_100_150_ms": c,
           "a_median_ms": med(a), "b_median_ms": med(b), "c_median_ms": med(c), "b_over_a": med(b) / med(a),
           "a_spread": spread(a), "b_spread": spread(b), "c_spread": spread(c), "a_equals_b": True,
           "counters": {"a": {k: ua[k] for k in ("n_extensions", "passes", "multi_passes", "seeding_passes")},
                        "c": {k: uc[k] for k in ("n_extensions", "passes", "multi_passes", "seeding_passes")}},
           "aligned_fraction": {"a": float((ua["best_loc"] >= 0).float().mean()), "c": float((uc["best_loc"] >= 0).float().mean())}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    fmi.close()


if __name__ == "__main__":
    main()
