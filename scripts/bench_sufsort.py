"""Time the set suffix sort and the set BWT (nvbio_set_suffix_sort, nvbio_set_bwt) on one GPU, on three sets of the shape of the
reference's nvSetBWT input (reads x 100 bp, 2 bits):
  reads   sampled at 30x from a seeded genome: most suffixes tie with the overlapping reads' for several words
  random  the same number of random reads: next to nothing ties after the first word
  all-A   every suffix ties with every longer one in every word
Device events around each library call, after one warm-up; medians of 3 (every step's time is kept beside the median).  Per set: suffixes/s of the sort and of the BWT, the peak
device bytes the call allocated and the suffixes that entered each round's sort.  In the same run, the cost of the reference's scheme
on this chip: ceil( 101 / 14 ) = 8 radix sorts of all n (32-bit key, 32-bit value) pairs, rocPRIM alone (scripts/ubench/radix_pairs.hip,
run as a child process); reported as a ratio, reference scheme / this library's sort.  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

UBENCH = os.path.join(ROOT, "scripts", "ubench", "radix_pairs")


def reference_scheme_ms(n, sorts, steps):
    if not os.path.exists(UBENCH):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", UBENCH + ".hip", "-o", UBENCH])
    return json.loads(subprocess.run([UBENCH, str(n), str(sorts), str(steps)], check=True, capture_output=True, text=True, timeout=600).stdout)


def packed2(torch, amd, syms):
    flat = syms.reshape(-1).to(torch.int64)
    flat = torch.cat([flat, torch.zeros((-flat.numel()) % 16 + 64, dtype=torch.int64, device=flat.device)]).reshape(-1, 16)
    words = (flat << (30 - 2 * torch.arange(16, device=flat.device))).sum(dim=1)
    words = torch.where(words >= (1 << 31), words - (1 << 32), words).to(torch.int32)
    return amd.PackedStringSet(words, 2, syms.shape[0], fixed_len=syms.shape[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=100)
    ap.add_argument("--coverage", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sufsort_bench.json"))
    a = ap.parse_args()
    import torch
    amd = ge.load_package()
    dev = "cuda:0"
    N, L = a.reads, a.len
    g = torch.Generator(device=dev).manual_seed(2024)
    genome = torch.randint(0, 4, (N * L // a.coverage,), dtype=torch.uint8, device=dev, generator=g)
    starts = torch.randint(0, genome.numel() - L + 1, (N,), device=dev, generator=g)
    sets = dict(reads=lambda: genome[starts[:, None] + torch.arange(L, device=dev)],
                random=lambda: torch.randint(0, 4, (N, L), dtype=torch.uint8, device=dev, generator=g),
                all_a=lambda: torch.zeros((N, L), dtype=torch.uint8, device=dev))
    n = N * (L + 1)
    suf = torch.empty((n, 2), dtype=torch.int32, device=dev)
    glb = torch.empty(n, dtype=torch.int32, device=dev)
    bwt = torch.empty(n, dtype=torch.uint8, device=dev)
    import ctypes
    lib, stream = amd.lib(), amd._stream_ptr(dev)

    def median_of(f):
        ts = []
        for step in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = f()
            e1.record()
            torch.cuda.synchronize()
            if step >= a.warmup:
                ts.append(e0.elapsed_time(e1))
        return r, float(np.median(ts)), ts

    out = dict(workload="sufsort", n_reads=N, read_len=L, coverage=a.coverage, n_suffixes=n, steps=a.steps, warmup=a.warmup)
    for name, make in sets.items():
        sset = packed2(torch, amd, make())
        ss = sset.c_struct()

        def sort():
            cnt, st = ctypes.c_uint32(0), amd._SufsortStats()
            amd._check(lib.nvbio_set_suffix_sort(0, ctypes.byref(ss), 0, amd._ptr(suf), amd._ptr(glb), ctypes.c_uint64(n), ctypes.byref(cnt),
                                                 ctypes.byref(st), stream))
            return st.as_dict()

        def set_bwt():
            cnt, st = ctypes.c_uint32(0), amd._SufsortStats()
            amd._check(lib.nvbio_set_bwt(0, ctypes.byref(ss), 0, amd._ptr(bwt), None, ctypes.c_uint64(n), ctypes.byref(cnt), ctypes.byref(st), stream))
            return st.as_dict()

        st, t_sort, ts_sort = median_of(sort)
        _, t_bwt, ts_bwt = median_of(set_bwt)
        out[name] = dict(sort_ms=t_sort, sort_msuffixes_per_s=n / (t_sort * 1e-3) / 1e6, bwt_ms=t_bwt, bwt_msuffixes_per_s=n / (t_bwt * 1e-3) / 1e6,
                         peak_bytes=st["peak_bytes"], rounds=st["rounds"], sorted_per_round=st["sorted_per_round"][:st["rounds"]],
                         symbols_per_word=st["symbols_per_word"], sort_ms_steps=ts_sort, bwt_ms_steps=ts_bwt)
        del sset
    del suf, glb, bwt, genome, starts
    torch.cuda.empty_cache()
    ref = reference_scheme_ms(n, -(-(L + 1) // 14), a.steps)
    out["reference_scheme"] = ref
    for name in sets:
        out[name]["reference_scheme_over_sort"] = ref["ms"] / out[name]["sort_ms"]
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
