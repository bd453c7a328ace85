"""Time the FASTA parser (nvbio_fasta_scan, nvbio_fasta_encode) on one GPU: a synthetic reference of --bytes bytes already in HBM -- --seqs
sequences in 60-column lines, --n-runs runs of N of --n-run-len symbols each -- parsed as ONE chunk from a fresh state.  Device events
around each call, medians of --steps runs after --warmup:
  scan      nvbio_fasta_scan: the tiles' functions, their scan, the tiles' counts, their scan, the summary
  encode    nvbio_fasta_encode: zeroing, the emit pass (text2, names, sequence and hole tables), the state
  d2d       a device-to-device copy of the text's bytes
  h2d       a copy of the text from pinned host memory: what delivers the text to the parser
Per-launch times come from one `rocprofv3 --kernel-trace --stats` run of this script.  Prints one JSON line and writes it to --out."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

LINE = 61


def make_text(torch, nbytes, n_seqs, n_runs, run_len, dev):
    """lines of 60 random ACGT and a newline; every (lines / n_seqs)-th line is a header `>chrNN synthetic ...`; runs of N laid over the body"""
    g = torch.Generator(device=dev).manual_seed(11)
    lines = nbytes // LINE
    t = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)[torch.randint(0, 4, (lines, LINE), device=dev, generator=g)]
    t[:, LINE - 1] = 10
    flat = t.reshape(-1)
    rng = np.random.default_rng(11)
    for at in rng.integers(0, lines * LINE - run_len, n_runs):
        span = flat[int(at):int(at) + run_len]
        span[span != 10] = ord("N")
    per = lines // n_seqs
    for i in range(n_seqs):
        head = (b">chr%02d synthetic" % (i + 1)).ljust(LINE - 1) + b"\n"
        t[i * per] = torch.tensor(list(head), dtype=torch.uint8, device=dev)
    return flat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--seqs", type=int, default=24)
    ap.add_argument("--n-runs", type=int, default=200)
    ap.add_argument("--n-run-len", type=int, default=50000)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fasta_parse_bench.json"))
    a = ap.parse_args()
    import torch
    amd = ge.load_package()
    dev = "cuda:0"
    text = make_text(torch, a.bytes, a.seqs, a.n_runs, a.n_run_len, dev)
    nb = text.numel()
    lib, stream = amd.lib(), amd._stream_ptr(dev)
    temp, temp_bytes = amd._temp_for(lib.nvbio_fasta_temp_bytes, nb, device=dev)
    state0 = amd.fasta_state_init(11, dev)
    state = state0.clone()
    summary = torch.zeros(8, dtype=torch.int32, device=dev)
    stp = ctypes.cast(state.data_ptr(), ctypes.POINTER(amd._FastaState))
    sp = ctypes.cast(summary.data_ptr(), ctypes.POINTER(amd._FastaSummary))
    words = (nb + 15) // 16 + 4
    max_seqs, max_holes = a.seqs + 16, 2 * a.n_runs + 1024
    text2 = torch.empty(words, dtype=torch.int32, device=dev)
    seq_offset, name_index = (torch.empty(max_seqs + 1, dtype=torch.int32, device=dev) for _ in range(2))
    names = torch.empty(64 * max_seqs, dtype=torch.uint8, device=dev)
    hole_offset, hole_rank = (torch.empty(max_holes, dtype=torch.int32, device=dev) for _ in range(2))
    hole_amb = torch.empty(max_holes, dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def scan():
        amd._check(lib.nvbio_fasta_scan(0, amd._ptr(text), nb, stp, sp, amd._ptr(temp), temp.numel(), stream))

    def encode():                                                              # from the scan's copy of the state: every call does the same work
        amd._check(lib.nvbio_fasta_encode(0, amd._ptr(text), nb, amd._ptr(temp), temp.numel(), stp, amd._ptr(text2), words, amd._ptr(seq_offset),
                                          amd._ptr(name_index), max_seqs, amd._ptr(names), names.numel(), amd._ptr(hole_offset), amd._ptr(hole_rank),
                                          amd._ptr(hole_amb), max_holes, amd._ptr(status), stream))

    def both():
        scan()
        encode()

    def median_of(f, fresh=False):
        ts = []
        for step in range(a.warmup + a.steps):
            if fresh:
                state.copy_(state0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            if step >= a.warmup:
                ts.append(e0.elapsed_time(e1))
        return float(np.median(ts)), ts

    t_scan, ts_scan = median_of(scan, fresh=True)
    t_encode, ts_encode = median_of(encode)
    t_total, ts_total = median_of(both, fresh=True)
    copy_dst = torch.empty_like(text)
    t_d2d, ts_d2d = median_of(lambda: copy_dst.copy_(text))
    host = torch.empty(nb, dtype=torch.uint8).pin_memory()
    host.copy_(text)
    t_h2d, ts_h2d = median_of(lambda: copy_dst.copy_(host, non_blocking=True))
    torch.cuda.synchronize()
    s, st = amd.fasta_summary(summary), amd.fasta_state(state)
    lines = nb // LINE
    assert s["status"] == 0 and s["consumed_bytes"] == nb and s["n_seqs"] == a.seqs and int(status.item()) == 0, s
    assert st["n_symbols"] == s["n_symbols"] == (lines - a.seqs) * (LINE - 1) and sum(st["freq"]) == st["n_symbols"] and 0 < st["n_holes"] <= max_holes, st
    out = dict(workload="fasta_parse", text_bytes=nb, seqs=a.seqs, symbols=st["n_symbols"], ambiguous=st["n_ambs"], holes=st["n_holes"], temp_bytes=int(temp_bytes),
               steps=a.steps, warmup=a.warmup, scan_ms=t_scan, encode_ms=t_encode, total_ms=t_total, d2d_copy_ms=t_d2d, h2d_copy_ms=t_h2d,
               parse_gb_per_s=nb / (t_total * 1e-3) / 1e9, d2d_gb_per_s=nb / (t_d2d * 1e-3) / 1e9, h2d_gb_per_s=nb / (t_h2d * 1e-3) / 1e9,
               parse_over_d2d=t_total / t_d2d, parse_over_h2d=t_total / t_h2d, scan_ms_steps=ts_scan, encode_ms_steps=ts_encode, total_ms_steps=ts_total,
               d2d_ms_steps=ts_d2d, h2d_ms_steps=ts_h2d, summary=s)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
