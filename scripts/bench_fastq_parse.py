"""Time the FASTQ parser (nvbio_fastq_scan, nvbio_fastq_encode) on one GPU: --records four-line records of --len bp with --name-len byte
names, the text already in HBM, max_records = --records (so the scan's temp is sized by the records, not by text_bytes / 5).  Device
events around each call, medians of --steps runs after --warmup:
  scan      nvbio_fastq_scan: the state scan, the records' offsets and lengths, the index scan, the summary
  encode    nvbio_fastq_encode: names, qualities, 4-bit words, both indices (REVERSE_OP, Phred33: how nvBowtie loads)
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


def make_text(torch, n, L, name_len, dev):
    """n records `@r<digits>\\n<L symbols>\\n+\\n<L qualities>\\n` as one uint8 device tensor"""
    g = torch.Generator(device=dev).manual_seed(11)
    line = name_len + 2 + L + 1 + 2 + L + 1
    t = torch.empty((n, line), dtype=torch.uint8, device=dev)
    t[:, 0] = ord("@")
    t[:, 1] = ord("r")
    idx = torch.arange(n, device=dev, dtype=torch.int64)
    for k in range(name_len - 1):
        t[:, 2 + k] = (48 + (idx // 10 ** (name_len - 2 - k)) % 10).to(torch.uint8)
    t[:, name_len + 1] = 10
    s0 = name_len + 2
    t[:, s0:s0 + L] = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)[torch.randint(0, 4, (n, L), device=dev, generator=g)]
    t[:, s0 + L] = 10
    t[:, s0 + L + 1] = ord("+")
    t[:, s0 + L + 2] = 10
    q0 = s0 + L + 3
    t[:, q0:q0 + L] = torch.randint(35, 74, (n, L), device=dev, generator=g).to(torch.uint8)
    t[:, q0 + L] = 10
    return t.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--name-len", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fastq_parse_bench.json"))
    a = ap.parse_args()
    import torch
    amd = ge.load_package()
    dev = "cuda:0"
    n = a.records
    text = make_text(torch, n, a.len, a.name_len, dev)
    nb = text.numel()
    lib, stream = amd.lib(), amd._stream_ptr(dev)
    params = amd._FastqParams(amd.FASTQ_PHRED33, amd.FASTQ_REVERSE_OP, amd.FASTQ_UNLIMITED, n)
    temp, temp_bytes = amd._temp_for(lib.nvbio_fastq_temp_bytes, nb, n, device=dev)
    summary = torch.zeros(10, dtype=torch.int32, device=dev)
    sp = ctypes.cast(summary.data_ptr(), ctypes.POINTER(amd._FastqSummary))
    words = (n * a.len + 7) // 8
    reads4 = torch.empty(words, dtype=torch.int32, device=dev)
    quals = torch.empty(8 * words, dtype=torch.uint8, device=dev)
    names = torch.empty(n * a.name_len, dtype=torch.uint8, device=dev)
    read_index = torch.empty(n + 1, dtype=torch.int32, device=dev)
    name_index = torch.empty(n + 1, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def scan():
        amd._check(lib.nvbio_fastq_scan(0, amd._ptr(text), nb, ctypes.byref(params), sp, amd._ptr(temp), temp.numel(), stream))

    def encode():
        amd._check(lib.nvbio_fastq_encode(0, amd._ptr(text), nb, ctypes.byref(params), amd._ptr(temp), temp.numel(), amd._ptr(reads4), words, amd._ptr(read_index),
                                          amd._ptr(quals), amd._ptr(names), names.numel(), amd._ptr(name_index), amd._ptr(status), stream))

    def both():
        scan()
        encode()

    def median_of(f):
        ts = []
        for step in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            if step >= a.warmup:
                ts.append(e0.elapsed_time(e1))
        return float(np.median(ts)), ts

    t_scan, ts_scan = median_of(scan)
    t_encode, ts_encode = median_of(encode)
    t_total, ts_total = median_of(both)
    copy_dst = torch.empty_like(text)
    t_d2d, ts_d2d = median_of(lambda: copy_dst.copy_(text))
    host = torch.empty(nb, dtype=torch.uint8).pin_memory()
    host.copy_(text)
    t_h2d, ts_h2d = median_of(lambda: copy_dst.copy_(host, non_blocking=True))
    torch.cuda.synchronize()
    s = amd.fastq_summary(summary)
    assert s["n_records"] == n and s["status"] == 0 and s["consumed_bytes"] == nb and int(status.item()) == 0, s
    assert int(read_index[-1].item()) == n * a.len and int(name_index[-1].item()) == n * a.name_len
    out = dict(workload="fastq_parse", records=n, read_len=a.len, name_len=a.name_len, text_bytes=nb, temp_bytes=int(temp_bytes), steps=a.steps, warmup=a.warmup,
               scan_ms=t_scan, encode_ms=t_encode, total_ms=t_total, d2d_copy_ms=t_d2d, h2d_copy_ms=t_h2d,
               parse_gb_per_s=nb / (t_total * 1e-3) / 1e9, records_per_s=n / (t_total * 1e-3), d2d_gb_per_s=nb / (t_d2d * 1e-3) / 1e9,
               h2d_gb_per_s=nb / (t_h2d * 1e-3) / 1e9, parse_over_d2d=t_total / t_d2d, parse_over_h2d=t_total / t_h2d,
               scan_ms_steps=ts_scan, encode_ms_steps=ts_encode, total_ms_steps=ts_total, d2d_ms_steps=ts_d2d, h2d_ms_steps=ts_h2d, summary=s)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
