"""Time the BAM formatter and the BGZF framing (nvbio_bam_record_offsets, nvbio_bam_format, nvbio_bgzf_frame) on one GPU, over the
records of scripts/bench_sam_format.py (--records single-end records of --len bp, 95 % mapped, at most 3 edits, names of 20 bytes,
qualities, 25 reference sequences), with the SAM formatter's three steps on the same records in the same run as the yardstick.
Device events around each call, medians of --steps runs after --warmup:
  lengths   nvbio_bam_record_offsets with NVBIO_BAM_LENGTHS_ONLY
  scan      nvbio_bam_record_offsets whole, minus the lengths (the tiled scan of n + 1 uint64)
  write     nvbio_bam_format
  frame     nvbio_bgzf_frame over the records: a copy plus a CRC-32
  copy      a device-to-device copy of as many bytes as the records have: the yardstick of write and frame
  sam_*     nvbio_sam_record_offsets (lengths, scan) and nvbio_sam_format, and a copy of the text's bytes
The framed bytes are inflated on the host once (Python's gzip, which verifies every CRC) and compared with the records.
Prints one JSON line and writes it to --out."""
import argparse
import ctypes
import gzip
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import __graft_entry__ as ge  # noqa: E402
from bench_sam_format import make_records  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bam_format_bench.json"))
    a = ap.parse_args()
    import torch
    amd = ge.load_package()
    dev = "cuda:0"
    n = a.records
    refs, records = make_records(amd, torch, n, a.len, dev)
    lib, stream = amd.lib(), amd._stream_ptr(dev)
    rs, cs = refs.c_struct(), records.c_struct()
    words = torch.zeros(2, dtype=torch.int32, device=dev)
    skipped_p, status_p = ctypes.c_void_p(words.data_ptr()), ctypes.c_void_p(words.data_ptr() + 4)

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

    def three_steps(kind, offsets_call, format_call, temp_call, lengths_only):
        offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
        tmp, nb = amd._temp_for(temp_call, n, device=dev)
        record_offsets = lambda flags: amd._check(offsets_call(0, ctypes.byref(rs), ctypes.byref(cs), flags, amd._ptr(offsets), amd._ptr(tmp), nb, stream))
        t_len, ts_len = median_of(lambda: record_offsets(lengths_only))
        t_off, ts_off = median_of(lambda: record_offsets(0))
        total = int(offsets[-1].item())
        data = torch.empty(total, dtype=torch.uint8, device=dev)
        src = torch.empty(total, dtype=torch.uint8, device=dev)
        write = lambda: amd._check(format_call(0, ctypes.byref(rs), ctypes.byref(cs), 0, amd._ptr(offsets), amd._ptr(data), total, skipped_p, status_p, stream))
        t_write, ts_write = median_of(write)
        t_copy, ts_copy = median_of(lambda: src.copy_(data))
        write()
        torch.cuda.synchronize()
        n_skipped, status = (int(v) for v in words.cpu().numpy())
        out = {"bytes": total, "bytes_per_record": total / n, "n_skipped": n_skipped, "status": status, "lengths_ms": t_len, "offsets_ms": t_off,
               "scan_ms": max(t_off - t_len, 0.0), "write_ms": t_write, "copy_ms": t_copy, "write_over_copy": t_write / t_copy,
               "write_ns_per_record": t_write * 1e6 / n, "records_per_s": n / ((t_off + t_write) * 1e-3), "lengths_ms_steps": ts_len,
               "offsets_ms_steps": ts_off, "write_ms_steps": ts_write, "copy_ms_steps": ts_copy}
        return {kind + "_" + k: v for k, v in out.items()}, data

    out = dict(workload="bam_format", records=n, read_len=a.len, steps=a.steps, warmup=a.warmup)
    bam, data = three_steps("bam", lib.nvbio_bam_record_offsets, lib.nvbio_bam_format, lib.nvbio_bam_format_temp_bytes, amd.BAM_LENGTHS_ONLY)
    out.update(bam)
    total = data.numel()
    framed = torch.empty(amd.bgzf_framed_bytes(total), dtype=torch.uint8, device=dev)
    frame = lambda: amd._check(lib.nvbio_bgzf_frame(0, amd._ptr(data), total, amd._ptr(framed), framed.numel(), stream))
    t_frame, ts_frame = median_of(frame)
    ok = gzip.decompress(framed.cpu().numpy().tobytes() + amd.BGZF_EOF) == data.cpu().numpy().tobytes()
    out.update(framed_bytes=framed.numel(), frame_ms=t_frame, frame_ms_steps=ts_frame, frame_over_copy=t_frame / bam["bam_copy_ms"],
               frame_gb_per_s=total / (t_frame * 1e-3) / 1e9, copy_gb_per_s=total / (bam["bam_copy_ms"] * 1e-3) / 1e9, framed_inflates_to_the_records=ok)
    del framed
    sam, _ = three_steps("sam", lib.nvbio_sam_record_offsets, lib.nvbio_sam_format, lib.nvbio_sam_format_temp_bytes, amd.SAM_LENGTHS_ONLY)
    out.update(sam)
    out["bam_write_over_sam_write"] = bam["bam_write_ms"] / sam["sam_write_ms"]
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
