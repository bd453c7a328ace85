"""Time the SAM formatter (nvbio_sam_record_offsets, nvbio_sam_format) on one GPU: --records single-end records of --len bp, 95 % mapped,
CIGARs and MDS streams of alignments with at most 3 edits (most ungapped, one in ten with an insertion or a deletion), names of ~20
bytes, qualities, 25 reference sequences.  Device events around each call, medians of --steps runs after --warmup:
  lengths   nvbio_sam_record_offsets with NVBIO_SAM_LENGTHS_ONLY
  scan      nvbio_sam_record_offsets whole, minus the lengths (the rocPRIM scan of n + 1 uint64)
  write     nvbio_sam_format
  copy      a device-to-device copy of as many bytes as the text has: the yardstick
Prints one JSON line and writes it to --out."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def make_records(amd, torch, n, L, dev):
    g = torch.Generator(device=dev).manual_seed(7)
    rnd = lambda lo, hi, shape, dtype=torch.int32: torch.randint(lo, hi, shape, device=dev, generator=g).to(dtype)
    n_seqs, seq_len = 25, 100_000_000
    refs = amd.SamRefs(["chr%d" % (i + 1) for i in range(n_seqs)], np.arange(n_seqs + 1, dtype=np.int64) * seq_len, device=dev)
    name_len = 20
    names = (rnd(48, 123, (n * name_len,), torch.uint8), (torch.arange(n + 1, device=dev, dtype=torch.int32) * name_len), name_len)
    reads4 = rnd(-2 ** 31, 2 ** 31 - 1, ((n * L + 7) // 8 + 1,)) & 0x33333333          # symbols 0..3
    read_index = torch.arange(n + 1, device=dev, dtype=torch.int32) * L
    quals = rnd(2, 42, (n * L,), torch.uint8)
    aligned = torch.rand(n, device=dev, generator=g) < 0.95
    state = aligned.to(torch.uint8) | (rnd(0, 2, (n,), torch.uint8) << 1)
    pos = (rnd(0, n_seqs, (n,)).to(torch.int64) * seq_len + rnd(0, seq_len - 2 * L, (n,)).to(torch.int64)).to(torch.int32)
    # CIGAR: LM, or a M + 1..2 I/D + b M for one read in ten (backtracking order: last element first)
    stride, mstride = 8, 32
    gapped = torch.rand(n, device=dev, generator=g) < 0.1
    a = rnd(20, L - 20, (n,))
    gl = rnd(1, 3, (n,))
    is_del = rnd(0, 2, (n,)) == 1
    b = torch.where(is_del, L - a, L - a - gl)
    cig = torch.zeros((n, stride), dtype=torch.int32, device=dev)
    cig[:, 0] = torch.where(gapped, b << 2, torch.full_like(a, L << 2))
    cig[:, 1] = torch.where(gapped, (gl << 2) | torch.where(is_del, 2, 1), torch.zeros_like(a))
    cig[:, 2] = torch.where(gapped, a << 2, torch.zeros_like(a))
    cigar_lens = torch.where(gapped, 3, 1).to(torch.int32) * aligned.to(torch.int32)
    # MDS: [0 a] [1 sym] [0 rest] for up to two mismatches; gapped reads: [0 a] [3|2 l syms] [0 b]
    mds = torch.zeros((n, mstride), dtype=torch.uint8, device=dev)
    nm = rnd(0, 3, (n,))
    m1 = rnd(1, L // 2, (n,))
    m2 = rnd(1, L // 2 - 1, (n,))
    u8 = lambda t: t.to(torch.uint8)
    body0 = torch.stack([u8(torch.zeros_like(a)), u8(torch.full_like(a, L))], 1)                                           # L matches
    body1 = torch.stack([u8(a * 0), u8(m1), u8(a * 0 + 1), u8(rnd(0, 4, (n,))), u8(a * 0), u8(L - 1 - m1)], 1)
    body2 = torch.stack([u8(a * 0), u8(m1), u8(a * 0 + 1), u8(rnd(0, 4, (n,))), u8(a * 0), u8(m2), u8(a * 0 + 1), u8(rnd(0, 4, (n,))), u8(a * 0),
                         u8(L - 2 - m1 - m2)], 1)
    bodyg = torch.stack([u8(a * 0), u8(a), u8(torch.where(is_del, 3, 2)), u8(gl), u8(rnd(0, 4, (n,))), u8(rnd(0, 4, (n,))), u8(a * 0), u8(b)], 1)
    mds_lens = torch.zeros(n, dtype=torch.int32, device=dev)
    for sel, body in ((~gapped & (nm == 0), body0), (~gapped & (nm == 1), body1), (~gapped & (nm == 2), body2), (gapped & (gl == 2), bodyg)):
        k = body.shape[1]
        mds[sel, 2:2 + k] = body[sel]
        mds[sel, 0] = k + 2
        mds_lens[sel] = k + 2
    sel = gapped & (gl == 1)                                              # a gap of one symbol: the token is one byte shorter
    one = torch.cat([bodyg[:, :5], bodyg[:, 6:]], 1)
    mds[sel, 2:9] = one[sel]
    mds[sel, 0] = 9
    mds_lens[sel] = 9
    mds_lens = mds_lens * aligned.to(torch.int32)
    ed = torch.where(gapped, gl, nm).to(torch.int32)
    score = -(6 * nm + torch.where(gapped, 5 + 3 * gl, torch.zeros_like(gl))).to(torch.int32)
    second = torch.where(torch.rand(n, device=dev, generator=g) < 0.3, score - 12, torch.full_like(score, amd.SCORE_MIN))
    records = amd.SamRecords(names, reads4, read_index, L, state, pos, score, ed, rnd(0, 43, (n,), torch.uint8), cig.to(torch.int16), cigar_lens, quals=quals,
                             second_score=second, mds=mds, mds_lens=mds_lens, device=dev)
    return refs, records


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sam_format_bench.json"))
    a = ap.parse_args()
    import torch
    amd = ge.load_package()
    dev = "cuda:0"
    n = a.records
    refs, records = make_records(amd, torch, n, a.len, dev)
    lib, stream = amd.lib(), amd._stream_ptr(dev)
    rs, cs = refs.c_struct(), records.c_struct()
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    tmp, nb = amd._temp_for(lib.nvbio_sam_format_temp_bytes, n, device=dev)
    words = torch.zeros(2, dtype=torch.int32, device=dev)

    def record_offsets(flags):
        amd._check(lib.nvbio_sam_record_offsets(0, ctypes.byref(rs), ctypes.byref(cs), flags, amd._ptr(offsets), amd._ptr(tmp), nb, stream))

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

    t_len, ts_len = median_of(lambda: record_offsets(amd.SAM_LENGTHS_ONLY))
    t_off, ts_off = median_of(lambda: record_offsets(0))
    total = int(offsets[-1].item())
    text = torch.empty(total, dtype=torch.uint8, device=dev)
    copy_src = torch.empty(total, dtype=torch.uint8, device=dev)

    def write():
        amd._check(lib.nvbio_sam_format(0, ctypes.byref(rs), ctypes.byref(cs), 0, amd._ptr(offsets), amd._ptr(text), total, ctypes.c_void_p(words.data_ptr()),
                                        ctypes.c_void_p(words.data_ptr() + 4), stream))

    t_write, ts_write = median_of(write)
    t_copy, ts_copy = median_of(lambda: text.copy_(copy_src))
    write()
    torch.cuda.synchronize()
    n_skipped, status = (int(v) for v in words.cpu().numpy())
    first = bytes(text[:int(offsets[2].item())].cpu().numpy()).decode("latin-1")
    out = dict(workload="sam_format", records=n, read_len=a.len, text_bytes=total, bytes_per_record=total / n, n_skipped=n_skipped, status=status,
               steps=a.steps, warmup=a.warmup, lengths_ms=t_len, offsets_ms=t_off, scan_ms=max(t_off - t_len, 0.0), write_ms=t_write, copy_ms=t_copy,
               write_gb_per_s=total / (t_write * 1e-3) / 1e9, copy_gb_per_s=total / (t_copy * 1e-3) / 1e9, write_over_copy=t_write / t_copy,
               records_per_s=n / ((t_off + t_write) * 1e-3), lengths_ms_steps=ts_len, offsets_ms_steps=ts_off, write_ms_steps=ts_write, copy_ms_steps=ts_copy,
               first_records=first)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
