"""Packs tests/golden/fastq_known.fq, fastq_marker.fq and the hand-written answers of fastq_known.txt into fastq_known.npz.  It only
packs: it reads the files, un-escapes the answers and stores them as arrays.  Nothing here parses FASTQ, and nothing calls the
restatement (tests/fastq_cpu.py) or the library.

Per file F in (known, marker):  F_text uint8; F_names uint8 + F_name_index; F_symbols uint8 (codes 0..5) and F_quals uint8 (the raw
quality bytes) + F_read_index; F_summary = status, first_bad_record, consumed_bytes, error_offset, error_char (none = 0xFFFFFFFF)."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CODES = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4, "-": 5}
SUMMARY_KEYS = ("status", "first_bad_record", "consumed_bytes", "error_offset", "error_char")


def unescape(field):
    return field.encode("latin-1").decode("unicode_escape").encode("latin-1")


def load():
    files, cur = {}, None
    for line in open(os.path.join(HERE, "fastq_known.txt"), encoding="latin-1").read().split("\n"):
        if not line or line.startswith("#"):
            continue
        key, *rest = line.split("\t")
        if key == "file":
            cur = files.setdefault(rest[0], dict(records=[]))
        elif key == "record":
            name, symbols, quals = (rest + ["", "", ""])[:3]
            cur["records"].append((unescape(name), [CODES[c] for c in symbols], unescape(quals)))
        else:
            cur[key] = 0xFFFFFFFF if rest[0] == "none" else int(rest[0])
    return files


def pack():
    out = {}
    for fname, f in load().items():
        tag = fname.split(".")[0].split("_")[1]
        recs = f["records"]
        assert all(len(s) == len(q) for _, s, q in recs), fname
        out[tag + "_text"] = np.frombuffer(open(os.path.join(HERE, fname), "rb").read(), dtype=np.uint8)
        out[tag + "_names"] = np.frombuffer(b"".join(n for n, _, _ in recs), dtype=np.uint8)
        out[tag + "_name_index"] = np.cumsum([0] + [len(n) for n, _, _ in recs]).astype(np.uint32)
        out[tag + "_symbols"] = np.array([c for _, s, _ in recs for c in s], dtype=np.uint8)
        out[tag + "_quals"] = np.frombuffer(b"".join(q for _, _, q in recs), dtype=np.uint8)
        out[tag + "_read_index"] = np.cumsum([0] + [len(s) for _, s, _ in recs]).astype(np.uint32)
        out[tag + "_summary"] = np.array([f[k] for k in SUMMARY_KEYS], dtype=np.uint32)
    return out


if __name__ == "__main__":
    np.savez(os.path.join(HERE, "fastq_known.npz"), **pack())
