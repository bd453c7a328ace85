"""Packs tests/golden/fasta_known.fa, fasta_end.fa, fasta_cut.fa and the hand-written answers of fasta_known.txt into fasta_known.npz.
It only packs: it reads the files, un-escapes the answers and stores them as arrays.  Nothing here parses FASTA, and nothing calls the
restatement (tests/fasta_cpu.py) or the library.

draws uint8.  Per file F in (known, end, cut):  F_text uint8; F_names uint8 + F_name_index; F_symbols uint8 (codes 0..3; the k-th '.' of
the file is draws[k]) and F_ambiguous (bool: which were '.'); F_seq_offset (n + 1, from the lengths) and F_seq_n_ambs; F_hole_offset,
F_hole_len, F_hole_amb; F_summary = status, consumed_bytes, machine."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CODES = {"A": 0, "C": 1, "G": 2, "T": 3}
SUMMARY_KEYS = ("status", "consumed", "machine")


def unescape(field):
    return field.encode("latin-1").decode("unicode_escape").encode("latin-1")


def load():
    files, cur, draws = {}, None, None
    for line in open(os.path.join(HERE, "fasta_known.txt"), encoding="latin-1").read().split("\n"):
        if not line or line.startswith("#"):
            continue
        key, *rest = line.split("\t")
        if key == "draws":
            draws = [int(v) for v in rest[0].split()]
        elif key == "file":
            cur = files.setdefault(rest[0], dict(seqs=[], holes=[]))
        elif key == "seq":
            name, offset, length, n_ambs, symbols = (rest + [""])[:5]
            cur["seqs"].append((unescape(name), int(offset), int(length), int(n_ambs), symbols))
        elif key == "hole":
            cur["holes"].append((int(rest[0]), int(rest[1]), unescape(rest[2])[0]))
        else:
            cur[key] = int(rest[0])
    return files, draws


def pack():
    files, draws = load()
    out = {"draws": np.array(draws, dtype=np.uint8)}
    for fname, f in files.items():
        tag = fname.split(".")[0].split("_")[1]
        seqs, holes = f["seqs"], f["holes"]
        assert all(len(s[4]) == s[2] for s in seqs), fname
        assert [s[1] for s in seqs] == list(np.cumsum([0] + [s[2] for s in seqs])[:-1]), fname
        chars = "".join(s[4] for s in seqs)
        k, symbols = 0, []
        for c in chars:
            symbols.append(draws[k] if c == "." else CODES[c])
            k += c == "."
        out[tag + "_text"] = np.frombuffer(open(os.path.join(HERE, fname), "rb").read(), dtype=np.uint8)
        out[tag + "_names"] = np.frombuffer(b"".join(s[0] for s in seqs), dtype=np.uint8)
        out[tag + "_name_index"] = np.cumsum([0] + [len(s[0]) for s in seqs]).astype(np.uint32)
        out[tag + "_symbols"] = np.array(symbols, dtype=np.uint8)
        out[tag + "_ambiguous"] = np.array([c == "." for c in chars], dtype=bool)
        out[tag + "_seq_offset"] = np.cumsum([0] + [s[2] for s in seqs]).astype(np.uint32)
        out[tag + "_seq_n_ambs"] = np.array([s[3] for s in seqs], dtype=np.uint32)
        out[tag + "_hole_offset"] = np.array([h[0] for h in holes], dtype=np.uint32)
        out[tag + "_hole_len"] = np.array([h[1] for h in holes], dtype=np.uint32)
        out[tag + "_hole_amb"] = np.array([h[2] for h in holes], dtype=np.uint8)
        out[tag + "_summary"] = np.array([f[k] for k in SUMMARY_KEYS], dtype=np.uint32)
    return out


if __name__ == "__main__":
    np.savez(os.path.join(HERE, "fasta_known.npz"), **pack())
