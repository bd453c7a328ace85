"""CPU-only: the plain-Python restatement of the SAM record format (tests/sam_cpu.py) against tests/golden/sam_known.txt -- 24 records
worked out by hand from the rules (tests/golden/make_sam_known.py holds their input arrays and spells the lines out), and the header of
two sequences.  The GPU tests compare the library with the restatement; this file is what ties the restatement to the format."""
import os

import numpy as np

import sam_cpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def known():
    """(refs, single-end records, paired records, the expected bytes) of the golden files"""
    with np.load(os.path.join(GOLDEN, "sam_known.npz"), allow_pickle=False) as z:
        z = {k: z[k] for k in z.files}
    split = lambda data, index: [bytes(data[index[i]:index[i + 1]]) for i in range(len(index) - 1)]
    refs = dict(sequence_index=z["sequence_index"], names=split(z["ref_names"], z["ref_names_index"]))

    def records(prefix):
        r = {k[len(prefix):]: v for k, v in z.items() if k.startswith(prefix)}
        r["names"] = split(r.pop("names"), r.pop("name_index"))
        r["reads_reversed"] = True
        return r

    return refs, records("se_"), records("pe_"), open(os.path.join(GOLDEN, "sam_known.txt"), "rb").read()


def test_restatement_equals_the_hand_written_records():
    refs, se, pe, want = known()
    header = sam_cpu.sam_header(refs["names"], np.diff(refs["sequence_index"].astype(np.int64)))
    assert header == b"@HD\tVN:1.3\n@PG\tID:nvBowtie\tPN:nvBowtie\tVN:0.5.1\n@SQ\tSN:chr1\tLN:1000\n@SQ\tSN:chrB\tLN:500\n"
    assert want.startswith(header)
    lines = want[len(header):].split(b"\n")
    assert lines[-1] == b"" and len(lines) == 22
    got = [sam_cpu.sam_record(refs, se, i) for i in range(14)] + [sam_cpu.sam_record(refs, pe, i) for i in range(10)]
    names = se["names"] + pe["names"]
    skipped = [names[i] for i, g in enumerate(got) if g is None]
    assert skipped == [b"trunc", b"trunc2", b"badsum"]
    for g, w in zip([g for g in got if g is not None], lines[:-1]):
        assert g == w + b"\n", (g, w)
    st, so, sk = sam_cpu.sam_records(refs, se)
    pt, po, pk = sam_cpu.sam_records(refs, pe)
    assert header + st + pt == want and (sk, pk) == (3, 0)
    assert so[0] == 0 and so[-1] == len(st) and so[8] == so[9] == so[10] == so[11] and po[-1] == len(pt)


def test_the_known_records_cover_the_cases():
    """what the golden file is there for, read off its own lines"""
    _, _, _, want = known()
    text = want.decode("latin-1")
    by_name = {l.split("\t")[0]: l.split("\t") for l in text.splitlines() if not l.startswith("@")}
    assert by_name["r0"][1] == "4" and by_name["r0"][2:9] == ["*", "0", "0", "*", "*", "0", "0"] and "N" in by_name["r0"][9]
    assert by_name["rcN"][1] == "80" and "N" in by_name["rcN"][9] and "AS:i:-1" in by_name["rcN"] and "XS:i:-7" in by_name["rcN"]
    assert by_name["del"][5] == "147M2D3M" and by_name["del"][-1] == "MD:Z:147^AT03"
    assert by_name["clip"][5] == "2S6M2S" and "XO:i:2" in by_name["clip"]
    assert by_name["run300"][-1] == "MD:Z:300" and not any(f.startswith("XS:") for f in by_name["run300"])
    assert by_name["straddle"][1] == "68" and len(by_name["straddle"]) == 11
    assert by_name["pA/2"][8] == "-208" and by_name["pB/1"][6] == "chrB" and by_name["pC/1"][6:9] == ["=", "701", "0"]
    assert "trunc" not in by_name and "badsum" not in by_name


def test_md_walk_details():
    """the MDS rules one by one: merged runs without the reference's uint8 wrap, a stream of two bytes, a deletion of 255, tokens cut by the stride"""
    mk = lambda stream, stride=None: dict(mds=np.array([stream + [0] * ((stride or len(stream)) - len(stream))], np.uint8),
                                          mds_lens=np.array([len(stream)], np.uint32))
    s = lambda *tokens: [2 + sum(len(t) for t in tokens) & 255, 2 + sum(len(t) for t in tokens) >> 8] + [b for t in tokens for b in t]
    assert sam_cpu.md_and_counts(mk(s([0, 255], [0, 255], [0, 90])), 0) == ("600", 0, 0, 0)
    assert sam_cpu.md_and_counts(mk([2, 0]), 0) == ("", 0, 0, 0)
    assert sam_cpu.md_and_counts(mk(s([1, 0], [1, 3], [0, 1])), 0) == ("AT1", 2, 0, 0)
    assert sam_cpu.md_and_counts(mk(s([3, 255] + [1] * 255)), 0) == ("^" + "C" * 255 + "0", 0, 1, 254)
    assert sam_cpu.md_and_counts(mk(s([2, 3, 0, 0, 0], [0, 7])), 0) == ("7", 0, 1, 2)
    assert sam_cpu.md_and_counts(dict(mds=None), 0) == ("", 0, 0, 0)
    cut = mk(s([0, 5], [3, 4, 1, 1, 1, 1]))                           # 10 bytes, of which a stride of 8 keeps the deletion's first two symbols
    cut["mds"] = cut["mds"][:, :8]
    assert sam_cpu.md_and_counts(cut, 0) == ("5^CCAA0", 0, 1, 3)
