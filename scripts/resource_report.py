#!/usr/bin/env python3
"""Compare two builds kernel by kernel: the compiler's resource report and the device code.

  resource_report.py PARENT_BUILD NEW_BUILD file [file ...]

*_BUILD is the object directory of a build with the Makefile's flags plus -save-temps=obj (the saved gfx950 assembly carries the figures
that -Rpass-analysis=kernel-resource-usage prints), `file` a source name without suffix (gotoh_banded ...).  Prints one row per kernel, parent -> new, and says
how many kernels' disassembly (llvm-objdump -d of the gfx950 code object, addresses and encodings stripped) is identical."""
import re
import subprocess
import sys

FIELDS = [("VGPRs", "VGPRs"), ("ScratchSize [bytes/lane]", "scratch B"), ("Occupancy [waves/SIMD]", "occupancy"),
          ("SGPRs Spill", "SGPR spills"), ("VGPRs Spill", "VGPR spills"), ("TotalSGPRs", "SGPRs")]


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    short = {}
    for m, d in zip(names, out):
        d = re.sub(r"^void ", "", d)
        d = re.sub(r"nvbio_amd::|\(anonymous namespace\)::", "", d)
        short[m] = re.sub(r"\(.*$", "", d)
    return short


def report(build, src):
    """{kernel: {field: value}} from the kernel-info comments and the metadata of the saved gfx950 assembly"""
    res, cur, meta = {}, None, {}
    names = {"TotalNumSgprs": "TotalSGPRs", "NumVgprs": "VGPRs", "ScratchSize": "ScratchSize [bytes/lane]", "Occupancy": "Occupancy [waves/SIMD]"}
    for line in open("%s/%s-hip-amdgcn-amd-amdhsa-gfx950.s" % (build, src)):
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
        m = re.match(r"; (\w+): (\d+)", line)
        if m and cur is not None and m.group(1) in names:
            cur[names[m.group(1)]] = m.group(2)
        m = re.match(r"\s+\.(sgpr|vgpr)_spill_count:\s+(\d+)", line)
        if m:
            meta["SGPRs Spill" if m.group(1) == "sgpr" else "VGPRs Spill"] = m.group(2)
        m = re.match(r"\s+\.symbol:\s+(\S+)\.kd", line)
        if m:
            res[m.group(1)]["SGPRs Spill"] = meta.pop("SGPRs Spill")    # (.sgpr_spill_count comes before .symbol, .vgpr_spill_count after it)
            cur = res[m.group(1)]
            continue
        if "VGPRs Spill" in meta and cur is not None:
            cur["VGPRs Spill"] = meta.pop("VGPRs Spill")
    return res


def disasm(build, src):
    txt = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", "%s/%s-hip-amdgcn-amd-amdhsa-gfx950.out" % (build, src)],
                         capture_output=True, text=True, check=True).stdout
    fns, cur = {}, None
    for line in txt.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            cur = fns.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(re.sub(r"\s*//.*$", "", line).strip())
    return fns


def main():
    pbuild, nbuild = sys.argv[1:3]
    same = total = 0
    worse = []
    for src in sys.argv[3:]:
        p, n = report(pbuild, src), report(nbuild, src)
        pd, nd = disasm(pbuild, src), disasm(nbuild, src)
        short = demangle(sorted(set(p) | set(n)))
        print("# %s.hip" % src)
        print("%-74s %s  code" % ("kernel", "  ".join("%-11s" % h for _, h in FIELDS)))
        for k in sorted(set(p) | set(n), key=lambda k: short[k]):
            if "rocprim::" in short[k]:
                continue                                         # the library's kernels (DeviceSelect, DeviceRadixSort)
            if k not in p or k not in n:
                print("%-74s %s" % (short[k], "only in the parent" if k in p else "only in this build"))
                worse.append(short[k])
                continue
            cells = ["%-11s" % ("%s -> %s" % (p[k].get(f, "?"), n[k].get(f, "?")) if p[k].get(f) != n[k].get(f) else p[k].get(f, "?")) for f, _ in FIELDS]
            ident = pd.get(k) == nd.get(k) and pd.get(k) is not None
            total += 1
            same += ident
            print("%-74s %s  %s" % (short[k][:74], "  ".join(cells), "identical" if ident else "differs"))
            if (int(n[k]["ScratchSize [bytes/lane]"]) > int(p[k]["ScratchSize [bytes/lane]"]) or int(n[k]["VGPRs Spill"]) > int(p[k]["VGPRs Spill"])
                    or int(n[k]["Occupancy [waves/SIMD]"]) < int(p[k]["Occupancy [waves/SIMD]"])):
                worse.append(short[k])
    print("# kernels: %d, device code identical to the parent's: %d, differing: %d" % (total, same, total - same))
    print("# kernels that gain scratch or a VGPR spill or lose a wave of occupancy: %s" % (", ".join(worse) if worse else "none"))


if __name__ == "__main__":
    main()
