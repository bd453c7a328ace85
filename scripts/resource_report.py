#!/usr/bin/env python3
"""Compare two builds kernel by kernel: the compiler's resource report and the device code.

  resource_report.py PARENT_BUILD NEW_BUILD file [file ...]
  resource_report.py PARENT_BUILD NEW_BUILD --parent file [file ...] --new file [file ...]

*_BUILD is the object directory of a build with the Makefile's flags plus -save-temps=obj (the saved gfx950 assembly carries the figures
that -Rpass-analysis=kernel-resource-usage prints), `file` a source name without suffix (gotoh_banded ...).  The first form reads the same
files from both builds; the second is for a change that moves kernels between files: the parent's kernels are the union over --parent, this
build's the union over --new, and a kernel is paired with itself by its mangled name wherever it lives.  Prints one row per kernel, parent ->
new, with the file that holds it now, and says how many kernels' disassembly (llvm-objdump -d of the gfx950 code object, addresses and
encodings stripped) is identical.  A kernel "only in the parent" or "only in this build" means the set of kernels changed."""
import argparse
import re
import subprocess

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
    for code in fns.values():                                # the padding behind a kernel's end depends on what follows it in its file
        while code and code[-1] in ("s_nop 0", "...", "s_code_end"):
            code.pop()
    return fns


def union(build, srcs):
    """the kernels of `srcs` together: {kernel: figures}, {kernel: disassembly}, {kernel: the files that hold it}"""
    figures, code, where = {}, {}, {}
    for src in srcs:
        r, d = report(build, src), disasm(build, src)
        for k in r:
            where.setdefault(k, []).append(src)
            figures[k], code[k] = r[k], d.get(k)
    return figures, code, where


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent_build")
    ap.add_argument("new_build")
    ap.add_argument("files", nargs="*", help="source names read from both builds")
    ap.add_argument("--parent", nargs="+", default=[], help="source names of the parent build")
    ap.add_argument("--new", nargs="+", default=[], help="source names of this build")
    a = ap.parse_args()
    psrcs, nsrcs = a.files + a.parent, a.files + a.new
    if not psrcs or not nsrcs:
        ap.error("no source files for one of the builds")
    p, pd, pw = union(a.parent_build, psrcs)
    n, nd, nw = union(a.new_build, nsrcs)
    same = total = 0
    worse = []
    short = demangle(sorted(set(p) | set(n)))
    print("# scripts/resource_report.py PARENT_BUILD NEW_BUILD%s%s%s   (both builds: the Makefile's flags plus -save-temps=obj)"
          % ("".join(" " + s for s in a.files), " --parent " + " ".join(a.parent) if a.parent else "", " --new " + " ".join(a.new) if a.new else ""))
    print("# parent: %s  ->  this build: %s" % (" ".join(s + ".hip" for s in psrcs), " ".join(s + ".hip" for s in nsrcs)))
    print("%-74s %-18s %s  code" % ("kernel", "in", "  ".join("%-11s" % h for _, h in FIELDS)))
    for k in sorted(set(p) | set(n), key=lambda k: short[k]):
        if "rocprim::" in short[k]:
            continue                                         # the library's kernels (DeviceSelect, DeviceRadixSort)
        if k not in p or k not in n:
            print("%-74s %-18s %s" % (short[k][:74], ",".join((pw if k in p else nw)[k]), "only in the parent" if k in p else "only in this build"))
            worse.append(short[k])
            continue
        if len(nw[k]) > 1:
            worse.append(short[k] + " (in %d files)" % len(nw[k]))
        cells = ["%-11s" % ("%s -> %s" % (p[k].get(f, "?"), n[k].get(f, "?")) if p[k].get(f) != n[k].get(f) else p[k].get(f, "?")) for f, _ in FIELDS]
        ident = pd.get(k) == nd.get(k) and pd.get(k) is not None
        total += 1
        same += ident
        print("%-74s %-18s %s  %s" % (short[k][:74], ",".join(nw[k]), "  ".join(cells), "identical" if ident else "differs"))
        if (int(n[k]["ScratchSize [bytes/lane]"]) > int(p[k]["ScratchSize [bytes/lane]"]) or int(n[k]["VGPRs Spill"]) > int(p[k]["VGPRs Spill"])
                or int(n[k]["Occupancy [waves/SIMD]"]) < int(p[k]["Occupancy [waves/SIMD]"])):
            worse.append(short[k])
    rocprim = (sum("rocprim::" in short[k] for k in p), sum("rocprim::" in short[k] for k in n))
    print("# kernels: %d, device code identical to the parent's: %d, differing: %d  (rocprim's kernels, not listed: %d -> %d)"
          % (total, same, total - same, rocprim[0], rocprim[1]))
    print("# kernels only in one build, in two files, or that gain scratch or a VGPR spill or lose a wave of occupancy: %s" % (", ".join(worse) if worse else "none"))


if __name__ == "__main__":
    main()
