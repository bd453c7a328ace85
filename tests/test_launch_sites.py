"""CPU-only: every kernel of the library is launched through the one checked launch of csrc/common.h (launch_kernel, spelled
NVB_LAUNCH at the sites), so that no launch's status can go unread: no other source holds a raw launch, and common.h holds one."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nvbio-gpl_amd", "csrc")

_RAW = re.compile(r"hipLaunchKernelGGL|<<<")


def raw_launches():
    """file -> the number of raw launches (hipLaunchKernelGGL or a <<< >>> launch) outside // comments"""
    out = {}
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h")):
            src = open(os.path.join(CSRC, f)).read()
            src = re.sub(r"//[^\n]*", "", src)
            out[f] = len(_RAW.findall(src))
    return out


def test_only_common_h_launches_and_it_launches_once():
    n = raw_launches()
    assert "common.h" in n and len(n) > 10, "the library sources were not found"
    others = {f: c for f, c in n.items() if f != "common.h" and c}
    assert not others, "raw kernel launches outside common.h: %s" % others
    assert n["common.h"] == 1


def test_every_source_goes_through_the_checked_launch():
    """the helper is in use: the sources hold launches, all of them NVB_LAUNCH"""
    total = 0
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h")) and f != "common.h":
            src = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, f)).read())
            total += len(re.findall(r"\bNVB_LAUNCH\(", src))
    assert total >= 100
