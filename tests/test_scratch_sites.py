"""CPU-only: every ScratchBlock site of the library carries one of the tags that tests/test_gpu_scratch_check.py expects to see
checked, so that a new site cannot go untested by the scratch check mode."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nvbio-gpl_amd", "csrc")

# one per ScratchBlock::alloc / alloc_layout call in nvbio-gpl_amd/csrc
SCRATCH_TAGS = (
    "fm_filter_scan", "fm_hamming_backtrack", "fm_seed_pass", "fm_seed_pass_both", "fm_residual_diagonals",
    "banded_length_sort", "banded_job_list",
    "full_job_lists", "full_columns", "full_best2_columns",
    "banded_tb_job_list", "banded_tb_dirs",
    "full_tb_job_list", "full_tb_dirs",
    "rank_dictionary_build", "sort_unique_keys", "read_queue_filter", "select_flagged_indices",
    "mem_filter_head", "mem_filter_arena",
    "qgram_generate", "qgram_filter_rank", "qgram_filter_merge",
)

_CALL = re.compile(r"(?:\.|->)alloc(?:_layout)?\(\s*(\"[a-z0-9_]*\")?")


def site_tags():
    """(tag or None, file) for every ScratchBlock alloc call of the library sources (core.hip defines them)"""
    out = []
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h")) and f not in ("core.hip", "common.h"):
            src = open(os.path.join(CSRC, f)).read()
            src = re.sub(r"//[^\n]*", "", src)
            for m in _CALL.finditer(src):
                out.append((m.group(1).strip('"') if m.group(1) else None, f))
    return out


def test_scratch_site_tags_equal_the_expected_set():
    sites = site_tags()
    untagged = [f for t, f in sites if t is None]
    assert not untagged, "ScratchBlock alloc without a tag in %s" % untagged
    tags = [t for t, _ in sites]
    assert len(tags) == len(set(tags)), "tags must be unique: %s" % sorted(tags)
    assert sorted(tags) == sorted(SCRATCH_TAGS)
    assert len(tags) == 23
