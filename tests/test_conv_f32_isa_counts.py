"""profiles/conv_f32_isa_counts.json (tools/isa_side_count.py; no GPU needed): what the compiler emits beside the MFMAs of
conv_f32_kernel, for this tree (`this`) and for the commit it was made against (`parent`).  The file is held to the
sources by its stamp, and the counts to the parent's: after a change to conv_f32.hip or the Makefile the tool is run again,
and the change has to leave the kernels no heavier than it found them."""
import hashlib
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sp_orb_slam_amd", "csrc")
# the instantiations the headline (752x480 x 8 frames, f32) launches: LAYER,CIN,KS,KC,WM,WN,MT,NT,POOL,RELU
HEADLINE = ["<1,64,3,16,4,1,4,2,1,1>", "<1,64,3,16,4,1,2,2,1,1>", "<0,64,3,16,4,1,2,2,0,1>", "<0,64,3,16,4,1,2,2,1,1>",
            "<0,128,3,16,4,1,2,2,1,1>", "<0,128,3,16,2,2,2,1,0,1>", "<0,128,3,16,2,2,1,1,0,1>"]


@pytest.fixture(scope="module")
def counts():
    return json.load(open(os.path.join(ROOT, "profiles", "conv_f32_isa_counts.json")))


def _pairs(counts):
    this, parent = counts["this"]["kernels"], counts["parent"]["kernels"]
    assert this and sorted(this) == sorted(parent)
    assert all(k in this for k in HEADLINE)
    return [(k, this[k], parent[k]) for k in sorted(this)]


def test_counts_are_stamped_with_the_sources_they_were_made_from(counts):
    for name, sha in counts["this"]["source_sha16"].items():
        got = hashlib.sha256(open(os.path.join(CSRC, name), "rb").read()).hexdigest()[:16]
        assert got == sha, "%s changed since tools/isa_side_count.py wrote profiles/conv_f32_isa_counts.json" % name
    assert sorted(counts["this"]["source_sha16"]) == ["Makefile", "conv_f32.hip"]


def test_no_packed_f32_beside_the_mfmas(counts):
    for k, t, _ in _pairs(counts):
        assert t["packed_f32"] == 0, k


def test_no_more_spills_than_the_parent(counts):
    for k, t, p in _pairs(counts):
        assert t["vgpr_spill_count"] <= p["vgpr_spill_count"], k
        assert t["private_segment_size"] <= p["private_segment_size"], k


def test_steady_bodies_are_no_larger_than_the_parents(counts):
    for k, t, p in _pairs(counts):
        assert t["steady_side"] <= p["steady_side"], k


def test_pooled_epilogue_is_at_most_55_percent_of_the_parents(counts):
    """epilogue extra = what a tile's first stage and its once-per-tile code hold beyond a later chunk's pass; 16 of the 29
    instructions per pooled store are 55 %"""
    pooled = [(k, t, p) for k, t, p in _pairs(counts) if k.split(",")[8] == "1"]
    assert pooled
    for k, t, p in pooled:
        extra, extra_parent = t["epilogue_side"] - t["steady_side"], p["epilogue_side"] - p["steady_side"]
        assert extra <= 0.55 * extra_parent, (k, extra, extra_parent)


def test_side_instructions_per_mfma_do_not_exceed_the_parents(counts):
    for k, t, p in _pairs(counts):
        if k in HEADLINE:
            assert t["side_per_mfma"] <= p["side_per_mfma"], k
