"""GPU: a new keyframe on resident state — spfe_insert_keyframe_resident, spfe_list_observations_resident and the two host-array
forms — against tests/newkf_ref/newkf_ref.c byte for byte: the blocks, the row, the state, the track descriptors.  The cases are the
named cases of tests/newkf_ref/newkf_cases.py (frames of 0 - 1025 keypoints on both sides of a wavefront, a workgroup and the one
workgroup's chunk; every code in one frame, a point three times, repeats across a chunk; every refusal with the state untouched;
descriptors from f32 and bf16 records and with either array missing; lists of 0 - 1025 entries with empty, wild and repeated entries,
without an index array, whole rows; points seen by 0 - 300 keyframes and twice in one row, bad observers; the capacity exact and one
short; 1 - 4100 slots, row pitches 1 - 1001 with the rows 0 - 12 bytes off a 16-byte boundary; tables of 1 and 50,000 rows)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "newkf_ref"))
import newkf_cases as nc  # noqa: E402
import newkf_gpu as ng  # noqa: E402
import newkf_ref as nr  # noqa: E402

from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import SPExtractor  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = nc.named_cases()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return nr.build(tmp_path_factory.mktemp("newkf_ref"))


@pytest.fixture(scope="module")
def exts():
    made = {}

    def get(bf16):
        if bf16 not in made:
            made[bf16] = SPExtractor(nc.KMAX - 1, 64, 96, weights.synthetic(7, "trackable"), with_heat=False, desc_bf16=bf16)
            assert made[bf16].layout.kmax == nc.KMAX
        return made[bf16]
    yield get
    for e in made.values():
        e.close()


def handle_for(exts, c):
    return exts(c.get("rec_desc") is not None and c["rec_desc"].dtype == np.uint16)


@pytest.mark.parametrize("name", sorted(CASES))
def test_named_case_equals_the_reference_in_both_forms(exts, ref, name):
    c = CASES[name]
    ext = handle_for(exts, c)
    ng.check(ext, ref, c, what=name)
    if c["op"] == "list" or name in ("insert_every_code", "insert_n_kp_65"):     # the rows 4, 8 and 12 bytes off a 16-byte boundary
        want, _ = ng.want_of(ref, c)
        for shift in (4, 8, 12):
            ng.same(ng.run_resident(ext, c, shift), want, c, "%s, rows %d bytes off" % (name, shift))


def test_a_smaller_call_behind_a_larger_one_uses_the_grown_scratch(exts, ref):
    """the handle's scratch is carved by the call's own sizes: a small call behind the largest, and the largest again"""
    ext = exts(False)
    for name in ("list_table_50000", "list_m_1", "insert_table_50000_slots_300", "insert_1x1_table_1", "list_observers_0_to_300", "list_table_50000"):
        c = CASES[name]
        want, _ = ng.want_of(ref, c)
        ng.same(ng.run_resident(ext, c), want, c, name)


def test_added_point_is_a_list_as_it_lies(exts, ref):
    """the insertion's block on the device, then the listing on added_point INSIDE it, on one stream without a synchronisation in
    between: the ranges are those of the reference chained the same way"""
    import torch
    from sp_orb_slam_amd import extractor as X
    ext = exts(False)
    c = CASES["insert_n_kp_257"]
    n, stride = c["rows"].shape
    n_kp, nt = len(c["frame"]), len(c["flags"])
    w = nr.copy_world(c)
    r = nr.insert(ref, w, c["frame"], int(c["cur_slot"]), c["rec_desc"])
    cap = 4 * stride
    want = nr.list_obs(ref, w, r["added_point"], 0, stride, cap)
    t = {k: torch.from_numpy(ng.raw(c[k]).copy()).cuda() for k in ("rows", "kf_flags", "ref_slot") + nr.STATE}
    t["frame"] = torch.from_numpy(ng.raw(c["frame"]).copy()).cuda()
    o = X.newkf_offsets(n_kp, stride)
    d_ins = torch.full((o["out_bytes"],), ng.FILL, dtype=torch.uint8, device="cuda")
    d_list = torch.full((X.listobs_offsets(stride, cap)["out_bytes"],), ng.FILL, dtype=torch.uint8, device="cuda")
    life = X.mp_life(dict(flags=t["flags"].data_ptr(), nobs=t["nobs"].data_ptr(), recent=t["recent"].data_ptr(), recent_n=t["recent_n"].data_ptr()),
                     nt, len(c["recent"]))
    ext.insert_keyframe_resident(life, t["frame"].data_ptr(), n_kp, int(c["cur_slot"]), t["rows"].data_ptr(), stride, t["kf_flags"].data_ptr(), n,
                                 d_ins.data_ptr())
    ext.list_observations_resident(d_ins.data_ptr() + o["added_point"], 0, stride, t["rows"].data_ptr(), stride, t["kf_flags"].data_ptr(), n,
                                   t["ref_slot"].data_ptr(), nt, cap, d_list.data_ptr())
    torch.cuda.synchronize()
    assert d_ins.cpu().numpy().tobytes() == r["block"].tobytes()
    assert d_list.cpu().numpy().tobytes() == want["block"].tobytes()
    assert want["n_first"] == r["n_added"] and want["n_obs"] >= r["n_added"] + r["n_repeated"]
