"""GPU: the two resident forms of a new keyframe held to the buffer extents include/spfe.h documents, as
tests/test_gpu_map_point_culling_extents.py holds the map-point cull's: each form is called (a) with separate torch tensors and (b),
(c) with EVERY pointer argument — the frame's holders, the rows, the keyframe flags, the four state arrays, the record, the track
descriptors, the index array, the table's ref_slot, the block — inside one arena (tests/extent_arena.py) at exactly its documented
size, the bytes between the buffers filled with 0xFF, then with 0x80.  No byte outside a buffer may change, and every output must be
byte-identical across the three calls and equal to tests/newkf_ref/newkf_ref.c.  Rows of 101 and 1001 entries start off a 16-byte
boundary in three slots of four, and the last row ends where the arena's poison begins: the scan's 16-byte loads have to stop inside
it.  The cases hold wild entries (beyond the table, negative, INT32_MIN / MAX) in the frame, the rows and the lists: none is
followed.  And every SPFE_EINVAL case leaves the state, the rows and the block untouched."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("newkf_ref", ""):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
import extent_arena as ea  # noqa: E402
import newkf_cases as nc  # noqa: E402
import newkf_gpu as ng  # noqa: E402
import newkf_ref as nr  # noqa: E402

from sp_orb_slam_amd import extractor as X  # noqa: E402
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
        return made[bf16]
    yield get
    for e in made.values():
        e.close()


def three_calls(ext, ref, c):
    import torch
    spec, sizes, outs = ng.buffers(ext, c), ng.extents(ext, c), ng.outputs(c)
    want, _ = ng.want_of(ref, c)
    plain = ng.run_resident(ext, c)
    for k in outs:
        assert plain[k].tobytes() == np.asarray(want[k]).tobytes(), k
    arena = ea.Arena("cuda")
    for name, v in spec.items():
        arena.place(name, v, init=0xA5)
        assert arena.size(name) == sizes[name], (name, arena.size(name), sizes[name])

    def run(ar):
        ng.call(ext, {k: ar.ptr(k) for k in spec}, c)
        torch.cuda.synchronize()
    found, _ = ea.report(arena, run, outs, plain)
    assert found == [], found


@pytest.mark.parametrize("name", ["insert_n_kp_0", "insert_n_kp_1", "insert_n_kp_65", "insert_n_kp_257", "insert_n_kp_1025", "insert_every_code",
                                  "insert_every_code_bf16", "insert_no_record", "insert_no_track_table", "insert_repeats_across_chunks",
                                  "insert_recent_cap_reached", "insert_recent_cap_one_short", "insert_all_refusals", "insert_1x1_table_1"])
def test_insert_keyframe_resident(exts, ref, name):
    c = CASES[name]
    three_calls(exts(c.get("rec_desc") is not None and c["rec_desc"].dtype == np.uint16), ref, c)


@pytest.mark.parametrize("name", ["list_m_0", "list_m_1", "list_m_65", "list_m_1025", "list_no_index_array", "list_no_index_array_past_the_table",
                                  "list_whole_row", "list_all_empty_wild_repeated", "list_capacity_exact", "list_capacity_one_short",
                                  "list_capacity_0", "list_observers_0_to_300", "list_observers_one_short", "list_rows_1x1", "list_rows_2x3",
                                  "list_rows_7x101", "list_rows_9x1001", "list_table_1"])
def test_list_observations_resident(exts, ref, name):
    three_calls(exts(False), ref, CASES[name])


def test_einval_leaves_everything_untouched(exts):
    import torch
    ext = exts(False)
    ci, cl = CASES["insert_every_code"], CASES["list_whole_row"]
    t = {}
    for key, case in (("i", ci), ("l", cl)):
        for k, v in ng.buffers(ext, case).items():
            t[key + k] = (torch.full((int(v),), 0xA5, dtype=torch.uint8, device="cuda") if isinstance(v, (int, np.integer)) else
                          torch.from_numpy(ng.raw(v).copy()).cuda())
    before = {k: v.clone() for k, v in t.items()}

    def ptrs(key):
        return {k[1:]: v.data_ptr() for k, v in t.items() if k[0] == key}

    def refused(fn, what):
        with pytest.raises(X.SpfeError) as info:
            fn()
        assert str(info.value).startswith("SPFE_EINVAL"), (what, info.value)

    # the insertion
    P = ptrs("i")
    n, stride = ci["rows"].shape
    ok = dict(P, n_table=len(ci["flags"]), recent_cap=len(ci["recent"]), stride=stride, n=n, n_kp=len(ci["frame"]), cur=1)
    bad = [dict(n_table=0), dict(n_table=262145), dict(recent_cap=0), dict(recent_cap=262145), dict(stride=0), dict(stride=16385), dict(n=0),
           dict(n=65537), dict(n_kp=-1), dict(n_kp=stride + 1), dict(cur=-1), dict(cur=n), dict(frame=None), dict(rows=None), dict(kf_flags=None),
           dict(d_out=None), dict(frame=P["frame"] + 2), dict(rows=P["rows"] + 1), dict(record=P["record"] + 8), dict(desc_track=P["desc_track"] + 4),
           dict(d_out=P["d_out"] + 8), dict(stride=ext.layout.kmax + 1, n_kp=ext.layout.kmax + 1, n=1, cur=0)]
    bad += [{k: None} for k in nr.STATE] + [{k: P[k] + 2} for k in nr.STATE if k != "flags"]
    for change in bad:
        q = dict(ok, **change)
        life = X.mp_life({k: q[k] for k in nr.STATE}, q["n_table"], q["recent_cap"])
        refused(lambda: ext.insert_keyframe_resident(life, q["frame"], q["n_kp"], q["cur"], q["rows"], q["stride"], q["kf_flags"], q["n"], q["d_out"],
                                                     d_kf_record=q["record"], d_desc_track=q["desc_track"]), change)
    # the listing
    P = ptrs("l")
    n, stride = cl["rows"].shape
    ok = dict(P, first_row=0, m=int(cl["m"]), stride=stride, n=n, n_table=len(cl["ref_slot"]), cap=int(cl["obs_cap"]))
    bad = [dict(m=-1), dict(m=262145), dict(cap=-1), dict(cap=4194305), dict(n_table=0), dict(n_table=262145), dict(first_row=-1), dict(stride=0),
           dict(stride=16385), dict(n=0), dict(n=65537), dict(rows=None), dict(kf_flags=None), dict(ref_slot=None), dict(d_out=None),
           dict(point_idx=P["point_idx"] + 2), dict(rows=P["rows"] + 2), dict(ref_slot=P["ref_slot"] + 1), dict(d_out=P["d_out"] + 4)]
    for change in bad:
        q = dict(ok, **change)
        refused(lambda: ext.list_observations_resident(q["point_idx"], q["first_row"], q["m"], q["rows"], q["stride"], q["kf_flags"], q["n"],
                                                       q["ref_slot"], q["n_table"], q["cap"], q["d_out"]), change)
    torch.cuda.synchronize()
    for k in t:
        assert torch.equal(t[k], before[k]), k
