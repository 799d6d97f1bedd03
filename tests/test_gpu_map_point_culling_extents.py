"""GPU: the four resident forms of map-point culling held to the buffer extents include/spfe.h documents, as
tests/test_gpu_keyframe_culling_extents.py holds the keyframe cull's: each form is called (a) with separate torch tensors and (b),
(c) with EVERY pointer argument — the seven state arrays, the rows, the keyframe flags, the table's xyz, the creation's blocks, the
neighbour slots, both holder arrays, the list, the search's and the pose step's blocks up to the last byte the call reads, the block —
inside one arena (tests/extent_arena.py) at exactly its documented size, the bytes between the buffers filled with 0xFF, then with
0x80.  No byte outside a buffer may change, and every output must be byte-identical across the three calls and equal to
tests/mpcull_ref/mpcull_ref.c.  Rows of 101 and 1001 entries start off a 16-byte boundary in three slots of four, and the last row
ends where the arena's poison begins: the row scan's 16-byte loads have to stop inside it.  And every SPFE_EINVAL case leaves the
state, the rows and the block untouched."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("mpcull_ref", ""):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
import extent_arena as ea  # noqa: E402
import mpcull_cases as mc  # noqa: E402
import mpcull_gpu as mg  # noqa: E402
import mpcull_ref as mr  # noqa: E402

from sp_orb_slam_amd import extractor as X  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import SPExtractor  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = mc.named_cases()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return mr.build(tmp_path_factory.mktemp("mpcull_ref"))


@pytest.fixture(scope="module")
def ext():
    e = SPExtractor(mc.KMAX - 1, 64, 96, weights.synthetic(7, "trackable"), with_heat=False)
    yield e
    e.close()


def three_calls(ext, ref, c):
    import torch
    spec, sizes, outs = mg.buffers(c), mg.extents(c), mg.outputs(c)
    want, _ = mg.want_of(ref, c)
    plain = mg.run_resident(ext, c)
    for k in outs:
        assert plain[k].tobytes() == np.asarray(want[k]).tobytes(), k
    arena = ea.Arena("cuda")
    for name, v in spec.items():
        arena.place(name, v, init=0xA5)
        assert arena.size(name) == sizes[name], (name, arena.size(name), sizes[name])

    def run(ar):
        mg.call(ext, {k: ar.ptr(k) for k in spec}, c)
        torch.cuda.synchronize()
    found, _ = ea.report(arena, run, outs, plain)
    assert found == [], found


@pytest.mark.parametrize("name", ["cull_rows_1x1", "cull_rows_2x3", "cull_rows_7x101", "cull_rows_9x1001", "cull_list_1025", "cull_every_code",
                                  "cull_bad_cap_0", "cull_count_beyond_cap", "cull_list_0"])
def test_cull_map_points_resident(ext, ref, name):
    three_calls(ext, ref, CASES[name])


@pytest.mark.parametrize("name", ["admit_one_neighbour", "admit_32_neighbours", "admit_n_new_1", "admit_n_new_65_and_kmax",
                                  "admit_refused_and_skipped_blocks", "admit_recent_cap_reached", "admit_recent_cap_one_short",
                                  "admit_id_at_n_table", "admit_count_beyond_kmax"])
def test_admit_map_points_resident(ext, ref, name):
    three_calls(ext, ref, CASES[name])


@pytest.mark.parametrize("name", ["stat_n_kp_0", "stat_n_kp_1", "stat_n_kp_65", "stat_n_kp_1001", "stat_point_cap_1", "stat_small"])
def test_track_statistics_resident(ext, ref, name):
    three_calls(ext, ref, CASES[name])


@pytest.mark.parametrize("first,n_rows,reset_list", [(0, 1, False), (3, 40, True), (47, 1, True), (0, 0, True), (0, 48, False)])
def test_mp_life_reset_resident(ext, ref, first, n_rows, reset_list):
    import torch
    w = mc.mixed_world(9, 40)
    assert len(w["flags"]) == 48
    want = mr.copy_world(w)
    mr.reset(ref, want, first, n_rows, reset_list)
    arena = ea.Arena("cuda")
    for k in mr.STATE:
        arena.place(k, w[k])

    def run(ar):
        ext.mp_life_reset_resident(X.mp_life({k: ar.ptr(k) for k in mr.STATE}, 48, len(w["recent"])), first, n_rows, reset_list)
        torch.cuda.synchronize()
    found, _ = ea.report(arena, run, mr.STATE, {k: want[k] for k in mr.STATE})
    assert found == [], found


def test_einval_leaves_everything_untouched(ext):
    import torch
    c = CASES["cull_every_code"]
    a = CASES["admit_one_neighbour"]
    s = CASES["stat_small"]
    t = {}
    for key, case in (("c", c), ("a", a), ("s", s)):
        for k, v in mg.buffers(case).items():
            t[key + k] = (torch.full((int(v),), 0xA5, dtype=torch.uint8, device="cuda") if isinstance(v, (int, np.integer)) else
                          torch.from_numpy(mg.raw(v).copy()).cuda())
    before = {k: v.clone() for k, v in t.items()}

    def ptrs(key):
        return {k[1:]: v.data_ptr() for k, v in t.items() if k[0] == key}

    def refused(fn, what):
        with pytest.raises(X.SpfeError) as info:
            fn()
        assert str(info.value).startswith("SPFE_EINVAL"), (what, info.value)

    # the cull
    P = ptrs("c")
    n, stride = c["rows"].shape
    ok = dict(P, n_table=len(c["flags"]), recent_cap=len(c["recent"]), stride=stride, n=n, th_obs=2, bad_cap=8)
    bad = [dict(n_table=0), dict(n_table=262145), dict(recent_cap=0), dict(recent_cap=262145), dict(stride=0), dict(stride=16385), dict(n=0),
           dict(n=65537), dict(th_obs=-1), dict(bad_cap=-1), dict(bad_cap=262145), dict(rows=None), dict(kf_flags=None), dict(d_out=None),
           dict(rows=P["rows"] + 2), dict(d_out=P["d_out"] + 8)]
    bad += [{k: None} for k in mr.STATE] + [{k: P[k] + 2} for k in mr.STATE if k != "flags"]
    for change in bad:
        q = dict(ok, **change)
        life = X.mp_life({k: q[k] for k in mr.STATE}, q["n_table"], q["recent_cap"])
        refused(lambda: ext.cull_map_points_resident(life, q["rows"], q["stride"], q["kf_flags"], q["n"], 50, q["d_out"], th_obs=q["th_obs"],
                                                     bad_cap=q["bad_cap"]), change)
    # the admission
    P = ptrs("a")
    n, stride = a["rows"].shape
    ok = dict(P, n_table=len(a["flags"]), recent_cap=len(a["recent"]), stride=stride, n=n, n_neigh=1, cur=6)
    bad = [dict(n_table=0), dict(recent_cap=262145), dict(stride=0), dict(n=65537), dict(n_neigh=0), dict(n_neigh=33), dict(cur=-1), dict(cur=n),
           dict(tri=None), dict(neigh_slot=None), dict(rows=None), dict(xyz=None), dict(d_out=None), dict(tri=P["tri"] + 8),
           dict(neigh_slot=P["neigh_slot"] + 2), dict(rows=P["rows"] + 1), dict(xyz=P["xyz"] + 2), dict(d_out=P["d_out"] + 4)]
    bad += [{k: None} for k in mr.STATE] + [{k: P[k] + 1} for k in mr.STATE if k != "flags"]
    for change in bad:
        q = dict(ok, **change)
        life = X.mp_life({k: q[k] for k in mr.STATE}, q["n_table"], q["recent_cap"])
        refused(lambda: ext.admit_map_points_resident(life, q["tri"], q["n_neigh"], q["neigh_slot"], q["cur"], 50, q["rows"], q["stride"], q["n"],
                                                      q["xyz"], q["d_out"]), change)
    # the statistics
    P = ptrs("s")
    n_kp, cap = len(s["entry"]), len(s["point_idx"])
    ok = dict(P, n_table=len(s["flags"]), recent_cap=4, n_kp=n_kp, cap=cap)
    bad = [dict(n_table=0), dict(recent_cap=0), dict(n_kp=-1), dict(n_kp=8193), dict(cap=0), dict(cap=8193), dict(entry=None), dict(after=None),
           dict(point_idx=None), dict(proj_out=None), dict(pose_out=None), dict(d_out=None), dict(flags=None), dict(found=None),
           dict(visible=None), dict(entry=P["entry"] + 2), dict(after=P["after"] + 1), dict(point_idx=P["point_idx"] + 2),
           dict(found=P["found"] + 2), dict(visible=P["visible"] + 1), dict(d_out=P["d_out"] + 8)]
    for change in bad:
        q = dict(ok, **change)
        life = X.mp_life({k: q.get(k) for k in mr.STATE}, q["n_table"], q["recent_cap"])
        refused(lambda: ext.track_statistics_resident(life, q["entry"], q["after"], q["n_kp"], q["point_idx"], q["cap"], q["proj_out"],
                                                      q["pose_out"], q["d_out"]), change)
    # the reset
    P = ptrs("c")
    life = X.mp_life({k: P[k] for k in mr.STATE}, len(c["flags"]), len(c["recent"]))
    for first, n_rows, rl in ((-1, 1, 0), (0, -1, 1), (0, 0, 0), (len(c["flags"]), 1, 0), (1, len(c["flags"]), 1)):
        refused(lambda: ext.mp_life_reset_resident(life, first, n_rows, rl), (first, n_rows, rl))
    for k in mr.STATE:
        refused(lambda: ext.mp_life_reset_resident(X.mp_life(dict({q: P[q] for q in mr.STATE}, **{k: None}), len(c["flags"]), len(c["recent"])),
                                                   0, 1, 1), k)
    torch.cuda.synchronize()
    for k in t:
        assert torch.equal(t[k], before[k]), k
