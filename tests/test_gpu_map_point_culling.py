"""GPU: map-point culling on the device and its resident state — spfe_mp_life_reset_resident, spfe_admit_map_points_resident,
spfe_track_statistics_resident, spfe_cull_map_points_resident and the three host-array forms — against
tests/mpcull_ref/mpcull_ref.c byte for byte: the state, the rows, the table, the list and the blocks.  The cases are the named
cases of tests/mpcull_ref/mpcull_cases.py (list lengths on both sides of a wavefront, of a decision workgroup and of a compaction
chunk; duplicates inside a chunk and across its boundary; the ratio's threshold with its rounding case; ages and observation counts;
every code, wild entries, bad_cap 0 and cut; 1 - 300 slots and row pitches 1 - 1001 with the rows 0 - 12 bytes off a 16-byte boundary;
admissions of 1 and 32 neighbours, refused and skipped blocks, the all-or-nothing refusals, a displaced holder; statistics of 0 -
1001 keypoints) and a sequence of 60 keyframes whose state never leaves the device, alternating with
spfe_update_connections_resident and spfe_cull_keyframes_resident and compared at every step."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("mpcull_ref", "cull_ref", "covis_ref"):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
import covis_ref  # noqa: E402
import cull_ref  # noqa: E402
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
    assert e.layout.kmax == mc.KMAX
    yield e
    e.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_named_case_equals_the_reference_in_both_forms(ext, ref, name):
    c = CASES[name]
    mg.check(ext, ref, c, what=name)
    if c["op"] == "cull":                      # the rows 4, 8 and 12 bytes off a 16-byte boundary
        want, _ = mg.want_of(ref, c)
        for shift in (4, 8, 12):
            mg.same(mg.run_resident(ext, c, shift), want, c, "%s, rows %d bytes off" % (name, shift))


def test_reset_presets_a_row_range_and_the_list(ext, ref):
    import torch
    w = mc.mixed_world(3, 40)
    want = mr.copy_world(w)
    mr.reset(ref, want, 5, 17, True)
    want2 = mr.copy_world(want)
    mr.reset(ref, want2, len(w["flags"]) - 1, 1, False)
    t = {k: torch.from_numpy(mg.raw(w[k]).copy()).cuda() for k in mr.STATE}
    life = X.mp_life({k: v.data_ptr() for k, v in t.items()}, len(w["flags"]), len(w["recent"]))
    ext.mp_life_reset_resident(life, 5, 17, True)
    torch.cuda.synchronize()
    for k in mr.STATE:
        assert t[k].cpu().numpy().tobytes() == mg.raw(want[k]).tobytes(), k
    ext.mp_life_reset_resident(life, len(w["flags"]) - 1, 1, False)
    torch.cuda.synchronize()
    for k in mr.STATE:
        assert t[k].cpu().numpy().tobytes() == mg.raw(want2[k]).tobytes(), k
    assert want["recent_n"][0] == 0 and (want["recent"] == -1).all() and want["first_kf"][5] == -1 and want["flags"][21] == 0


def test_sequence_of_60_keyframes_on_resident_state(ext, ref, tmp_path):
    """the mapping cycle per keyframe — the host's row (single-entry writes), the map-point cull at its id, the admission of its new
    points, UpdateConnections, two tracked frames' statistics and, every other keyframe, the keyframe cull — with every array on the
    device from the first call to the last, against the host references chained on one world, compared after every call"""
    import torch
    kref, cref = cull_ref.build(tmp_path), covis_ref.build(tmp_path)
    n, cap, th, bad_cap = 60, 16, 3, 32
    w, rng, geo = mc.sequence_world(77, n_slots=n)
    stride, n_table, rc = w["rows"].shape[1], len(w["flags"]), len(w["recent"])
    w.update(cull_ref.new_state(n, cap))
    w["mp_flags"] = w["flags"]                                   # ONE array under the two references' names
    for k, nb in (("best_a", 20), ("best_b", 10)):
        w[k] = np.full((n, nb), -1, np.int32)
    names = tuple(mr.WORLD) + tuple(cull_ref.STATE) + ("best_a", "best_b")
    t = {k: torch.from_numpy(mg.raw(w[k]).copy()).cuda() for k in names}
    P = {k: v.data_ptr() for k, v in t.items()}
    blocks = dict(mp=ext.mpcull_out_bytes(rc, bad_cap), admit=X.ADMIT_OUT_BYTES, stat=X.MPSTAT_OUT_BYTES, covis=ext.covis_out_bytes(n, cap),
                  kf=ext.cull_out_bytes(n, cap, bad_cap))
    d_out = {k: torch.full((v,), mg.FILL, dtype=torch.uint8, device="cuda") for k, v in blocks.items()}
    life = X.mp_life({k: P[k] for k in mr.STATE}, n_table, rc)
    graph = X.covis_graph({k: P[k] for k in cull_ref.STATE}, n, cap)
    # the state's preset is the library's: poison first
    for k in mr.STATE:
        t[k].fill_(0x5A)
    ext.mp_life_reset_resident(life, 0, n_table, True)
    ext.covis_reset_slots_resident(graph, 0, n)
    shadow = {k: np.ascontiguousarray(w[k]).copy() for k in names}          # what the device holds, as far as the host has written

    def push():
        """the host's edits since the last call, as single-entry writes"""
        for k in names:
            flat, old = w[k].reshape(-1), shadow[k].reshape(-1)
            idx = np.flatnonzero(flat.view(np.uint32 if flat.dtype == np.float32 else flat.dtype) !=
                                 old.view(np.uint32 if old.dtype == np.float32 else old.dtype))
            if len(idx):
                view = t[k].view(torch.int32 if flat.dtype.itemsize == 4 else torch.uint8)
                src = flat[idx].view(np.int32) if flat.dtype.itemsize == 4 else flat[idx]
                view[torch.from_numpy(idx).cuda()] = torch.from_numpy(src.copy()).cuda()

    def compare(what, key, block):
        torch.cuda.synchronize()
        assert d_out[key].cpu().numpy().tobytes() == block.tobytes(), (what, "block")
        for k in names:
            got = t[k].cpu().numpy()
            assert got.tobytes() == mg.raw(w[k]).tobytes(), (what, k, np.flatnonzero(got != mg.raw(w[k]))[:6].tolist())
            shadow[k] = np.ascontiguousarray(w[k]).copy()

    codes, culled_kf = np.zeros(6, np.int64), 0
    for s in range(n):
        mc.sequence_keyframe(w, rng, geo, s)
        push()
        kf_id = mc.SEQ["first_id"] + s
        r = mr.cull(ref, w, kf_id, 2, 0.25, bad_cap)
        ext.cull_map_points_resident(life, P["rows"], stride, P["kf_flags"], n, kf_id, d_out["mp"].data_ptr(), th_obs=2, found_ratio=0.25,
                                     bad_cap=bad_cap)
        compare("keyframe %d: map-point cull" % s, "mp", r["block"])
        codes += np.bincount(r["entry_code"][:r["n_listed"]], minlength=6)
        a = mc.sequence_admission(w, rng, geo, s)
        r = mr.admit(ref, w, a["tri"], mc.KMAX, a["n_neigh"], a["neigh_slot"], s, kf_id)
        d_tri, d_ns = torch.from_numpy(a["tri"]).cuda(), torch.from_numpy(a["neigh_slot"]).cuda()
        ext.admit_map_points_resident(life, d_tri.data_ptr(), a["n_neigh"], d_ns.data_ptr(), s, kf_id, P["rows"], stride, n, P["xyz"],
                                      d_out["admit"].data_ptr())
        compare("keyframe %d: admission" % s, "admit", r["block"])
        r = covis_ref.update(cref, w["rows"], w["kf_flags"], w["mp_flags"], {k: w[k] for k in covis_ref.STATE}, s, th, 0, w["best_a"], w["best_b"])
        ext.update_connections_resident(graph, P["rows"], stride, P["kf_flags"], P["flags"], n_table, s, d_out["covis"].data_ptr(), th=th,
                                        origin_slot=0, d_best_cov_a=P["best_a"], n_best_a=20, d_best_cov_b=P["best_b"], n_best_b=10)
        compare("keyframe %d: UpdateConnections" % s, "covis", r["block"])
        for f in range(2):
            fr = mc.sequence_frame(w, rng)
            c = mc.stat_case(w, fr["entry"], fr["after"], fr["point_idx"], fr["in_view"], fr["outlier"])
            r = mr.stat(ref, w, fr["entry"], fr["after"], fr["point_idx"], fr["in_view"], fr["outlier"])
            b = mg.buffers(c)
            d = {k: torch.from_numpy(mg.raw(b[k]).copy()).cuda() for k in ("entry", "after", "point_idx", "proj_out", "pose_out")}
            ext.track_statistics_resident(life, d["entry"].data_ptr(), d["after"].data_ptr(), len(fr["entry"]), d["point_idx"].data_ptr(),
                                          len(fr["point_idx"]), d["proj_out"].data_ptr(), d["pose_out"].data_ptr(), d_out["stat"].data_ptr())
            compare("keyframe %d: statistics of frame %d" % (s, f), "stat", r["block"])
        if s % 2 == 1:
            r = cull_ref.cull(kref, w, s, th_obs=4, cov_ratio=0.8, origin_slot=0, bad_cap=bad_cap)
            ext.cull_keyframes_resident(graph, P["rows"], stride, P["kf_flags"], P["flags"], P["nobs"], n_table, s, d_out["kf"].data_ptr(),
                                        th_obs=4, cov_ratio=0.8, origin_slot=0, bad_cap=bad_cap, d_best_cov_a=P["best_a"], n_best_a=20,
                                        d_best_cov_b=P["best_b"], n_best_b=10)
            compare("keyframe %d: keyframe cull" % s, "kf", r["block"])
            culled_kf += r["n_culled"]
        good = (w["flags"] & 1).astype(bool)
        fresh = cull_ref.count(kref, w["rows"], w["kf_flags"], n_table)
        assert (w["nobs"][good] == fresh[good]).all(), "nobs drifted from the rows at keyframe %d" % s
    print("codes over the sequence", codes.tolist(), "keyframes culled", culled_kf)
    assert (codes[:5] >= 3).all() and culled_kf >= 3, (codes, culled_kf)
