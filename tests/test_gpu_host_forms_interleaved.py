"""GPU: the thirteen host-array forms share one staging buffer and one pinned mirror per handle.  One handle runs a fixed
sequence of them in which the staging grows in the middle (spfe_bundle_adjust on ba_cases.large()) and small calls follow large
ones; every array and block every call returns must equal, byte for byte, what a handle returns that was created for that one
call.  Blocks are handed in filled with 0x5A, so a block or mirror another form left dirty, or one read at a stale size, shows.

The frame is the 64 x 96 one of the fuse, guided, sim3, loop-point and loop-fuse fixtures (NF = 100).  dust_small was made for a
30 x 40 map: its map is sampled down to this frame's 8 x 12 cells and its intrinsics are scaled with it, so that its 40 points
still project into the map (3 iterations, 21 inliers by the oracle) — both handles see the same arrays."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("ba_ref", "fuse_ref", "guided_ref", "loopfuse_ref", "sim3_ref"):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
import ba_cases  # noqa: E402
import ba_ref  # noqa: E402
import fuse_cases as fc  # noqa: E402
import guided_cases as gc  # noqa: E402
import loopfuse_cases as lc  # noqa: E402
import sim3_cases as sc  # noqa: E402

from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import SPExtractor  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden")
H, W, NF = 64, 96, 100
FILL = 0x5A


def golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def dust(ext):
    g = golden("dust_small")
    fx, fy, cx, cy = [float(v) for v in g["intr"]]
    hc, wc = H // 8, W // 8
    sy, sx = hc / g["dust"].shape[0], wc / g["dust"].shape[1]
    m = np.ascontiguousarray(g["dust"][(np.arange(hc) / sy).astype(int)][:, (np.arange(wc) / sx).astype(int)])
    return ext.align_dust(m, g["pts"], g["Tcw_init"], fx * sx, fy * sy, (cx - 3.5) * sx + 3.5, (cy - 3.5) * sy + 3.5)


def fuse(ext):
    g = fc.load("proposed")
    t, p = fc.targets(g)[0], fc.points(g)
    return ext.fuse_search(t["kp_xy"], t["occ"], t["kp_desc"], t["kf_mp"], t["Tcw"], *[p[k] for k in fc.POINT_KEYS],
                           *[float(v) for v in g["intr"]])


def loop_fuse(ext):
    g = lc.load("proposed")
    t, p = lc.targets(g)[0], lc.points(g)
    return ext.loop_fuse_search(t["kp_xy"], t["occ"], t["kp_desc"], t["kf_mp"], t["Scw"], *[p[k] for k in lc.POINT_KEYS],
                                *[float(v) for v in g["intr"]])


def ba(c):
    def run(ext):
        a = ba_ref.arrays(c)
        return ext.bundle_adjust(a["edges"], a["obs_xy"], a["inv_sigma2"], a["Tcw"], a["fixed"], a["xyz"], [float(v) for v in c["intr"]],
                                 schedule=int(c["schedule"]), iterations=[int(v) for v in c["iterations"]], robust=int(c["robust"]),
                                 inv_sigma2_full=float(c["inv_sigma2_full"]), stop=1 if int(c["stop_reads"]) == 0 else None, fill=FILL)
    return run


def guided(ext):
    g = gc.load("reasons")
    kf1, kf2 = gc.keyframes(g)
    return ext.search_by_sim3(kf1, kf2, *[g[k] for k in gc.MAP_KEYS], kf1["Tcw"], kf2["Tcw"], g["T12"], g["seed12"], g["intr1"],
                              g["intr2"], fill=FILL, **gc.prm_of(g))


def sim3(ext):
    g = sc.load("n_eq_min")
    K1, K2 = int(g["K1"]), int(g["K2"])
    return ext.sim3_ransac(g["match12"][:K1], g["mp1"][:K1], g["mp2"][:K2], g["xyz"], g["flags"], g["Tcw1"], g["Tcw2"], g["rnd"],
                           g["intr1"], g["intr2"], min_inliers=int(g["min_inliers"]), fix_scale=int(g["fix_scale"]), fill=FILL)


def loop_points(ext):
    g = gc.lp_load("reasons")
    return ext.search_loop_points(g["kp_xy"], g["occ"], g["kp_desc"], g["Scw"], g["matched"], *[g[k] for k in gc.POINT_KEYS],
                                  *[float(v) for v in g["intr"]])


def sim3opt(ext):
    g = golden("sim3opt_kept10")
    v = [float(x) for x in g["intr"]]
    return ext.optimize_sim3(g["kp_xy1"], g["mp1"], g["kp_xy2"], g["mp2"], g["xyz"], g["flags"], g["Tcw1"], g["Tcw2"], g["T12"],
                             g["matches12"], v[:4], v[4:], fix_scale=int(g["fix_scale"]), fill=FILL)


def proj(ext):
    g = golden("proj_far_best")
    run = g["runs"][0]
    return ext.search_projection(g["kp_xy"], g["occ"], g["kp_desc"], g["xyz"], g["normal"], g["desc"], g["flags"], g["mp_of_kp"],
                                 g["Tcw"], *g["intr"], mode=int(run[0]), th=run[1], th_dist=run[2], view_cos_limit=run[3],
                                 adaptive=bool(run[4]), c2_thresh=run[5])


def pose(ext):
    g = golden("pose_n10")
    return ext.refine_pose(g["obs"], g["w"], g["pts"], g["Tcw_init"], *g["intr"])


def keyframe():
    """the 61 keypoints of proj_visibility and 24 map points that re-observe distinct ones (descriptor noise 0.2), for the matchers"""
    t = golden("proj_visibility")
    rng = np.random.default_rng(3)
    k = rng.permutation(len(t["kp_xy"]))[:24]
    noise = rng.standard_normal((24, 256)).astype(np.float32)
    desc = (t["kp_desc"][k] + np.float32(0.2) * noise / np.linalg.norm(noise, axis=1, keepdims=True)).astype(np.float32)
    uv = (np.floor(t["kp_xy"][k] / 8) - rng.integers(0, 2, (24, 2)) + rng.random((24, 2)) * 0.999).astype(np.float32)
    return t, desc, uv


def match(ext):
    t, desc, _ = keyframe()
    return ext.match(desc, t["kp_desc"], cross_check=True)


def knn2(ext):
    t, desc, _ = keyframe()
    return ext.match_knn2(desc, t["kp_desc"])


def patches(ext):
    t, desc, uv = keyframe()
    return ext.match_patches(desc, uv, t["occ"], t["kp_desc"])


def flat(r, path="r"):
    """a result (array, scalar, tuple or dict of them) -> [(path, bytes)]"""
    if isinstance(r, dict):
        return [x for k in sorted(r) for x in flat(r[k], "%s[%s]" % (path, k))]
    if isinstance(r, (tuple, list)):
        return [x for i, v in enumerate(r) for x in flat(v, "%s[%d]" % (path, i))]
    a = np.asarray(r)
    return [(path, str(a.dtype).encode() + repr(a.shape).encode() + a.tobytes())]


def test_interleaved_forms_equal_a_fresh_handle_byte_for_byte():
    blob = weights.synthetic(7, "trackable")
    forms = {"dust": dust, "fuse": fuse, "ba_small": ba(golden("ba_small")), "guided": guided, "ba_large": ba(ba_cases.large()),
             "sim3": sim3, "loop_points": loop_points, "sim3opt": sim3opt, "proj": proj, "pose": pose, "match": match,
             "patches": patches, "loop_fuse": loop_fuse, "knn2": knn2}
    first = ["dust", "fuse", "ba_small", "guided"]
    order = first + ["ba_large"] + first[::-1] + ["sim3", "loop_points", "sim3opt", "proj", "pose", "match", "patches", "loop_fuse",
                                                  "knn2"]
    raw, want = {}, {}
    for name in dict.fromkeys(order):          # a handle created for that one call and that one form
        ext = SPExtractor(NF, H, W, blob, with_heat=False)
        raw[name] = forms[name](ext)
        want[name] = flat(raw[name])
        ext.close()
    # the reference calls did their work: what is compared below is not untouched fill
    assert raw["dust"]["iterations"] >= 2 and raw["dust"]["n_inlier"] > 0 and raw["fuse"]["n_fused"] > 0
    assert (raw["match"][0] >= 0).sum() >= 12 and (raw["patches"] >= 0).sum() >= 12 and (raw["knn2"][0] >= 0).all()
    for name, c in (("ba_small", golden("ba_small")), ("ba_large", ba_cases.large())):
        n_kf, n, E = len(c["Tcw"]), len(c["xyz"]), len(c["edges"])
        d = SPExtractor.decode_ba_out(raw[name], n_kf, n, E)
        assert d["status"] == 0 and d["n_served"] == E and d["iterations"].sum() > 0, name
    assert len(raw["ba_large"]) > 16 * len(raw["ba_small"])         # the staging grows in the middle of the sequence
    ext = SPExtractor(NF, H, W, blob, with_heat=False)
    try:
        for step, name in enumerate(order):
            got = flat(forms[name](ext))
            assert [p for p, _ in got] == [p for p, _ in want[name]], (step, name)
            for (p, g), (_, w) in zip(got, want[name]):
                assert g == w, (step, name, p)
    finally:
        ext.close()
