"""GPU: the search of SPMatcher::Fuse on resident keyframe records (spfe_fuse_search, spfe_fuse_record_device,
spfe_fuse_targets_record_device: fuse.hip) against the host reference tests/fuse_ref/fuse_ref.c, which shares
include/spfe_fuse_math.h with the kernels: every output, best_dist included, bit for bit — on the fixtures
tests/golden/fuse_*.npz laid out as records by spfe_get_record_layout, with f32 and with bf16 descriptor rows; the targets
form against the one-target form byte for byte; the boundary shapes of the point count, the keypoint count and the target
count; one extracted scene end to end; the refusals and the decision on overflowed records."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "fuse_ref"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tri_ref"))
sys.path.insert(0, os.path.join(ROOT, "tests", "track_ref"))
import fuse_cases as fc  # noqa: E402
import fuse_ref  # noqa: E402
import track_cases as trk  # noqa: E402

from sp_orb_slam_amd import extractor as X  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import SPExtractor  # noqa: E402
from tools import track_scene as ts  # noqa: E402

pytestmark = pytest.mark.gpu
H, W, NF = 64, 96, 100          # the fixtures' frame; kmax = 101 > 65 keypoints
FILL = 0xA5
OUT = ("reason", "kp_of_mp", "holder", "fused_idx")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return fuse_ref.build(tmp_path_factory.mktemp("fuse_ref"))


@pytest.fixture(scope="module")
def exts():
    blob = weights.synthetic(7, "trackable")
    e = {False: SPExtractor(NF, H, W, blob, with_heat=False), True: SPExtractor(NF, H, W, blob, with_heat=False, desc_bf16=True)}
    yield e
    for x in e.values():
        x.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def record_host(ext, t, K=None, status=0):
    """a target (kp_xy, occ, kp_desc f32) as the bytes of one record of the handle's layout; K: the header's count"""
    L = ext.layout
    n = len(t["kp_xy"])
    K = n if K is None else K
    assert n <= L.kmax and t["occ"].shape == (ext.height // 8, ext.width // 8)
    b = np.zeros(ext.record_bytes(), np.uint8)
    b[L.off_hdr:L.off_hdr + 16].view(np.int32)[:] = [K, K, status, 0]
    b[L.off_xy:L.off_xy + 8 * n].view(np.float32)[:] = np.ascontiguousarray(t["kp_xy"], np.float32).reshape(-1)
    b[L.off_occ:L.off_occ + 2 * t["occ"].size].view(np.int16)[:] = np.ascontiguousarray(t["occ"], np.int16).reshape(-1)
    if ext.desc_bf16:
        b[L.off_desc:L.off_desc + 512 * n].view(np.uint16)[:] = fuse_ref.to_bf16(t["kp_desc"]).reshape(-1)
    else:
        b[L.off_desc:L.off_desc + 1024 * n].view(np.float32)[:] = np.ascontiguousarray(t["kp_desc"], np.float32).reshape(-1)
    return b


def record(ext, t, K=None, status=0):
    """... on the device"""
    return dev(record_host(ext, t, K, status))


def padded(ext, mp, fill=-1):
    out = np.full(ext.layout.kmax, fill, np.int32)
    out[:len(mp)] = mp
    return out


def dev_points(p, n=None):
    """the point arrays on the device (one dummy row when there is none: the pointers are not read)"""
    n = len(p["point_id"]) if n is None else n
    return {k: dev(p[k][:n] if n else np.zeros((1,) + p[k].shape[1:], p[k].dtype)) for k in fc.POINT_KEYS}


def point_ptrs(d):
    return [d[k].data_ptr() for k in fc.POINT_KEYS]


def one_target(ext, d_rec, kf_mp, Tcw, d_pts, n, intr, n_cap=None, **kw):
    """spfe_fuse_record_device -> (decoded block, raw block); checks that kf_mp_of_kp is left alone"""
    import torch
    cap = max(n, 1) if n_cap is None else n_cap
    d_mp, d_T = dev(kf_mp), dev(np.asarray(Tcw, np.float32).reshape(16))
    d_out = torch.full((ext.fuse_out_bytes(cap),), FILL, dtype=torch.uint8, device="cuda")
    ext.fuse_record_device(d_rec.data_ptr(), d_mp.data_ptr(), d_T.data_ptr(), *point_ptrs(d_pts), n, d_out.data_ptr(), *intr,
                           n_cap=cap, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(d_mp.cpu().numpy(), kf_mp)
    raw = d_out.cpu().numpy()
    return ext.decode_fuse_out(raw, cap), raw


def many_targets(ext, d_recs, kf_mps, Tcws, d_pts, n, intr, n_cap=None, **kw):
    """spfe_fuse_targets_record_device -> raw blocks [n_targets][out_bytes]"""
    import torch
    cap = max(n, 1) if n_cap is None else n_cap
    nt, ob = len(d_recs), ext.fuse_out_bytes(cap)
    mp = np.stack(kf_mps)
    d_mp, d_T = dev(mp), dev(np.stack([np.asarray(T, np.float32).reshape(16) for T in Tcws]))
    d_out = torch.full((nt * ob,), FILL, dtype=torch.uint8, device="cuda")
    ext.fuse_targets_record_device([r.data_ptr() for r in d_recs], d_mp.data_ptr(), d_T.data_ptr(), *point_ptrs(d_pts), n,
                                   d_out.data_ptr(), *intr, n_cap=cap, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(d_mp.cpu().numpy(), mp)
    return d_out.cpu().numpy().reshape(nt, ob)


def same(got, want, what):
    for k in OUT:
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    assert got["n_fused"] == want["n_fused"], what
    assert np.array_equal(got["best_dist"].view(np.uint32), want["best_dist"].view(np.uint32)), (what, "best_dist bits")


def unwritten(ext, raw, n, n_fused, cap):
    """entries at and beyond n (fused_idx: n_fused) and the padding keep the fill"""
    o = X.fuse_offsets(cap)
    assert (raw[12:64] == FILL).all()
    for lo, size, used, end in ((64, 4, n, o["best_dist"]), (o["best_dist"], 4, n, o["holder"]), (o["holder"], 4, n, o["fused_idx"]),
                                (o["fused_idx"], 4, n_fused, o["reason"]), (o["reason"], 1, n, o["out_bytes"])):
        assert (raw[lo + size * used:end] == FILL).all(), lo


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", fc.NAMES)
def test_all_three_forms_equal_the_host_reference_bit_for_bit(exts, ref, name, bf16):
    g = fc.load(name)
    assert (int(g["H"]), int(g["W"])) == (H, W)
    ext = exts[bf16]
    tgs, p = fc.targets(g), fc.points(g)
    n, intr = len(p["point_id"]), [float(v) for v in g["intr"]]
    d_pts = dev_points(p)
    recs = [record(ext, t) for t in tgs]
    mps = [padded(ext, t["kf_mp"]) for t in tgs]
    raws = []
    for j, t in enumerate(tgs):
        want = fc.run_ref(ref, g, j)                                      # (the fixtures' rows are bf16 values: both see the same numbers)
        assert fc.differences(g, j, want) == []
        got, raw = one_target(ext, recs[j], mps[j], t["Tcw"], d_pts, n, intr)
        same(got, want, (name, j, "record form"))
        assert got["n"] == n and got["status"] == 0
        unwritten(ext, raw, n, got["n_fused"], max(n, 1))
        raws.append(raw)
        if not bf16:
            host = ext.fuse_search(t["kp_xy"], t["occ"], t["kp_desc"], t["kf_mp"], t["Tcw"], *[p[k] for k in fc.POINT_KEYS], *intr)
            same(host, want, (name, j, "host form"))
    blocks = many_targets(ext, recs, mps, [t["Tcw"] for t in tgs], d_pts, n, intr)
    for j in range(len(tgs)):
        assert np.array_equal(blocks[j], raws[j]), (name, j, "targets form")


def big_target(seed=11, K=65):
    """65 keypoints in neighbouring cells (several per window), and points on them"""
    rng = np.random.default_rng(seed)
    cells = [(ix, iy) for iy in range(1, 7) for ix in range(12)][:K]
    occ = np.full((H // 8, W // 8), -1, np.int16)
    kp = np.zeros((K, 2), np.float32)
    for k, (ix, iy) in enumerate(cells):
        occ[iy, ix] = k
        kp[k] = (8 * ix + rng.integers(2, 14) * 0.5, 8 * iy + rng.integers(2, 14) * 0.5)
    base = rng.normal(size=(K, 256))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = (0.05, -0.03, 0.1)
    return dict(kp_xy=kp, occ=occ, kp_desc=base.astype(np.float32), kf_mp=np.full(K, -1, np.int32), Tcw=T)


def points_on(t, n, seed, intr):
    """n points near the target's keypoints (some off them, bad, out of range, behind or turned away)"""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = intr
    K = len(t["kp_xy"])
    k = rng.integers(0, K, n)
    uv = t["kp_xy"][k] + rng.normal(0, 1.2, (n, 2))
    z = rng.uniform(2, 6, n) * np.where(rng.random(n) < 0.03, -1, 1)
    T = t["Tcw"].astype(np.float64)
    Pc = np.stack([(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, z], 1)
    P = (Pc - T[:3, 3]) @ T[:3, :3]
    PO = P + T[:3, :3].T @ T[:3, 3]
    dist = np.linalg.norm(PO, axis=1)
    noise = rng.normal(size=(n, 256))
    noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    desc = t["kp_desc"][k] + rng.choice([0.05, 0.2, 0.29, 0.31, 0.6], (n, 1)) * noise
    lo, hi = rng.choice([0.7, 0.7, 0.9, 0.9, 0.9, 1.26], n), rng.choice([1.4, 1.4, 1.1, 1.1, 1.1, 0.82], n)
    tilt = rng.choice([1.0, 1.0, 0.8, 0.8, 0.45, 2.0], n)
    return dict(point_id=(1000 + np.arange(n)).astype(np.int32), xyz=P.astype(np.float32),
                normal=(PO / dist[:, None] * tilt[:, None]).astype(np.float32),
                dist_range=np.stack([dist * lo, dist * hi], 1).astype(np.float32), desc=desc.astype(np.float32),
                flags=rng.choice(np.array([1, 1, 1, 1, 1, 1, 3, 3, 0, 2], np.uint8), n))


def ref_run(ref, t, p, n, K, intr):
    return fuse_ref.search(ref, t["kp_xy"][:K], t["occ"], t["kp_desc"][:K], t["kf_mp"][:K], t["Tcw"], *[p[k][:n] for k in fc.POINT_KEYS],
                           intr, W, H)


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, X.PROJ_MAX_POINTS])
def test_point_counts_around_a_workgroup_of_four_waves_and_at_the_capacity(exts, ref, n):
    ext, intr = exts[False], (ts.FX / 4, ts.FY / 4, 47.5, 31.25)
    t = big_target()
    p = points_on(t, max(n, 8), 12, intr)
    p["flags"][2] = 1
    t["kf_mp"][[3, 9]] = (p["point_id"][2], 77)                           # point 2 is in the keyframe; a holder
    want = ref_run(ref, t, p, n, 65, intr)
    cap = max(n, 1) + (3 if n < 100 else 0)                               # a capacity above n: the layout is the capacity's
    got, raw = one_target(ext, record(ext, t), padded(ext, t["kf_mp"]), t["Tcw"], dev_points(p, n), n, intr, n_cap=cap)
    same(got, want, n)
    unwritten(ext, raw, n, got["n_fused"], cap)
    if n >= 3:
        assert want["reason"][2] == fuse_ref.SKIP_IN_KF
    if n == X.PROJ_MAX_POINTS:
        print("reasons at the capacity:", np.bincount(want["reason"], minlength=10)[1:])
        assert (np.bincount(want["reason"], minlength=10)[1:] > 0).sum() >= 8 and want["n_fused"] > 1000


@pytest.mark.parametrize("K", [0, 63, 64, 65])
def test_keypoint_counts_around_the_id_scans_stride(exts, ref, K):
    """The ids of points 0, 1, 2 are held by keypoints 62, 63, 64: the last entries a scan of 63, 64, 65 keypoints reads.
    Entries at and beyond K are ignored, in the holder array as in the record."""
    ext, intr = exts[False], (ts.FX / 4, ts.FY / 4, 47.5, 31.25)
    t = big_target()
    p = points_on(t, 40, 13, intr)
    p["flags"][:3] = 1
    t["kf_mp"][[62, 63, 64]] = p["point_id"][:3]
    want = ref_run(ref, t, p, 40, K, intr)
    assert [int(r == fuse_ref.SKIP_IN_KF) for r in want["reason"][:3]] == [int(K > 62), int(K > 63), int(K > 64)]
    got, _ = one_target(ext, record(ext, t, K=K), padded(ext, t["kf_mp"], fill=int(p["point_id"][5])), t["Tcw"], dev_points(p), 40, intr)
    same(got, want, K)                                                     # (the padding beyond the keypoints names point 5: ignored)
    assert want["reason"][5] != fuse_ref.SKIP_IN_KF
    if K == 0:
        assert want["n_fused"] == 0 and fuse_ref.NO_CANDIDATE in want["reason"]


def test_the_largest_window_takes_two_rounds_of_cells(exts, ref):
    """th = SPFE_PROJ_MAX_RADIUS: up to 11 x 11 cells, more than the 64 a wavefront tests at once; without the chi-square gate
    (chi2 = 1e9) every keypoint of the window is a candidate."""
    ext, intr = exts[False], (ts.FX / 4, ts.FY / 4, 47.5, 31.25)
    t = big_target()
    p = points_on(t, 60, 14, intr)
    kw = dict(th=float(X.PROJ_MAX_RADIUS), chi2=1e9)
    want = fuse_ref.search(ref, t["kp_xy"], t["occ"], t["kp_desc"], t["kf_mp"], t["Tcw"], *[p[k] for k in fc.POINT_KEYS], intr, W, H, **kw)
    got, _ = one_target(ext, record(ext, t), padded(ext, t["kf_mp"]), t["Tcw"], dev_points(p), 60, intr, **kw)
    same(got, want, "th = 32")
    assert want["n_fused"] >= 10


@pytest.mark.parametrize("nt", [1, 2, X.FUSE_MAX_TARGETS])
def test_target_counts_equal_the_one_target_form_byte_for_byte(exts, nt):
    ext = exts[False]
    g = fc.load("chain")
    tgs, p = fc.targets(g), fc.points(g)
    n, intr = len(p["point_id"]), [float(v) for v in g["intr"]]
    d_pts = dev_points(p)
    recs = [record(ext, t) for t in tgs]
    mps = [padded(ext, t["kf_mp"]) for t in tgs]
    singles = [one_target(ext, recs[j], mps[j], tgs[j]["Tcw"], d_pts, n, intr, n_cap=16)[1] for j in range(3)]
    pick = [(5 * j + j // 3) % 3 for j in range(nt)]
    blocks = many_targets(ext, [recs[j] for j in pick], [mps[j] for j in pick], [tgs[j]["Tcw"] for j in pick], d_pts, n, intr, n_cap=16)
    for j, src in enumerate(pick):
        assert np.array_equal(blocks[j], singles[src]), (nt, j)
    assert len({s.tobytes() for s in singles}) == 3


# ---- one extracted scene, end to end ---------------------------------------------------------------------------------------
SCENE_N_NEW, SCENE_N_FUSED = 108, 85      # the reference run's counts (fuse_ref.c on the extracted records)
OWN_RADIUS = 2                            # SPFE_NMS_DIST / 2, see the scene test


def test_points_created_between_two_views_are_proposed_into_a_third_at_their_own_keypoints(ref):
    """Frames 2 and 4 of tools/track_scene (pans of 32 and 64 px) give new map points
    (spfe_create_map_points_pair_record_device); frame 3 (pan 48, 8) sees the same plane.  Every point created at keypoint k1
    of frame 2 is searched in frame 3 with that keypoint's descriptor: what is proposed is the point's own keypoint, frame 3's
    detection of the feature that lies one pan from k1.  The network pads with zeros and its receptive field (84 px) is most
    of this 128-row frame, so a detection near a border may move inside its cell from one pan to the next (the reference run
    has one such point in the second cell row, one pixel off in x and y; all others coincide).  What identifies the own
    keypoint whatever the detector did is the NMS: two keypoints of a frame are never within SPFE_NMS_DIST = 4 px of each
    other in both axes, so at most ONE keypoint of frame 3 lies within 2 px (both axes) of k1 - pan, and two points, created
    at keypoints of frame 2 more than 4 px apart, cannot claim the same one.  The test asserts that the proposed keypoint is
    that one.  The counts are the reference run's (fuse_ref.c on the same records): 108 points created, 85 proposed, 22
    without a candidate in the window, 1 too far."""
    import torch
    ext = SPExtractor(trk.NF, trk.H, trk.W, weights.synthetic(7, "trackable"), with_heat=False)
    try:
        world = ts.texture(21, *ts.world_size(trk.H, trk.W))
        views = []
        for k in (2, 4, 3):
            ox, oy = ts.offsets(k)
            d_img = dev(world[oy:oy + trk.H, ox:ox + trk.W][None].copy())
            d_rec = torch.zeros(ext.record_bytes(), dtype=torch.uint8, device="cuda")
            ext.wait_records(ext.extract_batch_device(d_img.data_ptr(), 1, d_rec.data_ptr()))
            torch.cuda.synchronize()
            fr = ext.view_record(d_rec.cpu().numpy())
            assert fr.status == 0 and fr.K >= trk.MIN_KEYPOINTS
            views.append((d_rec, fr, ts.pose(ox, oy), (ox, oy)))
        (d1, f1, T1, o1), (d2, f2, T2, _), (d3, f3, T3, o3) = views
        kmax = ext.layout.kmax
        d_mp1, d_mp2 = dev(np.full(kmax, -1, np.int32)), dev(np.full(kmax, -1, np.int32))
        d_tri = torch.zeros(ext.tri_out_bytes(), dtype=torch.uint8, device="cuda")
        d_T1, d_T2 = dev(T1.reshape(16)), dev(T2.reshape(16))
        ext.create_map_points_pair_record_device(d1.data_ptr(), d2.data_ptr(), d_mp1.data_ptr(), d_mp2.data_ptr(), d_T1.data_ptr(),
                                                 d_T2.data_ptr(), d_tri.data_ptr(), trk.INTR)
        torch.cuda.synchronize()
        tri = ext.decode_tri_out(d_tri.cpu().numpy(), kmax)
        n = tri["n_new"]
        assert n >= trk.MIN_KEYPOINTS // 2
        xyz = tri["new_xyz"]
        O1, O2 = -T1[:3, 3].astype(np.float64), -T2[:3, 3].astype(np.float64)
        d1n, d2n = xyz - O1, xyz - O2
        normal = 0.5 * (d1n / np.linalg.norm(d1n, axis=1, keepdims=True) + d2n / np.linalg.norm(d2n, axis=1, keepdims=True))
        dist = np.linalg.norm(d1n, axis=1)                                # one pyramid level: mfMinDistance == mfMaxDistance
        p = dict(point_id=(5000 + np.arange(n)).astype(np.int32), xyz=xyz.astype(np.float32), normal=normal.astype(np.float32),
                 dist_range=np.stack([dist, dist], 1).astype(np.float32), desc=np.ascontiguousarray(f1.descriptors[tri["new_k1"]], np.float32),
                 flags=np.ones(n, np.uint8))
        kf_mp = np.full(kmax, -1, np.int32)
        kf_mp[::9] = 77                                                   # some keypoints of the third view hold another point
        kf_mp[f3.K:] = -1
        got, _ = one_target(ext, d3, kf_mp, T3, dev_points(p), n, trk.INTR)
        want = fuse_ref.search(ref, f3.kp_xy, f3.occ_grid, f3.descriptors, kf_mp[:f3.K], T3, *[p[k] for k in fc.POINT_KEYS],
                               trk.INTR, trk.W, trk.H)
        same(got, want, "scene")
        print("scene: n_new", n, "n_fused", got["n_fused"], "reasons", np.bincount(got["reason"], minlength=10)[1:])
        pan = np.subtract(o3, o1)
        prop = got["fused_idx"]
        assert len(prop) >= 1
        own = f1.kp_xy[tri["new_k1"][prop]] - pan
        cheb = np.abs(f3.kp_xy[None, :f3.K] - own[:, None]).max(axis=2)   # [proposed, keypoints of frame 3]
        print("scene: offsets of the proposed keypoints from k1 - pan:", np.bincount(cheb[np.arange(len(prop)), got["kp_of_mp"][prop]].astype(int)))
        assert ((cheb <= OWN_RADIUS).sum(axis=1) <= 1).all()              # the NMS: the own keypoint is unique
        assert (cheb[np.arange(len(prop)), got["kp_of_mp"][prop]] <= OWN_RADIUS).all()   # and it is the one proposed
        assert len(set(got["kp_of_mp"][prop].tolist())) == len(prop)
        assert np.array_equal(got["holder"][prop], kf_mp[got["kp_of_mp"][prop]]) and (got["best_dist"][prop] <= np.float32(0.3)).all()
        assert (n, want["n_fused"], got["n_fused"]) == (SCENE_N_NEW, SCENE_N_FUSED, SCENE_N_FUSED)
    finally:
        ext.close()


# ---- refusals and the overflow decision --------------------------------------------------------------------------------------
def test_an_overflowed_record_is_searched_and_its_status_passed_through(exts, ref):
    """SPFE_STATUS_COV_OVERFLOW says that cov2 / cov2_inv are not valid; keypoints, grid and rows are complete and Fuse reads no
    covariance: the result is that of the clean record, and the block's status names the bit."""
    ext = exts[False]
    g = fc.load("held_best")
    t, p = fc.targets(g)[0], fc.points(g)
    n, intr = len(p["point_id"]), [float(v) for v in g["intr"]]
    clean, raw0 = one_target(ext, record(ext, t), padded(ext, t["kf_mp"]), t["Tcw"], dev_points(p), n, intr)
    over, raw1 = one_target(ext, record(ext, t, status=1), padded(ext, t["kf_mp"]), t["Tcw"], dev_points(p), n, intr)
    same(over, fc.run_ref(ref, g, 0), "overflowed")
    assert clean["status"] == 0 and over["status"] == 1 and over["n_fused"] == clean["n_fused"] > 0
    assert np.array_equal(raw0[12:], raw1[12:]) and np.array_equal(raw0[:8], raw1[:8])


def test_invalid_arguments_return_before_any_launch(exts):
    import torch
    ext = exts[False]
    g = fc.load("held_best")
    t, p = fc.targets(g)[0], fc.points(g)
    n, intr = len(p["point_id"]), [float(v) for v in g["intr"]]
    d_rec, d_mp, d_T, d_pts = record(ext, t), dev(padded(ext, t["kf_mp"])), dev(t["Tcw"].reshape(16)), dev_points(p)
    d_out = torch.full((2 * ext.fuse_out_bytes(8),), FILL, dtype=torch.uint8, device="cuda")
    q = lambda x: x.data_ptr()   # noqa: E731
    good = [q(d_rec), q(d_mp), q(d_T)] + point_ptrs(d_pts) + [n, q(d_out)]
    bad = []
    for i in list(range(9)) + [10]:                                        # every pointer
        a = list(good)
        a[i] = 0
        bad.append((a, {}))
    bad += [(good, dict(n_cap=n - 1)), (good, dict(n_cap=0)), (good, dict(n_cap=X.PROJ_MAX_POINTS + 1)), (good, dict(th=0.0)),
            (good, dict(th=float(X.PROJ_MAX_RADIUS) + 0.01)), (good, dict(th=float("nan")))]
    a = list(good)
    a[9] = -1
    bad.append((a, {}))
    a = list(good)
    a[9] = X.PROJ_MAX_POINTS + 1
    bad.append((a, dict(n_cap=X.PROJ_MAX_POINTS + 1)))
    for a, kw in bad:
        with pytest.raises(X.SpfeError, match="SPFE_EINVAL"):
            ext.fuse_record_device(*a, *intr, **kw)
    many = lambda recs, **kw: ext.fuse_targets_record_device(recs, *good[1:], *intr, **kw)   # noqa: E731
    for recs in ([], [q(d_rec)] * (X.FUSE_MAX_TARGETS + 1), [q(d_rec), 0]):
        with pytest.raises(X.SpfeError, match="SPFE_EINVAL"):
            many(recs)
    for kw in (dict(th=33.0), dict(n_cap=n - 1)):
        with pytest.raises(X.SpfeError, match="SPFE_EINVAL"):
            many([q(d_rec), q(d_rec)], **kw)
    with pytest.raises(X.SpfeError, match="SPFE_EINVAL"):                   # the host form: more points than the capacity
        big = X.PROJ_MAX_POINTS + 1
        ext.fuse_search(t["kp_xy"], t["occ"], t["kp_desc"], t["kf_mp"], t["Tcw"], np.zeros(big, np.int32), np.zeros((big, 3), np.float32),
                        np.zeros((big, 3), np.float32), np.zeros((big, 2), np.float32), np.zeros((big, 256), np.float32),
                        np.zeros(big, np.uint8), *intr)
    with pytest.raises(X.SpfeError, match="SPFE_EINVAL"):
        ext.fuse_search(t["kp_xy"], t["occ"], t["kp_desc"], t["kf_mp"], t["Tcw"], *[p[k] for k in fc.POINT_KEYS], *intr, th=40.0)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == FILL).all() and np.array_equal(d_mp.cpu().numpy(), padded(ext, t["kf_mp"]))
    ext.fuse_record_device(*good, *intr, th=float(X.PROJ_MAX_RADIUS), n_cap=8)          # the radius at the cap is served
    torch.cuda.synchronize()
    assert ext.decode_fuse_out(d_out.cpu().numpy(), 8)["n"] == n
