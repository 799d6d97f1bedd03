"""GPU: the covariance-weighted pose refinement (pose.hip) against its host reference tests/pose_ref/pose_ref.c — flags,
counts and iteration counts equal, pose within 1e-6 (the device's sin / cos in the exponential map) — in the host form,
the record form (real records; a record with more edges than the LDS holds) and the batch form; refused records."""
import glob
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "pose_ref"))
import pose_ref  # noqa: E402

from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import POSE_STATUS_COV_OVERFLOW, SPExtractor  # noqa: E402
from tools import track_scene as ts  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "pose_*.npz")))
SCHEDULES = (pose_ref.DUST_POST, pose_ref.OPTIMIZATION)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return pose_ref.build(tmp_path_factory.mktemp("pose_ref"))


def same(g, r, n=None):
    assert np.array_equal(g["iterations"], r["iterations"]), (g["iterations"], r["iterations"])
    assert g["n_good"] == r["n_good"], (g["n_good"], r["n_good"])
    assert np.array_equal(g["outlier"][:n] if n is not None else g["outlier"], r["outlier"])
    d = float(np.abs(g["Tcw"].astype(np.float64) - r["Tcw"]).max())
    assert d <= 1e-6, d


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_host_form_matches_reference(ref, path):
    g = np.load(path)
    ext = SPExtractor(100, 64, 96, weights.synthetic(7, "dense"), with_heat=False)
    for code in SCHEDULES:
        r = pose_ref.solve(ref, g["obs"], g["w"], g["pts"], g["Tcw_init"], g["intr"], code)
        k = ext.refine_pose(g["obs"], g["w"], g["pts"], g["Tcw_init"], *g["intr"], schedule=code)
        same(k, r)
        if len(g["obs"]) < 3:
            assert np.array_equal(k["Tcw"], g["Tcw_init"])     # echoed bit for bit
    ext.close()


def _record(ext, H, W, k):
    import torch
    world = ts.texture(21, *ts.world_size(H, W))
    img = torch.from_numpy(ts.frame(world, k, H, W)[None]).cuda()
    d_rec = torch.zeros(ext.record_bytes(), dtype=torch.uint8, device="cuda")
    t = ext.extract_batch_device(img.data_ptr(), 1, d_rec.data_ptr(), 0)
    ext.wait_records(t, 0)
    torch.cuda.synchronize()
    return d_rec


def _edges(rec, kmax, seed, frac=0.6, outliers=0.2):
    """map points for a fraction of the record's keypoints: back-projected at the true pose of frame 3, some displaced"""
    rng = np.random.default_rng(seed)
    K = rec.K
    mp_of_kp = np.full(kmax, -1, np.int32)
    sel = np.flatnonzero(rng.random(K) < frac)
    rng.shuffle(sel)
    mp_of_kp[sel] = np.arange(len(sel))
    T = ts.pose(*ts.offsets(3)).astype(np.float64)
    z = rng.uniform(3.0, 6.0, len(sel))
    xy = rec.kp_xy[sel].astype(np.float64)
    Xc = np.stack([(xy[:, 0] - ts.CX) / ts.FX * z, (xy[:, 1] - ts.CY) / ts.FY * z, z], 1)
    bad = rng.random(len(sel)) < outliers
    Xc[bad, :2] += rng.normal(0, 0.3, (bad.sum(), 2))
    pts = (Xc - T[:3, 3]).astype(np.float32)
    return mp_of_kp, pts


def _start_pose():
    T = ts.pose(*ts.offsets(3)).copy()
    T[0, 3] += 0.03
    T[1, 3] -= 0.02
    c, s = np.cos(0.01), np.sin(0.01)
    T[:2, :2] = np.array([[c, -s], [s, c]], np.float32)
    return T


def _check_record(ext, ref, d_rec, mp_of_kp, pts, T0, code):
    import torch
    rec = ext.view_record(d_rec.cpu().numpy())
    kmax = len(mp_of_kp)
    d_map = torch.from_numpy(mp_of_kp).cuda()
    d_pts = torch.from_numpy(pts).cuda()
    d_T = torch.from_numpy(T0.reshape(16)).cuda()
    d_out = torch.zeros(ext.pose_out_bytes(), dtype=torch.uint8, device="cuda")
    ext.refine_pose_record_device(d_rec.data_ptr(), d_map.data_ptr(), d_pts.data_ptr(), d_T.data_ptr(), d_out.data_ptr(),
                                  ts.FX, ts.FY, ts.CX, ts.CY, schedule=code)
    torch.cuda.synchronize()
    g = ext.decode_pose_out(d_out.cpu().numpy(), kmax)
    kp = np.flatnonzero(mp_of_kp[:rec.K] >= 0)                  # edge order: ascending keypoint index
    r = pose_ref.solve(ref, rec.kp_xy[kp], rec.cov2_inv[kp], pts[mp_of_kp[kp]], T0, (ts.FX, ts.FY, ts.CX, ts.CY), code)
    assert g["status"] == 0 and g["n_initial"] == len(kp)
    full = np.zeros(kmax, bool)
    full[kp] = r["outlier"]
    r = dict(r, outlier=full)
    same(g, r)
    return g, r


@pytest.mark.parametrize("code", SCHEDULES)
def test_record_form_on_real_records(ref, code):
    H, W, nf = 480, 752, 1000
    ext = SPExtractor(nf, H, W, weights.synthetic(7, "trackable"), with_heat=False)
    d_rec = _record(ext, H, W, 3)
    rec = ext.view_record(d_rec.cpu().numpy())
    assert rec.K > 500
    for seed in range(3):
        mp_of_kp, pts = _edges(rec, nf + 1, seed)
        g, _ = _check_record(ext, ref, d_rec, mp_of_kp, pts, _start_pose(), code)
        assert g["n_good"] >= 0.5 * g["n_initial"]
    ext.close()


@pytest.mark.parametrize("code", SCHEDULES)
def test_record_form_beyond_lds(ref, code):
    """8,000 features: the edge data of ~5,000 edges does not fit in LDS beside the per-edge state; it is read from global
    memory on every evaluation.  A sparse selection on the same handle takes the LDS path."""
    H, W, nf = 480, 752, 8000
    ext = SPExtractor(nf, H, W, weights.synthetic(7, "dense"), with_heat=False)
    d_rec = _record(ext, H, W, 3)
    rec = ext.view_record(d_rec.cpu().numpy())
    assert rec.K > 4000, rec.K
    mp_of_kp, pts = _edges(rec, nf + 1, 11, frac=0.95)
    assert (mp_of_kp >= 0).sum() > 3500
    _check_record(ext, ref, d_rec, mp_of_kp, pts, _start_pose(), code)
    mp_of_kp, pts = _edges(rec, nf + 1, 12, frac=0.05)
    _check_record(ext, ref, d_rec, mp_of_kp, pts, _start_pose(), code)
    ext.close()


def test_batch_form_equals_single_calls(ref):
    import torch
    H, W, nf, nb = 480, 752, 1000, 8
    ext = SPExtractor(nf, H, W, weights.synthetic(7, "trackable"), max_batch=nb, with_heat=False)
    world = ts.texture(21, *ts.world_size(H, W))
    imgs = torch.from_numpy(np.stack([ts.frame(world, k, H, W) for k in range(nb)])).cuda()
    rb, kmax, ob = ext.record_bytes(), nf + 1, ext.pose_out_bytes()
    d_recs = torch.zeros(nb * rb, dtype=torch.uint8, device="cuda")
    t = ext.extract_batch_device(imgs.data_ptr(), nb, d_recs.data_ptr(), 0)
    ext.wait_records(t, 0)
    torch.cuda.synchronize()
    host = d_recs.cpu().numpy()
    stride = 4096 * 3
    maps = np.full((nb, kmax), -1, np.int32)
    pts = np.zeros((nb, stride), np.float32)
    for f in range(nb):
        rec = ext.view_record(host[f * rb:(f + 1) * rb])
        m, p = _edges(rec, kmax, 100 + f)
        maps[f] = m
        pts[f, :p.size] = p.reshape(-1)
    Ts = np.stack([_start_pose().reshape(16)] * nb)
    d_maps, d_pts, d_T = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (maps, pts, Ts))
    for code in SCHEDULES:
        d_out = torch.zeros(nb * ob, dtype=torch.uint8, device="cuda")
        ext.refine_pose_batch_device(d_recs.data_ptr(), nb, d_maps.data_ptr(), d_pts.data_ptr(), stride, d_T.data_ptr(),
                                     d_out.data_ptr(), ts.FX, ts.FY, ts.CX, ts.CY, schedule=code)
        torch.cuda.synchronize()
        batch = d_out.cpu().numpy()
        for f in range(nb):
            one = torch.zeros(ob, dtype=torch.uint8, device="cuda")
            ext.refine_pose_record_device(d_recs.data_ptr() + f * rb, d_maps[f].data_ptr(), d_pts[f].data_ptr(),
                                          d_T[f].data_ptr(), one.data_ptr(), ts.FX, ts.FY, ts.CX, ts.CY, schedule=code)
            torch.cuda.synchronize()
            assert np.array_equal(batch[f * ob:(f + 1) * ob], one.cpu().numpy()), f
            assert ext.decode_pose_out(batch[f * ob:(f + 1) * ob], kmax)["n_initial"] > 100
    ext.close()


def test_covariance_overflow_record_is_refused():
    import torch
    H, W, nf = 480, 752, 1000
    ext = SPExtractor(nf, H, W, weights.synthetic(7, "trackable"), with_heat=False)
    d_rec = _record(ext, H, W, 3)
    rec = ext.view_record(d_rec.cpu().numpy())
    mp_of_kp, pts = _edges(rec, nf + 1, 0)
    off = ext.layout.off_hdr
    hdr = d_rec[off:off + 16].view(torch.int32)
    hdr[2] = hdr[2] | 1                                          # SPFE_STATUS_COV_OVERFLOW
    T0 = _start_pose()
    d_map, d_pts, d_T = torch.from_numpy(mp_of_kp).cuda(), torch.from_numpy(pts).cuda(), torch.from_numpy(T0.reshape(16)).cuda()
    d_out = torch.full((ext.pose_out_bytes(),), 0x55, dtype=torch.uint8, device="cuda")
    ext.refine_pose_record_device(d_rec.data_ptr(), d_map.data_ptr(), d_pts.data_ptr(), d_T.data_ptr(), d_out.data_ptr(),
                                  ts.FX, ts.FY, ts.CX, ts.CY)
    torch.cuda.synchronize()
    g = ext.decode_pose_out(d_out.cpu().numpy(), nf + 1)
    assert g["status"] == POSE_STATUS_COV_OVERFLOW
    assert g["n_initial"] == 0 and g["n_good"] == 0 and not g["iterations"].any() and not g["outlier"].any()
    assert np.array_equal(g["Tcw"], T0)
    ext.close()


# ---- boundaries, mixed batches, repeatability -------------------------------------------------------------------------
# Flags are compared for equality, so the inputs of the cases below are chosen the way the fixtures are: the first seed for
# which the host reference keeps every classified chi2 a relative 1e-5 away from its threshold (pose_ref's chi2_margin).
# The choice reads the reference only, never the kernel.

CHI2_MARGIN = 1e-5
INTR = (ts.FX, ts.FY, ts.CX, ts.CY)


def _edges_n(rec, kmax, seed, m, behind=0.0):
    """_edges with exactly m mapped keypoints; a fraction `behind` of the points is mirrored to negative depth"""
    rng = np.random.default_rng(seed)
    assert m <= rec.K
    mp_of_kp = np.full(kmax, -1, np.int32)
    sel = rng.permutation(rec.K)[:m]
    mp_of_kp[sel] = np.arange(m)
    T = ts.pose(*ts.offsets(3)).astype(np.float64)
    z = rng.uniform(3.0, 6.0, m)
    xy = rec.kp_xy[sel].astype(np.float64)
    Xc = np.stack([(xy[:, 0] - ts.CX) / ts.FX * z, (xy[:, 1] - ts.CY) / ts.FY * z, z], 1)
    bad = rng.random(m) < 0.2
    Xc[bad, :2] += rng.normal(0, 0.3, (bad.sum(), 2))
    Xc[rng.random(m) < behind, 2] *= -1.0
    return mp_of_kp, (Xc - T[:3, 3]).astype(np.float32)


def _ref_record(ref, rec, mp_of_kp, pts, T0, code, iterations=10, intr=INTR):
    """the host reference on a record's edges (ascending keypoint index), flags scattered to keypoints"""
    kp = np.flatnonzero(mp_of_kp[:rec.K] >= 0)
    if len(kp) == 0:
        return dict(Tcw=np.asarray(T0, np.float32).reshape(4, 4), outlier=np.zeros(len(mp_of_kp), bool),
                    iterations=np.zeros(4, np.int32), n_good=0, chi2_margin=np.inf, n=0)
    r = pose_ref.solve(ref, rec.kp_xy[kp], rec.cov2_inv[kp], pts[mp_of_kp[kp]], T0, intr, code, iterations=iterations)
    full = np.zeros(len(mp_of_kp), bool)
    full[kp] = r["outlier"]
    return dict(r, outlier=full, n=len(kp))


def _stable_edges(ref, rec, kmax, seed, m, T0, **kw):
    """the first of seed, seed + 1, ... whose edges keep every chi2 of the host reference away from the thresholds, under
    both schedules"""
    for s in range(seed, seed + 50):
        mp_of_kp, pts = _edges_n(rec, kmax, s, m, **kw)
        if all(_ref_record(ref, rec, mp_of_kp, pts, T0, code)["chi2_margin"] >= CHI2_MARGIN for code in SCHEDULES):
            return mp_of_kp, pts
    raise AssertionError("no stable selection")


def _run_record(ext, d_rec, mp_of_kp, pts, T0, code, iterations=10, intr=INTR):
    """one record-form call into a block pre-filled with 0x55 -> the raw block"""
    import torch
    d_map, d_pts = torch.from_numpy(mp_of_kp).cuda(), torch.from_numpy(np.ascontiguousarray(pts)).cuda()
    d_T = torch.from_numpy(np.ascontiguousarray(T0, np.float32).reshape(16)).cuda()
    d_out = torch.full((ext.pose_out_bytes(),), 0x55, dtype=torch.uint8, device="cuda")
    ext.refine_pose_record_device(d_rec.data_ptr(), d_map.data_ptr(), d_pts.data_ptr(), d_T.data_ptr(), d_out.data_ptr(),
                                  *intr, schedule=code, iterations=iterations)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


NB = 8


@pytest.fixture(scope="module")
def big():
    """An 8,000-feature handle (kmax 8001: fewer edges fit in LDS than the record has keypoints) with eight dense records."""
    import torch
    H, W, nf = 480, 752, 8000
    ext = SPExtractor(nf, H, W, weights.synthetic(7, "dense"), max_batch=NB, with_heat=False)
    world = ts.texture(21, *ts.world_size(H, W))
    imgs = torch.from_numpy(np.stack([ts.frame(world, k, H, W) for k in range(NB)])).cuda()
    rb = ext.record_bytes()
    d_recs = torch.zeros(NB * rb, dtype=torch.uint8, device="cuda")
    t = ext.extract_batch_device(imgs.data_ptr(), NB, d_recs.data_ptr(), 0)
    ext.wait_records(t, 0)
    torch.cuda.synchronize()
    host = d_recs.cpu().numpy()
    recs = [ext.view_record(host[f * rb:(f + 1) * rb]) for f in range(NB)]
    yield dict(ext=ext, d_recs=d_recs, recs=recs, rb=rb, kmax=nf + 1, cap=ext.pose_lds_edge_capacity())
    ext.close()


def test_lds_capacity_is_below_kmax_only_for_large_handles(big):
    """The boundary tests need a handle whose LDS holds fewer edges than it has keypoints; if the layout changes and the
    boundary moves out of reach, this fails instead of the boundary silently going untested."""
    assert 256 < big["cap"] < big["kmax"], (big["cap"], big["kmax"])
    assert min(r.K for r in big["recs"]) > big["cap"] + 256          # a record can supply more edges than fit
    small = SPExtractor(1000, 64, 96, weights.synthetic(7, "dense"), with_heat=False)
    assert small.pose_lds_edge_capacity() == 1001
    small.close()


@pytest.mark.parametrize("code", SCHEDULES)
@pytest.mark.parametrize("delta", (-1, 0, 1))
def test_record_form_at_the_lds_boundary(ref, big, code, delta):
    """cap - 1, cap (the last float of the LDS allocation is the z of the last edge) and cap + 1 edges (the first count
    read from global memory)."""
    ext, rec, n = big["ext"], big["recs"][3], big["cap"] + delta
    T0 = _start_pose()
    mp_of_kp, pts = _stable_edges(ref, rec, big["kmax"], 300 + delta, n, T0)
    d_rec = big["d_recs"][3 * big["rb"]:4 * big["rb"]]
    g = ext.decode_pose_out(_run_record(ext, d_rec, mp_of_kp, pts, T0, code), big["kmax"])
    r = _ref_record(ref, rec, mp_of_kp, pts, T0, code)
    assert g["status"] == 0 and g["n_initial"] == n == r["n"]
    same(g, r)
    assert 0.5 * n <= g["n_good"] < n


@pytest.mark.parametrize("iterations", (0, 1, 3))
def test_iterations_argument(ref, big, iterations):
    """iterations other than 10, host form (257 edges: thread 0 owns two) and record form.  With 0 nothing is optimised:
    the pose is the input through the quaternion form and back, and every edge is classified at it."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "pose_n257.npz"))
    ext = big["ext"]
    rec, d_rec = big["recs"][3], big["d_recs"][3 * big["rb"]:4 * big["rb"]]
    T0 = _start_pose()
    mp_of_kp, pts = _edges_n(rec, big["kmax"], 40, 700)
    for code in SCHEDULES:
        r = pose_ref.solve(ref, g["obs"], g["w"], g["pts"], g["Tcw_init"], g["intr"], code, iterations=iterations)
        k = ext.refine_pose(g["obs"], g["w"], g["pts"], g["Tcw_init"], *g["intr"], schedule=code, iterations=iterations)
        assert r["chi2_margin"] >= CHI2_MARGIN
        calls = 2 if code == pose_ref.DUST_POST else 4
        assert r["iterations"].tolist() == [iterations] * calls + [0] * (4 - calls)
        same(k, r)
        r = _ref_record(ref, rec, mp_of_kp, pts, T0, code, iterations=iterations)
        assert r["chi2_margin"] >= CHI2_MARGIN
        same(ext.decode_pose_out(_run_record(ext, d_rec, mp_of_kp, pts, T0, code, iterations=iterations), big["kmax"]), r)


def test_host_form_with_other_intrinsics(ref, big):
    """fx != fy, 1280 x 720, the principal point off centre; 300 edges."""
    intr = tuple(float(np.float32(v)) for v in (1050.0, 980.0, 700.5, 330.25))
    fx, fy, cx, cy = intr
    for seed in range(7, 57):
        rng = np.random.default_rng(seed)
        n = 300
        z = rng.uniform(2.0, 9.0, n)
        Pc = np.stack([(rng.uniform(10, 1270, n) - cx) / fx * z, (rng.uniform(10, 710, n) - cy) / fy * z, z], 1)
        a = 0.07
        Tt = np.eye(4)
        Tt[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        Tt[:3, 3] = (0.3, -0.2, 0.4)
        pts = ((Pc - Tt[:3, 3]) @ Tt[:3, :3]).astype(np.float32)
        obs = np.stack([Pc[:, 0] / z * fx + cx, Pc[:, 1] / z * fy + cy], 1) + rng.standard_normal((n, 2)) * 0.6
        m = rng.random(n) < 0.15
        obs[m] += rng.uniform(15, 60, (m.sum(), 2)) * rng.choice([-1, 1], (m.sum(), 2))
        w = np.repeat(rng.uniform(0.5, 2.0, (n, 1)), 2, 1).astype(np.float32)
        T0 = Tt.astype(np.float32)
        T0[:3, 3] += np.array([0.04, -0.03, 0.05], np.float32)
        rs = [pose_ref.solve(ref, obs, w, pts, T0, intr, code) for code in SCHEDULES]
        if all(r["chi2_margin"] >= CHI2_MARGIN for r in rs):
            break
    else:
        raise AssertionError("no stable scene")
    for code, r in zip(SCHEDULES, rs):
        assert 0.7 * n <= r["n_good"] < n and np.abs(r["pose64"] - Tt).max() < 1e-2    # the scene means something
        same(big["ext"].refine_pose(obs, w, pts, T0, *intr, schedule=code), r)
        e = pose_ref.solve(ref, obs, w, pts, T0, INTR, code)                          # and the intrinsics matter
        assert not np.array_equal(e["outlier"], r["outlier"])


def test_mixed_batch(ref, big):
    """One launch over frames that take every way out of the kernel — no edge, 2 edges (both echo the pose), 5 edges (one
    round), an LDS-path frame, a global-path frame, a refused record, another LDS-path frame, exactly cap edges — with
    n_frames below max_batch and equal to it.  Each frame writes its own block only: every block equals the single call's
    block byte for byte, and the guard blocks before and after (and the blocks of the frames not launched) keep their fill."""
    import torch
    ext, kmax, cap, rb, ob = big["ext"], big["kmax"], big["cap"], big["rb"], big["ext"].pose_out_bytes()
    counts = [0, 2, 5, 600, cap + 200, 900, 450, cap]
    REFUSED = 5
    d_recs = big["d_recs"].clone()
    off = REFUSED * rb + ext.layout.off_hdr
    hdr = d_recs[off:off + 16].view(torch.int32)
    hdr[2] = hdr[2] | 1                                          # SPFE_STATUS_COV_OVERFLOW
    stride = (kmax + 7) // 8 * 8 * 3
    maps = np.full((NB, kmax), -1, np.int32)
    pts = np.zeros((NB, stride), np.float32)
    Ts = np.zeros((NB, 16), np.float32)
    for f, m in enumerate(counts):
        T0 = _start_pose()
        T0[2, 3] += 0.004 * f                                    # a pose of its own per frame
        Ts[f] = T0.reshape(16)
        if m:
            mp, p = _stable_edges(ref, big["recs"][f], kmax, 500 + 10 * f, m, T0) if m >= 3 else \
                _edges_n(big["recs"][f], kmax, 500 + 10 * f, m)
            maps[f] = mp
            pts[f, :p.size] = p.reshape(-1)
    d_maps, d_pts, d_T = (torch.from_numpy(a).cuda() for a in (maps, pts, Ts))
    for code in SCHEDULES:
        singles = [_run_record(ext, d_recs[f * rb:(f + 1) * rb], maps[f], pts[f].reshape(-1, 3), Ts[f], code) for f in range(NB)]
        for nfr in (6, NB):
            d_out = torch.full(((NB + 2) * ob,), 0x55, dtype=torch.uint8, device="cuda")
            ext.refine_pose_batch_device(d_recs.data_ptr(), nfr, d_maps.data_ptr(), d_pts.data_ptr(), stride, d_T.data_ptr(),
                                         d_out.data_ptr() + ob, *INTR, schedule=code)
            torch.cuda.synchronize()
            out = d_out.cpu().numpy().reshape(NB + 2, ob)
            assert (out[0] == 0x55).all() and (out[nfr + 1:] == 0x55).all(), (code, nfr)
            for f in range(nfr):
                assert np.array_equal(out[1 + f], singles[f]), (code, nfr, f)
        for f, m in enumerate(counts):
            g = ext.decode_pose_out(singles[f], kmax)
            if f == REFUSED:
                assert g["status"] == POSE_STATUS_COV_OVERFLOW and g["n_initial"] == 0
            else:
                assert g["status"] == 0 and g["n_initial"] == m
            if f == REFUSED or m < 3:                            # echoed: the input pose bit for bit, nothing counted
                assert g["n_good"] == 0 and not g["iterations"].any() and not g["outlier"].any()
                assert np.array_equal(g["Tcw"].reshape(16), Ts[f])
            else:
                same(g, _ref_record(ref, big["recs"][f], maps[f], pts[f].reshape(-1, 3), Ts[f], code))
                assert g["iterations"][0] > 0


def test_repeatable_and_independent_of_the_previous_call(ref, big):
    """The same call twice gives the same bytes, and a 600-edge call right after a (cap + 1)-edge call on the same handle
    (per-edge state of a larger solve, the double buffer of partial sums left on either side) equals the same call on a
    fresh handle."""
    ext, kmax, rb = big["ext"], big["kmax"], big["rb"]
    rec, d_rec = big["recs"][2], big["d_recs"][2 * rb:3 * rb]
    T0 = _start_pose()
    large = _edges_n(rec, kmax, 71, big["cap"] + 1)
    small = _edges_n(rec, kmax, 72, 600)
    fresh = SPExtractor(kmax - 1, 480, 752, weights.synthetic(7, "dense"), with_heat=False)
    assert fresh.record_bytes() == rb and fresh.pose_out_bytes() == ext.pose_out_bytes()
    for code in SCHEDULES:
        a = _run_record(ext, d_rec, *large, T0, code)
        b = _run_record(ext, d_rec, *large, T0, code)
        assert np.array_equal(a, b)
        c = _run_record(ext, d_rec, *small, T0, code)
        d = _run_record(fresh, d_rec, *small, T0, code)
        assert np.array_equal(c, d)
        assert np.array_equal(c, _run_record(ext, d_rec, *small, T0, code))
        g = ext.decode_pose_out(c, kmax)
        assert g["n_initial"] == 600 and g["iterations"][0] > 0
    fresh.close()


@pytest.mark.parametrize("code", SCHEDULES)
def test_record_form_with_degenerate_edges(ref, code):
    """A third of the mapped points behind the camera and a tenth of the mapped keypoints with cov2_inv zeroed in the device
    record; the reference reads the values back from that record."""
    import torch
    H, W, nf = 480, 752, 1000
    ext = SPExtractor(nf, H, W, weights.synthetic(7, "trackable"), with_heat=False)
    d_rec = _record(ext, H, W, 3)
    rec0 = ext.view_record(d_rec.cpu().numpy())
    T0 = _start_pose()
    for seed in range(90, 140):
        mp_of_kp, pts = _edges_n(rec0, nf + 1, seed, 600, behind=1.0 / 3.0)
        kp = np.flatnonzero(mp_of_kp >= 0)
        zero = kp[np.random.default_rng(seed).permutation(len(kp))[:len(kp) // 10]]
        d_mod = d_rec.clone()
        cinv = d_mod[ext.layout.off_cinv:ext.layout.off_cinv + 8 * (nf + 1)].view(torch.float32).view(-1, 2)
        cinv[torch.from_numpy(zero).cuda()] = 0.0
        torch.cuda.synchronize()
        rec = ext.view_record(d_mod.cpu().numpy())
        assert not rec.cov2_inv[zero].any() and rec.cov2_inv[np.setdiff1d(kp, zero)].all()
        r = _ref_record(ref, rec, mp_of_kp, pts, T0, code)
        if r["chi2_margin"] >= CHI2_MARGIN:
            break
    else:
        raise AssertionError("no stable selection")
    Xc = pts[mp_of_kp[kp]].astype(np.float64) @ T0[:3, :3].astype(np.float64).T + T0[:3, 3]
    assert 150 <= (Xc[:, 2] < 0).sum() <= 250
    g = ext.decode_pose_out(_run_record(ext, d_mod, mp_of_kp, pts, T0, code), nf + 1)
    assert g["status"] == 0 and g["n_initial"] == 600
    same(g, r)
    ext.close()
