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
