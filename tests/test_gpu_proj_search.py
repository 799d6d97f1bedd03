"""GPU: the window search by projection (spfe_search_projection*: proj.hip) against its host reference
(tests/proj_ref/proj_ref.c — the same header, the same operations) — the host-array form on the fixtures of
tests/golden/make_golden_proj.py, the record and batch forms on extracted records (752x480 and a ragged small size, f32 and
bf16 networks, bf16 descriptor records).  Everything is compared for equality, proj_uv and view_cos bit for bit: the
arithmetic is shared and has no transcendental."""
import glob
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "proj_ref"))
import proj_ref  # noqa: E402

from sp_orb_slam_amd import extractor as X  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import SPExtractor, SpfeError  # noqa: E402
from tools import track_scene as ts  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "proj_*.npz")))
NAMES = [os.path.basename(p)[5:-4] for p in FIXTURES]
INTR = (ts.FX, ts.FY, ts.CX, ts.CY)
PRM = dict(th=1.0, th_dist=0.7, view_cos_limit=0.5, adaptive=True, c2_thresh=81.0)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return proj_ref.build(tmp_path_factory.mktemp("proj_ref"))


def same(got, want, what=""):
    for k in ("mp_of_kp", "kp_of_mp", "in_view"):
        assert np.array_equal(got[k], want[k]), (what, k)
    assert got["n_matches"] == want["n_matches"] and got["n_to_match"] == want["n_to_match"], what
    assert np.array_equal(got["proj_uv"].view(np.uint32), want["proj_uv"].view(np.uint32)), (what, "proj_uv bits")
    assert np.array_equal(got["view_cos"].view(np.uint32), want["view_cos"].view(np.uint32)), (what, "view_cos bits")


def test_host_form_on_the_fixtures(ref):
    blob = weights.synthetic(7, "dense")
    exts = {}
    try:
        for name, path in zip(NAMES, FIXTURES):
            g = np.load(path)
            H, W = int(g["H"]), int(g["W"])
            if (H, W) not in exts:
                exts[(H, W)] = SPExtractor(100, H, W, blob, with_heat=False)
            ext = exts[(H, W)]
            for j, run in enumerate(g["runs"]):
                kw = dict(mode=int(run[0]), th=run[1], th_dist=run[2], view_cos_limit=run[3], adaptive=bool(run[4]),
                          c2_thresh=run[5])
                want = proj_ref.search(ref, g["kp_xy"], g["occ"], g["kp_desc"], g["xyz"], g["normal"], g["desc"], g["flags"],
                                       g["mp_of_kp"], g["Tcw"], g["intr"], W, H, **kw)
                got = ext.search_projection(g["kp_xy"], g["occ"], g["kp_desc"], g["xyz"], g["normal"], g["desc"], g["flags"],
                                            g["mp_of_kp"], g["Tcw"], *g["intr"], **kw)
                same(got, want, (name, j))
                for k in ("mp_of_kp", "kp_of_mp", "in_view"):     # ... and so the independent f64 statement's
                    assert np.array_equal(got[k], g["r%d_%s" % (j, k)]), (name, j, k)
    finally:
        for e in exts.values():
            e.close()


def make_map(rec, n, seed, H, W, K_entry=0.15):
    """n map points for a record: most sit on its keypoints (random depth, pose and view angle; descriptor near the
    keypoint's), the rest anywhere (also outside the frame and behind the camera); some keypoints hold a point on entry."""
    rng = np.random.default_rng(seed)
    K = rec.K
    T = np.eye(4)
    a = rng.normal(0, 0.03, 3)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T[:3, :3] = np.linalg.qr(np.eye(3) + Kx)[0]
    T[:3, :3] *= np.sign(np.diag(T[:3, :3]))
    T[:3, 3] = rng.normal(0, 0.2, 3)
    T = T.astype(np.float32)
    T64 = T.astype(np.float64)
    on = rng.random(n) < 0.8 if K else np.zeros(n, bool)
    kk = rng.integers(0, max(K, 1), n)
    u = np.where(on, rec.kp_xy[kk, 0] if K else 0, rng.uniform(-60, W + 60, n)) + rng.normal(0, 1.2, n)
    v = np.where(on, rec.kp_xy[kk, 1] if K else 0, rng.uniform(-60, H + 60, n)) + rng.normal(0, 1.2, n)
    z = rng.uniform(1.5, 8, n) * np.where(rng.random(n) < 0.03, -1, 1)
    Pc = np.stack([(u - ts.CX) / ts.FX * z, (v - ts.CY) / ts.FY * z, z], 1)
    Pw = (Pc - T64[:3, 3]) @ T64[:3, :3]
    Ow = -T64[:3, :3].T @ T64[:3, 3]
    d = Pw - Ow
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = np.cross(d, rng.normal(size=(n, 3)))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    ang = np.arccos(rng.choice([0.9999, 0.9985, 0.9975, 0.9, 0.6, 0.51, 0.49, 0.1], n))
    nrm = np.cos(ang)[:, None] * d + np.sin(ang)[:, None] * p
    noise = rng.normal(size=(n, 256))
    noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    desc = noise.copy()
    if K:
        desc[on] = rec.descriptors[kk[on]] + rng.choice([0.2, 0.5, 0.68, 0.72, 0.9, 1.3], (int(on.sum()), 1)) * noise[on]
    flags = rng.choice(np.array([3, 3, 3, 1, 2, 0], np.uint8), n)
    mp = np.full(K, -1, np.int32)
    if K and n:
        held = rng.random(K) < K_entry
        mp[held] = rng.integers(0, n, int(held.sum()))
    return dict(xyz=Pw.astype(np.float32), normal=nrm.astype(np.float32), desc=desc.astype(np.float32), flags=flags,
                mp_of_kp=mp, Tcw=T)


def extract_record(ext, H, W, seed):
    import torch
    img = ts.texture(seed, H, W)
    d_img = torch.from_numpy(img[None].copy()).cuda()
    d_rec = torch.zeros(ext.record_bytes(), dtype=torch.uint8, device="cuda")
    t = ext.extract_batch_device(d_img.data_ptr(), 1, d_rec.data_ptr())
    ext.wait_records(t)
    torch.cuda.synchronize()
    return d_rec, ext.view_record(d_rec.cpu().numpy())


def device_search(ext, d_rec, m, n, kmax, guard=0, **kw):
    """spfe_search_projection_record_device on the first n points of map m -> decoded block + the updated mp_of_kp [kmax]"""
    import torch
    d = {k: torch.from_numpy(np.ascontiguousarray(m[k][:max(n, 1)] if len(m[k]) else np.zeros((1,) + m[k].shape[1:], m[k].dtype))).cuda()
         for k in ("xyz", "normal", "desc", "flags")}
    mp = np.full(kmax, -1, np.int32)
    mp[:len(m["mp_of_kp"])] = np.where(m["mp_of_kp"] < n, m["mp_of_kp"], -1)
    d_mp = torch.from_numpy(mp).cuda()
    d_T = torch.from_numpy(m["Tcw"].reshape(16)).cuda()
    d_out = torch.full((ext.proj_out_bytes() + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
    ext.search_projection_record_device(d_rec.data_ptr(), d["xyz"].data_ptr(), d["normal"].data_ptr(), d["desc"].data_ptr(),
                                        d["flags"].data_ptr(), n, d_mp.data_ptr(), d_T.data_ptr(), d_out.data_ptr() + guard,
                                        *INTR, **kw)
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    assert (raw[:guard] == 0xA5).all() and (raw[guard + ext.proj_out_bytes():] == 0xA5).all()
    g = ext.decode_proj_out(raw[guard:guard + ext.proj_out_bytes()])
    assert g["n"] == n
    g["mp_of_kp"] = d_mp.cpu().numpy()
    return g, mp


def ref_search(ref, rec, m, n, mp_entry, H, W, **kw):
    K = rec.K
    r = proj_ref.search(ref, rec.kp_xy, rec.occ_grid, rec.descriptors, m["xyz"][:n], m["normal"][:n], m["desc"][:n],
                        m["flags"][:n], mp_entry[:K], m["Tcw"], INTR, W, H, **kw)
    full = mp_entry.copy()
    full[:K] = r["mp_of_kp"]
    r["mp_of_kp"] = full           # entries at and beyond K are left alone
    return r


@pytest.mark.parametrize("H,W,nf,precision,desc_bf16", [(480, 752, 1000, "f32", False), (480, 752, 1000, "bf16", False),
                                                       (480, 752, 1000, "f32", True), (72, 104, 60, "f32", False),
                                                       (72, 104, 60, "bf16", True)])
def test_record_form_on_extracted_records(ref, H, W, nf, precision, desc_bf16):
    ext = SPExtractor(nf, H, W, weights.synthetic(7, "trackable"), with_heat=False, precision=precision, desc_bf16=desc_bf16)
    try:
        d_rec, rec = extract_record(ext, H, W, 21)
        assert rec.K > nf // 3
        kmax = nf + 1
        m = make_map(rec, 1500, 5, H, W)
        for kw in (dict(PRM, mode=X.PROJ_LOCAL_MAP), dict(PRM, mode=X.PROJ_LOCAL_MAP, th=5.0),
                   dict(PRM, mode=X.PROJ_LOCAL_MAP, th=5.0, adaptive=False), dict(PRM, mode=X.PROJ_LAST_FRAME, th=15.0),
                   dict(PRM, mode=X.PROJ_LAST_FRAME, th=30.0)):
            got, mp_entry = device_search(ext, d_rec, m, 1500, kmax, guard=4096, **kw)
            want = ref_search(ref, rec, m, 1500, mp_entry, H, W, **kw)
            same(got, want, kw)
            assert want["n_matches"] > 50 or H < 100
            again, _ = device_search(ext, d_rec, m, 1500, kmax, **kw)      # repeatable
            same(again, got, "second run")
    finally:
        ext.close()


def test_point_counts_and_radius_at_the_capacities(ref):
    H, W, nf = 480, 752, 1000
    ext = SPExtractor(nf, H, W, weights.synthetic(7, "trackable"), with_heat=False)
    try:
        d_rec, rec = extract_record(ext, H, W, 22)
        kmax = nf + 1
        m = make_map(rec, X.PROJ_MAX_POINTS, 6, H, W)
        kw = dict(PRM, mode=X.PROJ_LOCAL_MAP)
        for n in (0, 1, X.PROJ_MAX_POINTS - 1, X.PROJ_MAX_POINTS):
            got, mp_entry = device_search(ext, d_rec, m, n, kmax, guard=4096, **kw)
            same(got, ref_search(ref, rec, m, n, mp_entry, H, W, **kw), n)
        with pytest.raises(SpfeError, match="n_points"):
            device_search(ext, d_rec, m, X.PROJ_MAX_POINTS + 1, kmax, **kw)
        # the radius at the cap (LOCAL_MAP: 4 th = 32; LAST_FRAME: th = 32) and just above it
        for kw in (dict(PRM, mode=X.PROJ_LOCAL_MAP, th=8.0), dict(PRM, mode=X.PROJ_LAST_FRAME, th=32.0)):
            got, mp_entry = device_search(ext, d_rec, m, 2000, kmax, guard=4096, **kw)
            same(got, ref_search(ref, rec, m, 2000, mp_entry, H, W, **kw), kw)
        for kw in (dict(PRM, mode=X.PROJ_LOCAL_MAP, th=8.001), dict(PRM, mode=X.PROJ_LAST_FRAME, th=32.001),
                   dict(PRM, mode=X.PROJ_LAST_FRAME, th=0.0), dict(PRM, mode=7)):
            with pytest.raises(SpfeError):
                device_search(ext, d_rec, m, 10, kmax, **kw)
    finally:
        ext.close()


def test_mixed_batch_of_eight_frames_with_guards(ref):
    import torch
    H, W, nf, B, stride = 72, 104, 60, 8, 400
    ext = SPExtractor(nf, H, W, weights.synthetic(7, "trackable"), max_batch=B, with_heat=False)
    try:
        kmax, rb, ob = nf + 1, ext.record_bytes(), ext.proj_out_bytes()
        imgs = np.stack([ts.texture(30 + f, H, W) for f in range(B)])
        imgs[3] = 0                                             # a frame without keypoints
        d_img = torch.from_numpy(imgs).cuda()
        d_recs = torch.zeros(B * rb, dtype=torch.uint8, device="cuda")
        ext.wait_records(ext.extract_batch_device(d_img.data_ptr(), B, d_recs.data_ptr()))
        torch.cuda.synchronize()
        recs = [ext.view_record(d_recs[f * rb:(f + 1) * rb].cpu().numpy()) for f in range(B)]
        assert recs[3].K == 0
        counts = np.array([400, 0, 1, 399, 250, 37, 400, 128], np.int32)
        maps = [make_map(recs[f], stride, 40 + f, H, W) for f in range(B)]
        mp = np.full((B, kmax), -1, np.int32)
        for f in range(B):
            e = maps[f]["mp_of_kp"]
            mp[f, :len(e)] = np.where(e < counts[f], e, -1)
        cat = {k: torch.from_numpy(np.concatenate([m_[k] for m_ in maps])).cuda() for k in ("xyz", "normal", "desc", "flags")}
        d_T = torch.from_numpy(np.stack([m_["Tcw"].reshape(16) for m_ in maps])).cuda()
        for kw in (dict(PRM, mode=X.PROJ_LOCAL_MAP, th=5.0), dict(PRM, mode=X.PROJ_LAST_FRAME, th=15.0)):
            d_mp = torch.from_numpy(mp.copy()).cuda()
            d_n = torch.from_numpy(counts).cuda()
            d_out = torch.full((B * ob,), 0xA5, dtype=torch.uint8, device="cuda")
            ext.search_projection_batch_device(d_recs.data_ptr(), B, cat["xyz"].data_ptr(), cat["normal"].data_ptr(),
                                               cat["desc"].data_ptr(), cat["flags"].data_ptr(), d_n.data_ptr(), stride,
                                               d_mp.data_ptr(), d_T.data_ptr(), d_out.data_ptr(), *INTR, **kw)
            torch.cuda.synchronize()
            raw, got_mp = d_out.cpu().numpy().reshape(B, ob), d_mp.cpu().numpy()
            for f in range(B):
                n = int(counts[f])
                g = ext.decode_proj_out(raw[f])
                assert g["n"] == n
                g["mp_of_kp"] = got_mp[f]
                same(g, ref_search(ref, recs[f], maps[f], n, mp[f], H, W, **kw), (f, kw))
                # the block's unused regions are guards: nothing beyond the frame's own n entries is written
                for off, size in ((X.PROJ_OFF_KP, 4), (X.PROJ_OFF_UV, 8), (X.PROJ_OFF_COS, 4), (X.PROJ_OFF_VIEW, 1)):
                    assert (raw[f, off + size * n:off + size * X.PROJ_MAX_POINTS] == 0xA5).all(), (f, off)
                assert (raw[f, 12:X.PROJ_OFF_KP] == 0xA5).all() and (raw[f, X.PROJ_OFF_VIEW + X.PROJ_MAX_POINTS:] == 0xA5).all()
    finally:
        ext.close()


def test_long_dependency_chain(ref):
    """The domino of the chain fixture at the size of a frame: 1000 keypoints on a snake through the 752x480 grid, 1000
    points of which each finds its best keypoint taken by its predecessor — the fixed point needs as many rounds as there
    are points, and the answer is the sequential one."""
    H, W = 480, 752
    rng = np.random.default_rng(3)
    hc, wc, K = H // 8, W // 8, 1000
    cells = [(ix if iy % 2 == 0 else wc - 1 - ix, iy) for iy in range(hc) for ix in range(wc)][:K]
    base = rng.normal(size=256)
    base /= np.linalg.norm(base)
    e = rng.normal(size=(K, 256))
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    occ = np.full((hc, wc), -1, np.int16)
    kp = np.zeros((K, 2), np.float32)
    for j, (ix, iy) in enumerate(cells):
        occ[iy, ix] = j
        kp[j] = (8 * ix + 3, 8 * iy + 4)
    kd = (base + 0.25 * e).astype(np.float32)
    desc = np.concatenate([[base + 0.25 * e[0] + 0.05 * e[1]], base + 0.25 * (0.7 * e[:-1] + 0.3 * e[1:])]).astype(np.float32)
    uv = np.concatenate([kp[:1], kp[:-1]]) + rng.uniform(-0.8, 0.8, (K, 2))
    z = rng.uniform(2, 6, K)
    xyz = np.stack([(uv[:, 0] - ts.CX) / ts.FX * z, (uv[:, 1] - ts.CY) / ts.FY * z, z], 1).astype(np.float32)
    nrm = xyz / np.linalg.norm(xyz, axis=1, keepdims=True)
    c, s_ = 0.9, np.sqrt(1 - 0.81)
    perp = np.cross(nrm, [0.3, -0.5, 0.8])
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    nrm = (c * nrm + s_ * perp).astype(np.float32)
    flags = np.full(K, 3, np.uint8)
    mp = np.full(K, -1, np.int32)
    T = np.eye(4, dtype=np.float32)
    kw = dict(PRM, mode=X.PROJ_LOCAL_MAP, th=5.0)
    want = proj_ref.search(ref, kp, occ, kd, xyz, nrm, desc, flags, mp, T, INTR, W, H, **kw)
    assert want["n_matches"] == K and np.array_equal(want["kp_of_mp"], np.arange(K))
    ext = SPExtractor(K - 1, H, W, weights.synthetic(7, "dense"), with_heat=False)
    try:
        got = ext.search_projection(kp, occ, kd, xyz, nrm, desc, flags, mp, T, *INTR, **kw)
        same(got, want, "chain")
    finally:
        ext.close()
