"""GPU: the loop closer's fusion step on resident keyframe records (spfe_loop_fuse_search, spfe_loop_fuse_record_device,
spfe_loop_fuse_targets_record_device, spfe_loop_corrected_poses_device: loopfuse.hip) against the host reference
tests/loopfuse_ref/loopfuse_ref.c, which shares include/spfe_loopfuse_math.h with the kernels: every output, best_dist
included, bit for bit — on the fixtures tests/golden/loopfuse_*.npz laid out as records, with f32 and with bf16 descriptor
rows; the targets form against the one-target form byte for byte; the boundary shapes of the point count (around the strip
of SPFE_LOOPFUSE_STRIP points a workgroup serves), of the keypoint count (around the 16-byte reads of the id scan, at the
largest record, on both sides of 48 KB of staged holders and at the int16 grid's limit) and of the target count; the
largest window; a NaN similarity; one extracted scene against the mapper's fuse search without its gate; the corrected poses
against the host function; the chain of the two calls on one stream; the refusals and the decision on overflowed records."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "loopfuse_ref"))
sys.path.insert(0, os.path.join(ROOT, "tests", "track_ref"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import loopfuse_cases as lc  # noqa: E402
import loopfuse_ref  # noqa: E402
import test_gpu_fuse as tgf  # noqa: E402  (its record / point helpers and its scene)
import track_cases as trk  # noqa: E402

from sp_orb_slam_amd import extractor as X  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import SPExtractor  # noqa: E402
from tools import track_scene as ts  # noqa: E402

pytestmark = pytest.mark.gpu
H, W, NF = 64, 96, 100          # the fixtures' frame; kmax = 101 > 65 keypoints
FILL = tgf.FILL
S = X.LOOPFUSE_STRIP
dev, record, padded, dev_points, point_ptrs, same, unwritten = (tgf.dev, tgf.record, tgf.padded, tgf.dev_points, tgf.point_ptrs,
                                                                tgf.same, tgf.unwritten)
INTR = (ts.FX / 4, ts.FY / 4, 47.5, 31.25)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return loopfuse_ref.build(tmp_path_factory.mktemp("loopfuse_ref"))


@pytest.fixture(scope="module")
def exts():
    blob = weights.synthetic(7, "trackable")
    e = {False: SPExtractor(NF, H, W, blob, with_heat=False), True: SPExtractor(NF, H, W, blob, with_heat=False, desc_bf16=True)}
    yield e
    for x in e.values():
        x.close()


def scw_of(Tcw, s):
    """[s R | s t] of a pose, f32"""
    out = np.eye(4)
    out[:3, :] = s * np.asarray(Tcw, np.float64)[:3, :]
    return out.astype(np.float32)


def one_target(ext, d_rec, kf_mp, Scw, d_pts, n, intr, n_cap=None, **kw):
    """spfe_loop_fuse_record_device -> (decoded block, raw block); checks that kf_mp_of_kp is left alone"""
    import torch
    cap = max(n, 1) if n_cap is None else n_cap
    d_mp, d_S = dev(kf_mp), dev(np.asarray(Scw, np.float32).reshape(16))
    d_out = torch.full((ext.fuse_out_bytes(cap),), FILL, dtype=torch.uint8, device="cuda")
    ext.loop_fuse_record_device(d_rec.data_ptr(), d_mp.data_ptr(), d_S.data_ptr(), *point_ptrs(d_pts), n, d_out.data_ptr(), *intr,
                                n_cap=cap, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(d_mp.cpu().numpy(), kf_mp)
    raw = d_out.cpu().numpy()
    return ext.decode_fuse_out(raw, cap), raw


def many_targets(ext, d_recs, kf_mps, Scws, d_pts, n, intr, n_cap=None, d_S=None, **kw):
    """spfe_loop_fuse_targets_record_device -> raw blocks [n_targets][out_bytes]; d_S: the similarities already on the device"""
    import torch
    cap = max(n, 1) if n_cap is None else n_cap
    nt, ob = len(d_recs), ext.fuse_out_bytes(cap)
    mp = np.stack(kf_mps)
    d_mp = dev(mp)
    if d_S is None:
        d_S = dev(np.stack([np.asarray(T, np.float32).reshape(16) for T in Scws]))
    d_out = torch.full((nt * ob,), FILL, dtype=torch.uint8, device="cuda")
    ext.loop_fuse_targets_record_device([r.data_ptr() for r in d_recs], d_mp.data_ptr(), d_S.data_ptr(), *point_ptrs(d_pts), n,
                                        d_out.data_ptr(), *intr, n_cap=cap, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(d_mp.cpu().numpy(), mp)
    return d_out.cpu().numpy().reshape(nt, ob)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", lc.NAMES)
def test_all_three_forms_equal_the_host_reference_bit_for_bit(exts, ref, name, bf16):
    g = lc.load(name)
    assert (int(g["H"]), int(g["W"])) == (H, W)
    ext = exts[bf16]
    tgs, p = lc.targets(g), lc.points(g)
    n, intr = len(p["point_id"]), [float(v) for v in g["intr"]]
    d_pts = dev_points(p)
    recs = [record(ext, t) for t in tgs]
    mps = [padded(ext, t["kf_mp"]) for t in tgs]
    raws = []
    for j, t in enumerate(tgs):
        want = lc.run_ref(ref, g, j)                                      # (the fixtures' rows are bf16 values: both see the same numbers)
        assert lc.differences(g, j, want) == []
        got, raw = one_target(ext, recs[j], mps[j], t["Scw"], d_pts, n, intr)
        same(got, want, (name, j, "record form"))
        assert got["n"] == n and got["status"] == 0
        unwritten(ext, raw, n, got["n_fused"], max(n, 1))
        raws.append(raw)
        if not bf16:
            host = ext.loop_fuse_search(t["kp_xy"], t["occ"], t["kp_desc"], t["kf_mp"], t["Scw"], *[p[k] for k in lc.POINT_KEYS], *intr)
            same(host, want, (name, j, "host form"))
    blocks = many_targets(ext, recs, mps, [t["Scw"] for t in tgs], d_pts, n, intr)
    for j in range(len(tgs)):
        assert np.array_equal(blocks[j], raws[j]), (name, j, "targets form")


def big_target(seed=11, K=65, s=3.0):
    t = tgf.big_target(seed, K)
    t["Scw"] = scw_of(t["Tcw"], s)
    return t


def points_on(t, n, seed, intr):
    """tgf.points_on with descriptor distances about TH_HIGH instead of TH_LOW"""
    p = tgf.points_on(t, n, seed, intr)
    rng = np.random.default_rng(seed + 1000)
    k = rng.integers(0, len(t["kp_xy"]), n)
    noise = rng.normal(size=(n, 256))
    noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    far = rng.random(n) < 0.5                                             # half of the points get a row near ANOTHER keypoint's
    p["desc"] = np.where(far[:, None], t["kp_desc"][k] + rng.choice([0.2, 0.69, 0.71], (n, 1)) * noise,
                         p["desc"] + rng.choice([0.0, 0.4, 0.7], (n, 1)) * noise).astype(np.float32)
    return p


def ref_run(ref, t, p, n, K, intr, W_=W, H_=H, **kw):
    return loopfuse_ref.search(ref, t["kp_xy"][:K], t["occ"], t["kp_desc"][:K], t["kf_mp"][:K], t["Scw"],
                               *[p[k][:n] for k in lc.POINT_KEYS], intr, W_, H_, **kw)


@pytest.mark.parametrize("n", [0, 1, S - 1, S, S + 1, 2 * S + 1, X.PROJ_MAX_POINTS - 5, X.PROJ_MAX_POINTS])
def test_point_counts_around_the_strip_and_at_the_capacity(exts, ref, n):
    """0 and 1 points, one point less than a strip, a strip, one more (a second workgroup with one point), one more than two
    strips, and SPFE_PROJ_MAX_POINTS = 8192.  The block is laid out over a capacity above n; no capacity lies above 8192, so
    8192 points run at n_cap = n and 8187 under n_cap = 8192."""
    ext = exts[False]
    t = big_target()
    p = points_on(t, max(n, 8), 12, INTR)
    p["flags"][2] = 1
    t["kf_mp"][[3, 9]] = (p["point_id"][2], 77)                           # point 2 is in the keyframe; a holder
    want = ref_run(ref, t, p, n, 65, INTR)
    cap = min(n + 5, X.PROJ_MAX_POINTS)                                   # a capacity above n: the layout is the capacity's
    got, raw = one_target(ext, record(ext, t), padded(ext, t["kf_mp"]), t["Scw"], dev_points(p, n), n, INTR, n_cap=max(cap, 1))
    same(got, want, n)
    assert got["n"] == n
    unwritten(ext, raw, n, got["n_fused"], max(cap, 1))
    if n >= 3:
        assert want["reason"][2] == loopfuse_ref.SKIP_IN_KF
    if n >= S - 1:
        assert want["n_fused"] >= 5 and want["reason"][n - 1] != 0
    if n == X.PROJ_MAX_POINTS:
        print("reasons at the capacity:", np.bincount(want["reason"], minlength=10)[1:])
        assert (np.bincount(want["reason"], minlength=10)[1:] > 0).sum() >= 8 and want["n_fused"] > 1000


@pytest.mark.parametrize("K", [0, 61, 62, 63, 64, 65])
def test_keypoint_counts_around_the_id_scans_reads(exts, ref, K):
    """The ids of points 0 .. 4 are held by keypoints 60 .. 64: the last entries a scan of 61 .. 65 keypoints reads — through a
    16-byte read (K a multiple of four) or through the tail of up to three entries behind it.  Entries at and beyond K are
    ignored, in the holder array as in the record."""
    ext = exts[False]
    t = big_target()
    p = points_on(t, 40, 13, INTR)
    p["flags"][:5] = 1
    t["kf_mp"][[60, 61, 62, 63, 64]] = p["point_id"][:5]
    want = ref_run(ref, t, p, 40, K, INTR)
    assert [int(r == loopfuse_ref.SKIP_IN_KF) for r in want["reason"][:5]] == [int(K > 60 + i) for i in range(5)]
    got, _ = one_target(ext, record(ext, t, K=K), padded(ext, t["kf_mp"], fill=int(p["point_id"][7])), t["Scw"], dev_points(p), 40, INTR)
    same(got, want, K)                                                     # (the padding beyond the keypoints names point 7: ignored)
    assert want["reason"][7] != loopfuse_ref.SKIP_IN_KF
    if K == 0:
        assert want["n_fused"] == 0 and loopfuse_ref.NO_CANDIDATE in want["reason"]


def test_the_largest_window_takes_two_rounds_of_cells(exts, ref):
    """th = SPFE_PROJ_MAX_RADIUS: up to 11 x 11 cells, more than the 64 a wavefront tests at once; every keypoint of the window
    is a candidate."""
    ext = exts[False]
    t = big_target()
    p = points_on(t, 60, 14, INTR)
    kw = dict(th=float(X.PROJ_MAX_RADIUS))
    want = ref_run(ref, t, p, 60, 65, INTR, **kw)
    got, _ = one_target(ext, record(ext, t), padded(ext, t["kf_mp"]), t["Scw"], dev_points(p), 60, INTR, **kw)
    same(got, want, "th = 32")
    assert want["n_fused"] >= 10


def test_a_nan_similarity_refuses_every_searchable_point_as_outside(exts, ref):
    ext = exts[False]
    t = big_target()
    p = points_on(t, 70, 16, INTR)
    for bad in (np.full((4, 4), np.nan, np.float32), np.where(np.eye(4) > 0, np.nan, t["Scw"]).astype(np.float32)):
        t["Scw"] = bad
        want = ref_run(ref, t, p, 70, 65, INTR)
        got, _ = one_target(ext, record(ext, t), padded(ext, t["kf_mp"]), bad, dev_points(p), 70, INTR)
        same(got, want, "NaN Scw")
        ok = (p["flags"] & 1) == 1
        assert (want["reason"][ok] == loopfuse_ref.OUTSIDE).all() and (want["reason"][~ok] == loopfuse_ref.SKIP_BAD).all()


@pytest.mark.parametrize("nt", [1, 2, X.FUSE_MAX_TARGETS])
def test_target_counts_equal_the_one_target_form_byte_for_byte(exts, nt):
    ext = exts[False]
    g = lc.load("chain")
    tgs, p = lc.targets(g), lc.points(g)
    n, intr = len(p["point_id"]), [float(v) for v in g["intr"]]
    d_pts = dev_points(p)
    recs = [record(ext, t) for t in tgs]
    mps = [padded(ext, t["kf_mp"]) for t in tgs]
    singles = [one_target(ext, recs[j], mps[j], tgs[j]["Scw"], d_pts, n, intr, n_cap=16)[1] for j in range(3)]
    pick = [(5 * j + j // 3) % 3 for j in range(nt)]
    blocks = many_targets(ext, [recs[j] for j in pick], [mps[j] for j in pick], [tgs[j]["Scw"] for j in pick], d_pts, n, intr, n_cap=16)
    for j, src in enumerate(pick):
        assert np.array_equal(blocks[j], singles[src]), (nt, j)
    assert len({s.tobytes() for s in singles}) == 3


# ---- large keypoint counts ---------------------------------------------------------------------------------------------------
class TestLargeTargets:
    """A 1024 x 2048 frame has 32768 grid cells: one keypoint per cell up to the int16 grid's 32767.  The record form stages
    kmax = 10001 holders (40,004 bytes: inside the default 48 KB of dynamic LDS); the host-array form stages K of them and
    raises the limit beyond 12,288."""
    H, W = 1024, 2048
    INTR = (600.0, 600.0, 1024.0, 512.0)

    @pytest.fixture(scope="class")
    def ext(self):
        e = SPExtractor(10000, self.H, self.W, weights.synthetic(7, "trackable"), with_heat=False)
        yield e
        e.close()

    @pytest.fixture(scope="class")
    def scene(self):
        """32767 keypoints, one per cell in row-major order, and 300 points on keypoints all over the index range — the first
        ones on the last keypoints a given K keeps"""
        rng = np.random.default_rng(31)
        K, hc, wc = 32767, self.H // 8, self.W // 8
        occ = np.full((hc, wc), -1, np.int16)
        occ.reshape(-1)[:K] = np.arange(K, dtype=np.int16)
        cell = np.arange(K)
        kp = np.stack([8 * (cell % wc) + rng.integers(2, 14, K) * 0.5, 8 * (cell // wc) + rng.integers(2, 14, K) * 0.5], 1).astype(np.float32)
        desc = rng.standard_normal((K, 256), dtype=np.float32)
        desc /= np.linalg.norm(desc, axis=1, keepdims=True)
        T = np.eye(4, dtype=np.float32)
        T[:3, 3] = (0.05, -0.03, 0.1)
        t = dict(kp_xy=kp, occ=occ, kp_desc=desc, kf_mp=np.full(K, -1, np.int32), Tcw=T, Scw=scw_of(T, 3.0))
        n = 300
        ks = np.concatenate([[10000, 9999, 12286, 12288, 32766, 32765], rng.integers(0, K, n - 6)])
        fx, fy, cx, cy = self.INTR
        uv = kp[ks] + rng.normal(0, 1.2, (n, 2))
        z = rng.uniform(2, 6, n)
        Pc = np.stack([(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, z], 1)
        P = Pc - T[:3, 3].astype(np.float64)
        dist = np.linalg.norm(Pc, axis=1)
        noise = rng.normal(size=(n, 256))
        noise /= np.linalg.norm(noise, axis=1, keepdims=True)
        p = dict(point_id=(1000 + np.arange(n)).astype(np.int32), xyz=P.astype(np.float32), normal=(Pc / dist[:, None]).astype(np.float32),
                 dist_range=np.stack([0.8 * dist, 1.2 * dist], 1).astype(np.float32),
                 desc=(desc[ks] + np.where(np.arange(n) < 9, 0.1, rng.choice([0.1, 0.5, 0.69, 0.71], n))[:, None] * noise).astype(np.float32),
                 flags=np.ones(n, np.uint8))
        return t, p, ks

    def holders(self, t, p, K):
        """the ids of points 6 and 7 sit in the last two entries a scan of K keypoints reads, that of point 8 just beyond"""
        mp = t["kf_mp"].copy()
        mp[K - 1], mp[K - 2] = p["point_id"][6], p["point_id"][7]
        if K < len(mp):
            mp[K] = p["point_id"][8]
        return mp

    def test_record_form_at_10001_keypoints(self, ext, ref, scene):
        t, p, ks = scene
        K = 10001
        assert ext.layout.kmax == K
        sub = dict(t, kp_xy=t["kp_xy"][:K], kp_desc=t["kp_desc"][:K], kf_mp=self.holders(t, p, K)[:K])
        sub["occ"] = np.where(t["occ"] < K, t["occ"], -1).astype(np.int16)
        n = len(p["point_id"])
        want = ref_run(ref, sub, p, n, K, self.INTR, W_=self.W, H_=self.H)
        got, raw = one_target(ext, record(ext, sub), sub["kf_mp"], t["Scw"], dev_points(p), n, self.INTR)
        same(got, want, "K = 10001")
        assert want["reason"][0] == loopfuse_ref.PROPOSED and want["kp_of_mp"][0] == 10000       # the last keypoint is found
        assert (want["reason"][[6, 7]] == loopfuse_ref.SKIP_IN_KF).all() and want["reason"][8] != loopfuse_ref.SKIP_IN_KF

    @pytest.mark.parametrize("K", [12287, 12289, 32767])
    def test_host_form_on_both_sides_of_48_kb_of_staged_holders_and_at_the_grid_limit(self, ext, ref, scene, K):
        t, p, ks = scene
        mp = self.holders(t, p, K)
        sub = dict(t, kf_mp=mp)
        sub["occ"] = np.where(t["occ"] < K, t["occ"], -1).astype(np.int16)
        n = len(p["point_id"])
        want = ref_run(ref, sub, p, n, K, self.INTR, W_=self.W, H_=self.H)
        got = ext.loop_fuse_search(t["kp_xy"][:K], sub["occ"], t["kp_desc"][:K], mp[:K], t["Scw"], *[p[k] for k in lc.POINT_KEYS], *self.INTR)
        same(got, want, K)
        assert (want["reason"][[6, 7]] == loopfuse_ref.SKIP_IN_KF).all() and want["reason"][8] != loopfuse_ref.SKIP_IN_KF
        assert want["n_fused"] >= 20
        near_top = want["kp_of_mp"][want["reason"] == loopfuse_ref.PROPOSED].max()
        assert near_top == {12287: 12286, 12289: 12288, 32767: 32766}[K]                        # a proposal at the last keypoint


# ---- one extracted scene against the mapper's fuse search without its gate ---------------------------------------------------
def test_scene_with_a_doubled_pose_equals_the_fuse_search_without_its_gate():
    """The three extracted views of test_gpu_fuse's scene; their poses are pure pans (R = I), so Scw = 2 Tcw is exact in f32 and
    its normalisation gives Tcw back exactly.  With chi2 = 1e9 (every keypoint of the window passes) and the same th and th_dist
    the mapper's search differs only in best = 256 for FLT_MAX, which no distance between finite rows of unit length reaches: the
    two blocks must be equal byte for byte, into each of the three views."""
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
            views.append((d_rec, fr, ts.pose(ox, oy)))
        (d1, f1, T1), (d2, f2, T2), _ = views
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
        dn = xyz - (-T1[:3, 3].astype(np.float64))
        dist = np.linalg.norm(dn, axis=1)
        p = dict(point_id=(5000 + np.arange(n)).astype(np.int32), xyz=xyz.astype(np.float32), normal=(dn / dist[:, None]).astype(np.float32),
                 dist_range=np.stack([0.9 * dist, 1.1 * dist], 1).astype(np.float32),
                 desc=np.ascontiguousarray(f1.descriptors[tri["new_k1"]], np.float32), flags=np.ones(n, np.uint8))
        d_pts = dev_points(p)
        total = 0
        for d_rec, fr, T in views:
            assert np.array_equal(T[:3, :3], np.eye(3, dtype=T.dtype))
            kf_mp = np.full(kmax, -1, np.int32)
            kf_mp[::9] = 77
            kf_mp[fr.K:] = -1
            kw = dict(th=4.0, th_dist=0.7)
            _, mapper = tgf.one_target(ext, d_rec, kf_mp, T, d_pts, n, trk.INTR, chi2=1e9, **kw)
            got, loop = one_target(ext, d_rec, kf_mp, scw_of(T, 2.0), d_pts, n, trk.INTR, **kw)
            assert np.array_equal(loop, mapper)
            total += got["n_fused"]
        print("scene: points", n, "proposed into the three views", total)
        assert total >= n // 2
    finally:
        ext.close()


# ---- the corrected poses and the chain ---------------------------------------------------------------------------------------
def opt_block(ext, S12):
    """an optimise block that holds S12 (f64 [13]) where spfe_optimize_sim3 stores it; the rest keeps the fill"""
    b = np.full(ext.sim3opt_out_bytes(), FILL, np.uint8)
    b[X.SIM3OPT_OFF_S12:X.SIM3OPT_OFF_S12 + 104] = np.ascontiguousarray(S12, np.float64).view(np.uint8)
    return dev(b)


def device_poses(ext, S12, Tcw2, Twc, Tiw, cur, stream=None):
    import torch
    T = len(Tiw)
    d_in = [opt_block(ext, S12), dev(np.asarray(Tcw2, np.float32).reshape(16)), dev(np.asarray(Twc, np.float32).reshape(16)),
            dev(np.asarray(Tiw, np.float32).reshape(T, 16))]
    d_S = torch.full((T + 1, 16), float("nan"), dtype=torch.float32, device="cuda")
    d_T = torch.full((T + 1, 16), float("nan"), dtype=torch.float32, device="cuda")
    ext.loop_corrected_poses_device(*[d.data_ptr() for d in d_in], T, cur, d_S.data_ptr(), d_T.data_ptr(), stream=stream)
    return d_S, d_T, d_in


@pytest.mark.parametrize("cur", ["none", "first", "last"])
def test_device_poses_equal_the_host_function_bit_for_bit(exts, cur):
    import torch
    ext = exts[False]
    for c in lc.load_poses():
        T = len(c["Tiw"])
        ci = {"none": -1, "first": 0, "last": T - 1}[cur]
        d_S, d_T, _ = device_poses(ext, c["S12"], c["Tcw2"], c["Twc"], c["Tiw"], ci)
        torch.cuda.synchronize()
        Siw, Tc = SPExtractor.loop_corrected_poses(c["S12"], c["Tcw2"], c["Twc"], c["Tiw"], ci)
        gS, gT = d_S.cpu().numpy(), d_T.cpu().numpy()
        assert gS[:T].tobytes() == Siw.tobytes() and gT[:T].tobytes() == Tc.tobytes()
        assert np.isnan(gS[T]).all() and np.isnan(gT[T]).all()            # nothing is written beyond n_targets
    # a NaN S12: every NaN leaves as the quiet NaN, on both sides
    S12 = c["S12"].copy()
    S12[3] = np.nan
    d_S, d_T, _ = device_poses(ext, S12, c["Tcw2"], c["Twc"], c["Tiw"], 1)
    torch.cuda.synchronize()
    Siw, Tc = SPExtractor.loop_corrected_poses(S12, c["Tcw2"], c["Twc"], c["Tiw"], 1)
    assert d_S.cpu().numpy()[:T].tobytes() == Siw.tobytes() and d_T.cpu().numpy()[:T].tobytes() == Tc.tobytes()
    assert np.isnan(Siw).any()


def test_poses_then_targets_on_one_stream_equal_the_targets_form_fed_the_host_poses(exts):
    """spfe_loop_corrected_poses_device writes d_Siw, spfe_loop_fuse_targets_record_device reads it as d_Scw: two calls on one
    stream, nothing in between.  S12 = (2, I, 0), Tcw2 = Twc = I and Tiw[j] = [I | 2 t_j] give Siw[j] = [2 I | 2 t_j]: the
    fixture's pans under the scale 2."""
    import torch
    ext = exts[False]
    g = lc.load("chain")
    tgs, p = lc.targets(g), lc.points(g)
    n, intr = len(p["point_id"]), [float(v) for v in g["intr"]]
    d_pts = dev_points(p)
    recs = [record(ext, t) for t in tgs]
    mps = [padded(ext, t["kf_mp"]) for t in tgs]
    Tiw = []
    for t in tgs:
        s = np.linalg.norm(t["Scw"][0, :3].astype(np.float64))
        T = np.eye(4, dtype=np.float32)
        T[:3, 3] = 2.0 * (t["Scw"][:3, 3].astype(np.float64) / s)
        Tiw.append(T)
    S12 = np.array([2.0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])
    I4 = np.eye(4, dtype=np.float32)
    Siw, _ = SPExtractor.loop_corrected_poses(S12, I4, I4, np.stack(Tiw), -1)
    want = many_targets(ext, recs, mps, list(Siw), d_pts, n, intr)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_S, d_T, keep = device_poses(ext, S12, I4, I4, np.stack(Tiw), -1, stream=stream.cuda_stream)
        got = many_targets(ext, recs, mps, None, d_pts, n, intr, d_S=d_S, stream=stream.cuda_stream)
    assert np.array_equal(got, want)
    assert d_S.cpu().numpy()[:3].tobytes() == Siw.tobytes()
    blocks = [ext.decode_fuse_out(b, max(n, 1)) for b in got]
    assert sum(b["n_fused"] for b in blocks) >= 10 and len({b.tobytes() for b in got}) == 3


# ---- refusals and the overflow decision --------------------------------------------------------------------------------------
def test_an_overflowed_record_is_searched_and_its_status_passed_through(exts, ref):
    ext = exts[False]
    g = lc.load("held_best")
    t, p = lc.targets(g)[0], lc.points(g)
    n, intr = len(p["point_id"]), [float(v) for v in g["intr"]]
    clean, raw0 = one_target(ext, record(ext, t), padded(ext, t["kf_mp"]), t["Scw"], dev_points(p), n, intr)
    over, raw1 = one_target(ext, record(ext, t, status=1), padded(ext, t["kf_mp"]), t["Scw"], dev_points(p), n, intr)
    same(over, lc.run_ref(ref, g, 0), "overflowed")
    assert clean["status"] == 0 and over["status"] == 1 and over["n_fused"] == clean["n_fused"] > 0
    assert np.array_equal(raw0[12:], raw1[12:]) and np.array_equal(raw0[:8], raw1[:8])


def test_invalid_arguments_return_before_any_launch(exts):
    import torch
    ext = exts[False]
    g = lc.load("held_best")
    t, p = lc.targets(g)[0], lc.points(g)
    n, intr = len(p["point_id"]), [float(v) for v in g["intr"]]
    d_rec, d_mp, d_S, d_pts = record(ext, t), dev(padded(ext, t["kf_mp"])), dev(t["Scw"].reshape(16)), dev_points(p)
    d_out = torch.full((2 * ext.fuse_out_bytes(8),), FILL, dtype=torch.uint8, device="cuda")
    q = lambda x: x.data_ptr()   # noqa: E731
    good = [q(d_rec), q(d_mp), q(d_S)] + point_ptrs(d_pts) + [n, q(d_out)]
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
            ext.loop_fuse_record_device(*a, *intr, **kw)
    many = lambda recs, **kw: ext.loop_fuse_targets_record_device(recs, *good[1:], *intr, **kw)   # noqa: E731
    for recs in ([], [q(d_rec)] * (X.FUSE_MAX_TARGETS + 1), [q(d_rec), 0]):
        with pytest.raises(X.SpfeError, match="SPFE_EINVAL"):
            many(recs)
    for kw in (dict(th=33.0), dict(n_cap=n - 1)):
        with pytest.raises(X.SpfeError, match="SPFE_EINVAL"):
            many([q(d_rec), q(d_rec)], **kw)
    with pytest.raises(X.SpfeError, match="SPFE_EINVAL"):                   # the host form: more points than the capacity
        big = X.PROJ_MAX_POINTS + 1
        ext.loop_fuse_search(t["kp_xy"], t["occ"], t["kp_desc"], t["kf_mp"], t["Scw"], np.zeros(big, np.int32), np.zeros((big, 3), np.float32),
                             np.zeros((big, 3), np.float32), np.zeros((big, 2), np.float32), np.zeros((big, 256), np.float32),
                             np.zeros(big, np.uint8), *intr)
    with pytest.raises(X.SpfeError, match="SPFE_EINVAL"):
        ext.loop_fuse_search(t["kp_xy"], t["occ"], t["kp_desc"], t["kf_mp"], t["Scw"], *[p[k] for k in lc.POINT_KEYS], *intr, th=40.0)
    # the poses: every pointer, the target count, the current keyframe's index
    d_blk, d_I = opt_block(ext, np.array([1.0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])), dev(np.eye(4, dtype=np.float32).reshape(16))
    d_Ti = dev(np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (4, 1)))
    d_po = torch.full((2, 4, 16), float("nan"), dtype=torch.float32, device="cuda")
    pg = [q(d_blk), q(d_I), q(d_I), q(d_Ti), 4, 0, q(d_po[0]), q(d_po[1])]
    pbad = []
    for i in (0, 1, 2, 3, 6, 7):
        a = list(pg)
        a[i] = 0
        pbad.append(a)
    for nt, cur in ((0, -1), (X.FUSE_MAX_TARGETS + 1, 0), (4, 4), (4, -2)):
        a = list(pg)
        a[4], a[5] = nt, cur
        pbad.append(a)
    for a in pbad:
        with pytest.raises(X.SpfeError, match="SPFE_EINVAL"):
            ext.loop_corrected_poses_device(*a)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == FILL).all() and np.array_equal(d_mp.cpu().numpy(), padded(ext, t["kf_mp"]))
    assert torch.isnan(d_po).all()
    ext.loop_fuse_record_device(*good, *intr, th=float(X.PROJ_MAX_RADIUS), n_cap=8)          # the radius at the cap is served
    ext.loop_corrected_poses_device(*pg)
    torch.cuda.synchronize()
    assert ext.decode_fuse_out(d_out.cpu().numpy(), 8)["n"] == n and not torch.isnan(d_po).any()
