"""GPU: the Sim3 hypotheses of loop verification (spfe_sim3_ransac, spfe_sim3_ransac_device, spfe_loop_verify_records_device:
sim3.hip) against the host reference tests/sim3_ref/sim3_ref.c, which shares include/spfe_sim3_math.h with the kernels: every
byte the contract says is written — N, the k1 list, T12, counts, inlier words, return list, best — bit for bit on the fixtures
tests/golden/sim3_*.npz, every other byte left alone; 1, 5, 300 and 512 hypotheses; the chain over 1, 2 and 16 candidates
against the two single forms byte for byte; the refusals; one extracted scene whose second keyframe's map lies under a known
similarity; and generated cases of 1300 keypoints (sim3_cases.large: six 256-lane chunks of the pairs kernel, 21 inlier
words) cut around the chunk edges, with 512 hypotheses, and of 10001 keypoints (40 chunks, 157 words)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "sim3_ref"))
sys.path.insert(0, os.path.join(ROOT, "tests", "track_ref"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_sim3 as gen  # noqa: E402
import sim3_cases as sc  # noqa: E402
import sim3_ref  # noqa: E402
import track_cases as trk  # noqa: E402

from sp_orb_slam_amd import extractor as X  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import SPExtractor  # noqa: E402
from tools import track_scene as ts  # noqa: E402

pytestmark = pytest.mark.gpu
H, W, NF = 64, 96, 100          # kmax = 101 > the fixtures' 72 keypoints
FILL = 0xA5
T12_BOUND = 2 * 2.7e-5          # 2 C, C = the largest |T12_f32 - T12_f64| of sim3_ref.c over the fixtures


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return sim3_ref.build(tmp_path_factory.mktemp("sim3_ref"))


@pytest.fixture(scope="module")
def ext():
    e = SPExtractor(NF, H, W, weights.synthetic(7, "trackable"), with_heat=False)
    yield e
    e.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_form(ext, g, rnd, **kw):
    """spfe_sim3_ransac_device on the fixture's arrays padded to kmax -> raw block on a background of FILL"""
    import torch
    kmax = ext.layout.kmax
    n = len(g["flags"])
    arrs = [dev(sim3_ref.pad(g[k], kmax)) for k in ("match12", "mp1", "mp2")]
    d_xyz, d_fl = dev(g["xyz"] if n else np.zeros((1, 3), np.float32)), dev(g["flags"] if n else np.zeros(1, np.uint8))
    d_T1, d_T2, d_r = dev(g["Tcw1"].reshape(16)), dev(g["Tcw2"].reshape(16)), dev(np.ascontiguousarray(rnd, np.uint32))
    d_out = torch.full((ext.sim3_out_bytes(len(rnd)) + 64,), FILL, dtype=torch.uint8, device="cuda")
    ext.sim3_ransac_device(int(g["K1"]), *[a.data_ptr() for a in arrs], d_xyz.data_ptr(), d_fl.data_ptr(), n, d_T1.data_ptr(),
                           d_T2.data_ptr(), d_r.data_ptr(), len(rnd), d_out.data_ptr(), g["intr1"], g["intr2"],
                           min_inliers=int(g["min_inliers"]), fix_scale=int(g["fix_scale"]), **kw)
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    assert (raw[-64:] == FILL).all()
    return raw[:-64]


def same_block(ref, g, rnd, got, kcap, what):
    """got == sim3_ref.c on the written bytes, and FILL everywhere else"""
    want_d, want, _, o = sc.run_ref(ref, g, kcap=kcap, rnd=rnd, fill=FILL)
    assert o["out_bytes"] == len(got) == X.sim3_offsets(kcap, len(rnd))["out_bytes"], what
    m = sim3_ref.written_mask(want_d, kcap, len(rnd), o)
    diff = np.flatnonzero(got != want)
    assert diff.size == 0, (what, "first differing byte", int(diff[0]), "written" if m[diff[0]] else "NOT to be written", o)
    assert (want[~m] == FILL).all()
    return want_d


@pytest.mark.parametrize("name", sc.NAMES)
def test_device_and_host_form_equal_the_host_reference_bit_for_bit(ext, ref, name):
    g = sc.load(name)
    kmax = ext.layout.kmax
    d = same_block(ref, g, g["rnd"], device_form(ext, g, g["rnd"]), kmax, (name, "device form"))
    assert sc.differences(g, d) == []                                   # (and the reference the float64 expectation)
    K1, K2 = int(g["K1"]), int(g["K2"])
    raw, kcap = ext.sim3_ransac(g["match12"][:K1], g["mp1"][:K1], g["mp2"][:K2], g["xyz"], g["flags"], g["Tcw1"], g["Tcw2"], g["rnd"],
                                g["intr1"], g["intr2"], min_inliers=int(g["min_inliers"]), fix_scale=int(g["fix_scale"]), fill=FILL)
    assert kcap == max(K1, K2)
    same_block(ref, g, g["rnd"], raw, kcap, (name, "host form"))
    dec = ext.decode_sim3_out(raw, kcap, len(g["rnd"]))
    assert dec["N"] == d["N"] and np.array_equal(dec["return_idx"], d["return_idx"])
    if d["evaluated"]:
        vb = np.zeros((len(g["rnd"]), kcap), bool)
        vb[:, d["k1"]] = g["want_inliers"]
        assert np.array_equal(dec["vbInliers"], vb)


@pytest.mark.parametrize("n_hyp", [1, 5, 300, 512])
def test_hypothesis_counts(ext, ref, n_hyp):
    g = sc.load("outliers40")
    rnd = np.random.default_rng(n_hyp).integers(0, 1 << 32, (n_hyp, 3), dtype=np.uint64).astype(np.uint32)
    rnd[0] = (0xffffffff, 0xffffffff, 0xffffffff)                       # the last live slot of every draw
    d = same_block(ref, g, rnd, device_form(ext, g, rnd), ext.layout.kmax, n_hyp)
    if n_hyp >= 300:
        assert d["n_returns"] >= 2 and d["best_count"] == 36


def chain_inputs(ext, n_cand, seed=2):
    """keyframe 1 and n_cand candidates as records with related rows, holders into one random map"""
    rng = np.random.default_rng(seed)
    kmax, K = ext.layout.kmax, 90
    L = ext.layout

    def rec(desc):
        b = np.zeros(ext.record_bytes(), np.uint8)
        b[L.off_hdr:L.off_hdr + 16].view(np.int32)[:] = [K, K, 0, 0]
        b[L.off_desc:L.off_desc + 1024 * K].view(np.float32)[:] = desc.astype(np.float32).reshape(-1)
        return dev(b)

    base = rng.normal(size=(K, 256))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    n = 400
    sceneP = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1, 1, n), rng.uniform(3, 6, n)], 1).astype(np.float32)
    flags = (rng.random(n) < 0.95).astype(np.uint8)
    mp1 = np.full(kmax, -1, np.int32)
    mp1[:K] = np.where(rng.random(K) < 0.85, rng.integers(0, n, K), -1)
    recs, mp2 = [rec(base)], np.full((n_cand, kmax), -1, np.int32)
    for j in range(n_cand):
        perm = rng.permutation(K)
        recs.append(rec(base[perm] + 0.05 * rng.normal(size=(K, 256))))
        mp2[j, :K] = np.where(rng.random(K) < (0.85 if j != 1 else 0.15), rng.integers(0, n, K), -1)   # candidate 1: too few pairs
    T1 = np.eye(4, dtype=np.float32)
    T2 = np.stack([ts.pose(3 * j, j) for j in range(n_cand)])
    return recs, mp1, mp2, sceneP, flags, T1, T2


@pytest.mark.parametrize("n_cand", [1, 2, 16])
def test_chain_equals_the_single_forms_byte_for_byte(ext, n_cand):
    import torch
    kmax, n_hyp = ext.layout.kmax, 24
    recs, mp1, mp2, P, flags, T1, T2 = chain_inputs(ext, n_cand)
    rnd = np.random.default_rng(9).integers(0, 1 << 32, (n_cand, n_hyp, 3), dtype=np.uint64).astype(np.uint32)
    ob = ext.sim3_out_bytes(n_hyp)
    d_mp1, d_mp2, d_P, d_f, d_T1, d_T2, d_r = dev(mp1), dev(mp2), dev(P), dev(flags), dev(T1.reshape(16)), dev(T2.reshape(-1, 16)), dev(rnd)
    q = lambda t: t.data_ptr()   # noqa: E731
    new = lambda nbytes: torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")   # noqa: E731
    c_m, c_n, c_out = new(n_cand * kmax * 4), new(n_cand * 4 + 8), new(n_cand * ob + 64)
    ext.loop_verify_records_device(q(recs[0]), [q(r) for r in recs[1:]], q(d_mp1), q(d_mp2), q(d_P), q(d_f), len(flags), q(d_T1),
                                   q(d_T2), q(d_r), n_hyp, q(c_m), q(c_n), q(c_out), trk.INTR)
    s_m, s_n, s_out = new(n_cand * kmax * 4), new(n_cand * 4 + 8), new(n_cand * ob + 64)
    for j in range(n_cand):
        ext.loop_match_record_device(q(recs[0]), q(recs[1 + j]), q(d_mp1), q(d_mp2[j]), q(s_m) + 4 * kmax * j, q(s_n) + 4 * j)
        ext.sim3_ransac_device(90, q(s_m) + 4 * kmax * j, q(d_mp1), q(d_mp2[j]), q(d_P), q(d_f), len(flags), q(d_T1), q(d_T2[j]),
                               q(d_r[j]), n_hyp, q(s_out) + ob * j, trk.INTR)
    torch.cuda.synchronize()
    for a, b in ((c_m, s_m), (c_n, s_n), (c_out, s_out)):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert (c_out.cpu().numpy()[-64:] == FILL).all() and (c_n.cpu().numpy()[-8:] == FILL).all()
    blocks = [ext.decode_sim3_out(c_out.cpu().numpy()[j * ob:(j + 1) * ob], kmax, n_hyp) for j in range(n_cand)]
    nm = c_n.cpu().numpy()[:4 * n_cand].view(np.int32)
    assert blocks[0]["N"] >= 20 and blocks[0]["best_h"] >= 0 and (nm >= [b["N"] for b in blocks]).all()
    if n_cand > 1:
        assert blocks[1]["N"] < 20 and blocks[1]["best_h"] == -1 and (blocks[1]["count"] == 0).all()


def test_invalid_arguments_return_before_any_launch(ext):
    import torch
    g = sc.load("clean_scale")
    kmax = ext.layout.kmax
    arrs = [dev(sim3_ref.pad(g[k], kmax)) for k in ("match12", "mp1", "mp2")]
    d_xyz, d_fl, d_T, d_r = dev(g["xyz"]), dev(g["flags"]), dev(g["Tcw1"].reshape(16)), dev(g["rnd"])
    d_out = torch.full((ext.sim3_out_bytes(8),), FILL, dtype=torch.uint8, device="cuda")
    q = lambda t: t.data_ptr()   # noqa: E731
    n = len(g["flags"])
    good = [int(g["K1"]), q(arrs[0]), q(arrs[1]), q(arrs[2]), q(d_xyz), q(d_fl), n, q(d_T), q(d_T), q(d_r), 8, q(d_out)]
    bad = []
    for i in (1, 2, 3, 4, 5, 7, 8, 9, 11):                                 # every pointer
        a = list(good)
        a[i] = 0
        bad.append((a, {}))
    for i, v in ((0, -1), (0, kmax + 1), (6, -1), (6, X.PROJ_MAX_POINTS + 1), (10, 0), (10, X.SIM3_MAX_HYPOTHESES + 1)):
        a = list(good)
        a[i] = v
        bad.append((a, {}))
    bad.append((good, dict(min_inliers=-1)))
    for a, kw in bad:
        with pytest.raises(X.SpfeError, match="SPFE_EINVAL"):
            ext.sim3_ransac_device(*a, g["intr1"], **kw)
    rec = torch.zeros(ext.record_bytes(), dtype=torch.uint8, device="cuda")
    chain = lambda recs, n_hyp=8, **kw: ext.loop_verify_records_device(   # noqa: E731
        q(rec), recs, q(arrs[1]), q(arrs[2]), q(d_xyz), q(d_fl), n, q(d_T), q(d_T), q(d_r), n_hyp, q(arrs[0]), q(d_out), q(d_out),
        g["intr1"], **kw)
    for recs in ([], [q(rec)] * (X.SIM3_MAX_CANDIDATES + 1), [0]):
        with pytest.raises(X.SpfeError, match="SPFE_EINVAL"):
            chain(recs)
    for n_hyp in (0, X.SIM3_MAX_HYPOTHESES + 1):
        with pytest.raises(X.SpfeError, match="SPFE_EINVAL"):
            chain([q(rec)], n_hyp)
    with pytest.raises(X.SpfeError, match="SPFE_EINVAL"):
        ext.loop_match_record_device(q(rec), 0, q(arrs[1]), q(arrs[2]), q(arrs[0]), q(d_out))
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == FILL).all() and np.array_equal(arrs[0].cpu().numpy(), sim3_ref.pad(g["match12"], kmax))


def test_two_extracted_keyframes_under_a_known_similarity():
    """Frames 2 and 4 of tools/track_scene (pans of 32 and 64 px) as the current keyframe and a loop candidate; every keypoint
    holds the point it back-projects to on the plane.  The candidate's map — its points and its pose — is expressed under the
    similarity (s0, R0, t0), as a map that drifted before the loop would be: X' = s0 R0 X + t0, Tcw2' = [R2 R0^T | s0 t2 -
    R2 R0^T t0], so that the candidate sees its points at s0 times their depth.  Then X1c = (1 / s0) X2c' + (t1 - t2): the first
    transform the chain returns is that one within 2 C, and more than min_inliers pairs agree with it."""
    import torch
    e = SPExtractor(trk.NF, trk.H, trk.W, weights.synthetic(7, "trackable"), with_heat=False)
    try:
        world = ts.texture(21, *ts.world_size(trk.H, trk.W))
        views = []
        for k in (2, 4):
            ox, oy = ts.offsets(k)
            d_img = dev(world[oy:oy + trk.H, ox:ox + trk.W][None].copy())
            d_rec = torch.zeros(e.record_bytes(), dtype=torch.uint8, device="cuda")
            e.wait_records(e.extract_batch_device(d_img.data_ptr(), 1, d_rec.data_ptr()))
            torch.cuda.synchronize()
            fr = e.view_record(d_rec.cpu().numpy())
            assert fr.status == 0 and fr.K >= trk.MIN_KEYPOINTS
            views.append((d_rec, fr, ts.pose(ox, oy).astype(np.float64)))
        (d1, f1, T1), (d2, f2, T2) = views
        kmax = e.layout.kmax
        fx, fy, cx, cy = trk.INTR

        def plane(fr, T):
            Xc = np.stack([(fr.kp_xy[:fr.K, 0] - cx) / fx * ts.Z0, (fr.kp_xy[:fr.K, 1] - cy) / fy * ts.Z0, np.full(fr.K, ts.Z0)], 1)
            return Xc - T[:3, 3]
        s0, t0 = 1.25, np.array([0.4, -0.3, 0.7])
        c, s = np.cos(0.2), np.sin(0.2)
        R0 = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
        P1, P2 = plane(f1, T1), s0 * plane(f2, T2) @ R0.T + t0
        T2d = np.eye(4)
        T2d[:3, :3] = T2[:3, :3] @ R0.T
        T2d[:3, 3] = s0 * T2[:3, 3] - T2d[:3, :3] @ t0
        xyz = np.concatenate([P1, P2]).astype(np.float32)
        mp1, mp2 = np.full(kmax, -1, np.int32), np.full(kmax, -1, np.int32)
        mp1[:f1.K], mp2[:f2.K] = np.arange(f1.K), f1.K + np.arange(f2.K)
        n_hyp = 64
        rnd = np.random.default_rng(0).integers(0, 1 << 32, (n_hyp, 3), dtype=np.uint64).astype(np.uint32)
        d_in = [dev(v) for v in (mp1, mp2, xyz, np.ones(len(xyz), np.uint8), T1.astype(np.float32).reshape(16),
                                 T2d.astype(np.float32).reshape(16), rnd)]
        d_m, d_n = dev(np.zeros(kmax, np.int32)), dev(np.zeros(1, np.int32))
        d_out = torch.zeros(e.sim3_out_bytes(n_hyp), dtype=torch.uint8, device="cuda")
        p = [t.data_ptr() for t in d_in]
        e.loop_verify_records_device(d1.data_ptr(), [d2.data_ptr()], p[0], p[1], p[2], p[3], len(xyz), p[4], p[5], p[6], n_hyp,
                                     d_m.data_ptr(), d_n.data_ptr(), d_out.data_ptr(), trk.INTR)
        torch.cuda.synchronize()
        out = e.decode_sim3_out(d_out.cpu().numpy(), kmax, n_hyp)
        print("scene: K", f1.K, f2.K, "n_matches", int(d_n.cpu()[0]), "N", out["N"], "returns", out["return_idx"][:8], "counts",
              out["count"][out["return_idx"][:8]], "best", out["best_h"], out["best_count"])
        assert out["n_returns"] >= 1
        h = int(out["return_idx"][0])
        want = np.concatenate([[1 / s0], np.eye(3).reshape(9), (T1[:3, 3] - T2[:3, 3])])
        print("scene: T12 error of the first return", np.abs(out["T12"][h] - want).max())
        assert out["count"][h] >= 21 and out["vbInliers"][h].sum() == out["count"][h]
        assert np.abs(out["T12"][h] - want).max() <= T12_BOUND
    finally:
        e.close()


# ---- beyond one pass of a workgroup ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ext_large():
    e = SPExtractor(1300, H, W, weights.synthetic(7, "trackable"), with_heat=False)
    assert e.layout.kmax == 1301
    yield e
    e.close()


@pytest.fixture(scope="module")
def large():
    return sc.large(0)


def test_large_case_device_and_host_form_equal_the_host_reference_bit_for_bit(ext_large, ref, large):
    g, ext = large, ext_large
    d = same_block(ref, g, g["rnd"], device_form(ext, g, g["rnd"]), ext.layout.kmax, "large, device form")
    assert sc.differences(g, d) == [] and d["N"] >= 1100 and d["n_returns"] >= 2
    K1, K2 = int(g["K1"]), int(g["K2"])
    raw, kcap = ext.sim3_ransac(g["match12"][:K1], g["mp1"][:K1], g["mp2"][:K2], g["xyz"], g["flags"], g["Tcw1"], g["Tcw2"], g["rnd"],
                                g["intr1"], g["intr2"], min_inliers=int(g["min_inliers"]), fill=FILL)
    assert kcap == 1300
    d = same_block(ref, g, g["rnd"], raw, kcap, "large, host form")
    assert sc.differences(g, d) == []
    dec = ext.decode_sim3_out(raw, kcap, len(g["rnd"]))
    vb = np.zeros((len(g["rnd"]), kcap), bool)
    vb[:, d["k1"]] = g["want_inliers"]
    assert np.array_equal(dec["vbInliers"], vb)


EDGES = [(k, None) for k in sc.CUTS] + [(1025, slice(0, 192)), (1025, slice(256, 512))]


@pytest.mark.parametrize("K1,empty", EDGES, ids=["%d%s" % (k, "" if e is None else "_without_%d_%d" % (e.start, e.stop)) for k, e in EDGES])
def test_chunk_and_wavefront_edges(ext_large, ref, large, K1, empty):
    """K1 at, one below and one beyond a multiple of the pairs kernel's 256 lanes, a pair in the last row; no pair in the
    first three wavefronts; no pair in a whole middle chunk"""
    c = sc.cut(large, K1, empty)
    rnd = large["rnd"][:8]                                               # (any words draw from any N)
    d = same_block(ref, c, rnd, device_form(ext_large, c, rnd), ext_large.layout.kmax, (K1, empty))
    k1 = gen.pairs64(c)[0]
    assert d["N"] == len(k1) and np.array_equal(d["k1"], k1) and k1[-1] == K1 - 1
    assert d["evaluated"]                                                # every cut keeps more than min_inliers pairs


def test_512_hypotheses_on_the_large_case(ext_large, ref, large):
    rnd = sc.words512(large)
    d = same_block(ref, large, rnd, device_form(ext_large, large, rnd), ext_large.layout.kmax, "512 hypotheses")
    assert len(set(int(h) // 64 for h in d["return_idx"])) >= 3          # (tests/test_sim3_reference.py: on the reference)


def test_capacity_10001_keypoints(ref):
    """spfe_create's largest num_features: 40 chunks of the pairs kernel, 157 inlier words per hypothesis"""
    g = sc.capacity(0)
    e = SPExtractor(10000, H, W, weights.synthetic(7, "trackable"), with_heat=False)
    try:
        assert e.layout.kmax == 10001 == int(g["K1"])
        d = same_block(ref, g, g["rnd"], device_form(e, g, g["rnd"]), e.layout.kmax, "capacity")
        assert sc.differences(g, d) == [] and d["N"] >= 9000 and d["n_returns"] >= 2
    finally:
        e.close()
