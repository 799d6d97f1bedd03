"""GPU: LocalMapping::CreateNewMapPointsOverride on resident keyframe records (spfe_create_map_points_pair_record_device,
spfe_create_map_points_record_device) against the host reference tests/tri_ref/tri_ref.c, which shares
include/spfe_tri_math.h with the kernels: every output, new_xyz included, bit for bit — on the fixtures tests/golden/tri_*.npz
laid out as records by spfe_get_record_layout, with f32 and with bf16 descriptor rows; the chain form against the pair form
called per neighbour with the skip decided on the host; real extractions of tools/track_scene at 128x160; the refusals; and
both forms on a generated case of 1300 keypoints (tri_cases.large: 6 blocks of the gate kernel, two 1024-lane chunks of the
triangulation) with its cuts to 1023, 1024, 1025 train rows and 256, 257 query rows."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tri_ref"))
sys.path.insert(0, os.path.join(ROOT, "tests", "track_ref"))
import track_cases as trk  # noqa: E402
import tri_cases as tc  # noqa: E402
import tri_ref  # noqa: E402

from sp_orb_slam_amd import extractor as X  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import SPExtractor  # noqa: E402
from tools import track_scene as ts  # noqa: E402

pytestmark = pytest.mark.gpu
KMAX = trk.KMAX
EPS = 2.0 ** -24
C_MEASURED = 3.77          # tests/test_tri_reference.py: the f32 null vector against the f64 one, measured on tri_ref.c
FILL = 0xA5


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return tri_ref.build(tmp_path_factory.mktemp("tri_ref"))


@pytest.fixture(scope="module")
def exts():
    e = {False: SPExtractor(trk.NF, trk.H, trk.W, weights.synthetic(7, "trackable"), with_heat=False),
         True: SPExtractor(trk.NF, trk.H, trk.W, weights.synthetic(7, "trackable"), with_heat=False, desc_bf16=True)}
    assert e[False].layout.kmax == KMAX
    yield e
    for x in e.values():
        x.close()


def record(ext, kf, status=0):
    """(kp_xy, cinv, desc f32) as one record of the handle's layout, on the device"""
    import torch
    L = ext.layout
    kp, cinv, desc = kf
    K = len(kp)
    assert K <= L.kmax
    b = np.zeros(ext.record_bytes(), np.uint8)
    b[L.off_hdr:L.off_hdr + 16].view(np.int32)[:] = [K, K, status, 0]
    b[L.off_xy:L.off_xy + 8 * K].view(np.float32)[:] = np.ascontiguousarray(kp, np.float32).reshape(-1)
    b[L.off_cinv:L.off_cinv + 8 * K].view(np.float32)[:] = np.ascontiguousarray(cinv, np.float32).reshape(-1)
    if ext.desc_bf16:
        b[L.off_desc:L.off_desc + 512 * K].view(np.uint16)[:] = tri_ref.to_bf16(desc).reshape(-1)
    else:
        b[L.off_desc:L.off_desc + 1024 * K].view(np.float32)[:] = np.ascontiguousarray(desc, np.float32).reshape(-1)
    return torch.from_numpy(b).cuda()


def padded(mp, kmax=KMAX):
    out = np.full(kmax, -1, np.int32)
    out[:len(mp)] = mp
    return out


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def intrinsics(g, j):
    return tuple(float(v) for v in g["intr1"]), tuple(float(v) for v in g["intr2"][j])


def gate_kw(g):
    p = [float(v) for v in g["params"]]
    return dict(ratio=p[0], epipole_r2=p[1], chi2_line=p[2], chi2_reproj=p[3], cos_parallax_max=p[4], min_baseline_depth_ratio=p[5])


def pair_forms(ext, ref, g, recs):
    """the fixture's chain as pair calls from the host, the skip decided on the host -> ([decoded block or None], [mp2 after],
    mp1 after, [raw block or None])"""
    import torch
    d1, d2s = recs
    n = int(g["n_neigh"])
    kmax = ext.layout.kmax
    d_mp1 = dev(padded(g["mp1"], kmax))
    d_T1 = dev(g["Tcw1"].reshape(16))
    base = int(g["point_base"])
    outs, mp2s, raws = [], [], []
    for j in range(n):
        d_mp2 = dev(padded(g["mp2_%d" % j], kmax))
        if tri_ref.skip(ref, g["Tcw1"], g["Tcw2"][j], tc.params(g, j), g["median_depth"][j]):
            outs.append(None); raws.append(None); mp2s.append(d_mp2.cpu().numpy())
            continue
        d_out = torch.full((ext.tri_out_bytes(),), FILL, dtype=torch.uint8, device="cuda")
        i1, i2 = intrinsics(g, j)
        d_T2 = dev(g["Tcw2"][j].reshape(16))             # (named: a temporary's memory is free again before the launch reads it)
        ext.create_map_points_pair_record_device(d1.data_ptr(), d2s[j].data_ptr(), d_mp1.data_ptr(), d_mp2.data_ptr(), d_T1.data_ptr(),
                                                 d_T2.data_ptr(), d_out.data_ptr(), i1, i2, point_base=base,
                                                 **gate_kw(g))
        torch.cuda.synchronize()
        raw = d_out.cpu().numpy()
        o = ext.decode_tri_out(raw, kmax)
        base += o["n_new"]
        outs.append(o); raws.append(raw); mp2s.append(d_mp2.cpu().numpy())
    return outs, mp2s, d_mp1.cpu().numpy(), raws


def records_of(ext, g):
    kf1, neigh = tc.frames(g)
    return record(ext, kf1), [record(ext, kf2) for kf2 in neigh]


def compare(name, g, got, want):
    outs, mp2s, mp1, _ = got
    wouts, wmp1 = want
    kmax = len(mp1)
    for j, (o, w) in enumerate(zip(outs, wouts)):
        assert (o is None) == (w is None), (name, j)
        if o is None:
            continue
        K1 = len(w["match12"])
        assert o["status"] == 0 and o["skipped"] == 0
        for k in tri_ref.COUNTS:
            print(name, j, k, o[k], w[k])
            assert o[k] == w[k], (name, j, k)
        assert np.array_equal(o["match12"][:K1], w["match12"]) and (o["match12"][K1:] == -1).all(), (name, j)
        assert np.array_equal(o["verdict"][:K1], w["verdict"]) and (o["verdict"][K1:] == 0).all(), (name, j)
        assert np.array_equal(o["new_k1"], w["new_k1"]) and np.array_equal(o["new_k2"], w["new_k2"]), (name, j)
        assert np.array_equal(o["new_xyz"].view(np.uint32), w["new_xyz"].view(np.uint32)), (name, j)      # bitwise
        assert np.array_equal(mp2s[j], padded(w["mp2"], kmax)), (name, j)
    assert np.array_equal(mp1, padded(wmp1, kmax)), name


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", tc.NAMES)
def test_pair_form_equals_the_host_reference_bit_for_bit(exts, ref, name, bf16):
    g = tc.load(name)
    ext = exts[bf16]
    want = tc.run_ref(ref, g, bf16=bf16)
    compare(name, g, pair_forms(ext, ref, g, records_of(ext, g)), want)
    if not bf16:                                      # (the fixture's rows are bf16 values: both runs see the same numbers)
        for j, w in enumerate(want[0]):
            if w is not None:
                assert np.array_equal(w["match12"], g["e%d_match12" % j]) and np.array_equal(w["verdict"], g["e%d_verdict" % j])


@pytest.mark.parametrize("name", ["chain", "no_free_rows", "behind_camera"])
def test_chain_form_equals_the_pair_form_per_neighbour(exts, ref, name):
    import torch
    g = tc.load(name)
    ext = exts[False]
    recs = records_of(ext, g)
    outs, mp2s, mp1, raws = pair_forms(ext, ref, g, recs)
    n = int(g["n_neigh"])
    ob = ext.tri_out_bytes()
    d_mp1 = dev(padded(g["mp1"]))
    d_mp2 = dev(np.concatenate([padded(g["mp2_%d" % j]) for j in range(n)]))
    d_out = torch.full((n * ob,), FILL, dtype=torch.uint8, device="cuda")
    i1, i2 = intrinsics(g, 0)
    assert all(intrinsics(g, j) == (i1, i2) for j in range(n))      # one chain call serves the neighbours of one camera
    d_T1, d_T2, d_med = dev(g["Tcw1"].reshape(16)), dev(g["Tcw2"].reshape(-1)), dev(g["median_depth"].astype(np.float32))
    ext.create_map_points_record_device(recs[0].data_ptr(), [r.data_ptr() for r in recs[1]], d_mp1.data_ptr(), d_mp2.data_ptr(),
                                        d_T1.data_ptr(), d_T2.data_ptr(), d_med.data_ptr(), d_out.data_ptr(), i1, i2,
                                        point_base=int(g["point_base"]), **gate_kw(g))
    torch.cuda.synchronize()
    blocks = d_out.cpu().numpy().reshape(n, ob)
    for j in range(n):
        o = ext.decode_tri_out(blocks[j], KMAX)
        if outs[j] is None:
            assert o["skipped"] == 1 and o["status"] == 0 and all(o[k] == 0 for k in tri_ref.COUNTS), (name, j)
            assert (blocks[j][64:] == FILL).all()                         # a skipped neighbour writes its int32 fields only
        else:
            K1 = len(g["kp1"])
            nn = o["n_new"]
            offs = X.tri_offsets(KMAX)
            assert np.array_equal(blocks[j][:36], raws[j][:36]), (name, j)                   # the int32 fields, point_base too
            for lo, hi in ((64, 64 + 4 * KMAX), (offs["verdict"], offs["verdict"] + 4 * KMAX), (offs["new_xyz"], offs["new_xyz"] + 12 * nn),
                           (offs["new_k1"], offs["new_k1"] + 4 * nn), (offs["new_k2"], offs["new_k2"] + 4 * nn)):
                assert np.array_equal(blocks[j][lo:hi], raws[j][lo:hi]), (name, j, lo)
            assert (blocks[j][offs["new_xyz"] + 12 * nn:offs["new_k1"]] == FILL).all()       # beyond n_new: not written
            assert K1 <= KMAX
    assert np.array_equal(d_mp1.cpu().numpy(), mp1)
    assert np.array_equal(d_mp2.cpu().numpy().reshape(n, KMAX), np.stack(mp2s))


# ---- real extractions ------------------------------------------------------------------------------------------------------
def extract(ext, img):
    import torch
    d_img = torch.from_numpy(np.ascontiguousarray(img)[None].copy()).cuda()
    d_rec = torch.zeros(ext.record_bytes(), dtype=torch.uint8, device="cuda")
    ext.wait_records(ext.extract_batch_device(d_img.data_ptr(), 1, d_rec.data_ptr()))
    torch.cuda.synchronize()
    return d_rec, ext.view_record(d_rec.cpu().numpy())


def scene_pair(ext, ref, off1, off2):
    """two views of the scene's plane panned by off1 / off2 pixels -> (decoded block, the reference's result, frames)"""
    import torch
    world = ts.texture(21, *ts.world_size(trk.H, trk.W))
    views = []
    for ox, oy in (off1, off2):
        d_rec, fr = extract(ext, world[oy:oy + trk.H, ox:ox + trk.W])
        assert fr.status == 0 and fr.K >= trk.MIN_KEYPOINTS
        views.append((d_rec, fr, ts.pose(ox, oy)))
    (d1, f1, T1), (d2, f2, T2) = views
    d_mp1, d_mp2 = dev(np.full(KMAX, -1, np.int32)), dev(np.full(KMAX, -1, np.int32))
    d_out = torch.full((ext.tri_out_bytes(),), FILL, dtype=torch.uint8, device="cuda")
    d_T1, d_T2 = dev(T1.reshape(16)), dev(T2.reshape(16))
    ext.create_map_points_pair_record_device(d1.data_ptr(), d2.data_ptr(), d_mp1.data_ptr(), d_mp2.data_ptr(), d_T1.data_ptr(),
                                             d_T2.data_ptr(), d_out.data_ptr(), trk.INTR)
    torch.cuda.synchronize()
    o = ext.decode_tri_out(d_out.cpu().numpy(), KMAX)
    w = tri_ref.pair(ref, (f1.kp_xy, f1.cov2_inv, f1.descriptors), (f2.kp_xy, f2.cov2_inv, f2.descriptors), np.full(f1.K, -1), np.full(f2.K, -1),
                     T1, T2, tri_ref.params(trk.INTR, trk.INTR))
    for k in tri_ref.COUNTS:
        print(off1, off2, k, o[k], w[k])
        assert o[k] == w[k], k
    assert np.array_equal(o["match12"][:f1.K], w["match12"]) and np.array_equal(o["verdict"][:f1.K], w["verdict"])
    assert np.array_equal(o["new_xyz"].view(np.uint32), w["new_xyz"].view(np.uint32))
    assert np.array_equal(d_mp1.cpu().numpy(), padded(w["mp1"])) and np.array_equal(d_mp2.cpu().numpy(), padded(w["mp2"]))
    return o, w, (f1, T1), (f2, T2)


def test_scene_frames_two_pans_apart_give_points_on_the_plane(exts, ref):
    """Frames 2 and 4 of tools/track_scene (pans of 32 and 64 px along x): the keypoints repeat from frame to frame at whole
    pixels, so every triangulated point lies on the plane z = Z0 up to the f32 null vector's error,
    2 C 2^-24 (sigma_1 / sigma_3) |x| (tests/test_tri_reference.py), sigma from the f64 SVD of that pair's A."""
    o, w, (f1, T1), (f2, T2) = scene_pair(exts[False], ref, ts.offsets(2), ts.offsets(4))
    assert o["n_new"] >= trk.MIN_KEYPOINTS // 2
    fx, fy, cx, cy = trk.INTR
    worst = 0.0
    for x, k1, k2 in zip(o["new_xyz"].astype(np.float64), o["new_k1"], o["new_k2"]):
        rows = []
        for (f, T), k in (((f1, T1), k1), ((f2, T2), k2)):
            P = T.astype(np.float64)[:3]
            xn = (f.kp_xy[k, 0] - np.float64(np.float32(cx))) / fx, (f.kp_xy[k, 1] - np.float64(np.float32(cy))) / fy
            rows += [xn[0] * P[2] - P[0], xn[1] * P[2] - P[1]]
        sv = np.linalg.svd(np.stack(rows), compute_uv=False)
        bound = 2 * C_MEASURED * EPS * sv[0] / sv[2] * np.linalg.norm(x)
        worst = max(worst, abs(x[2] - ts.Z0) / bound)
        assert abs(x[2] - ts.Z0) <= bound, (k1, k2, x, bound)
    print("largest |z - Z0| / bound:", worst)


def test_frames_eight_pixels_apart_in_y_give_parallax_rejections_only(exts, ref):
    o, _, _, _ = scene_pair(exts[False], ref, (32, 0), (32, 8))
    assert o["n_new"] == 0 and o["n_rej_parallax"] >= trk.MIN_KEYPOINTS // 2
    assert o["n_rej_parallax"] == (o["match12"] >= 0).sum() and o["n_rej_depth"] == o["n_rej_reproj"] == o["n_rej_degenerate"] == 0


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_overflowed_neighbour_is_skipped_and_the_next_one_runs(exts, ref):
    import torch
    g = tc.load("no_free_rows")                        # three neighbours; the last one makes points
    ext = exts[False]
    kf1, neigh = tc.frames(g)
    d1 = record(ext, kf1)
    d2s = [record(ext, neigh[2], status=1), record(ext, neigh[2])]
    ob = ext.tri_out_bytes()
    d_mp1 = dev(padded(g["mp1"]))
    d_mp2 = dev(np.concatenate([padded(g["mp2_2"])] * 2))
    d_out = torch.full((2 * ob,), FILL, dtype=torch.uint8, device="cuda")
    T2 = np.stack([g["Tcw2"][2]] * 2)
    d_T1, d_T2, d_med = dev(g["Tcw1"].reshape(16)), dev(T2.reshape(-1)), dev(np.full(2, 6.0, np.float32))
    ext.create_map_points_record_device(d1.data_ptr(), [d.data_ptr() for d in d2s], d_mp1.data_ptr(), d_mp2.data_ptr(),
                                        d_T1.data_ptr(), d_T2.data_ptr(), d_med.data_ptr(), d_out.data_ptr(), intrinsics(g, 2)[0], point_base=5)
    torch.cuda.synchronize()
    b = d_out.cpu().numpy().reshape(2, ob)
    assert b[0][28:32].view(np.int32)[0] == X.TRI_STATUS_COV_OVERFLOW
    assert (b[0][:28] == FILL).all() and (b[0][32:] == FILL).all()                    # the status and nothing else
    mp2 = d_mp2.cpu().numpy().reshape(2, KMAX)
    assert np.array_equal(mp2[0], padded(g["mp2_2"]))
    o = ext.decode_tri_out(b[1], KMAX)
    want = tri_ref.pair(ref, kf1, neigh[2], g["mp1"], g["mp2_2"], g["Tcw1"], g["Tcw2"][2], tc.params(g, 2), 5)
    assert o["status"] == 0 and o["n_new"] == want["n_new"] > 0 and o["point_base"] == 5
    assert np.array_equal(o["new_xyz"].view(np.uint32), want["new_xyz"].view(np.uint32))
    assert np.array_equal(d_mp1.cpu().numpy(), padded(want["mp1"])) and np.array_equal(mp2[1], padded(want["mp2"]))


def test_overflowed_current_keyframe_writes_nothing(exts):
    import torch
    g = tc.load("no_free_rows")
    ext = exts[False]
    kf1, neigh = tc.frames(g)
    d1 = record(ext, kf1, status=1)
    d2s = [record(ext, neigh[2]), record(ext, neigh[2])]
    ob = ext.tri_out_bytes()
    mp1, mp2 = padded(g["mp1"]), np.concatenate([padded(g["mp2_2"])] * 2)
    d_mp1, d_mp2 = dev(mp1), dev(mp2)
    d_out = torch.full((2 * ob,), FILL, dtype=torch.uint8, device="cuda")
    d_T1, d_T2, d_med = dev(g["Tcw1"].reshape(16)), dev(np.stack([g["Tcw2"][2]] * 2).reshape(-1)), dev(np.full(2, 6.0, np.float32))
    ext.create_map_points_record_device(d1.data_ptr(), [d.data_ptr() for d in d2s], d_mp1.data_ptr(), d_mp2.data_ptr(),
                                        d_T1.data_ptr(), d_T2.data_ptr(), d_med.data_ptr(), d_out.data_ptr(), intrinsics(g, 2)[0])
    torch.cuda.synchronize()
    b = d_out.cpu().numpy().reshape(2, ob)
    for j in range(2):
        assert b[j][28:32].view(np.int32)[0] == X.TRI_STATUS_COV_OVERFLOW and (b[j][:28] == FILL).all() and (b[j][32:] == FILL).all()
    assert np.array_equal(d_mp1.cpu().numpy(), mp1) and np.array_equal(d_mp2.cpu().numpy(), mp2)


def test_invalid_arguments_return_before_any_launch(exts):
    import torch
    ext = exts[False]
    g = tc.load("one_train_row")
    kf1, neigh = tc.frames(g)
    d1, d2 = record(ext, kf1), record(ext, neigh[0])
    d_mp = dev(np.full(KMAX, -1, np.int32))
    d_T = dev(np.eye(4, dtype=np.float32).reshape(16))
    d_med = dev(np.ones(40, np.float32))
    d_out = torch.full((ext.tri_out_bytes(),), FILL, dtype=torch.uint8, device="cuda")
    intr = intrinsics(g, 0)[0]
    p = lambda t: t.data_ptr()   # noqa: E731
    good = [p(d1), p(d2), p(d_mp), p(d_mp), p(d_T), p(d_T), p(d_out)]
    for i in range(7):
        a = list(good)
        a[i] = 0
        with pytest.raises(X.SpfeError, match="SPFE_EINVAL"):
            ext.create_map_points_pair_record_device(*a, intr)
    with pytest.raises(X.SpfeError, match="SPFE_EINVAL"):
        ext.create_map_points_pair_record_device(*good, intr, point_base=-1)
    chain = lambda recs, **kw: ext.create_map_points_record_device(p(d1), recs, p(d_mp), p(d_mp), p(d_T), p(d_T), p(d_med), p(d_out), intr, **kw)   # noqa: E731
    for recs in ([], [p(d2)] * (X.TRI_MAX_NEIGHBOURS + 1), [p(d2), 0]):
        with pytest.raises(X.SpfeError, match="SPFE_EINVAL"):
            chain(recs)
    with pytest.raises(X.SpfeError, match="SPFE_EINVAL"):
        ext.create_map_points_record_device(p(d1), [p(d2)], p(d_mp), p(d_mp), p(d_T), p(d_T), 0, p(d_out), intr)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == FILL).all() and (d_mp.cpu().numpy() == -1).all()


# ---- 1300 keypoints: more than one block of the gate kernel, more than one chunk of the triangulation ----------------------
NF_LARGE = 1300


@pytest.fixture(scope="module")
def large():
    return tc.large(0)


@pytest.fixture(scope="module")
def large_exts():
    made = {}

    def get(bf16):
        if bf16 not in made:
            made[bf16] = SPExtractor(NF_LARGE, 64, 96, weights.synthetic(7, "trackable"), with_heat=False, desc_bf16=bf16)
            assert made[bf16].layout.kmax == NF_LARGE + 1
        return made[bf16]
    yield get
    for x in made.values():
        x.close()


def only_fill_outside_the_extents(raw, kmax):
    """a block that ran: the nine int32 fields, match12 and verdict over kmax, n_new rows of new_xyz / new_k1 / new_k2"""
    o, n = X.tri_offsets(kmax), int(raw[4:8].view(np.int32)[0])
    m = np.zeros(len(raw), bool)
    m[:4 * len(X.TRI_FIELDS)] = True
    m[X.TRI_OFF_MATCH12:o["new_xyz"] + 12 * n] = True
    m[o["new_k1"]:o["new_k1"] + 4 * n] = True
    m[o["new_k2"]:o["new_k2"] + 4 * n] = True
    assert len(raw) == o["out_bytes"] and (raw[~m] == FILL).all()


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_large_pair_form_equals_the_host_reference_bit_for_bit(large_exts, ref, large, bf16):
    g, ext = large, large_exts(bf16)
    want = tc.run_ref(ref, g, bf16=bf16)
    got = pair_forms(ext, ref, g, records_of(ext, g))
    compare("large", g, got, want)
    outs, raws = got[0], got[3]
    assert outs[0]["point_base"] == int(g["point_base"]) and outs[1]["point_base"] == int(g["point_base"]) + outs[0]["n_new"]
    assert outs[0]["n_new"] == len(g["e0_new_k1"]) >= 300 and outs[1]["n_new"] == len(g["e1_new_k1"]) >= 100   # (not vacuous)
    for raw in raws:
        only_fill_outside_the_extents(raw, ext.layout.kmax)
    for j, w in enumerate(want[0]):                    # and the reference the f64 statement
        assert np.array_equal(w["match12"], g["e%d_match12" % j]) and np.array_equal(w["verdict"], g["e%d_verdict" % j])


def test_large_chain_form_equals_the_host_reference_bit_for_bit(large_exts, ref, large):
    import torch
    g, ext = large, large_exts(False)
    kmax, ob, n = ext.layout.kmax, ext.tri_out_bytes(), int(g["n_neigh"])
    d1, d2s = records_of(ext, g)
    d_mp1 = dev(padded(g["mp1"], kmax))
    d_mp2 = dev(np.concatenate([padded(g["mp2_%d" % j], kmax) for j in range(n)]))
    d_out = torch.full((n * ob + 64,), FILL, dtype=torch.uint8, device="cuda")
    i1, i2 = intrinsics(g, 0)
    assert intrinsics(g, 1) == (i1, i2)
    d_T1, d_T2, d_med = dev(g["Tcw1"].reshape(16)), dev(g["Tcw2"].reshape(-1)), dev(g["median_depth"].astype(np.float32))
    ext.create_map_points_record_device(d1.data_ptr(), [r.data_ptr() for r in d2s], d_mp1.data_ptr(), d_mp2.data_ptr(),
                                        d_T1.data_ptr(), d_T2.data_ptr(), d_med.data_ptr(), d_out.data_ptr(), i1, i2,
                                        point_base=int(g["point_base"]), **gate_kw(g))
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    assert (raw[n * ob:] == FILL).all()
    blocks = raw[:n * ob].reshape(n, ob)
    outs = [ext.decode_tri_out(b, kmax) for b in blocks]
    compare("large chain", g, (outs, list(d_mp2.cpu().numpy().reshape(n, kmax)), d_mp1.cpu().numpy(), None), tc.run_ref(ref, g))
    assert outs[0]["point_base"] == int(g["point_base"]) and outs[1]["point_base"] == int(g["point_base"]) + outs[0]["n_new"] > int(g["point_base"])
    for b in blocks:
        only_fill_outside_the_extents(b, kmax)


@pytest.mark.parametrize("K1,K2", [(1023, None), (1024, None), (1025, None), (None, 256), (None, 257)])
def test_large_case_cut_at_the_chunk_and_block_edges(large_exts, ref, large, K1, K2):
    """the last lane of a 1024-lane chunk, the first of the next one, and the last lane of a block of the gate kernel hold the
    pair of a new point (tests/test_tri_reference.py asserts that on the reference)"""
    ext = large_exts(False)
    c = tc.cut(large, K1, K2)
    want = tc.run_ref(ref, c)
    got = pair_forms(ext, ref, c, records_of(ext, c))
    compare("cut %s %s" % (K1, K2), c, got, want)
    w = want[0][0]
    assert (w["new_k1"][-1] == K1 - 1) if K1 else (w["new_k2"] == K2 - 1).any()
    only_fill_outside_the_extents(got[3][0], ext.layout.kmax)
