"""GPU: the three ordered-claim kernels — proj_resolve_kernel (spfe_search_projection*), patch_resolve_kernel
(spfe_match_patches*) and loopproj_claim_kernel (spfe_search_loop_points*) — beyond the 1024 keypoints one trip of their
workgroup covers, on the launches that need more than 48 KB of dynamic LDS, and at the largest keypoint counts the library
accepts, against tests/proj_ref/proj_ref.c, oracle_match_patches and tests/guided_ref/guided_ref.c: everything for equality,
float outputs bit for bit.  The cases are tests/proj_ref/proj_cases.py, tests/patch_cases.py and tests/guided_ref/guided_cases.py;
tests/test_claim_scale_cases.py shows on the CPU that in them the keypoints above each boundary decide the answer.

The limits: a workgroup has 163,840 bytes of LDS, and the kernels' static variables count.
  projection search   16 + 9 K + 16 bytes: K <= 18200   patches   4 + 5 K + 16: K <= 32764   loop points   80 + 5 K + 16: K <= 32748
spfe_create bounds num_features to 10000, so only the host-array forms, which size the claim by K, reach them."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("proj_ref", "guided_ref"):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import guided_cases as gc  # noqa: E402
import guided_ref  # noqa: E402
import patch_cases as pac  # noqa: E402
import proj_cases as pjc  # noqa: E402
import proj_ref  # noqa: E402

from oracle import oracle  # noqa: E402
from sp_orb_slam_amd import extractor as X  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import SPExtractor, SpfeError  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 0xA5
PROJ_MAX_K, PATCH_MAX_K, LOOP_MAX_K = 18200, 32764, 32748


@pytest.fixture(scope="module")
def pref(tmp_path_factory):
    return proj_ref.build(tmp_path_factory.mktemp("proj_ref"))


@pytest.fixture(scope="module")
def gref(tmp_path_factory):
    return guided_ref.build(tmp_path_factory.mktemp("guided_ref"))


@pytest.fixture(scope="module")
def blob():
    return weights.synthetic(7, "trackable")


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sync():
    import torch
    torch.cuda.synchronize()


def record(ext, occ, kp_desc, kp_xy=None, K=None):
    """(kp_xy, occ, kp_desc f32) as one record of the handle's layout, on the device; K: the header's count"""
    L = ext.layout
    n = len(kp_desc)
    K = n if K is None else K
    assert n <= L.kmax and occ.shape == (ext.height // 8, ext.width // 8)
    b = np.zeros(ext.record_bytes(), np.uint8)
    b[L.off_hdr:L.off_hdr + 16].view(np.int32)[:] = [K, K, 0, 0]
    if kp_xy is not None:
        b[L.off_xy:L.off_xy + 8 * n].view(np.float32)[:] = np.ascontiguousarray(kp_xy, np.float32).reshape(-1)
    b[L.off_occ:L.off_occ + 2 * occ.size].view(np.int16)[:] = np.ascontiguousarray(occ, np.int16).reshape(-1)
    if ext.desc_bf16:
        b[L.off_desc:L.off_desc + 512 * n].view(np.uint16)[:] = guided_ref.to_bf16(kp_desc).reshape(-1)
    else:
        b[L.off_desc:L.off_desc + 1024 * n].view(np.float32)[:] = np.ascontiguousarray(kp_desc, np.float32).reshape(-1)
    return dev(b)


def bf16_rows(rows):
    return guided_ref.widen_bf16(guided_ref.to_bf16(rows))


# ---- the window search by projection -------------------------------------------------------------------------------------------
def proj_same(got, want, what):
    for k in ("mp_of_kp", "kp_of_mp", "in_view"):
        assert np.array_equal(got[k], want[k]), (what, k)
    assert got["n_matches"] == want["n_matches"] and got["n_to_match"] == want["n_to_match"], what
    assert np.array_equal(got["proj_uv"].view(np.uint32), want["proj_uv"].view(np.uint32)), (what, "proj_uv bits")
    assert np.array_equal(got["view_cos"].view(np.uint32), want["view_cos"].view(np.uint32)), (what, "view_cos bits")


def proj_host(ext, g, **kw):
    return ext.search_projection(g["kp_xy"], g["occ"], g["kp_desc"], g["xyz"], g["normal"], g["desc"], g["flags"], g["mp_of_kp"], g["Tcw"],
                                 *g["intr"], **kw)


class TestProjectionSearch:
    H, W, NF = 480, 752, 5700

    @pytest.fixture(scope="class")
    def exts(self, blob):
        e = {False: SPExtractor(self.NF, self.H, self.W, blob, with_heat=False),
             True: SPExtractor(self.NF, self.H, self.W, blob, with_heat=False, desc_bf16=True)}
        yield e
        for x in e.values():
            x.close()

    @pytest.mark.parametrize("K", [1023, 1024, 1025, 2049, 5459, 5460, 5640])
    def test_host_form_around_the_thread_count_and_the_lds_threshold(self, exts, pref, K):
        g = pjc.scale(K)
        for kw in pjc.MODES + (dict(pjc.MODES[0], adaptive=False),):
            want = pjc.run_ref(proj_ref, pref, g, **kw)
            proj_same(proj_host(exts[False], g, **kw), want, (K, kw))
            assert want["n_matches"] >= 300 and want["kp_of_mp"].max() >= K - 20

    def test_chain_of_1500_takes_a_round_per_point(self, exts, pref):
        c = pjc.chain(1500)
        want = pjc.run_ref(proj_ref, pref, c, **pjc.MODES[0])
        assert np.array_equal(want["kp_of_mp"], np.arange(1500))
        proj_same(proj_host(exts[False], c, **pjc.MODES[0]), want, "chain")

    def device_search(self, ext, g, d_rec, n, **kw):
        import torch
        kmax, K = ext.layout.kmax, len(g["kp_xy"])
        mp = np.full(kmax, 777, np.int32)                                  # entries at and beyond K: left alone
        mp[:K] = np.where(g["mp_of_kp"] < n, g["mp_of_kp"], -1)
        d = [dev(g[k][:n]) for k in ("xyz", "normal", "desc", "flags")]
        d_mp, d_T = dev(mp), dev(g["Tcw"].reshape(16))
        guard, ob = 4096, ext.proj_out_bytes()
        d_out = torch.full((ob + 2 * guard,), FILL, dtype=torch.uint8, device="cuda")
        ext.search_projection_record_device(d_rec.data_ptr(), *[t.data_ptr() for t in d], n, d_mp.data_ptr(), d_T.data_ptr(),
                                            d_out.data_ptr() + guard, *g["intr"], **kw)
        sync()
        raw = d_out.cpu().numpy()
        assert (raw[:guard] == FILL).all() and (raw[guard + ob:] == FILL).all()
        got = ext.decode_proj_out(raw[guard:guard + ob])
        assert got["n"] == n
        m = d_mp.cpu().numpy()
        assert (m[K:] == 777).all()
        got["mp_of_kp"] = m[:K]
        return got

    @pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
    @pytest.mark.parametrize("K", [1025, 5640])
    def test_record_form_on_a_handle_of_5700_features(self, exts, pref, K, bf16):
        ext = exts[bf16]
        assert ext.layout.kmax == 5701                                    # 9 * 5701 + 16 bytes: the raised-LDS launch at every K
        g = pjc.scale(K)
        if bf16:
            g = dict(g, kp_desc=bf16_rows(g["kp_desc"]))
        d_rec = record(ext, g["occ"], g["kp_desc"], g["kp_xy"])
        for n, kw in ((1500, pjc.MODES[0]), (1203, pjc.MODES[1])):
            want = pjc.run_ref(proj_ref, pref, g, n=n, **kw)
            proj_same(self.device_search(ext, g, d_rec, n, **kw), want, (K, n, kw))
            assert want["n_matches"] >= 250

    def test_batch_of_two_frames_with_guards(self, exts, pref):
        import torch
        ext = exts[False]
        kmax, rb, ob, stride = ext.layout.kmax, ext.record_bytes(), ext.proj_out_bytes(), 1500
        cases, counts = [pjc.scale(1025, seed=1), pjc.scale(5640, seed=2)], np.array([1203, 1500], np.int32)
        d_recs = torch.cat([record(ext, g["occ"], g["kp_desc"], g["kp_xy"]) for g in cases])
        assert d_recs.numel() == 2 * rb
        mp = np.full((2, kmax), 777, np.int32)
        for f, g in enumerate(cases):
            mp[f, :len(g["kp_xy"])] = np.where(g["mp_of_kp"] < counts[f], g["mp_of_kp"], -1)
        cat = {k: dev(np.concatenate([g[k] for g in cases])) for k in ("xyz", "normal", "desc", "flags")}
        d_T = dev(np.stack([g["Tcw"].reshape(16) for g in cases]))
        for kw in pjc.MODES:
            d_mp, d_n = dev(mp), dev(counts)
            d_out = torch.full((2 * ob,), FILL, dtype=torch.uint8, device="cuda")
            ext.search_projection_batch_device(d_recs.data_ptr(), 2, cat["xyz"].data_ptr(), cat["normal"].data_ptr(), cat["desc"].data_ptr(),
                                               cat["flags"].data_ptr(), d_n.data_ptr(), stride, d_mp.data_ptr(), d_T.data_ptr(),
                                               d_out.data_ptr(), *cases[0]["intr"], **kw)
            sync()
            raw, got_mp = d_out.cpu().numpy().reshape(2, ob), d_mp.cpu().numpy()
            for f, g in enumerate(cases):
                n, K = int(counts[f]), len(g["kp_xy"])
                got = ext.decode_proj_out(raw[f])
                assert got["n"] == n and (got_mp[f, K:] == 777).all()
                got["mp_of_kp"] = got_mp[f, :K]
                proj_same(got, pjc.run_ref(proj_ref, pref, g, n=n, **kw), (f, kw))
                for off, size in ((X.PROJ_OFF_KP, 4), (X.PROJ_OFF_UV, 8), (X.PROJ_OFF_COS, 4), (X.PROJ_OFF_VIEW, 1)):
                    assert (raw[f, off + size * n:off + size * X.PROJ_MAX_POINTS] == FILL).all(), (f, off)
                assert (raw[f, 12:X.PROJ_OFF_KP] == FILL).all() and (raw[f, X.PROJ_OFF_VIEW + X.PROJ_MAX_POINTS:] == FILL).all()


# ---- the patch association and the loop points on a handle of 10,000 features ------------------------------------------------------
def lp_same(got, m, want, what):
    for k in ("reason", "kp_of_mp", "matched_idx"):
        assert np.array_equal(got[k], want[k]), (what, k)
    assert got["n_matched"] == want["n_matched"], what
    assert np.array_equal(got["best_dist"].view(np.uint32), want["best_dist"].view(np.uint32)), (what, "best_dist bits")
    assert np.array_equal(m[:len(want["matched"])], want["matched"]), (what, "matched")


def lp_host(ext, g):
    return ext.search_loop_points(g["kp_xy"], g["occ"], g["kp_desc"], g["Scw"], g["matched"], *[g[k] for k in gc.POINT_KEYS],
                                  *[float(v) for v in g["intr"]])


def patches_record(ext, g, d_rec, max_dist=0.75):
    import torch
    m = len(g["desc"])
    d_desc, d_uv = dev(g["desc"]), dev(g["uv"])
    d_out = torch.full((m + 64,), -7, dtype=torch.int32, device="cuda")
    ext.match_patches_record_device(d_desc.data_ptr(), d_uv.data_ptr(), m, d_rec.data_ptr(), d_out.data_ptr(), max_dist, None)
    sync()
    out = d_out.cpu().numpy()
    assert (out[m:] == -7).all()
    return out[:m]


class TestPatchesAndLoopPoints:
    @pytest.fixture(scope="class")
    def exts(self, blob):
        try:
            H, W = 800, 1024                                              # 12,800 cells
            big = SPExtractor(10000, H, W, blob, with_heat=False)
        except SpfeError:
            H, W = 720, 1280                                              # 14,400 cells
            big = SPExtractor(10000, H, W, blob, with_heat=False)
        e = dict(big=big, small=SPExtractor(1100, H, W, blob, with_heat=False), H=H, W=W)
        yield e
        e["big"].close()
        e["small"].close()

    @pytest.mark.parametrize("K", [1025, 9827, 9900])
    def test_patches_both_forms(self, exts, K):
        ext, hc, wc = exts["big"], exts["H"] // 8, exts["W"] // 8
        assert ext.layout.kmax == 10001                                   # 5 * 10001 + 16 bytes: the record form raises the LDS limit
        g = pac.scale(K, hc=hc, wc=wc)
        want = oracle.match_patches(g["desc"], g["uv"], g["occ"], g["kp_desc"])
        assert want.max() >= K - 5 and ((want >= 1024).sum() >= 20 or K == 1025)
        assert np.array_equal(ext.match_patches(g["desc"], g["uv"], g["occ"], g["kp_desc"]), want)
        assert np.array_equal(patches_record(ext, g, record(ext, g["occ"], g["kp_desc"])), want)
        if K == 1025:                                                     # ... and below 48 KB with a second trip: kmax 1101
            small = exts["small"]
            assert np.array_equal(patches_record(small, g, record(small, g["occ"], g["kp_desc"])), want)
            assert np.array_equal(small.match_patches(g["desc"], g["uv"], g["occ"], g["kp_desc"]), want)

    def test_patch_chain_of_1500_takes_a_round_per_point(self, exts):
        ext = exts["big"]
        c = pac.chain(1500, hc=exts["H"] // 8, wc=exts["W"] // 8)
        want = oracle.match_patches(c["desc"], c["uv"], c["occ"], c["kp_desc"])
        assert np.array_equal(want, np.arange(1500))
        assert np.array_equal(ext.match_patches(c["desc"], c["uv"], c["occ"], c["kp_desc"]), want)
        assert np.array_equal(patches_record(ext, c, record(ext, c["occ"], c["kp_desc"])), want)

    @pytest.mark.parametrize("K", [1025, 9827, 9828, 9900])
    def test_loop_points_host_form(self, exts, gref, K):
        g = gc.lp_scale(K, H=exts["H"], W=exts["W"])
        want = gc.lp_ref(gref, g)
        assert want["n_matched"] >= 300 and want["kp_of_mp"].max() >= K - 5
        got = lp_host(exts["big"], g)
        lp_same(got, got["matched"], want, K)

    def test_loop_points_record_form(self, exts, gref):
        import torch
        ext, K = exts["big"], 9900
        g = gc.lp_scale(K, H=exts["H"], W=exts["W"])
        want = gc.lp_ref(gref, g)
        n = len(g["point_id"])
        m0 = np.full(ext.layout.kmax, 12345, np.int32)
        m0[:K] = g["matched"]
        d_rec, d_m, d_S = record(ext, g["occ"], g["kp_desc"], g["kp_xy"]), dev(m0), dev(np.asarray(g["Scw"], np.float32).reshape(16))
        pts = [dev(g[k]) for k in gc.POINT_KEYS]
        d_out = torch.full((ext.loop_proj_out_bytes(n + 3),), FILL, dtype=torch.uint8, device="cuda")
        ext.search_loop_points_record_device(d_rec.data_ptr(), d_S.data_ptr(), d_m.data_ptr(), *[t.data_ptr() for t in pts], n,
                                             d_out.data_ptr(), *[float(v) for v in g["intr"]], n_cap=n + 3)
        sync()
        m = d_m.cpu().numpy()
        assert (m[K:] == 12345).all()
        got = ext.decode_loop_proj_out(d_out.cpu().numpy(), n + 3)
        assert got["n"] == n and got["status"] == 0
        lp_same(got, m, want, "record form")


# ---- the patch association at the grid's edges -----------------------------------------------------------------------------------
class TestPatchesAtTheEdges:
    H, W, NF = 240, 320, 1300

    @pytest.fixture(scope="class")
    def ext(self, blob):
        e = SPExtractor(self.NF, self.H, self.W, blob, with_heat=False)
        yield e
        e.close()

    def test_positions_over_the_border_outside_and_not_finite(self, ext):
        e = pac.edges(self.H // 8, self.W // 8)
        want = oracle.match_patches(e["desc"], e["uv"], e["occ"], e["kp_desc"])
        assert (want[~e["inside"]] == -1).all() and (want[e["inside"]] >= 0).sum() >= 8
        assert np.array_equal(ext.match_patches(e["desc"], e["uv"], e["occ"], e["kp_desc"]), want)
        assert np.array_equal(patches_record(ext, e, record(ext, e["occ"], e["kp_desc"])), want)
        for i in range(len(e["uv"])):                                     # ... and each point alone, nothing taken before it
            one = {k: e[k][i:i + 1] for k in ("desc", "uv")}
            want1 = oracle.match_patches(one["desc"], one["uv"], e["occ"], e["kp_desc"])
            assert (want1[0] >= 0) == bool(e["inside"][i])
            assert np.array_equal(ext.match_patches(one["desc"], one["uv"], e["occ"], e["kp_desc"]), want1), e["uv"][i]

    def test_a_header_count_below_the_indices_in_the_grid(self, ext):
        e = pac.edges(self.H // 8, self.W // 8)
        g = pac.scale(1200, m=600, hc=self.H // 8, wc=self.W // 8, hot=100)
        for K in (700, 1, 0):
            want = oracle.match_patches(g["desc"], g["uv"], g["occ"], g["kp_desc"][:K])
            assert (g["occ"] >= K).sum() >= 500 and ((want >= 0).sum() >= 100 or K < 2)
            assert np.array_equal(patches_record(ext, g, record(ext, g["occ"], g["kp_desc"], K=K)), want), K
        want = oracle.match_patches(e["desc"], e["uv"], e["occ"], e["kp_desc"][:600])
        assert np.array_equal(patches_record(ext, e, record(ext, e["occ"], e["kp_desc"], K=600)), want)

    def test_max_dist_equal_to_a_candidates_distance(self, ext):
        g = pac.scale(1200, m=40, hc=self.H // 8, wc=self.W // 8, contention=0.0)
        d_rec = record(ext, g["occ"], g["kp_desc"])
        tried = 0
        for i in range(12):
            one = dict(desc=g["desc"][i:i + 1], uv=g["uv"][i:i + 1])
            near = oracle.match_patches(one["desc"], one["uv"], g["occ"], g["kp_desc"], max_dist=10.0)[0]   # the point alone
            if near < 0:
                continue
            d = pac.dist(one["desc"][0], g["kp_desc"][near])              # the nearest candidate's distance, the oracle's bits
            for md, hit in ((float(d), False), (float(np.nextafter(d, np.float32(np.inf))), True)):
                want = oracle.match_patches(one["desc"], one["uv"], g["occ"], g["kp_desc"], max_dist=md)
                assert (want[0] == near) == hit and (hit or want[0] == -1)
                assert np.array_equal(ext.match_patches(one["desc"], one["uv"], g["occ"], g["kp_desc"], md), want), (i, md)
                assert np.array_equal(patches_record(ext, one, d_rec, md), want), (i, md)
            tried += 1
        assert tried >= 8


# ---- the largest keypoint counts the claim stages serve, and one more -----------------------------------------------------------
class TestLimits:
    """Host-array forms on a 64 x 96 handle: the claim's LDS is sized by K, and only 96 of the K keypoints need a cell."""
    H, W = 64, 96

    @pytest.fixture(scope="class")
    def ext(self, blob):
        e = SPExtractor(100, self.H, self.W, blob, with_heat=False)
        yield e
        e.close()

    def test_no_handle_reaches_the_limits_through_its_records(self, blob):
        with pytest.raises(SpfeError, match="SPFE_EINVAL"):
            SPExtractor(10001, self.H, self.W, blob, with_heat=False)
        assert 10001 < min(PROJ_MAX_K, PATCH_MAX_K, LOOP_MAX_K)

    def test_projection_search_at_18200_keypoints_and_one_more(self, ext, pref):
        g = pjc.sparse(PROJ_MAX_K)
        for kw in pjc.MODES:
            want = pjc.run_ref(proj_ref, pref, g, **kw)
            proj_same(proj_host(ext, g, **kw), want, kw)
            assert want["n_matches"] >= 20 and want["kp_of_mp"].max() >= pjc.LDS_THRESHOLD
        g = pjc.sparse(PROJ_MAX_K + 1)
        with pytest.raises(SpfeError, match="SPFE_EINVAL.*too many"):
            proj_host(ext, g, **pjc.MODES[0])
        proj_same(proj_host(ext, pjc.sparse(2000), **pjc.MODES[0]), pjc.run_ref(proj_ref, pref, pjc.sparse(2000), **pjc.MODES[0]), "after")

    def test_patches_at_32764_keypoints_and_one_more(self, ext):
        g = pac.sparse(PATCH_MAX_K, self.H // 8, self.W // 8)
        want = oracle.match_patches(g["desc"], g["uv"], g["occ"], g["kp_desc"])
        assert (want >= 0).sum() >= 20 and want.max() >= PATCH_MAX_K - 3
        assert np.array_equal(ext.match_patches(g["desc"], g["uv"], g["occ"], g["kp_desc"]), want)
        g = pac.sparse(PATCH_MAX_K + 1, self.H // 8, self.W // 8)
        with pytest.raises(SpfeError, match="SPFE_EINVAL.*too many"):
            ext.match_patches(g["desc"], g["uv"], g["occ"], g["kp_desc"])
        g = pac.sparse(2000, self.H // 8, self.W // 8)                    # the refusal left nothing behind
        assert np.array_equal(ext.match_patches(g["desc"], g["uv"], g["occ"], g["kp_desc"]),
                              oracle.match_patches(g["desc"], g["uv"], g["occ"], g["kp_desc"]))

    def test_loop_points_at_32748_keypoints_and_one_more(self, ext, gref):
        g = gc.lp_sparse(LOOP_MAX_K)
        want = gc.lp_ref(gref, g)
        assert want["n_matched"] >= 20 and want["kp_of_mp"].max() >= LOOP_MAX_K - 3
        got = lp_host(ext, g)
        lp_same(got, got["matched"], want, "limit")
        g = gc.lp_sparse(LOOP_MAX_K + 1)
        with pytest.raises(SpfeError, match="SPFE_EINVAL.*too many"):
            lp_host(ext, g)
        g = gc.lp_sparse(2000)
        got = lp_host(ext, g)
        lp_same(got, got["matched"], gc.lp_ref(gref, g), "after")
