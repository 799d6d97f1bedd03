"""GPU: the Sim3 optimisation of a loop hypothesis (sp_orb_slam_amd/csrc/sim3opt.hip, spfe_optimize_sim3*) against the host
reference tests/sim3opt_ref/sim3opt_ref.c: every integer, verdict, iteration and trial count equal; the transform up to the
device's sin / cos / exp in the applied updates; Scw and matched bit for bit from the block's own S12 and matches12_out.

Measured on an MI355X (ROCm 7): the largest |S12 entry (device) - S12 entry (sim3opt_ref.c)| over the 13 fixtures, the record
test, the two capacity cases and the 16 distinct jobs of the batched test is 0.0 — every S12 and T12_out came out bit for bit
(MEASURED_S12).  The Jacobians hold no libm call, and in the applied updates the device's sin / cos / exp gave glibc's bits on
every argument these solves produced (a few general-branch updates per solve; the steps near the optimum fall into the branch
below eps, which has none).  The committed bound is 4 times the measured deviation, as for the CPU pair: 0.  A ROCm whose libm
differs in a last bit will fail here on S12 first (the noisy numeric Jacobian then amplifies that bit to some 1e-8 and may move
a trial count); the bound is then to be measured again, not guessed now."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("sim3opt_ref", "golden", "guided_ref"):
    sys.path.insert(0, os.path.join(ROOT, "tests", sub))
sys.path.insert(0, ROOT)
import guided_cases as gc  # noqa: E402
import make_golden_sim3opt as stmt  # noqa: E402
import sim3opt_ref  # noqa: E402

from sp_orb_slam_amd import extractor as X  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import SPExtractor  # noqa: E402
from tools import track_scene as ts  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ("clean", "outliers", "kept9", "kept10", "all_removed", "c128", "c129", "skipped", "fix_scale", "behind", "two_cameras",
         "rejected_run", "exact")
FILL = 0xA5
MEASURED_S12 = 0.0
S12_BOUND = 4 * MEASURED_S12
H, W = 64, 96


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return sim3opt_ref.build(tmp_path_factory.mktemp("sim3opt_ref"))


@pytest.fixture(scope="module")
def exts():
    blob = weights.synthetic(7, "trackable")
    e = {"host": SPExtractor(100, H, W, blob, with_heat=False), "small": SPExtractor(79, H, W, blob, with_heat=False)}
    yield e
    for x in e.values():
        x.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def load(name):
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "sim3opt_%s.npz" % name)))


def intr_of(g):
    v = [float(x) for x in g["intr"]]
    return v[:4], v[4:]


def same(got, want, Tcw2, mp2, ref, what):
    """the block `got` (decoded) against the reference's result `want`; -> the largest S12 deviation"""
    for k in ("n_corr", "n_bad", "n_in", "accepted"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("matches12_out", "matched", "verdict", "iterations", "trials"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    dev_s = float(np.abs(got["S12"] - want["S12"]).max())
    dev_t = float(np.abs(got["T12_out"].astype(np.float64) - want["T12_out"].astype(np.float64)).max())
    print("%s: n_corr %d n_bad %d n_in %d iterations %s trials %s |S12 - ref| %.3e |T12_out - ref| %.3e" %
          (what, got["n_corr"], got["n_bad"], got["n_in"], got["iterations"].tolist(), got["trials"].tolist(), dev_s, dev_t))
    assert dev_s <= S12_BOUND, (what, dev_s)
    # T12_out is the cast of S12 (asserted below): beyond S12's bound it may differ by one float32 rounding, and by nothing at 0
    rounding = 2.0 ** -24 * max(1.0, float(np.abs(want["T12_out"]).max())) if S12_BOUND > 0 else 0.0
    assert dev_t <= S12_BOUND + rounding, (what, dev_t)
    assert np.array_equal(got["T12_out"], got["S12"].astype(np.float32))
    # Scw and matched, bit for bit, from the block's own S12 and matches12_out
    assert np.array_equal(got["Scw"].view(np.uint32), sim3opt_ref.scw_of(ref, got["S12"], Tcw2).view(np.uint32)), what
    k2 = got["matches12_out"]
    mp2 = np.asarray(mp2)
    ok = (k2 >= 0) & (k2 < len(mp2))
    assert np.array_equal(got["matched"], np.where(ok, mp2[np.clip(k2, 0, max(len(mp2) - 1, 0))] if len(mp2) else -1, -1)), what
    return dev_s


def host_form(ext, g, **kw):
    i1, i2 = intr_of(g)
    raw, kcap = ext.optimize_sim3(g["kp_xy1"], g["mp1"], g["kp_xy2"], g["mp2"], g["xyz"], g["flags"], g["Tcw1"], g["Tcw2"], g["T12"],
                                  g["matches12"], i1, i2, fix_scale=int(g["fix_scale"]), fill=FILL, **kw)
    o = X.sim3opt_offsets(kcap)
    # the padding keeps the caller's bytes
    assert (raw[36:64] == FILL).all() and (raw[220:224] == FILL).all() and (raw[288:320] == FILL).all() and (raw[o["verdict"] + kcap:] == FILL).all()
    return ext.decode_sim3opt_out(raw, kcap)


@pytest.mark.parametrize("name", NAMES)
def test_host_form_on_every_fixture(exts, ref, name):
    g = load(name)
    i1, i2 = intr_of(g)
    want = sim3opt_ref.solve(ref, g, sim3opt_ref.params(i1, i2, fix_scale=int(g["fix_scale"])))
    got = host_form(exts["host"], g)
    same(got, want, g["Tcw2"], g["mp2"], ref, name)
    assert got["status"] == 0
    if name in ("kept9", "all_removed"):   # the input echoed bit for bit
        assert got["T12_out"].tobytes() == g["T12"].tobytes() and got["S12"].tobytes() == g["T12"].astype(np.float64).tobytes()
        assert got["n_in"] == 0 and got["accepted"] == 0 and (got["matches12_out"][got["verdict"] == X.SIM3OPT_REMOVED] == -1).all()


def big_case(C, K, seed=5):
    """C correspondences among K1 = K2 = K keypoints, 8 % of them gross"""
    return stmt.make_scene(seed, C, n_out=C // 12, extra=K - C)


def test_both_sides_of_the_lds_capacity(exts, ref):
    """K1 = K2 = 3800: the per-keypoint state leaves room for the edge data of fewer correspondences than there are keypoints;
    exactly the capacity is staged in LDS, one more is read from the scratch array on every evaluation."""
    ext, K = exts["host"], 3800
    cap = ext.sim3opt_lds_edge_capacity(K)
    assert 256 < cap < K - 1, cap
    assert ext.sim3opt_lds_edge_capacity(101) == 101 and ext.sim3opt_lds_edge_capacity(32768) == -1
    for C in (cap, cap + 1):
        g = big_case(C, K)
        i1, i2 = intr_of(g)
        want = sim3opt_ref.solve(ref, g, sim3opt_ref.params(i1, i2))
        assert want["n_corr"] == C and want["n_bad"] > 0 and want["n_in"] > 0.8 * C and want["chi2_margin"] >= 1e-5
        same(host_form(ext, g), want, g["Tcw2"], g["mp2"], ref, "capacity %d%+d" % (cap, C - cap))


# ---- the record form on real records ----------------------------------------------------------------------------------------
def test_record_form_on_real_records(ref):
    import torch
    Hh, Ww, nf = 480, 752, 1000
    ext = SPExtractor(nf, Hh, Ww, weights.synthetic(7, "trackable"), max_batch=2, with_heat=False)
    try:
        world = ts.texture(21, *ts.world_size(Hh, Ww))
        imgs = torch.from_numpy(np.stack([ts.frame(world, k, Hh, Ww) for k in (3, 5)])).cuda()
        rb, kmax = ext.record_bytes(), ext.layout.kmax
        d_recs = torch.zeros(2 * rb, dtype=torch.uint8, device="cuda")
        t = ext.extract_batch_device(imgs.data_ptr(), 2, d_recs.data_ptr(), 0)
        ext.wait_records(t, 0)
        torch.cuda.synchronize()
        host = d_recs.cpu().numpy()
        r1, r2 = ext.view_record(host[:rb]), ext.view_record(host[rb:])
        assert r1.K > 500 and r2.K > 500
        # points at a known Sim3: the point keypoint k2 holds projects to obs1 through S12, the one k1 holds to obs2 through
        # its inverse; 15 % displaced grossly; the start value perturbed
        rng = np.random.default_rng(3)
        intr = stmt.INTR
        C = 400
        k1s, k2s = np.sort(rng.permutation(r1.K)[:C]), rng.permutation(r2.K)[:C]
        St = stmt.expm(stmt.hat(np.r_[0.03, -0.06, 0.02, 0.3, -0.1, 0.2, np.log(1.2)]))
        Tcw1, Tcw2 = stmt.small_pose(rng), stmt.small_pose(rng)
        back = lambda uv, z: np.c_[(uv[:, 0] - intr[2]) / intr[0] * z, (uv[:, 1] - intr[3]) / intr[1] * z, z]   # noqa: E731
        to = lambda M, P: (M[:3, :3] @ P.T).T + M[:3, 3]   # noqa: E731
        P2 = to(np.linalg.inv(St), back(r1.kp_xy[k1s].astype(np.float64), rng.uniform(3, 7, C)))    # held by k2, seen at obs1
        P1 = to(St, back(r2.kp_xy[k2s].astype(np.float64), rng.uniform(3, 7, C)))                   # held by k1, seen at obs2
        gross = rng.random(C) < 0.15
        P2[gross] += rng.normal(0, 0.4, (int(gross.sum()), 3))
        xyz = np.concatenate([to(np.linalg.inv(Tcw1.astype(np.float64)), P1), to(np.linalg.inv(Tcw2.astype(np.float64)), P2)]).astype(np.float32)
        flags = np.ones(2 * C, np.uint8)
        mp1, mp2, m12 = np.full(kmax, -1, np.int32), np.full(kmax, -1, np.int32), np.full(kmax, -1, np.int32)
        mp1[k1s], mp2[k2s], m12[k1s] = np.arange(C), C + np.arange(C), k2s
        S0 = stmt.expm(stmt.hat(np.r_[rng.normal(0, 0.01, 3), rng.normal(0, 0.04, 3), 0.03])) @ St
        T12 = stmt.T12_of(S0).astype(np.float32)
        d = [dev(a) for a in (mp1, mp2, xyz, flags, Tcw1.reshape(16), Tcw2.reshape(16), T12, m12)]
        d_out = torch.full((ext.sim3opt_out_bytes() + 64,), FILL, dtype=torch.uint8, device="cuda")
        q = lambda t: t.data_ptr()   # noqa: E731
        ext.optimize_sim3_record_device(q(d_recs), q(d_recs) + rb, q(d[0]), q(d[1]), q(d[2]), q(d[3]), 2 * C, q(d[4]), q(d[5]), q(d[6]),
                                        q(d[7]), q(d_out), intr)
        torch.cuda.synchronize()
        raw = d_out.cpu().numpy()
        assert (raw[-64:] == FILL).all() and np.array_equal(d_recs.cpu().numpy(), host)
        got = ext.decode_sim3opt_out(raw[:-64], kmax)
        case = dict(kp_xy1=r1.kp_xy, kp_xy2=r2.kp_xy, mp1=mp1[:r1.K], mp2=mp2[:r2.K], xyz=xyz, flags=flags, Tcw1=Tcw1, Tcw2=Tcw2,
                    T12=T12, matches12=m12[:r1.K])
        want = sim3opt_ref.solve(ref, case, sim3opt_ref.params(intr))
        assert want["chi2_margin"] >= 1e-5
        kc = max(r1.K, r2.K)
        for k in ("matches12_out", "matched", "verdict"):   # the reference's arrays over max(K1, K2), the block's over kmax
            assert (got[k][kc:] == (0 if k == "verdict" else -1)).all()
            got[k] = got[k][:kc]
        same(got, want, Tcw2, mp2[:r2.K], ref, "records")
        assert got["n_corr"] == C and got["n_in"] >= 0.7 * got["n_corr"] and got["accepted"] == 1 and got["n_bad"] >= 0.1 * C
        assert np.abs(got["S12"] - stmt.T12_of(St)).max() < 1e-3
    finally:
        ext.close()


# ---- the batched form behind verify and guided match ------------------------------------------------------------------------
def record(ext, t):
    L = ext.layout
    n = len(t["kp_xy"])
    b = np.zeros(ext.record_bytes(), np.uint8)
    b[L.off_hdr:L.off_hdr + 16].view(np.int32)[:] = [n, n, 0, 0]
    b[L.off_xy:L.off_xy + 8 * n].view(np.float32)[:] = np.ascontiguousarray(t["kp_xy"], np.float32).reshape(-1)
    b[L.off_occ:L.off_occ + 2 * t["occ"].size].view(np.int16)[:] = np.ascontiguousarray(t["occ"], np.int16).reshape(-1)
    b[L.off_desc:L.off_desc + 1024 * n].view(np.float32)[:] = np.ascontiguousarray(t["kp_desc"], np.float32).reshape(-1)
    return dev(b)


def padded(ext, a, fill=-1):
    out = np.full(ext.layout.kmax, fill, np.int32)
    out[:len(a)] = a
    return out


N_HYP = 8


@pytest.fixture(scope="module")
def chain(exts):
    """verify (two candidates: the second keyframe twice, candidate 0 holding fewer points) and the guided match of 32 jobs on
    the generated 80-keypoint case of tests/guided_ref/guided_cases.py; a second verify whose candidate 0 holds no point"""
    import torch
    ext = exts["small"]
    c = gc.large(K=80, H=H, W=W, seed=3, n_seed=12)
    kmax = ext.layout.kmax
    assert kmax == 80
    q = lambda t: t.data_ptr()   # noqa: E731
    out = {}
    for key, empty_first in (("full", False), ("empty", True)):
        rng = np.random.default_rng(17)
        mp2 = np.stack([padded(ext, c["kf2"]["kf_mp"])] * 2)
        mp2[0, rng.random(kmax) < (1.0 if empty_first else 0.2)] = -1
        rnd = rng.integers(0, 1 << 32, (2, N_HYP, 3), dtype=np.uint64).astype(np.uint32)
        T = np.eye(4, dtype=np.float32).reshape(16)
        d = dict(rec1=record(ext, c["kf1"]), rec2=[record(ext, c["kf2"]), record(ext, c["kf2"])], mp1=dev(padded(ext, c["kf1"]["kf_mp"])),
                 mp2=dev(mp2), T1=dev(T), T2=dev(np.stack([T, T])), rnd=dev(rnd),
                 map=[dev(c[k]) for k in gc.MAP_KEYS], match12=torch.zeros(2 * kmax, dtype=torch.int32, device="cuda"),
                 nm=torch.zeros(2, dtype=torch.int32, device="cuda"),
                 ver=torch.full((2 * ext.sim3_out_bytes(N_HYP),), FILL, dtype=torch.uint8, device="cuda"), mp2_host=mp2)
        ext.loop_verify_records_device(q(d["rec1"]), [q(r) for r in d["rec2"]], q(d["mp1"]), q(d["mp2"]), q(d["map"][0]), q(d["map"][1]),
                                       len(c["flags"]), q(d["T1"]), q(d["T2"]), q(d["rnd"]), N_HYP, q(d["match12"]), q(d["nm"]),
                                       q(d["ver"]), c["intr"], min_inliers=12)
        torch.cuda.synchronize()
        ob = ext.sim3_out_bytes(N_HYP)
        raw = d["ver"].cpu().numpy()
        d["blocks"] = [ext.decode_sim3_out(raw[j * ob:(j + 1) * ob], kmax, N_HYP) for j in range(2)]
        out[key] = d
    return ext, c, out


def guided(ext, c, d, jobs):
    import torch
    q = lambda t: t.data_ptr()   # noqa: E731
    d_out = torch.full((len(jobs) * ext.guided_out_bytes(),), FILL, dtype=torch.uint8, device="cuda")
    ext.loop_guided_match_records_device(q(d["rec1"]), [q(r) for r in d["rec2"]], jobs, q(d["mp1"]), q(d["mp2"]), *[q(t) for t in d["map"]],
                                         len(c["flags"]), q(d["T1"]), q(d["T2"]), q(d["match12"]), q(d["ver"]), N_HYP, q(d_out), c["intr"])
    torch.cuda.synchronize()
    return d_out


def optimise(ext, c, d, jobs, d_guided, d_out=None, **kw):
    import torch
    q = lambda t: t.data_ptr()   # noqa: E731
    sb = ext.sim3opt_out_bytes()
    if d_out is None:
        d_out = torch.full((len(jobs) * sb + 64,), FILL, dtype=torch.uint8, device="cuda")
    ext.loop_optimize_sim3_records_device(q(d["rec1"]), [q(r) for r in d["rec2"]], jobs, q(d["mp1"]), q(d["mp2"]), q(d["map"][0]),
                                          q(d["map"][1]), len(c["flags"]), q(d["T1"]), q(d["T2"]), q(d["ver"]), N_HYP, q(d_guided),
                                          q(d_out), c["intr"], **kw)
    torch.cuda.synchronize()
    return d_out


def jobs_of(blocks, n_jobs):
    rets = [(j, int(h)) for j, b in enumerate(blocks) for h in b["return_idx"]]
    assert rets, "no hypothesis returns"
    if n_jobs == 1:
        return [rets[0]]
    return ((rets + [(1, 0), (0, 7), (0, 0), (1, 7)] + [(j, h) for h in range(N_HYP) for j in (1, 0)]) * 4)[:n_jobs]


@pytest.mark.parametrize("n_jobs", [1, 2, 32])
def test_batched_form_equals_the_record_form_byte_for_byte(chain, ref, n_jobs):
    import torch
    ext, c, ds = chain
    d = ds["full"]
    kmax, sb, gb = ext.layout.kmax, ext.sim3opt_out_bytes(), ext.guided_out_bytes()
    jobs = jobs_of(d["blocks"], n_jobs)
    d_guided = guided(ext, c, d, jobs)
    g_before = d_guided.cpu().numpy().copy()
    raw = optimise(ext, c, d, jobs, d_guided, min_inliers=5).cpu().numpy()
    assert (raw[-64:] == FILL).all() and np.array_equal(d_guided.cpu().numpy(), g_before)
    q = lambda t: t.data_ptr()   # noqa: E731
    seen, best = {}, 0
    for q_, (j, h) in enumerate(jobs):
        got = raw[q_ * sb:(q_ + 1) * sb]
        if (j, h) not in seen:   # the record form, fed with the hypothesis and the guided matches decoded on the host
            gd = ext.decode_guided_out(g_before[q_ * gb:(q_ + 1) * gb], kmax, 80, 80)
            T12 = d["blocks"][j]["T12"][h]
            d_single = torch.full((sb,), FILL, dtype=torch.uint8, device="cuda")
            d_T12, d_m12 = dev(T12), dev(gd["matches12"])
            ext.optimize_sim3_record_device(q(d["rec1"]), q(d["rec2"][j]), q(d["mp1"]), q(d["mp2"]) + 4 * kmax * j, q(d["map"][0]),
                                            q(d["map"][1]), len(c["flags"]), q(d["T1"]), q(d["T2"]) + 64 * j, q(d_T12),
                                            q(d_m12), q(d_single), c["intr"], min_inliers=5)
            torch.cuda.synchronize()
            seen[(j, h)] = d_single.cpu().numpy()
            r = ext.decode_sim3opt_out(seen[(j, h)], kmax)
            case = dict(kp_xy1=c["kf1"]["kp_xy"], kp_xy2=c["kf2"]["kp_xy"], mp1=c["kf1"]["kf_mp"], mp2=d["mp2_host"][j][:80],
                        xyz=c["xyz"], flags=c["flags"], Tcw1=np.eye(4), Tcw2=np.eye(4), T12=T12, matches12=gd["matches12"][:80])
            i = [float(v) for v in c["intr"]]
            want = sim3opt_ref.solve(ref, case, sim3opt_ref.params(i, min_inliers=5))
            if want["chi2_margin"] >= 1e-5 and np.isfinite(want["S12"]).all():
                same(r, want, np.eye(4), d["mp2_host"][j][:80], ref, "job (%d, %d)" % (j, h))
            best = max(best, r["n_in"])
        assert np.array_equal(got, seen[(j, h)]), (q_, j, h)
    print("jobs", len(jobs), "distinct", len(seen), "most inliers", best)
    assert best >= 10


def test_a_job_that_was_not_evaluated_gives_the_empty_block(chain):
    ext, c, ds = chain
    d = ds["empty"]
    kmax = ext.layout.kmax
    assert d["blocks"][0]["best_h"] == -1 and d["blocks"][1]["best_h"] >= 0
    jobs = [(0, 3), (1, 3)]
    d_guided = guided(ext, c, d, jobs)
    raw = optimise(ext, c, d, jobs, d_guided).cpu().numpy()
    sb, o = ext.sim3opt_out_bytes(), X.sim3opt_offsets(kmax)
    b = raw[:sb]
    assert b[:36].view(np.int32).tolist() == [0] * 8 + [X.SIM3OPT_STATUS_NOT_EVALUATED]
    assert (b[o["matches12"]:o["verdict"]].view(np.int32) == -1).all()
    assert (b[36:o["matches12"]] == FILL).all() and (b[o["verdict"]:] == FILL).all()   # S12, T12_out, Scw, verdict: not written
    assert raw[sb:2 * sb][32:36].view(np.int32)[0] == 0 and (raw[-64:] == FILL).all()


def test_the_block_feeds_the_loop_point_search_in_place(chain):
    """Scw and matched of the accepted job, as pointers into its block, are the d_Scw and d_matched of the loop-point search:
    the same result as from host copies of the two arrays."""
    import torch
    ext, c, ds = chain
    d = ds["full"]
    kmax, sb = ext.layout.kmax, ext.sim3opt_out_bytes()
    jobs = jobs_of(d["blocks"], 32)
    d_out = optimise(ext, c, d, jobs, guided(ext, c, d, jobs), min_inliers=5)
    raw = d_out.cpu().numpy()
    blocks = [ext.decode_sim3opt_out(raw[i * sb:(i + 1) * sb], kmax) for i in range(len(jobs))]
    acc = [i for i, b in enumerate(blocks) if b["accepted"]]
    assert acc, [b["n_in"] for b in blocks]
    a = max(acc, key=lambda i: blocks[i]["n_in"])
    o = X.sim3opt_offsets(kmax)
    n = len(c["flags"])
    rng = np.random.default_rng(2)
    normal = rng.standard_normal((n, 3)).astype(np.float32)
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    pts = [dev(v) for v in (np.arange(n, dtype=np.int32), c["xyz"], normal, c["dist_range"], c["desc"], c["flags"])]
    q = lambda t: t.data_ptr()   # noqa: E731
    i = [float(v) for v in c["intr"]]
    res = []
    d_block = d_out.clone()
    d_S, d_m = dev(blocks[a]["Scw"].reshape(16)), dev(blocks[a]["matched"])
    for p_S, p_m, read in ((q(d_block) + a * sb + o["Scw"], q(d_block) + a * sb + o["matched"],
                            lambda: d_block.cpu().numpy()[a * sb + o["matched"]:a * sb + o["verdict"]].view(np.int32).copy()),
                           (q(d_S), q(d_m), lambda: d_m.cpu().numpy())):
        d_lp = torch.full((ext.loop_proj_out_bytes(n),), FILL, dtype=torch.uint8, device="cuda")
        ext.search_loop_points_record_device(q(d["rec1"]), p_S, p_m, *[q(t) for t in pts], n, q(d_lp), *i[:4])
        torch.cuda.synchronize()
        res.append((d_lp.cpu().numpy(), read()))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    lp = ext.decode_loop_proj_out(res[0][0], n)
    print("accepted job %d (n_in %d): the loop-point search matched %d of %d points" % (a, blocks[a]["n_in"], lp["n_matched"], n))
    after = d_block.cpu().numpy()
    keep = np.ones(len(after), bool)
    keep[a * sb + o["matched"]:a * sb + o["verdict"]] = False
    assert np.array_equal(after[keep], raw[keep])   # the search wrote nothing else of the blocks


def test_refusals_leave_the_output_untouched(chain):
    import torch
    ext, c, ds = chain
    d = ds["full"]
    jobs = jobs_of(d["blocks"], 2)
    d_guided = guided(ext, c, d, jobs)
    q = lambda t: t.data_ptr()   # noqa: E731
    sb = ext.sim3opt_out_bytes()
    d_out = torch.full((33 * sb,), FILL, dtype=torch.uint8, device="cuda")
    good = [q(d["rec1"]), [q(r) for r in d["rec2"]], jobs, q(d["mp1"]), q(d["mp2"]), q(d["map"][0]), q(d["map"][1]), len(c["flags"]),
            q(d["T1"]), q(d["T2"]), q(d["ver"]), N_HYP, q(d_guided), q(d_out)]
    bad = []
    for i in (0, 3, 4, 5, 6, 8, 9, 10, 12, 13):   # every pointer
        a = list(good)
        a[i] = 0
        bad.append((a, {}))
    bad.append((good[:1] + [[q(d["rec2"][0]), 0]] + good[2:], {}))
    for jb in ([(0, 0)] * 33, [(0, N_HYP)], [(2, 0)], [(0, -1)], []):
        bad.append((good[:2] + [jb] + good[3:], {}))
    for nn in (-1, X.PROJ_MAX_POINTS + 1):
        bad.append((good[:7] + [nn] + good[8:], {}))
    bad += [(good, dict(iterations=0)), (good[:11] + [0] + good[12:], {}), (good[:11] + [X.SIM3_MAX_HYPOTHESES + 1] + good[12:], {})]
    for a, kw in bad:
        with pytest.raises(X.SpfeError, match="SPFE_EINVAL"):
            ext.loop_optimize_sim3_records_device(*a, c["intr"], **kw)
    single = [q(d["rec1"]), q(d["rec2"][0]), q(d["mp1"]), q(d["mp2"]), q(d["map"][0]), q(d["map"][1]), len(c["flags"]), q(d["T1"]),
              q(d["T2"]), q(d["T1"]), q(d["match12"]), q(d_out)]
    for i in (0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11):
        a = list(single)
        a[i] = 0
        with pytest.raises(X.SpfeError, match="SPFE_EINVAL"):
            ext.optimize_sim3_record_device(*a, c["intr"])
    with pytest.raises(X.SpfeError, match="SPFE_EINVAL"):
        ext.optimize_sim3_record_device(*single, c["intr"], iterations=0)
    g = load("clean")
    i1, i2 = intr_of(g)
    with pytest.raises(X.SpfeError, match="SPFE_EINVAL"):
        ext.optimize_sim3(g["kp_xy1"], g["mp1"], g["kp_xy2"], g["mp2"], g["xyz"], g["flags"], g["Tcw1"], g["Tcw2"], g["T12"],
                          g["matches12"], i1, i2, iterations=0)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == FILL).all()
