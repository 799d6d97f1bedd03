"""GPU: the loop-point projection, SPMatcher::SearchByProjectionLoop, on a resident keyframe record (spfe_search_loop_points,
spfe_search_loop_points_record_device: guided.hip) against the sequential loop of tests/guided_ref/guided_ref.c, which shares
include/spfe_guided_math.h with the kernels: every output, best_dist included, bit for bit — on the fixtures
tests/golden/loopproj_*.npz with f32 and bf16 rows; point counts around the claim workgroup's 1024 threads; candidate lists of more than 64
keypoints (th = 32); a contested chain
of 200 points (a round per point); chunked calls with `matched` carried; the bytes that are not written, the inputs,
`matched` changing only where the reference changes it, the refusals and an overflowed record."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "guided_ref"))
import guided_cases as gc  # noqa: E402
import guided_ref  # noqa: E402

from sp_orb_slam_amd import extractor as X  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import SPExtractor  # noqa: E402

pytestmark = pytest.mark.gpu
H, W, NF = 64, 96, 100
FILL = 0xA5
OUT = ("reason", "kp_of_mp", "matched_idx")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return guided_ref.build(tmp_path_factory.mktemp("guided_ref"))


@pytest.fixture(scope="module")
def exts():
    blob = weights.synthetic(7, "trackable")
    e = {False: SPExtractor(NF, H, W, blob, with_heat=False), True: SPExtractor(NF, H, W, blob, with_heat=False, desc_bf16=True),
         "big": SPExtractor(1299, 320, 416, blob, with_heat=False)}
    yield e
    for x in e.values():
        x.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def record(ext, g, K=None, status=0):
    L = ext.layout
    n = len(g["kp_xy"])
    K = n if K is None else K
    assert n <= L.kmax and g["occ"].shape == (ext.height // 8, ext.width // 8)
    b = np.zeros(ext.record_bytes(), np.uint8)
    b[L.off_hdr:L.off_hdr + 16].view(np.int32)[:] = [K, K, status, 0]
    b[L.off_xy:L.off_xy + 8 * n].view(np.float32)[:] = np.ascontiguousarray(g["kp_xy"], np.float32).reshape(-1)
    b[L.off_occ:L.off_occ + 2 * g["occ"].size].view(np.int16)[:] = np.ascontiguousarray(g["occ"], np.int16).reshape(-1)
    if ext.desc_bf16:
        b[L.off_desc:L.off_desc + 512 * n].view(np.uint16)[:] = guided_ref.to_bf16(g["kp_desc"]).reshape(-1)
    else:
        b[L.off_desc:L.off_desc + 1024 * n].view(np.float32)[:] = np.ascontiguousarray(g["kp_desc"], np.float32).reshape(-1)
    return dev(b)


def padded(ext, a, fill):
    out = np.full(ext.layout.kmax, fill, np.int32)
    out[:len(a)] = a
    return out


def dev_points(g, lo=0, hi=None):
    n = len(g["point_id"][lo:hi])
    return [dev(g[k][lo:hi] if n else np.zeros((1,) + g[k].shape[1:], g[k].dtype)) for k in gc.POINT_KEYS], n


def run(ext, g, d_rec=None, matched=None, lo=0, hi=None, n_cap=None, K=None, status=0, **kw):
    """spfe_search_loop_points_record_device -> (decoded block, raw block, matched [kmax] after the call); the inputs are checked
    to be unchanged, and the entries of matched at and beyond K (they hold 12345) too"""
    import torch
    rec = record(ext, g, K, status) if d_rec is None else d_rec
    rec0 = rec.cpu().numpy()
    K = len(g["kp_xy"]) if K is None else K
    m0 = padded(ext, (g["matched"] if matched is None else matched)[:K], 12345)
    d_m, d_S = dev(m0), dev(np.asarray(g["Scw"], np.float32).reshape(16))
    pts, n = dev_points(g, lo, hi)
    host = [t.cpu().numpy() for t in pts]
    cap = max(n, 1) if n_cap is None else n_cap
    d_out = torch.full((ext.loop_proj_out_bytes(cap),), FILL, dtype=torch.uint8, device="cuda")
    ext.search_loop_points_record_device(rec.data_ptr(), d_S.data_ptr(), d_m.data_ptr(), *[t.data_ptr() for t in pts], n, d_out.data_ptr(),
                                         *[float(v) for v in g["intr"]], n_cap=cap, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(rec.cpu().numpy(), rec0) and all(np.array_equal(t.cpu().numpy(), h) for t, h in zip(pts, host))
    m = d_m.cpu().numpy()
    assert (m[K:] == 12345).all()
    raw = d_out.cpu().numpy()
    return ext.decode_loop_proj_out(raw, cap), raw, m


def same(got, m, want, what):
    for k in OUT:
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    assert got["n_matched"] == want["n_matched"], what
    assert np.array_equal(got["best_dist"].view(np.uint32), want["best_dist"].view(np.uint32)), (what, "best_dist bits")
    assert np.array_equal(m[:len(want["matched"])], want["matched"]), (what, "matched")   # changed only where the reference changes it


def unwritten(raw, n, n_matched, cap):
    o = X.loop_proj_offsets(cap)
    assert (raw[12:64] == FILL).all()
    for lo, size, used, end in ((64, 4, n, o["best_dist"]), (o["best_dist"], 4, n, o["matched_idx"]), (o["matched_idx"], 4, n_matched, o["reason"]),
                                (o["reason"], 1, n, o["out_bytes"])):
        assert (raw[lo + size * used:end] == FILL).all(), lo


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", gc.LP_NAMES)
def test_both_forms_equal_the_sequential_loop_bit_for_bit(exts, ref, name, bf16):
    g = gc.lp_load(name)
    assert (int(g["H"]), int(g["W"])) == (H, W)
    ext = exts[bf16]
    want = gc.lp_ref(ref, g)
    assert gc.lp_differences(g, want) == []
    n = len(g["point_id"])
    got, raw, m = run(ext, g, n_cap=max(n, 1) + 3)
    same(got, m, want, (name, "record form"))
    assert got["n"] == n and got["status"] == 0
    unwritten(raw, n, got["n_matched"], max(n, 1) + 3)
    if not bf16:
        host = ext.search_loop_points(g["kp_xy"], g["occ"], g["kp_desc"], g["Scw"], g["matched"], *[g[k] for k in gc.POINT_KEYS],
                                      *[float(v) for v in g["intr"]])
        same(host, host["matched"], want, (name, "host form"))


@pytest.fixture(scope="module")
def big():
    return gc.lp_large()


@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 1300])
def test_point_counts_around_the_claim_workgroup(exts, ref, big, n):
    ext = exts["big"]
    want = gc.lp_ref(ref, big, hi=n)
    got, raw, m = run(ext, big, hi=n)
    same(got, m, want, n)
    unwritten(raw, n, got["n_matched"], max(n, 1))
    if n == 1300:
        print("1300: reasons", np.bincount(want["reason"], minlength=10)[1:], "matched", want["n_matched"])
        assert want["n_matched"] >= 300


def lp_dense(n=40, H=128, W=160, seed=5):
    """a keypoint in every cell of an H x W frame (the numbering is random) and n good points that project at least 44 px from
    the border; every point's row is near that of its nearest keypoint -> (case, uv [n][2] float64)"""
    rng = np.random.default_rng([seed, n])
    hc, wc = H // 8, W // 8
    K = hc * wc
    intr = (300.0, 300.0, W / 2 - 0.5, H / 2 - 0.25)
    fx, fy, cx, cy = intr
    occ = rng.permutation(K).astype(np.int16).reshape(hc, wc)
    kp = np.zeros((K, 2), np.float32)
    kp[occ.reshape(-1)] = np.stack([np.arange(K) % wc * 8 + rng.uniform(0.5, 7.5, K), np.arange(K) // wc * 8 + rng.uniform(0.5, 7.5, K)], 1)
    rows = (gc.unit_rows(rng, 1) + 0.3 * gc.unit_rows(rng, K)).astype(np.float32)
    uv = np.stack([rng.uniform(44, W - 44, n), rng.uniform(44, H - 44, n)], 1)
    near = np.array([np.argmin(((kp - p) ** 2).sum(1)) for p in uv])
    z = rng.uniform(2, 6, n)
    P = np.stack([(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, z], 1)
    dist = np.linalg.norm(P, axis=1)
    desc = rows[near] + rng.choice([0.05, 0.2, 0.4, 0.9], (n, 1)).astype(np.float32) * gc.unit_rows(rng, n)
    matched = np.where(rng.random(K) < 0.1, 900000 + np.arange(K), -1).astype(np.int32)
    return dict(kp_xy=kp, occ=occ, kp_desc=rows, Scw=np.diag([1.25, 1.25, 1.25, 1.0]).astype(np.float32), matched=matched,
                point_id=(1000 + np.arange(n)).astype(np.int32), xyz=P.astype(np.float32), normal=(P / dist[:, None] * 0.9).astype(np.float32),
                dist_range=np.stack([dist * 0.9, dist * 1.1], 1).astype(np.float32), desc=desc.astype(np.float32), flags=np.ones(n, np.uint8),
                intr=np.array(intr, np.float32), H=H, W=W), uv


def test_a_candidate_list_of_more_than_64_keypoints_spans_two_ballots(ref):
    """th = SPFE_PROJ_MAX_RADIUS on 16 x 20 cells that all hold a keypoint: a window has up to 11 x 11 cells (two passes of the
    walk) and holds more than 64 keypoints for some points (at most SPFE_PROJ_MAX_CAND = 121 by construction).  Every other
    point with such a list carries the row of the free keypoint that comes LAST in its list, so that matches come from behind
    the 64th candidate"""
    r = float(X.PROJ_MAX_RADIUS)
    g, uv = lp_dense()
    kp = g["kp_xy"].astype(np.float64)
    lists = []                                                            # the candidate lists: ix outer, iy inner
    for u, v in uv:
        k = np.flatnonzero((np.abs(kp[:, 0] - u) < r) & (np.abs(kp[:, 1] - v) < r))
        lists.append(k[np.lexsort((kp[k, 1] // 8, kp[k, 0] // 8))])
    sizes = np.array([len(k) for k in lists])
    assert (sizes > 64).any() and sizes.max() <= X.PROJ_MAX_CAND, sizes
    late = []
    for i in np.flatnonzero(sizes > 64)[::2]:
        k = [k for k in lists[i][64:] if g["matched"][k] < 0 and max(abs(kp[k, 0] - uv[i, 0]), abs(kp[k, 1] - uv[i, 1])) < r - 1]
        if k:
            g["desc"][i] = g["kp_desc"][k[-1]]
            late.append((i, k[-1]))
    want = gc.lp_ref(ref, g, th=r)
    n_late = sum(int(want["kp_of_mp"][i] == k) for i, k in late)
    print("th = 32: candidates per point", sizes, "reasons", np.bincount(want["reason"], minlength=10)[1:], "matched", want["n_matched"],
          "behind the 64th candidate", n_late)
    assert n_late >= 1 and want["n_matched"] >= 20
    ext = SPExtractor(g["kp_xy"].shape[0] - 1, g["H"], g["W"], weights.synthetic(7, "trackable"), with_heat=False)
    try:
        assert ext.layout.kmax == 320
        got, raw, m = run(ext, g, th=r)
        same(got, m, want, "th = 32")
        unwritten(raw, len(uv), got["n_matched"], len(uv))
    finally:
        ext.close()


def test_chunked_calls_with_matched_carried_equal_the_single_call(exts, ref, big):
    ext = exts["big"]
    one, _, m_one = run(ext, big)
    d_rec = record(ext, big)
    a, _, m_a = run(ext, big, d_rec=d_rec, hi=1024)
    b, _, m_b = run(ext, big, d_rec=d_rec, lo=1024, matched=m_a[:1300])
    for k in ("reason", "kp_of_mp", "best_dist"):
        assert np.array_equal(np.concatenate([a[k], b[k]]), one[k]), k
    assert np.array_equal(np.concatenate([a["matched_idx"], 1024 + b["matched_idx"]]), one["matched_idx"]) and np.array_equal(m_b, m_one)
    assert b["n"] == 276 and a["n_matched"] + b["n_matched"] == one["n_matched"]


def test_a_contested_chain_of_200_points_takes_a_round_per_point(exts, ref):
    """every point contests its predecessor's keypoint: the bound of n rounds is reached, and the loop ends by construction"""
    ext, c = exts["big"], gc.lp_chain()
    want = gc.lp_ref(ref, c)
    assert list(want["kp_of_mp"]) == list(range(200))
    got, _, m = run(ext, c)
    same(got, m, want, "chain")


def test_keypoint_counts_and_an_overflowed_record(exts, ref):
    """entries of the record, the grid and `matched` at and beyond K are ignored; SPFE_STATUS_COV_OVERFLOW is passed through"""
    ext = exts[False]
    g = gc.lp_load("chain")
    for K in (0, 1, 5, 10):
        got, _, m = run(ext, g, K=K)
        same(got, m, gc.lp_ref(ref, g, K=K), K)
    clean, raw0, _ = run(ext, g)
    over, raw1, m = run(ext, g, status=1)
    same(over, m, gc.lp_ref(ref, g), "overflowed")
    assert clean["status"] == 0 and over["status"] == 1 and np.array_equal(raw0[12:], raw1[12:]) and np.array_equal(raw0[:8], raw1[:8])


def test_invalid_arguments_return_before_any_launch(exts):
    import torch
    ext = exts[False]
    g = gc.lp_load("blocked")
    n, intr = len(g["point_id"]), [float(v) for v in g["intr"]]
    m0 = padded(ext, g["matched"], -1)
    d_rec, d_S, d_m = record(ext, g), dev(g["Scw"].reshape(16)), dev(m0)
    pts, _ = dev_points(g)
    d_out = torch.full((ext.loop_proj_out_bytes(8),), FILL, dtype=torch.uint8, device="cuda")
    q = lambda t: t.data_ptr()   # noqa: E731
    good = [q(d_rec), q(d_S), q(d_m)] + [q(t) for t in pts] + [n, q(d_out)]
    bad = []
    for i in list(range(9)) + [10]:                                        # every pointer
        a = list(good)
        a[i] = 0
        bad.append((a, {}))
    bad += [(good, dict(n_cap=n - 1)), (good, dict(n_cap=0)), (good, dict(n_cap=X.PROJ_MAX_POINTS + 1)), (good, dict(th=0.0)),
            (good, dict(th=float(X.PROJ_MAX_RADIUS) + 0.01)), (good, dict(th=float("nan")))]
    for v, kw in ((-1, {}), (X.PROJ_MAX_POINTS + 1, dict(n_cap=X.PROJ_MAX_POINTS + 1))):
        a = list(good)
        a[9] = v
        bad.append((a, kw))
    for a, kw in bad:
        with pytest.raises(X.SpfeError, match="SPFE_EINVAL"):
            ext.search_loop_points_record_device(*a, *intr, **kw)
    with pytest.raises(X.SpfeError, match="SPFE_EINVAL"):
        ext.search_loop_points(g["kp_xy"], g["occ"], g["kp_desc"], g["Scw"], g["matched"], *[g[k] for k in gc.POINT_KEYS], *intr, th=40.0)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == FILL).all() and np.array_equal(d_m.cpu().numpy(), m0)
    ext.search_loop_points_record_device(*good, *intr, th=float(X.PROJ_MAX_RADIUS), n_cap=8)     # the radius at the cap is served
    torch.cuda.synchronize()
    assert ext.decode_loop_proj_out(d_out.cpu().numpy(), 8)["n"] == n
