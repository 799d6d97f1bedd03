"""GPU: the loop closer's guided match, SPMatcher::SearchBySim3Override, on resident keyframe records (spfe_search_by_sim3,
spfe_search_by_sim3_record_device, spfe_loop_guided_match_records_device: guided.hip) against the host reference
tests/guided_ref/guided_ref.c, which shares include/spfe_guided_math.h with the kernels: every output, the distances included,
bit for bit — on the fixtures tests/golden/guided_*.npz laid out as records by spfe_get_record_layout, with f32 and with bf16
descriptor rows; the batched form on the real output of spfe_loop_verify_records_device against the single form fed from
decode_sim3_out, byte for byte, with 1 and 32 jobs; keypoint counts around a wavefront and at kmax; windows of more than 64 cells (th = 32); 1300 keypoints (beyond one
1024-row chunk of the agree kernel); the bytes that are not written, the inputs, the refusals and overflowed records."""
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
H, W, NF = 64, 96, 100          # the fixtures' frame; kmax = 101
FILL = 0xA5
INTS = ("match1", "match2", "matches12", "reason1", "reason2")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return guided_ref.build(tmp_path_factory.mktemp("guided_ref"))


@pytest.fixture(scope="module")
def exts():
    blob = weights.synthetic(7, "trackable")
    e = {False: SPExtractor(NF, H, W, blob, with_heat=False), True: SPExtractor(NF, H, W, blob, with_heat=False, desc_bf16=True),
         "small": SPExtractor(79, H, W, blob, with_heat=False)}          # kmax = 80 <= the frame's 96 cells: K = kmax can occur
    yield e
    for x in e.values():
        x.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def record(ext, t, K=None, status=0):
    """a keyframe (kp_xy, occ, kp_desc f32) as one record of the handle's layout, on the device; K: the header's count"""
    L = ext.layout
    n = len(t["kp_xy"])
    K = n if K is None else K
    assert n <= L.kmax and t["occ"].shape == (ext.height // 8, ext.width // 8)
    b = np.zeros(ext.record_bytes(), np.uint8)
    b[L.off_hdr:L.off_hdr + 16].view(np.int32)[:] = [K, K, status, 0]
    b[L.off_xy:L.off_xy + 8 * n].view(np.float32)[:] = np.ascontiguousarray(t["kp_xy"], np.float32).reshape(-1)
    b[L.off_occ:L.off_occ + 2 * t["occ"].size].view(np.int16)[:] = np.ascontiguousarray(t["occ"], np.int16).reshape(-1)
    if ext.desc_bf16:
        b[L.off_desc:L.off_desc + 512 * n].view(np.uint16)[:] = guided_ref.to_bf16(t["kp_desc"]).reshape(-1)
    else:
        b[L.off_desc:L.off_desc + 1024 * n].view(np.float32)[:] = np.ascontiguousarray(t["kp_desc"], np.float32).reshape(-1)
    return dev(b)


def padded(ext, a, fill=-1):
    out = np.full(ext.layout.kmax, fill, np.int32)
    out[:len(a)] = a
    return out


def dev_map(m):
    """the map arrays on the device (one dummy row when there is none: the pointers are not read)"""
    n = len(m["flags"])
    return [dev(m[k] if n else np.zeros((1,) + m[k].shape[1:], m[k].dtype)) for k in gc.MAP_KEYS]


class Case:
    """the inputs of one guided match on the device, and a check that the call left them alone"""

    def __init__(self, ext, kf1, kf2, m, T12, seed12, K1=None, K2=None, status=(0, 0)):
        self.ext, self.n = ext, len(m["flags"])
        self.host = [padded(ext, kf1["kf_mp"]), padded(ext, kf2["kf_mp"]), np.asarray(kf1["Tcw"], np.float32).reshape(16),
                     np.asarray(kf2["Tcw"], np.float32).reshape(16), np.asarray(T12, np.float32).reshape(13), padded(ext, seed12, fill=7)]
        self.rec = [record(ext, kf1, K1, status[0]), record(ext, kf2, K2, status[1])]
        self.rec_host = [r.cpu().numpy() for r in self.rec]
        self.d = [dev(a) for a in self.host]
        self.map_host = [np.ascontiguousarray(m[k]) for k in gc.MAP_KEYS]
        self.map = dev_map(m)

    def args(self, d_out):
        q = lambda t: t.data_ptr()   # noqa: E731
        return [q(self.rec[0]), q(self.rec[1]), q(self.d[0]), q(self.d[1])] + [q(t) for t in self.map] + \
            [self.n, q(self.d[2]), q(self.d[3]), q(self.d[4]), q(self.d[5]), q(d_out)]

    def run(self, intr1, intr2=None, **kw):
        """spfe_search_by_sim3_record_device -> raw block"""
        import torch
        d_out = torch.full((self.ext.guided_out_bytes(),), FILL, dtype=torch.uint8, device="cuda")
        self.ext.search_by_sim3_record_device(*self.args(d_out), intr1, intr2, **kw)
        torch.cuda.synchronize()
        self.unchanged()
        return d_out.cpu().numpy()

    def unchanged(self):
        for t, h in zip(self.d + self.rec, self.host + self.rec_host):
            assert np.array_equal(t.cpu().numpy(), h)
        if self.n:
            for t, h in zip(self.map, self.map_host):
                assert np.array_equal(t.cpu().numpy(), h)


def same(got, want, what):
    for k in INTS:
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    for k in guided_ref.COUNTS:
        assert got[k] == want[k], (what, k)
    for k in ("dist1", "dist2"):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (what, k + " bits")


def unwritten(raw, kmax, K1, K2):
    """entries at and beyond K1 / K2 and the padding keep the fill; matches12 is written over all kmax entries"""
    o = X.guided_offsets(kmax)
    assert (raw[16:64] == FILL).all()
    for lo, size, used, end in ((o["match1"], 4, K1, o["match2"]), (o["match2"], 4, K2, o["dist1"]), (o["dist1"], 4, K1, o["dist2"]),
                                (o["dist2"], 4, K2, o["matches12"]), (o["reason1"], 1, K1, o["reason2"]),
                                (o["reason2"], 1, K2, o["out_bytes"])):
        assert (raw[lo + size * used:end] == FILL).all(), lo
    assert (raw[o["matches12"] + 4 * K1:o["reason1"]].view(np.int32) == -1).all()


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", gc.NAMES)
def test_all_forms_equal_the_host_reference_bit_for_bit(exts, ref, name, bf16):
    g = gc.load(name)
    assert (int(g["H"]), int(g["W"])) == (H, W)
    ext = exts[bf16]
    kmax = ext.layout.kmax
    kf1, kf2 = gc.keyframes(g)
    K1, K2 = len(kf1["kp_xy"]), len(kf2["kp_xy"])
    m = {k: g[k] for k in gc.MAP_KEYS}
    want = gc.run_ref(ref, g, kcap=kmax)                                  # (the fixtures' rows are bf16 values: both see the same numbers)
    assert gc.differences(g, want) == []
    prm = gc.prm_of(g)
    raw = Case(ext, kf1, kf2, m, g["T12"], g["seed12"]).run(g["intr1"], g["intr2"], **prm)
    got = ext.decode_guided_out(raw, kmax, K1, K2)
    same(got, want, (name, "record form"))
    assert got["status"] == 0
    unwritten(raw, kmax, K1, K2)
    if not bf16:
        hraw, kcap = ext.search_by_sim3(kf1, kf2, *[m[k] for k in gc.MAP_KEYS], kf1["Tcw"], kf2["Tcw"], g["T12"], g["seed12"], g["intr1"],
                                        g["intr2"], fill=FILL, **prm)
        assert kcap == max(K1, K2, 1)
        same(ext.decode_guided_out(hraw, kcap, K1, K2), gc.run_ref(ref, g), (name, "host form"))
        unwritten(hraw, kcap, K1, K2)


def ref_case(ref, c, K1=None, K2=None, kcap=None, **kw):
    kf1 = c["kf1"] if K1 is None else gc.cut(c["kf1"], K1)
    kf2 = c["kf2"] if K2 is None else gc.cut(c["kf2"], K2)
    return guided_ref.search(ref, kf1, kf2, c["xyz"], c["flags"], c["dist_range"], c["desc"], kf1["Tcw"], kf2["Tcw"], c["T12"], c["seed12"],
                             c["intr"], c["W"], c["H"], kcap=kcap, **kw)


@pytest.fixture(scope="module")
def frame80():
    return gc.large(K=80, H=H, W=W, seed=3, n_seed=12)


@pytest.mark.parametrize("K", [0, 1, 63, 64, 65, 80])
def test_keypoint_counts_around_a_wavefront_and_at_kmax(exts, ref, frame80, K):
    """the header of one record says K, the other record is full (80 = kmax): entries at and beyond K are ignored, in the
    record, the holder array and the grid, and are not written"""
    ext, c = exts["small"], frame80
    kmax = ext.layout.kmax
    assert kmax == 80
    m = {k: c[k] for k in gc.MAP_KEYS}
    for K1, K2 in ((K, 80), (80, K)):
        want = ref_case(ref, c, K1, K2, kcap=kmax)
        raw = Case(ext, c["kf1"], c["kf2"], m, c["T12"], c["seed12"], K1, K2).run(c["intr"])
        same(ext.decode_guided_out(raw, kmax, K1, K2), want, (K1, K2))
        unwritten(raw, kmax, K1, K2)
    if K == 80:
        print("K = kmax: reasons", np.bincount(want["reason1"], minlength=10)[1:], np.bincount(want["reason2"], minlength=10)[1:],
              "found / total / seed", want["n_found"], want["n_total"], want["n_seed"])
        assert want["n_found"] >= 5 and want["n_seed"] == 12


def window_of(c, d, i, r):
    """the window of keypoint i (direction d: 0 = keyframe 1's into keyframe 2) by a float64 projection -> (u, v, its cells
    (ix, iy) in the order of the walk: ix outer, iy inner)"""
    fx, fy, cx, cy = c["intr"]
    T = c["T12"].astype(np.float64)
    s, R, t = T[0], T[1:10].reshape(3, 3), T[10:]
    P = c["xyz"][(c["kf1"], c["kf2"])[d]["kf_mp"][i]].astype(np.float64)      # (identity poses: world = the keyframe's camera)
    Y = s * R @ P + t if d else (P - t) @ R / s
    u, v = fx * Y[0] / Y[2] + cx, fy * Y[1] / Y[2] + cy
    x0, x1 = max(int(np.floor((u - r) / 8)), 0), min(int(np.ceil((u + r) / 8)), c["W"] // 8 - 1)
    y0, y1 = max(int(np.floor((v - r) / 8)), 0), min(int(np.ceil((v + r) / 8)), c["H"] // 8 - 1)
    return u, v, [(ix, iy) for ix in range(x0, x1 + 1) for iy in range(y0, y1 + 1)]


def test_a_window_of_more_than_64_cells_is_walked_in_two_passes(exts, ref, frame80):
    """th = SPFE_PROJ_MAX_RADIUS: in the 8 x 12 cells of the frame a window holds up to 8 x 11 cells, more than the 64 lanes of
    one pass.  Every other point whose window has a keypoint in a cell of the second pass carries that keypoint's descriptor
    row, so that matches come out of the second pass; both directions against the host reference, bit for bit"""
    ext, r = exts["small"], float(X.PROJ_MAX_RADIUS)
    kmax = ext.layout.kmax
    c = dict(frame80, desc=frame80["desc"].copy())
    plain = ref_case(ref, frame80, kcap=kmax, th=r)
    late = ([], [])
    for d, (src, tgt) in enumerate(((c["kf1"], c["kf2"]), (c["kf2"], c["kf1"]))):
        for i in np.flatnonzero(plain["reason%d" % (d + 1)] >= guided_ref.NO_CANDIDATE):                   # it reaches its window
            u, v, cells = window_of(c, d, i, r)
            ks = [tgt["occ"][iy, ix] for ix, iy in cells[64:]]
            ks = [k for k in ks if k >= 0 and abs(tgt["kp_xy"][k, 0] - u) < r - 1 and abs(tgt["kp_xy"][k, 1] - v) < r - 1]   # well inside
            if ks:
                late[d].append((i, ks[0]))
        late[d][:] = late[d][::2]
        for i, k in late[d]:
            c["desc"][src["kf_mp"][i]] = tgt["kp_desc"][k]
    want = ref_case(ref, c, kcap=kmax, th=r)
    n_late = [sum(int(want[key][i] == k) for i, k in late[d]) for d, key in enumerate(("match1", "match2"))]
    print("th = 32: reasons", np.bincount(want["reason1"], minlength=10)[1:], np.bincount(want["reason2"], minlength=10)[1:],
          "matches out of the second pass", n_late, "found / total / seed", want["n_found"], want["n_total"], want["n_seed"])
    assert (want["match1"] >= 0).any() and (want["match2"] >= 0).any() and min(n_late) >= 1
    raw = Case(ext, c["kf1"], c["kf2"], {k: c[k] for k in gc.MAP_KEYS}, c["T12"], c["seed12"]).run(c["intr"], th=r)
    same(ext.decode_guided_out(raw, kmax, 80, 80), want, "th = 32")
    unwritten(raw, kmax, 80, 80)


def test_1300_keypoints_beyond_one_chunk_of_the_agree_kernel(ref):
    c = gc.large()
    ext = SPExtractor(1299, c["H"], c["W"], weights.synthetic(7, "trackable"), with_heat=False)
    try:
        kmax = ext.layout.kmax
        assert kmax == 1300 == len(c["kf1"]["kp_xy"])
        want = ref_case(ref, c)
        r1, r2 = np.bincount(want["reason1"], minlength=10)[1:], np.bincount(want["reason2"], minlength=10)[1:]
        print("1300: reasons", r1, r2, "found / total / seed", want["n_found"], want["n_total"], want["n_seed"])
        hit = np.flatnonzero((want["matches12"] >= 0) & (c["seed12"] < 0))
        assert (r1[[0, 1, 2, 5, 7, 8]] > 0).all() and (r2[[0, 1, 2, 5, 7, 8]] > 0).all() and want["n_found"] >= 100
        assert (hit < 1024).any() and (hit >= 1024).any() and ((c["seed12"] >= 0)[1024:]).any()      # both chunks carry counts
        m = {k: c[k] for k in gc.MAP_KEYS}
        raw = Case(ext, c["kf1"], c["kf2"], m, c["T12"], c["seed12"]).run(c["intr"])
        same(ext.decode_guided_out(raw, kmax, 1300, 1300), want, "1300")
        unwritten(raw, kmax, 1300, 1300)
    finally:
        ext.close()


# ---- the batched form behind the verify call ---------------------------------------------------------------------------------
def verified(ext, c, empty_first=False):
    """spfe_loop_verify_records_device on two candidates (the second keyframe twice; candidate 0 holds fewer points, or none)
    -> (the device arrays, the decoded verify blocks, match12 [2][kmax])"""
    import torch
    kmax, n_hyp = ext.layout.kmax, 8
    rng = np.random.default_rng(17)
    mp2 = np.stack([padded(ext, c["kf2"]["kf_mp"])] * 2)
    mp2[0, rng.random(kmax) < (1.0 if empty_first else 0.2)] = -1
    rnd = rng.integers(0, 1 << 32, (2, n_hyp, 3), dtype=np.uint64).astype(np.uint32)
    T = np.eye(4, dtype=np.float32).reshape(16)
    d = dict(rec1=record(ext, c["kf1"]), rec2=[record(ext, c["kf2"]), record(ext, c["kf2"])], mp1=dev(padded(ext, c["kf1"]["kf_mp"])),
             mp2=dev(mp2), T1=dev(T), T2=dev(np.stack([T, T])), rnd=dev(rnd), map=dev_map({k: c[k] for k in gc.MAP_KEYS}),
             match12=torch.zeros(2 * kmax, dtype=torch.int32, device="cuda"), nm=torch.zeros(2, dtype=torch.int32, device="cuda"),
             out=torch.full((2 * ext.sim3_out_bytes(n_hyp),), FILL, dtype=torch.uint8, device="cuda"), mp2_host=mp2)
    q = lambda t: t.data_ptr()   # noqa: E731
    ext.loop_verify_records_device(q(d["rec1"]), [q(r) for r in d["rec2"]], q(d["mp1"]), q(d["mp2"]), q(d["map"][0]), q(d["map"][1]),
                                   len(c["flags"]), q(d["T1"]), q(d["T2"]), q(d["rnd"]), n_hyp, q(d["match12"]), q(d["nm"]), q(d["out"]),
                                   c["intr"], min_inliers=12)
    torch.cuda.synchronize()
    ob = ext.sim3_out_bytes(n_hyp)
    raw = d["out"].cpu().numpy()
    return d, [ext.decode_sim3_out(raw[j * ob:(j + 1) * ob], kmax, n_hyp) for j in range(2)], d["match12"].cpu().numpy().reshape(2, kmax)


def batched(ext, c, d, jobs):
    import torch
    q = lambda t: t.data_ptr()   # noqa: E731
    gb = ext.guided_out_bytes()
    d_out = torch.full((len(jobs) * gb + 64,), FILL, dtype=torch.uint8, device="cuda")
    ext.loop_guided_match_records_device(q(d["rec1"]), [q(r) for r in d["rec2"]], jobs, q(d["mp1"]), q(d["mp2"]), *[q(t) for t in d["map"]],
                                         len(c["flags"]), q(d["T1"]), q(d["T2"]), q(d["match12"]), q(d["out"]), 8, q(d_out), c["intr"])
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    assert (raw[-64:] == FILL).all()
    return raw[:-64].reshape(len(jobs), gb)


@pytest.mark.parametrize("n_jobs", [1, 32])
def test_batched_form_reads_the_verify_blocks_and_equals_the_single_form_byte_for_byte(exts, ref, frame80, n_jobs):
    import torch
    ext, c = exts["small"], frame80
    kmax = ext.layout.kmax
    d, blocks, match12 = verified(ext, c)
    assert all(b["best_h"] >= 0 and b["N"] >= 12 for b in blocks), [(b["N"], b["best_h"]) for b in blocks]
    rets = [(j, int(h)) for j, b in enumerate(blocks) for h in b["return_idx"]]
    assert rets, "no hypothesis returns"
    jobs = ([(1, 0), (0, 7), (0, 0), (1, 7)] + rets + [(j, h) for h in range(8) for j in (1, 0)])[:n_jobs] if n_jobs > 1 else [rets[0]]
    jobs = (jobs * 32)[:n_jobs]
    got = batched(ext, c, d, jobs)
    verify_before = d["out"].cpu().numpy().copy()
    seen = {}
    best = 0
    for q_, (j, h) in enumerate(jobs):
        if (j, h) not in seen:                                            # the single form, fed from the decoded verify block
            seed = np.where(blocks[j]["vbInliers"][h], match12[j], -1).astype(np.int32)
            kf2 = dict(c["kf2"], kf_mp=d["mp2_host"][j][:len(c["kf2"]["kp_xy"])])
            case = Case(ext, c["kf1"], kf2, {k: c[k] for k in gc.MAP_KEYS}, blocks[j]["T12"][h], seed)
            case.d[5] = dev(seed)                                         # (all kmax entries, as the device builds them)
            case.host[5] = seed
            seen[(j, h)] = case.run(c["intr"])
            r = ext.decode_guided_out(seen[(j, h)], kmax, 80, 80)
            want = guided_ref.search(ref, c["kf1"], kf2, c["xyz"], c["flags"], c["dist_range"], c["desc"], np.eye(4), np.eye(4),
                                     blocks[j]["T12"][h], seed, c["intr"], W, H, kcap=kmax)
            same(r, want, (j, h))
            assert r["n_seed"] == blocks[j]["count"][h]
            if (j, h) in rets:                                            # a return has more than min_inliers = 12 inliers: all seeded
                assert r["n_total"] >= r["n_seed"] > 12
                best = max(best, r["n_found"])
        assert np.array_equal(got[q_], seen[(j, h)]), (q_, j, h)
    print("jobs", len(jobs), "distinct", len(seen), "most agreements behind a returning hypothesis", best)
    torch.cuda.synchronize()
    assert np.array_equal(d["out"].cpu().numpy(), verify_before) and np.array_equal(d["match12"].cpu().numpy().reshape(2, kmax), match12)


def test_a_verify_block_that_was_not_evaluated_gives_an_empty_job(exts, frame80):
    ext, c = exts["small"], frame80
    kmax = ext.layout.kmax
    d, blocks, _ = verified(ext, c, empty_first=True)
    assert blocks[0]["best_h"] == -1 and blocks[1]["best_h"] >= 0
    got = batched(ext, c, d, [(0, 3), (1, 3)])
    o = X.guided_offsets(kmax)
    assert got[0][:16].view(np.int32).tolist() == [0, 0, 0, X.GUIDED_STATUS_NOT_EVALUATED]
    assert (got[0][o["matches12"]:o["reason1"]].view(np.int32) == -1).all()
    assert (got[0][16:o["matches12"]] == FILL).all() and (got[0][o["reason1"]:] == FILL).all()
    assert got[1][:16].view(np.int32)[3] == 0


# ---- refusals and the overflow decision --------------------------------------------------------------------------------------
def test_overflowed_records_are_matched_and_their_status_passed_through(exts, ref):
    ext = exts[False]
    g = gc.load("one_way")
    kf1, kf2 = gc.keyframes(g)
    m = {k: g[k] for k in gc.MAP_KEYS}
    raws = [Case(ext, kf1, kf2, m, g["T12"], g["seed12"], status=st).run(g["intr1"]) for st in ((0, 0), (1, 0), (0, 1))]
    assert [int(r[12:16].view(np.int32)[0]) for r in raws] == [0, 1, 1]
    for r in raws[1:]:
        assert np.array_equal(r[:12], raws[0][:12]) and np.array_equal(r[16:], raws[0][16:])
    same(ext.decode_guided_out(raws[1], ext.layout.kmax, len(kf1["kp_xy"]), len(kf2["kp_xy"])), gc.run_ref(ref, g, kcap=ext.layout.kmax), "overflowed")


def test_invalid_arguments_return_before_any_launch(exts, frame80):
    import torch
    ext = exts[False]
    g = gc.load("one_way")
    kf1, kf2 = gc.keyframes(g)
    case = Case(ext, kf1, kf2, {k: g[k] for k in gc.MAP_KEYS}, g["T12"], g["seed12"])
    d_out = torch.full((2 * ext.guided_out_bytes(),), FILL, dtype=torch.uint8, device="cuda")
    good = case.args(d_out)
    bad = []
    for i in list(range(8)) + [9, 10, 11, 12, 13]:                         # every pointer
        a = list(good)
        a[i] = 0
        bad.append((a, {}))
    for v in (-1, X.PROJ_MAX_POINTS + 1):
        a = list(good)
        a[8] = v
        bad.append((a, {}))
    bad += [(good, dict(th=0.0)), (good, dict(th=float(X.PROJ_MAX_RADIUS) + 0.01)), (good, dict(th=float("nan")))]
    for a, kw in bad:
        with pytest.raises(X.SpfeError, match="SPFE_EINVAL"):
            ext.search_by_sim3_record_device(*a, g["intr1"], **kw)
    q = lambda t: t.data_ptr()   # noqa: E731
    ver = torch.full((2 * ext.sim3_out_bytes(8),), FILL, dtype=torch.uint8, device="cuda")
    m12 = torch.zeros(2 * ext.layout.kmax, dtype=torch.int32, device="cuda")
    mp2 = dev(np.full((2, ext.layout.kmax), -1, np.int32))

    def many(recs, jobs, n_hyp=8, **kw):
        ext.loop_guided_match_records_device(good[0], recs, jobs, good[2], q(mp2), *good[4:8], good[8], good[9], good[10], q(m12), q(ver),
                                             n_hyp, q(d_out), g["intr1"], **kw)
    two = [good[1], good[1]]
    for recs, jobs, kw in (([], [(0, 0)], {}), (two, [], {}), (two, [(0, 0)] * (X.GUIDED_MAX_JOBS + 1), {}), (two, [(2, 0)], {}),
                           (two, [(0, 8)], {}), (two, [(-1, 0)], {}), (two, [(0, -1)], {}), ([good[1], 0], [(0, 0)], {}),
                           (two, [(0, 0)], dict(n_hyp=0)), (two, [(0, 0)], dict(n_hyp=X.SIM3_MAX_HYPOTHESES + 1)),
                           (two, [(0, 0)], dict(th=33.0)), ([good[1]] * (X.SIM3_MAX_CANDIDATES + 1), [(0, 0)], {})):
        with pytest.raises(X.SpfeError, match="SPFE_EINVAL"):
            many(recs, jobs, **kw)
    with pytest.raises(X.SpfeError, match="SPFE_EINVAL"):                   # the host form
        ext.search_by_sim3(kf1, kf2, *[g[k] for k in gc.MAP_KEYS], kf1["Tcw"], kf2["Tcw"], g["T12"], g["seed12"], g["intr1"], th=40.0)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == FILL).all()
    case.unchanged()
    ext.search_by_sim3_record_device(*good, g["intr1"], th=float(X.PROJ_MAX_RADIUS))      # the radius at the cap is served
    torch.cuda.synchronize()
    assert d_out.cpu().numpy()[:4].view(np.int32)[0] >= 0 and (d_out.cpu().numpy()[ext.guided_out_bytes():] == FILL).all()
