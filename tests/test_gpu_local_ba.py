"""GPU: bundle adjustment (spfe_bundle_adjust, spfe_local_ba_records_device; sp_orb_slam_amd/csrc/ba.hip) against its host
statement tests/ba_ref/ba_ref.c, both built on include/spfe_ba_math.h.

Host form, on every fixture tests/golden/ba_*.npz and on the generated cases large (20 + 12 keyframes, 1300 points, ~8000
edges), capacity (64 + 64 keyframes, the 384 x 384 system) and lds_edge (the two numbers of free keyframes either side of
spfe_ba_lds_free_capacity): every integer, verdict, erase_idx, iteration and trial count equal; Tcw_out and xyz_out within 4
times the deviation measured on an MI355X.
Measured on an MI355X (ROCm 7, gfx950): MEASURED_TCW = MEASURED_XYZ = 0.0 on every case: the blocks are equal byte for byte,
chi2 and lambda included (the device's sqrt, sin and cos give the host's bits on every argument the schedule meets).  A ROCm
whose libm differs in a last bit fails here first; the bound is then measured again, not guessed.

Record form: six frames of tools/track_scene.py extracted into records, keypoints associated by world position (the scene pans
by whole cells), poses and points perturbed; the block is byte for byte the host form's on the arrays read back from those
records, and records and inputs are unchanged afterwards.

The stop flag on the device is tested as set on entry and as present but 0.  A flag that turns 1 while the kernel runs
(SPFE_BA_STATUS_STOPPED: the break inside a round, the read between the rounds) cannot be made deterministic from the host and is
NOT exercised on the GPU: that path is held to the independent statement by ba_ref.c alone (tests/test_ba_reference.py).

The solve's scratch and the host form's staging are the handle's: a handle created after another was destroyed, and two live
handles solving in turn, give the reference's blocks.

More than SPFE_BA_MAX_FREE free keyframes: the host form refuses the call, the record form (d_fixed is device memory) answers
with SPFE_BA_STATUS_TOO_MANY_FREE before it touches anything sized by that limit; both are tested, the second against ba_ref.c."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "ba_ref", "golden"):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
import ba_cases  # noqa: E402
import ba_ref  # noqa: E402
import extent_cases as ec  # noqa: E402
from make_golden_ba import NAMES  # noqa: E402

from sp_orb_slam_amd import extractor as X  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import SPExtractor, SpfeError  # noqa: E402
from tools import track_scene as ts  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden")
H, W, NF = 240, 320, 400
FRAMES = (1, 2, 3, 4, 5, 6)
INTR = (ts.FX, ts.FY, ts.CX, ts.CY)
MEASURED_TCW = 0.0
MEASURED_XYZ = 0.0


class Scene:
    pass


def build_scene(mktemp):
    """the handle, the host reference, six records of the panning scene and a bundle-adjustment problem on them; mktemp(name) ->
    a directory for the host reference.  The caller closes s.ext.  (Also the scene of tests/graph_forms.py.)"""
    import torch
    s = Scene()
    s.ext = ext = SPExtractor(NF, H, W, weights.synthetic(7, "trackable"), max_batch=len(FRAMES), with_heat=False)
    s.ref = ba_ref.build(mktemp("ba_ref"))
    world = ts.texture(21, *ts.world_size(H, W))
    d_img = torch.from_numpy(np.stack([ts.frame(world, k, H, W) for k in FRAMES])).cuda()
    s.rb = ext.record_bytes()
    s.d_recs = torch.zeros(len(FRAMES) * s.rb, dtype=torch.uint8, device="cuda")
    ext.wait_records(ext.extract_batch_device(d_img.data_ptr(), len(FRAMES), s.d_recs.data_ptr()))
    torch.cuda.synchronize()
    s.raw = s.d_recs.cpu().numpy().reshape(len(FRAMES), s.rb).copy()
    s.recs = [ext.view_record(r) for r in s.raw]
    assert all(r.status == 0 and r.K >= 100 for r in s.recs), [r.K for r in s.recs]
    # points: keypoints of the first frame on the plane; their keypoints in the other frames by the pan
    pts, _, sel = ts.map_points(s.recs[0].kp_xy, s.recs[0].descriptors, FRAMES[0], max_points=160)
    edges = []
    kp_of = [ec.exact_associations(s.recs[0].kp_xy[sel], np.subtract(ts.offsets(k), ts.offsets(FRAMES[0])), s.recs[f].kp_xy)
             for f, k in enumerate(FRAMES)]
    for p in range(len(pts)):
        for f in range(len(FRAMES)):
            if kp_of[f][p] >= 0:
                edges.append((p, f, int(kp_of[f][p])))
    s.edges = np.array(edges, np.int32)
    assert len(s.edges) > 2 * len(pts) and (np.bincount(s.edges[:, 1], minlength=6) > 20).all()
    rng = np.random.default_rng(5)
    s.fixed = np.array([0, 0, 0, 0, 1, 1], np.uint8)
    Tcw = []
    for f, k in enumerate(FRAMES):
        T = ts.pose(*ts.offsets(k)).astype(np.float64)
        if not s.fixed[f]:
            T = ba_cases.pose(rng.normal(0, 0.002, 3), rng.normal(0, 0.01, 3)) @ T
        Tcw.append(T.astype(np.float32).reshape(16))
    s.Tcw = np.stack(Tcw)
    s.xyz = (np.asarray(pts, np.float64) + rng.normal(0, 0.02, (len(pts), 3))).astype(np.float32)
    s.obs = np.stack([s.recs[f].kp_xy[kp] for _, f, kp in s.edges]).astype(np.float32)
    s.w = np.stack([s.recs[f].cov2_inv[kp] for _, f, kp in s.edges]).astype(np.float32)
    return s


@pytest.fixture(scope="module")
def S(tmp_path_factory):
    s = build_scene(tmp_path_factory.mktemp)
    yield s
    s.ext.close()


def load(name):
    if name in NAMES:
        return dict(np.load(os.path.join(GOLDEN, "ba_%s.npz" % name)))
    return {"large": ba_cases.large, "capacity": ba_cases.capacity}[name]()


def run_host(ext, c, fill=0, **kw):
    a = ba_ref.arrays(c)
    stop = 1 if int(c["stop_reads"]) == 0 else None
    return ext.bundle_adjust(a["edges"], a["obs_xy"], a["inv_sigma2"], a["Tcw"], a["fixed"], a["xyz"], [float(v) for v in c["intr"]],
                             schedule=int(c["schedule"]), iterations=[int(v) for v in c["iterations"]], robust=int(c["robust"]),
                             inv_sigma2_full=float(c["inv_sigma2_full"]), stop=stop, fill=fill, **kw)


def same_as_reference(s, c, what):
    a = ba_ref.arrays(c)
    n_kf, n, E = len(a["Tcw"]), len(a["xyz"]), len(a["edges"])
    blk = run_host(s.ext, c, fill=0x5A)
    r = ba_ref.solve(s.ref, c, fill=0x5A)
    g = X.SPExtractor.decode_ba_out(blk, n_kf, n, E)
    for k in ("n_kf", "n_free", "n_points", "n_edges", "n_served", "n_level1", "n_erase", "status"):
        assert g[k] == r[k], (what, k, g[k], r[k])
    assert np.array_equal(g["iterations"], r["iterations"]) and np.array_equal(g["trials"], r["trials"]), \
        (what, g["iterations"], r["iterations"], g["trials"], r["trials"])
    assert np.array_equal(g["verdict"], r["verdict"]) and np.array_equal(g["erase_idx"], r["erase_idx"]), what
    dT = float(np.abs(g["Tcw_out"].astype(np.float64) - r["Tcw_out"]).max())
    dX = float(np.abs(g["xyz_out"].astype(np.float64) - r["xyz_out"]).max()) if n else 0.0
    print("%s: |Tcw_out - ref| %.3e, |xyz_out - ref| %.3e, chi2 exit %.17g / %.17g, lambda %.17g / %.17g, blocks equal %s" % (
        what, dT, dX, g["chi2_exit"], r["chi2_exit"], g["lambda_"], r["lambda_"], blk.tobytes() == r["block"].tobytes()))
    assert dT <= 4 * MEASURED_TCW and dX <= 4 * MEASURED_XYZ, (what, dT, dX)
    if MEASURED_TCW == 0.0 and MEASURED_XYZ == 0.0:   # nothing deviates: then the whole block, chi2 and lambda included, is equal
        assert blk.tobytes() == r["block"].tobytes(), what
    return g, r, blk


@pytest.mark.parametrize("name", NAMES + ("large", "capacity"))
def test_host_form_equals_the_reference(S, name):
    c = load(name)
    g, r, blk = same_as_reference(S, c, name)
    # what the block does not name keeps the caller's bytes
    o = X.ba_offsets(g["n_kf"], g["n_points"], g["n_edges"])
    assert (blk[48:64] == 0x5A).all() and (blk[88:128] == 0x5A).all()
    assert (blk[o["erase"] + 4 * g["n_erase"]:] == 0x5A).all() and (blk[o["verdict"] + g["n_edges"]:o["erase"]] == 0x5A).all()
    if name == "stop_on_entry":
        assert g["status"] == X.BA_STATUS_STOPPED_EARLY and g["Tcw_out"].tobytes() == c["Tcw"].tobytes()
        assert g["xyz_out"].tobytes() == c["xyz"].tobytes() and (g["verdict"] == X.BA_SKIPPED).all()
    if name == "capacity":
        assert g["n_free"] == X.BA_MAX_FREE and g["n_kf"] == X.BA_MAX_KEYFRAMES


def test_either_side_of_the_lds_capacity(S):
    cap = S.ext.ba_lds_free_capacity()
    assert 1 <= cap < X.BA_MAX_FREE
    for n_free in (cap, cap + 1):
        g, r, _ = same_as_reference(S, ba_cases.lds_edge(n_free), "lds_edge %d" % n_free)
        assert g["n_free"] == n_free and g["iterations"].sum() > 2
    # the same problem with its system in LDS and in scratch: free keyframes without an edge change nothing but n_free
    c = ba_cases.lds_edge(cap)
    pad = cap + 1 - int((c["fixed"] == 0).sum())
    d = dict(c, Tcw=np.concatenate([c["Tcw"], np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (pad, 1))]),
             fixed=np.concatenate([c["fixed"], np.zeros(pad, np.uint8)]))
    a = X.SPExtractor.decode_ba_out(run_host(S.ext, c), len(c["Tcw"]), len(c["xyz"]), len(c["edges"]))
    b = X.SPExtractor.decode_ba_out(run_host(S.ext, d), len(d["Tcw"]), len(d["xyz"]), len(d["edges"]))
    assert b["n_free"] == cap + 1 and a["n_free"] == cap
    assert a["xyz_out"].tobytes() == b["xyz_out"].tobytes() and a["Tcw_out"].tobytes() == b["Tcw_out"][:len(c["Tcw"])].tobytes()
    assert np.array_equal(a["verdict"], b["verdict"]) and np.array_equal(a["trials"], b["trials"]) and a["lambda_"] == b["lambda_"]


def test_two_calls_give_the_same_bytes(S):
    c = load("outliers")
    assert run_host(S.ext, c).tobytes() == run_host(S.ext, c).tobytes()


def test_the_buffers_live_and_die_with_their_handle(S):
    """The solve's scratch and the staging belong to the handle: a handle that is created where a destroyed one was starts
    with none, and two live handles keep theirs apart.  On the 64 x 96 frame of the loop fixtures (NF = 100)."""
    blob = weights.synthetic(7, "trackable")
    small, two_kf = load("small"), load("two_kf")

    def handle():
        s = Scene()
        s.ref, s.ext = S.ref, SPExtractor(100, 64, 96, blob, with_heat=False)
        return s

    a = handle()
    same_as_reference(a, small, "first handle: small")
    a.ext.close()
    b = handle()
    same_as_reference(b, two_kf, "second handle: two_kf")
    same_as_reference(b, small, "second handle: small")
    b.ext.close()
    c, d = handle(), handle()
    try:
        for rnd in range(2):
            same_as_reference(c, small, "two handles, round %d: c small" % rnd)
            same_as_reference(d, two_kf, "two handles, round %d: d two_kf" % rnd)
            same_as_reference(c, two_kf, "two handles, round %d: c two_kf" % rnd)
            same_as_reference(d, small, "two handles, round %d: d small" % rnd)
    finally:
        c.ext.close()
        d.ext.close()


def record_call(s, d_recs, edges, Tcw, fixed, xyz, schedule=X.BA_LOCAL, iterations=(5, 10), stop=None, fill=0x5A):
    import torch
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v).reshape(-1).view(np.uint8).copy()).cuda()   # noqa: E731
    n_kf, n, E = len(Tcw), len(xyz), len(edges)
    ins = dict(edges=t(edges), Tcw=t(Tcw), fixed=t(fixed), xyz=t(xyz))
    d_stop = None if stop is None else torch.tensor([stop], dtype=torch.int32, device="cuda")
    d_out = torch.full((X.ba_offsets(n_kf, n, E)["bytes"],), fill, dtype=torch.uint8, device="cuda")
    before = {k: v.clone() for k, v in ins.items()}
    recs_before = d_recs.clone()
    # (more keyframes than records: the slots share the six records)
    s.ext.local_ba_records_device([d_recs.data_ptr() + (f % len(FRAMES)) * s.rb for f in range(n_kf)], ins["edges"].data_ptr(), E,
                                  ins["Tcw"].data_ptr(), ins["fixed"].data_ptr(), ins["xyz"].data_ptr(), n, d_out.data_ptr(), INTR,
                                  schedule=schedule, iterations=iterations, d_stop=None if d_stop is None else d_stop.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(d_recs, recs_before) and all(torch.equal(ins[k], before[k]) for k in ins)
    return d_out.cpu().numpy()


def test_record_form_equals_the_host_form_on_real_records(S):
    n_kf, n, E = len(S.Tcw), len(S.xyz), len(S.edges)
    blk = record_call(S, S.d_recs, S.edges, S.Tcw, S.fixed, S.xyz)
    host = S.ext.bundle_adjust(S.edges, S.obs, S.w, S.Tcw, S.fixed, S.xyz, INTR, fill=0x5A)
    g = X.SPExtractor.decode_ba_out(blk, n_kf, n, E)
    print("records: E %d, n %d, iterations %s, trials %s, level1 %d, erase %d, chi2 %.6g -> %.6g" % (
        E, n, g["iterations"], g["trials"], g["n_level1"], g["n_erase"], g["chi2_entry"], g["chi2_exit"]))
    assert blk.tobytes() == host.tobytes()
    assert g["status"] == 0 and g["n_served"] == E and g["iterations"][0] > 0 and g["chi2_exit"] < g["chi2_entry"]
    c = dict(edges=S.edges, obs_xy=S.obs, inv_sigma2=S.w, Tcw=S.Tcw, fixed=S.fixed, xyz=S.xyz, intr=np.array(INTR, np.float32),
             schedule=np.int32(0), iterations=np.array([5, 10], np.int32), robust=np.int32(1), inv_sigma2_full=np.float32(1),
             stop_reads=np.int32(-1))
    r = ba_ref.solve(S.ref, c, fill=0x5A)
    assert np.array_equal(g["verdict"], r["verdict"]) and np.array_equal(g["trials"], r["trials"])
    # an edge whose keypoint is the record's K is skipped (the host form knows no K and would serve it)
    e2 = S.edges.copy()
    e2[7, 2] = S.recs[e2[7, 1]].K
    g2 = X.SPExtractor.decode_ba_out(record_call(S, S.d_recs, e2, S.Tcw, S.fixed, S.xyz), n_kf, n, E)
    assert g2["verdict"][7] == X.BA_SKIPPED and g2["n_served"] == E - 1


def test_cov_overflow_is_refused_in_local_and_served_in_full(S):
    import torch
    n_kf, n, E = len(S.Tcw), len(S.xyz), len(S.edges)
    raw = S.raw.copy()
    raw[2, S.ext.layout.off_hdr:S.ext.layout.off_hdr + 12].view(np.int32)[2] |= 1   # SPFE_STATUS_COV_OVERFLOW
    d = torch.from_numpy(raw.reshape(-1)).cuda()
    g = X.SPExtractor.decode_ba_out(record_call(S, d, S.edges, S.Tcw, S.fixed, S.xyz), n_kf, n, E)
    assert g["status"] == (1 | X.BA_STATUS_COV_OVERFLOW) and g["n_served"] == 0 and g["iterations"].sum() == 0
    assert g["Tcw_out"].tobytes() == S.Tcw.tobytes() and g["xyz_out"].tobytes() == S.xyz.tobytes() and (g["verdict"] == 0).all()
    f = X.SPExtractor.decode_ba_out(record_call(S, d, S.edges, S.Tcw, S.fixed, S.xyz, schedule=X.BA_FULL, iterations=(5, 0)), n_kf, n, E)
    assert f["status"] == 1 and f["n_served"] == E and f["iterations"][0] > 0 and (f["verdict"] == X.BA_INLIER).all()
    clean = X.SPExtractor.decode_ba_out(record_call(S, S.d_recs, S.edges, S.Tcw, S.fixed, S.xyz, schedule=X.BA_FULL, iterations=(5, 0)),
                                        n_kf, n, E)
    assert f["Tcw_out"].tobytes() == clean["Tcw_out"].tobytes() and f["xyz_out"].tobytes() == clean["xyz_out"].tobytes()


def test_stop_on_entry_echoes_the_inputs(S):
    n_kf, n, E = len(S.Tcw), len(S.xyz), len(S.edges)
    g = X.SPExtractor.decode_ba_out(record_call(S, S.d_recs, S.edges, S.Tcw, S.fixed, S.xyz, stop=1), n_kf, n, E)
    assert g["status"] == X.BA_STATUS_STOPPED_EARLY and g["Tcw_out"].tobytes() == S.Tcw.tobytes()
    assert g["xyz_out"].tobytes() == S.xyz.tobytes() and (g["verdict"] == X.BA_SKIPPED).all() and g["n_erase"] == 0
    g0 = X.SPExtractor.decode_ba_out(record_call(S, S.d_recs, S.edges, S.Tcw, S.fixed, S.xyz, stop=0), n_kf, n, E)
    g1 = X.SPExtractor.decode_ba_out(record_call(S, S.d_recs, S.edges, S.Tcw, S.fixed, S.xyz), n_kf, n, E)
    assert g0["status"] == 0 and g0["xyz_out"].tobytes() == g1["xyz_out"].tobytes() and np.array_equal(g0["trials"], g1["trials"])


def test_more_free_keyframes_than_the_limit_in_the_record_form(S):
    """65 of 70 flags are 0: SPFE_BA_STATUS_TOO_MANY_FREE, nothing optimised, the inputs echoed, the padding kept — ba_ref.c's
    block byte for byte; with 64 the same call is served"""
    n, E, n_kf = len(S.xyz), len(S.edges), 70
    Tcw = np.tile(S.Tcw, (12, 1))[:n_kf].copy()
    fixed64 = np.r_[S.fixed, np.zeros(60, np.uint8), np.ones(4, np.uint8)]   # the scene's two fixed keyframes stay fixed
    fixed = fixed64.copy()
    fixed[66] = 0
    assert int((fixed64 == 0).sum()) == X.BA_MAX_FREE and int((fixed == 0).sum()) == X.BA_MAX_FREE + 1
    blk = record_call(S, S.d_recs, S.edges, Tcw, fixed, S.xyz)
    g = X.SPExtractor.decode_ba_out(blk, n_kf, n, E)
    assert g["status"] == X.BA_STATUS_TOO_MANY_FREE and g["n_kf"] == n_kf and g["n_free"] == 65 and g["n_points"] == n and g["n_edges"] == E
    assert g["n_served"] == 0 and g["iterations"].sum() == 0 and g["trials"].sum() == 0 and g["n_level1"] == 0 and g["n_erase"] == 0
    assert g["Tcw_out"].tobytes() == Tcw.tobytes() and g["xyz_out"].tobytes() == S.xyz.tobytes() and (g["verdict"] == X.BA_SKIPPED).all()
    assert g["chi2_entry"] == 0.0 and g["chi2_exit"] == 0.0 and g["lambda_"] == 0.0
    o = X.ba_offsets(n_kf, n, E)
    assert (blk[48:64] == 0x5A).all() and (blk[88:128] == 0x5A).all() and (blk[o["verdict"] + E:] == 0x5A).all()
    c = dict(edges=S.edges, obs_xy=S.obs, inv_sigma2=S.w, Tcw=Tcw, fixed=fixed, xyz=S.xyz, intr=np.array(INTR, np.float32),
             schedule=np.int32(0), iterations=np.array([5, 10], np.int32), robust=np.int32(1), inv_sigma2_full=np.float32(1),
             stop_reads=np.int32(-1))
    K = np.array([S.recs[f % len(FRAMES)].K for f in range(n_kf)], np.int32)
    assert blk.tobytes() == ba_ref.solve(S.ref, c, K=K, rec_status=np.zeros(n_kf, np.int32), fill=0x5A)["block"].tobytes()
    # the records' status words are ORed in beside the bit
    raw = S.raw.copy()
    raw[1, S.ext.layout.off_hdr:S.ext.layout.off_hdr + 12].view(np.int32)[2] |= 1
    import torch
    g1 = X.SPExtractor.decode_ba_out(record_call(S, torch.from_numpy(raw.reshape(-1)).cuda(), S.edges, Tcw, fixed, S.xyz), n_kf, n, E)
    assert g1["status"] == (1 | X.BA_STATUS_COV_OVERFLOW | X.BA_STATUS_TOO_MANY_FREE) and g1["Tcw_out"].tobytes() == Tcw.tobytes()
    # 64 free keyframes are the limit, not beyond it: the same call is served and equals the reference
    b64 = record_call(S, S.d_recs, S.edges, Tcw, fixed64, S.xyz)
    g64 = X.SPExtractor.decode_ba_out(b64, n_kf, n, E)
    assert g64["status"] == 0 and g64["n_free"] == 64 and g64["n_served"] == E and g64["iterations"][0] > 0
    assert b64.tobytes() == ba_ref.solve(S.ref, dict(c, fixed=fixed64), K=K, fill=0x5A)["block"].tobytes()


def test_refusals_leave_the_output_untouched(S):
    import torch
    e = S.ext
    c = load("small")
    a = ba_ref.arrays(c)
    intr = [float(v) for v in c["intr"]]
    big = X.ba_offsets(129, 16385, 8)["bytes"]

    def refused(call):
        out = np.full(big, 0xC3, np.uint8)
        with pytest.raises(SpfeError):
            call(out)
        assert (out == 0xC3).all()

    T129 = np.tile(a["Tcw"][:1], (129, 1))
    refused(lambda o: e.bundle_adjust(a["edges"], a["obs_xy"], a["inv_sigma2"], T129, np.ones(129, np.uint8), a["xyz"], intr, out=o))
    T128 = np.tile(a["Tcw"][:1], (128, 1))
    f65 = np.r_[np.zeros(65, np.uint8), np.ones(63, np.uint8)]
    refused(lambda o: e.bundle_adjust(a["edges"], a["obs_xy"], a["inv_sigma2"], T128, f65, a["xyz"], intr, out=o))
    refused(lambda o: e.bundle_adjust(a["edges"], a["obs_xy"], a["inv_sigma2"], a["Tcw"], a["fixed"], np.zeros((16385, 3), np.float32),
                                      intr, out=o))
    E1 = X.BA_MAX_EDGES + 1
    out = np.full(X.ba_offsets(5, 40, E1)["bytes"], 0xC3, np.uint8)
    with pytest.raises(SpfeError):
        e.bundle_adjust(np.zeros((E1, 3), np.int32), np.zeros((E1, 2), np.float32), np.zeros((E1, 2), np.float32), a["Tcw"], a["fixed"],
                        a["xyz"], intr, out=out)
    assert (out == 0xC3).all()
    refused(lambda o: e.bundle_adjust(a["edges"], a["obs_xy"], a["inv_sigma2"], a["Tcw"], a["fixed"], a["xyz"], intr, schedule=2, out=o))
    refused(lambda o: e.bundle_adjust(a["edges"], a["obs_xy"], a["inv_sigma2"], a["Tcw"], a["fixed"], a["xyz"], intr,
                                      iterations=(5, 1001), out=o))
    refused(lambda o: e.bundle_adjust(a["edges"], a["obs_xy"], None, a["Tcw"], a["fixed"], a["xyz"], intr, out=o))   # LOCAL reads it
    # null arguments, straight at the C ABI
    prm = e._ba_params(intr, 0, (5, 10), 1, 1.0)
    out = np.full(big, 0xC3, np.uint8)
    p = lambda v: v.ctypes.data   # noqa: E731
    L, h = e._lib, e._h
    full = [h, p(a["edges"]), p(a["obs_xy"]), p(a["inv_sigma2"]), len(a["edges"]), p(a["Tcw"]), p(a["fixed"]), 5, p(a["xyz"]), 40,
            C.byref(prm), None, p(out)]
    for i in (0, 1, 2, 5, 6, 8, 10, 12):
        args = list(full)
        args[i] = None
        assert L.spfe_bundle_adjust(*args) != 0, i
    assert (out == 0xC3).all()
    # the record form: limits + 1, null arguments, a bad schedule; d_out keeps its bytes
    d_out = torch.full((big,), 0xC3, dtype=torch.uint8, device="cuda")
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v).reshape(-1).view(np.uint8).copy()).cuda()   # noqa: E731
    d = dict(edges=t(S.edges), Tcw=t(S.Tcw), fixed=t(S.fixed), xyz=t(S.xyz))
    recs = [S.d_recs.data_ptr() + f * S.rb for f in range(6)]
    ok = dict(d_records=recs, d_edges=d["edges"].data_ptr(), E=len(S.edges), d_Tcw=d["Tcw"].data_ptr(), d_fixed=d["fixed"].data_ptr(),
              d_xyz=d["xyz"].data_ptr(), n=len(S.xyz), d_out=d_out.data_ptr(), intr=INTR)
    for bad in (dict(d_records=recs * 22), dict(n=X.BA_MAX_POINTS + 1), dict(E=X.BA_MAX_EDGES + 1), dict(schedule=7), dict(d_Tcw=0),
                dict(d_fixed=0), dict(d_edges=0), dict(d_xyz=0), dict(d_out=0), dict(d_records=recs[:5] + [0]), dict(iterations=(-1, 10))):
        with pytest.raises(SpfeError):
            e.local_ba_records_device(**dict(ok, **bad))
    torch.cuda.synchronize()
    assert bool((d_out == 0xC3).all())
