"""Every *_device form of include/spfe.h held to its stream contract — "N launches on `stream`, no host synchronisation, no host
decision; scratch is allocated before the first launch" — by capturing one call into a hipGraph and replaying it on other inputs.

FORMS has one entry per device form (spfe_extract_batch_device has its own test, tools/graph_capture_check.py).  An entry builds
a handle and two input sets A and B with the SAME host-side arguments (n, caps, params, job lists, host pointer arrays) that
differ in everything the form reads from device memory: other records (another K in the header), other points, poses, holder
arrays, counts and — for the chained loop forms — other verify / guided blocks.  main(name), run in a fresh process per form:
  1. the fixed device buffers of the call are allocated once; A and B are copied INTO them, so no pointer ever changes; outputs
     are prefilled with 0xA5 and in/out arrays restored to their starting bytes before every call and every replay;
  2. a direct call on A (checked as the existing tests check the form: against its host form / host reference where that is
     a line, else the scene's own expectations), a direct call on B; every output of B must differ from A's, and at least one
     device-side count must differ where the form has one;
  3. A is put back and ONE call is captured on a torch.cuda.Stream in global mode (tests/hip_graph.py);
  4. the graph's shape: only kernel and memset nodes, one root, edges == nodes - 1 (one chain: no parallel branch is ever
     replayed), and as many kernel nodes as include/spfe.h states for the form (FORMS quotes the sentence; where the header says
     only "launches" the number is the measured one);
  5. replays on A, on B and on A again: every output buffer, compared whole, equals the direct call's bytes for that input.
A launch on another stream is missing from the graph and leaves 0xA5 behind; a synchronising or allocating call invalidates the
capture (its status is reported); a count read on the host at enqueue time is frozen into the graph and the replay on B differs.

SAFETY RULE, kept by construction: kernel arguments baked into a graph include the handle's scratch pointers, and the handle
frees a scratch block when a later call grows it.  So each process makes its largest call first (A and B have the same sizes, and
the set-up calls of a chain come before everything else), makes NO library call between the capture and the last replay, and
every buffer the graph names — and the handle — stays alive until the graph is destroyed.

The process prints one line, "graph-form <name>: PASS kernel=<k> memset=<m>" or "... FAIL: <reasons>", and exits 0 / 1.
usage: python -m tests.graph_forms <name>"""
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _d in ("", "proj_ref", "pose_ref", "track_ref", "guided_ref", "sim3_ref", "sim3opt_ref", "fuse_ref", "loopfuse_ref", "eg_ref",
           "loopdet_ref", "ba_ref", "golden"):
    _p = os.path.join(ROOT, "tests", _d)
    if _p not in sys.path:
        sys.path.insert(0, _p)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FILL = 0xA5


class Form:
    """kernels: the kernel nodes of one captured call; sentence: the words of include/spfe.h that state that number, or (stated
    False) the words that promise launches without a number — then `kernels` is the measured count; memsets: memset nodes"""

    def __init__(self, build, kernels, sentence, stated=True, memsets=0):
        self.build, self.kernels, self.sentence, self.stated, self.memsets = build, kernels, sentence, stated, memsets


class Case:
    """A, B: name -> ndarray (an input, or the starting bytes of an in/out array) or int (an output of that many bytes); call(P,
    stream) enqueues the form on the addresses P[name]; outputs: the names compared; check(got): the direct call on A against its
    reference; counts(spec, got): the device-side counts of a call (A's and B's must differ); pointers: name -> the buffers whose
    addresses that DEVICE array holds"""

    def __init__(self, ext, A, B, call, outputs, check=None, counts=None, pointers=None, keep=()):
        self.ext, self.A, self.B, self.call, self.outputs = ext, A, B, call, tuple(outputs)
        self.check, self.counts, self.pointers, self.keep = check, counts, pointers or {}, keep


def mktemp(name):
    return tempfile.mkdtemp(prefix="graph_forms_%s_" % name)


def raw_bytes(v):
    return np.ascontiguousarray(v).reshape(-1).view(np.uint8)


def is_out(v):
    return isinstance(v, (int, np.integer))


def direct(spec, call, outputs):
    """a set-up call of a chain on tensors of its own -> dict name -> uint8 array of `outputs`"""
    import torch
    tens = {k: (torch.full((max(int(v), 16),), FILL, dtype=torch.uint8, device="cuda") if is_out(v) else
                torch.from_numpy(np.concatenate([raw_bytes(v), np.zeros(16, np.uint8)])).cuda()) for k, v in spec.items()}
    torch.cuda.synchronize()
    call({k: t.data_ptr() for k, t in tens.items()}, None)
    torch.cuda.synchronize()
    return {k: tens[k].cpu().numpy()[:int(spec[k])].copy() for k in outputs}


class Buffers:
    """The fixed device buffers of one Case: allocated once (16 bytes of slack each), A and B are copied INTO them, so no
    address ever changes.  P: name -> address; the DEVICE pointer tables of case.pointers are filled with those addresses (in
    case.A and case.B) before the images are taken.  load(key) puts the inputs and the starting bytes of the in/out arrays of
    "A" / "B" back and prefills every output with FILL; read(names) brings buffers back whole (default: case.outputs).
    stream None (run() below): the copies go to the current stream and both wait for the whole device.  With a
    torch.cuda.Stream (tests/test_gpu_threads.py, one per host thread) the copies and fills are enqueued on that stream and
    both wait for that stream alone, so threads with a stream each never wait for one another."""

    def __init__(self, case, stream=None, device="cuda"):
        import torch
        self.torch, self.case, self.stream = torch, case, stream
        self.names = names = list(case.A)
        assert names == list(case.B), "A and B name the same buffers"
        self.size = size = {}
        for k in names:
            a, b = case.A[k], case.B[k]
            assert is_out(a) == is_out(b), k
            size[k] = int(a) if is_out(a) else len(raw_bytes(a))
            assert size[k] == (int(b) if is_out(b) else len(raw_bytes(b))), ("A and B differ in the size of", k)
        self.bufs = {k: torch.full((size[k] + 16,), FILL, dtype=torch.uint8, device=device) for k in names}
        self.P = {k: t.data_ptr() for k, t in self.bufs.items()}
        for k, members in case.pointers.items():
            for spec in (case.A, case.B):
                spec[k] = np.array([self.P[r] for r in members], np.int64)
        self.spec_of = {"A": case.A, "B": case.B}
        self.img = {key: {k: torch.from_numpy(raw_bytes(spec[k]).copy()) for k in names if not is_out(spec[k]) and size[k]}
                    for key, spec in self.spec_of.items()}
        torch.cuda.synchronize()     # the prefill above ran on the current stream: it is done before `stream` is first used

    def wait(self):
        if self.stream is None:
            self.torch.cuda.synchronize()
        else:
            self.stream.synchronize()

    def _on_stream(self):
        import contextlib
        return contextlib.nullcontext() if self.stream is None else self.torch.cuda.stream(self.stream)

    def load(self, key):
        with self._on_stream():
            for k in self.names:
                if is_out(self.spec_of[key][k]):
                    self.bufs[k].fill_(FILL)
                elif self.size[k]:
                    self.bufs[k][:self.size[k]].copy_(self.img[key][k])
        self.wait()

    def read(self, names=None):
        self.wait()
        with self._on_stream():
            return {k: self.bufs[k][:self.size[k]].cpu().numpy() for k in (self.case.outputs if names is None else names)}

    def loaded(self, key, k):
        """the bytes load(key) puts into input / in-out buffer k"""
        return self.img[key][k].numpy() if k in self.img[key] else np.zeros(0, np.uint8)


def i32(a, at=0):
    return int(np.ascontiguousarray(a).view(np.uint8)[at:at + 4].view(np.int32)[0])


def header_K(rec):
    return i32(rec, _state["off_hdr"])


_state = {"off_hdr": 0}


def up(T):
    return np.ascontiguousarray(T, np.float32).reshape(-1)


# ---- the panning scene of tests/test_gpu_extents.py: tracking, mapping, the map-point table -------------------------------
def track_scene():
    """-> (S, [view A, view B]): A tracks record 2 (frame 3) from record 1, B tracks record 1 (frame 2) from record 2; the dust
    points, their descriptors and the local map are cut to the common count"""
    import test_gpu_extents as tge
    from tools import track_scene as ts
    import copy
    S = tge.build_scene()
    L = S.ext.layout
    _state["off_hdr"] = L.off_hdr
    # B's records: the same three frames with 5, 6 and 7 keypoints fewer in the header (the rows at and beyond K are never read)
    # and the cells of those keypoints emptied in the grid, so that every record B puts into a buffer has another K than A's
    SB = copy.copy(S)
    SB.raw = S.raw.copy()
    for f in range(len(tge.FRAMES)):
        K = S.recs[f].K - 5 - f
        SB.raw[f, L.off_hdr:L.off_hdr + 4].view(np.int32)[0] = K
        occ = SB.raw[f, L.off_occ:L.off_occ + 2 * (tge.H // 8) * (tge.W // 8)].view(np.int16)
        occ[occ >= K] = -1
    SB.recs = [S.ext.view_record(r) for r in SB.raw]
    assert [r.K for r in SB.recs] == [r.K - 5 - f for f, r in enumerate(S.recs)]
    views = []
    for Sx, (rl, rc, old) in ((S, (1, 2, 0)), (SB, (2, 1, 0))):
        v = types.SimpleNamespace(S=Sx, rl=rl, rc=rc, old=old, k_last=tge.FRAMES[rl], k_cur=tge.FRAMES[rc], last=Sx.recs[rl],
                                  cur=Sx.recs[rc])
        v.pts, v.mpd, v.sel = ts.map_points(v.last.kp_xy, v.last.descriptors, v.k_last, max_points=tge.N_POINTS)
        v.T0 = ts.pose(ts.offsets(v.k_cur)[0], ts.offsets(v.k_last)[1])      # x from the motion model, y from the last frame
        v.lm = ts.local_map([(tge.FRAMES[i], Sx.recs[i].kp_xy, Sx.recs[i].descriptors) for i in (old, rl)], tge.N_POINTS // 2,
                            max_points=tge.N_POINTS)
        v.sel_lm = ts.map_points(v.last.kp_xy, v.last.descriptors, v.k_last, max_points=tge.N_POINTS // 2)[2]
        v.T_near = ts.pose(*ts.offsets(v.k_cur)).copy()
        v.T_near[0, 3] += np.float32(0.4 * ts.Z0 / ts.FX)
        views.append(v)
    n = min(len(v.pts) for v in views)
    n_lm = min(len(v.lm["xyz"]) for v in views)
    for v in views:
        v.pts, v.mpd, v.sel, v.n = v.pts[:n], v.mpd[:n], v.sel[:n], n
        v.lm = {k: (a[:n_lm] if k != "n_dust" else a) for k, a in v.lm.items()}
        v.n_lm = n_lm
    assert not {r.K for r in S.recs} & {r.K for r in SB.recs}, [r.K for r in S.recs + SB.recs]
    return S, views


def two(build_spec, views):
    return build_spec(views[0]), build_spec(views[1])


def K_of(*names):
    return lambda spec, got: tuple(header_K(spec[k]) for k in names)


def pose_counts(e, name="d_pose_out"):
    def f(spec, got):
        g = e.decode_pose_out(got[name], e.layout.kmax)
        return (g["n_initial"], g["n_good"], g["n_matches"], g["verdict"])
    return f


def build_stage_batch():
    from oracle import oracle
    from sp_orb_slam_amd import weights
    from sp_orb_slam_amd.extractor import SPExtractor
    import test_gpu_stage as tst
    H, W, B, hs, ws = 120, 160, 2, 128, 176
    ext = SPExtractor(100, H, W, weights.synthetic(7, "dense"), max_batch=B, with_heat=False)
    mx, my = tst.undistort_maps(hs, ws)
    ext.set_staging(hs, ws, 3, False, mx, my)
    raws = [np.stack([tst._raw(np.random.default_rng(s + i), hs, ws, 3) for i in range(B)]) for s in (4, 40)]
    A, Bs = (dict(d_src=r, d_gray=B * H * W) for r in raws)

    def check(got):
        want = np.stack([oracle.stage_input(raws[0][i], H, W, mx, my) for i in range(B)])
        assert np.array_equal(got["d_gray"], want.reshape(-1)), "the gray frames differ from the oracle's"
    return Case(ext, A, Bs, lambda P, s: ext.stage_batch_device(P["d_src"], B, P["d_gray"], s), ("d_gray",), check)


def build_match_records():
    S, V = track_scene()
    e, F = S.ext, 2
    A = dict(d_query_records=np.concatenate([S.raw[2], S.raw[0]]), d_train_records=np.concatenate([S.raw[1], S.raw[2]]),
             d_out=F * S.dims["match"])
    SB = V[1].S
    B = dict(d_query_records=np.concatenate([SB.raw[0], SB.raw[1]]), d_train_records=np.concatenate([SB.raw[2], SB.raw[0]]),
             d_out=F * S.dims["match"])

    def check(got):
        for f, (q, t) in enumerate(((2, 1), (0, 2))):
            idx, dist = e.decode_match_out(got["d_out"][f * S.dims["match"]:(f + 1) * S.dims["match"]], S.recs[q].K)
            w_idx, w_dist = e.match(S.recs[q].descriptors, S.recs[t].descriptors)
            assert np.array_equal(idx, w_idx) and np.array_equal(dist.view(np.uint32), w_dist.view(np.uint32)), "pair %d" % f
    return Case(e, A, B, lambda P, s: e.match_records_device(P["d_query_records"], P["d_train_records"], F, P["d_out"], stream=s),
                ("d_out",), check, lambda spec, got: (header_K(spec["d_query_records"]), header_K(spec["d_train_records"])))


def build_match_patches_record():
    from tools import track_scene as ts
    S, V = track_scene()
    e = S.ext

    def spec(v):
        pan = np.subtract(ts.offsets(v.k_cur), ts.offsets(v.k_last))
        uv = ((v.last.kp_xy[v.sel] - pan - 3.5) / 8.0).astype(np.float32)
        return dict(d_mp_desc=v.mpd, d_mp_uv=uv, d_record=v.S.raw[v.rc], d_kp_idx=4 * v.n)
    A, B = two(spec, V)
    n = V[0].n

    def check(got):
        want = e.match_patches(V[0].mpd, A["d_mp_uv"], V[0].cur.occ_grid, V[0].cur.descriptors)
        assert np.array_equal(got["d_kp_idx"].view(np.int32), want) and (want >= 0).sum() > 20
    return Case(e, A, B, lambda P, s: e.match_patches_record_device(P["d_mp_desc"], P["d_mp_uv"], n, P["d_record"], P["d_kp_idx"],
                                                                    stream=s), ("d_kp_idx",), check, K_of("d_record"))


def dust_counts(e, n, name="d_out"):
    def f(spec, got):
        g = e.decode_dust_out(got[name][:tge_dust_bytes()], n)
        return (int(g["n_inlier"]), int(g["iterations"]))
    return f


def tge_dust_bytes():
    from sp_orb_slam_amd.extractor import DUST_OUT_BYTES
    return DUST_OUT_BYTES


def build_align_dust_record():
    import test_gpu_extents as tge
    S, V = track_scene()
    e, n = S.ext, V[0].n
    A, B = two(lambda v: dict(d_record=v.S.raw[v.rc], d_points_xyz=v.pts, d_Tcw=up(v.T0), d_out=tge.DUST_OUT_BYTES), V)

    def check(got):
        v = V[0]
        w = e.align_dust(v.cur.dense_dust, v.pts, v.T0, *tge.INTR)
        g = e.decode_dust_out(got["d_out"], n)
        assert g["n_inlier"] == w["n_inlier"] > 20 and g["iterations"] == w["iterations"], (g["n_inlier"], w["n_inlier"])
        assert np.array_equal(g["inlier"], w["inlier"]) and np.array_equal(g["Tcw"], w["Tcw"]), "pose / flags against the host form"
    return Case(e, A, B, lambda P, s: e.align_dust_record_device(P["d_record"], P["d_points_xyz"], n, P["d_Tcw"], P["d_out"],
                                                                 *tge.INTR, stream=s), ("d_out",), check, dust_counts(e, n))


def build_align_dust_batch():
    import test_gpu_extents as tge
    from tools import track_scene as ts
    S, V = track_scene()
    e, F = S.ext, 3

    def spec(v, counts, order):
        pts = np.zeros((F, tge.DUST_MAX_POINTS, 3), np.float32)
        pts[:, :v.n] = v.pts
        return dict(d_records=np.concatenate([v.S.raw[f] for f in order]), d_points_xyz=pts, d_n_points=np.array(counts, np.int32),
                    d_Tcw=np.concatenate([up(ts.start_pose(tge.FRAMES[f])) for f in order]), d_out=F * tge.DUST_OUT_BYTES)
    A, B = spec(V[0], [V[0].n, 0, 37], (0, 1, 2)), spec(V[1], [11, V[1].n, 0], (2, 0, 1))

    def check(got):
        g = e.decode_dust_out(got["d_out"][2 * tge.DUST_OUT_BYTES:], 37)     # frame 2: record 2, the first 37 dust points
        w = e.align_dust(S.recs[2].dense_dust, V[0].pts[:37], ts.start_pose(tge.FRAMES[2]), *tge.INTR)
        assert g["n_inlier"] == w["n_inlier"] and np.array_equal(g["Tcw"], w["Tcw"]), (g["n_inlier"], w["n_inlier"])
    return Case(e, A, B, lambda P, s: e.align_dust_batch_device(P["d_records"], F, P["d_points_xyz"], P["d_n_points"], P["d_Tcw"],
                                                                P["d_out"], *tge.INTR, stream=s), ("d_out",), check,
                lambda spec, got: tuple(spec["d_n_points"].tolist()))


def build_track_dust_record():
    import test_gpu_extents as tge
    S, V = track_scene()
    e, n = S.ext, V[0].n
    A, B = two(lambda v: dict(d_record=v.S.raw[v.rc], d_points_xyz=v.pts, d_mp_desc=v.mpd, d_Tcw=up(v.T0),
                              d_dust_out=tge.DUST_OUT_BYTES, d_kp_idx=4 * n), V)

    def check(got):
        assert e.decode_dust_out(got["d_dust_out"], n)["n_inlier"] > 20 and (got["d_kp_idx"].view(np.int32) >= 0).sum() > 20
    return Case(e, A, B, lambda P, s: e.track_dust_record_device(P["d_record"], P["d_points_xyz"], P["d_mp_desc"], n, P["d_Tcw"],
                                                                 P["d_dust_out"], P["d_kp_idx"], *tge.INTR, min_inliers=20, stream=s),
                ("d_dust_out", "d_kp_idx"), check, dust_counts(e, n, "d_dust_out"))


def build_refine_pose_record():
    import test_gpu_extents as tge
    S, V = track_scene()
    e = S.ext
    maps = [tge.association(v.S, v.rc, v.sel, k_from=v.k_last) for v in V]
    A, B = (dict(d_record=v.S.raw[v.rc], d_mp_of_kp=m, d_points_xyz=v.pts, d_Tcw=up(v.T0), d_out=S.dims["pose"])
            for v, m in zip(V, maps))

    def check(got):
        g = e.decode_pose_out(got["d_out"], tge.KMAX)
        assert g["n_good"] > 20 and g["n_initial"] == int((maps[0][:V[0].cur.K] >= 0).sum()), (g["n_good"], g["n_initial"])
    return Case(e, A, B, lambda P, s: e.refine_pose_record_device(P["d_record"], P["d_mp_of_kp"], P["d_points_xyz"], P["d_Tcw"],
                                                                  P["d_out"], *tge.INTR, stream=s), ("d_out",), check,
                pose_counts(e, "d_out"))


def build_refine_pose_batch():
    import test_gpu_extents as tge
    from tools import track_scene as ts
    S, V = track_scene()
    e, F, n = S.ext, 3, V[0].n
    empty = np.full(tge.KMAX, -1, np.int32)

    def spec(v, order, which):
        maps = [tge.association(v.S, f, v.sel, k_from=v.k_last) if f in which else empty for f in order]
        return dict(d_records=np.concatenate([v.S.raw[f] for f in order]), d_mp_of_kp=np.concatenate(maps),
                    d_points_xyz=np.tile(v.pts, (F, 1)), d_Tcw=np.concatenate([up(ts.start_pose(tge.FRAMES[f])) for f in order]),
                    d_out=F * S.dims["pose"])
    A, B = spec(V[0], (0, 1, 2), (0, 2)), spec(V[1], (1, 2, 0), (1, 0))

    def check(got):
        blocks = got["d_out"].reshape(F, -1)
        assert [e.decode_pose_out(b, tge.KMAX)["n_initial"] > 20 for b in blocks] == [True, False, True]
    return Case(e, A, B, lambda P, s: e.refine_pose_batch_device(P["d_records"], F, P["d_mp_of_kp"], P["d_points_xyz"], 3 * n,
                                                                 P["d_Tcw"], P["d_out"], *tge.INTR, stream=s), ("d_out",), check,
                lambda spec, got: tuple(e.decode_pose_out(b, tge.KMAX)["n_initial"] for b in got["d_out"].reshape(F, -1)))


def build_track_dust_refine_record():
    import test_gpu_extents as tge
    from sp_orb_slam_amd import extractor as X
    S, V = track_scene()
    e, n = S.ext, V[0].n
    A, B = two(lambda v: dict(d_record=v.S.raw[v.rc], d_points_xyz=v.pts, d_mp_desc=v.mpd, d_Tcw=up(v.T0),
                              d_dust_out=tge.DUST_OUT_BYTES, d_kp_idx=4 * n, d_pose_out=S.dims["pose"]), V)

    def check(got):
        assert e.decode_pose_out(got["d_pose_out"], tge.KMAX)["verdict"] == X.TRACK_OK
    return Case(e, A, B, lambda P, s: e.track_dust_refine_record_device(P["d_record"], P["d_points_xyz"], P["d_mp_desc"], n, P["d_Tcw"],
                                                                        P["d_dust_out"], P["d_kp_idx"], P["d_pose_out"], *tge.INTR,
                                                                        20, 20, 0.35, stream=s),
                ("d_dust_out", "d_kp_idx", "d_pose_out"), check, pose_counts(e))


def search_maps(S, V):
    import test_gpu_extents as tge
    from test_gpu_proj_search import make_map
    out = []
    for v, seed in zip(V, (5, 6)):
        m = make_map(v.cur, tge.N_POINTS, seed, tge.H, tge.W)
        out.append((m, tge.clean_entry(m, v.cur.K, tge.N_POINTS)))
    return out


def proj_counts(e, name="d_out"):
    def f(spec, got):
        g = e.decode_proj_out(got[name][:tge_proj_bytes()])
        return (g["n_matches"], g["n_to_match"])
    return f


def tge_proj_bytes():
    from sp_orb_slam_amd.extractor import PROJ_OUT_BYTES
    return PROJ_OUT_BYTES


def build_search_projection_record():
    import test_gpu_extents as tge
    import proj_ref
    S, V = track_scene()
    e, n = S.ext, tge.N_POINTS
    kw = dict(tge.SEARCHES[0], th_dist=0.7, view_cos_limit=0.5, adaptive=True, c2_thresh=81.0)
    ms = search_maps(S, V)
    A, B = (dict(d_record=v.S.raw[v.rc], d_xyz=m["xyz"], d_normal=m["normal"], d_desc=m["desc"], d_flags=m["flags"], d_mp_of_kp=entry,
                 d_Tcw=up(m["Tcw"]), d_out=tge.PROJ_OUT_BYTES) for v, (m, entry) in zip(V, ms))

    def check(got):
        S.refs = (None, proj_ref.build(mktemp("proj_ref")))
        want = tge.ref_search(S, V[0].cur, ms[0][0], n, ms[0][1], kw)
        tge.same_search(S, got["d_out"], got["d_mp_of_kp"].view(np.int32), want, n, "search against proj_ref.c")
        assert want["n_matches"] > 20
    return Case(e, A, B, lambda P, s: e.search_projection_record_device(P["d_record"], P["d_xyz"], P["d_normal"], P["d_desc"],
                                                                        P["d_flags"], n, P["d_mp_of_kp"], P["d_Tcw"], P["d_out"],
                                                                        *tge.INTR, stream=s, **kw),
                ("d_out", "d_mp_of_kp"), check, proj_counts(e))


def build_search_projection_batch():
    import test_gpu_extents as tge
    from test_gpu_proj_search import make_map
    S, V = track_scene()
    e, F, stride, kw = S.ext, 3, tge.N_POINTS, tge.SEARCHES[0]

    def spec(Sx, order, counts, seed):
        maps = [make_map(Sx.recs[f], stride, seed + f, tge.H, tge.W) for f in order]
        entries = [tge.clean_entry(m, Sx.recs[f].K, int(c)) for m, f, c in zip(maps, order, counts)]
        cat = {k: np.concatenate([m[k] for m in maps]) for k in ("xyz", "normal", "desc", "flags")}
        return dict(d_records=np.concatenate([Sx.raw[f] for f in order]), d_xyz=cat["xyz"], d_normal=cat["normal"], d_desc=cat["desc"],
                    d_flags=cat["flags"], d_n_points=np.array(counts, np.int32), d_mp_of_kp=np.concatenate(entries),
                    d_Tcw=np.concatenate([up(m["Tcw"]) for m in maps]), d_out=F * tge.PROJ_OUT_BYTES)
    A, B = spec(S, (0, 1, 2), [stride, 0, 37], 40), spec(V[1].S, (2, 0, 1), [53, stride, 0], 50)

    def counts(spec, got):
        return tuple(e.decode_proj_out(b)["n_matches"] for b in got["d_out"].reshape(F, -1)) + tuple(spec["d_n_points"].tolist())

    def check(got):
        blocks = got["d_out"].reshape(F, -1)
        assert [e.decode_proj_out(b)["n"] for b in blocks] == [stride, 0, 37] and e.decode_proj_out(blocks[0])["n_matches"] > 20
    return Case(e, A, B, lambda P, s: e.search_projection_batch_device(P["d_records"], F, P["d_xyz"], P["d_normal"], P["d_desc"],
                                                                       P["d_flags"], P["d_n_points"], stride, P["d_mp_of_kp"],
                                                                       P["d_Tcw"], P["d_out"], *tge.INTR, stream=s, **kw),
                ("d_out", "d_mp_of_kp"), check, counts)


def build_track_local_map_record():
    import test_gpu_extents as tge
    from sp_orb_slam_amd import extractor as X
    S, V = track_scene()
    e, n = S.ext, V[0].n_lm
    entries = [tge.association(v.S, v.rc, v.sel_lm, k_from=v.k_last, every=2) for v in V]
    A, B = (dict(d_record=v.S.raw[v.rc], d_xyz=v.lm["xyz"], d_normal=v.lm["normal"], d_desc=v.lm["desc"], d_flags=v.lm["flags"],
                 d_mp_of_kp=en, d_Tcw=up(v.T_near), d_proj_out=tge.PROJ_OUT_BYTES, d_pose_out=S.dims["pose"])
            for v, en in zip(V, entries))

    def check(got):
        g = e.decode_pose_out(got["d_pose_out"], tge.KMAX)
        assert g["verdict"] == X.TRACK_OK and g["n_matches"] > 20 and g["n_initial"] > (entries[0] >= 0).sum(), g
    return Case(e, A, B, lambda P, s: e.track_local_map_record_device(P["d_record"], P["d_xyz"], P["d_normal"], P["d_desc"],
                                                                      P["d_flags"], n, P["d_mp_of_kp"], P["d_Tcw"], P["d_proj_out"],
                                                                      P["d_pose_out"], *tge.INTR, tge.TH_NINLIER_LOW, stream=s),
                ("d_mp_of_kp", "d_proj_out", "d_pose_out"), check, pose_counts(e))


def build_track_motion_model_record():
    import test_gpu_extents as tge
    import track_cases as tc
    S, V = track_scene()
    e = S.ext
    ms = [tc.last_frame_points(v.last, v.k_last, v.k_cur, size=(tge.H, tge.W)) for v in V]
    n = min(len(m["xyz"]) for m in ms)
    A, B = (dict(d_record=v.S.raw[v.rc], d_xyz=m["xyz"][:n], d_desc=m["desc"][:n], d_flags=m["flags"][:n],
                 d_mp_of_kp=np.full(tge.KMAX, 12345, np.int32), d_Tcw=up(v.T0), d_proj_out=tge.PROJ_OUT_BYTES,
                 d_pose_out=S.dims["pose"]) for v, m in zip(V, ms))

    def check(got):
        g = e.decode_pose_out(got["d_pose_out"], tge.KMAX)
        assert g["widened"] == 0 and g["n_matches"] > 20, g
    return Case(e, A, B, lambda P, s: e.track_motion_model_record_device(P["d_record"], P["d_xyz"], P["d_desc"], P["d_flags"], n,
                                                                         P["d_mp_of_kp"], P["d_Tcw"], P["d_proj_out"],
                                                                         P["d_pose_out"], *tge.INTR, stream=s),
                ("d_mp_of_kp", "d_proj_out", "d_pose_out"), check, pose_counts(e))


def build_track_reference_kf_record():
    import test_gpu_extents as tge
    import track_cases as tc
    from sp_orb_slam_amd import extractor as X
    from tools import track_scene as ts
    S, V = track_scene()
    e = S.ext
    held = [tc.half_held(v.last, v.k_last, kmax=tge.KMAX) for v in V]
    n = min(len(p["xyz"]) for _, p in held)
    held = [(np.where(mp >= n, -1, mp).astype(np.int32), {k: a[:n] for k, a in p.items()}) for mp, p in held]
    A, B = (dict(d_record=v.S.raw[v.rc], d_kf_record=v.S.raw[v.rl], d_kf_mp_of_kp=mp, d_xyz=p["xyz"], d_flags=p["flags"],
                 d_mp_of_kp=np.full(tge.KMAX, 12345, np.int32), d_Tcw=up(ts.pose(*ts.offsets(v.k_last))), d_pose_out=S.dims["pose"])
            for v, (mp, p) in zip(V, held))

    def check(got):
        g = e.decode_pose_out(got["d_pose_out"], tge.KMAX)
        assert g["verdict"] == X.TRACK_OK and g["n_matches"] > 20, g
    return Case(e, A, B, lambda P, s: e.track_reference_kf_record_device(P["d_record"], P["d_kf_record"], P["d_kf_mp_of_kp"],
                                                                         P["d_xyz"], P["d_flags"], n, P["d_mp_of_kp"], P["d_Tcw"],
                                                                         P["d_pose_out"], *tge.INTR, stream=s),
                ("d_mp_of_kp", "d_pose_out"), check, pose_counts(e))


def tri_counts(e, F=1):
    def f(spec, got):
        import test_gpu_extents as tge
        return tuple(v for b in got["d_out"].reshape(F, -1) for v in (e.decode_tri_out(b, tge.KMAX)["n_matches"],
                                                                        e.decode_tri_out(b, tge.KMAX)["n_new"]))
    return f


def build_create_map_points_pair_record():
    import test_gpu_extents as tge
    S, V = track_scene()
    e = S.ext
    A, B = (dict(d_record1=Sx.raw[a], d_record2=Sx.raw[b], d_mp1_of_kp=tge.half_free(Sx, a, sd), d_mp2_of_kp=tge.half_free(Sx, b, sd + 1),
                 d_Tcw1=tge.frame_pose(tge.FRAMES[a]), d_Tcw2=tge.frame_pose(tge.FRAMES[b]), d_out=S.dims["tri"])
            for Sx, a, b, sd in ((S, 2, 1, 1), (V[1].S, 0, 2, 11)))

    def check(got):
        g = e.decode_tri_out(got["d_out"], tge.KMAX)
        assert g["status"] == 0 and g["n_matches"] > 0, g["n_matches"]
    return Case(e, A, B, lambda P, s: e.create_map_points_pair_record_device(P["d_record1"], P["d_record2"], P["d_mp1_of_kp"],
                                                                             P["d_mp2_of_kp"], P["d_Tcw1"], P["d_Tcw2"], P["d_out"],
                                                                             tge.INTR, point_base=5000, stream=s),
                ("d_mp1_of_kp", "d_mp2_of_kp", "d_out"), check, tri_counts(e))


def build_create_map_points_record():
    import test_gpu_extents as tge
    from tools import track_scene as ts
    S, V = track_scene()
    e, F = S.ext, 2
    A, B = (dict(d_record1=Sx.raw[a], d_record2_0=Sx.raw[b], d_record2_1=Sx.raw[c], d_mp1_of_kp=tge.half_free(Sx, a, sd),
                 d_mp2_of_kp=np.concatenate([tge.half_free(Sx, b, sd + 1), tge.half_free(Sx, c, sd + 2)]),
                 d_Tcw1=tge.frame_pose(tge.FRAMES[a]),
                 d_Tcw2=np.concatenate([tge.frame_pose(tge.FRAMES[b]), tge.frame_pose(tge.FRAMES[c])]), d_median_depth=md,
                 d_out=F * S.dims["tri"])
            for Sx, a, b, c, sd, md in ((S, 2, 1, 0, 1, np.full(F, ts.Z0, np.float32)),
                                        (V[1].S, 0, 2, 1, 11, np.array([1e6, ts.Z0], np.float32))))   # B: neighbour 0 skipped ON THE DEVICE

    def check(got):
        blocks = [e.decode_tri_out(b, tge.KMAX) for b in got["d_out"].reshape(F, -1)]
        assert all(b["status"] == 0 and b["skipped"] == 0 for b in blocks) and blocks[0]["n_matches"] > 0

    def counts(spec, got):
        return tri_counts(e, F)(spec, got) + tuple(e.decode_tri_out(b, tge.KMAX)["skipped"] for b in got["d_out"].reshape(F, -1))
    return Case(e, A, B, lambda P, s: e.create_map_points_record_device(P["d_record1"], [P["d_record2_0"], P["d_record2_1"]],
                                                                        P["d_mp1_of_kp"], P["d_mp2_of_kp"], P["d_Tcw1"], P["d_Tcw2"],
                                                                        P["d_median_depth"], P["d_out"], tge.INTR, point_base=5000,
                                                                        stream=s),
                ("d_mp1_of_kp", "d_mp2_of_kp", "d_out"), check, counts)


def build_loop_match_record():
    import test_gpu_extents as tge
    S, V = track_scene()
    e = S.ext
    A, B = (dict(d_record1=Sx.raw[a], d_record2=Sx.raw[b], d_kf1_mp_of_kp=tge.half_free(Sx, a, sd),
                 d_kf2_mp_of_kp=tge.half_free(Sx, b, sd + 1), d_match12=4 * tge.KMAX, d_n_matches=4)
            for Sx, a, b, sd in ((S, 2, 0, 6), (V[1].S, 1, 2, 16)))

    def check(got):
        r1, r2, mp1, mp2 = S.recs[2], S.recs[0], A["d_kf1_mp_of_kp"], A["d_kf2_mp_of_kp"]
        h1, h2 = np.flatnonzero(mp1[:r1.K] >= 0), np.flatnonzero(mp2[:r2.K] >= 0)
        idx, _ = e.match(r2.descriptors[h2], r1.descriptors[h1])            # queries: record 2's rows, train: record 1's
        want = np.full(tge.KMAX, -1, np.int32)
        for q, t in enumerate(idx):
            if t >= 0:
                want[h1[t]] = h2[q]
        m12 = got["d_match12"].view(np.int32)
        n = i32(got["d_n_matches"])
        assert n == (m12 >= 0).sum() > 20 and np.array_equal(m12, want), "match12 against spfe_match on the compacted rows"
    return Case(e, A, B, lambda P, s: e.loop_match_record_device(P["d_record1"], P["d_record2"], P["d_kf1_mp_of_kp"],
                                                                 P["d_kf2_mp_of_kp"], P["d_match12"], P["d_n_matches"], stream=s),
                ("d_match12", "d_n_matches"), check, lambda spec, got: (i32(got["d_n_matches"]),))


# ---- the map-point table on the same scene --------------------------------------------------------------------------------
def table_of(S, v, seed):
    """the fuse point list of a view as the table, B's perturbed"""
    from tools import track_scene as ts
    n = v.n_lm
    rng = np.random.default_rng(seed)
    return dict(d_xyz=(v.lm["xyz"] + rng.normal(0, 0.01, (n, 3))).astype(np.float32), d_flags=v.lm["flags"].copy(),
                d_normal=v.lm["normal"], d_dist_range=np.tile(np.array([0.5 * ts.Z0, 2.0 * ts.Z0], np.float32), (n, 1)) * np.float32(seed),
                d_desc=v.lm["desc"])


def build_refresh_map_points():
    import test_gpu_extents as tge
    from sp_orb_slam_amd import extractor as X
    from tools import track_scene as ts
    S, V = track_scene()
    e, F, n = S.ext, 3, V[0].n_lm
    counts = [1, 2, 3, 5, 16, 17, 41, 0, 4, 7, 2, 64, 3, 6, 9, 2, 33, 5]
    m, E = len(counts), int(np.sum(counts))
    RECS = ["d_record_%d" % f for f in range(F)]

    def spec(v, order, seed, kf_flags):
        rng = np.random.default_rng(seed)
        c = list(rng.permutation(counts))
        obs = np.array([(f, int(rng.integers(v.S.recs[order[f]].K))) for k in c for f in rng.integers(0, F, k)], np.int32).reshape(-1, 2)
        t = table_of(S, v, seed)
        return dict({RECS[f]: v.S.raw[order[f]] for f in range(F)}, d_kf_records=8 * F, d_kf_flags=np.array(kf_flags, np.uint8),
                    d_Tcw=np.stack([up(ts.pose(*ts.offsets(tge.FRAMES[f]))) for f in order]),
                    d_obs_start=np.concatenate([[0], np.cumsum(c)]).astype(np.int32), d_obs=obs,
                    d_ref_slot=rng.integers(0, F, m).astype(np.int32), d_xyz=t["d_xyz"], d_flags=t["d_flags"], d_normal=12 * n,
                    d_dist_range=8 * n, d_desc=1024 * n, d_out=X.mp_offsets(m)["out_bytes"], d_point_idx=rng.permutation(n)[:m].astype(np.int32))
    A, B = spec(V[0], (0, 1, 2), 3, [0, 1, 0]), spec(V[1], (2, 0, 1), 4, [0, 0, 1])
    for s_ in (A, B):
        s_["d_kf_records"] = np.zeros(F, np.int64)       # filled with the buffers' addresses (Case.pointers)

    def check(got):
        g = X.SPExtractor.decode_mp_out(got["d_out"], m)
        assert g["m"] == m and g["n_desc_written"] >= 10 and (g["code"] <= X.MP_NO_OBS).any() and g["n_good"].max() > X.MP_WAVE_OBS
        unlisted = np.setdiff1d(np.arange(n), A["d_point_idx"])
        assert (got["d_desc"].reshape(n, 1024)[unlisted] == FILL).all() and (got["d_normal"].reshape(n, 12)[unlisted] == FILL).all()

    def call(P, s):
        e.refresh_map_points_device(P["d_kf_records"], P["d_kf_flags"], P["d_Tcw"], F, P["d_point_idx"], P["d_obs_start"], P["d_obs"],
                                    P["d_ref_slot"], m, E, P["d_xyz"], P["d_flags"], P["d_normal"], P["d_dist_range"], P["d_desc"], n,
                                    P["d_out"], stream=s)

    def cnt(spec, got):
        g = X.SPExtractor.decode_mp_out(got["d_out"], m)
        return (g["n_desc_written"], g["n_nd_written"]) + tuple(g["n_good"].tolist())
    return Case(e, A, B, call, ("d_normal", "d_dist_range", "d_desc", "d_out"), check, cnt, pointers={"d_kf_records": RECS})


def build_gather_map_points():
    S, V = track_scene()
    e, g, n = S.ext, 37, V[0].n_lm
    outs = ("d_point_id", "d_list_xyz", "d_list_normal", "d_list_dist_range", "d_list_desc", "d_list_flags")

    def spec(v, seed):
        idx = np.random.default_rng(seed).integers(0, n, g).astype(np.int32)
        idx[[3 + seed % 3, 11 + seed % 5]] = (-1, n)                         # not followed
        return dict(table_of(S, v, seed), d_idx=idx, d_point_id=4 * g, d_list_xyz=12 * g, d_list_normal=12 * g, d_list_dist_range=8 * g,
                    d_list_desc=1024 * g, d_list_flags=g)
    A, B = spec(V[0], 4), spec(V[1], 5)

    def check(got):
        idx = A["d_idx"]
        ok = (idx >= 0) & (idx < n)
        row = np.clip(idx, 0, n - 1)
        assert np.array_equal(got["d_point_id"].view(np.int32), idx)
        assert np.array_equal(got["d_list_flags"], np.where(ok, A["d_flags"][row], 0))
        for name, src in (("d_list_desc", "d_desc"), ("d_list_xyz", "d_xyz"), ("d_list_normal", "d_normal"), ("d_list_dist_range", "d_dist_range")):
            assert got[name].tobytes() == np.where(ok[:, None], A[src][row], np.float32(0)).tobytes(), name

    def call(P, s):
        e.gather_map_points_device(P["d_idx"], g, P["d_xyz"], P["d_flags"], P["d_normal"], P["d_dist_range"], P["d_desc"], n,
                                   *[P[k] for k in outs], stream=s)
    return Case(e, A, B, call, outs, check)


# ---- fuse and loop fuse: generated targets on the 64 x 96 frame, bf16 rows ------------------------------------------------
def small_handle(nf=100, bf16=False):
    from sp_orb_slam_amd import weights
    from sp_orb_slam_amd.extractor import SPExtractor
    ext = SPExtractor(nf, 64, 96, weights.synthetic(7, "trackable"), with_heat=False, desc_bf16=bf16)
    _state["off_hdr"] = ext.layout.off_hdr
    return ext


def fuse_targets(loop, seeds, Ks):
    """generated targets with bf16-valued rows (record and reference see the same numbers) and their points"""
    import fuse_ref
    import test_gpu_fuse as tgf
    import test_gpu_loop_fuse as tlf
    out = []
    for j, (seed, K) in enumerate(zip(seeds, Ks)):
        if j == 0:
            t = (tlf.big_target(seed, 65, s=1.0 + 0.25 * seed) if loop else tgf.big_target(seed, 65))
            t["kp_desc"] = fuse_ref.widen_bf16(fuse_ref.to_bf16(t["kp_desc"]))
        else:       # the same view a quarter of a pixel on (every keypoint stays in its cell): the shared list finds it too
            t = {k: np.array(v, copy=True) for k, v in out[0].items()}
            t["kp_xy"] = (t["kp_xy"] + np.float32(0.25 * j)).astype(np.float32)
        t["K"] = K
        out.append(t)
    return out


def fuse_case(loop, n_targets):
    import fuse_ref
    import loopfuse_ref
    import test_gpu_fuse as tgf
    import test_gpu_loop_fuse as tlf
    from tools import track_scene as ts
    ext = small_handle(bf16=True)
    n, intr = 40, (ts.FX / 4, ts.FY / 4, 47.5, 31.25)
    mod, pose = (tlf, "Scw") if loop else (tgf, "Tcw")
    sets = []
    for seeds, Ks, pseed in (((11, 12), (65, 63), 13), ((21, 22), (60, 64), 23)):
        tg = fuse_targets(loop, seeds[:n_targets], Ks)
        p = mod.points_on(tg[0], n, pseed, intr)
        p["flags"][:3] = 1
        for j, t in enumerate(tg):
            t["kf_mp"][[5 + j, 9]] = (p["point_id"][2 - j], 77)              # a point that is in the keyframe; a holder
        sets.append((tg, p))
    recn = ["d_record_%d" % j for j in range(n_targets)] if n_targets > 1 else ["d_record"]

    def spec(tg, p):
        s_ = {recn[j]: tgf.record_host(ext, t, K=t["K"]) for j, t in enumerate(tg)}
        s_.update(d_kf_mp_of_kp=np.concatenate([tgf.padded(ext, t["kf_mp"]) for t in tg]),
                  d_pose=np.concatenate([up(t[pose]) for t in tg]), d_out=n_targets * ext.fuse_out_bytes(n))
        s_.update({"d_" + k: p[k] for k in ("point_id", "xyz", "normal", "dist_range", "desc", "flags")})
        return s_
    A, B = (spec(tg, p) for tg, p in sets)
    pts = lambda P: [P["d_" + k] for k in ("point_id", "xyz", "normal", "dist_range", "desc", "flags")]   # noqa: E731
    if n_targets == 1:
        fn = ext.loop_fuse_record_device if loop else ext.fuse_record_device
        call = lambda P, s: fn(P["d_record"], P["d_kf_mp_of_kp"], P["d_pose"], *pts(P), n, P["d_out"], *intr, stream=s)   # noqa: E731
    else:
        fn = ext.loop_fuse_targets_record_device if loop else ext.fuse_targets_record_device
        call = lambda P, s: fn([P[r] for r in recn], P["d_kf_mp_of_kp"], P["d_pose"], *pts(P), n, P["d_out"], *intr, stream=s)   # noqa: E731

    def check(got):
        L = (loopfuse_ref if loop else fuse_ref).build(mktemp("fuse_ref"))
        tg, p = sets[0]
        fused = []
        for j, t in enumerate(tg):
            want = mod.ref_run(L, t, p, n, t["K"], intr)
            g = ext.decode_fuse_out(got["d_out"].reshape(n_targets, -1)[j], n)
            tgf.same(g, want, ("target", j))
            fused.append(want["n_fused"])
        assert min(fused) > 0, fused

    def counts(spec, got):
        return tuple(ext.decode_fuse_out(b, n)["n_fused"] for b in got["d_out"].reshape(n_targets, -1)) + \
            tuple(header_K(spec[r]) for r in recn)
    return Case(ext, A, B, call, ("d_out",), check, counts)


# ---- the loop closer's chain on generated keyframes of 80 keypoints (tests/guided_ref/guided_cases.py) ------------------------
N_HYP, JOBS = 8, [(1, 0), (0, 7), (0, 0), (1, 7)]
MAP = ("xyz", "flags", "dist_range", "desc")


LOOP_KMAX = 80


def loop_case(seed, rows_bf16):
    """the arrays of loop_inputs that need no handle (numpy only: tests/test_loop_extent_cases.py runs the CPU references on
    them) -> (case, dict(d_kf1_mp_of_kp [kmax], d_kf2_mp_of_kp [2][kmax], the map, the poses, d_rand_u32))"""
    import guided_cases as gc
    import guided_ref
    kmax = LOOP_KMAX
    c = gc.large(K=kmax, H=64, W=96, seed=seed, n_seed=12)
    if rows_bf16:
        for kf in (c["kf1"], c["kf2"]):
            kf["kp_desc"] = guided_ref.widen_bf16(guided_ref.to_bf16(kf["kp_desc"]))
    rng = np.random.default_rng(17 + seed)
    mp2 = np.stack([np.ascontiguousarray(c["kf2"]["kf_mp"], np.int32)] * 2)
    mp2[0, rng.random(kmax) < 0.2] = -1
    T = np.eye(4, dtype=np.float32).reshape(16)
    return c, dict(d_kf1_mp_of_kp=np.array(c["kf1"]["kf_mp"], np.int32), d_kf2_mp_of_kp=mp2, d_xyz=c["xyz"],
                   d_flags=c["flags"], d_dist_range=c["dist_range"], d_desc=c["desc"], d_Tcw1=T, d_Tcw2=np.stack([T, T]),
                   d_rand_u32=rng.integers(0, 1 << 32, (2, N_HYP, 3), dtype=np.uint64).astype(np.uint32))


def loop_inputs(ext, seed, K1, K2, rows_bf16):
    """keyframe 1 and two candidates (the second keyframe twice, candidate 0 holding fewer points) -> (case, spec of the inputs
    every loop form shares); K1 / K2: the counts in the record headers (rows beyond them are never read)"""
    import test_gpu_fuse as tgf
    assert ext.layout.kmax == LOOP_KMAX
    c, arrays = loop_case(seed, rows_bf16)
    spec = dict(d_record1=tgf.record_host(ext, c["kf1"], K=K1), d_record2_0=tgf.record_host(ext, c["kf2"], K=K2),
                d_record2_1=tgf.record_host(ext, c["kf2"], K=K2), **arrays)
    return c, spec


LOOP_SETS = ((3, 80, 80), (5, 76, 73))          # (seed, K1, K2) of A and of B


def verify_call(ext, c):
    n = len(c["flags"])
    return lambda P, s: ext.loop_verify_records_device(P["d_record1"], [P["d_record2_0"], P["d_record2_1"]], P["d_kf1_mp_of_kp"],
                                                       P["d_kf2_mp_of_kp"], P["d_xyz"], P["d_flags"], n, P["d_Tcw1"], P["d_Tcw2"],
                                                       P["d_rand_u32"], N_HYP, P["d_match12"], P["d_n_matches"], P["d_verify_out"],
                                                       c["intr"], min_inliers=12, stream=s)


def verify_spec(ext, base):
    return dict(base, d_match12=4 * 2 * ext.layout.kmax, d_n_matches=8, d_verify_out=2 * ext.sim3_out_bytes(N_HYP))


def guided_call(ext, c):
    n = len(c["flags"])
    return lambda P, s: ext.loop_guided_match_records_device(P["d_record1"], [P["d_record2_0"], P["d_record2_1"]], JOBS,
                                                             P["d_kf1_mp_of_kp"], P["d_kf2_mp_of_kp"], P["d_xyz"], P["d_flags"],
                                                             P["d_dist_range"], P["d_desc"], n, P["d_Tcw1"], P["d_Tcw2"], P["d_match12"],
                                                             P["d_verify_out"], N_HYP, P["d_guided_out"], c["intr"], stream=s)


def verify_blocks(ext, raw):
    ob = ext.sim3_out_bytes(N_HYP)
    return [ext.decode_sim3_out(raw[j * ob:(j + 1) * ob], ext.layout.kmax, N_HYP) for j in range(2)]


def build_loop_verify_records():
    ext = small_handle(79)
    sets = [loop_inputs(ext, *s_, rows_bf16=False) for s_ in LOOP_SETS]
    A, B = (verify_spec(ext, spec) for _, spec in sets)
    c = sets[0][0]

    def check(got):
        blocks = verify_blocks(ext, got["d_verify_out"])
        nm = got["d_n_matches"].view(np.int32)
        assert all(b["best_h"] >= 0 and b["N"] >= 12 for b in blocks) and (nm >= [b["N"] for b in blocks]).all(), [(b["N"], b["best_h"]) for b in blocks]
        # the two single forms per candidate, byte for byte (the statement of spfe.h)
        ob, kmax = ext.sim3_out_bytes(N_HYP), ext.layout.kmax
        for j in range(2):
            one = dict(A, d_record2=A["d_record2_%d" % j], d_kf2=A["d_kf2_mp_of_kp"][j].copy(), d_T2=A["d_Tcw2"][j].copy(),
                       d_r=A["d_rand_u32"][j].copy(), d_m=4 * kmax, d_n=4, d_o=ob)
            n = len(c["flags"])

            def single(P, s):
                ext.loop_match_record_device(P["d_record1"], P["d_record2"], P["d_kf1_mp_of_kp"], P["d_kf2"], P["d_m"], P["d_n"])
                ext.sim3_ransac_device(80, P["d_m"], P["d_kf1_mp_of_kp"], P["d_kf2"], P["d_xyz"], P["d_flags"], n, P["d_Tcw1"], P["d_T2"],
                                       P["d_r"], N_HYP, P["d_o"], c["intr"], min_inliers=12)
            w = direct({k: v for k, v in one.items() if not (is_out(v) and k not in ("d_m", "d_n", "d_o"))}, single, ("d_m", "d_n", "d_o"))
            assert np.array_equal(w["d_m"], got["d_match12"][4 * kmax * j:4 * kmax * (j + 1)]), ("match12", j)
            assert np.array_equal(w["d_n"], got["d_n_matches"][4 * j:4 * j + 4]), ("n_matches", j)
            assert np.array_equal(w["d_o"], got["d_verify_out"][ob * j:ob * (j + 1)]), ("block", j)
    return Case(ext, A, B, verify_call(ext, c), ("d_match12", "d_n_matches", "d_verify_out"), check,
                lambda spec, got: tuple(got["d_n_matches"].view(np.int32).tolist()) + tuple(b["N"] for b in verify_blocks(ext, got["d_verify_out"])))


def build_sim3_ransac():
    import sim3_cases as sc
    import sim3_ref
    ext = small_handle(100)
    kmax = ext.layout.kmax
    g = sc.load("outliers40")
    K1, n, n_hyp = int(g["K1"]), len(g["flags"]), len(g["rnd"])
    rng = np.random.default_rng(1)
    m12 = np.asarray(g["match12"]).copy()
    m12[::5] = -1                                                           # B: fewer pairs, another map, other draws
    gB = dict(match12=m12, mp1=np.roll(np.asarray(g["mp1"]), 2), mp2=np.roll(np.asarray(g["mp2"]), 1), xyz=(g["xyz"] + rng.normal(0, 0.01, g["xyz"].shape)).astype(np.float32),
              flags=np.where(rng.random(n) < 0.9, g["flags"], 0).astype(np.uint8), Tcw1=g["Tcw2"], Tcw2=g["Tcw1"],
              rnd=rng.integers(0, 1 << 32, (n_hyp, 3), dtype=np.uint64).astype(np.uint32))
    A, B = (dict(d_match12=sim3_ref.pad(x["match12"], kmax), d_kf1_mp_of_kp=sim3_ref.pad(x["mp1"], kmax),
                 d_kf2_mp_of_kp=sim3_ref.pad(x["mp2"], kmax), d_xyz=x["xyz"], d_flags=x["flags"], d_Tcw1=up(x["Tcw1"]), d_Tcw2=up(x["Tcw2"]),
                 d_rand_u32=np.ascontiguousarray(x["rnd"], np.uint32), d_out=ext.sim3_out_bytes(n_hyp)) for x in (g, gB))

    def check(got):
        L = sim3_ref.build(mktemp("sim3_ref"))
        d, want, _, _ = sc.run_ref(L, g, kcap=kmax, rnd=g["rnd"], fill=FILL)
        assert np.array_equal(got["d_out"], want) and sc.differences(g, d) == [], "the block against sim3_ref.c"
    return Case(ext, A, B, lambda P, s: ext.sim3_ransac_device(K1, P["d_match12"], P["d_kf1_mp_of_kp"], P["d_kf2_mp_of_kp"], P["d_xyz"],
                                                               P["d_flags"], n, P["d_Tcw1"], P["d_Tcw2"], P["d_rand_u32"], n_hyp,
                                                               P["d_out"], g["intr1"], g["intr2"], min_inliers=int(g["min_inliers"]),
                                                               fix_scale=int(g["fix_scale"]), stream=s),
                ("d_out",), check, lambda spec, got: (i32(got["d_out"], 0), i32(got["d_out"], 12)))


def guided_single_spec(ext, c, base, T12, seed12):
    import test_gpu_fuse as tgf
    s_ = {k: base[k] for k in ("d_record1", "d_kf1_mp_of_kp", "d_xyz", "d_flags", "d_dist_range", "d_desc", "d_Tcw1")}
    s_.update(d_record2=base["d_record2_1"], d_kf2_mp_of_kp=base["d_kf2_mp_of_kp"][1].copy(), d_Tcw2=base["d_Tcw2"][1].copy(),
              d_T12=np.asarray(T12, np.float32).reshape(13), d_seed12=tgf.padded(ext, seed12, fill=7))
    return s_


def guided_single_call(ext, c):
    n = len(c["flags"])
    return lambda P, s: ext.search_by_sim3_record_device(P["d_record1"], P["d_record2"], P["d_kf1_mp_of_kp"], P["d_kf2_mp_of_kp"],
                                                         P["d_xyz"], P["d_flags"], P["d_dist_range"], P["d_desc"], n, P["d_Tcw1"],
                                                         P["d_Tcw2"], P["d_T12"], P["d_seed12"], P["d_out"], c["intr"], stream=s)


def guided_counts(ext, n_blocks=1, name="d_out"):
    return lambda spec, got: tuple(int(v) for b in got[name].reshape(n_blocks, -1) for v in b[:12].view(np.int32))


def build_search_by_sim3_record():
    import guided_ref
    import test_gpu_guided_match as tgm
    ext = small_handle(79, bf16=True)
    sets = [loop_inputs(ext, *s_, rows_bf16=True) for s_ in LOOP_SETS]
    A, B = (dict(guided_single_spec(ext, c, base, c["T12"] if i == 0 else c["T12"] * np.float32(1.01), c["seed12"]), d_out=ext.guided_out_bytes())
            for i, (c, base) in enumerate(sets))
    c = sets[0][0]

    def check(got):
        L = guided_ref.build(mktemp("guided_ref"))
        kf2 = dict(c["kf2"], kf_mp=A["d_kf2_mp_of_kp"][:80])
        want = guided_ref.search(L, c["kf1"], kf2, c["xyz"], c["flags"], c["dist_range"], c["desc"], np.eye(4), np.eye(4), c["T12"],
                                 c["seed12"], c["intr"], 96, 64, kcap=80)
        tgm.same(ext.decode_guided_out(got["d_out"], 80, 80, 80), want, "record form against guided_ref.c")
        assert want["n_found"] >= 5
    return Case(ext, A, B, guided_single_call(ext, c), ("d_out",), check, guided_counts(ext))


def chain_sets(ext, rows_bf16, upto):
    """the chain verify [-> guided] run directly on A's and B's inputs -> [(case, spec with the blocks of the chain as inputs)]"""
    out = []
    for s_ in LOOP_SETS:
        c, base = loop_inputs(ext, *s_, rows_bf16=rows_bf16)
        got = direct(verify_spec(ext, base), verify_call(ext, c), ("d_match12", "d_n_matches", "d_verify_out"))
        spec = dict(base, d_match12=got["d_match12"], d_verify_out=got["d_verify_out"])
        if upto == "guided":
            g = direct(dict(spec, d_guided_out=len(JOBS) * ext.guided_out_bytes()), guided_call(ext, c), ("d_guided_out",))
            spec["d_guided_out"] = g["d_guided_out"]
        out.append((c, spec))
    return out


def build_loop_guided_match_records():
    ext = small_handle(79, bf16=True)
    sets = chain_sets(ext, True, "verify")
    gb = ext.guided_out_bytes()
    A, B = (dict(spec, d_guided_out=len(JOBS) * gb) for _, spec in sets)
    c = sets[0][0]

    def check(got):
        blocks = verify_blocks(ext, A["d_verify_out"])
        m12 = A["d_match12"].view(np.int32).reshape(2, 80)
        assert all(b["best_h"] >= 0 for b in blocks), "A's verify blocks are evaluated"
        for q, (j, h) in enumerate(JOBS):                                    # the single form fed from the decoded verify block
            seed = np.where(blocks[j]["vbInliers"][h], m12[j], -1).astype(np.int32)
            one = guided_single_spec(ext, c, A, blocks[j]["T12"][h], seed)
            one.update(d_record2=A["d_record2_%d" % j], d_kf2_mp_of_kp=A["d_kf2_mp_of_kp"][j].copy(), d_Tcw2=A["d_Tcw2"][j].copy(), d_out=gb)
            w = direct(one, guided_single_call(ext, c), ("d_out",))
            assert np.array_equal(w["d_out"], got["d_guided_out"][q * gb:(q + 1) * gb]), ("job", q, j, h)
    return Case(ext, A, B, guided_call(ext, c), ("d_guided_out",), check, guided_counts(ext, len(JOBS), "d_guided_out"))


def opt_counts(ext, n_blocks=1):
    return lambda spec, got: tuple(int(v) for b in got["d_out"].reshape(n_blocks, -1) for v in b[:36].view(np.int32))


def build_optimize_sim3_record():
    import sim3opt_ref
    import test_gpu_optimize_sim3 as tos
    ext = small_handle(79)
    sets = []
    for s_ in LOOP_SETS:
        c, base = loop_inputs(ext, *s_, rows_bf16=False)
        one = dict(guided_single_spec(ext, c, base, c["T12"], c["seed12"]), d_out=ext.guided_out_bytes())
        g = ext.decode_guided_out(direct(one, guided_single_call(ext, c), ("d_out",))["d_out"], 80, s_[1], s_[2])
        spec = {k: one[k] for k in ("d_record1", "d_record2", "d_kf1_mp_of_kp", "d_kf2_mp_of_kp", "d_xyz", "d_flags", "d_Tcw1", "d_Tcw2", "d_T12")}
        spec.update(d_matches12=g["matches12"].astype(np.int32), d_out=ext.sim3opt_out_bytes())
        sets.append((c, spec))
    (c, A), (_, B) = sets
    n = len(c["flags"])

    def check(got):
        L = sim3opt_ref.build(mktemp("sim3opt_ref"))
        r = ext.decode_sim3opt_out(got["d_out"], 80)
        case = dict(kp_xy1=c["kf1"]["kp_xy"], kp_xy2=c["kf2"]["kp_xy"], mp1=c["kf1"]["kf_mp"], mp2=A["d_kf2_mp_of_kp"][:80], xyz=c["xyz"],
                    flags=c["flags"], Tcw1=np.eye(4), Tcw2=np.eye(4), T12=c["T12"], matches12=A["d_matches12"][:80])
        want = sim3opt_ref.solve(L, case, sim3opt_ref.params([float(v) for v in c["intr"]], min_inliers=5))
        assert r["n_corr"] > 0, r["n_corr"]
        if want["chi2_margin"] >= 1e-5 and np.isfinite(want["S12"]).all():
            tos.same(r, want, np.eye(4), A["d_kf2_mp_of_kp"][:80], L, "record form against sim3opt_ref.c")
    return Case(ext, A, B, lambda P, s: ext.optimize_sim3_record_device(P["d_record1"], P["d_record2"], P["d_kf1_mp_of_kp"],
                                                                        P["d_kf2_mp_of_kp"], P["d_xyz"], P["d_flags"], n, P["d_Tcw1"],
                                                                        P["d_Tcw2"], P["d_T12"], P["d_matches12"], P["d_out"], c["intr"],
                                                                        min_inliers=5, stream=s), ("d_out",), check, opt_counts(ext))


def build_loop_optimize_sim3_records():
    ext = small_handle(79)
    sets = chain_sets(ext, False, "guided")
    sb, gb = ext.sim3opt_out_bytes(), ext.guided_out_bytes()
    A, B = (dict(spec, d_out=len(JOBS) * sb) for _, spec in sets)
    c = sets[0][0]
    n = len(c["flags"])

    def call(P, s):
        ext.loop_optimize_sim3_records_device(P["d_record1"], [P["d_record2_0"], P["d_record2_1"]], JOBS, P["d_kf1_mp_of_kp"],
                                              P["d_kf2_mp_of_kp"], P["d_xyz"], P["d_flags"], n, P["d_Tcw1"], P["d_Tcw2"], P["d_verify_out"],
                                              N_HYP, P["d_guided_out"], P["d_out"], c["intr"], min_inliers=5, stream=s)

    def check(got):
        blocks = verify_blocks(ext, A["d_verify_out"])
        for q, (j, h) in enumerate(JOBS):                                    # the record form fed with the decoded hypothesis and matches
            gd = ext.decode_guided_out(A["d_guided_out"][q * gb:(q + 1) * gb], 80, 80, 80)
            one = {k: A[k] for k in ("d_record1", "d_kf1_mp_of_kp", "d_xyz", "d_flags", "d_Tcw1")}
            one.update(d_record2=A["d_record2_%d" % j], d_kf2=A["d_kf2_mp_of_kp"][j].copy(), d_T2=A["d_Tcw2"][j].copy(),
                       d_T12=np.ascontiguousarray(blocks[j]["T12"][h], np.float32), d_m12=gd["matches12"].astype(np.int32), d_o=sb)
            w = direct(one, lambda P, s: ext.optimize_sim3_record_device(P["d_record1"], P["d_record2"], P["d_kf1_mp_of_kp"], P["d_kf2"],
                                                                         P["d_xyz"], P["d_flags"], n, P["d_Tcw1"], P["d_T2"], P["d_T12"],
                                                                         P["d_m12"], P["d_o"], c["intr"], min_inliers=5), ("d_o",))
            assert np.array_equal(w["d_o"], got["d_out"][q * sb:(q + 1) * sb]), ("job", q, j, h)
    return Case(ext, A, B, call, ("d_out",), check, opt_counts(ext, len(JOBS)))


def build_search_loop_points_record():
    import guided_cases as gc
    import guided_ref
    import test_gpu_fuse as tgf
    import test_gpu_loop_points as tlp
    ext = small_handle(100)
    n, kmax = 150, ext.layout.kmax
    gs = [(gc.lp_large(n=n, K=80, H=64, W=96, seed=sd), K) for sd, K in ((0, 80), (1, 71))]

    def spec(g, K):
        m0 = np.full(kmax, 12345, np.int32)
        m0[:K] = g["matched"][:K]
        return dict({"d_" + k: g[k] for k in gc.POINT_KEYS}, d_record=tgf.record_host(ext, g, K=K), d_Scw=up(g["Scw"]), d_matched=m0,
                    d_out=ext.loop_proj_out_bytes(n))
    A, B = (spec(g, K) for g, K in gs)
    g0 = gs[0][0]
    intr = [float(v) for v in g0["intr"]]

    def check(got):
        L = guided_ref.build(mktemp("guided_ref"))
        want = gc.lp_ref(L, g0)
        tlp.same(ext.decode_loop_proj_out(got["d_out"], n), got["d_matched"].view(np.int32), want, "against the sequential loop")
        assert want["n_matched"] > 10 and (got["d_matched"].view(np.int32)[80:] == 12345).all()
    return Case(ext, A, B, lambda P, s: ext.search_loop_points_record_device(P["d_record"], P["d_Scw"], P["d_matched"],
                                                                             *[P["d_" + k] for k in gc.POINT_KEYS], n, P["d_out"], *intr,
                                                                             n_cap=n, stream=s),
                ("d_out", "d_matched"), check, lambda spec, got: (i32(got["d_out"]), header_K(spec["d_record"])))


def opt_block(ext, S12):
    from sp_orb_slam_amd import extractor as X
    blk = np.full(ext.sim3opt_out_bytes(), FILL, np.uint8)
    blk[X.SIM3OPT_OFF_S12:X.SIM3OPT_OFF_S12 + 104] = np.ascontiguousarray(S12, np.float64).view(np.uint8)
    return blk


def build_loop_corrected_poses():
    import test_gpu_essential_graph as tg
    from sp_orb_slam_amd import extractor as X
    ext = small_handle(100)
    F, cur = 5, 1

    def spec(seed, s):
        rng, Tcw = tg.pose_set(seed, F + 2)
        c, sn = np.cos(0.1 * seed), np.sin(0.1 * seed)
        S12 = np.concatenate([[s], [c, -sn, 0, sn, c, 0, 0, 0, 1], [0.1, -0.2, 0.05 * seed]])
        return dict(d_opt_block=opt_block(ext, S12), d_Tcw2=Tcw[F].reshape(16).copy(),
                    d_Twc=np.linalg.inv(Tcw[F + 1].reshape(4, 4).astype(np.float64)).astype(np.float32).reshape(16),
                    d_Tiw=Tcw[:F].reshape(F, 16).copy(), d_Siw=64 * F, d_Tiw_corrected=64 * F), S12
    (A, S12), (B, _) = spec(4, 1.03), spec(5, 0.9)

    def check(got):
        Siw, Tc = X.SPExtractor.loop_corrected_poses(S12, A["d_Tcw2"], A["d_Twc"], A["d_Tiw"], cur)
        assert got["d_Siw"].tobytes() == Siw.tobytes() and got["d_Tiw_corrected"].tobytes() == Tc.tobytes(), "against the host function"
    return Case(ext, A, B, lambda P, s: ext.loop_corrected_poses_device(P["d_opt_block"], P["d_Tcw2"], P["d_Twc"], P["d_Tiw"], F, cur,
                                                                        P["d_Siw"], P["d_Tiw_corrected"], stream=s),
                ("d_Siw", "d_Tiw_corrected"), check)


# ---- bundle adjustment on the six records of tests/test_gpu_local_ba.py -------------------------------------------------------
def build_local_ba_records():
    import ba_cases
    import test_gpu_local_ba as tb
    from sp_orb_slam_amd import extractor as X
    from tools import track_scene as ts
    S = tb.build_scene(mktemp)
    e = S.ext
    n_kf, n, E = len(S.Tcw), len(S.xyz), len(S.edges)
    RECS = ["d_record_%d" % f for f in range(n_kf)]
    A = dict({RECS[f]: S.raw[f] for f in range(n_kf)}, d_edges=S.edges, d_Tcw=S.Tcw, d_fixed=S.fixed, d_xyz=S.xyz,
             d_stop=np.zeros(1, np.int32), d_out=X.ba_offsets(n_kf, n, E)["bytes"])
    # B: the records in reverse order (slot f holds record 5 - f), other free keyframes, other noise, every 9th edge not served
    rng = np.random.default_rng(6)
    fixed = np.array([1, 0, 0, 0, 0, 1], np.uint8)
    edges = S.edges.copy()
    edges[:, 1] = n_kf - 1 - edges[:, 1]
    edges = edges[np.lexsort((edges[:, 2], edges[:, 1], edges[:, 0]))]
    edges[::9] = -1
    Tcw = []
    for slot in range(n_kf):
        T = ts.pose(*ts.offsets(tb.FRAMES[n_kf - 1 - slot])).astype(np.float64)
        if not fixed[slot]:
            T = ba_cases.pose(rng.normal(0, 0.002, 3), rng.normal(0, 0.01, 3)) @ T
        Tcw.append(T.astype(np.float32).reshape(16))
    B = dict({RECS[f]: S.raw[n_kf - 1 - f] for f in range(n_kf)}, d_edges=edges.astype(np.int32), d_Tcw=np.stack(Tcw), d_fixed=fixed,
             d_xyz=(S.xyz + rng.normal(0, 0.02, S.xyz.shape)).astype(np.float32), d_stop=np.zeros(1, np.int32), d_out=A["d_out"])

    def check(got):
        want = e.bundle_adjust(S.edges, S.obs, S.w, S.Tcw, S.fixed, S.xyz, tb.INTR, stop=0, fill=FILL)
        g = X.SPExtractor.decode_ba_out(got["d_out"], n_kf, n, E)
        assert got["d_out"].tobytes() == want.tobytes() and g["n_served"] == E and g["iterations"][0] > 0, "the block against the host form"

    def counts(spec, got):
        g = X.SPExtractor.decode_ba_out(got["d_out"], n_kf, n, E)
        return (g["n_free"], g["n_served"], g["n_erase"], g["status"]) + tuple(g["iterations"]) + tuple(g["trials"])
    return Case(e, A, B, lambda P, s: e.local_ba_records_device([P[r] for r in RECS], P["d_edges"], E, P["d_Tcw"], P["d_fixed"],
                                                                P["d_xyz"], n, P["d_out"], tb.INTR, d_stop=P["d_stop"], stream=s),
                ("d_out",), check, counts)


# ---- the essential graph, the map correction, the loop detection ----------------------------------------------------------------
def graph_handle():
    from sp_orb_slam_amd import weights
    from sp_orb_slam_amd.extractor import SPExtractor
    return SPExtractor(100, 128, 160, weights.synthetic(7, "dense"), with_heat=False)


def build_essential_graph_sim3():
    import test_gpu_essential_graph as tg
    from sp_orb_slam_amd.extractor import SPExtractor
    ext = graph_handle()
    n, cur, n_conn = 30, 21, 7

    def spec(seed, conn, s):
        rng, Tcw = tg.pose_set(seed, n)
        S12 = np.concatenate([[s], np.eye(3).reshape(-1), [0.1, -0.2, 0.05 * seed]])
        Twc = np.linalg.inv(Tcw[cur].reshape(4, 4).astype(np.float64)).astype(np.float32)
        return dict(d_Tcw=Tcw, d_opt_block=opt_block(ext, S12), d_Tcw2=Tcw[seed].copy(), d_Twc=Twc, d_conn_slot=np.array(conn, np.int32),
                    d_Scw_est=64 * n, d_Scw_meas=64 * n), S12
    (A, S12), (B, _) = spec(4, [21, -1, 19, 25, 3, 40, 11], 1.03), spec(5, [2, 21, 8, -7, 29, 14, 1], 0.95)

    def check(got):
        est, meas = SPExtractor.essential_graph_sim3(A["d_Tcw"], S12, A["d_Tcw2"], A["d_Twc"], A["d_conn_slot"], cur)
        assert got["d_Scw_est"].tobytes() == est.tobytes() and got["d_Scw_meas"].tobytes() == meas.tobytes(), "against the host function"
    return Case(ext, A, B, lambda P, s: ext.essential_graph_sim3_device(P["d_Tcw"], P["d_opt_block"], P["d_Tcw2"], P["d_Twc"],
                                                                        P["d_conn_slot"], n_conn, cur, P["d_Scw_est"], P["d_Scw_meas"], n,
                                                                        stream=s), ("d_Scw_est", "d_Scw_meas"), check)


def build_optimize_essential_graph():
    import eg_cases
    import eg_ref
    from sp_orb_slam_amd import extractor as X
    from sp_orb_slam_amd.extractor import SPExtractor
    ext = graph_handle()
    a = eg_ref.arrays(eg_cases.banded(70, wide_row=True))
    b = eg_ref.arrays(eg_cases.banded(70, seed=1, wide_row=True))
    n, E = len(a["est"]), len(a["edges"])
    assert len(b["est"]) == n and len(b["edges"]) == E
    b["flags"] = b["flags"].copy()
    b["flags"][[0, 9]] = (0, 1)                          # B: another fixed keyframe (n_unknown is read on the device) ...
    b["edges"] = b["edges"][::-1].copy()                 # ... the edges in another order, three of them never followed
    cap = max(SPExtractor.essential_graph_envelope(x["flags"], x["edges"])[0] for x in (a, b))
    b["edges"][[5, 40, E - 1], 0] = (-1, n, n + 3)
    A, B = (dict(d_Scw_est=x["est"], d_Scw_meas=x["meas"], d_flags=x["flags"], d_edges=x["edges"], d_out=X.essgraph_offsets(n)["out_bytes"])
            for x in (a, b))

    def check(got):
        want = ext.optimize_essential_graph(a["est"], a["meas"], a["flags"], a["edges"], cap, iterations=3, fill=FILL)
        g = SPExtractor.decode_essgraph_out(got["d_out"], n)
        assert got["d_out"].tobytes() == want.tobytes() and g["iterations"] == 3 and g["status"] == X.ESSGRAPH_OK, "against the host form"

    def counts(spec, got):
        g = SPExtractor.decode_essgraph_out(got["d_out"], n)
        return (g["n_unknown"], g["n_edges_followed"], g["n_skipped"], g["env_blocks"], g["trials"])
    return Case(ext, A, B, lambda P, s: ext.optimize_essential_graph_device(P["d_Scw_est"], P["d_Scw_meas"], P["d_flags"], n, P["d_edges"],
                                                                            E, cap, P["d_out"], iterations=3, stream=s),
                ("d_out",), check, counts)


def build_correct_map_points():
    import test_gpu_essential_graph as tg
    ext = graph_handle()
    cases = [tg.correction_case(seed=sd, n_kf=6, n_table=900) for sd in (8, 9)]
    m = len(cases[0][3])
    assert len(cases[1][3]) == m
    A, B = (dict(d_S_from=Sf, d_S_to=St, d_ref_slot=rs, d_point_idx=idx, d_xyz=xyz, d_tflags=fl, d_code=m)
            for Sf, St, rs, idx, xyz, fl in cases)

    def check(got):
        Sf, St, rs, idx, xyz, fl = cases[0]
        w_xyz = xyz.copy()
        w_code = ext.correct_map_points(Sf, St, rs, idx, w_xyz, fl)
        assert got["d_xyz"].tobytes() == w_xyz.tobytes() and np.array_equal(got["d_code"], w_code), "against the host form"
    return Case(ext, A, B, lambda P, s: ext.correct_map_points_device(P["d_S_from"], P["d_S_to"], 6, P["d_ref_slot"], P["d_point_idx"], m,
                                                                      P["d_xyz"], P["d_tflags"], 900, P["d_code"], stream=s),
                ("d_xyz", "d_code"), check, lambda spec, got: tuple(np.bincount(got["d_code"], minlength=4).tolist()))


def build_detect_loop_candidates():
    import loopdet_cases as lc
    import loopdet_ref
    from sp_orb_slam_amd import extractor as X
    ext = small_handle(100)
    n, dim, cur = 300, 64, 150
    cs = [lc.generated(sd, n, dim, p_pass=p, cur=cur).arrays() for sd, p in ((41, 0.5), (42, 0.3))]
    n_conn, n_cov = (min(len(c[k]) for c in cs) for k in ("connected", "covisible"))
    cs = [dict(c, connected=c["connected"][:n_conn], covisible=c["covisible"][:n_cov]) for c in cs]
    cs[1]["in_db"] = np.where(np.arange(n) % 7 == 0, 0, cs[1]["in_db"]).astype(np.uint8)
    arrs = [loopdet_ref.arrays(c) for c in cs]
    A, B = (dict(d_gdesc=a["gdesc"], d_kf_flags=a["kf_flags"], d_in_db=a["in_db"], d_best_cov=a["best_cov"], d_connected=a["connected"],
                 d_covisible=a["covisible"], d_out=X.loopdet_offsets(n)["out_bytes"]) for a in arrs)
    prm = [float(cs[0][k]) for k in ("min_score_init", "min_score_floor", "retain_ratio")]

    def check(got):
        a = arrs[0]
        want = ext.detect_loop_candidates(a["gdesc"], a["kf_flags"], a["in_db"], a["best_cov"], cur, a["connected"], a["covisible"], *prm,
                                          fill=FILL)
        g = ext.decode_loopdet_out(got["d_out"], n)
        assert got["d_out"].tobytes() == want.tobytes() and g["n_pass"] > 50 and g["n_cand"] >= 1, "the block against the host form"

    def counts(spec, got):
        g = ext.decode_loopdet_out(got["d_out"], n)
        return (g["n_scored"], g["n_pass"], g["n_cand"])
    return Case(ext, A, B, lambda P, s: ext.detect_loop_candidates_device(P["d_gdesc"], dim, P["d_kf_flags"], P["d_in_db"], P["d_best_cov"],
                                                                          n, cur, P["d_connected"], n_conn, P["d_covisible"], n_cov,
                                                                          P["d_out"], *prm, stream=s), ("d_out",), check, counts)


# ---- the table: one entry per *_device function of include/spfe.h other than spfe_extract_batch_device ----------------------
# stated False: the header promises launches without a number, and the count is the one measured on an MI355X (for the two
# loops over host pointer arrays with the case's two neighbours / two candidates)
FORMS = {
    # staging and patches
    "stage_batch": Form(build_stage_batch, 1, "with one gather kernel that writes the gray H x W frame conv1a reads"),
    "match_records": Form(build_match_records, 5, "reading K from the record headers on the device; no host synchronisation", False),
    "match_patches_record": Form(build_match_patches_record, 2, "enqueued on `stream`, no host synchronisation", False),
    # dust and pose
    "align_dust_record": Form(build_align_dust_record, 1, "Enqueued on `stream` (NULL = the handle's), no host synchronisation", False),
    "align_dust_batch": Form(build_align_dust_batch, 1, "n_frames independent solves in ONE launch, one workgroup each"),
    "refine_pose_record": Form(build_refine_pose_record, 1, "Enqueued on `stream` (NULL = the handle's), no host synchronisation", False),
    "refine_pose_batch": Form(build_refine_pose_batch, 1, "n_frames solves in ONE launch, one workgroup each"),
    # projection search and tracking
    "search_projection_record": Form(build_search_projection_record, 3, "Three launches back to back on `stream` (NULL = the handle's), no host synchronisation"),
    "search_projection_batch": Form(build_search_projection_batch, 3, "n_frames searches in the same three launches"),
    "track_dust_record": Form(build_track_dust_record, 3, "Three launches behind each other on `stream`"),
    "track_dust_refine_record": Form(build_track_dust_refine_record, 6, "All kernels back to back on `stream`, no host synchronisation", False),
    "track_local_map_record": Form(build_track_local_map_record, 5, "All launches back to back on `stream`, no host synchronisation", False),
    "track_motion_model_record": Form(build_track_motion_model_record, 7, "every launch back to back on `stream` (NULL = the handle's), no host synchronisation, no host decision", False),
    "track_reference_kf_record": Form(build_track_reference_kf_record, 8, "every launch back to back on `stream` (NULL = the handle's), no host synchronisation, no host decision", False),
    # map-point creation and fusion
    "create_map_points_pair_record": Form(build_create_map_points_pair_record, 7, "all launches back to back on `stream` (NULL = the handle's), no host synchronisation", False),
    "create_map_points_record": Form(build_create_map_points_record, 14, "The loop over the neighbours (local_mapper.cpp:592-800) as one call", False),
    "fuse_record": Form(lambda: fuse_case(False, 1), 2, "One target record: two launches on `stream` (NULL = the handle's), no host synchronisation"),
    "fuse_targets_record": Form(lambda: fuse_case(False, 2), 2, "the same two launches whatever n_targets is"),
    # loop verification and Sim3
    "sim3_ransac": Form(build_sim3_ransac, 3, "Three launches (pairs, hypotheses, select) on `stream`"),
    "loop_match_record": Form(build_loop_match_record, 6, "All launches on `stream` (NULL = the handle's), no host synchronisation", False),
    "loop_verify_records": Form(build_loop_verify_records, 15, "Match, pairs, hypotheses and select run back to back on `stream` without host synchronisation or copies", False),
    "search_by_sim3_record": Form(build_search_by_sim3_record, 3, "three launches (prepare, search, agree) on `stream` (NULL = the handle's), no host synchronisation"),
    "loop_guided_match_records": Form(build_loop_guided_match_records, 3, "the same three launches whatever n_jobs is"),
    "optimize_sim3_record": Form(build_optimize_sim3_record, 1, "one launch on `stream` (NULL = the handle's), no host synchronisation"),
    "loop_optimize_sim3_records": Form(build_loop_optimize_sim3_records, 1, "The solves of n_jobs hypotheses as ONE launch behind spfe_loop_guided_match_records_device"),
    # loop correction
    "search_loop_points_record": Form(build_search_loop_points_record, 2, "two launches (candidates, claim) on `stream`, no host synchronisation"),
    "loop_corrected_poses": Form(build_loop_corrected_poses, 1, "The device form is one launch on `stream`, no host synchronisation"),
    "loop_fuse_record": Form(lambda: fuse_case(True, 1), 2, "One target record: two launches on `stream` (NULL = the handle's), no host synchronisation"),
    "loop_fuse_targets_record": Form(lambda: fuse_case(True, 2), 2, "the same two launches whatever n_targets is"),
    # bundle adjustment and map maintenance
    "local_ba_records": Form(build_local_ba_records, 1, "One launch on `stream` (NULL = the handle's), no host synchronisation"),
    "refresh_map_points": Form(build_refresh_map_points, 2, "two launches on `stream` (NULL = the handle's) whatever m is, no host synchronisation, no allocation"),
    "gather_map_points": Form(build_gather_map_points, 1, "One launch on `stream`, no host synchronisation"),
    # essential graph and loop detection
    "essential_graph_sim3": Form(build_essential_graph_sim3, 2, "The graph's start values from the poses, two launches on `stream`"),
    "optimize_essential_graph": Form(build_optimize_essential_graph, 4, "The optimisation: launches on `stream` (NULL = the handle's), no host synchronisation", False),
    "correct_map_points": Form(build_correct_map_points, 1, "The map-point correction, one launch, one thread per listed point"),
    "detect_loop_candidates": Form(build_detect_loop_candidates, 3, "three launches on `stream` (NULL = the handle's) whatever n_slots is"),
}


# ---- the sequence ---------------------------------------------------------------------------------------------------------------
def run(name):
    """-> (list of failures, dict(kernel, memset, ...) or None)"""
    import torch
    import hip_graph
    form = FORMS[name]
    case = form.build()
    stream = torch.cuda.Stream()
    held = Buffers(case)
    P, load, read = held.P, held.load, held.read

    failures, want = [], {}
    for key in ("A", "B"):                                # the direct calls (the first sizes the scratch)
        load(key)
        case.call(P, stream.cuda_stream)
        want[key] = read()
        if key == "A" and case.check is not None:
            try:
                case.check(want["A"])
            except AssertionError as e:
                failures.append("direct call on A against its reference: %s" % (str(e).splitlines()[0][:300] if str(e) else "assertion"))
    same = [k for k in case.outputs if np.array_equal(want["A"][k], want["B"][k])]
    if same:
        failures.append("A and B give the same %s: the replay on B would prove nothing" % same)
    if case.counts is not None:
        ca, cb = case.counts(case.A, want["A"]), case.counts(case.B, want["B"])
        print("device-side counts  A %s  B %s" % (ca, cb))
        if ca == cb:
            failures.append("no device-side count differs between A and B: %s" % (ca,))
    load("A")
    cap = hip_graph.capture(stream, lambda: case.call(P, stream.cuda_stream))
    if not cap.ok:
        failures.append("capture refused or invalidated: %s" % cap.why())
        cap.destroy()
        torch.cuda.synchronize()
        return failures, None
    shape = cap.shape()
    print("graph", shape)
    if shape["other"]:
        failures.append("nodes other than kernels and memsets: %s" % shape["other"])
    if shape["roots"] != 1 or shape["edges"] != shape["nodes"] - 1:
        failures.append("not one chain: %d nodes, %d edges, %d roots" % (shape["nodes"], shape["edges"], shape["roots"]))
    if form.kernels is None:
        failures.append("the table has no kernel count for this form: measured kernel=%d memset=%d" % (shape["kernel"], shape["memset"]))
    elif shape["kernel"] != form.kernels or shape["memset"] != form.memsets:
        failures.append("%d kernel and %d memset nodes, the table says %d and %d (%s: %r)" % (
            shape["kernel"], shape["memset"], form.kernels, form.memsets, "include/spfe.h" if form.stated else "measured", form.sentence))
    status = cap.instantiate()
    if status != 0:
        failures.append("hipGraphInstantiate: %s" % hip_graph.error_name(status))
    else:
        for step, key in enumerate(("A", "B", "A")):      # no library call from here to the last replay
            load(key)
            status = cap.launch(stream.cuda_stream)
            got = read()
            if status != 0:
                failures.append("replay %d (%s): hipGraphLaunch: %s" % (step + 1, key, hip_graph.error_name(status)))
                break
            for k in case.outputs:
                d = np.flatnonzero(got[k] != want[key][k])
                if len(d):
                    other = "B" if key == "A" else "A"
                    what = (" — the bytes of the direct call on %s: frozen at capture" % other if np.array_equal(got[k], want[other][k])
                            else " — still the 0xA5 prefill: nothing was written" if (got[k][d] == FILL).all() else "")
                    at = int(d[0]) // 4 * 4
                    failures.append("replay %d on %s: %r differs from the direct call in %d byte(s), the first at %d (got %s, direct %s)%s" % (
                        step + 1, key, k, len(d), d[0], got[k][at:at + 8].tobytes().hex(), want[key][k][at:at + 8].tobytes().hex(), what))
    torch.cuda.synchronize()
    cap.destroy()
    # the handle is usable behind the graph: the direct call gives its bytes again
    load("B")
    case.call(P, stream.cuda_stream)
    again = read()
    for k in case.outputs:
        if not np.array_equal(again[k], want["B"][k]):
            failures.append("a direct call behind the graph: %r differs" % k)
    case.ext.close()
    return failures, shape


def main(name):
    if name not in FORMS:
        print("graph-form %s: FAIL: no such form" % name)
        return 1
    try:
        failures, shape = run(name)
    except Exception as e:      # a set-up error is a failure of the case, with its text in the verdict
        import traceback
        traceback.print_exc()
        failures, shape = ["%s: %s" % (type(e).__name__, str(e).splitlines()[0][:300] if str(e) else "")], None
    counts = "" if shape is None else " kernel=%d memset=%d" % (shape["kernel"], shape["memset"])
    if failures:
        print("graph-form %s: FAIL:%s %s" % (name, counts, " | ".join(failures)), flush=True)
        return 1
    print("graph-form %s: PASS%s" % (name, counts), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
