"""GPU: the device forms of the map-point table held to the buffer extents include/spfe.h documents, as
tests/test_gpu_loop_fuse_extents.py holds the loop closer's: every entry point is called (a) with separate torch tensors and
(b), (c) with EVERY pointer argument — the records and the device array of record pointers included — inside one arena
(tests/extent_arena.py) at exactly its documented size, the bytes between the buffers filled with 0xFF, then with 0x80.  No byte
outside a buffer may change, and every output must be byte-identical across the three calls; a second pass overwrites the rows of
the records at and beyond K with the poison.  The scene and the records are test_gpu_extents.py's; the table is its fuse point
list.  The forms: spfe_refresh_map_points_device (with and without d_point_idx), spfe_gather_map_points_device, and the chain of
the two with the table rows read where they were written."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import extent_arena as ea  # noqa: E402
import test_gpu_extents as tge  # noqa: E402
from test_gpu_extents import S  # noqa: E402,F401  (the module's scene fixture)

from sp_orb_slam_amd import extractor as X  # noqa: E402
from tools import track_scene as ts  # noqa: E402

pytestmark = pytest.mark.gpu
FRAMES = tge.FRAMES
F = len(FRAMES)
RECS = ["d_record_%d" % f for f in range(F)]

# argument -> bytes, by the comments above the declarations of the section "the map-point table" of include/spfe.h.
# d: F = n_kf, m, E, n = n_table, g = the gather's n, rb = spfe_record_bytes
TABLE = dict(d_xyz=lambda d: 12 * d["n"], d_flags=lambda d: d["n"], d_normal=lambda d: 12 * d["n"], d_dist_range=lambda d: 8 * d["n"],
             d_desc=lambda d: 1024 * d["n"])
KEYFRAMES = dict({r: tge.REC for r in RECS}, d_kf_records=lambda d: 8 * d["F"], d_kf_flags=lambda d: d["F"], d_Tcw=lambda d: 64 * d["F"])
LISTED = dict(d_obs_start=lambda d: 4 * (d["m"] + 1), d_obs=lambda d: 8 * d["E"], d_ref_slot=lambda d: 4 * d["m"],
              d_out=lambda d: X.mp_offsets(d["m"])["out_bytes"])
LIST = dict(d_idx=lambda d: 4 * d["g"], d_point_id=lambda d: 4 * d["g"], d_list_xyz=lambda d: 12 * d["g"], d_list_normal=lambda d: 12 * d["g"],
            d_list_dist_range=lambda d: 8 * d["g"], d_list_desc=lambda d: 1024 * d["g"], d_list_flags=lambda d: d["g"])
EXTENTS = {
    "refresh_map_points_device": dict(KEYFRAMES, **LISTED, **TABLE, d_point_idx=lambda d: 4 * d["m"]),
    "refresh_map_points_device, rows in order": dict(KEYFRAMES, **LISTED, **TABLE),
    "gather_map_points_device": dict(LIST, **TABLE),
    "refresh_then_gather": dict(KEYFRAMES, **LISTED, **TABLE, **LIST, d_point_idx=lambda d: 4 * d["m"]),
}
LIST_OUT = ("d_point_id", "d_list_xyz", "d_list_normal", "d_list_dist_range", "d_list_desc", "d_list_flags")
TABLE_OUT = ("d_normal", "d_dist_range", "d_desc")


def three_calls(entry, spec, call, outputs, dims):
    """spec: name -> ndarray (an input), int (an output of that many bytes, 0xA5 on entry) or a function of the poison pattern
    (None: plain); d_kf_records is filled with the addresses of the records wherever they lie.  -> dict name -> uint8 array"""
    import torch

    def plain(v):
        return v(None) if callable(v) else v

    def pointers(addr):
        return np.array([addr(r) for r in RECS], np.int64)
    has_kf = "d_kf_records" in spec
    tens = {}
    for name, v in spec.items():
        v = plain(v)
        tens[name] = (torch.full((int(v),), 0xA5, dtype=torch.uint8, device="cuda") if isinstance(v, (int, np.integer)) else
                      torch.from_numpy(np.ascontiguousarray(v).reshape(-1).view(np.uint8).copy()).cuda())
    if has_kf:
        tens["d_kf_records"] = torch.from_numpy(pointers(lambda r: tens[r].data_ptr()).view(np.uint8)).cuda()
    call({k: t.data_ptr() for k, t in tens.items()})
    torch.cuda.synchronize()
    want = {k: tens[k].cpu().numpy() for k in outputs}
    arena = ea.Arena("cuda")
    for name, v in spec.items():
        arena.place(name, plain(v), init=0xA5)
        assert arena.size(name) == EXTENTS[entry][name](dims), (entry, name, arena.size(name), EXTENTS[entry][name](dims))
    assert set(spec) == set(EXTENTS[entry]), entry
    if has_kf:
        arena.set_initial("d_kf_records", pointers(arena.ptr))

    def run(a):
        call({k: a.ptr(k) for k in spec})
        torch.cuda.synchronize()
    found, got = ea.report(arena, run, outputs, want)
    assert found == [], (entry, found)

    def tails(a, p):                                  # the second pass: poison in the rows nobody may depend on
        for name, v in spec.items():
            if callable(v):
                a.set_initial(name, v(p))
    found, _ = ea.report(arena, run, outputs, want, before_fill=tails)
    assert found == [], (entry, "rows beyond K", found)
    return got


def problem(S, seed, with_idx):  # noqa: F811
    """a refresh of m points of the fuse point list from the scene's three records: observation counts on either side of the
    wavefront / workgroup boundary and of the staging capacity, every keypoint below its record's K"""
    rng = np.random.default_rng(seed)
    pts = tge.fuse_points(S)
    n = S.n_lm
    counts = [1, 2, 3, 5, 16, 17, 41, 0, 4, 7, 2, 64, 3, 6, 9, 2, 33, 5]
    m = len(counts)
    obs = np.array([(f, int(rng.integers(S.recs[f].K))) for c in counts for f in rng.integers(0, F, c)], np.int32).reshape(-1, 2)
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    spec = dict({RECS[f]: tge.record(S, f) for f in range(F)}, d_kf_records=8 * F, d_kf_flags=np.array([0, 1, 0], np.uint8),
                d_Tcw=np.stack([ts.pose(*ts.offsets(k)).astype(np.float32).reshape(16) for k in FRAMES]), d_obs_start=start, d_obs=obs,
                d_ref_slot=rng.integers(0, F, m).astype(np.int32), d_xyz=pts["d_xyz"], d_flags=pts["d_flags"], d_normal=12 * n,
                d_dist_range=8 * n, d_desc=1024 * n, d_out=X.mp_offsets(m)["out_bytes"])
    if with_idx:
        spec["d_point_idx"] = rng.permutation(n)[:m].astype(np.int32)
    return spec, dict(F=F, m=m, E=len(obs), n=n, rb=S.rb)


def refresh(e, P, d, with_idx):
    e.refresh_map_points_device(P["d_kf_records"], P["d_kf_flags"], P["d_Tcw"], d["F"], P["d_point_idx"] if with_idx else None,
                                P["d_obs_start"], P["d_obs"], P["d_ref_slot"], d["m"], d["E"], P["d_xyz"], P["d_flags"], P["d_normal"],
                                P["d_dist_range"], P["d_desc"], d["n"], P["d_out"])


def gather(e, P, d):
    e.gather_map_points_device(P["d_idx"], d["g"], P["d_xyz"], P["d_flags"], P["d_normal"], P["d_dist_range"], P["d_desc"], d["n"],
                               *[P[k] for k in LIST_OUT])


@pytest.mark.parametrize("with_idx", [True, False], ids=["point_idx", "rows in order"])
def test_refresh_map_points_device(S, with_idx):  # noqa: F811
    spec, d = problem(S, 3, with_idx)
    entry = "refresh_map_points_device" + ("" if with_idx else ", rows in order")
    got = three_calls(entry, spec, lambda P: refresh(S.ext, P, d, with_idx), TABLE_OUT + ("d_out",), d)
    g = X.SPExtractor.decode_mp_out(got["d_out"], d["m"])
    assert g["m"] == d["m"] and g["n_desc_written"] >= 10 and (g["code"] <= X.MP_NO_OBS).any() and g["n_good"].max() > X.MP_WAVE_OBS
    rows = spec["d_point_idx"] if with_idx else np.arange(d["m"])
    unlisted = np.setdiff1d(np.arange(d["n"]), rows)
    assert (got["d_desc"].reshape(d["n"], 1024)[unlisted] == 0xA5).all() and (got["d_normal"].reshape(d["n"], 12)[unlisted] == 0xA5).all()


def list_spec(S, g, seed):  # noqa: F811
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, S.n_lm, g).astype(np.int32)
    idx[[3, 11]] = (-1, S.n_lm)                       # not followed
    return dict(d_idx=idx, d_point_id=4 * g, d_list_xyz=12 * g, d_list_normal=12 * g, d_list_dist_range=8 * g, d_list_desc=1024 * g,
                d_list_flags=g)


def test_gather_map_points_device(S):  # noqa: F811
    pts = tge.fuse_points(S)
    g, n = 37, S.n_lm
    spec = dict(list_spec(S, g, 4), **{k: pts[k] for k in TABLE})
    d = dict(g=g, n=n)
    got = three_calls("gather_map_points_device", spec, lambda P: gather(S.ext, P, d), LIST_OUT, d)
    assert np.array_equal(got["d_point_id"].view(np.int32), spec["d_idx"])
    ok = (spec["d_idx"] >= 0) & (spec["d_idx"] < n)
    assert np.array_equal(got["d_list_flags"], np.where(ok, pts["d_flags"][np.clip(spec["d_idx"], 0, n - 1)], 0))
    assert got["d_list_desc"].tobytes() == np.where(ok[:, None], pts["d_desc"][np.clip(spec["d_idx"], 0, n - 1)], np.float32(0)).tobytes()


def test_refresh_then_gather(S):  # noqa: F811
    spec, d = problem(S, 5, True)
    g = 29
    spec.update(list_spec(S, g, 6))
    spec["d_idx"][:d["m"]] = spec["d_point_idx"]      # the refreshed rows first
    d["g"] = g

    def call(P):
        refresh(S.ext, P, d, True)
        gather(S.ext, P, d)
    got = three_calls("refresh_then_gather", spec, call, TABLE_OUT + ("d_out",) + LIST_OUT, d)
    code = X.SPExtractor.decode_mp_out(got["d_out"], d["m"])["code"]
    rows = spec["d_point_idx"][code == X.MP_REFRESHED]
    assert len(rows) >= 10
    lst = got["d_list_desc"].reshape(g, 1024)[:d["m"]][code == X.MP_REFRESHED]
    assert lst.tobytes() == got["d_desc"].reshape(d["n"], 1024)[rows].tobytes() and not (lst == 0xA5).all()
