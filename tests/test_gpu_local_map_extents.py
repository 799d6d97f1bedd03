"""GPU: the resident forms of the local map held to the buffer extents include/spfe.h documents, as
tests/test_gpu_loop_detect_extents.py holds the loop detection's: each form is called (a) with separate torch tensors and (b), (c)
with EVERY pointer argument inside one arena (tests/extent_arena.py) at exactly its documented size, the bytes between the buffers
filled with 0xFF, then with 0x80.  No byte outside a buffer may change, and the outputs must be byte-identical across the three
calls and equal to tests/localmap_ref/localmap_ref.c.  Rows of 101 entries are 404 bytes: only every fourth starts on a 16-byte
boundary, and the last row ends where the arena's poison begins — a kernel that read its last 16-byte load in full, or a full wave
of tail entries, would carry the poison into the last slot's votes.  Rows of 1, 4 and 5 entries are shorter than one load."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("localmap_ref", ""):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
import extent_arena as ea  # noqa: E402
import localmap_cases as lc  # noqa: E402
import localmap_ref  # noqa: E402

from sp_orb_slam_amd import extractor as X  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import SPExtractor  # noqa: E402

pytestmark = pytest.mark.gpu

# argument -> bytes, by the comments above the declarations in include/spfe.h
EXTENTS = dict(d_kf_mp_of_kp=lambda d: 4 * d["stride"] * d["n"], d_kf_flags=lambda d: d["n"], d_best_cov=lambda d: 4 * d["n_best"] * d["n"],
               d_parent=lambda d: 4 * d["n"], d_mp_flags=lambda d: d["n_table"], d_mp_of_kp=lambda d: 4 * d["n_kp"],
               d_out=lambda d: X.localmap_offsets(d["n"], d["cap"], d["n_kp"])["out_bytes"], d_outlier=lambda d: d["n_kp"],
               d_votes=lambda d: 4 * d["n"], d_total=lambda d: 4 * d["n"], d_point_idx=lambda d: 4 * d["cap"],
               d_mp_of_kp_list=lambda d: 4 * d["n_kp"], d_mp_of_kp_rows=lambda d: 4 * d["n_kp"])


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return localmap_ref.build(tmp_path_factory.mktemp("localmap_ref"))


@pytest.fixture(scope="module")
def ext():
    e = SPExtractor(100, 64, 96, weights.synthetic(7, "trackable"), with_heat=False)
    yield e
    e.close()


def three_calls(spec, dims, call, outputs, want):
    """spec: name -> array (an input) or int (an output of that many bytes); call(P); want: name -> the reference's bytes"""
    import torch
    assert set(spec) <= set(EXTENTS)
    # (a) separate tensors
    tens = {k: (torch.full((int(v),), 0xA5, dtype=torch.uint8, device="cuda") if isinstance(v, (int, np.integer)) else
                torch.from_numpy(np.ascontiguousarray(v).reshape(-1).view(np.uint8).copy()).cuda()) for k, v in spec.items()}
    call({k: t.data_ptr() for k, t in tens.items()})
    torch.cuda.synchronize()
    plain = {k: tens[k].cpu().numpy() for k in outputs}
    for k in outputs:
        assert plain[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), k
    # (b), (c) the arena
    arena = ea.Arena("cuda")
    for name, v in spec.items():
        arena.place(name, v, init=0xA5)
        assert arena.size(name) == EXTENTS[name](dims), (name, arena.size(name), EXTENTS[name](dims))

    def run(ar):
        call({k: ar.ptr(k) for k in spec})
        torch.cuda.synchronize()
    found, _ = ea.report(arena, run, outputs, plain)
    assert found == [], found


def update_case(ext, ref, c):
    a = localmap_ref.arrays(c)
    n, stride = a["kf_mp_of_kp"].shape
    n_kp, n_table, n_best, cap = len(a["mp_of_kp"]), len(a["mp_flags"]), a["best_cov"].shape[1], int(c["point_cap"])
    dims = dict(n=n, stride=stride, n_best=n_best, n_table=n_table, n_kp=n_kp, cap=cap)
    want = localmap_ref.update(ref, c)
    spec = dict(d_kf_mp_of_kp=a["kf_mp_of_kp"], d_kf_flags=a["kf_flags"], d_best_cov=a["best_cov"], d_parent=a["parent"],
                d_mp_flags=a["mp_flags"], d_out=X.localmap_offsets(n, cap, n_kp)["out_bytes"])
    if n_kp:
        spec["d_mp_of_kp"] = a["mp_of_kp"]

    def call(P):
        ext.update_local_map_resident(P["d_kf_mp_of_kp"], stride, P["d_kf_flags"], P["d_best_cov"], n_best, P["d_parent"], n,
                                      P["d_mp_flags"], n_table, P.get("d_mp_of_kp"), n_kp, P["d_out"], cap, int(c["max_keyframes"]))
    three_calls(spec, dims, call, ("d_out",), {"d_out": want["block"]})
    return want, a, dims


@pytest.mark.parametrize("stride", [1, 4, 5, 101, 1001])
def test_update_local_map_resident(ext, ref, stride):
    c = lc.generated(400 + stride, 65, stride, 3000, 300, point_cap=2048, vote_all=True)
    mp = c["mp_of_kp"]
    held = mp[(mp >= 0) & (mp < 3000)]
    c["kf_mp_of_kp"][64, :] = held[(c["mp_flags"][held] & 1) != 0][0]    # the last row is full to its last entry, and voted
    c["kf_flags"][64] = 0
    want, _, _ = update_case(ext, ref, c)
    assert want["votes"][64] >= stride and want["total"][64] == stride and want["n_voted"] >= 2


def test_update_local_map_resident_without_keypoints(ext, ref):
    want, _, _ = update_case(ext, ref, lc.generated(450, 9, 6, 50, 0, point_cap=7))
    assert want["status"] == X.LOCALMAP_NO_VOTES


@pytest.mark.parametrize("masked", [False, True])
def test_count_shared_points_resident(ext, ref, masked):
    c = lc.generated(460, 65, 101, 3000, 300, vote_all=True)
    a = localmap_ref.arrays(c)
    n, stride = a["kf_mp_of_kp"].shape
    mask = (np.arange(300) % 3 == 0).astype(np.uint8) if masked else None
    votes, total = localmap_ref.count(ref, c, mask)
    dims = dict(n=n, stride=stride, n_table=3000, n_kp=300)
    spec = dict(d_kf_mp_of_kp=a["kf_mp_of_kp"], d_mp_flags=a["mp_flags"], d_mp_of_kp=a["mp_of_kp"], d_votes=4 * n, d_total=4 * n)
    if masked:
        spec["d_outlier"] = mask

    def call(P):
        ext.count_shared_points_resident(P["d_kf_mp_of_kp"], stride, n, P["d_mp_flags"], 3000, P["d_mp_of_kp"], P.get("d_outlier"), 300,
                                         P["d_votes"], P["d_total"])
    three_calls(spec, dims, call, ("d_votes", "d_total"), {"d_votes": votes, "d_total": total})
    assert votes.max() >= 3


def test_local_map_rows_resident(ext, ref):
    c = lc.generated(470, 65, 101, 3000, 300, point_cap=700, vote_all=True)
    r = localmap_ref.update(ref, c)
    lst = r["mp_of_kp_list"].copy()
    lst[np.flatnonzero(lst < 0)[:3]] = [699, 700, -9]
    rows = np.where((lst >= 0) & (lst < 700), r["point_idx"][np.clip(lst, 0, 699)], -1).astype(np.int32)
    spec = dict(d_point_idx=r["point_idx"], d_mp_of_kp_list=lst, d_mp_of_kp_rows=4 * 300)
    three_calls(spec, dict(cap=700, n_kp=300), lambda P: ext.local_map_rows_resident(P["d_point_idx"], 700, P["d_mp_of_kp_list"], 300,
                                                                                      P["d_mp_of_kp_rows"]),
                ("d_mp_of_kp_rows",), {"d_mp_of_kp_rows": rows})
    assert (rows >= 0).sum() > 100
