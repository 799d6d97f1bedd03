"""GPU: the device form of the loop detection held to the buffer extents include/spfe.h documents, as
tests/test_gpu_map_points_extents.py holds the map-point table's: spfe_detect_loop_candidates_device is called (a) with separate
torch tensors and (b), (c) with EVERY pointer argument inside one arena (tests/extent_arena.py) at exactly its documented size, the
bytes between the buffers filled with 0xFF, then with 0x80.  No byte outside a buffer may change, and the block must be
byte-identical across the three calls; a second pass overwrites what the call has no business reading — the rows of d_gdesc of the
slots without a role, the rows of d_best_cov of the slots that do not pass — with the poison.  The forms: with both lists, with
null lists, and with rows of 1028 floats, whose last pass is one float4 (a thread that read its full share would leave the row,
and at the last slot the table)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("loopdet_ref", ""):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
import extent_arena as ea  # noqa: E402
import loopdet_cases as lc  # noqa: E402
import loopdet_ref  # noqa: E402

from sp_orb_slam_amd import extractor as X  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import SPExtractor  # noqa: E402

pytestmark = pytest.mark.gpu

# argument -> bytes, by the comment above the declaration of spfe_detect_loop_candidates_device in include/spfe.h
EXTENTS = dict(d_gdesc=lambda d: 4 * d["dim"] * d["n"], d_kf_flags=lambda d: d["n"], d_in_db=lambda d: d["n"],
               d_best_cov=lambda d: 40 * d["n"], d_connected=lambda d: 4 * d["n_conn"], d_covisible=lambda d: 4 * d["n_cov"],
               d_out=lambda d: X.loopdet_offsets(d["n"])["out_bytes"])


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return loopdet_ref.build(tmp_path_factory.mktemp("loopdet_ref"))


@pytest.fixture(scope="module")
def ext():
    e = SPExtractor(100, 64, 96, weights.synthetic(7, "trackable"), with_heat=False)
    yield e
    e.close()


def three_calls(ext, ref, c, lists=True):
    import torch
    a = loopdet_ref.arrays(c)
    if not lists:
        c = dict(c, connected=np.zeros(0, np.int32), covisible=np.zeros(0, np.int32))
        a = loopdet_ref.arrays(c)
    want = loopdet_ref.detect(ref, c)
    n, dim = a["gdesc"].shape
    dims = dict(n=n, dim=dim, n_conn=len(a["connected"]), n_cov=len(a["covisible"]))
    spec = dict(d_gdesc=a["gdesc"], d_kf_flags=a["kf_flags"], d_in_db=a["in_db"], d_best_cov=a["best_cov"],
                d_out=X.loopdet_offsets(n)["out_bytes"])
    if lists:
        spec.update(d_connected=a["connected"], d_covisible=a["covisible"])
    prm = [float(c[k]) for k in ("min_score_init", "min_score_floor", "retain_ratio")]

    def call(P):
        ext.detect_loop_candidates_device(P["d_gdesc"], dim, P["d_kf_flags"], P["d_in_db"], P["d_best_cov"], n, int(c["cur_slot"]),
                                          P.get("d_connected"), dims["n_conn"], P.get("d_covisible"), dims["n_cov"], P["d_out"], *prm)
        torch.cuda.synchronize()
    # (a) separate tensors
    tens = {k: (torch.full((int(v),), 0xA5, dtype=torch.uint8, device="cuda") if isinstance(v, (int, np.integer)) else
                torch.from_numpy(np.ascontiguousarray(v).reshape(-1).view(np.uint8).copy()).cuda()) for k, v in spec.items()}
    call({k: t.data_ptr() for k, t in tens.items()})
    plain = tens["d_out"].cpu().numpy()
    assert plain.tobytes() == want["block"].tobytes()
    # (b), (c) the arena
    arena = ea.Arena("cuda")
    for name, v in spec.items():
        arena.place(name, v, init=0xA5)
        assert arena.size(name) == EXTENTS[name](dims), (name, arena.size(name), EXTENTS[name](dims))
    assert set(spec) <= set(EXTENTS)

    def run(ar):
        call({k: ar.ptr(k) for k in spec})
    found, got = ea.report(arena, run, ("d_out",), {"d_out": plain})
    assert found == [], found

    def unread(ar, p):                                # the second pass: poison in the rows nobody may depend on
        g = a["gdesc"].copy()
        g.view(np.uint8).reshape(n, -1)[want["role"] == 0] = p
        g[int(c["cur_slot"])] = a["gdesc"][int(c["cur_slot"])]
        ar.set_initial("d_gdesc", g)
        b = a["best_cov"].copy()
        b.view(np.uint8).reshape(n, -1)[np.setdiff1d(np.arange(n), want["pass_slot"])] = p
        ar.set_initial("d_best_cov", b)
    found, _ = ea.report(arena, run, ("d_out",), {"d_out": plain}, before_fill=unread)
    assert found == [], ("rows without a part in the query", found)
    return want


def test_with_both_lists(ext, ref):
    want = three_calls(ext, ref, lc.generated(41, 300, 64, p_pass=0.5).arrays())
    assert want["n_pass"] > 50 and (want["role"] == 0).sum() > 5 and want["n_cand"] >= 1


def test_with_null_lists(ext, ref):
    want = three_calls(ext, ref, lc.generated(42, 130, 256, p_pass=0.5).arrays(), lists=False)
    assert want["n_pass"] > 20 and np.isinf(want["cov_min_score"])


def test_rows_whose_last_pass_is_one_float4(ext, ref):
    want = three_calls(ext, ref, lc.generated(43, 61, 1028, p_pass=0.5, cur=30).arrays())
    assert want["role"][60] != 0 and want["n_pass"] > 10           # the last row of the table is read
