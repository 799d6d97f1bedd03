"""GPU: the resident forms of keyframe culling held to the buffer extents include/spfe.h documents, as
tests/test_gpu_covisibility_extents.py holds the graph's: each form is called (a) with separate torch tensors and (b), (c) with EVERY
pointer argument — the rows, both flag arrays, the observation counts, the eight state arrays, the two tables, the block — inside
one arena (tests/extent_arena.py) at exactly its documented size, the bytes between the buffers filled with 0xFF, then with 0x80.
No byte outside a buffer may change, and every output must be byte-identical across the three calls and equal to
tests/cull_ref/cull_ref.c.  Rows of 101 entries are 404 bytes: only every fourth starts on a 16-byte boundary, and the last row
ends where the arena's poison begins; the culled keyframe, a touched neighbour and a re-parented child are the LAST slots, so their
state rows and table rows end there too.  And every SPFE_EINVAL case leaves the state and the block untouched."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("cull_ref", ""):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
import cull_cases as cc  # noqa: E402
import cull_ref  # noqa: E402
import extent_arena as ea  # noqa: E402

from sp_orb_slam_amd import extractor as X  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import SPExtractor  # noqa: E402

pytestmark = pytest.mark.gpu

# argument -> bytes, by the comments above the declarations in include/spfe.h
EXTENTS = dict(rows=lambda d: 4 * d["stride"] * d["n"], kf_flags=lambda d: d["n"], mp_flags=lambda d: d["n_table"],
               nobs=lambda d: 4 * d["n_table"], conn_slot=lambda d: 4 * d["n"] * d["cap"], conn_w=lambda d: 4 * d["n"] * d["cap"],
               conn_n=lambda d: 4 * d["n"], ord_slot=lambda d: 4 * d["n"] * d["cap"], ord_w=lambda d: 4 * d["n"] * d["cap"],
               ord_n=lambda d: 4 * d["n"], parent=lambda d: 4 * d["n"], first_conn=lambda d: d["n"],
               best_a=lambda d: 4 * d["n_best_a"] * d["n"], best_b=lambda d: 4 * d["n_best_b"] * d["n"],
               d_out=lambda d: X.cull_offsets(d["n"], d["cap"], d["bad_cap"])["out_bytes"])


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return cull_ref.build(tmp_path_factory.mktemp("cull_ref"))


@pytest.fixture(scope="module")
def ext():
    e = SPExtractor(100, 64, 96, weights.synthetic(7, "trackable"), with_heat=False)
    yield e
    e.close()


def three_calls(spec, dims, call, outputs, want):
    """spec: name -> array (initial contents) or int (an output of that many bytes); call(P); want: name -> the reference's bytes"""
    import torch
    assert set(spec) <= set(EXTENTS)
    tens = {k: (torch.full((int(v),), 0xA5, dtype=torch.uint8, device="cuda") if isinstance(v, (int, np.integer)) else
                torch.from_numpy(np.ascontiguousarray(v).reshape(-1).view(np.uint8).copy()).cuda()) for k, v in spec.items()}
    call({k: t.data_ptr() for k, t in tens.items()})
    torch.cuda.synchronize()
    plain = {k: tens[k].cpu().numpy() for k in outputs}
    for k in outputs:
        assert plain[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), k
    arena = ea.Arena("cuda")
    for name, v in spec.items():
        arena.place(name, v, init=0xA5)
        assert arena.size(name) == EXTENTS[name](dims), (name, arena.size(name), EXTENTS[name](dims))

    def run(ar):
        call({k: ar.ptr(k) for k in spec})
        torch.cuda.synchronize()
    found, _ = ea.report(arena, run, outputs, plain)
    assert found == [], found


def last_slots_world(stride, n_table):
    """n = 12: the current keyframe 8 lists slot 11, which is culled; slot 10 holds a link to it and is its child with a link to its
    parent 9; one of the culled row's points goes bad and the last entry of the last live row (10) names one of them"""
    n, cap = 12, 4
    w = cull_ref.new_world(n, stride, n_table, cap, 32, 1)
    w["first_conn"][:] = 0
    w["parent"][:] = np.arange(n) - 1
    w["parent"][11], w["parent"][10] = 9, 11
    pts = np.arange(stride) % n_table
    w["rows"][11] = pts
    w["rows"][10] = -1
    w["rows"][10, stride - 1] = pts[0]
    w["nobs"][:] = 9
    w["nobs"][pts[0]] = 3 if stride <= n_table else 9
    cc.link(w, 10, 11, 7)
    cc.link(w, 10, 9, 5)
    cc.link(w, 8, 11, 30)
    cc.set_links(w, 8, {11: 30}, [(11, 30)])
    return w, dict(cur=8, th_obs=3, cov_ratio=0.9, origin_slot=0, bad_cap=3)


@pytest.mark.parametrize("stride,n_table", [(1, 1), (5, 9), (101, 300), (1001, 1500)])
def test_cull_keyframes_resident_last_slots(ext, ref, stride, n_table):
    w, prm = last_slots_world(stride, n_table)
    n, cap = w["conn_slot"].shape
    dims = dict(n=n, stride=stride, n_table=n_table, cap=cap, n_best_a=32, n_best_b=1, bad_cap=prm["bad_cap"])
    spec = {k: w[k] for k in cull_ref.WORLD}
    spec["d_out"] = X.cull_offsets(n, cap, prm["bad_cap"])["out_bytes"]
    ww = cull_ref.copy_world(w)
    r = cull_ref.cull(ref, ww, **prm)
    assert r["n_culled"] == 1 and r["touched_slot"][:r["n_touched"]].tolist() == [8, 10] and r["event_child"][0] == 10
    assert r["n_bad"] == (1 if stride <= n_table else 0) and ww["parent"][10] == 9
    want = dict({k: ww[k] for k in cull_ref.WORLD}, d_out=r["block"])

    def call(P):
        g = X.covis_graph({k: P[k] for k in cull_ref.STATE}, n, cap)
        ext.cull_keyframes_resident(g, P["rows"], stride, P["kf_flags"], P["mp_flags"], P["nobs"], n_table, prm["cur"], P["d_out"],
                                    th_obs=prm["th_obs"], cov_ratio=prm["cov_ratio"], origin_slot=prm["origin_slot"],
                                    bad_cap=prm["bad_cap"], d_best_cov_a=P["best_a"], n_best_a=32, d_best_cov_b=P["best_b"], n_best_b=1)
    three_calls(spec, dims, call, tuple(cull_ref.WORLD) + ("d_out",), want)


@pytest.mark.parametrize("n,stride,n_table", [(1, 1, 1), (7, 5, 3), (65, 101, 700), (300, 1001, 40)])
def test_count_observations_resident(ext, ref, n, stride, n_table):
    w, _ = cc.generated_world(30 + n, n, stride, n_table, 2, 1, dup=True)
    w["rows"][n - 1, stride - 1] = n_table - 1
    w["kf_flags"][n - 1] = 0
    dims = dict(n=n, stride=stride, n_table=n_table)
    spec = dict(rows=w["rows"], kf_flags=w["kf_flags"], nobs=4 * n_table)
    want = dict(nobs=cull_ref.count(ref, w["rows"], w["kf_flags"], n_table))

    def call(P):
        ext.count_observations_resident(P["rows"], stride, P["kf_flags"], n, P["nobs"], n_table)
    three_calls(spec, dims, call, ("nobs",), want)


def test_einval_leaves_state_and_block_untouched(ext):
    import torch
    c = cc.named_cases()["one_culled"]
    w, prm = cull_ref.case_world(c), cull_ref.case_params(c)
    n, stride = w["rows"].shape
    cap, n_table = w["conn_slot"].shape[1], len(w["mp_flags"])
    t = {k: torch.from_numpy(np.ascontiguousarray(w[k]).reshape(-1).view(np.uint8).copy()).cuda() for k in cull_ref.WORLD}
    t["d_out"] = torch.full((X.cull_offsets(n, cap, 8)["out_bytes"],), 0xA5, dtype=torch.uint8, device="cuda")
    before = {k: v.clone() for k, v in t.items()}
    P = {k: v.data_ptr() for k, v in t.items()}
    ok = dict(graph=dict(P), n=n, cap=cap, rows=P["rows"], stride=stride, kf_flags=P["kf_flags"], mp_flags=P["mp_flags"],
              nobs=P["nobs"], n_table=n_table, cur=prm["cur"], out=P["d_out"], th_obs=3, cov_ratio=0.75, origin_slot=0, bad_cap=8,
              best_a=P["best_a"], n_best_a=3, best_b=P["best_b"], n_best_b=2)
    bad = [dict(n=0), dict(n=65537), dict(cap=0), dict(cap=4097), dict(stride=0), dict(stride=16385), dict(n_table=-1),
           dict(n_table=262145), dict(cur=-1), dict(cur=n), dict(th_obs=0), dict(bad_cap=-1), dict(bad_cap=262145),
           dict(origin_slot=-2), dict(origin_slot=n), dict(n_best_a=0), dict(n_best_a=33), dict(n_best_b=0), dict(n_best_b=33),
           dict(rows=None), dict(kf_flags=None), dict(mp_flags=None), dict(nobs=None), dict(out=None), dict(rows=P["rows"] + 2),
           dict(nobs=P["nobs"] + 1), dict(best_a=P["best_a"] + 2), dict(best_b=P["best_b"] + 1), dict(out=P["d_out"] + 8)]
    bad += [dict(graph=dict(P, **{k: None})) for k in cull_ref.STATE]
    bad += [dict(graph=dict(P, **{k: P[k] + 2})) for k in cull_ref.STATE if k != "first_conn"]
    for change in bad:
        a = dict(ok, **change)
        g = X.covis_graph({k: a["graph"][k] for k in cull_ref.STATE}, a["n"], a["cap"])
        with pytest.raises(X.SpfeError) as info:
            ext.cull_keyframes_resident(g, a["rows"], a["stride"], a["kf_flags"], a["mp_flags"], a["nobs"], a["n_table"], a["cur"],
                                        a["out"], th_obs=a["th_obs"], cov_ratio=a["cov_ratio"], origin_slot=a["origin_slot"],
                                        bad_cap=a["bad_cap"], d_best_cov_a=a["best_a"], n_best_a=a["n_best_a"],
                                        d_best_cov_b=a["best_b"], n_best_b=a["n_best_b"])
        assert str(info.value).startswith("SPFE_EINVAL"), (change, info.value)
    for change in (dict(n=0), dict(stride=0), dict(n_table=-1), dict(rows=None), dict(kf_flags=None), dict(nobs=None),
                   dict(rows=P["rows"] + 1), dict(nobs=P["nobs"] + 2)):
        a = dict(ok, **change)
        with pytest.raises(X.SpfeError) as info:
            ext.count_observations_resident(a["rows"], a["stride"], a["kf_flags"], a["n"], a["nobs"], a["n_table"])
        assert str(info.value).startswith("SPFE_EINVAL"), (change, info.value)
    torch.cuda.synchronize()
    for k in t:
        assert torch.equal(t[k], before[k]), k
