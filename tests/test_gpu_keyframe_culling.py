"""GPU: keyframe culling on the device (spfe_cull_keyframes_resident, spfe_cull_keyframes, spfe_count_observations_resident) against
tests/cull_ref/cull_ref.c byte for byte — the block, all eight graph arrays, both tables, the rows, both flag arrays and the
observation counts, from both forms — on every fixture tests/golden/cull_*.npz and at the smallest shapes where the kernels can go
wrong: one and two slots, rows of 1, 3, 5, 64 and 1001 entries whose base lies 4 - 12 bytes off a 16-byte boundary, lists on both
sides of a wavefront's share, of the 16 wavefronts and of the workgroup, conn_cap 1, 2, 256 and 4096, tables of 1 and 50,000 points,
more than 40 passes in one call, 0, 1 and 300 touched neighbours, neighbour maps of 1, 255 - 259 and 4095 keys, and 80 calls alternating with
spfe_update_connections_resident on state that never leaves the device.  The kernels keep no per-point table in LDS (they read
mp_flags and nobs from L2), so there is no LDS capacity to stand on either side of.  The block and the tables hold 0xA5 before a
call and the graph rows the call has no business with 0x5A: whatever the contract leaves alone keeps those bytes."""
import glob
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("cull_ref", "covis_ref", ""):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
import covis_ref  # noqa: E402
import cull_cases as cc  # noqa: E402
import cull_gpu as cg  # noqa: E402
import cull_ref  # noqa: E402

from sp_orb_slam_amd import extractor as X  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import SPExtractor  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "cull_*.npz")))
NAMES = [os.path.basename(p)[5:-4] for p in FIXTURES]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return cull_ref.build(tmp_path_factory.mktemp("cull_ref"))


@pytest.fixture(scope="module")
def cref(tmp_path_factory):
    return covis_ref.build(tmp_path_factory.mktemp("covis_ref"))


@pytest.fixture(scope="module")
def ext():
    e = SPExtractor(100, 64, 96, weights.synthetic(7, "trackable"), with_heat=False)
    yield e
    e.close()


def count_check(ext, w, shift=0):
    """spfe_count_observations_resident on the world's rows against numpy; the array starts as rubbish"""
    import torch
    n, stride = w["rows"].shape
    n_table = len(w["mp_flags"])
    want = np.zeros(n_table, np.int64)
    for s in range(n):
        if not w["kf_flags"][s] & 1:
            r = w["rows"][s]
            np.add.at(want, r[(r >= 0) & (r < n_table)], 1)
    d_rows, d_f = cg.dev(w["rows"], shift), cg.dev(w["kf_flags"])
    d_nobs = torch.full((4 * n_table + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    ext.count_observations_resident(d_rows.data_ptr(), stride, d_f.data_ptr(), n, d_nobs.data_ptr(), n_table)
    torch.cuda.synchronize()
    raw = d_nobs.cpu().numpy()
    assert (raw[4 * n_table:] == 0xA5).all(), "bytes behind d_mp_nobs were written"
    assert (raw[:4 * n_table].view(np.int32) == want).all()


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_fixture(ext, ref, path):
    c = cc.load_fixture(path)
    w, prm = cull_ref.case_world(c), cull_ref.case_params(c)
    r, ww = cg.check(ext, ref, w, prm, what=os.path.basename(path))
    assert r["block"].tobytes() == c["e_block"].tobytes()
    for k in cull_ref.WORLD:
        if k not in cg.ROWS4:                       # the rows the call does not read were poisoned here
            assert ww[k].tobytes() == c["e_" + k].tobytes(), k


# n_slots, kp_stride, n_table, conn_cap, listed, th_obs, cov_ratio, bad_cap, shift of the rows' base, seed
SHAPES = {
    "one_slot_empty_list": (1, 1, 1, 1, 0, 1, 0.5, 0, 4, 11),
    "two_slots_stride_3_table_of_one": (2, 3, 1, 1, 1, 1, 0.5, 1, 4, 12),
    "two_slots_stride_5_cap_2": (2, 5, 7, 2, 1, 1, 0.5, 3, 8, 13),
    "list_15": (300, 64, 3000, 256, 15, 4, 0.5, 40, 12, 14),
    "list_16": (300, 64, 3000, 256, 16, 4, 0.5, 40, 4, 15),
    "list_17": (300, 64, 3000, 256, 17, 4, 0.5, 40, 8, 16),
    "list_63": (300, 64, 3000, 256, 63, 4, 0.5, 400, 12, 17),
    "list_64": (300, 64, 3000, 256, 64, 4, 0.5, 400, 4, 18),
    "list_65": (300, 64, 3000, 256, 65, 4, 0.5, 400, 8, 19),
    "list_300_stride_1001_table_50000_cap_4096": (301, 1001, 50000, 4096, 300, 4, 0.55, 5000, 12, 20),
    "more_than_40_passes": (130, 33, 600, 128, 120, 3, 0.4, 600, 4, 21),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shape(ext, ref, name):
    n, stride, n_table, cap, listed, th_obs, cov, bad_cap, shift, seed = SHAPES[name]
    w, cur = cc.generated_world(seed, n, stride, n_table, cap, listed, dup=seed % 2 == 0)
    prm = dict(cur=cur, th_obs=th_obs, cov_ratio=cov, origin_slot=0 if n > 2 else -1, bad_cap=bad_cap)
    count_check(ext, w, shift)
    r, _ = cg.check(ext, ref, w, prm, shift=shift, what=name)
    print(name, {k: r[k] for k in cull_ref.FIELDS})
    assert r["n_listed"] == min(listed, n - 1)
    if name.startswith("list_"):
        assert r["n_culled"] >= 1 and r["n_passes"] >= 2 and r["n_touched"] >= 1 and r["n_bad"] >= 1, name
    if name == "more_than_40_passes":
        assert r["n_passes"] >= 40, r["n_passes"]
        assert r["status"] & cull_ref.EVENT_CUT and r["n_reparented"] > r["n_events"] == n, (r["n_reparented"], r["n_events"])


def star(n, cap, hub, spokes, stride=3):
    """slot `hub` linked with every slot of `spokes`, the current keyframe n - 1 listing the hub alone; the hub's row is all
    redundant, so it is culled"""
    w = cull_ref.new_world(n, stride, 16, cap, 20, 10)
    w["nobs"][:] = 9
    w["first_conn"][:] = 0
    w["parent"][:] = np.maximum(np.arange(n) - 1, 0)
    w["parent"][0] = -1
    w["rows"][hub] = np.arange(stride)
    cur = n - 1
    cc.set_links(w, hub, {int(s): 3 + int(s) % 5 for s in spokes})
    for s in spokes:
        cc.set_links(w, int(s), {hub: 3 + int(s) % 5})
    cc.set_links(w, cur, {hub: 50}, [(hub, 50)])
    return w, dict(cur=cur, th_obs=3, cov_ratio=0.9, origin_slot=0, bad_cap=4)


def test_three_hundred_touched_neighbours_with_maps_of_one_key(ext, ref):
    w, prm = star(320, 512, 7, [s for s in range(8, 308)])
    r, ww = cg.check(ext, ref, w, prm, what="300 touched")
    assert r["n_touched"] == 300 and r["n_culled"] == 1 and (ww["conn_n"][8:308] == 0).all()


def test_no_touched_neighbour(ext, ref):
    """the hub holds links nobody returns: nothing is removed anywhere, its own rows are cleared"""
    w, prm = star(40, 64, 7, [s for s in range(8, 30)])
    for s in range(8, 30):
        cc.set_links(w, s, {})
    r, ww = cg.check(ext, ref, w, prm, what="no touched")
    assert r["n_touched"] == 0 and r["n_culled"] == 1 and ww["conn_n"][7] == 0


def test_neighbour_map_of_4095_keys(ext, ref):
    """conn_cap 4096: the one touched neighbour holds 4095 keys, the culled keyframe among them in the middle; ord is rebuilt from
    a part of the map to all 4094 that stay, equal weights by slot descending"""
    n, cap, hub, nb = 4100, 4096, 2000, 4099 - 1
    w = cull_ref.new_world(n, 3, 16, cap, 32, 1)
    w["nobs"][:] = 9
    w["first_conn"][:] = 0
    w["parent"][:] = np.maximum(np.arange(n) - 1, 0)
    w["rows"][hub] = [0, 1, 2]
    keys = [s for s in range(3, 3 + 4095)]
    assert hub in keys and nb not in keys
    cc.set_links(w, nb, {s: 1 + (s * 7) % 13 for s in keys}, [(s, 1 + (s * 7) % 13) for s in keys[:100]])
    cc.set_links(w, hub, {nb: 5})
    cc.set_links(w, n - 1, {hub: 50}, [(hub, 50)])
    prm = dict(cur=n - 1, th_obs=3, cov_ratio=0.9, origin_slot=0, bad_cap=0)
    r, ww = cg.check(ext, ref, w, prm, poison=False, what="4095 keys")
    assert r["n_touched"] == 1 and ww["conn_n"][nb] == 4094 and ww["ord_n"][nb] == 4094


@pytest.mark.parametrize("k", [255, 256, 257, 258])
def test_neighbour_maps_on_both_sides_of_a_wavefronts_share(ext, ref, k):
    """a neighbour map of up to 256 keys is one wavefront's work, a larger one the whole workgroup's: two neighbours of k and k + 1
    keys beside 20 small ones, ord rebuilt from a part of the map"""
    n, cap, hub = 600, 512, 7
    w, prm = star(n, cap, hub, [s for s in range(8, 30)])
    for nb, size in ((8, k), (9, k + 1)):
        keys = [hub] + [s for s in range(40, 40 + size - 1)]
        cc.set_links(w, nb, {s: 2 + (s * 5) % 11 for s in keys}, [(s, 2 + (s * 5) % 11) for s in keys[:9]])
    r, ww = cg.check(ext, ref, w, prm, what="maps of %d and %d keys" % (k, k + 1))
    assert r["n_touched"] == 22 and ww["conn_n"][8] == k - 1 and ww["ord_n"][9] == k


def test_eighty_calls_alternating_with_update_connections_on_the_device(ext, ref, cref):
    """40 keyframes inserted one by one: spfe_update_connections_resident, then the cull, the world resident throughout (the host
    writes the new row, clears its flag and adds its observations with single-entry writes); every block and the final world
    equal the two host references chained"""
    import torch
    w, rng, geo = cc.sequence_world(9, n_slots=40)
    n, stride = w["rows"].shape
    n_table, cap = len(w["mp_flags"]), w["conn_slot"].shape[1]
    d = cg.DeviceWorld(w)
    nb_cull, nb_cov = ext.cull_out_bytes(n, cap, 16), ext.covis_out_bytes(n, cap)
    d_cull = torch.full((n, nb_cull), cg.FILL, dtype=torch.uint8, device="cuda")
    d_cov = torch.full((n, nb_cov), cg.FILL, dtype=torch.uint8, device="cuda")
    rows_t, nobs_t = d.t["rows"][:4 * n * stride].view(torch.int32).view(n, stride), d.t["nobs"][:4 * n_table].view(torch.int32)
    want_cull, want_cov, culled = [], [], 0
    for s in range(n):
        cc.insert_keyframe(w, rng, geo, s)
        row = torch.from_numpy(w["rows"][s].copy()).cuda()
        rows_t[s] = row
        d.t["kf_flags"][s] = 0
        nobs_t[row[row >= 0].long()] += 1
        prm = dict(cur=s, th_obs=3, cov_ratio=0.6, origin_slot=0, bad_cap=16)
        ext.update_connections_resident(d.graph, d.ptr("rows"), stride, d.ptr("kf_flags"), d.ptr("mp_flags"), n_table, s,
                                        d_cov[s].data_ptr(), th=8, origin_slot=0, d_best_cov_a=d.ptr("best_a"), n_best_a=20,
                                        d_best_cov_b=d.ptr("best_b"), n_best_b=10)
        d.cull(ext, d_cull[s].data_ptr(), prm)
        want_cov.append(covis_ref.update(cref, w["rows"], w["kf_flags"], w["mp_flags"], {k: w[k] for k in covis_ref.STATE}, s, 8, 0,
                                         w["best_a"], w["best_b"])["block"])
        r = cull_ref.cull(ref, w, **prm)
        want_cull.append(r["block"])
        culled += r["n_culled"]
    torch.cuda.synchronize()
    assert culled >= 3
    got_cull, got_cov = d_cull.cpu().numpy(), d_cov.cpu().numpy()
    for s in range(n):
        assert got_cov[s].tobytes() == want_cov[s].tobytes(), ("UpdateConnections block", s)
        cg.same((got_cull[s], w), (want_cull[s], w), dict(bad_cap=16), "cull block %d" % s)
    cg.same((want_cull[-1], d.download()), (want_cull[-1], w), dict(bad_cap=16), "the world after 80 calls")


def test_null_tables_and_default_stream(ext, ref):
    c = cc.named_cases()["nobs_three_to_two_goes_bad"]
    w, prm = cull_ref.case_world(c), cull_ref.case_params(c)
    w["best_a"] = None
    cg.check(ext, ref, w, prm, what="no table a")
    w["best_b"] = None
    cg.check(ext, ref, w, prm, what="no table")
