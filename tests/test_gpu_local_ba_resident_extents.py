"""GPU: the two resident forms around the local bundle adjustment held to the buffer extents include/spfe.h documents, as
tests/test_gpu_map_point_culling_extents.py holds the map-point cull's: each form is called (a) with separate torch tensors and (b),
(c) with EVERY pointer argument — the graph's ord_slot, the rows, both flag arrays, the counts, the reference slots, the positions,
the poses, the gather's block, the solver's block at exactly SPFE_BA_OUT_BYTES of the gather's counts, the block — inside one arena
(tests/extent_arena.py) at exactly its documented size, the bytes between the buffers filled with 0xFF, then with 0x80.  No byte
outside a buffer may change, and every output must be byte-identical across the three calls and equal to tests/lba_ref/lba_ref.c.
Rows of 5, 7 and 1001 entries start off a 16-byte boundary, and the last row ends where the arena's poison begins: the row scan's
16-byte loads have to stop inside it.  Wild indices in the rows, in the ord row, in erase_idx, in the blocks' counts and entries are
never followed: the poison would show it.  And every SPFE_EINVAL case leaves everything untouched."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("lba_ref", ""):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
import extent_arena as ea  # noqa: E402
import lba_cases as lc  # noqa: E402
import lba_gpu as lg  # noqa: E402
import lba_ref as lr  # noqa: E402

from sp_orb_slam_amd import extractor as X  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import SPExtractor  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = lc.named_cases()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return lr.build(tmp_path_factory.mktemp("lba_ref"))


@pytest.fixture(scope="module")
def ext():
    e = SPExtractor(100, 64, 96, weights.synthetic(7, "trackable"), with_heat=False)
    yield e
    e.close()


def wild_rows(c, seed=3):
    """the case with a sixth of its row entries and half of its ord row overwritten with values that name nothing"""
    rng = np.random.RandomState(seed)
    c = dict(c, rows=c["rows"].copy(), ord_row=c["ord_row"].copy())
    nt, n = len(c["mp_flags"]), c["rows"].shape[0]
    hit = rng.rand(*c["rows"].shape) < 1 / 6
    c["rows"][hit] = rng.choice([-2, nt, nt + 1, 1 << 30, -(1 << 31)], int(hit.sum()))
    half = rng.rand(len(c["ord_row"])) < 0.5
    c["ord_row"][half] = rng.choice([-2, n, n + 7, 1 << 30, -(1 << 31)], int(half.sum()))
    return c


def three_calls(ext, ref, c):
    import torch
    spec, sizes, outs = lg.buffers(c), lg.extents(c), lg.outputs(c)
    want, _ = lg.want_of(ref, c)
    plain = lg.run_resident(ext, c)
    for k in outs:
        assert plain[k].tobytes() == np.asarray(want[k]).tobytes(), k
    arena = ea.Arena("cuda")
    for name, v in spec.items():
        arena.place(name, v, init=0xA5)
        assert arena.size(name) == sizes[name], (name, arena.size(name), sizes[name])

    def run(ar):
        lg.call(ext, {k: ar.ptr(k) for k in spec}, c)
        torch.cuda.synchronize()
    found, _ = ea.report(arena, run, outs, plain)
    assert found == [], found


@pytest.mark.parametrize("name", ["g_one_slot_one_entry_one_point", "g_pitch_1", "g_pitch_3", "g_pitch_5", "g_pitch_7", "g_pitch_1001", "g_slots_300",
                                  "g_points_0", "g_points_1025", "g_seen_by_1_2_3_4_200_and_twice_in_a_row", "g_ord_bad_wild_repeated",
                                  "g_ord_full_to_conn_cap", "g_kf_cap_plus_1", "g_point_cap_one_short", "g_edge_cap_exact", "g_edge_cap_one_short"])
def test_gather_local_ba_resident(ext, ref, name):
    three_calls(ext, ref, CASES[name])


@pytest.mark.parametrize("name", ["g_pitch_7", "g_slots_300", "g_ord_full_to_conn_cap"])
def test_gather_never_follows_a_wild_entry(ext, ref, name):
    three_calls(ext, ref, wild_rows(CASES[name]))


@pytest.mark.parametrize("name", ["a_erase_nothing", "a_3_to_2_goes_bad", "a_erase_every_observation", "a_bad_cap_exceeded", "a_bad_cap_0",
                                  "a_200_observations_half_erased", "a_random_erases", "a_refused_unsorted", "a_refused_n_edges_differs",
                                  "a_refused_gather_overflowed", "a_wild_erase_indices", "a_wild_n_erase", "a_wild_count_n_kf",
                                  "a_wild_count_n_points", "a_wild_count_n_obs", "a_wild_count_n_edges", "a_wild_count_n_local",
                                  "a_wild_count_n_points_negative", "a_wild_entries_in_the_gather_block"])
def test_apply_local_ba_resident(ext, ref, name):
    three_calls(ext, ref, CASES[name])


def test_einval_leaves_everything_untouched(ext):
    import torch
    g, a = CASES["g_ord_bad_wild_repeated"], CASES["a_3_to_2_goes_bad"]
    t = {}
    for key, case in (("g", g), ("a", a)):
        for k, v in lg.buffers(case).items():
            t[key + k] = (torch.full((int(v),), 0xA5, dtype=torch.uint8, device="cuda") if isinstance(v, (int, np.integer)) else
                          torch.from_numpy(lg.raw(v).copy()).cuda())
    before = {k: v.clone() for k, v in t.items()}

    def ptrs(key):
        return {k[1:]: v.data_ptr() for k, v in t.items() if k[0] == key}

    def refused(fn, what):
        with pytest.raises(X.SpfeError) as info:
            fn()
        assert str(info.value).startswith("SPFE_EINVAL"), (what, info.value)

    P = ptrs("g")
    n, stride = g["rows"].shape
    ok = dict(P, conn_cap=len(g["ord_row"]), stride=stride, n=n, n_table=len(g["mp_flags"]), cur=6, origin=2, kf_cap=8, free_cap=8, point_cap=64,
              edge_cap=512)
    bad = [dict(conn_cap=0), dict(conn_cap=4097), dict(stride=0), dict(stride=16385), dict(n=0), dict(n=65537), dict(n_table=0), dict(n_table=262145),
           dict(cur=-1), dict(cur=n), dict(origin=-2), dict(origin=n), dict(kf_cap=0), dict(kf_cap=129), dict(free_cap=0), dict(free_cap=65),
           dict(point_cap=0), dict(point_cap=16385), dict(edge_cap=0), dict(edge_cap=131073)]
    bad += [{k: None} for k in ("ord_slot", "rows", "kf_flags", "mp_flags", "xyz", "Tcw", "d_out")]
    bad += [{k: P[k] + 2} for k in ("ord_slot", "rows", "xyz", "Tcw")] + [dict(d_out=P["d_out"] + 8)]
    for change in bad:
        q = dict(ok, **change)
        refused(lambda: ext.gather_local_ba_resident(q["ord_slot"], q["conn_cap"], q["rows"], q["stride"], q["kf_flags"], q["n"], q["mp_flags"],
                                                     q["xyz"], q["n_table"], q["Tcw"], q["cur"], q["d_out"], origin_slot=q["origin"],
                                                     kf_cap=q["kf_cap"], free_cap=q["free_cap"], point_cap=q["point_cap"],
                                                     edge_cap=q["edge_cap"]), change)
    P = ptrs("a")
    n, stride = a["rows"].shape
    ok = dict(P, stride=stride, n=n, n_table=len(a["mp_flags"]), kf_cap=128, point_cap=8, edge_cap=256, bad_cap=8)
    bad = [dict(stride=0), dict(stride=16385), dict(n=0), dict(n=65537), dict(n_table=0), dict(n_table=262145), dict(kf_cap=0), dict(kf_cap=129),
           dict(point_cap=0), dict(point_cap=16385), dict(edge_cap=0), dict(edge_cap=131073), dict(bad_cap=-1), dict(bad_cap=16385)]
    bad += [{k: None} for k in ("gather", "ba", "rows", "kf_flags", "mp_flags", "nobs", "ref_slot", "xyz", "Tcw", "d_out")]
    bad += [{k: P[k] + 2} for k in ("rows", "nobs", "ref_slot", "xyz", "Tcw")] + [{k: P[k] + 8} for k in ("gather", "ba", "d_out")]
    for change in bad:
        q = dict(ok, **change)
        refused(lambda: ext.apply_local_ba_resident(q["gather"], q["ba"], q["rows"], q["stride"], q["kf_flags"], q["n"], q["mp_flags"], q["nobs"],
                                                    q["ref_slot"], q["xyz"], q["n_table"], q["Tcw"], q["kf_cap"], q["point_cap"], q["edge_cap"],
                                                    q["d_out"], bad_cap=q["bad_cap"]), change)
    torch.cuda.synchronize()
    for k in t:
        assert torch.equal(t[k], before[k]), k
