"""GPU: the tracker's local map on the device (spfe_update_local_map_resident, spfe_update_local_map, spfe_count_shared_points_resident,
spfe_local_map_rows_resident: localmap.hip) against the host reference tests/localmap_ref/localmap_ref.c, which shares
include/spfe_localmap_math.h with the kernels: the WHOLE output block byte for byte, from both forms, every byte behind it still
holding the preset — on the fixtures tests/golden/localmap_*.npz (every rule of the walk); at 1, 2, 65 and 300 slots (300 voted
keyframes: the walk stops at once); at row pitches of 1, 4, 5, 101 and 1001 entries (rows that are not 16-byte aligned, a table
that starts 4 bytes off a boundary); at tables of 1, 257 and 50,000 points and on either side of the weight table's LDS capacity;
with 0, 1 and 1001 keypoints; the count form with and without an outlier mask; the rows form as a round trip; the refusals."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "localmap_ref"))
import localmap_cases as lc  # noqa: E402
import localmap_ref  # noqa: E402

from sp_orb_slam_amd import extractor as X  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import SPExtractor, SpfeError  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = localmap_ref.FILL
GUARD = 1024          # bytes behind the block that must keep the preset
ARRAYS = ("kf_mp_of_kp", "kf_flags", "best_cov", "parent", "mp_flags", "mp_of_kp")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return localmap_ref.build(tmp_path_factory.mktemp("localmap_ref"))


@pytest.fixture(scope="module")
def ext():
    e = SPExtractor(100, 64, 96, weights.synthetic(7, "trackable"), with_heat=False)
    yield e
    e.close()


def dev(a, shift=0):
    """the array's bytes on the device, `shift` bytes behind a 256-byte boundary"""
    import torch
    a = np.ascontiguousarray(a)
    raw = a.reshape(-1).view(np.uint8)
    t = torch.zeros(shift + max(len(raw), 16), dtype=torch.uint8, device="cuda")
    if len(raw):
        t[shift:shift + len(raw)] = torch.from_numpy(raw.copy()).cuda()
    return t[shift:]


def upload(c, shift=0):
    a = localmap_ref.arrays(c)
    return a, {k: dev(a[k], shift if k == "kf_mp_of_kp" else 0) for k in ARRAYS}


def call_device(ext, c, a, d, d_out, stream=None):
    n, stride = a["kf_mp_of_kp"].shape
    n_kp = len(a["mp_of_kp"])
    ext.update_local_map_resident(d["kf_mp_of_kp"].data_ptr(), stride, d["kf_flags"].data_ptr(), d["best_cov"].data_ptr(),
                                  a["best_cov"].shape[1], d["parent"].data_ptr(), n,
                                  d["mp_flags"].data_ptr() if len(a["mp_flags"]) else None, len(a["mp_flags"]),
                                  d["mp_of_kp"].data_ptr() if n_kp else None, n_kp, d_out.data_ptr(), int(c["point_cap"]),
                                  int(c["max_keyframes"]), stream=stream)


def run_resident(ext, c, shift=0):
    """spfe_update_local_map_resident on a block and a guard behind it filled with FILL -> the block (the guard checked)"""
    import torch
    a, d = upload(c, shift)
    nb = ext.localmap_out_bytes(len(a["kf_mp_of_kp"]), c["point_cap"], len(a["mp_of_kp"]))
    d_out = torch.full((nb + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    before = {k: v.clone() for k, v in d.items()}
    call_device(ext, c, a, d, d_out)
    torch.cuda.synchronize()
    assert all(torch.equal(d[k], before[k]) for k in d), "an input was written"
    raw = d_out.cpu().numpy()
    assert (raw[nb:] == FILL).all(), "bytes behind the block were written"
    return raw[:nb]


def run_host(ext, c):
    a = localmap_ref.arrays(c)
    return ext.update_local_map(a["kf_mp_of_kp"], a["kf_flags"], a["best_cov"], a["parent"], a["mp_flags"], a["mp_of_kp"],
                                int(c["point_cap"]), int(c["max_keyframes"]), fill=FILL)


def same(block, want, c, what):
    if block.tobytes() == want["block"].tobytes():
        return
    n, cap, n_kp = len(c["kf_mp_of_kp"]), int(c["point_cap"]), len(np.asarray(c["mp_of_kp"]).reshape(-1))
    g = X.SPExtractor.decode_localmap_out(block, n, cap, n_kp)
    for k in localmap_ref.FIELDS:
        assert g[k] == want[k], (what, k, g[k], want[k])
    for k in ("votes", "total", "local_kf", "point_idx", "mp_of_kp_list"):
        assert g[k].tobytes() == want[k].tobytes(), (what, k, np.flatnonzero(g[k] != want[k])[:8])
    diff = np.flatnonzero(block != want["block"])
    assert not len(diff), (what, "bytes the block does not name", diff[:8])


def both_forms(ext, ref, c, what, shift=0):
    want = localmap_ref.update(ref, c)
    same(run_resident(ext, c, shift), want, c, what + ", resident form")
    same(run_host(ext, c), want, c, what + ", host form")
    return want


@pytest.mark.parametrize("name", sorted(lc.named_cases()))
def test_fixtures(ext, ref, name):
    z = np.load(os.path.join(ROOT, "tests", "golden", "localmap_%s.npz" % name))
    c = {k: (int(z[k]) if z[k].ndim == 0 else z[k]) for k in lc.KEYS}
    want = both_forms(ext, ref, c, name)
    assert want["block"].tobytes() == z["e_block"].tobytes(), name     # ... and the reference still gives what was recorded
    assert (want["point_idx"][want["n_points"]:] == -1).all()


# seed, n_slots, kp_stride, n_table, n_kp, keywords: every value of the four axes, and the pairs that take another path
SHAPES = [
    (301, 1, 1, 1, 0, {}), (302, 1, 1001, 257, 1, dict(p_hold=1.0)), (303, 2, 4, 1, 1, {}), (304, 2, 5, 257, 1001, dict(point_cap=1001)),
    (305, 65, 1, 257, 1, dict(p_hold=1.0)), (306, 65, 5, 50000, 1001, dict(point_cap=8192)), (307, 65, 101, 257, 1001, dict(point_cap=2000)),
    (308, 65, 1001, 50000, 1001, dict(point_cap=8192, chain=True)), (309, 300, 4, 257, 1001, dict(point_cap=4096, vote_all=True, p_hold=1.0)),
    (310, 300, 101, 50000, 1001, dict(point_cap=8192)), (311, 300, 1001, 50000, 1001, dict(point_cap=8192, chain=True, vote_all=True)),
    (312, 300, 5, 257, 0, dict(point_cap=64)), (313, 65, 101, 50000, 1001, dict(point_cap=1001, n_best=32, vote_all=True)),
    (314, 40, 33, 900, 150, dict(chain=True, vote_all=True, p_hold=1.0, point_cap=8192)),
    (315, 30, 17, 400, 100, dict(chain=True, vote_all=True, max_keyframes=3, n_best=1)),
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "s%d_k%d_t%d_kp%d" % s[1:5])
def test_shapes(ext, ref, shape):
    seed, n, stride, n_table, n_kp, kw = shape
    c = lc.generated(seed, n, stride, n_table, n_kp, **kw)
    want = both_forms(ext, ref, c, "%s" % (shape,))
    if n == 300 and kw.get("vote_all"):
        assert want["n_voted"] > 80 and want["n_local_kf"] == want["n_voted"]        # the walk stops at once
    if seed == 314:
        assert want["n_local_kf"] > want["n_voted"] > 10                                 # ... and here it goes on
    if seed == 313:
        assert want["status"] & X.LOCALMAP_TRUNCATED and (want["point_idx"][want["n_points"]:] == -1).all()


@pytest.mark.parametrize("stride", [4, 5, 101])
def test_table_four_bytes_off_a_boundary(ext, ref, stride):
    """d_kf_mp_of_kp itself 4, 8 and 12 bytes behind a 16-byte boundary: the head of every row changes"""
    c = lc.generated(320 + stride, 65, stride, 2000, 300, point_cap=4096)
    want = localmap_ref.update(ref, c)
    for shift in (4, 8, 12):
        same(run_resident(ext, c, shift), want, c, "stride %d shift %d" % (stride, shift))
    assert want["n_voted"] >= 3


def test_either_side_of_the_lds_capacity(ext, ref):
    """the weight table in LDS, and one point more: from global memory.  The votes concentrate on the last points of the table."""
    cap = ext.localmap_lds_point_capacity()
    assert 50000 < cap < 262144
    for n_table in (cap, cap + 1):
        c = lc.generated(330, 65, 101, n_table, 1001, point_cap=8192, vote_all=True)
        c["kf_mp_of_kp"][64, :3] = [n_table - 1, n_table - 2, n_table]        # the table's last rows, and the first row behind it
        c["mp_of_kp"][:2] = [n_table - 1, n_table - 1]
        c["mp_flags"][n_table - 1] = 1
        c["kf_flags"][64] = 0
        want = both_forms(ext, ref, c, "n_table %d" % n_table)
        assert want["votes"][64] >= 2 and 64 in want["local_kf"]


def test_count_form_with_and_without_outliers(ext, ref):
    import torch
    for seed, n, stride, n_table, n_kp in ((340, 65, 101, 5000, 1001), (341, 300, 1001, 50000, 600), (342, 2, 5, 257, 1)):
        c = lc.generated(seed, n, stride, n_table, n_kp)
        a, d = upload(c)
        mask = (np.random.default_rng(seed).random(n_kp) < 0.3).astype(np.uint8)
        for m in (None, mask):
            want_v, want_t = localmap_ref.count(ref, c, m)
            d_v = torch.full((n + 64,), -7, dtype=torch.int32, device="cuda")
            d_t = torch.full((n + 64,), -7, dtype=torch.int32, device="cuda")
            d_m = None if m is None else dev(m)
            ext.count_shared_points_resident(d["kf_mp_of_kp"].data_ptr(), stride, n, d["mp_flags"].data_ptr(), n_table,
                                             d["mp_of_kp"].data_ptr(), None if m is None else d_m.data_ptr(), n_kp, d_v.data_ptr(),
                                             d_t.data_ptr())
            torch.cuda.synchronize()
            v, t = d_v.cpu().numpy(), d_t.cpu().numpy()
            assert np.array_equal(v[:n], want_v) and np.array_equal(t[:n], want_t), (seed, m is None)
            assert (v[n:] == -7).all() and (t[n:] == -7).all()


def test_rows_round_trip(ext, ref):
    """list positions back into table rows: the frame's holders come back as they went in, -1 where nothing was held; a position
    TrackLocalMap added (any position of the list) gives that point's row, and a position outside the list -1"""
    import torch
    c = lc.generated(350, 65, 101, 5000, 1001, point_cap=2000)
    want = localmap_ref.update(ref, c)
    block = run_resident(ext, c)
    cap, n_kp = c["point_cap"], 1001
    o = X.localmap_offsets(65, cap, n_kp)
    d_block = dev(block)
    d_rows = torch.full((n_kp + 16,), -7, dtype=torch.int32, device="cuda")
    ext.local_map_rows_resident(d_block.data_ptr() + o["point_idx"], cap, d_block.data_ptr() + o["mp_of_kp_list"], n_kp, d_rows.data_ptr())
    torch.cuda.synchronize()
    rows = d_rows.cpu().numpy()
    mp = np.asarray(c["mp_of_kp"])
    held = want["mp_of_kp_list"] >= 0
    assert held.sum() > 100 and np.array_equal(rows[:n_kp][held], mp[held]) and (rows[:n_kp][~held] == -1).all()
    assert (rows[n_kp:] == -7).all()
    lst = want["mp_of_kp_list"].copy()
    free = np.flatnonzero(~held)
    lst[free[0]], lst[free[1]], lst[free[2]], lst[free[3]] = want["n_points"] - 1, cap - 1, cap, -5
    d_list = dev(lst)
    ext.local_map_rows_resident(d_block.data_ptr() + o["point_idx"], cap, d_list.data_ptr(), n_kp, d_rows.data_ptr())
    torch.cuda.synchronize()
    rows = d_rows.cpu().numpy()
    assert rows[free[0]] == want["point_idx"][want["n_points"] - 1] and rows[free[1]] == want["point_idx"][cap - 1]
    assert rows[free[2]] == -1 and rows[free[3]] == -1


def test_refusals(ext):
    import torch
    c = lc.generated(360, 20, 9, 300, 50, point_cap=100)
    a, d = upload(c)
    n, stride = a["kf_mp_of_kp"].shape
    nb = ext.localmap_out_bytes(n, 100, 50)
    d_out = torch.full((nb,), FILL, dtype=torch.uint8, device="cuda")
    d_v = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    d_t = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    P = {k: v.data_ptr() for k, v in d.items()}

    def args(**over):
        v = dict(d_kf_mp_of_kp=P["kf_mp_of_kp"], kp_stride=stride, d_kf_flags=P["kf_flags"], d_best_cov=P["best_cov"], n_best=20,
                 d_parent=P["parent"], n_slots=n, d_mp_flags=P["mp_flags"], n_table=300, d_mp_of_kp=P["mp_of_kp"], n_kp=50,
                 d_out=d_out.data_ptr(), point_cap=100, max_keyframes=80)
        v.update(over)
        return v
    bad = [dict(n_slots=0), dict(n_slots=X.LOCALMAP_MAX_KEYFRAMES + 1), dict(kp_stride=0), dict(kp_stride=X.LOCALMAP_MAX_STRIDE + 1),
           dict(kp_stride=-1),
           dict(n_best=0), dict(n_best=X.LOCALMAP_MAX_BEST + 1), dict(n_table=-1), dict(n_table=262144 + 1), dict(n_kp=-1),
           dict(n_kp=101), dict(point_cap=0), dict(point_cap=8193), dict(point_cap=49), dict(max_keyframes=-1),
           dict(d_kf_mp_of_kp=None), dict(d_kf_flags=None), dict(d_best_cov=None), dict(d_parent=None), dict(d_mp_flags=None),
           dict(d_mp_of_kp=None), dict(d_out=None), dict(d_kf_mp_of_kp=P["kf_mp_of_kp"] + 2), dict(d_parent=P["parent"] + 1),
           dict(d_mp_of_kp=P["mp_of_kp"] + 3), dict(d_out=d_out.data_ptr() + 4)]
    for over in bad:
        with pytest.raises(SpfeError):
            ext.update_local_map_resident(**args(**over))
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == FILL).all(), "a refused call wrote"
    # the count form and the rows form
    count = dict(d_kf_mp_of_kp=P["kf_mp_of_kp"], kp_stride=stride, n_slots=n, d_mp_flags=P["mp_flags"], n_table=300,
                 d_mp_of_kp=P["mp_of_kp"], d_outlier=None, n_kp=50, d_votes=d_v.data_ptr(), d_total=d_t.data_ptr())
    for over in (dict(n_slots=0), dict(kp_stride=0), dict(n_table=-1), dict(n_kp=8193), dict(d_votes=None), dict(d_total=None),
                 dict(d_kf_mp_of_kp=None), dict(d_mp_flags=None), dict(d_mp_of_kp=None), dict(d_votes=d_v.data_ptr() + 2)):
        with pytest.raises(SpfeError):
            ext.count_shared_points_resident(**dict(count, **over))
    rows = dict(d_point_idx=P["parent"], point_cap=20, d_mp_of_kp_list=P["mp_of_kp"], n_kp=50, d_mp_of_kp_rows=d_v.data_ptr())
    for over in (dict(point_cap=0), dict(point_cap=8193), dict(n_kp=-1), dict(n_kp=8193), dict(d_point_idx=None),
                 dict(d_mp_of_kp_list=None), dict(d_mp_of_kp_rows=None), dict(d_mp_of_kp_rows=d_v.data_ptr() + 1)):
        with pytest.raises(SpfeError):
            ext.local_map_rows_resident(**dict(rows, **over))
    torch.cuda.synchronize()
    assert (d_v.cpu().numpy() == -7).all() and (d_t.cpu().numpy() == -7).all(), "a refused call wrote"
    # null arrays of no entries
    ext.update_local_map_resident(**args(d_mp_of_kp=None, n_kp=0, d_mp_flags=None, n_table=0))
    torch.cuda.synchronize()
    g = X.SPExtractor.decode_localmap_out(d_out.cpu().numpy(), n, 100, 0)
    assert g["status"] == X.LOCALMAP_NO_VOTES and g["n_points"] == 0 and (g["point_idx"] == -1).all()
    # the host form
    out = np.full(nb, FILL, np.uint8)
    for over in (dict(point_cap=49), dict(point_cap=8193), dict(max_keyframes=-1)):
        kw = dict(point_cap=100, max_keyframes=80)
        kw.update(over)
        with pytest.raises(SpfeError):
            ext.update_local_map(a["kf_mp_of_kp"], a["kf_flags"], a["best_cov"], a["parent"], a["mp_flags"], a["mp_of_kp"], out=out, **kw)
    with pytest.raises(SpfeError):
        ext.update_local_map(a["kf_mp_of_kp"], a["kf_flags"], a["best_cov"][:, :0], a["parent"], a["mp_flags"], a["mp_of_kp"], 100, out=out)
    assert (out == FILL).all()
