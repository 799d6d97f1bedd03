"""GPU: the map-point table on the device (spfe_refresh_map_points_device, spfe_refresh_map_points,
spfe_gather_map_points_device: mappoint.hip) against the host reference tests/mp_ref/mp_ref.c, which shares
include/spfe_mappoint_math.h with the kernels: the whole output block and normal, dist_range and desc at the listed rows bit for
bit, every other table row and every byte the block does not name still holding the poison — on the fixtures
tests/golden/mp_*.npz laid out as records with f32 and with bf16 descriptor rows, and the host form on the same data; the
observation counts at the median's small cases, at the wavefront's edges, either side of the wavefront / workgroup boundary
and of the LDS staging capacity of both row formats, at SPFE_MP_MAX_OBS and beyond; ties and NaN rows on the workgroup path;
the list shapes around the chunk of points a workgroup serves; a mixed list against its points served one by one; the gather
against numpy indexing and as the point list of the fuse search; the chain extract -> bundle adjustment -> refresh on one
stream; the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("mp_ref", "fuse_ref", ""):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
import fuse_cases as fc  # noqa: E402
import mp_cases  # noqa: E402
import mp_ref  # noqa: E402
import test_gpu_fuse as tgf  # noqa: E402  (its target and point helpers)
import test_gpu_local_ba as tlb  # noqa: E402
from test_gpu_local_ba import S  # noqa: E402,F401  (its scene fixture: six extracted frames and a bundle-adjustment problem)

from sp_orb_slam_amd import extractor as X  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import SPExtractor, SpfeError  # noqa: E402

pytestmark = pytest.mark.gpu
H, W, NF = 64, 96, 100          # kmax = 101 rows a record
FILL = mp_ref.FILL
TABLE = ("normal", "dist_range", "desc")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return mp_ref.build(tmp_path_factory.mktemp("mp_ref"))


@pytest.fixture(scope="module")
def exts():
    blob = weights.synthetic(7, "trackable")
    e = {False: SPExtractor(NF, H, W, blob, with_heat=False), True: SPExtractor(NF, H, W, blob, with_heat=False, desc_bf16=True)}
    yield e
    for x in e.values():
        x.close()


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.reshape(-1).view(np.uint8).copy() if a.size else np.zeros(16, np.uint8)).cuda()


def records(ext, c):
    """the keyframes of case c as records of the handle's layout -> (device buffer, int64 record pointers, 0 where there is none)"""
    L, rb, n_kf = ext.layout, ext.record_bytes(), len(c["kf_flags"])
    rows = c["kf_desc"].shape[1]
    assert rows <= L.kmax
    raw = np.zeros((n_kf, rb), np.uint8)
    for k in range(n_kf):
        K = int(c["kf_K"][k])
        raw[k, L.off_hdr:L.off_hdr + 16].view(np.int32)[:] = [max(K, 0), max(K, 0), int(c["kf_status"][k]), 0]
        if ext.desc_bf16:
            raw[k, L.off_desc:L.off_desc + 512 * rows].view(np.uint16)[:] = mp_ref.to_bf16(c["kf_desc"][k]).reshape(-1)
        else:
            raw[k, L.off_desc:L.off_desc + 1024 * rows].view(np.float32)[:] = c["kf_desc"][k].reshape(-1)
    d = dev(raw)
    return d, np.array([d.data_ptr() + k * rb if c["kf_K"][k] >= 0 else 0 for k in range(n_kf)], np.int64)


def run_record(ext, c, mode=None):
    """spfe_refresh_map_points_device on a poisoned table and block -> dict like mp_ref.refresh's"""
    import torch
    m, E, n_table, n_kf = len(c["ref_slot"]), len(c["obs"]), len(c["xyz"]), len(c["kf_flags"])
    d_rec, ptrs = records(ext, c)
    d = {k: dev(c[k]) for k in ("kf_flags", "Tcw", "obs_start", "obs", "ref_slot", "xyz", "flags")}
    d["ptrs"] = dev(ptrs)
    d["pi"] = None if c.get("point_idx") is None else dev(np.asarray(c["point_idx"], np.int32))
    tab = {k: dev(v) for k, v in zip(TABLE, mp_ref.poisoned_table(n_table))}
    d_out = torch.full((ext.mp_out_bytes(m),), FILL, dtype=torch.uint8, device="cuda")
    before = {k: v.clone() for k, v in d.items() if v is not None}
    ext.refresh_map_points_device(d["ptrs"].data_ptr(), d["kf_flags"].data_ptr(), d["Tcw"].data_ptr(), n_kf,
                                  None if d["pi"] is None else d["pi"].data_ptr(), d["obs_start"].data_ptr(), d["obs"].data_ptr(),
                                  d["ref_slot"].data_ptr(), m, E, d["xyz"].data_ptr(), d["flags"].data_ptr(), tab["normal"].data_ptr(),
                                  tab["dist_range"].data_ptr(), tab["desc"].data_ptr(), n_table, d_out.data_ptr(),
                                  mode=int(c["mode"]) if mode is None else mode, level_scale=float(c["level_scale"]),
                                  top_scale=float(c["top_scale"]))
    torch.cuda.synchronize()
    assert all(torch.equal(d[k], before[k]) for k in before)
    block = d_out.cpu().numpy()
    out = dict(X.SPExtractor.decode_mp_out(block, m), block=block)
    for k, w in zip(TABLE, (3, 2, 256)):
        out[k] = tab[k].cpu().numpy().view(np.float32)[:n_table * w].reshape(n_table, w)
    del d_rec                                                                # (alive until here: the pointer table names it)
    return out


def run_host(ext, L, c, mode=None):
    """spfe_refresh_map_points on the observations of case c gathered by the host, poisoned outputs"""
    hi = mp_cases.host_inputs(L, c)
    m = len(c["ref_slot"])
    normal, dist_range, desc = mp_ref.poisoned_table(m)
    block = ext.refresh_map_points(hi["obs_start"], hi["obs_desc"], hi["obs_good"], hi["obs_Ow"], hi["ref_Ow"], hi["xyz"], hi["flags"],
                                   normal, dist_range, desc, mode=int(c["mode"]) if mode is None else mode,
                                   level_scale=float(c["level_scale"]), top_scale=float(c["top_scale"]), fill=FILL)
    return dict(X.SPExtractor.decode_mp_out(block, m), block=block, normal=normal, dist_range=dist_range, desc=desc)


def same(got, want, what, status=True):
    """the block (padding and all) and the three table arrays (unlisted rows and all), byte for byte"""
    for k in ("code", "n_good", "best_obs"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    assert np.array_equal(got["best_median"].view(np.uint32), want["best_median"].view(np.uint32)), (what, "best_median bits")
    for k in TABLE:
        assert got[k].tobytes() == want[k].tobytes(), (what, k)
    if status:
        assert got["block"].tobytes() == want["block"].tobytes(), (what, "block", got["block"][:16].view(np.int32), want["block"][:16].view(np.int32))
    else:   # the host form knows no records: status 0
        assert got["block"][:12].tobytes() == want["block"][:12].tobytes() and got["status"] == 0
        assert got["block"][16:].tobytes() == want["block"][16:].tobytes(), what


def hostable(c, want):
    return c.get("point_idx") is None and not (want["code"] == mp_ref.INVALID).any()


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", sorted(mp_cases.CASES))
def test_fixtures_equal_the_host_reference_bit_for_bit(exts, ref, name, bf16):
    """Every named case — the small counts, the ties, the NaN rows, one case per code, every kind of INVALID, each mode bit
    alone, point_idx permuted and with a duplicate — in the record form with both row formats and in the host form."""
    c, rec = mp_cases.load(name)
    want = mp_ref.refresh(ref, c)
    assert mp_cases.differences(rec, want) == []
    same(run_record(exts[bf16], c), want, (name, "record form"))
    if hostable(c, want):
        same(run_host(exts[bf16], ref, c), want, (name, "host form"), status=False)


def distinct_obs(c, N, rng):
    """N different (slot, keypoint) pairs of the good keyframes"""
    good = c.good_slots()
    pick = rng.permutation(len(good) * c.K)[:N]
    return [(good[int(p) // c.K], int(p) % c.K) for p in pick]


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_observation_counts_at_every_edge(exts, ref, bf16):
    """N = 1 .. 5 (the median's small cases), 63 / 64 / 65 (one register of distances, and the second), the wavefront /
    workgroup boundary - 1, 0, + 1, the staging capacity of f32 rows and of bf16 rows - 1, 0, + 1 (both handles run all of them:
    each sees its own capacity as the path switch and the other's as a plain count), 256, and 257: TOO_MANY."""
    ext = exts[bf16]
    cap4, cap2, wv = ext.mp_lds_obs_capacity(4), ext.mp_lds_obs_capacity(2), X.MP_WAVE_OBS
    assert ext.mp_lds_obs_capacity() == (cap2 if bf16 else cap4) and cap2 == 2 * cap4 and wv < cap4 and cap2 < X.MP_MAX_OBS
    counts = [1, 2, 3, 4, 5, 63, 64, 65, wv - 1, wv, wv + 1, cap4 - 1, cap4, cap4 + 1, cap2 - 1, cap2, cap2 + 1, 256, 257]
    c = mp_cases.Case(11, n_kf=6, K=65)
    rng = np.random.default_rng(110)
    for N in counts:
        c.point(distinct_obs(c, N, rng))
    a = c.arrays()
    want = mp_ref.refresh(ref, a)
    assert list(want["n_good"]) == counts and list(want["code"]) == [mp_ref.REFRESHED] * 18 + [mp_ref.TOO_MANY]
    assert len(set(want["best_obs"][5:18])) > 6                              # (the choice is not trivial)
    same(run_record(ext, a), want, "counts")
    same(run_host(ext, ref, a), want, "counts, host form", status=False)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_ties_and_nan_rows_on_the_workgroup_path(exts, ref, bf16):
    """Beyond SPFE_MP_WAVE_OBS rows the four wavefronts share the rows and merge their bests: duplicate rows (the first
    wins), all rows identical, equal medians in rows that different wavefronts own, a NaN row first and in the middle, all rows
    NaN — staged in LDS and, for f32 rows, beyond the staging capacity too."""
    ext = exts[bf16]
    c = mp_cases.Case(12, n_kf=6, K=65)
    r = c.rng.normal(size=(60, 256)) / 16.0
    c.point_n(20, rows=np.concatenate([r[:10], r[:10]]))                    # every row twice: all medians tie in pairs
    c.point_n(50, rows=np.tile(r[10], (50, 1)))                              # all identical
    e = np.zeros((44, 256))
    e[np.arange(44), np.arange(44) % 4] = np.where(np.arange(44) % 8 < 4, 3.0, -3.0)   # eight rows, each five or six times
    c.point_n(44, rows=e)
    n = r[:30].copy()
    n[0, 3] = n[13, 200] = np.nan
    c.point_n(30, rows=n)
    c.point_n(45, rows=np.full((45, 256), np.nan))
    a = c.arrays()
    want = mp_ref.refresh(ref, a)
    assert want["best_obs"][0] < 10 and list(want["best_obs"][[1, 4]]) == [0, 0] and want["best_median"][4] == np.finfo(np.float32).max
    assert want["best_obs"][3] not in (0, 13) and want["best_median"][1] == 0 and want["best_median"][2] > 0
    same(run_record(ext, a), want, "ties")
    same(run_host(ext, ref, a), want, "ties, host form", status=False)


def mixed_case(seed=13):
    """all codes and all sizes; keyframe 5 is bad, keyframe 6 is bad and has no record"""
    c = mp_cases.Case(seed, n_kf=7, K=65, bad=(5, 6), null=(6,), status=(0, 0, 4, 0, 0, 2, 8))
    rng = np.random.default_rng(seed + 100)
    c.point_n(3, flags=0)
    c.point([])
    c.point([(0, 1), (7, 0)])
    c.point([(5, 2), (6, 0)], ref=6)
    c.point(distinct_obs(c, 257, rng))
    for N in (1, 3, 17, 41, 81, 100):
        c.point(distinct_obs(c, N, rng))
    c.point_n(6, bad_obs=3)
    c.point_n(20, bad_obs=2)
    return c


def test_a_mixed_list_equals_its_points_served_one_by_one(exts, ref):
    ext = exts[False]
    a = mixed_case().arrays()
    want = mp_ref.refresh(ref, a)
    assert sorted(set(want["code"])) == [1, 2, 3, 4, 5, 6] and want["status"] == (4 | 2)      # (the record-less keyframe has no status)
    got = run_record(ext, a)
    same(got, want, "mixed")
    for i in range(len(a["ref_slot"])):
        one = run_record(ext, mp_cases.subcase(a, [i]))
        for k in ("code", "n_good", "best_obs"):
            assert one[k][0] == got[k][i], (i, k)
        assert one["best_median"].view(np.uint32)[0] == got["best_median"].view(np.uint32)[i]
        for k in TABLE:
            assert one[k][i].tobytes() == got[k][i].tobytes(), (i, k)
            assert np.delete(one[k], i, 0).tobytes() == np.delete(mp_ref.poisoned_table(len(a["xyz"]))[TABLE.index(k)], i, 0).tobytes()


@pytest.mark.parametrize("mode", [3, X.MP_DESC, X.MP_NORMAL_DEPTH])
def test_host_form_with_bad_keyframes(exts, ref, mode):
    """obs_good = 0 rows are skipped in the descriptor and counted in the normal; every code the host form has"""
    c = mp_cases.Case(17, n_kf=7, K=65, bad=(5, 6), null=(6,))
    rng = np.random.default_rng(170)
    c.point_n(3, flags=0)
    c.point([])
    c.point([(5, 2), (6, 0)], ref=6)
    c.point(distinct_obs(c, 257, rng))
    c.point_n(3, bad_obs=2)
    c.point_n(20, bad_obs=3)
    c.point_n(1, bad_obs=1)
    a = c.arrays()
    want = mp_ref.refresh(ref, a, mode=mode)
    assert list(want["code"][:4]) == ([1, 2, 4, 5] if mode & 1 else [1, 2, 6, 6]) and list(want["n_good"][4:]) == [3, 20, 1]
    same(run_host(exts[False], ref, a, mode=mode), want, mode, status=False)
    same(run_record(exts[True], a, mode=mode), want, mode)


@pytest.mark.parametrize("m", [0, 1, X.MP_CHUNK - 1, X.MP_CHUNK, X.MP_CHUNK + 1, 2 * X.MP_CHUNK + 1])
def test_list_lengths_around_the_chunk(exts, ref, m):
    """no point, one, one less than the chunk a workgroup serves, a chunk, one more (a second workgroup with one point), and
    a third workgroup; wavefront-path and workgroup-path points alternate, so every wavefront of a chunk meets both"""
    ext = exts[True]
    c = mp_cases.Case(14, n_kf=6, K=65)
    rng = np.random.default_rng(140)
    for i in range(m):
        c.point(distinct_obs(c, (2, 19, 5, 1, 33, 16, 17, 3)[i % 8], rng))
    a = c.arrays()
    want = mp_ref.refresh(ref, a)
    assert want["m"] == m and want["n_desc_written"] == m
    same(run_record(ext, a), want, m)
    same(run_host(ext, ref, a), want, (m, "host form"), status=False)


def test_each_mode_bit_alone_on_the_workgroup_path(exts, ref):
    ext = exts[False]
    a = mixed_case(15).arrays()
    for mode in (X.MP_DESC, X.MP_NORMAL_DEPTH):
        want = mp_ref.refresh(ref, a, mode=mode)
        got = run_record(ext, a, mode=mode)
        same(got, want, mode)
        poison = mp_ref.poisoned_table(len(a["xyz"]))
        if mode == X.MP_DESC:
            assert got["normal"].tobytes() == poison[0].tobytes() and got["dist_range"].tobytes() == poison[1].tobytes()
            assert got["n_nd_written"] == 0 and got["n_desc_written"] > 5
        else:
            assert got["desc"].tobytes() == poison[2].tobytes() and got["n_desc_written"] == 0 and (got["best_obs"] == -1).all()
            assert list(got["code"][:5]) == [1, 2, 3, 6, 6]


def test_gather_equals_numpy_indexing_and_feeds_the_fuse_search(exts):
    import torch
    ext = exts[False]
    rng = np.random.default_rng(16)
    t = tgf.big_target()
    intr = (120.0, 120.0, 47.5, 31.25)
    p = tgf.points_on(t, 40, 17, intr)
    n_table = 50
    perm = rng.permutation(n_table)[:40].astype(np.int32)
    tab = dict(xyz=rng.normal(size=(n_table, 3)).astype(np.float32), normal=rng.normal(size=(n_table, 3)).astype(np.float32),
               dist_range=rng.random((n_table, 2)).astype(np.float32), desc=rng.normal(size=(n_table, 256)).astype(np.float32),
               flags=rng.integers(0, 4, n_table).astype(np.uint8))
    for k in tab:
        tab[k][perm] = p[k]
    d_tab = {k: dev(v) for k, v in tab.items()}

    def gather(idx):
        n = len(idx)
        d_idx = dev(idx)
        outs = dict(point_id=4 * n, xyz=12 * n, normal=12 * n, dist_range=8 * n, desc=1024 * n, flags=n)
        d_o = {k: torch.full((max(b, 16),), FILL, dtype=torch.uint8, device="cuda") for k, b in outs.items()}
        ext.gather_map_points_device(d_idx.data_ptr(), n, d_tab["xyz"].data_ptr(), d_tab["flags"].data_ptr(), d_tab["normal"].data_ptr(),
                                     d_tab["dist_range"].data_ptr(), d_tab["desc"].data_ptr(), n_table,
                                     *[d_o[k].data_ptr() for k in fc.POINT_KEYS])
        torch.cuda.synchronize()
        host = {k: d_o[k].cpu().numpy() for k in outs}
        assert all((host[k][b:] == FILL).all() for k, b in outs.items())
        return d_o, {k: host[k][:b] for k, b in outs.items()}

    # numpy indexing, repeats and all; an index outside the table gives a row of zeros under its own id
    idx = np.concatenate([rng.integers(0, n_table, 70), [-1, n_table, 2 ** 31 - 1, -2 ** 31, 0, n_table - 1]]).astype(np.int32)
    ok = (idx >= 0) & (idx < n_table)
    _, g = gather(idx)
    assert np.array_equal(g["point_id"].view(np.int32), idx)
    assert np.array_equal(g["flags"], np.where(ok, tab["flags"][np.clip(idx, 0, n_table - 1)], 0))
    for k in ("xyz", "normal", "dist_range", "desc"):
        want = np.where(ok[:, None], tab[k][np.clip(idx, 0, n_table - 1)], np.float32(0))
        assert g[k].tobytes() == want.astype(np.float32).tobytes(), k
    assert gather(np.zeros(0, np.int32))[1]["flags"].size == 0
    # the gathered list as the point list of the fuse search: the block of the same list uploaded from the host
    d_list, g = gather(perm)
    up = dict(p, point_id=perm)
    assert all(g[k].tobytes() == np.ascontiguousarray(up[k]).tobytes() for k in fc.POINT_KEYS)
    d_rec, mp = tgf.record(ext, t), tgf.padded(ext, t["kf_mp"])
    a, raw_a = tgf.one_target(ext, d_rec, mp, t["Tcw"], d_list, 40, intr)
    b, raw_b = tgf.one_target(ext, d_rec, mp, t["Tcw"], tgf.dev_points(up), 40, intr)
    assert raw_a.tobytes() == raw_b.tobytes() and a["n_fused"] > 5


def test_chain_extract_bundle_adjustment_refresh_on_one_stream(S, ref):  # noqa: F811
    """spfe_local_ba_records_device and the refresh with SPFE_MP_NORMAL_DEPTH back to back on the handle's stream, no host
    synchronisation in between: the refresh reads Tcw_out and xyz_out inside the bundle adjustment's block, where it wrote them.
    Against the same two steps with host copies in between, and against mp_ref.c; then both parts on the extracted rows."""
    import torch
    e, n_kf, n, E = S.ext, len(S.Tcw), len(S.xyz), len(S.edges)
    o = X.ba_offsets(n_kf, n, E)
    start = np.searchsorted(S.edges[:, 0], np.arange(n + 1)).astype(np.int32)
    assert (np.diff(S.edges[:, 0]) >= 0).all() and start[-1] == E
    obs = np.ascontiguousarray(S.edges[:, 1:3])
    ref_slot = obs[np.minimum(start[:-1], E - 1), 0].astype(np.int32)
    ptrs = np.array([S.d_recs.data_ptr() + f * S.rb for f in range(n_kf)], np.int64)
    d = {k: dev(v) for k, v in dict(edges=S.edges, Tcw=S.Tcw, fixed=S.fixed, xyz=S.xyz, ptrs=ptrs, kf_flags=np.zeros(n_kf, np.uint8),
                                    start=start, obs=obs, ref_slot=ref_slot, flags=np.ones(n, np.uint8)).items()}

    def refresh(d_Tcw, d_xyz, mode):
        tab = {k: dev(v) for k, v in zip(TABLE, mp_ref.poisoned_table(n))}
        d_out = torch.full((e.mp_out_bytes(n),), FILL, dtype=torch.uint8, device="cuda")
        e.refresh_map_points_device(d["ptrs"].data_ptr(), d["kf_flags"].data_ptr(), d_Tcw, n_kf, None, d["start"].data_ptr(),
                                    d["obs"].data_ptr(), d["ref_slot"].data_ptr(), n, E, d_xyz, d["flags"].data_ptr(),
                                    tab["normal"].data_ptr(), tab["dist_range"].data_ptr(), tab["desc"].data_ptr(), n, d_out.data_ptr(),
                                    mode=mode)
        return tab, d_out

    def fetch(tab, d_out):
        torch.cuda.synchronize()
        out = dict(block=d_out.cpu().numpy())
        for k, w in zip(TABLE, (3, 2, 256)):
            out[k] = tab[k].cpu().numpy().view(np.float32)[:n * w].reshape(n, w)
        return dict(out, **X.SPExtractor.decode_mp_out(out["block"], n))

    d_ba = torch.full((o["bytes"],), 0x5A, dtype=torch.uint8, device="cuda")
    e.local_ba_records_device([int(p) for p in ptrs], d["edges"].data_ptr(), E, d["Tcw"].data_ptr(), d["fixed"].data_ptr(),
                              d["xyz"].data_ptr(), n, d_ba.data_ptr(), tlb.INTR)
    chained = fetch(*refresh(d_ba.data_ptr() + o["tcw"], d_ba.data_ptr() + o["xyz"], X.MP_NORMAL_DEPTH))
    g = X.SPExtractor.decode_ba_out(d_ba.cpu().numpy(), n_kf, n, E)
    assert g["status"] == 0 and g["iterations"][0] > 0 and g["xyz_out"].tobytes() != S.xyz.tobytes()
    d_T2, d_x2 = dev(g["Tcw_out"]), dev(g["xyz_out"])                         # the host copies in between
    copied = fetch(*refresh(d_T2.data_ptr(), d_x2.data_ptr(), X.MP_NORMAL_DEPTH))
    kf_desc = np.zeros((n_kf, e.layout.kmax, 256), np.float32)
    for f in range(n_kf):
        kf_desc[f, :S.recs[f].K] = S.recs[f].descriptors[:S.recs[f].K]
    c = dict(kf_flags=np.zeros(n_kf, np.uint8), kf_K=np.array([r.K for r in S.recs], np.int32), kf_status=np.zeros(n_kf, np.int32),
             Tcw=g["Tcw_out"], kf_desc=kf_desc, point_idx=None, obs_start=start, obs=obs, ref_slot=ref_slot, xyz=g["xyz_out"],
             flags=np.ones(n, np.uint8), mode=X.MP_NORMAL_DEPTH, level_scale=1.0, top_scale=1.0)
    want = mp_ref.refresh(ref, c)
    assert want["n_nd_written"] == n and (want["code"] == mp_ref.REFRESHED).all()
    same(chained, want, "chained")
    same(copied, want, "host copies in between")
    both = fetch(*refresh(d_T2.data_ptr(), d_x2.data_ptr(), X.MP_DESC | X.MP_NORMAL_DEPTH))
    want = mp_ref.refresh(ref, c, mode=3)
    assert want["n_desc_written"] == n and want["n_good"].max() >= 4
    same(both, want, "both parts on extracted rows")


def test_refusals_leave_the_outputs_untouched(exts, ref):
    import torch
    ext = exts[False]
    c, _ = mp_cases.load("counts")
    m, E, n_kf = len(c["ref_slot"]), len(c["obs"]), len(c["kf_flags"])
    d_rec, ptrs = records(ext, c)
    d = {k: dev(c[k]) for k in ("kf_flags", "Tcw", "obs_start", "obs", "ref_slot", "xyz", "flags")}
    d["ptrs"] = dev(ptrs)
    tab = {k: dev(v) for k, v in zip(TABLE, mp_ref.poisoned_table(m))}
    d_out = torch.full((ext.mp_out_bytes(m),), FILL, dtype=torch.uint8, device="cuda")
    ok = dict(d_kf_records=d["ptrs"].data_ptr(), d_kf_flags=d["kf_flags"].data_ptr(), d_Tcw=d["Tcw"].data_ptr(), n_kf=n_kf, d_point_idx=None,
              d_obs_start=d["obs_start"].data_ptr(), d_obs=d["obs"].data_ptr(), d_ref_slot=d["ref_slot"].data_ptr(), m=m, E=E,
              d_xyz=d["xyz"].data_ptr(), d_flags=d["flags"].data_ptr(), d_normal=tab["normal"].data_ptr(),
              d_dist_range=tab["dist_range"].data_ptr(), d_desc=tab["desc"].data_ptr(), n_table=m, d_out=d_out.data_ptr())
    bads = [dict(m=X.MP_MAX_POINTS + 1), dict(E=X.MP_MAX_EDGES + 1), dict(n_kf=0), dict(m=-1), dict(E=-1), dict(n_table=-1), dict(mode=0),
            dict(mode=4), dict(mode=7)] + [{k: None} for k in ok if k.startswith("d_") and k != "d_point_idx"]
    for bad in bads:
        with pytest.raises(SpfeError):
            ext.refresh_map_points_device(**dict(ok, **bad))
    torch.cuda.synchronize()
    assert bool((d_out == FILL).all()) and all(bool((tab[k] == FILL).all()) for k in TABLE)
    # the gather
    lst = {k: torch.full((4096,), FILL, dtype=torch.uint8, device="cuda") for k in fc.POINT_KEYS}
    gok = [d["ref_slot"].data_ptr(), 3, d["xyz"].data_ptr(), d["flags"].data_ptr(), tab["normal"].data_ptr(), tab["dist_range"].data_ptr(),
           tab["desc"].data_ptr(), m] + [lst[k].data_ptr() for k in fc.POINT_KEYS]
    for i, v in [(1, X.MP_MAX_POINTS + 1), (1, -1), (7, -1)] + [(i, None) for i in (0, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13)]:
        args = list(gok)
        args[i] = v
        with pytest.raises(SpfeError):
            ext.gather_map_points_device(*args)
    torch.cuda.synchronize()
    assert all(bool((lst[k] == FILL).all()) for k in lst)
    # the host form, straight at the C ABI: limits + 1, a bad mode, every null argument
    hi = mp_cases.host_inputs(ref, c)
    normal, dist_range, desc = mp_ref.poisoned_table(m)
    out = np.full(ext.mp_out_bytes(m), FILL, np.uint8)
    p = lambda v: np.ascontiguousarray(v).ctypes.data   # noqa: E731
    hi = {k: np.ascontiguousarray(v) for k, v in hi.items()}
    prm = X.MpParams(3, 1.0, 1.0)
    full = [ext._h, p(hi["obs_start"]), p(hi["obs_desc"]), p(hi["obs_good"]), p(hi["obs_Ow"]), E, p(hi["ref_Ow"]), p(hi["xyz"]),
            p(hi["flags"]), m, C.byref(prm), p(normal), p(dist_range), p(desc), p(out)]
    for i, v in [(5, X.MP_MAX_EDGES + 1), (9, X.MP_MAX_POINTS + 1), (5, -1), (9, -1), (10, C.byref(X.MpParams(8, 1.0, 1.0))),
                 (10, C.byref(X.MpParams(0, 1.0, 1.0)))] + [(i, None) for i in (0, 1, 2, 3, 4, 6, 7, 8, 10, 11, 12, 13, 14)]:
        args = list(full)
        args[i] = v
        assert ext._lib.spfe_refresh_map_points(*args) != 0, i
    poison = mp_ref.poisoned_table(m)
    assert (out == FILL).all() and all(a.tobytes() == b.tobytes() for a, b in zip((normal, dist_range, desc), poison))
    with pytest.raises(SpfeError):
        ext.mp_lds_obs_capacity(3)
    del d_rec                                                                # (alive until here: the pointer table names it)
