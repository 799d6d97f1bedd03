"""GPU: SPMatcher::SearchByBruteForce(KeyFrame *, KeyFrame *) on resident records (spfe_loop_match_record_device: the
cross-check of match.hip with a mask on BOTH sides) against spfe_match on the rows of both sides compacted on the host, every
row keeping its keypoint index — with f32 and with bf16 descriptor rows; an empty side, one held row, every row held, masks
that differ per side, exact ties; and at 1300 keypoints (21 x 21 tiles of the masked matcher, six steps of the inversion's
stride loops) three candidates of 1300, 1100 and 700 rows against the CPU oracle's cross-check match on the compacted rows,
then the chain spfe_loop_verify_records_device against the single forms byte for byte."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tri_ref"))
import tri_ref  # noqa: E402  (to_bf16 / widen_bf16)

from oracle import oracle  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import SPExtractor  # noqa: E402

pytestmark = pytest.mark.gpu
H, W, NF = 64, 96, 100          # kmax = 101
FILL = 0x5A


@pytest.fixture(scope="module")
def exts():
    blob = weights.synthetic(7, "trackable")
    e = {False: SPExtractor(NF, H, W, blob, with_heat=False), True: SPExtractor(NF, H, W, blob, with_heat=False, desc_bf16=True)}
    yield e
    for x in e.values():
        x.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def record(ext, desc, status=0):
    L = ext.layout
    K = len(desc)
    b = np.zeros(ext.record_bytes(), np.uint8)
    b[L.off_hdr:L.off_hdr + 16].view(np.int32)[:] = [K, K, status, 0]
    if ext.desc_bf16:
        b[L.off_desc:L.off_desc + 512 * K].view(np.uint16)[:] = tri_ref.to_bf16(desc).reshape(-1)
    else:
        b[L.off_desc:L.off_desc + 1024 * K].view(np.float32)[:] = np.ascontiguousarray(desc, np.float32).reshape(-1)
    return dev(b)


def rows(seed, K1, K2):
    """two sets of unit rows, most of set 2 noisy copies of rows of set 1; values exact in bf16"""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(K1, 256))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    src = rng.integers(0, K1, K2)
    b = a[src] + 0.05 * rng.normal(size=(K2, 256))
    b[rng.random(K2) < 0.2] = rng.normal(size=256) / 16
    q = lambda v: tri_ref.widen_bf16(tri_ref.to_bf16(v.astype(np.float32))).reshape(v.shape)   # noqa: E731
    return q(a), q(b)


def loop_match(ext, d1, d2, mp1, mp2):
    import torch
    kmax = ext.layout.kmax
    m1, m2 = np.full(kmax, -1, np.int32), np.full(kmax, -1, np.int32)
    m1[:len(mp1)], m2[:len(mp2)] = mp1, mp2
    d_m1, d_m2 = dev(m1), dev(m2)
    d_out = torch.full((4 * kmax + 8,), FILL, dtype=torch.uint8, device="cuda")
    ext.loop_match_record_device(d1.data_ptr(), d2.data_ptr(), d_m1.data_ptr(), d_m2.data_ptr(), d_out.data_ptr(),
                                 d_out.data_ptr() + 4 * kmax)
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    assert (raw[4 * kmax + 4:] == FILL).all()
    return raw[:4 * kmax].view(np.int32).copy(), int(raw[4 * kmax:4 * kmax + 4].view(np.int32)[0])


def compacted(ext_f32, desc1, desc2, mp1, mp2, kmax):
    """spfe_match on the held rows of both sides (queries = keyframe 2's, train = keyframe 1's), mapped back"""
    i1, i2 = np.flatnonzero(mp1 >= 0), np.flatnonzero(mp2 >= 0)
    want = np.full(kmax, -1, np.int32)
    if len(i1) and len(i2):
        idx, _ = ext_f32.match(desc2[i2], desc1[i1], cross_check=True)
        for q, t in enumerate(idx):
            if t >= 0:
                want[i1[t]] = i2[q]
    return want, int((want >= 0).sum())


MASKS = {
    "empty_train": lambda rng, K1, K2: (np.full(K1, -1), rng.integers(0, 50, K2)),
    "empty_query": lambda rng, K1, K2: (rng.integers(0, 50, K1), np.full(K2, -1)),
    "one_row_each": lambda rng, K1, K2: (np.where(np.arange(K1) == 37, 5, -1), np.where(np.arange(K2) == 11, 9, -1)),
    "all_held": lambda rng, K1, K2: (np.arange(K1), np.arange(K2) + 100),
    "different_masks": lambda rng, K1, K2: (np.where(rng.random(K1) < 0.7, rng.integers(0, 900, K1), -1),
                                            np.where(rng.random(K2) < 0.4, rng.integers(0, 900, K2), -3)),
}


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("mask", list(MASKS))
def test_masked_match_equals_spfe_match_on_compacted_rows(exts, mask, bf16):
    ext = exts[bf16]
    kmax = ext.layout.kmax
    K1, K2 = 97, 66                        # more than one 64-row tile on either side, neither a multiple of the tile
    d1, d2 = rows(3, K1, K2)
    d2[40] = d2[7]                         # an exact tie between two queries: the order decides
    d1[90] = d1[13]                        # ... and between two train rows
    mp1, mp2 = [np.asarray(v, np.int32) for v in MASKS[mask](np.random.default_rng(5), K1, K2)]
    got, n = loop_match(ext, record(ext, d1), record(ext, d2), mp1, mp2)
    want, n_want = compacted(exts[False], d1, d2, mp1, mp2, kmax)
    assert np.array_equal(got, want), (mask, np.flatnonzero(got != want))
    assert n == n_want
    if mask.startswith("empty"):
        assert n == 0
    if mask == "all_held":
        assert n > 30
    held2 = set(np.flatnonzero(mp2 >= 0).tolist())
    assert all(int(k2) in held2 for k2 in got[got >= 0]) and (got[:K1][mp1 < 0] == -1).all() and (got[K1:] == -1).all()


def test_overflowed_records_are_matched(exts):
    """SPFE_STATUS_COV_OVERFLOW says that the covariances are not valid; the match reads none"""
    ext = exts[False]
    d1, d2 = rows(4, 50, 70)
    mp1, mp2 = np.arange(50, dtype=np.int32), np.arange(70, dtype=np.int32)
    clean = loop_match(ext, record(ext, d1), record(ext, d2), mp1, mp2)
    over = loop_match(ext, record(ext, d1, status=1), record(ext, d2, status=1), mp1, mp2)
    assert np.array_equal(clean[0], over[0]) and clean[1] == over[1] > 20


# ---- 1300 keypoints ----------------------------------------------------------------------------------------------------------
NF_LARGE, ROWS = 1300, (1300, 1100, 700)
INTR = (118.5, 117.25, 47.5, 31.25)


@pytest.fixture(scope="module")
def large_exts():
    made = {}

    def get(bf16):
        if bf16 not in made:
            made[bf16] = SPExtractor(NF_LARGE, H, W, weights.synthetic(7, "trackable"), with_heat=False, desc_bf16=bf16)
            assert made[bf16].layout.kmax == NF_LARGE + 1
        return made[bf16]
    yield get
    for x in made.values():
        x.close()


@pytest.fixture(scope="module")
def large():
    """keyframe 1 (1300 unit rows) and three candidates whose rows lie 0.05 from a row of keyframe 1 (one in five: unrelated),
    all values exact in bf16; holders on both sides into a map of 2000 points, candidate 1 with a dozen held rows only; and what
    the CPU oracle's cross-check match makes of the held rows, inverted: match12[k1] = k2, n_matches their number"""
    rng = np.random.default_rng(1300)
    q = lambda v: tri_ref.widen_bf16(tri_ref.to_bf16(v.astype(np.float32))).reshape(v.shape)   # noqa: E731
    unit = lambda n: (lambda d: d / np.linalg.norm(d, axis=1, keepdims=True))(rng.standard_normal((n, 256)))   # noqa: E731
    kmax, n = NF_LARGE + 1, 2000
    d1 = q(unit(ROWS[0]))
    mp1 = np.full(kmax, -1, np.int32)
    mp1[:ROWS[0]] = np.where(rng.random(ROWS[0]) < 0.8, rng.integers(0, n, ROWS[0]), -1)
    d2s, mp2, want, n_want = [], np.full((len(ROWS), kmax), -1, np.int32), np.full((len(ROWS), kmax), -1, np.int32), []
    for j, K2 in enumerate(ROWS):
        src = rng.permutation(ROWS[0])[:K2] if K2 <= ROWS[0] else rng.integers(0, ROWS[0], K2)
        d2 = d1[src] + 0.05 * unit(K2)                                   # (make_golden_tri.near)
        stray = rng.random(K2) < 0.2
        d2[stray] = unit(int(stray.sum()))
        d2s.append(q(d2))
        held = rng.random(K2) < (0.75 if j != 1 else 12.0 / K2)
        mp2[j, :K2] = np.where(held, rng.integers(0, n, K2), -2)
        i1, i2 = np.flatnonzero(mp1 >= 0), np.flatnonzero(mp2[j] >= 0)
        idx, _ = oracle.match_bruteforce(d2s[j][i2], d1[i1], True)
        for qq, t in enumerate(idx):
            if t >= 0:
                assert want[j, i1[t]] == -1                                  # the cross-check leaves a train row to one query
                want[j, i1[t]] = i2[qq]
        n_want.append(int((idx >= 0).sum()))
    xyz = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1, 1, n), rng.uniform(3, 6, n)], 1).astype(np.float32)
    flags = (rng.random(n) < 0.95).astype(np.uint8)
    T2 = np.stack([np.eye(4, dtype=np.float32)] * len(ROWS))
    T2[:, 0, 3] = [0.1, -0.2, 0.3]
    return dict(d1=d1, d2s=d2s, mp1=mp1, mp2=mp2, want=want, n_want=n_want, xyz=xyz, flags=flags, T2=T2)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_large_match_equals_the_cpu_oracle_and_the_chain_the_single_forms(large_exts, large, bf16):
    import torch
    ext, g = large_exts(bf16), large
    kmax, nc, n_hyp = ext.layout.kmax, len(ROWS), 24
    assert g["n_want"][0] >= 500 and g["n_want"][2] >= 250 and 0 < g["n_want"][1] < 20, g["n_want"]
    assert (g["mp1"] < 0).sum() >= 100 and all((g["mp2"][j, :ROWS[j]] < 0).sum() >= 100 for j in range(nc))   # masks on both sides
    r1, r2s = record(ext, g["d1"]), [record(ext, d) for d in g["d2s"]]
    # the single form against the CPU oracle
    for j in range(nc):
        got, n = loop_match(ext, r1, r2s[j], g["mp1"], g["mp2"][j])
        assert np.array_equal(got, g["want"][j]), (j, np.flatnonzero(got != g["want"][j])[:8])
        assert n == g["n_want"][j] == (got >= 0).sum()
    # the chain against the single forms
    rnd = np.random.default_rng(9).integers(0, 1 << 32, (nc, n_hyp, 3), dtype=np.uint64).astype(np.uint32)
    ob = ext.sim3_out_bytes(n_hyp)
    T1 = np.eye(4, dtype=np.float32)
    d_mp1, d_mp2, d_P, d_f, d_T1, d_T2, d_r = [dev(v) for v in (g["mp1"], g["mp2"], g["xyz"], g["flags"], T1.reshape(16),
                                                               g["T2"].reshape(-1, 16), rnd)]
    p = lambda t: t.data_ptr()   # noqa: E731
    new = lambda nbytes: torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")   # noqa: E731
    c_m, c_n, c_out = new(nc * kmax * 4), new(nc * 4 + 8), new(nc * ob + 64)
    ext.loop_verify_records_device(p(r1), [p(r) for r in r2s], p(d_mp1), p(d_mp2), p(d_P), p(d_f), len(g["flags"]), p(d_T1), p(d_T2),
                                   p(d_r), n_hyp, p(c_m), p(c_n), p(c_out), INTR)
    s_m, s_n, s_out = new(nc * kmax * 4), new(nc * 4 + 8), new(nc * ob + 64)
    for j in range(nc):
        ext.loop_match_record_device(p(r1), p(r2s[j]), p(d_mp1), p(d_mp2[j]), p(s_m) + 4 * kmax * j, p(s_n) + 4 * j)
        ext.sim3_ransac_device(ROWS[0], p(s_m) + 4 * kmax * j, p(d_mp1), p(d_mp2[j]), p(d_P), p(d_f), len(g["flags"]), p(d_T1),
                               p(d_T2[j]), p(d_r[j]), n_hyp, p(s_out) + ob * j, INTR)
    torch.cuda.synchronize()
    for a, b in ((c_m, s_m), (c_n, s_n), (c_out, s_out)):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert (c_out.cpu().numpy()[-64:] == FILL).all() and (c_n.cpu().numpy()[-8:] == FILL).all()
    assert np.array_equal(c_m.cpu().numpy().view(np.int32).reshape(nc, kmax), g["want"])
    assert c_n.cpu().numpy()[:4 * nc].view(np.int32).tolist() == g["n_want"]
    blocks = [ext.decode_sim3_out(c_out.cpu().numpy()[j * ob:(j + 1) * ob], kmax, n_hyp) for j in range(nc)]
    assert blocks[0]["N"] >= 400 and blocks[0]["best_h"] >= 0 and blocks[2]["N"] >= 200 and blocks[2]["best_h"] >= 0
    assert blocks[1]["N"] < 20 and blocks[1]["best_h"] == -1 and (blocks[1]["count"] == 0).all()
