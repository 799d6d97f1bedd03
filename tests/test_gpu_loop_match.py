"""GPU: SPMatcher::SearchByBruteForce(KeyFrame *, KeyFrame *) on resident records (spfe_loop_match_record_device: the
cross-check of match.hip with a mask on BOTH sides) against spfe_match on the rows of both sides compacted on the host, every
row keeping its keypoint index — with f32 and with bf16 descriptor rows; an empty side, one held row, every row held, masks
that differ per side, exact ties."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tri_ref"))
import tri_ref  # noqa: E402  (to_bf16 / widen_bf16)

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
