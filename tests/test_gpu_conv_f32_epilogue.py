"""conv_f32_kernel's epilogue (run with -m gpu on an MI355X): pool first, then bias and ReLU once; the row test made once per
tile; the pixel's place in its row in the store's scalar offset.  None of it may change a bit.

Shapes, the smallest that reach every path of the epilogue: a ragged last tile column (40, 72, 168 and 200 columns are
1.25, 2.25, 5.25 and 6.25 tiles), 1.5 / 2.5 / 7.5 / 8.5 tile rows of 16 (24, 40, 120 and 136 rows), and batches whose two half
batches are 1 + 2 frames.  Each runs on every tile form: conv1b on 8-row and on 16-row tiles (SPFE_TILE16X4 = 0 / 2), the
layers behind it on 4 / 8-row and on 2-row tiles (SPFE_TILE2_MASK = 0 / 0xEA), and conv1a fused into conv1b
(SPFE_FUSE_CONV1A = 1).  semi and coarse are held to the CPU oracle's bits, act1 and feat to the first form's.

Weights: the `dense` synthetic set, and two sets whose biases are all negative.  With the large ones every ReLU clips, every
pooled window is all zeros and the bias added after the maximum is what decides; with the small ones most windows clip and
some do not, side by side."""
import numpy as np
import pytest

from oracle import oracle
from sp_orb_slam_amd import synth, weights
from sp_orb_slam_amd.extractor import SPExtractor

pytestmark = pytest.mark.gpu

FORMS = [  # (SPFE_TILE16X4, SPFE_TILE2_MASK, SPFE_FUSE_CONV1A)
    ("0", "0", "0"),
    ("2", "0", "0"),
    ("0", "0xEA", "0"),
    ("2", "0xEA", "0"),
    ("0", "0", "1"),
]


def _negative_bias_blob(seed, floor, spread):
    """He-normal weights as weights.synthetic() draws them; every bias = -(floor + spread * |N(0, 1)|)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    named = {}
    for name, ci, co, k in weights.LAYERS:
        std = np.sqrt(2.0 / (ci * k * k))
        named[name + ".weight"] = (rng.standard_normal((co, ci, k, k)) * std).astype(np.float32)
        named[name + ".bias"] = (-floor - spread * np.abs(rng.standard_normal(co))).astype(np.float32)
    return weights.from_named_tensors(named)


def _blob(kind):
    if kind == "dense":
        return weights.synthetic(7, "dense")
    if kind == "all_clipped":
        return _negative_bias_blob(11, 0.5, 0.5)
    return _negative_bias_blob(11, 0.05, 0.1)   # "mostly_clipped"


def _bits(a):
    return np.ascontiguousarray(a).ravel().view(np.uint32)


@pytest.mark.parametrize("kind", ["dense", "all_clipped", "mostly_clipped"])
@pytest.mark.parametrize("H,W,B", [(24, 40, 2), (40, 72, 1), (120, 168, 3), (136, 200, 1)])
def test_f32_epilogue_bits_on_every_tile_form(monkeypatch, H, W, B, kind):
    blob = _blob(kind)
    imgs = [synth.make_image(210 + 7 * i + H, H, W) for i in range(B)]
    refs = [oracle.network(blob, im) for im in imgs]
    if kind == "all_clipped":   # the blob does what it is for: nothing survives the ReLUs
        assert all(not r[2].any() for r in refs)
    elif kind == "mostly_clipped":
        assert all(0.5 < float((r[2] == 0).mean()) < 0.99 for r in refs)
    first = None
    for t16, mask2, fuse in FORMS:
        monkeypatch.setenv("SPFE_TILE16X4", t16)
        monkeypatch.setenv("SPFE_TILE2_MASK", mask2)
        monkeypatch.setenv("SPFE_FUSE_CONV1A", fuse)
        ext = SPExtractor(100, H, W, blob, max_batch=B, with_heat=False)
        ext.extract_batch(imgs)
        got = [{nm: ext.debug_read(nm, i) for nm in ("act1", "feat", "semi", "coarse")} for i in range(B)]
        ext.close()
        for i in range(B):
            semi, coarse, feat = refs[i]
            assert np.array_equal(_bits(got[i]["semi"]), _bits(semi)), (t16, mask2, fuse, i)
            assert np.array_equal(_bits(got[i]["coarse"]), _bits(coarse)), (t16, mask2, fuse, i)
            assert np.array_equal(_bits(got[i]["feat"]), _bits(feat)), (t16, mask2, fuse, i)
        if first is None:
            first = got
        for a, b in zip(first, got):
            for nm in ("act1", "feat"):
                assert np.array_equal(_bits(a[nm]), _bits(b[nm])), (t16, mask2, fuse, nm)
