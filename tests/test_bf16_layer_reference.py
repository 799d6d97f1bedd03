"""CPU: the float64 per-layer reference of the bf16 mode (tests/bf16_ref/bf16_layers.py) and its checker.

Layout: the reference chained from the image (each layer's bf16-rounded output feeding the next) reproduces the oracle's bf16
emulation (oracle.network_bf16) up to rounding flips that propagate — a layout, padding, 1/255 fold or pool mistake is an
error of order 1e-1 of the logit scale.

Teeth: the checker passes an f32-accumulating, RNE-rounding model of each layer (bf16_layers.f32_kernel) and rejects each
mutation of that model the bf16 kernels could plausibly suffer: truncation in place of RNE, a weight dropped, the input one
column off, the right border replicated instead of zero-padded, a 32-channel block's bias dropped, the dustbin logit computed
with its neighbour's weights, another frame's activations."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "bf16_ref"))
import bf16_layers as R  # noqa: E402

from oracle import oracle  # noqa: E402
from sp_orb_slam_amd import synth, weights  # noqa: E402

# Chained reference against oracle.network_bf16 (the two differ only in the summation order inside a dot product, so by the
# logits most elements sit a flip or two apart).  Measured at the shapes below: max / scale 1.1e-3 ... 3.9e-3, share of logits
# within one bf16 step (2^-8 relative) 0.603 ... 0.609; the image shifted by one column gives max / scale 5.6e-2 ... 1.8e-1.
CHAIN_MAX_REL = 6e-3
CHAIN_STEP_SHARE = 0.55
# the f32-accumulating model of a kernel: exact-rounding fraction >= 0.9999 at every layer here; truncation: 0.85 ... 0.93
MODEL_FRACTION = 0.999
FLOOR = 0.99   # what the GPU test's floors may not go below (a truncating kernel must fail them)


def chain(blob, img):
    bufs = {"image": img}
    refs = {}
    for name, (src, dst, _, _, _) in R.LAYERS.items():
        ref = R.reference(blob, name, R.layer_input(name, bufs["head" if name in ("convPb", "convDb") else src]))
        bufs[dst] = R.exact_output(ref)
        refs[dst] = ref
    return bufs, refs


@pytest.mark.parametrize("H,W", [(24, 40), (64, 96), (136, 200)])
@pytest.mark.parametrize("det", ["dense", "sparse"])
def test_chained_reference_matches_the_oracle_bf16_network(H, W, det):
    blob = weights.synthetic(7, det)
    img = synth.make_image(3, H, W)
    bufs, refs = chain(blob, img)
    rsemi, rcoarse = oracle.network_bf16(blob, img)
    for nm, r in (("semi", rsemi), ("coarse", rcoarse)):
        mine = bufs[nm]
        r = r.reshape(mine.shape)
        d = np.abs(mine.astype(np.float64) - r)
        scale = np.abs(r).max()
        step_share = float((d <= 2.0 ** -8 * np.abs(r)).mean())
        print("%dx%d %s %s: max/scale %.2e, within one bf16 step %.3f" % (H, W, det, nm, d.max() / scale, step_share))
        assert d.max() <= CHAIN_MAX_REL * scale
        assert step_share >= CHAIN_STEP_SHARE
    # the conv stack's shapes are the library's debug-read shapes
    assert bufs["act0"].shape == (H, W, 64) and bufs["act1"].shape == (H // 2, W // 2, 64)
    assert bufs["act3"].shape == (H // 4, W // 4, 64) and bufs["act5"].shape == (H // 8, W // 8, 128)
    assert bufs["head"].shape == (H // 8, W // 8, 512) and bufs["semi"].shape == (H // 8, W // 8, 65)


def test_bf16_rounding_helpers():
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.standard_normal(20000) * 10.0 ** rng.integers(-6, 6, 20000), [0.0, 1.0, -1.0, 1 + 2.0 ** -8]])
    lo, hi = R.bf16_rd(x), R.bf16_ru(x)
    assert (lo <= x).all() and (hi >= x).all()
    assert np.array_equal(R.bf16_rne(lo.astype(np.float32)), lo.astype(np.float32))   # on the grid
    assert np.array_equal(R.bf16_rne(hi.astype(np.float32)), hi.astype(np.float32))
    exact = lo == x
    assert np.array_equal(exact, hi == x)
    gap = hi[~exact] - lo[~exact]   # one bf16 step apart: 2^-7 of the binade
    assert (gap > 0).all() and (gap <= np.abs(x[~exact]) * 2.0 ** -7).all()
    x32 = x.astype(np.float32)
    r = R.bf16_rne(x32).astype(np.float64)
    assert (np.abs(r - x32) <= np.abs(x32) * 2.0 ** -8 * (1 + 1e-9)).all()
    assert R.bf16_rne(np.float32(1 + 2.0 ** -8)) == 1.0 and R.bf16_rne(np.float32(1 + 3 * 2.0 ** -8)) == 1 + 2.0 ** -6


def test_row_bands_equal_the_whole_frame():
    blob = weights.synthetic(7, "dense")
    rng = np.random.default_rng(2)
    x = R.bf16_rne(np.maximum(rng.standard_normal((40, 24, 64)), 0).astype(np.float32))
    full = R.reference(blob, "conv2b", x)
    rows = np.array([0, 1, 7, 8, 9, 19])
    part = R.reference(blob, "conv2b", x, rows=rows)
    crow = np.stack([2 * rows, 2 * rows + 1], 1).reshape(-1)
    # (s: sums of bf16 x bf16 products, exact in float64 whatever the order; A is taken in f32)
    assert np.array_equal(part["s"], full["s"][crow]) and np.allclose(part["A"], full["A"][crow], rtol=1e-5, atol=0)
    band = R.conv_sum(x, *R.layer_params(blob, "conv2b"), rows=np.arange(40), band=5)
    assert np.array_equal(band[0], full["s"]) and np.allclose(band[1], full["A"], rtol=1e-5, atol=0)
    # A bounds the f64 magnitude sum from above
    w, b = R.layer_params(blob, "conv2b")
    xp = np.pad(x.astype(np.float64), ((1, 1), (1, 1), (0, 0)))
    a00 = np.abs(b) + sum(np.abs(xp[1 + dy, 1 + dx]) @ np.abs(w[:, :, 1 + dy, 1 + dx]).T for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    assert (full["A"][0, 0] >= a00).all() and (full["A"][0, 0] <= a00 * 1.002).all()


# ---------------------------------------------------------------------------------------------------------------------
# teeth
# ---------------------------------------------------------------------------------------------------------------------
def _inputs(name, H, W, seed):
    """Frames of a layer's input at its own resolution: u8 pixels for conv1a, else ReLU'd bf16 activations with zeros."""
    if name == "conv1a":
        return [synth.make_image(seed + f, H, W) for f in range(2)]
    cin = weights.layer_slices()["convPa" if name == "convPaDa" else name][1][1]
    rng = np.random.default_rng(seed)
    return [R.bf16_rne(np.maximum(rng.standard_normal((H, W, cin)) * 0.7, 0).astype(np.float32)) for _ in range(2)]


def _model(name, x, params, **kw):
    _, _, pooled, relu, bf16 = R.LAYERS[name]
    return R.f32_kernel(x, params[0], params[1], pooled, relu, bf16, **kw)


def _passes(st):
    return st["bad"] == 0 and (st["frac"] >= FLOOR or not st["bf16"])


BLOB = weights.synthetic(7, "sparse")
SHAPE = (16, 40)   # 40 columns: one full 32-column tile and a ragged one


@pytest.mark.parametrize("name", list(R.LAYERS))
def test_checker_passes_an_f32_accumulating_rne_kernel(name):
    params = R.layer_params(BLOB, name)
    x = _inputs(name, *SHAPE, seed=11)[0]
    st = R.check(_model(name, x, params), R.reference(BLOB, name, x, params=params))
    print(R.describe(name, st))
    assert st["bad"] == 0
    if st["bf16"]:
        assert st["frac"] >= MODEL_FRACTION


def _mutant(kind):
    """-> (layer, model output of the mutated kernel, reference of the correct layer)"""
    name = {"truncate": "conv2a", "tap": "conv1b", "shift": "conv2b", "edge": "conv3b", "bias32": "conv4a",
            "dustbin": "convPb", "frame": "convPaDa", "truncate1a": "conv1a", "shift1a": "conv1a"}[kind]
    params = R.layer_params(BLOB, name)
    w, b = params
    x0, x1 = _inputs(name, *SHAPE, seed=23)
    x = x0
    kw = {}
    if kind in ("truncate", "truncate1a"):
        kw["rounding"] = R.bf16_trunc
    elif kind == "tap":                        # one weight of the last tap (the one reading the right and bottom borders)
        w = w.copy()
        w[5, 17, 2, 2] = 0.0
    elif kind in ("shift", "shift1a"):          # the input read one column to the right
        x = np.zeros_like(x0)
        x[:, :-1] = x0[:, 1:]
    elif kind == "edge":
        kw["pad_mode"] = "edge"
    elif kind == "bias32":
        b = b.copy()
        b[32:64] = 0.0
    elif kind == "dustbin":
        w = w.copy()
        w[64] = w[63]
    y = _model(name, x, (w, b), **kw)
    ref_in = x1 if kind == "frame" else x0      # frame 0's activations handed in as frame 1's
    return name, y, R.reference(BLOB, name, ref_in, params=params)


@pytest.mark.parametrize("kind", ["truncate", "truncate1a", "tap", "shift", "shift1a", "edge", "bias32", "dustbin", "frame"])
def test_checker_rejects_a_mutated_kernel(kind):
    name, y, ref = _mutant(kind)
    st = R.check(y, ref)
    print(R.describe("%s (%s)" % (name, kind), st))
    assert not _passes(st), (kind, st["bad"], st["frac"])
    if kind.startswith("truncate"):
        assert st["bad"] == 0     # truncation stays inside the interval: the fraction is what catches it
