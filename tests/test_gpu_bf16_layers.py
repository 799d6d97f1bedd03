"""GPU: every bf16 conv layer, element by element, against the float64 reference of tests/bf16_ref/bf16_layers.py fed the
kernel's OWN input (the library's widened debug reads), so that errors do not compound and each output element is held to
a rigorous interval, and the exact-rounding fraction to a floor measured on the MI355X.

  layer          input                      output
  conv1a         image (u8)                 act0       (SPFE_FUSE_CONV1A=0, so that act0 exists)
  conv1b..4b     act0 .. act6               act1 .. act7
  convPa|Da      act7                       head       (Da half: listed cells only when convDa ran gathered)
  convPb         head[..., :256]            semi
  convDb         head[..., 256:]            coarse     (coarse_sparse at the listed cells, then the completed map)

Forced variants (SPFE_TWO_CHAINS=0: the handle's own buffers are the ones read).  Kernels each case runs, from one
`rocprofv3 --kernel-trace --stats` run per case on the MI355X (names without namespaces; every case also runs
conv1a_bf16_kernel, the tail and the selection):
  ws_off      SPFE_BF16_WS=0,0            conv_bf16_kernel<64, true|false, false, 2>, no conv_bf16_ws_kernel
  ws_on       SPFE_BF16_WS=15,0           conv_bf16_ws_kernel<false, 0>, <true, 0>, <true, 1>, no conv_bf16_kernel<64, ...>
  ws_on_small (24x40: only conv1b is 32 columns wide)   conv_bf16_ws_kernel<true, 1>, conv_bf16_kernel<64, ...> behind it
  rw_off      SPFE_BF16_RW=0              conv_bf16_kernel<128, true|false, false, 2>, no conv_bf16_rw_kernel
  rw4         SPFE_BF16_RW=1,0,0,0        conv_bf16_rw_kernel<4, true|false>
  rw2         SPFE_BF16_RW=1,1000000,0,0  conv_bf16_rw_kernel<2, true|false>
  rw3         SPFE_BF16_RW=1,0,0,1        conv_bf16_rw_kernel<4, ...> (the 3-row form is chosen per launch size)
  tile8       SPFE_BF16_TILE_ROWS=8,0  (with RW=0)   conv_bf16_kernel<128, ..., 2>
  tile12/16   SPFE_BF16_TILE_ROWS=12,1 / 16,1 (RW=0, 1280x720: smaller launches keep 8-row tiles)
              conv_bf16_kernel<128, false, false, 3> / conv_bf16_kernel<128, ..., 4>
  dyn0/dyn1   SPFE_BF16_DYN_QUEUE=0 / 1 (RW=0)   conv_bf16_kernel<128, ...>; the queue is a run-time choice the trace cannot
              show: dyn1 runs 1280x720 x 8, whose Cin = 128 launches have the >= 5 items per workgroup it needs
  pbtail0     SPFE_PBTAIL=0               head1x1_bf16_kernel<65, 512, false> + tail_kernel, no pbtail_bf16_kernel
  pbtail2/4   SPFE_PBTAIL=2 / 4           pbtail_bf16_kernel<2> / <4>
  sparse0     SPFE_SPARSE_DA=0, SPFE_SPARSE_DB=0   head1x1_bf16_kernel<256, 512, false>, no da_gather_bf16_kernel
  sparse1     SPFE_SPARSE_DA=1, SPFE_SPARSE_DB=1   da_gather_bf16_kernel, head1x1_bf16_kernel<256, 512, true>
Each case's last two fields list the names the trace must and must not show; the test itself does not use a profiler.

Large frames are checked in row bands: the first and last 16 rows, the rows on either side of tile edges (multiples of 8, 12
and 16), and one seeded band."""
import os
import sys

import numpy as np
import pytest

from oracle import oracle
from sp_orb_slam_amd import synth, weights
from sp_orb_slam_amd.extractor import SPExtractor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "bf16_ref"))
import bf16_layers as R  # noqa: E402

pytestmark = pytest.mark.gpu

# Exact-rounding fraction floor: the share of bf16 outputs equal to bf16_rne(relu(s)) of the exact sum, per layer and frame.
# Measured on the MI355X over every check of this file (795 lines): 0.99948 ... 1.0, the lowest on the smallest outputs
# (conv3b at 24x40: 1 of 1920 elements); 0.9997 ... 1.0 on outputs of 10^5 elements and more.  A truncating epilogue gives
# 0.73 ... 0.93 (CPU model, tests/test_bf16_layer_reference.py).  Up to FLIPS_ALLOWED elements may differ in any output, so
# that the floor does not fall on one flip in a tiny frame.
FRACTION_FLOOR = {name: 0.998 for name in R.LAYERS}
FLIPS_ALLOWED = 2
# f32 heads (convPb, convDb): the largest |y - s| / E measured is 0.0038 (the bound is a worst case over summation orders);
# a logit rounded to bf16 on the way out, or a product lost, uses far more of it.
F32_BOUND_USE = 0.02

# name, H, W, B, detector, environment, kernels the trace shows (see the docstring)
CASES = [
    ("ws_off", 136, 200, 2, "dense", {"SPFE_BF16_WS": "0,0"}, ["conv_bf16_kernel<64"], ["conv_bf16_ws_kernel"]),
    ("ws_on", 480, 752, 3, "sparse", {"SPFE_BF16_WS": "15,0"}, ["conv_bf16_ws_kernel"], ["conv_bf16_kernel<64"]),
    ("ws_on_small", 24, 40, 2, "dense", {"SPFE_BF16_WS": "15,0"}, [], []),
    ("rw_off", 264, 400, 1, "dense", {"SPFE_BF16_RW": "0"}, ["conv_bf16_kernel<128"], ["conv_bf16_rw_kernel"]),
    ("rw4", 480, 752, 3, "dense", {"SPFE_BF16_RW": "1,0,0,0"}, ["conv_bf16_rw_kernel"], []),
    ("rw2", 264, 400, 2, "sparse", {"SPFE_BF16_RW": "1,1000000,0,0"}, ["conv_bf16_rw_kernel"], []),
    ("rw3", 720, 1280, 2, "sparse", {"SPFE_BF16_RW": "1,0,0,1"}, ["conv_bf16_rw_kernel"], []),
    ("tile8", 136, 200, 2, "sparse", {"SPFE_BF16_TILE_ROWS": "8,0", "SPFE_BF16_RW": "0"}, ["conv_bf16_kernel<128"], []),
    ("tile12", 720, 1280, 2, "dense", {"SPFE_BF16_TILE_ROWS": "12,1", "SPFE_BF16_RW": "0"}, ["conv_bf16_kernel<128, false, false, 3>"], []),
    ("tile16", 720, 1280, 2, "sparse", {"SPFE_BF16_TILE_ROWS": "16,1", "SPFE_BF16_RW": "0"}, ["conv_bf16_kernel<128, true, false, 4>"], []),
    ("dyn0", 720, 1280, 2, "dense", {"SPFE_BF16_DYN_QUEUE": "0", "SPFE_BF16_RW": "0"}, ["conv_bf16_kernel<128"], []),
    ("dyn1", 720, 1280, 8, "sparse", {"SPFE_BF16_DYN_QUEUE": "1", "SPFE_BF16_RW": "0"}, ["conv_bf16_kernel<128"], []),
    ("pbtail0", 24, 40, 2, "dense", {"SPFE_PBTAIL": "0"}, ["head1x1_bf16_kernel", "tail_kernel"], ["pbtail_bf16_kernel"]),
    ("pbtail2", 136, 200, 2, "sparse", {"SPFE_PBTAIL": "2"}, ["pbtail_bf16_kernel<2>"], ["tail_kernel"]),
    ("pbtail4", 264, 400, 2, "dense", {"SPFE_PBTAIL": "4"}, ["pbtail_bf16_kernel<4>"], []),
    ("sparse0", 136, 200, 2, "dense", {"SPFE_SPARSE_DA": "0", "SPFE_SPARSE_DB": "0"}, ["head1x1_bf16_kernel<256, 512, false>"], ["da_gather_bf16_kernel"]),
    ("sparse1", 264, 400, 2, "sparse", {"SPFE_SPARSE_DA": "1", "SPFE_SPARSE_DB": "1"}, ["da_gather_bf16_kernel", "head1x1_bf16_kernel<256, 512, true>"], []),
]
BAND_PIXELS = 480 * 752   # frames above this many pixels are checked in row bands


def band_rows(Hout, seed, tile_scale=1):
    """Rows of a layer's output to check in a large frame: first / last 16, both sides of every tile edge (multiples of 8,
    12, 16 in the kernel's rows; tile_scale 2 for pooled layers, whose tiles count conv rows), one seeded 16-row band."""
    rows = set(range(min(16, Hout))) | set(range(max(0, Hout - 16), Hout))
    for m in (8, 12, 16):
        step = max(1, m // tile_scale)
        for e in range(step, Hout, step):
            if e < 96 or e > Hout - 96 or e % (48 // tile_scale or 1) == 0:
                rows |= {e - 1, e}
    r0 = int(np.random.default_rng(seed).integers(0, max(1, Hout - 16)))
    rows |= set(range(r0, min(Hout, r0 + 16)))
    return np.array(sorted(r for r in rows if 0 <= r < Hout))


def _env(monkeypatch, env):
    monkeypatch.setenv("SPFE_TWO_CHAINS", "0")
    monkeypatch.setenv("SPFE_FUSE_CONV1A", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _read_frames(ext, frames, skip=()):
    """Debug reads of every layer's buffers, in the order that keeps them what the last call computed: `head` before
    `coarse` (which completes a gathered map), then the completed map and the head it was computed from."""
    out = {f: {} for f in frames}
    for f in frames:
        for nm in ["image"] + ["act%d" % i for i in range(8)] + ["head", "semi"]:
            if nm not in skip:
                out[f][nm] = ext.debug_read(nm, f)
    gathered = int(ext.debug_read("da_gathered")[0])
    C = (ext.height // 8) * (ext.width // 8)
    try:
        total = int(ext.debug_read("db_total")[0])
        lst = ext.debug_read("db_list")[:total].astype(np.int64)
    except Exception:           # (no gathered descriptor head in this handle)
        total, lst = 0, np.zeros(0, np.int64)
    for f in frames:
        out[f]["cells"] = np.sort(lst[(lst >= f * C) & (lst < (f + 1) * C)] - f * C)
        out[f]["coarse_sparse"] = ext.debug_read("coarse_sparse", f)
    for f in frames:
        out[f]["coarse"] = ext.debug_read("coarse", f)
    if gathered:
        for f in frames:
            out[f]["head_completed"] = ext.debug_read("head", f)
    return out, gathered, total


def _sub(ref, lo, hi):
    return dict(ref, s=ref["s"][..., lo:hi], A=ref["A"][..., lo:hi])


def _cells_in_rows(cells, rows, wc):
    """flat indices into the checked rows' [len(rows) * wc] of the listed cells that lie in those rows"""
    pos = {int(r): i for i, r in enumerate(rows)}
    return np.array([pos[c // wc] * wc + c % wc for c in cells if c // wc in pos], np.int64)


def check_frame(tag, blob, bufs, gathered, banded, seed, params, layers=None, fail=None):
    """Run the checker on every layer of one frame; print one line per check; collect failures into `fail`."""
    results = []

    def one(label, name, y, ref, cols=None):
        st = R.check(y, ref, cols)
        print(R.describe("%s %s" % (tag, label), st))
        results.append((label, name, st))
        flips = round((1.0 - st["frac"]) * st["n"])
        low = st["bf16"] and flips > max(FLIPS_ALLOWED, (1.0 - FRACTION_FLOOR[name]) * st["n"])
        loose = not st["bf16"] and st["worst"][1] > F32_BOUND_USE
        if st["bad"] or low or loose:
            fail.append("%s %s: %d outside, exact %.6f, worst %.3g" % (tag, label, st["bad"], st["frac"], st["worst"][1]))

    for name, (src, dst, pooled, _, _) in R.LAYERS.items():
        if layers is not None and name not in layers:
            continue
        srcbuf = "head" if name in ("convPb", "convDb") else src
        if srcbuf not in bufs or dst not in bufs:
            continue
        x = R.layer_input(name, bufs[srcbuf])
        if name == "convDb" and gathered:   # convDa wrote the listed cells only: the others hold whatever was there (1x1: unread)
            keep = np.zeros(x.shape[0] * x.shape[1], bool)
            keep[bufs["cells"]] = True
            x = np.where(keep.reshape(x.shape[:2])[..., None], x, 0.0)
        Hout = x.shape[0] // 2 if pooled else x.shape[0]
        rows = band_rows(Hout, seed, 2 if pooled else 1) if banded else None
        ref = R.reference(blob, name, x, rows, params=params[name])
        wc = x.shape[1] // (2 if pooled else 1)
        if name == "convPaDa":
            one("convPa", name, bufs["head"][ref["rows"]][..., :256], _sub(ref, 0, 256))
            if gathered:
                one("convDa[listed]", name, bufs["head"][ref["rows"]][..., 256:], _sub(ref, 256, 512),
                    _cells_in_rows(bufs["cells"], ref["rows"], wc))
            else:
                one("convDa", name, bufs["head"][ref["rows"]][..., 256:], _sub(ref, 256, 512))
        elif name == "convDb":
            if len(bufs["cells"]):
                one("convDb[listed]", name, bufs["coarse_sparse"], ref, _cells_in_rows(bufs["cells"], ref["rows"], wc))
            if not gathered:
                one("convDb", name, bufs["coarse"], ref)
        else:
            one(name, name, bufs[dst], ref)
    if gathered and "head_completed" in bufs and (layers is None or "convPaDa" in layers):
        # the completed map: convDa through the gathered kernel on every cell, convDb densely behind it
        x = bufs["act7"]
        rows = band_rows(x.shape[0], seed) if banded else None
        ref = R.reference(blob, "convPaDa", x, rows, params=params["convPaDa"])
        one("convDa[completed]", "convPaDa", bufs["head_completed"][ref["rows"]][..., 256:], _sub(ref, 256, 512))
        ref = R.reference(blob, "convDb", bufs["head_completed"][..., 256:], rows, params=params["convDb"])
        one("convDb[completed]", "convDb", bufs["coarse"], ref)
    return results


def _params(blob):
    return {name: R.layer_params(blob, name) for name in R.LAYERS}


def _images(seed, H, W, B):
    return [synth.make_image(seed + i, H, W) for i in range(B)]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_bf16_layers_forced_variants(monkeypatch, case):
    tag, H, W, B, det, env, _, _ = case
    _env(monkeypatch, env)
    blob = weights.synthetic(7, det)
    ext = SPExtractor(300, H, W, blob, max_batch=B, precision="bf16", with_heat=False)
    imgs = _images(500 + H + B, H, W, B)
    ext.extract_batch(imgs)
    frames = sorted({0, B - 1})
    bufs, gathered, _ = _read_frames(ext, frames)
    ext.close()
    params = _params(blob)
    fail = []
    for f in frames:
        assert np.array_equal(bufs[f]["image"], imgs[f])
        check_frame("%s %dx%dx%d f%d" % (tag, W, H, B, f), blob, bufs[f], gathered, H * W > BAND_PIXELS, f + H, params,
                    fail=fail)
    assert not fail, fail


def _sweep_cases(n=10, seed=2024):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        H = int(rng.integers(2, 34)) * 8
        W = int(rng.integers(2, 51)) * 8
        out.append((i, H, W, int(rng.integers(1, 4)), ("dense", "sparse")[int(rng.integers(0, 2))],
                    int(rng.choice([1, 50, 300, 2000]))))
    return out


@pytest.mark.parametrize("i,H,W,B,det,nf", _sweep_cases())
def test_bf16_layers_random_sweep(monkeypatch, i, H, W, B, det, nf):
    """Seeded sizes (multiples of 8 in 16..264 x 16..400), batches 1..3, both detectors, 1..2000 features: every layer,
    every row, every frame; everything behind the logits equals the oracle's post-processing of the GPU's own logits."""
    _env(monkeypatch, {})
    blob = weights.synthetic(7, det)
    imgs = _images(900 + 10 * i, H, W, B)
    ext = SPExtractor(nf, H, W, blob, max_batch=B, precision="bf16", with_heat=False)
    frs = ext.extract_batch(imgs)
    bufs, gathered, _ = _read_frames(ext, list(range(B)))
    ext.close()
    params = _params(blob)
    fail = []
    for f in range(B):
        check_frame("sweep%d %dx%dx%d %s nf%d f%d" % (i, W, H, B, det, nf, f), blob, bufs[f], gathered, False, f, params,
                    fail=fail)
        ref = oracle.postprocess(bufs[f]["semi"], bufs[f]["coarse"], H, W, nf)
        fr = frs[f]
        assert fr.K == ref["K"] and np.array_equal(fr.kp_xy, ref["kp_xy"]) and np.array_equal(fr.occ_grid, ref["occ_grid"])
        assert np.array_equal(fr.descriptors.view(np.uint32), ref["desc"].view(np.uint32))
        assert np.array_equal(fr.cov2_inv.view(np.uint32), ref["cov2_inv"].view(np.uint32))
    assert not fail, fail


def test_bf16_layers_720p_batch8_last_frame(monkeypatch):
    """BASELINE configs[3]: 1280x720 x 8, frame 7 (the last frame's offsets), in row bands."""
    H, W, B = 720, 1280, 8
    _env(monkeypatch, {})
    blob = weights.synthetic(7, "sparse")
    imgs = _images(300, H, W, B)
    ext = SPExtractor(1000, H, W, blob, max_batch=B, precision="bf16", with_heat=False)
    ext.extract_batch(imgs)
    bufs, gathered, _ = _read_frames(ext, [B - 1])
    ext.close()
    fail = []
    check_frame("720p x8 f7", blob, bufs[B - 1], gathered, True, 7, _params(blob), fail=fail)
    assert not fail, fail


def test_bf16_layers_2160p(monkeypatch):
    """3840x2160 x 1 from conv2a on (the last rows sit near the end of the 32-bit bf16 offsets), in row bands.  act0 and
    conv1b are not read: act0 widened to f32 is 2.1 GB on the host."""
    H, W = 2160, 3840
    _env(monkeypatch, {"SPFE_FUSE_CONV1A": "1"})
    blob = weights.synthetic(7, "sparse")
    img = synth.make_image(79, H, W)
    ext = SPExtractor(1000, H, W, blob, max_batch=1, precision="bf16", with_heat=False)
    ext.extract_batch([img])
    bufs, gathered, _ = _read_frames(ext, [0], skip=("image", "act0"))
    ext.close()
    fail = []
    check_frame("2160p", blob, bufs[0], gathered, True, 3, _params(blob),
                layers=[n for n in R.LAYERS if n not in ("conv1a", "conv1b")], fail=fail)
    assert not fail, fail


def test_head_reads_back_in_both_precisions():
    """debug_read("head"): ReLU(convPa) | ReLU(convDa), f32 in f32 mode, bf16 widened in bf16 mode (compared on the convPa
    half: convDa may have run on the listed cells only)."""
    H, W = 64, 96
    blob = weights.synthetic(7, "dense")
    img = synth.make_image(5, H, W)
    heads = {}
    for prec in ("f32", "bf16"):
        ext = SPExtractor(100, H, W, blob, precision=prec, with_heat=False)
        ext(img, None)
        heads[prec] = ext.debug_read("head")[..., :256]
        ext.close()
    hb = heads["bf16"]
    assert hb.shape == (H // 8, W // 8, 256) and (hb >= 0).all() and (hb > 0).mean() > 0.2
    assert np.array_equal(R.bf16_rne(hb), hb)                                   # bf16 values
    d = np.abs(hb - heads["f32"])
    assert d.max() <= 0.05 * np.abs(heads["f32"]).max()
