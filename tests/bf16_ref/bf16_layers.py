"""float64 reference of one bf16 conv layer at a time, and the checker that holds a kernel's output to it.

Written from the arithmetic oracle/spfe_oracle.c states for the bf16 mode (oracle_network_bf16, conv1a_bf16) and the kernels
document (conv_bf16.hip, conv1a_mfma.h): bf16 weights, bf16 activations, f32 accumulation with the bias as the accumulator's
start, ReLU, round-to-nearest-even to bf16, 2x2 max-pool; the two 1x1 heads write f32.  A layer is fed the kernel's OWN
input (the library's widened debug read of the previous buffer), so errors do not compound and every output element can be
held to a rigorous bound:

  s = b + sum_k x_k w_k        exact (float64 of bf16 x bf16 products),   A = |b| + sum_k |x_k w_k|,
  E = (K + 2) 2^-23 A + 4 2^-126                                          (K products, any summation order in f32),
  bf16 output:  y in [rd(relu(s - E)), ru(relu(s + E))]  (then pooled: max is monotone),
  f32 output:   |y - s| <= E.

The interval never fails a correct kernel, whatever order its MFMA sums in.  What gives a test teeth is the exact-rounding
fraction, the share of elements equal to bf16_rne(relu(s)): an f32-accumulating, RNE-rounding kernel sits near 1, a
truncating one near 0.9.

Layers are named as in sp_orb_slam_amd/weights.py, plus "convPaDa" (convPa | convDa in one 512-channel output, the layout of
the library's `head` buffer).  Activations are NHWC [H][W][C] arrays, as the library's debug reads return them.
"""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sys  # noqa: E402

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from sp_orb_slam_amd import weights  # noqa: E402

if torch.get_num_threads() > 16:
    torch.set_num_threads(16)

ABS_TERM = 4.0 * 2.0 ** -126
BAND = 32   # rows per float64 convolution pass
A_PAD = 1.001   # the magnitude sum A is taken in f32 (8x the f64 rate); this covers its rounding with room to spare

# name -> (input buffer, output buffer, pooled, relu, bf16 output)
LAYERS = {
    "conv1a": ("image", "act0", False, True, True),
    "conv1b": ("act0", "act1", True, True, True),
    "conv2a": ("act1", "act2", False, True, True),
    "conv2b": ("act2", "act3", True, True, True),
    "conv3a": ("act3", "act4", False, True, True),
    "conv3b": ("act4", "act5", True, True, True),
    "conv4a": ("act5", "act6", False, True, True),
    "conv4b": ("act6", "act7", False, True, True),
    "convPaDa": ("act7", "head", False, True, True),
    "convPb": ("head[:256]", "semi", False, False, False),
    "convDb": ("head[256:]", "coarse", False, False, False),
}


# ---------------------------------------------------------------------------------------------------------------------
# bf16 rounding
# ---------------------------------------------------------------------------------------------------------------------
def bf16_rne(x):
    """float32 -> nearest-even bf16 value (as float32): the oracle's bit trick (finite inputs)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).copy()
    u += np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))
    u &= np.uint32(0xFFFF0000)
    return u.view(np.float32)


def bf16_trunc(x):
    """float32 -> bf16 by truncation (round toward zero): what a kernel that drops the low half does."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def _f32_down(x):
    x = np.asarray(x, np.float64)
    f = x.astype(np.float32)
    m = f.astype(np.float64) > x
    f[m] = np.nextafter(f[m], np.float32(-np.inf))
    return f


def bf16_rd(x):
    """float64 -> the largest bf16 value <= x (as float64)."""
    f = np.atleast_1d(_f32_down(x))
    u = f.view(np.uint32)
    t = u & np.uint32(0xFFFF0000)
    up = ((u >> np.uint32(31)) == 1) & (t != u)       # negative and inexact: truncation went up, step one bf16 ulp down
    t = t + np.where(up, np.uint32(0x10000), np.uint32(0)).astype(np.uint32)
    return t.view(np.float32).astype(np.float64).reshape(np.shape(x))


def bf16_ru(x):
    """float64 -> the smallest bf16 value >= x (as float64)."""
    return -bf16_rd(-np.asarray(x, np.float64))


# ---------------------------------------------------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------------------------------------------------
def layer_params(blob, name):
    """-> (w float64 OIHW holding bf16 values, b float64 holding the f32 bias) of a layer as the bf16 mode runs it.
    conv1a: 1/255 folded into the weight by one f32 multiply, then RNE (its input is the raw u8 pixel)."""
    blob = np.asarray(blob, np.float32)
    sl = weights.layer_slices()
    if name == "convPaDa":
        pa, da = layer_params(blob, "convPa"), layer_params(blob, "convDa")
        return np.concatenate([pa[0], da[0]]), np.concatenate([pa[1], da[1]])
    ws, shape, bs = sl[name]
    w = blob[ws].reshape(shape)
    if name == "conv1a":
        w = w * np.float32(1.0 / 255.0)
    return bf16_rne(w).astype(np.float64), blob[bs].astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# float64 convolution over chosen rows
# ---------------------------------------------------------------------------------------------------------------------
def _runs(rows, band):
    rows = np.asarray(rows, np.int64)
    cut = np.flatnonzero(np.diff(rows) != 1) + 1
    for run in np.split(rows, cut):
        for i in range(0, len(run), band):
            yield int(run[i]), int(run[min(i + band, len(run)) - 1]) + 1


def conv_sum(x, w, b, rows=None, band=BAND):
    """Stride-1 cross-correlation with zero padding ksize // 2, in float64, at the output rows `rows` (sorted; None = all).
    x [H][W][Cin], w [Cout][Cin][k][k], b [Cout] -> (s, A), each [len(rows)][W][Cout]: the exact sum b + sum x w and
    |b| + sum |x w|."""
    x = np.asarray(x)
    H, W, ci = x.shape
    co, ci2, k, _ = w.shape
    assert ci2 == ci, (ci2, ci)
    p = k // 2
    rows = np.arange(H) if rows is None else np.asarray(rows, np.int64)
    tw = torch.from_numpy(np.ascontiguousarray(w, np.float64))
    taw = tw.abs().float()   # A in f32 (all terms positive: relative error <= K 2^-24), padded by A_PAD below
    s = np.empty((len(rows), W, co), np.float64)
    A = np.empty_like(s)
    at = 0
    for r0, r1 in _runs(rows, band):
        xin = np.zeros((r1 - r0 + 2 * p, W, ci), np.float64)
        lo, hi = max(r0 - p, 0), min(r1 + p, H)
        xin[lo - (r0 - p):hi - (r0 - p)] = x[lo:hi]
        t = torch.from_numpy(xin).permute(2, 0, 1)[None]
        n = r1 - r0
        s[at:at + n] = torch.nn.functional.conv2d(t, tw, padding=(0, p))[0].permute(1, 2, 0).numpy()
        A[at:at + n] = torch.nn.functional.conv2d(t.abs().float(), taw, padding=(0, p))[0].permute(1, 2, 0).numpy()
        at += n
    return s + b, (A + np.abs(b)) * A_PAD


def layer_input(name, buf):
    """The slice of a library buffer a layer reads: the 256 convPa / convDa channels of `head` for the 1x1 heads."""
    if name == "convPb":
        return buf[..., :256]
    if name == "convDb":
        return buf[..., 256:]
    return buf


def reference(blob, name, x, rows=None, params=None):
    """float64 reference of layer `name` on its input x, at the OUTPUT rows `rows` (None = all; a pooled layer's output row
    r reads conv rows 2r and 2r + 1).  -> dict(s, A, K, pooled, relu, bf16, rows)"""
    _, _, pooled, relu, bf16 = LAYERS[name]
    w, b = params if params is not None else layer_params(blob, name)
    x = np.asarray(x, np.float64)
    if x.ndim == 2:
        x = x[:, :, None]
    Hout = x.shape[0] // 2 if pooled else x.shape[0]
    rows = np.arange(Hout) if rows is None else np.unique(np.asarray(rows, np.int64))
    crow = np.stack([2 * rows, 2 * rows + 1], 1).reshape(-1) if pooled else rows
    s, A = conv_sum(x, w, b, crow)
    return dict(s=s, A=A, K=int(np.prod(w.shape[1:])), pooled=pooled, relu=relu, bf16=bf16, rows=rows)


def pool2(a):
    """2x2 max-pool of [2n][W][C] (rows already paired) -> [n][W/2][C]."""
    n2, W, c = a.shape
    a = a[:, :W // 2 * 2].reshape(n2 // 2, 2, W // 2, 2, c)
    return a.max(axis=(1, 3))


def exact_output(ref):
    """What an exactly-summing kernel writes: bf16_rne(relu(s)) (pooled), or f32(s) for the f32 heads."""
    s = ref["s"]
    if not ref["bf16"]:
        return s.astype(np.float32)
    v = bf16_rne(np.maximum(s, 0.0).astype(np.float32) if ref["relu"] else s.astype(np.float32))
    return pool2(v) if ref["pooled"] else v


def bound(ref):
    return (ref["K"] + 2) * 2.0 ** -23 * ref["A"] + ABS_TERM


# ---------------------------------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------------------------------
def check(y, ref, cols=None):
    """Hold a kernel's output y (the layer's full output [Hout][Wout][C], or already the checked rows when its row count is
    len(ref["rows"])) to the reference.  cols: restrict to these output columns x rows pairs (a list of flat indices into
    the checked rows' [n * Wout]; the gathered heads).  -> dict(n, bad, frac, worst, first_bad)."""
    y = np.asarray(y, np.float32)
    if y.shape[0] != len(ref["rows"]):
        y = y[ref["rows"]]
    s = ref["s"]
    E = bound(ref)
    ex = exact_output(ref)
    if ref["bf16"]:
        f = (lambda v: np.maximum(v, 0.0)) if ref["relu"] else (lambda v: v)
        lo, hi = bf16_rd(f(s - E)), bf16_ru(f(s + E))
        if ref["pooled"]:
            lo, hi = pool2(lo), pool2(hi)
    else:
        lo, hi = s - E, s + E
    assert y.shape == ex.shape, (y.shape, ex.shape)
    if cols is not None:
        sel = lambda a: a.reshape(-1, a.shape[-1])[cols]  # noqa: E731
        y, ex, lo, hi = sel(y), sel(ex), sel(lo), sel(hi)
    yd = y.astype(np.float64)
    out = (yd < lo) | (yd > hi)
    if ref["bf16"]:
        d = np.abs(yd - ex.astype(np.float64))
        frac = float((y == ex).mean()) if y.size else 1.0
    else:   # f32 heads: the share of the bound used
        d = np.abs(yd - (lo + hi) / 2) / np.maximum((hi - lo) / 2, 1e-300)
        frac = float((y == ex).mean()) if y.size else 1.0
    wi = int(np.argmax(d)) if y.size else 0
    worst = (np.unravel_index(wi, y.shape), float(d.flat[wi]) if y.size else 0.0,
             float(y.flat[wi]) if y.size else 0.0, float(ex.flat[wi]) if y.size else 0.0)
    first_bad = None
    if out.any():
        bi = int(np.argmax(out))
        first_bad = (np.unravel_index(bi, y.shape), float(y.flat[bi]), float(lo.flat[bi]), float(hi.flat[bi]))
    return dict(n=int(y.size), bad=int(out.sum()), frac=frac, worst=worst, first_bad=first_bad, bf16=ref["bf16"])


def describe(tag, st):
    """One log line per layer and frame: the exact-rounding fraction and the worst element."""
    where, d, yv, ev = st["worst"]
    line = "%-34s n=%-9d exact %.6f  worst %s: got %.8g want %.8g (%s %.3g)" % (
        tag, st["n"], st["frac"], tuple(int(v) for v in where), yv, ev, "|d|" if st.get("bf16", True) else "d/E", d)
    if st["bad"]:
        line += "  OUTSIDE: %d, first %s" % (st["bad"], st["first_bad"])
    return line


# ---------------------------------------------------------------------------------------------------------------------
# an f32-accumulating model of a kernel (CPU tests: the checker's positive control and its mutations)
# ---------------------------------------------------------------------------------------------------------------------
def f32_kernel(x, w, b, pooled, relu, bf16, rounding=bf16_rne, pad_mode="zero", step=16):
    """The layer as an MFMA kernel computes it: bias as the f32 accumulator's start, K in steps of `step` products (each
    step's sum exact, then added in f32), ReLU, `rounding` to bf16, pool.  pad_mode "edge": the right border replicates
    the last column instead of reading zeros (a mutation)."""
    x = np.asarray(x, np.float64)
    if x.ndim == 2:
        x = x[:, :, None]
    H, W, ci = x.shape
    co, _, k, _ = w.shape
    p = k // 2
    xp = np.zeros((H + 2 * p, W + 2 * p, ci))
    xp[p:p + H, p:p + W] = x
    if pad_mode == "edge" and p:
        xp[p:p + H, p + W:] = x[:, W - 1:W]
    cols = np.stack([xp[ky:ky + H, kx:kx + W] for ky in range(k) for kx in range(k)], 2).reshape(H * W, k * k * ci)
    wk = np.ascontiguousarray(w.transpose(2, 3, 1, 0).reshape(k * k * ci, co))
    acc = np.broadcast_to(np.asarray(b, np.float32), (H * W, co)).copy()
    for k0 in range(0, k * k * ci, step):
        acc += (cols[:, k0:k0 + step] @ wk[k0:k0 + step]).astype(np.float32)
    y = acc.reshape(H, W, co)
    if not bf16:
        return y
    if relu:
        y = np.maximum(y, np.float32(0))
    y = rounding(y)
    return pool2(y) if pooled else y
