"""Generated cases of the patch-wise association (spfe_match_patches*, oracle_match_patches) beyond the claim workgroup's 1024
threads and the 48 KB of dynamic LDS a launch gets by default (patch_resolve_kernel keeps 5 bytes per keypoint: 9828 and more
raise it), a dependency chain, the positions at the grid's edges, and a numpy restatement of the sequential loop that can
forget which keypoints are taken — the oracle cannot — to show what the keypoints above a boundary decide.  numpy only."""
import numpy as np

LDS_THRESHOLD = 9828
assert 5 * (LDS_THRESHOLD - 1) + 16 <= 48 * 1024 < 5 * LDS_THRESHOLD + 16


def unit_rows(rng, n):
    a = rng.normal(size=(n, 256))
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def dist(a, b):
    """oracle_match_patches' distance, operation for operation: f32 differences, squares and sums in double — lane l of 64
    adds its dimensions 4 l .. 4 l + 3 in order, then the butterfly — and the square root rounded to f32.  a, b: [..., 256]"""
    d = (np.asarray(a, np.float32) - np.asarray(b, np.float32)).astype(np.float64)
    q = (d * d).reshape(d.shape[:-1] + (64, 4))
    v = ((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ off]
    return np.sqrt(v[..., 0]).astype(np.float32)


def sequential(mp_desc, mp_uv, occ, kp_desc, max_dist=0.75, forget_from=None):
    """The loop of oracle_match_patches in numpy -> kp_idx.  forget_from = B: a keypoint with index >= B is never removed from
    the grid, which is what a claim stage that loses the `taken` flags above B would compute."""
    occ = np.array(occ, np.int64)
    hc, wc = occ.shape
    K = len(kp_desc)
    uv = np.asarray(mp_uv, np.float32).reshape(-1, 2)
    out = np.full(len(uv), -1, np.int32)
    fl = np.floor(uv)
    ok = (fl[:, 0] >= 0) & (fl[:, 1] >= 0) & (fl[:, 0] < wc) & (fl[:, 1] < hc)          # False for NaN
    md = np.float32(max_dist)
    for i in np.flatnonzero(ok):
        u, v = int(fl[i, 0]), int(fl[i, 1])
        cells = [(u + du, v + dv) for du in (0, 1) for dv in (0, 1) if u + du < wc and v + dv < hc]
        cand = [(uu, vv, occ[vv, uu]) for uu, vv in cells if 0 <= occ[vv, uu] < K]
        if not cand:
            continue
        d = dist(mp_desc[i][None], kp_desc[[c[2] for c in cand]])
        best, bd = -1, md
        for j, dj in enumerate(d):
            if dj < bd:
                best, bd = j, dj
        if best >= 0:
            uu, vv, k = cand[best]
            out[i] = k
            if forget_from is None or k < forget_from:
                occ[vv, uu] = -1
    return out


def scale(K, m=3000, hc=100, wc=128, seed=0, hot=72, contention=0.3):
    """K keypoints, keypoint k in cell k in raster order (their rows close to one base row: a neighbour is a second choice below
    0.75), and m map points that re-observe them: 45 % on the `hot` keypoints with the highest indices; a point's position is
    its keypoint's cell less 0 or 1 in either axis plus a fraction, so that its own cell is one of the four; descriptor noise
    from 0.1 to 1.0 around max_dist; `contention` of the points repeat an earlier point's keypoint; some fall outside.
    -> dict(desc, uv, occ, kp_desc)"""
    rng = np.random.default_rng([seed, K, m, 5])
    assert 0 < K <= hc * wc
    occ = np.full((hc, wc), -1, np.int16)
    occ.reshape(-1)[:K] = np.arange(K)
    rows = (unit_rows(rng, 1) + 0.3 * unit_rows(rng, K)).astype(np.float32)
    lo = max(K - hot, 0)
    k = np.where(rng.random(m) < 0.45, rng.integers(lo, K, m), rng.integers(0, K, m))
    rep = np.flatnonzero(rng.random(m) < contention)
    rep = rep[rep > 0]
    k[rep] = k[rng.integers(0, rep)]                                     # an earlier point's keypoint
    desc = rows[k] + rng.choice([0.1, 0.3, 0.5, 0.7, 0.8, 1.0], (m, 1)) * unit_rows(rng, m)
    uv = np.stack([k % wc - rng.integers(0, 2, m) + rng.random(m) * 0.999, k // wc - rng.integers(0, 2, m) + rng.random(m) * 0.999], 1)
    uv[rng.random(m) < 0.03] = [-3.0, 500.0]
    return dict(desc=desc.astype(np.float32), uv=uv.astype(np.float32), occ=occ, kp_desc=rows)


def chain(n=1500, hc=100, wc=128, seed=1):
    """n keypoints along a snake of 4-connected cells (rows two cells apart, joined at alternating ends), rows close to one base
    row; point 0 sits on keypoint 0, point i on the 2 x 2 patch that holds keypoints i - 1 and i, nearest to keypoint i - 1 —
    which point i - 1 takes — and next to its own: the sequential answer is point i on keypoint i, and the fixed point needs a
    round per point."""
    rng = np.random.default_rng([seed, n, 6])
    path, iy, fwd = [], 1, True
    while len(path) < n:
        xs = range(1, wc - 1) if fwd else range(wc - 2, 0, -1)
        path += [(ix, iy) for ix in xs] + [((wc - 2) if fwd else 1, iy + 1)]
        iy, fwd = iy + 2, not fwd
    path = path[:n]
    assert iy + 1 < hc
    occ = np.full((hc, wc), -1, np.int16)
    for j, (ix, iy) in enumerate(path):
        occ[iy, ix] = j
    base = unit_rows(rng, 1)[0]
    e = unit_rows(rng, n)
    rows = (base + 0.25 * e).astype(np.float32)
    desc = np.concatenate([[base + 0.25 * e[0]], base + 0.25 * (0.7 * e[:-1] + 0.3 * e[1:])]).astype(np.float32)
    p = np.array(path, np.float64)
    corner = np.concatenate([p[:1], np.minimum(p[:-1], p[1:])])          # the patch's first cell
    uv = corner + rng.uniform(0.05, 0.95, (n, 2))
    return dict(desc=desc, uv=uv.astype(np.float32), occ=occ, kp_desc=rows)


def sparse(K, hc=8, wc=12, m=150, seed=0):
    """K keypoints of which only hc x wc sit in the small grid, with indices spread from 0 to K - 1, the last ones among them"""
    rng = np.random.default_rng([seed, K, 8])
    cells = hc * wc
    special = [v for v in (0, 1, 1023, 1024, 1025, LDS_THRESHOLD - 1, LDS_THRESHOLD, K - 3, K - 2, K - 1) if 0 <= v < K]
    others = rng.permutation(np.setdiff1d(np.arange(K), special))[:cells - len(special)]
    idx = rng.permutation(np.concatenate([np.array(special, np.int64), others]))
    occ = np.full((hc, wc), -1, np.int16)
    occ.reshape(-1)[:len(idx)] = idx
    rows = np.zeros((K, 256), np.float32)
    rows[idx] = unit_rows(rng, 1) + 0.3 * unit_rows(rng, len(idx))
    c = rng.integers(0, len(idx), m)
    desc = rows[idx[c]] + rng.choice([0.1, 0.5, 0.7, 0.8], (m, 1)) * unit_rows(rng, m)
    uv = np.stack([c % wc - rng.integers(0, 2, m) + rng.random(m) * 0.999, c // wc - rng.integers(0, 2, m) + rng.random(m) * 0.999], 1)
    return dict(desc=desc.astype(np.float32), uv=uv.astype(np.float32), occ=occ, kp_desc=rows)


def edges(hc=30, wc=40, seed=2):
    """Every cell of the grid holds a keypoint; the points sit where the 2 x 2 patch hangs over the border, where the position
    floors to -1 or to the first column / row outside, and where it is not finite.  -> dict(desc, uv, occ, kp_desc, inside:
    whether the position floors into the grid)"""
    rng = np.random.default_rng([seed, hc, wc])
    K = hc * wc
    occ = rng.permutation(K).astype(np.int16).reshape(hc, wc)
    rows = (unit_rows(rng, 1) + 0.3 * unit_rows(rng, K)).astype(np.float32)
    inf, nan = np.inf, np.nan
    uv = [(wc - 1 + f, y) for f in (0.0, 0.3, 0.999) for y in (0.0, 4.5, hc - 2.0, hc - 1.0, hc - 0.001)]
    uv += [(x, hc - 1 + f) for f in (0.0, 0.3, 0.999) for x in (0.0, 7.25, wc - 2.0, wc - 1.5)]
    n_in = len(uv)
    uv += [(-0.5, 3.0), (3.0, -0.5), (-0.5, -0.5), (-1.0, 0.0), (-1e-7, 5.0), (wc, 3.0), (3.0, hc), (wc, hc), (wc + 0.5, hc - 1.0)]
    uv += [(a, b) for a in (nan, inf, -inf, 1e30, -1e30, 3.0e9, -3.0e9) for b in (2.0,)] + [(2.0, a) for a in (nan, inf, -inf, 1e30, -1e30, 3.0e9)]
    uv += [(nan, nan), (inf, -inf), (1e30, 1e30)]
    uv = np.array(uv, np.float32)
    m = len(uv)
    near = np.clip(np.nan_to_num(np.floor(uv), nan=0.0, posinf=1e9, neginf=-1e9), 0, [wc - 1, hc - 1]).astype(int)
    desc = rows[occ[near[:, 1], near[:, 0]]] + 0.2 * unit_rows(rng, m)
    return dict(desc=desc.astype(np.float32), uv=uv, occ=occ, kp_desc=rows, inside=np.arange(m) < n_in)
