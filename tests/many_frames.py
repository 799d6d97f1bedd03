"""Calls of many frames (tests/test_gpu_many_frames.py, tests/test_many_frames_arith.py): the cases, the pattern of their
frames and the arithmetic that places the 2^31 and 2^32 byte crossings of a call's buffers.

A call of B frames is built from K_IMAGES = 7 distinct seeded images, frame i carrying image (i + rot) mod 7.  The library
addresses a frame of a buffer as base + i * S with S the frame's bytes in that buffer.  An offset that is truncated to 32
bits, or compared as a signed number, goes wrong first in the frame that holds byte 2^31 or 2^32 of the buffer.  check_case()
proves on the CPU, before a case touches the GPU, that such an access cannot land on equal data:
  * S divides neither 2^31 nor 2^32 in any buffer listed in frame_bytes(), so an offset reduced by 2^31 or 2^32 points INTO a
    frame, never at the start of one: what it reads or writes is shifted against every frame's own data;
  * the frame that holds the crossing and the frames on both sides of it carry three different images, so neither does an
    access that slips by one frame there.
Nothing here touches the GPU or the library; the call helpers at the end take an extractor from the caller."""
import ctypes as C

import numpy as np

K_IMAGES = 7
IMAGE_SEED = 4100                      # image j of a case is synth.make_image(IMAGE_SEED + j, H, W)
GRID_Y_MAX = 65535                     # the frame index is gridDim.y of the tail, selection and covariance launches
ROW_BYTES = {"f32": 2048, "bf16": 1024}   # the head activations of one cell: 512 channels
CROSSINGS = (1 << 31, 1 << 32)

# name -> (precision, H, W, B, num_features, async_cov, host form too).  B None: the largest max_batch spfe_create accepts.
CASES = {
    "act0_past_2_32": ("f32", 136, 200, 620, 100, False, True),
    "max_grid_y": ("f32", 16, 24, 65535, 8, False, True),
    "halves_unequal": ("f32", 136, 200, 621, 100, True, True),
    "act1_past_2_31": ("bf16", 136, 200, 2470, 100, False, True),
    "edge_f32": ("f32", 136, 200, None, 100, False, False),
    "edge_bf16": ("bf16", 136, 200, None, 100, False, False),
}


def cells(H, W):
    return (H // 8) * (W // 8)


def largest_max_batch(H, W, precision):
    """The whole-call limit of spfe_config::max_batch (include/spfe.h): at most 65,535 frames and
    max_batch * cells * R < 2^31 with R = ROW_BYTES[precision]."""
    return min(GRID_Y_MAX, ((1 << 31) - 1) // (cells(H, W) * ROW_BYTES[precision]))


def case(name):
    prec, H, W, B, nf, async_cov, host = CASES[name]
    if B is None:
        B = largest_max_batch(H, W, prec)
    # max_grid_y: frames of 16 rows have no keypoint outside the border, so the covariance stage's per-frame scratch (2.4 MB a
    # frame at its default capacities, 157 GB for 65,535 frames) is created at its smallest: SPFE_COV_CAPS = qcap,ovf_slots,ovf_cap
    cov_caps = (16, 1, 16) if name == "max_grid_y" else None
    return dict(name=name, precision=prec, H=H, W=W, B=B, nf=nf, async_cov=async_cov, host_form=host, cov_caps=cov_caps)


def _up(x, a):
    return (x + a - 1) // a * a


def record_layout(nf, H, W, desc_bf16=False):
    """spfe_record_layout as the library lays it out (f32 descriptors unless desc_bf16): offsets and bytes."""
    kmax, c = nf + 1, cells(H, W)
    o, r = 0, {"kmax": kmax}
    for key, size in (("hdr", 16), ("xy", kmax * 8), ("resp", kmax * 4), ("cov", kmax * 8), ("cinv", kmax * 8),
                      ("desc", kmax * 256 * (2 if desc_bf16 else 4)), ("occ", c * 2), ("dd", c * 4), ("sd", c * 4)):
        r[key] = o
        o = _up(o + size, 16)
    r["bytes"] = _up(o, 256)
    return r


def frame_bytes(H, W, nf, precision):
    """Bytes of ONE frame in the buffers a call addresses by frame: activations in the precision's element size, the
    descriptor map, the logarithmic heat map and the records in f32."""
    e, c = (2 if precision == "bf16" else 4), cells(H, W)
    return {"act0": H * W * 64 * e, "act1": (H // 2) * (W // 2) * 64 * e, "head": c * 512 * e, "coarse": c * 256 * 4,
            "heat_log": H * W * 4, "records": record_layout(nf, H, W)["bytes"]}


def image_of(i, rot=0):
    return (i + rot) % K_IMAGES


def crossings(B, S):
    """[(crossing, frame that holds that byte)] for the crossings below B * S."""
    return [(x, x // S) for x in CROSSINGS if B * S > x]


def check_case(cs, rot=0):
    """The CPU proof of the module docstring for one case and rotation; returns {buffer: [(crossing, frame)]} and the sorted
    frames worth reading back: the first, the last, and those at and beside every crossing."""
    B, out, frames = cs["B"], {}, {0, cs["B"] - 1}
    assert 1 <= B <= largest_max_batch(cs["H"], cs["W"], cs["precision"]), "the case is beyond the whole-call limit"
    for name, S in frame_bytes(cs["H"], cs["W"], cs["nf"], cs["precision"]).items():
        for x in CROSSINGS:
            assert x % S != 0, "%s: a frame of %d bytes divides 2^%d" % (name, S, x.bit_length() - 1)
        out[name] = crossings(B, S)
        for x, f in out[name]:
            assert 0 < f < B and f * S < x < (f + 1) * S, (name, x, f)   # strictly inside frame f
            near = [g for g in (f - 1, f, f + 1) if 0 <= g < B]
            assert len({image_of(g, rot) for g in near}) == len(near), "%s: equal images beside byte %d" % (name, x)
            frames.update(near)
    return out, sorted(frames)


def handle_bytes_estimate(cs):
    """Device bytes a handle of this case takes, from the allocations of the handle's build.  Per pixel: the eight activation
    maps (114 f32-sized elements in both precisions), the image, two logarithmic heat maps, heat_inv and the two claim maps.
    Per cell: head activations, logits, descriptor map, conv4b's second copy, the bf16 head activations, the selection's
    scratch.  Per frame: the record, the covariance queues (qcap pairs and 32 edges a keypoint) and the overflow lists
    (ovf_slots x ovf_cap pairs: 2 MB by default, whatever the frame size).  Per handle: the fallback list (32 MB)."""
    px, c, kmax = cs["H"] * cs["W"], cells(cs["H"], cs["W"]), cs["nf"] + 1
    qcap, ovf_slots, ovf_cap = cs.get("cov_caps") or (1024, 16, 16384)
    per_px = 114 * 4 + 1 + 5 * 4
    per_cell = (512 + 65 + 256 + 128) * 4 + (1024 if cs["precision"] == "bf16" else 0) + 20
    per_frame = px * per_px + c * per_cell + record_layout(cs["nf"], cs["H"], cs["W"])["bytes"] + kmax * (qcap * 8 + 32 * 8 + 40) + \
        ovf_slots * ovf_cap * 8
    return cs["B"] * per_frame + (40 << 20)


def images(cs):
    from sp_orb_slam_amd import synth
    return [synth.make_image(IMAGE_SEED + j, cs["H"], cs["W"]) for j in range(K_IMAGES)]


# ---- records of a call as one [n, record bytes] array, and their comparison with per-image references ----------------------

def host_call(ext, imgs, n, rot):
    """spfe_extract_batch of n frames (frame i = imgs[image_of(i, rot)]) -> copy of the n host records, [n, record bytes]
    uint8.  The results' views point into the library's contiguous host mirror of the records: checked, then read as one block."""
    from sp_orb_slam_amd.extractor import _Result, _check
    ptrs = (C.c_void_p * n)(*[imgs[image_of(i, rot)].ctypes.data for i in range(n)])
    res = (_Result * n)()
    _check(ext._lib.spfe_extract_batch(ext._h, ptrs, ext.width, n, res))
    rb, off_xy = int(ext.layout.bytes), int(ext.layout.off_xy)
    base = res[0].kp_xy - off_xy
    assert res[n - 1].kp_xy == base + (n - 1) * rb + off_xy and res[n // 2].kp_xy == base + (n // 2) * rb + off_xy
    ks = np.array([res[i].K for i in range(0, n, max(1, n // 64))])
    recs = np.frombuffer((C.c_char * (n * rb)).from_address(base), np.uint8).reshape(n, rb).copy()
    assert np.array_equal(ks, recs[::max(1, n // 64), :4].copy().view(np.int32)[:, 0])
    return recs


def reference_fields(ext_layout, ref):
    """[(field, byte offset, expected bytes)] of one frame's record from an oracle-style dict (K, n_candidates, kp_xy,
    response, cov2, cov2_inv, desc, occ_grid, dense_dust, semi_dust): the rows up to K, the per-cell maps whole."""
    f32, L = np.float32, ext_layout
    k = int(ref["K"])

    def b(a, dt):
        return np.ascontiguousarray(a, dt).reshape(-1).view(np.uint8)
    return [("hdr", int(L.off_hdr), b([k, ref["n_candidates"], 0], np.int32)),
            ("kp_xy", int(L.off_xy), b(ref["kp_xy"], f32)), ("response", int(L.off_resp), b(ref["response"], f32)),
            ("cov2", int(L.off_cov), b(ref["cov2"], f32)), ("cov2_inv", int(L.off_cinv), b(ref["cov2_inv"], f32)),
            ("desc", int(L.off_desc), b(ref["desc"], f32)), ("occ_grid", int(L.off_occ), b(ref["occ_grid"], np.int16)),
            ("dense_dust", int(L.off_dd), b(ref["dense_dust"], f32)), ("semi_dust", int(L.off_sd), b(ref["semi_dust"], f32))]


def record_as_ref(fr):
    """The same dict from a FrameResult (the bf16 reference: records of a seven-frame handle)."""
    return dict(K=fr.K, n_candidates=fr.n_candidates, kp_xy=fr.kp_xy, response=fr.response, cov2=fr.cov2, cov2_inv=fr.cov2_inv,
                desc=fr.descriptors, occ_grid=fr.occ_grid, dense_dust=fr.dense_dust, semi_dust=fr.semi_dust)


def mismatches(recs, fields_by_image, rot, limit=8):
    """Bitwise comparison of every frame's record with the fields of its image: ["frame i (image j): field", ...], empty when
    all n frames are equal.  One vectorised comparison per image and field."""
    n, bad = len(recs), []
    for j in range(K_IMAGES):
        idx = np.arange((j - rot) % K_IMAGES, n, K_IMAGES)
        if not len(idx):
            continue
        sub = recs[idx]
        for name, off, want in fields_by_image[j]:
            rows = np.flatnonzero((sub[:, off:off + len(want)] != want).any(axis=1))
            bad += ["frame %d (image %d): %s" % (idx[r], j, name) for r in rows[:limit]]
    return sorted(bad, key=lambda s: int(s.split()[1]))[:limit]
