"""GPU: calls of hundreds to 65,535 frames — whole-call offsets past 2^31 and 2^32 bytes, the largest gridDim.y, unequal half
batches, the gathered heads at cell indices up to the whole-call limit — and the limit itself (spfe_config::max_batch,
include/spfe.h: at most 65,535 frames and max_batch * cells * R < 2^31, R = 2048 bytes in f32, 1024 in bf16).

A call of B frames carries seven distinct images, frame i image (i + rot) mod 7 (tests/many_frames.py, which also proves on the
CPU that an offset wrapped at 2^31 or 2^32 cannot land on equal data).  Every frame's record is compared BITWISE with the
reference of its image: in f32 the CPU oracle's extraction, in bf16 the records of a seven-frame handle whose own logits the
oracle's post-processing is held to (the layers of such handles are held to float64 by test_gpu_bf16_layers.py).  The logits,
the descriptor map and conv4b's output are read back bitwise for the first frame, the last, and the frames at and beside every
crossing.  Each case makes, on ONE handle: the synchronous host call (not the two edge cases), the device call, the device
call again with the pattern rotated by 3 (claim maps and tile counters carry state between calls), and a call of
max_batch // 2 + 1 frames.

Measured on an MI355X, every case ran (none skipped for memory): device memory the handle took by hipMemGetInfo (and
many_frames.handle_bytes_estimate), seconds of wall time for the whole case with its references (the first case of a process
adds 2 to 4 s of start-up), of which inside the library's three or four calls:
    act0_past_2_32   f32  200x136 x    620      263,500 cells   11.04 GB (11.00)   0.7 s   0.10 s
    max_grid_y       f32   24x16  x 65,535      393,210 cells   14.48 GB (14.46)   1.6 s   0.48 s
    halves_unequal   f32  200x136 x    621      263,925 cells   11.05 GB (11.02)   0.6 s   0.10 s
    act1_past_2_31   bf16 200x136 x  2,470    1,049,750 cells   44.84 GB (44.79)   1.4 s   0.08 s
    edge_f32         f32  200x136 x  2,467    1,048,475 cells   43.68 GB (43.66)   2.3 s   0.26 s
    edge_bf16        bf16 200x136 x  4,934    2,096,950 cells   89.45 GB (89.43)   2.7 s   0.06 s
A frame costs 2.1 MB of covariance overflow lists whatever its size (16 slots x 16,384 pairs) and 8.5 KB a keypoint of queues:
max_grid_y at the default capacities took 156.67 GB and 4.3 s; its frames of 16 rows have no keypoint outside the 8-pixel border,
so the case creates its handle with the smallest capacities (SPFE_COV_CAPS, many_frames.case).  About 40 % of a call's cells are
listed for the gathered heads (852,158 of 2,096,950 in edge_bf16, the largest 2,096,895).  The refusals allocate nothing;
3840x2160 x 16 in bf16 (73.5 GB by the estimate) is created and closed in 4.6 s, x 8 in f32 (35.7 GB) in 0.04 s.
A case skips only when the device's free memory is below 1.5 times the estimate of its handle, with both numbers in the message."""
import time

import numpy as np
import pytest

import many_frames as mf
from oracle import oracle
from sp_orb_slam_amd import weights
from sp_orb_slam_amd.extractor import SPExtractor, SpfeError

pytestmark = pytest.mark.gpu

_BLOB = None
_REFS = {}


def _blob():
    global _BLOB
    if _BLOB is None:
        _BLOB = weights.synthetic(7, "dense")
    return _BLOB


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _references(cs):
    """Once per (precision, frame size, num_features): the seven images, one oracle-style dict per image (the record's
    fields) and per image the (semi, coarse, feat) maps the debug reads are compared with."""
    key = (cs["precision"], cs["H"], cs["W"], cs["nf"])
    if key in _REFS:
        return _REFS[key]
    H, W, nf = cs["H"], cs["W"], cs["nf"]
    imgs = mf.images(cs)
    assert len({im.tobytes() for im in imgs}) == mf.K_IMAGES
    refs, nets = [], []
    if cs["precision"] == "f32":
        for im in imgs:
            semi, coarse, feat = oracle.network(_blob(), im)
            refs.append(oracle.postprocess(semi, coarse, H, W, nf))
            nets.append((semi, coarse, feat))
    else:
        ext = SPExtractor(nf, H, W, _blob(), max_batch=mf.K_IMAGES, precision="bf16", with_heat=False)
        try:
            frs = ext.extract_batch(imgs)
            for j, fr in enumerate(frs):
                nets.append(tuple(ext.debug_read(n, j) for n in ("semi", "coarse", "feat")))
                _own_logits(fr, nets[j][0], nets[j][1], H, W, nf)
                refs.append(mf.record_as_ref(fr))
        finally:
            ext.close()
    assert all(r["K"] > 0 for r in refs) or H <= 16   # (16 rows: every pixel lies in the 8-pixel border, the per-cell maps remain)
    assert len({np.asarray(r["kp_xy"]).tobytes() + _bits(r["dense_dust"]).tobytes() for r in refs}) == mf.K_IMAGES
    _REFS[key] = (imgs, refs, nets)
    return _REFS[key]


def _own_logits(fr, semi, coarse, H, W, nf):
    """bf16: everything behind the logits equals the oracle's post-processing of the GPU's own logits."""
    ref = oracle.postprocess(semi, coarse, H, W, nf)
    assert fr.status == 0 and fr.K == ref["K"] and fr.n_candidates == ref["n_candidates"]
    assert np.array_equal(fr.kp_xy, ref["kp_xy"]) and np.array_equal(fr.occ_grid, ref["occ_grid"])
    assert np.array_equal(_bits(fr.descriptors), _bits(ref["desc"]))
    assert np.array_equal(_bits(fr.cov2_inv), _bits(ref["cov2_inv"]))
    assert np.array_equal(_bits(fr.dense_dust), _bits(ref["dense_dust"]))


def _free_or_skip(need, what):
    import torch
    torch.cuda.empty_cache()
    free, _total = torch.cuda.mem_get_info()
    if free < 1.5 * need:
        pytest.skip("%s: %d bytes of device memory are free, the handle needs about %d (1.5 x that is asked for)" % (what, free, need))
    return free


def _run_case(name, monkeypatch):
    import torch
    cs = mf.case(name)
    if cs["cov_caps"]:
        monkeypatch.setenv("SPFE_COV_CAPS", "%d,%d,%d" % cs["cov_caps"])
    else:
        monkeypatch.delenv("SPFE_COV_CAPS", raising=False)
    mf.check_case(cs, 3)
    _, read_back = mf.check_case(cs, 0)            # the CPU proof first: nothing below runs on a pattern that could hide a wrap
    H, W, nf, B, bf16 = cs["H"], cs["W"], cs["nf"], cs["B"], cs["precision"] == "bf16"
    t_case = time.perf_counter()
    imgs, refs, nets = _references(cs)
    need = mf.handle_bytes_estimate(cs)
    free = _free_or_skip(need, name)
    t_lib = 0.0
    ext = SPExtractor(nf, H, W, _blob(), max_batch=B, precision=cs["precision"], with_heat=False, async_cov=cs["async_cov"])
    try:
        torch.cuda.synchronize()
        took = free - torch.cuda.mem_get_info()[0]
        rb = ext.record_bytes()
        assert rb == mf.record_layout(nf, H, W)["bytes"] == int(ext.layout.bytes)
        fields = [mf.reference_fields(ext.layout, r) for r in refs]
        d_img7 = torch.from_numpy(np.stack(imgs)).cuda()
        d_rec = torch.zeros(B * rb, dtype=torch.uint8, device="cuda")

        def device_call(n, rot):
            nonlocal t_lib
            d = d_img7[(torch.arange(n, device="cuda") + rot) % mf.K_IMAGES].contiguous()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ext.wait_records(ext.extract_batch_device(d.data_ptr(), n, d_rec.data_ptr()))
            torch.cuda.synchronize()
            t_lib += time.perf_counter() - t0
            recs = d_rec[:n * rb].cpu().numpy().reshape(n, rb)
            bad = mf.mismatches(recs, fields, rot)
            assert not bad, "%s: device call of %d frames, rotation %d: %s" % (name, n, rot, bad)
            return recs

        if cs["host_form"]:
            t0 = time.perf_counter()
            recs = mf.host_call(ext, imgs, B, 0)
            t_lib += time.perf_counter() - t0
            bad = mf.mismatches(recs, fields, 0)
            assert not bad, "%s: host call of %d frames: %s" % (name, B, bad)
        recs = device_call(B, 0)
        if cs["async_cov"]:
            assert ext.debug_read("split_streams")[1] == 1, "the call did not run as two half batches"
        # the gathered heads: convDa and convDb ran on the listed cells, and the list reaches into the call's last frame
        gathered, total = int(ext.debug_read("da_gathered")[0]), int(ext.debug_read("db_total")[0])
        listed = ext.debug_read("db_list")[:max(total, 0)]
        print("\nmany_frames %s: convDa gathered %d, %d cells of %d listed, the largest %d" %
              (name, gathered, total, B * mf.cells(H, W), listed.max() if total > 0 else -1))
        if name.startswith("edge_"):
            assert gathered == 1 and 0 < total <= len(listed)
            assert listed.min() >= 0 and (B - 1) * mf.cells(H, W) <= listed.max() < B * mf.cells(H, W)
        for f in read_back:
            want = nets[mf.image_of(f, 0)]
            for k, buf in enumerate(("semi", "coarse", "feat")):
                got = ext.debug_read(buf, f)
                assert np.array_equal(_bits(got), _bits(want[k])), "%s: %s of frame %d" % (name, buf, f)
            if bf16:
                _own_logits(ext.view_record(recs[f]), ext.debug_read("semi", f), ext.debug_read("coarse", f), H, W, nf)
        device_call(B, 3)
        device_call(B // 2 + 1, 5)
    finally:
        ext.close()
    print("\nmany_frames %s: %s %dx%d x %d (%d cells a call), handle %.2f GB of device memory (estimate %.2f), case %.1f s, "
          "library calls %.2f s" % (name, cs["precision"], W, H, B, B * mf.cells(H, W), took / 1e9, need / 1e9,
                                    time.perf_counter() - t_case, t_lib))


@pytest.mark.parametrize("name", list(mf.CASES))
def test_many_frames(monkeypatch, name):
    _run_case(name, monkeypatch)


# ---- the whole-call limit: refused before anything is allocated, with the limit in the message ------------------------------

def _refused(H, W, precision, max_batch):
    import torch
    free = torch.cuda.mem_get_info()[0]
    with pytest.raises(SpfeError) as e:
        SPExtractor(8, H, W, _blob(), max_batch=max_batch, precision=precision, with_heat=False)
    assert torch.cuda.mem_get_info()[0] >= free - (64 << 20)   # (nothing was allocated: the runtime's own pools at the most)
    return str(e.value)


def test_more_frames_than_grid_y_are_refused():
    msg = _refused(16, 16, "f32", 65536)
    assert "SPFE_EINVAL" in msg and "65535" in msg and "precision is 65535" in msg


@pytest.mark.parametrize("H,W", [(136, 200), (2160, 3840)])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_largest_max_batch_plus_one_is_refused(H, W, precision):
    largest = mf.largest_max_batch(H, W, precision)
    assert largest == {(136, "f32"): 2467, (136, "bf16"): 4934, (2160, "f32"): 8, (2160, "bf16"): 16}[(H, precision)]
    msg = _refused(H, W, precision, largest + 1)
    assert "SPFE_EINVAL" in msg and "max_batch %d " % (largest + 1) in msg
    assert "65535" in msg and "2^31" in msg and "precision is %d" % largest in msg


@pytest.mark.parametrize("precision,max_batch", [("f32", 8), ("bf16", 16)])
def test_the_largest_documented_workloads_are_accepted(precision, max_batch):
    """3840x2160 x 8 in f32 (1,036,800 cells) and x 16 in bf16: created and closed, no call."""
    cs = dict(precision=precision, H=2160, W=3840, B=max_batch, nf=8)
    _free_or_skip(mf.handle_bytes_estimate(cs), "3840x2160 x %d %s" % (max_batch, precision))
    ext = SPExtractor(8, 2160, 3840, _blob(), max_batch=max_batch, precision=precision, with_heat=False)
    assert ext.max_batch == max_batch and ext.record_bytes() == mf.record_layout(8, 2160, 3840)["bytes"]
    ext.close()
