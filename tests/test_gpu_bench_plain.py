"""GPU: a plain `python bench.py --gpus 1 --steps K --warmup W` run — the headline and nothing else — and what its
--dump-outputs writes: the records of the last timed step, every frame against the oracle's extraction of it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    from oracle import oracle
    from sp_orb_slam_amd import synth, weights

    H, W, B, nf = 128, 160, 3, 100
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
                          "--height", str(H), "--width", str(W), "--frames-per-gpu", str(B), "--num-features", str(nf),
                          "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 4 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["dtype"] == "f32"
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0 and abs(d["value"] - B * 1e3 / d["ms_per_step"]) <= 1e-3 * d["value"] + 0.05
    for leg in ("stage_ms", "latency_batch1_ms", "host_path", "cpu_baseline", "parity_frame0", "match_bruteforce"):
        assert leg not in d, leg        # (those are --full's)

    a = {f[:-4]: np.load(os.path.join(str(tmp_path), f)) for f in os.listdir(str(tmp_path))}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert a["frame_index"].tolist() == list(range(B)) and a["descriptors"].shape == (B, nf + 1, 256)
    blob = weights.synthetic(7, "dense")
    for f in range(B):
        ref = oracle.extract(blob, synth.make_image(200 + f, H, W), nf)
        K = int(a["keypoint_count"][f])
        assert K == ref["K"] and a["status"][f] == 0
        assert np.array_equal(a["kp_xy"][f, :K], ref["kp_xy"])
        assert np.array_equal(a["descriptors"][f, :K].view(np.uint32), ref["desc"].view(np.uint32))
        assert np.array_equal(a["cov2_inv"][f, :K].view(np.uint32), ref["cov2_inv"].view(np.uint32))
        assert np.array_equal(a["occ_grid"][f], ref["occ_grid"].astype(np.float32))
