"""CPU: bench.py's --dump-outputs writer (dump_outputs) on canned records, and the options a plain run and a --full run
are told apart by.  The GPU form — a plain run's dump against the oracle — is tests/test_gpu_bench_plain.py."""
import os
import subprocess
import sys

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Rec:
    def __init__(self, K, hc, wc, seed):
        rng = np.random.default_rng(seed)
        self.K, self.n_candidates, self.status = K, K + 5, 0
        self.kp_xy = rng.integers(0, 64, (K, 2)).astype(np.float32)
        self.response = rng.random(K, dtype=np.float32)
        self.descriptors = rng.standard_normal((K, 256), dtype=np.float32)
        self.cov2 = rng.random((K, 2), dtype=np.float32)
        self.cov2_inv = rng.random((K, 2), dtype=np.float32)
        self.occ_grid = rng.integers(-1, K, (hc, wc)).astype(np.int16)
        self.dense_dust = rng.random((hc, wc), dtype=np.float32)
        self.semi_dust = rng.random((hc, wc), dtype=np.float32)


class _Sharded:
    """What dump_outputs reads of a ShardedExtractor: decode(frame) -> the frame's record."""

    def __init__(self, n, kmax, hc, wc):
        self.n, self.kmax, self.hc, self.wc = n, kmax, hc, wc

    def decode(self, frame):
        assert 0 <= frame < self.n
        return _Rec(1 + (7 * frame) % self.kmax, self.hc, self.wc, frame)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_outputs_writes_every_frame_padded_in_float(tmp_path):
    sh = _Sharded(5, 11, 6, 8)
    bench.dump_outputs(sh, 5, 11, str(tmp_path / "out"))
    a = _load(str(tmp_path / "out"))
    assert set(a) == {"frame_index", "keypoint_count", "n_candidates", "status", "kp_xy", "response", "descriptors", "cov2",
                      "cov2_inv", "occ_grid", "dense_dust", "semi_dust"}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert a["frame_index"].tolist() == [0, 1, 2, 3, 4]
    assert a["descriptors"].shape == (5, 11, 256) and a["occ_grid"].shape == (5, 6, 8)
    for f in range(5):
        r = sh.decode(f)
        assert a["keypoint_count"][f] == r.K and a["n_candidates"][f] == r.n_candidates
        assert np.array_equal(a["kp_xy"][f, :r.K], r.kp_xy) and not a["kp_xy"][f, r.K:].any()
        assert np.array_equal(a["descriptors"][f, :r.K].view(np.uint32), r.descriptors.view(np.uint32))
        assert not a["descriptors"][f, r.K:].any()
        assert np.array_equal(a["occ_grid"][f], r.occ_grid.astype(np.float32))
        assert np.array_equal(a["dense_dust"][f], r.dense_dust)


def test_dump_outputs_samples_a_large_batch_with_a_fixed_seed(tmp_path):
    n = 3 * bench.DUMP_MAX_FRAMES
    bench.dump_outputs(_Sharded(n, 4, 2, 2), n, 4, str(tmp_path / "a"))
    bench.dump_outputs(_Sharded(n, 4, 2, 2), n, 4, str(tmp_path / "b"))
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    idx = a["frame_index"]
    assert len(idx) == bench.DUMP_MAX_FRAMES and len(set(idx.tolist())) == len(idx) and idx.max() < n
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_dump_outputs_stays_under_the_size_limit(tmp_path):
    # 7680x4320 maps and 1001 keypoints a frame: the sample shrinks until the files fit
    n, kmax, hc, wc = 64, 1001, 540, 960
    sh = _Sharded(n, kmax, hc, wc)
    bench.dump_outputs(sh, n, kmax, str(tmp_path))
    total = sum(os.path.getsize(os.path.join(str(tmp_path), f)) for f in os.listdir(str(tmp_path)))
    assert total <= bench.DUMP_LIMIT_BYTES + 4096 * 12   # (+ the .npy headers)
    assert 0 < len(np.load(os.path.join(str(tmp_path), "frame_index.npy"))) < bench.DUMP_MAX_FRAMES


def test_options_of_a_plain_and_a_full_run():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0
    assert "--full" in out.stdout and "--dump-outputs" in out.stdout and "--steps" in out.stdout
