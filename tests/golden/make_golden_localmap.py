"""Writes the fixtures tests/golden/localmap_*.npz: the named cases of tests/localmap_ref/localmap_cases.py with the block
tests/localmap_ref/localmap_ref.c gives for them on a background of 0xA5, whole and decoded.

    python tests/golden/make_golden_localmap.py
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests", "localmap_ref"))
import localmap_cases  # noqa: E402
import localmap_ref  # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as tmp:
        L = localmap_ref.build(tmp)
        for name, c in localmap_cases.named_cases().items():
            r = localmap_ref.update(L, c)
            out = {k: np.asarray(c[k]) for k in localmap_cases.KEYS}
            out["e_header"] = np.array([r[k] for k in localmap_ref.FIELDS], np.int32)
            out["e_local_kf"], out["e_point_idx"], out["e_block"] = r["local_kf"], r["point_idx"], r["block"]
            path = os.path.join(ROOT, "tests", "golden", "localmap_%s.npz" % name)
            np.savez_compressed(path, **out)
            print("%-24s voted %d  local %s  ref %2d  points %s  status %d  %5d bytes" % (
                name, r["n_voted"], r["local_kf"].tolist(), r["ref_slot"], r["point_idx"][:r["n_points"]].tolist(), r["status"],
                os.path.getsize(path)))


if __name__ == "__main__":
    main()
