"""Writes the fixtures tests/golden/mp_*.npz: the named cases of tests/mp_ref/mp_cases.py (generated from fixed seeds) with the
outputs tests/mp_ref/mp_ref.c gives for them, on a table and a block filled with 0xA5.  The descriptor rows are stored as bf16
bit patterns: every row is a bf16-representable value.

    python tests/golden/make_golden_mappoint.py
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests", "mp_ref"))
import mp_cases  # noqa: E402
import mp_ref  # noqa: E402

EXPECTED = ("best_obs", "n_good", "best_median", "code", "normal", "dist_range", "desc")


def main():
    with tempfile.TemporaryDirectory() as tmp:
        L = mp_ref.build(tmp)
        for name, make in mp_cases.CASES.items():
            c = make().arrays()
            r = mp_ref.refresh(L, c)
            assert np.array_equal(mp_ref.widen_bf16(mp_ref.to_bf16(c["kf_desc"])).view(np.uint32), c["kf_desc"].view(np.uint32)), name
            out = {k: c[k] for k in mp_cases.KEYS}
            out["kf_desc_bf16"] = mp_ref.to_bf16(c["kf_desc"])
            if c["point_idx"] is not None:
                out["point_idx"] = c["point_idx"]
            out.update({"e_" + k: r[k] for k in EXPECTED})
            out["e_header"] = np.array([r["m"], r["n_desc_written"], r["n_nd_written"], r["status"]], np.int32)
            path = os.path.join(ROOT, "tests", "golden", "mp_%s.npz" % name)
            np.savez_compressed(path, **out)
            print("%-10s m %3d  E %4d  codes %s  %6d bytes" % (name, len(c["ref_slot"]), len(c["obs"]),
                                                               np.bincount(r["code"], minlength=7)[1:], os.path.getsize(path)))


if __name__ == "__main__":
    main()
