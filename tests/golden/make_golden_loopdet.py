"""Writes the fixtures tests/golden/loopdet_*.npz: the named cases of tests/loopdet_ref/loopdet_cases.py (generated from fixed
seeds) with the block tests/loopdet_ref/loopdet_ref.c gives for them on a background of 0xA5, decoded.  The margins of every case
are asserted on the way (loopdet_cases.check_margins).

    python tests/golden/make_golden_loopdet.py
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests", "loopdet_ref"))
import loopdet_cases  # noqa: E402
import loopdet_ref  # noqa: E402

EXPECTED = loopdet_ref.LISTS + loopdet_ref.FLOATS


def main():
    with tempfile.TemporaryDirectory() as tmp:
        L = loopdet_ref.build(tmp)
        for name, make in loopdet_cases.CASES.items():
            c = make().arrays()
            r = loopdet_ref.detect(L, c)
            loopdet_cases.check_margins(c, r)
            out = {k: c[k] for k in loopdet_cases.KEYS}
            out.update({"e_" + k: r[k] for k in EXPECTED})
            out["e_header"] = np.array([r[k] for k in loopdet_ref.INTS], np.int32)
            out["e_scores"] = np.array([r[k] for k in loopdet_ref.SCORES], np.float32)
            path = os.path.join(ROOT, "tests", "golden", "loopdet_%s.npz" % name)
            np.savez_compressed(path, **out)
            print("%-16s n %3d  scored %3d  pass %3d  cand %s  status %d  min %.4f  %5d bytes" % (
                name, len(c["gdesc"]), r["n_scored"], r["n_pass"], r["cand_slot"].tolist(), r["status"], r["min_score"],
                os.path.getsize(path)))


if __name__ == "__main__":
    main()
