"""Writes the fixtures tests/golden/newkf_*.npz: the small named cases of tests/newkf_ref/newkf_cases.py (fixture_names()) with
what tests/newkf_ref/newkf_ref.c gives for them — the block on a background of 0xA5 and the whole world after the call.  An array a
case does not have (no index array, no record, no track table) is stored as a bool scalar.

    python tests/golden/make_golden_newkf.py
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests", "newkf_ref"))
import newkf_cases  # noqa: E402
import newkf_ref  # noqa: E402

NONE = np.zeros((), bool)


def main():
    with tempfile.TemporaryDirectory() as tmp:
        L = newkf_ref.build(tmp)
        cases = newkf_cases.named_cases()
        for name in newkf_cases.fixture_names():
            c = cases[name]
            w, r = newkf_cases.run_ref(L, c)
            out = {k: NONE if v is None else np.asarray(v) for k, v in c.items()}
            out["e_block"] = r["block"]
            out.update({"e_" + k: NONE if w[k] is None else w[k] for k in newkf_ref.WORLD})
            path = os.path.join(ROOT, "tests", "golden", "newkf_%s.npz" % name)
            np.savez_compressed(path, **out)
            print("%-40s %s  %6d bytes" % (name, {k: v for k, v in r.items() if isinstance(v, int)}, os.path.getsize(path)))


if __name__ == "__main__":
    main()
