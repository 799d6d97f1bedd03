"""Writes the fixtures tests/golden/mpcull_*.npz: the small named cases of tests/mpcull_ref/mpcull_cases.py (fixture_names()) with
what tests/mpcull_ref/mpcull_ref.c gives for them — the block on a background of 0xA5 and the whole world after the call.

    python tests/golden/make_golden_mpcull.py
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests", "mpcull_ref"))
import mpcull_cases  # noqa: E402
import mpcull_ref  # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as tmp:
        L = mpcull_ref.build(tmp)
        cases = mpcull_cases.named_cases()
        for name in mpcull_cases.fixture_names():
            c = cases[name]
            w, r = mpcull_cases.run_ref(L, c)
            out = {k: np.asarray(v) for k, v in c.items()}
            out["e_block"] = r["block"]
            out.update({"e_" + k: w[k] for k in mpcull_ref.WORLD})
            path = os.path.join(ROOT, "tests", "golden", "mpcull_%s.npz" % name)
            np.savez_compressed(path, **out)
            print("%-40s %s  %6d bytes" % (name, {k: v for k, v in r.items() if isinstance(v, int)}, os.path.getsize(path)))


if __name__ == "__main__":
    main()
