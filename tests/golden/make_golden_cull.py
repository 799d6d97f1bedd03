"""Writes the fixtures tests/golden/cull_*.npz: the named cases of tests/cull_ref/cull_cases.py with what tests/cull_ref/cull_ref.c
gives for them — the block on a background of 0xA5 and the whole world after the call (table rows never written keep 0xA5).

    python tests/golden/make_golden_cull.py
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests", "cull_ref"))
import cull_cases  # noqa: E402
import cull_ref  # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as tmp:
        L = cull_ref.build(tmp)
        for name, c in cull_cases.named_cases().items():
            w, r = cull_ref.run_case(L, c)
            out = {k: np.asarray(c[k]) for k in cull_cases.KEYS}
            out["e_block"] = r["block"]
            out.update({"e_" + k: w[k] for k in cull_ref.WORLD})
            path = os.path.join(ROOT, "tests", "golden", "cull_%s.npz" % name)
            np.savez_compressed(path, **out)
            nl = r["n_listed"]
            print("%-42s status %2d passes %d codes %s culled %s events %s bad %s  %5d bytes" % (
                name, r["status"], r["n_passes"], r["entry_code"][:nl].tolist(), r["culled_slot"][:r["n_culled"]].tolist(),
                list(zip(r["event_child"][:r["n_events"]].tolist(), r["event_parent"][:r["n_events"]].tolist())),
                r["bad_point"][:r["n_bad_stored"]].tolist(), os.path.getsize(path)))


if __name__ == "__main__":
    main()
