"""Writes the fixtures tests/golden/covis_*.npz: the named cases of tests/covis_ref/covis_cases.py with what
tests/covis_ref/covis_ref.c gives for them — the block of every call on a background of 0xA5, the state after the last call and the
two tables (rows never written keep 0xA5).

    python tests/golden/make_golden_covis.py
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests", "covis_ref"))
import covis_cases  # noqa: E402
import covis_ref  # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as tmp:
        L = covis_ref.build(tmp)
        for name, c in covis_cases.named_cases().items():
            r = covis_ref.run_case(L, c)
            out = {k: np.asarray(c[k]) for k in covis_cases.KEYS}
            out["e_blocks"], out["e_best_a"], out["e_best_b"] = r["blocks"], r["best_a"], r["best_b"]
            out.update({"e_" + k: r["state"][k] for k in covis_ref.STATE})
            path = os.path.join(ROOT, "tests", "golden", "covis_%s.npz" % name)
            np.savez_compressed(path, **out)
            last = r["results"][-1]
            print("%-30s status %s  linked %s  codes %s  parent %s  %5d bytes" % (
                name, [x["status"] for x in r["results"]], last["linked_slot"][:last["n_linked"]].tolist(),
                last["linked_code"][:last["n_linked"]].tolist(), r["state"]["parent"].tolist(), os.path.getsize(path)))


if __name__ == "__main__":
    main()
