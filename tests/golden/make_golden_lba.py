"""Writes the fixtures tests/golden/lba_*.npz: the small named cases of tests/lba_ref/lba_cases.py (fixture_names()) with what
tests/lba_ref/lba_ref.c gives for them — the block and the whole world after the call.

    python tests/golden/make_golden_lba.py
"""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests", "lba_ref"))
import lba_cases  # noqa: E402
import lba_ref  # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as tmp:
        L = lba_ref.build(tmp)
        cases = lba_cases.named_cases()
        for name in lba_cases.fixture_names():
            c = cases[name]
            w, r = lba_cases.run_ref(L, c)
            path = os.path.join(ROOT, "tests", "golden", "lba_%s.npz" % name)
            lba_cases.save_fixture(path, c, w, r)
            print("%-45s %s  %6d bytes" % (name, {k: v for k, v in r.items() if isinstance(v, int)}, os.path.getsize(path)))


if __name__ == "__main__":
    main()
