"""CPU: the row split and the row walk of csrc/resident_rows.h — the scalar head in front of a keyframe row's first 16-byte
boundary, the 16-byte loads, the scalar tail, all inside [row, row + stride) — which lm_vote_kernel, mp_rows_kernel and
lba_scan_kernel share.  tests/hoststub/row_walk_check.cpp builds with a plain C++ compiler and no HIP include path and runs the
header's own walk thread by thread: row bases 0, 4, 8 and 12 bytes off a boundary, strides 1 .. 67, 101, 1000 and 1001, 64 and 256
threads a row, the plain and the uniform variant.  It holds head <= 3 and <= stride, the vectors on a boundary, a tail shorter than
a vector, and every entry visited exactly once and nothing outside the row."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "hoststub")


def test_row_walk_visits_every_entry_once_and_nothing_else(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "row_walk_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "sp_orb_slam_amd", "csrc"),
                    os.path.join(STUB, "row_walk_check.cpp"), "-o", exe], check=True, timeout=120)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    assert "280 rows, 0 failed checks" in p.stdout, p.stdout[-4000:]
