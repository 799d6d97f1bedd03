"""CPU: what the frame schedule (csrc/spfe_schedule.hip + conv_plan.h) issues, held against a recording.

tests/hoststub/schedule_trace.cpp drives the library's host code over the stub HIP runtime through 103 configurations
(sizes, batches, precisions, call forms, one environment switch each), three calls each, and prints every launch (kernel with
template arguments, grid, block, LDS, stream; of a
convolution also the geometry and buffer offsets of its parameter block), every event record, wait and
query and every asynchronous copy, with streams and events as indices.  tests/golden/schedule_trace.txt.gz is that output as
commit 320aa1d produced it (the same driver and stub built against that commit's csrc); the working tree must print the same
bytes.  A difference is a changed launch, grid, instantiation, stream or ordering call: a bug, or a deliberate change of the
schedule, which then records a new trace and says so.

tests/hoststub/plan_check.cpp builds with a plain C++ compiler and no HIP include path, plans all ten layers of the default
sections with conv_plan.h alone and holds the plans (half batches included) against the launches of the same recording.

Measured on an 8-core host: the host-only build 15 s (make -j8), the driver 1.1 s, plan_check's build and run 1.2 s."""
import gzip
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "hoststub")
GOLDEN = os.path.join(ROOT, "tests", "golden", "schedule_trace.txt.gz")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def golden():
    with gzip.open(GOLDEN, "rb") as f:
        return f.read()


def test_schedule_trace_equals_the_recording(golden, tmp_path):
    if not os.path.exists(HIPCC) or shutil.which("make") is None:
        pytest.skip("hipcc (%s) or make is missing: the host-only build cannot be made" % HIPCC)
    subprocess.run(["make", "-C", STUB, "-j8", "trace", "HIPCC=" + HIPCC], check=True, timeout=300,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    sys.path.insert(0, ROOT)
    from sp_orb_slam_amd import weights
    blob = str(tmp_path / "dense7.spfw")
    weights.save(blob, weights.synthetic(7, "dense"))
    env = {k: v for k, v in os.environ.items() if not k.startswith("SPFE_")}
    p = subprocess.run([os.path.join(STUB, "build", "trace", "schedule_trace"), blob], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=60, env=env)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:] + p.stdout.decode(errors="replace")[-2000:]
    if p.stdout != golden:
        got, want = p.stdout.decode().splitlines(), golden.decode().splitlines()
        at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        section = next((l for l in reversed(want[:at + 1]) if l.startswith("==")), "?")
        call = next((l for l in reversed(want[:at + 1]) if l.startswith("--") or l.startswith("==")), "?")
        pytest.fail("the schedule differs from the recording at line %d (%d lines against %d)\n  in %s / %s\n  recorded: %s\n  now:      %s"
                    % (at + 1, len(got), len(want), section, call, want[at] if at < len(want) else "<end>", got[at] if at < len(got) else "<end>"))


def test_planner_alone_matches_the_recorded_launches(golden, tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe, trace = str(tmp_path / "plan_check"), str(tmp_path / "schedule_trace.txt")
    # (no HIP include path: conv_plan.h is plain C++)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "sp_orb_slam_amd", "csrc"),
                    os.path.join(STUB, "plan_check.cpp"), "-o", exe], check=True, timeout=120)
    with open(trace, "wb") as f:
        f.write(golden)
    p = subprocess.run([exe, trace], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    assert " 0 mismatches" in p.stdout, p.stdout[-4000:]
