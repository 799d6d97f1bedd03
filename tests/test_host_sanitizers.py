"""CPU: the library's host code (csrc/spfe_*.hip, spfe_host.h) under AddressSanitizer + UndefinedBehaviorSanitizer and under
ThreadSanitizer, as a stand-alone program over a stub HIP runtime (tests/hoststub/: hip_stub.cpp is the runtime on the CPU,
host_main.cpp the driver with one scenario per test, the Makefile builds both configurations host-only with the sanitizer
runtimes linked statically).  "Device" memory is exactly-sized heap memory there, so every copy the host code issues is checked
on both sides: by the stub's registry of live ranges and by the sanitizer's red zones.  Kernels do not run.

A test runs one scenario of one configuration as a child process and asks for exit status 0 (every check of the driver held and
the stub counted no violation) and an output free of sanitizer reports.  Nothing is preloaded and no variable that loads a
library is set.

Measured on an 8-core build host (seconds of wall time): the build of both configurations 16.3 (make -j8);
              lifecycle  host_calls  pipeline  host_forms  device_forms  alloc_failure  threads  stub_selfcheck
    asan         3.53       0.32       0.35       1.31        0.08           3.24        0.11        0.02
    tsan        13.52       0.95       1.67       6.45        0.14          11.52        0.31        0.04
(lifecycle is the issue's whole product, 120 creates; a create packs the 1.3 M weights, 0.11 s under the thread sanitizer
whatever the frame size, so that one limit comes to 68 s.)
Each limit below is five times the measured value (the hosts that run the suite are shared), two seconds at the least."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "hoststub")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ROCM = os.path.dirname(os.path.dirname(os.path.abspath(HIPCC)))
BUILD_LIMIT = 5 * 16.3

SCENARIOS = ["lifecycle", "host_calls", "pipeline", "host_forms", "device_forms", "alloc_failure", "threads", "stub_selfcheck"]
# measured seconds per (configuration, scenario); the limit is five times that
MEASURED = {
    "asan": dict(zip(SCENARIOS, [3.53, 0.32, 0.35, 1.31, 0.08, 3.24, 0.11, 0.02])),
    "tsan": dict(zip(SCENARIOS, [13.52, 0.95, 1.67, 6.45, 0.14, 11.52, 0.31, 0.04])),
}
REPORTS = ("AddressSanitizer", "LeakSanitizer", "ThreadSanitizer", "runtime error:")


def _static_runtime(name):
    """the static sanitizer runtime archive of the toolchain, or None"""
    for base, _dirs, files in os.walk(os.path.join(ROCM, "lib", "llvm", "lib", "clang")):
        if "libclang_rt.%s-x86_64.a" % name in files:
            return os.path.join(base, "libclang_rt.%s-x86_64.a" % name)
    return None


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    if not os.path.exists(HIPCC) or shutil.which("make") is None:
        pytest.skip("hipcc (%s) or make is missing: the host-only sanitizer build cannot be made" % HIPCC)
    for rt in ("asan", "tsan"):
        if _static_runtime(rt) is None:
            pytest.skip("the toolchain ships no static %s runtime (libclang_rt.%s-x86_64.a)" % (rt, rt))
    subprocess.run(["make", "-C", STUB, "-j8", "all", "HIPCC=" + HIPCC], check=True, timeout=BUILD_LIMIT,
                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    sys.path.insert(0, ROOT)
    from sp_orb_slam_amd import weights
    d = tmp_path_factory.mktemp("hoststub")
    blob = weights.synthetic(7, "dense")
    f32 = str(d / "dense7.spfw")
    weights.save(f32, blob)
    # the same weights rounded to bf16 values: the blob a bf16 deployment ships
    import numpy as np
    u = blob.astype(np.float32).view(np.uint32).astype(np.uint64)
    rounded = (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
    bf16 = str(d / "dense7_bf16.spfw")
    weights.save(bf16, rounded)
    return {"f32": f32, "bf16": bf16}


@pytest.mark.parametrize("scenario", SCENARIOS)
@pytest.mark.parametrize("config", ["asan", "tsan"])
def test_host_code_under_sanitizer(built, config, scenario):
    exe = os.path.join(STUB, "build", config, "host_main")
    env = {k: v for k, v in os.environ.items() if not k.startswith("SPFE_")}   # (the library's switches at their defaults)
    if config == "asan":
        env["ASAN_OPTIONS"] = "detect_leaks=1"
    # the bf16-valued blob for the scenario that is mostly about the bf16 twin, the f32 one elsewhere: the host code reads both alike
    blob = built["bf16"] if scenario == "pipeline" else built["f32"]
    limit = max(2.0, 5 * MEASURED[config][scenario])
    p = subprocess.run([exe, scenario, blob], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=limit, env=env, text=True, errors="replace")
    tail = "\n".join(p.stdout.splitlines()[-60:])
    assert p.returncode == 0, "%s %s: exit status %d\n%s" % (config, scenario, p.returncode, tail)
    for word in REPORTS:
        assert word not in p.stdout, "%s %s: a %s report\n%s" % (config, scenario, word, tail)
    assert "%s: ok" % scenario in p.stdout, tail
