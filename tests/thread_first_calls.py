"""The first calls of a process, made by four host threads at the same moment (run by tests/test_gpu_threads.py as ONE fresh
child process: the once-per-process paths — the library load of the Python wrapper, spfe_create's first use of the device, and
the launchers that raise a kernel's dynamic-LDS limit on first use (spfe_kernels.h raise_lds_limit) — have long run in a pytest
process).

Four threads each create a handle of their own at one barrier (spfe_create beside itself and beside load_library()).  Then, at
a barrier before each step, every thread makes its first call of the same form:
  extract_batch             conv_f32 / head / cov / the gathered descriptor launchers
  bundle_adjust             ba.hip                    (tests/golden/ba_small.npz)
  refine_pose               pose.hip                  (pose_n10)
  optimize_sim3             sim3opt.hip               (sim3opt_kept10)
  optimize_essential_graph  essgraph.hip              (eg_cases.banded(70, wide_row=True))
  align_dust                dust.hip                  (dust_small on the 8 x 12 map)
Every result must equal, byte for byte, what a fifth handle gives afterwards, alone in the main thread; those are checked
against the host references the tests of these fixtures use (the oracle, ba_ref.c, pose_ref.c, sim3opt_ref.c, eg_ref.c).

Prints one line, "thread-first-calls: PASS" or "thread-first-calls: FAIL: <reasons>", and exits 0 / 1.  A thread still running
at the time limit counts as hung: the verdict says which, and the process ends at once without starting anything more.
usage: python -m tests.thread_first_calls"""
import os
import sys
import tempfile
import threading
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_THREADS = 4
H, W, NF = 64, 96, 100
# the whole sequence of one thread alone takes well under a second on an MI355X (the child as a whole: 2.8 s, most of it
# imports and the C references); the limit only catches a hang
JOIN_TIMEOUT = 120.0
FILL = 0x5A


def steps():
    """-> [(name, call(ext) -> result)] on fixtures loaded once; every thread gets the same arrays (read only)"""
    import graph_forms  # noqa: F401  (puts the reference directories on sys.path)
    import eg_cases
    import test_gpu_essential_graph as tg
    import test_gpu_host_forms_interleaved as hfi
    from sp_orb_slam_amd import synth
    imgs = [synth.make_image(7000 + i, H, W) for i in range(2)]
    eg = eg_cases.banded(70, wide_row=True)

    def extract(ext):
        return [(fr.K, fr.status, fr.kp_xy, fr.occ_grid, fr.descriptors, fr.cov2_inv) for fr in ext.extract_batch(imgs)]
    return [("extract_batch", extract), ("bundle_adjust", hfi.ba(hfi.golden("ba_small"))), ("refine_pose", hfi.pose),
            ("optimize_sim3", hfi.sim3opt), ("optimize_essential_graph", lambda ext: tg.host_form(ext, eg)), ("align_dust", hfi.dust)], imgs, eg


def against_references(ext, got, imgs, eg, blob):
    """the fifth handle's results against the host references of these fixtures, as their own tests compare them"""
    import ba_ref
    import eg_ref
    import pose_ref
    import sim3opt_ref
    import test_gpu_dust as td
    import test_gpu_essential_graph as tg
    import test_gpu_host_forms_interleaved as hfi
    import test_gpu_local_ba as tb
    import test_gpu_optimize_sim3 as tos
    import test_gpu_pose_refine as tp
    from oracle import oracle
    tmp = lambda name: tempfile.mkdtemp(prefix="thread_first_calls_%s_" % name)   # noqa: E731
    for fr, im in zip(got["extract_batch"], imgs):
        ref = oracle.extract(blob, im, NF)
        assert fr[0] == ref["K"] > 10 and fr[1] == 0 and np.array_equal(fr[2], ref["kp_xy"]) and np.array_equal(fr[3], ref["occ_grid"])
        assert np.array_equal(fr[4].view(np.uint32), ref["desc"].view(np.uint32)), "descriptor bits against the oracle"
        assert np.array_equal(fr[5].view(np.uint32), ref["cov2_inv"].view(np.uint32)), "cov2_inv bits against the oracle"
    _, _, blk = tb.same_as_reference(types.SimpleNamespace(ext=ext, ref=ba_ref.build(tmp("ba_ref"))), hfi.golden("ba_small"), "ba_small")
    assert blk.tobytes() == bytes(got["bundle_adjust"]), "the block compared with ba_ref.c is the one the threads are held to"
    g = hfi.golden("pose_n10")
    tp.same(got["refine_pose"], pose_ref.solve(pose_ref.build(tmp("pose_ref")), g["obs"], g["w"], g["pts"], g["Tcw_init"], g["intr"],
                                               pose_ref.DUST_POST))
    g = hfi.golden("sim3opt_kept10")
    L = sim3opt_ref.build(tmp("sim3opt_ref"))
    i1, i2 = tos.intr_of(g)
    raw, kcap = got["optimize_sim3"]
    tos.same(ext.decode_sim3opt_out(raw, kcap), sim3opt_ref.solve(L, g, sim3opt_ref.params(i1, i2, fix_scale=int(g["fix_scale"]))),
             g["Tcw2"], g["mp2"], L, "sim3opt_kept10")
    tg.same(got["optimize_essential_graph"], eg_ref.solve(eg_ref.build(tmp("eg_ref")), eg, env_cap=tg.cap_of(eg), fill=tg.FILL),
            len(eg["flags"]), "banded(70)")
    g = hfi.golden("dust_small")                        # the map and intrinsics as hfi.dust samples them down to 8 x 12 cells
    fx, fy, cx, cy = [float(v) for v in g["intr"]]
    hc, wc = H // 8, W // 8
    sy, sx = hc / g["dust"].shape[0], wc / g["dust"].shape[1]
    m = np.ascontiguousarray(g["dust"][(np.arange(hc) / sy).astype(int)][:, (np.arange(wc) / sx).astype(int)])
    r = oracle.align_dust(m, g["pts"], g["Tcw_init"], fx * sx, fy * sy, (cx - 3.5) * sx + 3.5, (cy - 3.5) * sy + 3.5)
    td._compare(got["align_dust"], r, m)
    assert r["iterations"] >= 2 and r["n_inlier"] > 0


def main():
    import thread_forms as tf
    import test_gpu_host_forms_interleaved as hfi
    from sp_orb_slam_amd import weights
    from sp_orb_slam_amd import extractor as X
    blob = weights.synthetic(7, "dense")
    forms, imgs, eg = steps()
    assert X._lib is None, "the library is loaded by the threads, not before them"
    exts, results = [None] * N_THREADS, [dict() for _ in range(N_THREADS)]
    step = threading.Barrier(N_THREADS)

    def worker(i):
        def f(r):
            try:
                step.wait(JOIN_TIMEOUT)
                if r == 0:
                    exts[i] = X.SPExtractor(NF, H, W, blob, max_batch=2, with_heat=False)
                else:
                    name, call = forms[r - 1]
                    results[i][name] = call(exts[i])
            except BaseException:
                step.abort()
                raise
        return f

    def hung(message):                                   # nothing more is started: no close, no fifth handle
        print("thread-first-calls: FAIL: %s" % message, flush=True)
        os._exit(1)
    failures = []
    try:
        tf.run_side_by_side([worker(i) for i in range(N_THREADS)], 1 + len(forms), JOIN_TIMEOUT,
                            ["thread %d" % i for i in range(N_THREADS)], on_hang=hung)
    except tf.WorkerFailed as e:
        print(e, file=sys.stderr)
        failures.append("a thread raised: %s" % str(e.__cause__).splitlines()[0][:300] if str(e.__cause__) else "a thread raised")
    if not failures:
        fifth = X.SPExtractor(NF, H, W, blob, max_batch=2, with_heat=False)
        alone = {name: call(fifth) for name, call in forms}
        want = {name: hfi.flat(v) for name, v in alone.items()}
        for i in range(N_THREADS):
            for name, _ in forms:
                got = hfi.flat(results[i][name])
                if [p for p, _ in got] != [p for p, _ in want[name]]:
                    failures.append("thread %d: %s returns another shape" % (i, name))
                    continue
                failures += ["thread %d: %s %s differs from the fifth handle's" % (i, name, p)
                             for (p, g), (_, w) in zip(got, want[name]) if g != w]
        try:
            against_references(fifth, alone, imgs, eg, blob)
        except AssertionError as e:
            import traceback
            traceback.print_exc()
            failures.append("the fifth handle against the host references: %s" % (str(e).splitlines()[0][:300] if str(e) else "assertion"))
        fifth.close()
    for e in exts:
        if e is not None:
            e.close()
    if failures:
        print("thread-first-calls: FAIL: %s" % " | ".join(failures[:8]), flush=True)
        return 1
    print("thread-first-calls: PASS", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
