"""GPU: distinct handles driven at the same moment from separate host threads (include/spfe.h "Threads").

The reference system runs three host threads — tracking, local mapping, loop closing — and the library has device forms for
the work of all three.  Every other test drives its handles from pytest's main thread, in turn; here each thread has handles
of its own and the calls interleave (tests/thread_forms.py).  What is compared is bytes: every form here is deterministic, so
a call made beside busy neighbours must return exactly what the same call returns alone, and the call made alone is checked
against its host reference first.  A stream or twin picked from the wrong handle, a process-wide counter that loses an
increment or an error text that crosses threads shows as a differing byte or a foreign message.

WHAT THESE TESTS CANNOT BE RELIED ON TO SHOW.  State that two handles share by mistake (a staging buffer, a pinned mirror, a
scratch block) corrupts a call only while the other thread's call touches the same bytes, and at the fixed orders and round
counts here that coincidence is rare.  Measured on an MI355X with libraries built to share on purpose, 100 runs each of
test_host_forms_in_two_threads (the only mutations that cannot send a kernel out of bounds; none exists for the record forms
of test_three_roles_side_by_side, whose scratch holds indices):
  - one pinned result mirror for all handles (the window is the microseconds between a call's D2H copy and its read of
    the mirror): caught in 1 run of 100 ("thread 0, step 13: pose r[outlier] differs from a fresh handle's");
  - one device staging buffer for spfe_align_dust and spfe_refine_pose, whose staged blocks are float data only (the window
    is the whole call, but thread 0 reaches those forms at steps 0, 8 and 13 and thread 1 at steps 4, 9 and 17): 0 of 100.
So a pass says little about cross-handle sharing; a failure is real.  The twin pick inverted (last_caller, spfe_host.h)
fails test_twin_pick_survives_a_busy_neighbour in its first round, alone already: that test holds the pick itself, and
shows a lost increment of the counter only when one falls between the pair's two stamps.

Every case and every solo expectation is made in the main thread before a thread starts, and so is every fixture load of
the host-array forms (Preloaded): a worker's round is spent inside the library.

TIME LIMITS.  They only catch hangs (a thread that is still running then ends the pytest session: nothing further is started
on the GPU), so they are a large multiple of the solo time of the same rounds, measured on an MI355X:
                                              alone, same rounds      threads side by side    limit
  test_three_roles_side_by_side               0.038 s (3 x 6 rounds)  0.031 s                 60 s
  test_extraction_in_two_threads[f32 / bf16]  0.023 / 0.017 s (2 x 4) 0.009 / 0.007 s         60 s
  test_twin_pick_survives_a_busy_neighbour    0.011 s (12 rounds)     0.025 s                 60 s
  test_host_forms_in_two_threads              0.056 s (2 x 18 calls)  0.029 s                 120 s
  test_last_error_is_the_calling_threads      -                       0.012 s (3 x 50)        60 s
  test_handle_on_another_device_...           not measured (it needs two devices)             120 s
  tests/thread_first_calls.py (child)         2.8 s, the whole process with its imports and   300 s (the threads
                                              the four C references                           inside it: 120 s)
Building the cases and the solo expectations of the three roles takes 1.3 s, once per module."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import graph_forms as gf  # noqa: E402  (puts the reference directories on sys.path)
import test_gpu_host_forms_interleaved as hfi  # noqa: E402
import thread_forms as tf  # noqa: E402

from oracle import oracle  # noqa: E402
from sp_orb_slam_amd import synth, weights  # noqa: E402
from sp_orb_slam_amd.extractor import SPExtractor, SpfeError  # noqa: E402

pytestmark = pytest.mark.gpu

H, W, NF = 64, 96, 100
JOIN_TIMEOUT = 60.0           # see the table above
JOIN_TIMEOUT_HOST_FORMS = 120.0
CHILD_TIMEOUT = 300.0


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


# ---- a. the three roles -----------------------------------------------------------------------------------------------------------
ROLES = (("tracker", ("track_motion_model_record", "track_local_map_record")),
         ("local mapper", ("create_map_points_record", "local_ba_records")),
         ("loop closer", ("loop_verify_records", "optimize_essential_graph")))
ROLE_ROUNDS = 6


class Solo:
    """one form of graph_forms.FORMS on a stream: its case, its fixed buffers and, per input set, the bytes of EVERY buffer
    after the call made alone (outputs, and the inputs and in/out arrays the form leaves alone)"""

    def __init__(self, name, stream):
        self.name, self.stream = name, stream
        self.case = case = gf.FORMS[name].build()
        self.held = held = gf.Buffers(case, stream)
        self.want = {}
        for key in ("A", "B"):
            self.want[key] = got = self.call(key)
            for k in held.names:             # what the form does not list as an output it leaves alone
                if k not in case.outputs and not gf.is_out(held.spec_of[key][k]):
                    assert np.array_equal(got[k], held.loaded(key, k)), (name, key, k, "an input changed")
        if case.check is not None:           # the call made alone, against its host reference
            case.check({k: self.want["A"][k] for k in case.outputs})
        same = [k for k in case.outputs if np.array_equal(self.want["A"][k], self.want["B"][k])]
        assert not same, (name, "A and B give the same", same)

    def call(self, key):
        """reload, call, read everything back (as graph_forms.run() does around each of its calls)"""
        self.held.load(key)
        self.case.call(self.held.P, self.stream.cuda_stream)
        return self.held.read(self.held.names)

    def expect(self, key, got, where):
        for k in self.held.names:
            d = np.flatnonzero(got[k] != self.want[key][k])
            assert not len(d), "%s: %s on %s: %r differs from the call made alone in %d byte(s), the first at %d" % (
                where, self.name, key, k, len(d), d[0])


@pytest.fixture(scope="module")
def roles():
    import torch
    t0 = time.monotonic()
    out = []
    for role, names in ROLES:
        stream = torch.cuda.Stream()
        out.append((role, stream, [Solo(n, stream) for n in names]))
    print("three roles: cases and solo expectations built in %.2f s" % (time.monotonic() - t0))
    yield out
    for _, _, solos in out:
        for s in solos:
            s.case.ext.close()


def role_round(solos, r):
    """round r of a role: its forms in turn, each seeing A, B, A / B, A, B"""
    return solos[r % 2], "AB"[(r // 2 + r % 2) % 2]


def test_three_roles_side_by_side(roles):
    t0 = time.monotonic()
    for role, _, solos in roles:                     # the same rounds alone, in turn (also: the time the limit is sized from)
        for r in range(ROLE_ROUNDS):
            s, key = role_round(solos, r)
            s.expect(key, s.call(key), "%s alone, round %d" % (role, r))
    solo = time.monotonic() - t0

    def worker(role, solos):
        def f(r):
            s, key = role_round(solos, r)
            s.expect(key, s.call(key), "%s, round %d" % (role, r))
        return f
    took = tf.run_side_by_side([worker(role, solos) for role, _, solos in roles], ROLE_ROUNDS, JOIN_TIMEOUT, [r for r, _, _ in roles])
    print("three roles: %d rounds alone in turn %.3f s, side by side %.3f s" % (ROLE_ROUNDS, solo, took))


# ---- b. extraction ------------------------------------------------------------------------------------------------------------------
EXT_ROUNDS, EXT_B = 4, 2
FRAME_FIELDS = ("kp_xy", "occ_grid", "descriptors", "cov2_inv")


def frame_bytes(fr):
    return (int(fr.K), int(fr.status)) + tuple(bits(getattr(fr, k)).tobytes() for k in FRAME_FIELDS)


def oracle_bytes(ref):
    return (int(ref["K"]), 0, bits(ref["kp_xy"]).tobytes(), bits(ref["occ_grid"].astype(np.int16)).tobytes(),
            bits(ref["desc"]).tobytes(), bits(ref["cov2_inv"]).tobytes())


@pytest.fixture(scope="module")
def extraction_images():
    """images[thread][round][frame], all different, and the oracle's result for each (CPU)"""
    blob = weights.synthetic(7, "dense")
    imgs = [[[synth.make_image(4000 + 100 * t + 10 * r + i, H, W) for i in range(EXT_B)] for r in range(EXT_ROUNDS)] for t in range(2)]
    want = [[[oracle_bytes(oracle.extract(blob, im, NF)) for im in rnd] for rnd in per] for per in imgs]
    assert len({w for per in want for rnd in per for w in rnd}) == 2 * EXT_ROUNDS * EXT_B, "the frames give different results"
    assert all(w[0] > 10 for per in want for rnd in per for w in rnd)
    return blob, imgs, want


class Extraction:
    """one handle, its stream, its images on the device and a record buffer: the three ways a frame is extracted"""

    def __init__(self, blob, imgs, precision, device="cuda"):
        import torch
        self.torch = torch
        self.ext = SPExtractor(NF, H, W, blob, max_batch=EXT_B, with_heat=False, precision=precision)
        self.imgs = imgs
        self.stream = torch.cuda.Stream(device=device)
        self.d_imgs = [torch.from_numpy(np.stack(rnd)).to(device) for rnd in imgs]
        self.rb = self.ext.record_bytes()
        self.d_rec = torch.zeros(EXT_B * self.rb, dtype=torch.uint8, device=device)
        torch.cuda.synchronize()

    def round(self, r):
        """-> [(how, frame, bytes)] of round r"""
        ext, out = self.ext, []
        out += [("extract_batch", i, frame_bytes(fr)) for i, fr in enumerate(ext.extract_batch(self.imgs[r]))]
        out += [("submit / collect", i, frame_bytes(fr)) for i, fr in enumerate(ext.collect_batch(ext.submit_batch(self.imgs[r])))]
        with self.torch.cuda.stream(self.stream):
            self.d_rec.zero_()
        ticket = ext.extract_batch_device(self.d_imgs[r].data_ptr(), EXT_B, self.d_rec.data_ptr(), self.stream.cuda_stream)
        ext.wait_records(ticket, self.stream.cuda_stream)
        self.stream.synchronize()
        with self.torch.cuda.stream(self.stream):
            host = self.d_rec.cpu().numpy()
        out += [("extract_batch_device", i, frame_bytes(ext.view_record(host[i * self.rb:(i + 1) * self.rb]))) for i in range(EXT_B)]
        return out


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_extraction_in_two_threads(extraction_images, precision):
    blob, imgs, oracle_want = extraction_images
    pair = [Extraction(blob, imgs[t], precision) for t in range(2)]
    try:
        t0 = time.monotonic()
        solo = [[x.round(r) for r in range(EXT_ROUNDS)] for x in pair]        # alone, in turn
        t_solo = time.monotonic() - t0
        for t in range(2):
            for r in range(EXT_ROUNDS):
                ways = {(how, i): b for how, i, b in solo[t][r]}
                for (how, i), b in ways.items():
                    if precision == "f32":                                    # bit-equal to the oracle, every way
                        assert b == oracle_want[t][r][i], ("alone", t, r, how, i)
                    else:                                                     # bf16: the three ways agree; rounds differ
                        assert b == ways[("extract_batch", i)] and b[1] == 0 and b[0] > 10, ("alone", t, r, how, i)
        if precision == "bf16":
            assert len({b for per in solo for rnd in per for _, _, b in rnd}) == 2 * EXT_ROUNDS * EXT_B

        def worker(t):
            def f(r):
                for (how, i, b), (_, _, w) in zip(pair[t].round(r), solo[t][r]):
                    assert b == w, ("thread %d, round %d: %s, frame %d differs from the call made alone" % (t, r, how, i))
                    if precision == "f32":
                        assert b == oracle_want[t][r][i]
            return f
        took = tf.run_side_by_side([worker(0), worker(1)], EXT_ROUNDS, JOIN_TIMEOUT, ["extraction 0", "extraction 1"])
        print("extraction %s: %d rounds alone in turn %.3f s, side by side %.3f s" % (precision, EXT_ROUNDS, t_solo, took))
    finally:
        for x in pair:
            x.ext.close()


# ---- c. the twin pick ---------------------------------------------------------------------------------------------------------------
TWIN_ROUNDS = 12


def test_twin_pick_survives_a_busy_neighbour(monkeypatch):
    """A handle with a twin (SPFE_FLAG_ASYNC_COV, two side chains) alternates its pipelined calls between the pair, and a debug
    read must come from the one that ran the LAST call: the pick compares the pair's stamps of a process-wide call counter
    (spfe_schedule.hip, spfe_host.h last_caller).  A neighbour thread bumps that counter as fast as it can meanwhile."""
    import torch
    blob = weights.synthetic(7, "dense")
    monkeypatch.setenv("SPFE_TWO_CHAINS", "1")         # (by workload a frame this small gets no twin)
    ext = SPExtractor(NF, H, W, blob, max_batch=EXT_B, with_heat=False, async_cov=True)
    monkeypatch.delenv("SPFE_TWO_CHAINS")
    other = SPExtractor(NF, H, W, blob, max_batch=EXT_B, with_heat=False)
    try:
        assert int(ext.debug_read("two_chains")[0]) == 1
        imgs = [[synth.make_image(5000 + 10 * r + i, H, W) for i in range(EXT_B)] for r in range(TWIN_ROUNDS)]
        want = [[oracle.network(blob, im)[:2] for im in rnd] for rnd in imgs]
        assert len({bits(w[0]).tobytes() for rnd in want for w in rnd}) == TWIN_ROUNDS * EXT_B
        d_imgs = [torch.from_numpy(np.stack(rnd)).cuda() for rnd in imgs]
        d_recs = [torch.zeros(EXT_B * ext.record_bytes(), dtype=torch.uint8, device="cuda") for _ in range(2)]
        stream = torch.cuda.Stream()
        busy = [synth.make_image(5500 + i, H, W) for i in range(EXT_B)]
        busy_want = [frame_bytes(fr) for fr in other.extract_batch(busy)]
        torch.cuda.synchronize()

        def driver(r):
            t = ext.extract_batch_device(d_imgs[r].data_ptr(), EXT_B, d_recs[r % 2].data_ptr(), stream.cuda_stream)
            ext.wait_records(t, stream.cuda_stream)
            stream.synchronize()
            for i in range(EXT_B):
                for name, w in zip(("semi", "coarse"), want[r][i]):
                    got = ext.debug_read(name, i)
                    assert np.array_equal(bits(got), bits(w)), "round %d, frame %d: %r is not this call's (%s)" % (
                        r, i, name, [q for q in range(TWIN_ROUNDS) if np.array_equal(bits(got), bits(want[q][i][name == "coarse"]))])

        def neighbour(r):
            for _ in range(4):
                assert [frame_bytes(fr) for fr in other.extract_batch(busy)] == busy_want, "the neighbour's own frames, round %d" % r

        t0 = time.monotonic()
        for r in range(TWIN_ROUNDS):                   # alone first
            driver(r)
        t_solo = time.monotonic() - t0
        took = tf.run_side_by_side([driver, neighbour], TWIN_ROUNDS, JOIN_TIMEOUT, ["twin pair", "neighbour"])
        print("twin pick: %d rounds alone %.3f s, beside the neighbour %.3f s" % (TWIN_ROUNDS, t_solo, took))
    finally:
        ext.close()
        other.close()


# ---- d. the host-array forms --------------------------------------------------------------------------------------------------------
def host_forms():
    """the forms and the sequence of tests/test_gpu_host_forms_interleaved.py (its functions; blocks go in filled with 0x5A)"""
    forms = {"dust": hfi.dust, "fuse": hfi.fuse, "ba_small": hfi.ba(hfi.golden("ba_small")), "guided": hfi.guided,
             "ba_large": hfi.ba(hfi.ba_cases.large()), "sim3": hfi.sim3, "loop_points": hfi.loop_points, "sim3opt": hfi.sim3opt,
             "proj": hfi.proj, "pose": hfi.pose, "match": hfi.match, "patches": hfi.patches, "loop_fuse": hfi.loop_fuse, "knn2": hfi.knn2}
    first = ["dust", "fuse", "ba_small", "guided"]
    order = first + ["ba_large"] + first[::-1] + ["sim3", "loop_points", "sim3opt", "proj", "pose", "match", "patches", "loop_fuse", "knn2"]
    return forms, order


class Preloaded:
    """While entered, the fixture loaders the form functions of test_gpu_host_forms_interleaved call on EVERY call (np.load of
    the golden files, the generated keyframe) answer from a memo filled in the main thread: the same functions make the same
    calls on the same arrays, but a round of a worker thread is spent inside the library, where the two threads can overlap,
    and not in Python under the interpreter lock.  The modules are put back on exit."""
    LOADERS = ((hfi, "golden"), (hfi, "keyframe"), (hfi.fc, "load"), (hfi.gc, "load"), (hfi.gc, "lp_load"), (hfi.lc, "load"),
               (hfi.sc, "load"))

    def __init__(self):
        self.memo, self.saved = {}, []

    def __enter__(self):
        for mod, name in self.LOADERS:
            fn = getattr(mod, name)
            self.saved.append((mod, name, fn))
            setattr(mod, name, self.memoised(fn, (mod.__name__, name)))
        return self

    def __exit__(self, *exc):
        for mod, name, fn in self.saved:
            setattr(mod, name, fn)
        self.saved = []

    def memoised(self, fn, tag):
        def f(*args):
            key = tag + args
            if key not in self.memo:
                v = fn(*args)
                self.memo[key] = v if isinstance(v, tuple) else Loaded(v)    # (an NpzFile reads the file again per key)
            return self.memo[key]
        return f


class Loaded(dict):
    """the arrays of a golden file, read once; `files` as numpy's NpzFile has it"""

    @property
    def files(self):
        return list(self)


@pytest.fixture(scope="module")
def fresh_handle_bytes():
    """every form on a handle created for that one call (the expectation of the interleaved test)"""
    blob = weights.synthetic(7, "trackable")
    forms, order = host_forms()
    raw, want = {}, {}
    for name in dict.fromkeys(order):
        ext = SPExtractor(hfi.NF, hfi.H, hfi.W, blob, with_heat=False)
        raw[name] = forms[name](ext)
        want[name] = hfi.flat(raw[name])
        ext.close()
    # the calls did their work: what is compared is not untouched fill
    assert raw["dust"]["iterations"] >= 2 and raw["dust"]["n_inlier"] > 0 and raw["fuse"]["n_fused"] > 0
    assert (raw["match"][0] >= 0).sum() >= 12 and (raw["patches"] >= 0).sum() >= 12 and (raw["knn2"][0] >= 0).all()
    assert len(raw["ba_large"]) > 16 * len(raw["ba_small"])
    return blob, forms, order, want


def test_host_forms_in_two_threads(fresh_handle_bytes):
    blob, forms, order, want = fresh_handle_bytes
    pair = [SPExtractor(hfi.NF, hfi.H, hfi.W, blob, with_heat=False) for _ in range(2)]
    orders = [order, order[::-1]]                      # thread 0 forwards, thread 1 backwards: the staging of one grows while
    try:                                               # the other's is small, and the other way round

        def worker(t):
            def f(r):
                name = orders[t][r]
                got = hfi.flat(forms[name](pair[t]))
                assert [p for p, _ in got] == [p for p, _ in want[name]], (t, r, name)
                for (p, g), (_, w) in zip(got, want[name]):
                    assert g == w, "thread %d, step %d: %s %s differs from a fresh handle's" % (t, r, name, p)
            return f
        with Preloaded():
            for r in range(len(order)):                # fills the memo, in the main thread
                worker(0)(r)
            t0 = time.monotonic()
            for t in range(2):                         # alone, in turn
                for r in range(len(order)):
                    worker(t)(r)
            t_solo = time.monotonic() - t0
            took = tf.run_side_by_side([worker(0), worker(1)], len(order), JOIN_TIMEOUT_HOST_FORMS, ["forwards", "backwards"])
        print("host forms: 2 x %d calls alone in turn %.3f s, side by side %.3f s" % (len(order), t_solo, took))
    finally:
        for e in pair:
            e.close()


# ---- e. the last error ----------------------------------------------------------------------------------------------------------------
ERR_ROUNDS = 50


def test_last_error_is_the_calling_threads():
    """spfe_last_error() is the calling thread's: two threads are refused on their arguments at the same moment, for different
    reasons (the refusals return before any launch), and each reads its own text; a third keeps making successful calls."""
    import threading
    blob = weights.synthetic(7, "trackable")
    exts = [SPExtractor(NF, H, W, blob, with_heat=False) for _ in range(3)]
    step = threading.Barrier(2)                        # the two refused calls of a round start together
    t_, desc, _ = hfi.keyframe()
    try:
        want_match = exts[2].match(desc, t_["kp_desc"])
        assert (want_match[0] >= 0).sum() >= 12

        def refused(ext, args, mine, theirs):
            def f(r):
                try:
                    step.wait(JOIN_TIMEOUT)
                    with pytest.raises(SpfeError) as e:
                        ext.set_staging(*args)
                    text = str(e.value)
                    assert mine in text and theirs not in text, "round %d: %r" % (r, text)
                except BaseException:
                    step.abort()
                    raise
            return f

        def matcher(r):
            idx, dist = exts[2].match(desc, t_["kp_desc"])
            assert np.array_equal(idx, want_match[0]) and np.array_equal(bits(dist), bits(want_match[1])), r
        took = tf.run_side_by_side([refused(exts[0], (60, 96, 3), "smaller", "channels"),
                                    refused(exts[1], (64, 96, 2), "channels", "smaller"), matcher], ERR_ROUNDS, JOIN_TIMEOUT,
                                   ["refused: smaller", "refused: channels", "match"])
        print("last error: %d rounds side by side %.3f s" % (ERR_ROUNDS, took))
    finally:
        for e in exts:
            e.close()


# ---- f. a handle on another device, driven from a thread that never used that device ----------------------------------------------
def current_hip_device():
    import ctypes
    import hip_graph
    d = ctypes.c_int(-1)
    assert hip_graph.hip().hipGetDevice(ctypes.byref(d)) == 0
    return d.value


def drive_everything(ext, dev, S, after_call):
    """the calls of the issue's list on `ext`, whose device is `dev`; every tensor with an explicit device.  after_call(what) is
    called behind each library call.  -> [(what, bytes)]; closes the handle"""
    import torch
    import test_gpu_local_ba as tb
    from sp_orb_slam_amd import extractor as X
    device = "cuda:%d" % dev
    out = []

    def done(what, *values):
        after_call(what)
        for j, v in enumerate(values):
            out.append(("%s[%d]" % (what, j), v))
    B = 2
    imgs = [synth.make_image(6000 + i, tb.H, tb.W) for i in range(B)]
    done("extract_batch", *[frame_bytes(fr) for fr in ext.extract_batch(imgs)])
    ticket = ext.submit_batch(imgs)
    after_call("submit_batch")
    done("collect_batch", *[frame_bytes(fr) for fr in ext.collect_batch(ticket)])
    stream = torch.cuda.Stream(device=device)
    d_img = torch.from_numpy(np.stack(imgs)).to(device)
    rb = ext.record_bytes()
    d_rec = torch.zeros(B * rb, dtype=torch.uint8, device=device)
    torch.cuda.synchronize(device)
    ticket = ext.extract_batch_device(d_img.data_ptr(), B, d_rec.data_ptr(), stream.cuda_stream)
    after_call("extract_batch_device")
    ext.wait_records(ticket, stream.cuda_stream)
    after_call("wait_records")
    stream.synchronize()
    host = d_rec.cpu().numpy()
    done("records", *[frame_bytes(ext.view_record(host[i * rb:(i + 1) * rb])) for i in range(B)])
    done("debug_read", bits(ext.debug_read("semi", 1)).tobytes())
    t_, desc, _ = hfi.keyframe()
    idx, dist = ext.match(desc, t_["kp_desc"])
    done("match", idx.tobytes(), dist.tobytes())
    done("bundle_adjust", bytes(hfi.ba(hfi.golden("ba_small"))(ext)))
    n_kf, n, E = len(S.Tcw), len(S.xyz), len(S.edges)
    up = lambda v: torch.from_numpy(gf.raw_bytes(v).copy()).to(device)   # noqa: E731
    d_recs, d_edges, d_Tcw, d_fixed, d_xyz = up(S.raw), up(S.edges), up(S.Tcw), up(S.fixed), up(S.xyz)
    d_out = torch.full((X.ba_offsets(n_kf, n, E)["bytes"],), 0x5A, dtype=torch.uint8, device=device)
    torch.cuda.synchronize(device)
    ext.local_ba_records_device([d_recs.data_ptr() + f * S.rb for f in range(n_kf)], d_edges.data_ptr(), E, d_Tcw.data_ptr(),
                                d_fixed.data_ptr(), d_xyz.data_ptr(), n, d_out.data_ptr(), tb.INTR, stream=stream.cuda_stream)
    after_call("local_ba_records_device")
    stream.synchronize()
    blk = d_out.cpu().numpy()
    assert X.SPExtractor.decode_ba_out(blk, n_kf, n, E)["n_served"] == E
    done("local_ba_records", blk.tobytes())
    ext.close()
    after_call("close")
    return out


def test_handle_on_another_device_from_a_fresh_thread(tmp_path_factory):
    """Almost every entry point begins with hipSetDevice(the handle's device), because HIP's current device is per thread: a
    thread that has never touched device 1 drives a handle that lives there.  Results equal a device-0 handle's, and — as
    include/spfe.h states — every call leaves the calling thread's current device at the handle's."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices: %d visible" % torch.cuda.device_count())
    import test_gpu_local_ba as tb
    S = tb.build_scene(tmp_path_factory.mktemp)                      # its handle: the device-0 one
    blob = weights.synthetic(7, "trackable")
    far = None
    try:
        want = drive_everything(S.ext, 0, S, lambda what: None)
        far = SPExtractor(tb.NF, tb.H, tb.W, blob, max_batch=len(tb.FRAMES), with_heat=False, device=1)
        assert current_hip_device() == 1                             # spfe_create too leaves the caller on the handle's device
        torch.cuda.set_device(0)
        got = []

        def fresh(r):
            assert current_hip_device() == 0                         # a new thread starts on device 0

            def after_call(what):
                assert current_hip_device() == 1, "after %s the thread's current device is %d" % (what, current_hip_device())
            got.extend(drive_everything(far, 1, S, after_call))
        tf.run_side_by_side([fresh], 1, JOIN_TIMEOUT_HOST_FORMS, ["fresh thread"])
        assert current_hip_device() == 0                             # another thread's calls do not move this one
        assert [w for w, _ in got] == [w for w, _ in want]
        for (what, g), (_, w) in zip(got, want):
            assert g == w, "%s on device 1 differs from device 0" % what
    finally:
        torch.cuda.set_device(0)
        if far is not None:
            far.close()
        S.ext.close()


# ---- the first calls of a process, made at the same moment (tests/thread_first_calls.py) ----------------------------------------
def test_first_calls_of_four_threads_at_the_same_moment():
    """One fresh child process (the once-per-process paths have long run in this one): four threads create their handles at one
    barrier and make the first call of each form at one barrier."""
    try:
        r = subprocess.run([sys.executable, "-m", "tests.thread_first_calls"], cwd=ROOT, capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:       # a hang, as in run_side_by_side: nothing further is started on the GPU
        pytest.exit("tests.thread_first_calls still running after %.0f s, counted as hung" % CHILD_TIMEOUT, returncode=1)
    out = r.stdout + r.stderr
    print(out[-6000:])
    verdict = [line for line in r.stdout.splitlines() if line.startswith("thread-first-calls: ")]
    if any("counted as hung" in line for line in verdict):
        pytest.exit(verdict[0], returncode=1)
    assert r.returncode == 0, verdict or out[-2000:]
    assert verdict == ["thread-first-calls: PASS"], verdict
