"""CPU: tests/extent_arena.py proves itself on its numpy backing, with numpy stand-ins for kernels that address the arena's
bytes as a kernel addresses memory — every way of leaving a buffer the GPU tests rely on it to see must be reported, and a
stand-in that keeps to its buffers must pass.  And the cases of tests/extent_cases.py, held against proj_ref on a frame the
CPU oracle extracted: the stale holders are there, in the numbers tests/test_gpu_extents.py asks for, where a point would
otherwise claim the keypoint and where nobody does."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "proj_ref", "track_ref"):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
import extent_arena as ea  # noqa: E402
import extent_cases as ec  # noqa: E402
import proj_ref  # noqa: E402
import track_cases as tc  # noqa: E402
from test_gpu_proj_search import make_map  # noqa: E402  (the generator of the projection tests, not a copy)

from oracle import oracle  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from tools import track_scene as ts  # noqa: E402

K, N = 11, 7


def inputs(seed=0):
    rng = np.random.default_rng(seed)
    mp = rng.integers(0, N, K).astype(np.int32)
    mp[::3] = -1
    return dict(mp=mp, w=rng.uniform(1, 2, K).astype(np.float32), pts=rng.uniform(1, 2, (N, 3)).astype(np.float32),
                flags=rng.choice(np.array([0, 1, 2, 3], np.uint8), N))


def standin(mem, o, bug=None):
    """The shape of the pose chain in small: out[k] = w[k] * (x + y + z of the point keypoint k holds), cnt = [keypoints
    that hold a point, points with the OBSERVED bit, sum of the holders].  mem: the bytes; o: name -> offset.  bug: the one
    way in which this run leaves its buffers."""
    def f32(off, i):
        return mem[off + 4 * i:off + 4 * i + 4].view(np.float32)[0]

    def i32(off, i):
        return int(mem[off + 4 * i:off + 4 * i + 4].view(np.int32)[0])
    out = np.zeros(K, np.float32)
    held = chk = 0
    for k in range(K + (bug == "read_index_past")):
        m = i32(o["mp"], k)
        chk += m
        if k >= K or m < 0 or (m >= N and bug != "follow_holder"):
            continue
        held += 1
        out[k] = f32(o["w"], k) * (f32(o["pts"], 3 * m) + f32(o["pts"], 3 * m + 1) + f32(o["pts"], 3 * m + 2))
    if bug == "read_f32_past":
        out[0] += f32(o["w"], K)
    observed = sum(int(mem[o["flags"] + i] >> 1) & 1 for i in range(N + (bug == "read_flag_past")))
    mem[o["out"]:o["out"] + 4 * K] = out.view(np.uint8)
    mem[o["cnt"]:o["cnt"] + 12] = np.array([held, observed, chk & 0x7fffffff], np.int32).view(np.uint8)
    if bug == "write_byte_past":
        mem[o["out"] + 4 * K] = 0
    if bug == "write_element_before":
        mem[o["out"] - 4:o["out"]] = 0


def ordinary(x):
    """the stand-in on separate arrays with room to spare, as the other tests call a kernel"""
    mem, o, at = np.zeros(8192, np.uint8), {}, 256
    for name, a in list(x.items()) + [("out", np.zeros(K, np.float32)), ("cnt", np.zeros(3, np.int32))]:
        b = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        mem[at:at + len(b)] = b
        o[name] = at
        at += len(b) + 512
    standin(mem, o)
    return dict(out=mem[o["out"]:o["out"] + 4 * K].copy(), cnt=mem[o["cnt"]:o["cnt"] + 12].copy())


def arena_for(x):
    a = ea.Arena("numpy")
    a.place("mp", x["mp"])
    a.place("w", x["w"])
    a.place("pts", x["pts"], slack_rows=ec.SLACK_ROWS, row_bytes=12)
    a.place("flags", x["flags"], slack_rows=ec.SLACK_ROWS, row_bytes=1)
    a.place("out", 4 * K, init=0xA5)
    a.place("cnt", 12, init=0xA5)
    return a


def run(x, bug):
    a = arena_for(x)
    names = ("mp", "w", "pts", "flags", "out", "cnt")
    return ea.report(a, lambda ar: standin(ar.mem, {n: ar.offset(n) for n in names}, bug), ("out", "cnt"), ordinary(x))[0]


def test_layout_keeps_every_buffer_apart_and_at_its_size():
    a = arena_for(inputs())
    a.fill(0xFF)
    spans = sorted((a.offset(n), a.size(n)) for n in ("mp", "w", "pts", "flags", "out", "cnt"))
    assert all(a.ptr(n) % ea.ALIGN == 0 for n in ("mp", "w", "pts", "flags", "out", "cnt"))
    assert spans[0][0] >= ea.GAP and a.nbytes - (spans[-1][0] + spans[-1][1]) >= ea.GAP
    for (o0, n0), (o1, _) in zip(spans, spans[1:]):
        assert o1 - (o0 + n0) >= ea.GAP
    assert a.size("pts") == N * 12 and a.size("flags") == N and a.size("mp") == 4 * K      # not a byte more
    behind_pts = min(o for o, _ in spans if o > a.offset("pts")) - (a.offset("pts") + N * 12)
    assert behind_pts >= ec.SLACK_ROWS * 12 and ec.stale_values(N)[2] * 12 + 12 <= N * 12 + behind_pts
    assert np.array_equal(a.read("pts", np.float32), inputs()["pts"].reshape(-1)) and a.violations() == []
    with pytest.raises(RuntimeError):
        a.place("late", 16)


def test_fill_restores_the_buffers_and_the_poison():
    a = arena_for(inputs())
    a.fill(0xFF)
    a.mem[:] = 0
    assert a.violations()
    a.fill(0x80)
    assert a.violations() == [] and np.array_equal(a.read("mp", np.int32), inputs()["mp"])
    assert (a.read("out") == 0xA5).all()


def test_well_behaved_standin_passes():
    assert run(inputs(), None) == []


@pytest.mark.parametrize("bug,buffer,where,what", [("write_byte_past", "out", "behind", "1 byte(s) written 0 byte(s) behind 'out'"),
                                                   ("write_element_before", "out", "before", "4 byte(s) written 0 byte(s) before 'out'")])
def test_writes_outside_an_output_are_reported(bug, buffer, where, what):
    found = run(inputs(), bug)
    assert sum(what in f for f in found) == 2, found           # under either poison
    a = arena_for(inputs())
    a.fill(0x80)
    names = ("mp", "w", "pts", "flags", "out", "cnt")
    standin(a.mem, {n: a.offset(n) for n in names}, bug)
    v = a.violations()
    assert len(v) == 1 and v[0]["buffer"] == buffer and v[0]["where"] == where and v[0]["distance"] == 0


@pytest.mark.parametrize("bug,output", [("read_f32_past", "out"), ("read_index_past", "cnt"), ("read_flag_past", "cnt")])
def test_reads_past_an_input_are_reported(bug, output):
    found = run(inputs(), bug)
    assert any(("%r depends on the poison" % output) in f or ("%r differs from the ordinary call" % output) in f for f in found), found
    assert not any("written" in f for f in found)


def test_flag_and_index_reads_show_between_the_two_fills_alone():
    """without the ordinary call to compare with: the two patterns differ where a flag or an index is read"""
    x = inputs()
    names = ("mp", "w", "pts", "flags", "out", "cnt")
    for bug in ("read_index_past", "read_flag_past", "read_f32_past"):
        found = ea.report(arena_for(x), lambda ar: standin(ar.mem, {n: ar.offset(n) for n in names}, bug), ("out", "cnt"))[0]
        assert any("depends on the poison" in f for f in found), (bug, found)


def test_following_a_holder_equal_to_n_is_reported():
    x = inputs()
    x["mp"][4] = N                                    # stale: one past the array, into the slack rows
    assert run(x, None) == []                         # counts as none
    found = run(x, "follow_holder")
    assert any("'out'" in f for f in found) and any("'cnt'" in f for f in found), found
    x["mp"][4] = ec.stale_values(N)[2]                # n + 37: still poison inside the arena
    assert run(x, None) == [] and any("'out'" in f for f in run(x, "follow_holder"))


def test_top_bit_rule_of_the_poison_patterns():
    assert ea.POISONS == (0xFF, 0x80)
    words = {p: np.full(4, p, np.uint8) for p in ea.POISONS}
    for p, w in words.items():
        assert p & 0x80
        assert w.view(np.int32)[0] < 0 and (w.view(np.int16) < 0).all()          # an index: none
    a, b = (words[p].view(np.float32)[0] for p in ea.POISONS)
    assert np.isnan(a) and b < 0 and abs(b) < 1e-37 and not a == b               # NaN / a tiny negative number
    assert (0xFF ^ 0x80) & 1 and (0xFF ^ 0x80) & 2                               # SEARCHABLE and OBSERVED both differ


# ---- the stale-holder cases on a frame of the oracle's ----------------------------------------------------------------
H, W, NF = 240, 320, 400
INTR = (ts.FX, ts.FY, ts.CX, ts.CY)


@pytest.fixture(scope="module")
def frame():
    world = ts.texture(21, *ts.world_size(H, W))
    return tc.from_oracle(oracle.extract(weights.synthetic(7, "trackable"), ts.frame(world, 3, H, W), NF))


@pytest.fixture(scope="module")
def jref(tmp_path_factory):
    return proj_ref.build(tmp_path_factory.mktemp("proj_ref"))


@pytest.mark.parametrize("mode,th", [(proj_ref.LOCAL_MAP, 5.0), (proj_ref.LAST_FRAME, 15.0)])
def test_stale_holder_case_has_the_counts_the_gpu_test_asks_for(frame, jref, mode, th):
    n, kmax = 300, NF + 1
    m = make_map(frame, n, 5, H, W)

    def search(entry):
        return proj_ref.search(jref, frame.kp_xy, frame.occ_grid, frame.descriptors, m["xyz"], m["normal"], m["desc"], m["flags"],
                               entry[:frame.K], m["Tcw"], INTR, W, H, mode=mode, th=th)
    entry = np.full(kmax, -1, np.int32)
    entry[:frame.K] = m["mp_of_kp"]
    stale, ck, ik = ec.stale_entry(search, entry, frame.K, n)
    c = ec.stale_counts(search, stale, frame.K, n)
    print(mode, c, ck, ik)
    assert c["stale"] >= ec.MIN_STALE and c["contested"] >= ec.MIN_CONTESTED and c["left_alone"]
    assert set(stale[np.concatenate([ck, ik])].tolist()) == set(ec.stale_values(n))            # every value is used
    assert ec.in_range(entry[:frame.K], n).sum() >= 20                                          # beside valid holders
    # the stale values count as none: the search from the masked entry gives the same answer but for the values left alone
    r, r0 = search(stale), search(ec.masked(stale, n))
    for k in ("kp_of_mp", "in_view", "n_matches", "n_to_match"):
        assert np.array_equal(r[k], r0[k]), k
    full = np.full(kmax, -1, np.int32)
    full[:frame.K] = r0["mp_of_kp"]
    assert np.array_equal(ec.restore_stale(full, stale, frame.K, n)[:frame.K], r["mp_of_kp"])
