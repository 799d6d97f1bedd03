"""CPU: tests/lba_ref/lba_ref.c — the oracle of the GPU tests of the gather in front of the local bundle adjustment and of the
application behind it — held to an independent Python statement of the reference's lines (tests/lba_ref/lba_cases.py: map points
with an mObservations list, keyframes as mvpMapPoints lists, the two stamps as sets, the sequential erase loop with its SetBadFlag
cascade and mpRefKF rule), on every fixture tests/golden/lba_*.npz, on every named case and on generated sequences of 40 keyframes in
which gather and apply alternate with the covisibility graph (covis_ref) and the keyframe cull (cull_ref); told apart from eleven
one-line misreadings; the observation counts of the good points kept equal to a fresh count of the rows; the layout held to the
header's macros; and the stand-alone driver run clean under the host sanitizers."""
import glob
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("lba_ref", "cull_ref", "covis_ref"):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
import covis_ref  # noqa: E402
import cull_ref  # noqa: E402
import lba_cases as lc  # noqa: E402
import lba_ref as lr  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "lba_*.npz")))
NAMES = [os.path.basename(p)[4:-4] for p in FIXTURES]
CASES = lc.named_cases()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return lr.build(tmp_path_factory.mktemp("lba_ref"))


@pytest.fixture(scope="module")
def kref(tmp_path_factory):
    return cull_ref.build(tmp_path_factory.mktemp("cull_ref"))


@pytest.fixture(scope="module")
def cref(tmp_path_factory):
    return covis_ref.build(tmp_path_factory.mktemp("covis_ref"))


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_fixture_is_what_lba_ref_gives(ref, path):
    c = lc.load_fixture(path)
    w, r = lc.run_ref(ref, c)
    assert r["block"].tobytes() == c["e_block"].tobytes()
    for k in lr.WORLD:
        assert w[k].tobytes() == c["e_" + k].tobytes(), k


def test_fixtures_are_the_small_named_cases():
    assert sorted(lc.fixture_names()) == sorted(NAMES) and len(NAMES) >= 40
    for name, path in zip(NAMES, FIXTURES):
        c = lc.load_fixture(path)
        assert os.path.getsize(path) < 64 * 1024, name
        for k, v in CASES[name].items():
            assert np.asarray(v).tobytes() == np.asarray(c[k]).tobytes(), (name, k)


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if not c.get("wild")))
def test_lba_ref_equals_the_python_statement_on_the_named_cases(ref, name):
    c = CASES[name]
    w, r = lc.run_ref(ref, c)
    lc.against_python(c, w, r)


def test_named_cases_show_what_they_are_named_for(ref):
    def run(name):
        return lc.run_ref(ref, CASES[name])
    _, r = run("g_seen_by_1_2_3_4_200_and_twice_in_a_row")
    assert r["point_idx"][:6].tolist() == [0, 1, 2, 3, 4, 5] and np.diff(r["obs_start"][:7]).tolist() == [1, 2, 3, 4, 200, 3]
    assert r["obs"][r["obs_start"][5]:r["obs_start"][6]].tolist() == [[5, 5], [5, 7], [6, 6]] and r["status"] == lr.FIXED_CUT and r["n_kf"] == 128
    assert r["kf_slot"][:6].tolist() == [0, 1, 5, 2, 3, 4] and r["fixed"][:6].tolist() == [0, 0, 0, 1, 1, 1]
    _, r = run("g_ord_bad_wild_repeated")
    assert r["kf_slot"][:4].tolist() == [6, 5, 2, 1] and r["fixed"][:4].tolist() == [0, 0, 1, 0] and (r["n_local"], r["n_free"]) == (4, 3)
    assert run("g_ord_empty")[1]["n_local"] == 1 and run("g_ord_full_to_conn_cap")[1]["n_local"] == 12
    _, r = run("g_cur_is_origin")
    assert r["fixed"][0] == 1 and r["n_free"] == 2 and r["n_local"] == 3 and r["status"] & lr.LOCAL_CUT
    _, r = run("g_origin_behind_the_free_cut")
    assert r["kf_slot"][:3].tolist() == [6, 1, 2] and r["status"] & lr.LOCAL_CUT and 0 not in r["kf_slot"][:3]   # a prefix: the origin would fit
    for name, status in (("g_free_cap_exact", 0), ("g_free_cap_plus_1", lr.LOCAL_CUT), ("g_kf_cap_exact", 0), ("g_kf_cap_plus_1", lr.FIXED_CUT),
                         ("g_point_cap_exact", 0), ("g_point_cap_one_short", lr.POINT_CUT), ("g_edge_cap_exact", 0),
                         ("g_edge_cap_one_short", lr.EDGE_OVERFLOW)):
        assert run(name)[1]["status"] == status, name
    _, r = run("g_edge_cap_one_short")
    assert r["n_obs_needed"] == 54 and (r["obs"] == -1).all() and (r["edges"] == -1).all() and (r["obs_start"] == -1).all() and r["n_kf"] == 12
    assert run("g_cur_is_bad")[1]["n_points"] > 0 and run("g_points_0")[1]["n_points"] == 0
    for n in (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025):
        assert run("g_points_%d" % n)[1]["n_points"] == n
    assert run("g_slots_4100_beyond_the_scan_grid")[1]["kf_slot"][0] == 4099 and run("g_table_50000")[1]["point_idx"][0] >= 49000
    w, r = run("a_3_to_2_goes_bad")
    assert r["bad_point"][:1].tolist() == [2] and w["nobs"][2] == 2 and w["mp_flags"][2] == 2 and (w["rows"][:, 2] != 2).all()
    w, r = run("a_4_to_3_stays")
    assert r["n_bad"] == 0 and w["nobs"][3] == 3 and w["mp_flags"][3] == 3 and w["ref_slot"][3] == 1 and r["n_ref_moved"] == 1
    w, r = run("a_erase_the_reference_keyframe")
    assert w["ref_slot"][4] == 3 and w["ref_slot"][3] == 1 and r["n_ref_moved"] == 2 and w["nobs"][4] == 197
    w, r = run("a_erase_every_observation")
    assert r["bad_point"][:3].tolist() == [0, 1, 2] and w["nobs"][:3].tolist() == [0, 0, 0]
    assert run("a_bad_cap_exceeded")[1]["status"] == lr.BAD_CUT and run("a_bad_cap_0")[1]["n_bad_stored"] == 0
    w, r = run("a_point_twice_in_a_row")
    assert r["bad_point"][:1].tolist() == [5] and w["rows"][5].tolist().count(5) == 0 and w["rows"][6, 6] == -1
    assert run("a_stopped_midway_is_applied")[1]["status"] == 0
    for name, c in CASES.items():
        if name.startswith("a_refused") or name.startswith("a_wild_count") or name == "a_wild_n_erase":
            w, r = lc.run_ref(ref, c)
            assert r["status"] == lr.NOT_APPLIED and not lr.diff_world(w, c), name
    assert run("a_wild_erase_indices")[1]["status"] == lr.WILD and run("a_wild_entries_in_the_gather_block")[1]["status"] & lr.WILD


def test_layout_is_the_headers(ref):
    import ctypes as C
    from sp_orb_slam_amd import extractor as X
    for k, p, e, b in ((1, 1, 1, 0), (3, 5, 7, 2), (16, 64, 512, 8), (128, 16384, 131072, 16384)):
        v, g, a, s = lr.layout(ref, k, p, e, b), lr.gather_offsets(k, p, e), lr.apply_offsets(p, e, b), lr.ba_offsets(k, p, e)
        assert v[:8] == [g[x] for x in ("fixed", "Tcw", "point_idx", "xyz", "obs_start", "obs", "edges", "out_bytes")]
        assert v[8:12] == [a[x] for x in ("obs_start", "obs", "ref_slot", "out_bytes")]
        assert all(x % 16 == 0 for x in v[:12]) and v[7] % 256 == 0 and v[11] % 256 == 0 and v[7] >= g["edges"] + 12 * e and v[11] >= a["ref_slot"] + 4 * p
        assert v[12] == lr.LOCAL_CUT | lr.POINT_CUT << 4 | lr.FIXED_CUT << 8 | lr.EDGE_OVERFLOW << 12
        assert v[13] == lr.NOT_APPLIED | lr.BAD_CUT << 4 | lr.WILD << 8
        assert v[14:16] == [C.sizeof(X.LbaGatherParams), C.sizeof(X.LbaApplyParams)] == [24, 16]
        assert v[16:19] == [s["xyz"], s["erase"], s["out_bytes"]]
        assert X.lba_gather_offsets(k, p, e) == g and X.lba_apply_offsets(p, e, b) == a
    assert X.LBA_GATHER_FIELDS == lr.GATHER_FIELDS and X.LBA_APPLY_FIELDS == lr.APPLY_FIELDS
    assert (X.LBA_LOCAL_CUT, X.LBA_POINT_CUT, X.LBA_FIXED_CUT, X.LBA_EDGE_OVERFLOW, X.LBA_NOT_APPLIED, X.LBA_BAD_CUT, X.LBA_WILD) == (1, 2, 4, 8, 1, 2, 4)


def run_sequence(ref, kref, cref, seed, mutate=0, check=True):
    """40 keyframes: the host's row of the new keyframe, UpdateConnections, gather, a solver's block with a random erase list, apply,
    and every fourth keyframe the keyframe cull -> (counts, the digest of every step)"""
    S = lc.SEQ
    rng = np.random.RandomState(seed)
    w = cull_ref.new_world(S["n_slots"], S["stride"], S["n_table"], S["conn_cap"], None, None)
    w["kf_flags"][:] = 1
    w["mp_flags"][:] = 0
    extra = lr.new_world(S["n_slots"], S["stride"], S["n_table"])
    w.update(ref_slot=extra["ref_slot"], xyz=extra["xyz"], Tcw=extra["Tcw"])
    state = {k: w[k] for k in covis_ref.STATE}
    next_point, digest, counts = 0, [], dict(bad=0, moved=0, erased=0, cuts=0, fixed=0)
    for s in range(S["n_slots"]):
        next_point = lc.sequence_keyframe(w, rng, s, next_point)
        covis_ref.update(cref, w["rows"], w["kf_flags"], w["mp_flags"], state, s, th=3, origin_slot=0)
        gprm = dict(cur_slot=s, origin_slot=0, kf_cap=S["kf_cap"], free_cap=S["free_cap"], point_cap=S["point_cap"], edge_cap=S["edge_cap"])
        gc = dict(lr.copy_world(w), op="gather", ord_row=w["ord_slot"][s].copy(), **gprm)
        g = lr.gather(ref, w, gc["ord_row"], gprm, mutate)
        if check:
            lc.against_python(gc, w, g)
        assert not g["status"] & lr.EDGE_OVERFLOW
        counts["cuts"] += g["status"] != 0
        counts["fixed"] += g["n_fixed"]
        erase = np.sort(rng.choice(g["n_edges"], g["n_edges"] // 12, replace=False)) if g["n_edges"] else []
        ac = lc.apply_case(gc, lambda _g: erase, bad_cap=S["bad_cap"], seed=s, block=g["block"], status=lr.BA_STOPPED if s % 7 == 3 else 0)
        a = lr.apply(ref, w, ac["gather"], ac["ba"], ac, mutate)
        if check:
            lc.against_python(ac, w, a)
            good = (w["mp_flags"] & 1).astype(bool)
            assert (w["nobs"][good] == lr.count_nobs(w)[good]).all(), "nobs drifted from the rows"
            assert (w["nobs"][good] == cull_ref.count(kref, w["rows"], w["kf_flags"], S["n_table"])[good]).all()
        counts["bad"] += a["n_bad"]
        counts["moved"] += a["n_ref_moved"]
        counts["erased"] += a["n_erased"]
        digest.append(g["block"].tobytes() + a["block"].tobytes() + b"".join(w[k].tobytes() for k in lr.WORLD))
        if s % 4 == 3:
            cull_ref.cull(kref, {k: w[k] for k in cull_ref.WORLD}, s, th_obs=3, cov_ratio=0.9, origin_slot=0, bad_cap=0)
    return counts, digest


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_sequences_equal_the_python_statement_and_keep_nobs_consistent(ref, kref, cref, seed):
    counts, _ = run_sequence(ref, kref, cref, seed)
    print("over the sequence", counts)
    assert counts["bad"] >= 5 and counts["moved"] >= 5 and counts["erased"] >= 100 and counts["cuts"] >= 5 and counts["fixed"] >= 20, counts


@pytest.mark.parametrize("name", sorted(lr.MUTATIONS))
def test_mutation_is_told_apart(ref, name):
    """every misreading changes the bytes of some named case that is also a fixture"""
    m = lr.MUTATIONS[name]
    hit = []
    for cname, c in sorted(CASES.items()):
        w0, r0 = lc.run_ref(ref, c)
        w1, r1 = lc.run_ref(ref, c, mutate=m)
        if r0["block"].tobytes() != r1["block"].tobytes() or lr.diff_world(w0, w1):
            hit.append(cname)
    print(name, "told apart by the cases", hit)
    assert hit, name
    assert [h for h in hit if h in NAMES], (name, "no fixture tells it apart", hit)


def test_lba_ref_runs_clean_under_the_host_sanitizers(tmp_path):
    """lba_ref.c with its stand-alone driver (tests/lba_ref/lba_ref_main.c, a main of its own), built with AddressSanitizer and
    UndefinedBehaviorSanitizer and run as a program on the CPU: any report aborts it"""
    import subprocess
    exe = str(tmp_path / "lba_ref_main")
    src = [os.path.join(ROOT, "tests", "lba_ref", f) for f in ("lba_ref_main.c", "lba_ref.c")]
    subprocess.check_call(["gcc", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe] + src)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "lba_ref_main: 2880 runs" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
