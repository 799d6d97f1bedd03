"""CPU: tests/mpcull_ref/mpcull_ref.c — the oracle of the GPU tests of map-point culling and of its resident state — held to an
independent Python statement of the reference's lines (tests/mpcull_ref/mpcull_cases.py: map-point objects in a dict, rows as lists,
the recent list walked with erase, numpy.float32 division), on every fixture tests/golden/mpcull_*.npz, on every named case and on
generated sequences of 48 keyframes of admission -> statistics of three frames -> cull; told apart from eleven one-line misreadings;
the observation counts kept consistent with a fresh count of the edited rows; the layout held to the header's macros; and the
stand-alone driver run clean under the host sanitizers."""
import glob
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("mpcull_ref", "cull_ref"):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
import cull_ref  # noqa: E402
import mpcull_cases as mc  # noqa: E402
import mpcull_ref as mr  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "mpcull_*.npz")))
NAMES = [os.path.basename(p)[7:-4] for p in FIXTURES]
CASES = mc.named_cases()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return mr.build(tmp_path_factory.mktemp("mpcull_ref"))


@pytest.fixture(scope="module")
def kref(tmp_path_factory):
    return cull_ref.build(tmp_path_factory.mktemp("cull_ref"))


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_fixture_is_what_mpcull_ref_gives(ref, path):
    c = mc.load_fixture(path)
    w, r = mc.run_ref(ref, c)
    assert r["block"].tobytes() == c["e_block"].tobytes()
    for k in mr.WORLD:
        assert w[k].tobytes() == c["e_" + k].tobytes(), k


def test_fixtures_are_the_small_named_cases():
    assert sorted(mc.fixture_names()) == sorted(NAMES) and len(NAMES) >= 30
    for name, path in zip(NAMES, FIXTURES):
        c = mc.load_fixture(path)
        assert os.path.getsize(path) < 64 * 1024, name
        for k, v in CASES[name].items():
            assert np.asarray(v).tobytes() == np.asarray(c[k]).tobytes(), (name, k)


@pytest.mark.parametrize("name", sorted(CASES))
def test_mpcull_ref_equals_the_python_statement_on_the_named_cases(ref, name):
    c = CASES[name]
    w, r = mc.run_ref(ref, c)
    mc.against_python(c, w, r)


def test_named_cases_show_what_they_are_named_for(ref):
    def run(name):
        return mc.run_ref(ref, CASES[name])
    _, r = run("cull_ratio_threshold")
    assert r["entry_code"][:8].tolist() == [mr.KEPT, mr.CULLED_RATIO, mr.KEPT, mr.KEPT, mr.KEPT, mr.KEPT, mr.CULLED_RATIO, mr.KEPT]
    _, r = run("cull_age_and_observations")
    assert r["entry_code"][:8].tolist() == [mr.KEPT, mr.KEPT, mr.CULLED_OBS, mr.KEPT, mr.CULLED_OBS, mr.RETIRED, mr.CULLED_OBS, mr.RETIRED]
    w, r = run("cull_every_code")
    assert set(r["entry_code"][:14].tolist()) == set(range(6)) and r["status"] == mr.WILD_ENTRY and r["entry_code"][13] == mr.ERASED_BAD
    assert w["rows"][0].tolist() == [-1, -1, -1, 0, -1] and w["rows"][2].tolist() == [1, 2, 5, 0, 9] and w["flags"][9] == 0x82
    assert w["rows"][1].tolist() == [-1, 7, 3, 4, 8] and not (w["flags"][6] & 1) and 6 not in CASES["cull_every_code"]["rows"]
    assert run("cull_bad_cap_cut")[1]["status"] == mr.WILD_ENTRY | mr.BAD_CUT and run("cull_bad_cap_0")[1]["n_bad_stored"] == 0
    _, r = run("cull_duplicates_small")
    assert r["entry_code"][:8].tolist() == [mr.CULLED_RATIO, mr.KEPT, mr.ERASED_BAD, mr.KEPT, mr.CULLED_OBS, mr.ERASED_BAD, mr.RETIRED, mr.RETIRED]
    assert run("cull_nothing_culled")[1]["n_bad"] == 0 and run("cull_count_beyond_cap")[1]["n_listed"] == 16
    for name, status in (("admit_recent_cap_one_short", mr.RECENT_OVERFLOW), ("admit_id_at_n_table", mr.BAD_RANGE), ("admit_id_negative", mr.BAD_RANGE),
                         ("admit_keypoint_out_of_range", mr.BAD_RANGE), ("admit_keypoint_negative", mr.BAD_RANGE),
                         ("admit_neighbour_slot_out_of_range", mr.BAD_RANGE), ("admit_neighbour_is_current", mr.BAD_RANGE),
                         ("admit_neighbour_twice", mr.BAD_RANGE), ("admit_count_beyond_kmax", mr.BAD_RANGE), ("admit_count_negative", mr.BAD_RANGE)):
        w, r = run(name)
        assert r["status"] == status and r["n_admitted"] == 0 and not mr.diff_world(w, CASES[name]), name
    assert run("admit_recent_cap_one_short")[1]["n_needed"] == 12
    w, r = run("admit_recent_cap_reached")
    assert r["status"] == 0 and r["n_recent_after"] == 12 == len(w["recent"]) and (w["recent"] >= 0).all()
    _, r = run("admit_displaced_holder")
    assert r["status"] == mr.DISPLACED and r["n_displaced"] == 3
    _, r = run("admit_refused_and_skipped_blocks")
    assert r["admitted"][:5].tolist() == [0, 2, 0, 0, 1] and r["status"] == 0
    w, r = run("stat_small")
    assert (r["n_visible_held"], r["n_visible_view"], r["n_found"]) == (4, 2, 5)
    before = CASES["stat_small"]
    assert w["visible"][3] - before["visible"][3] == 4 and w["found"][3] - before["found"][3] == 1 and w["found"][5] - before["found"][5] == 1


def test_layout_is_the_headers(ref):
    from sp_orb_slam_amd import extractor as X
    for rc, bc, kmax in ((1, 0, 1), (8, 8, 100), (300, 50, 1000), (262144, 262144, 4096)):
        v, o, t = mr.layout(ref, rc, bc, kmax), mr.offsets(rc, bc), mr.tri_offsets(kmax)
        assert v[:4] == [o[k] for k in ("entry_point", "entry_code", "bad_point", "out_bytes")] and v[3] % 256 == 0 and v[3] >= v[2] + 4 * bc
        assert v[4:9] == [mr.BAD_CUT, mr.WILD_ENTRY, mr.RECENT_OVERFLOW, mr.BAD_RANGE, mr.DISPLACED]
        assert v[9:14] == [32, mr.ADMIT_OUT_BYTES, mr.STAT_OUT_BYTES, 262144, mr.MAX_NEIGH]
        assert v[14:18] == [t[k] for k in ("out_bytes", "new_xyz", "new_k1", "new_k2")]
        assert v[18:20] == [X.PROJ_OFF_VIEW, X.POSE_OFF_OUTLIER]
        import ctypes as C
        assert v[20:22] == [C.sizeof(mr.Life), C.sizeof(X.MpCullParams)] and C.sizeof(X.MpLife) == C.sizeof(mr.Life)
        assert v[22:24] == [36, 20]
        assert X.mpcull_offsets(rc, bc) == o and X.tri_offsets(kmax)["new_k1"] == t["new_k1"]
    assert (X.ADMIT_RECENT_OVERFLOW, X.ADMIT_BAD_RANGE, X.ADMIT_DISPLACED, X.MPCULL_BAD_CUT, X.MPCULL_WILD_ENTRY) == (1, 2, 4, 1, 2)
    assert X.ADMIT_FIELDS == mr.ADMIT_FIELDS and X.MPSTAT_FIELDS == mr.STAT_FIELDS and X.MPCULL_FIELDS == mr.CULL_FIELDS
    assert X.MP_LIFE_STATE == mr.STATE


def run_sequence(ref, kref, seed, mutate=0, check=True):
    """48 keyframes: the host's row of the new keyframe, the cull at its id, the admission of its new points, three tracked frames
    -> (the counts per code, the digest of every step)"""
    w, rng, geo = mc.sequence_world(seed)
    counts, digest = np.zeros(6, np.int64), []
    n_table = len(w["flags"])

    def step(op, r, before, **prm):
        if check:
            mc.against_python(dict(before, op=op, **prm), w, r)
        digest.append(r["block"].tobytes() + b"".join(w[k].tobytes() for k in mr.WORLD))

    for s in range(mc.SEQ["n_slots"]):
        mc.sequence_keyframe(w, rng, geo, s)
        before = mr.copy_world(w)
        prm = dict(cur_kf_id=mc.SEQ["first_id"] + s, th_obs=2, found_ratio=np.float32(0.25), bad_cap=16)
        r = mr.cull(ref, w, mutate=mutate, **prm)
        step("cull", r, before, **prm)
        counts += np.bincount(r["entry_code"][:r["n_listed"]], minlength=6)
        a = mc.sequence_admission(w, rng, geo, s)
        before = mr.copy_world(w)
        r = mr.admit(ref, w, a["tri"], mc.SEQ["kmax"], a["n_neigh"], a["neigh_slot"], a["cur_slot"], a["cur_kf_id"], mutate)
        assert r["status"] == 0, r["status"]
        step("admit", r, before, kmax=mc.SEQ["kmax"], **a)
        for _ in range(mc.SEQ["frames"]):
            f = mc.sequence_frame(w, rng)
            before = mr.copy_world(w)
            r = mr.stat(ref, w, f["entry"], f["after"], f["point_idx"], f["in_view"], f["outlier"], mutate)
            step("stat", r, before, **f)
        if check:
            good = (w["flags"] & 1).astype(bool)
            fresh = cull_ref.count(kref, w["rows"], w["kf_flags"], n_table)
            assert (w["nobs"][good] == fresh[good]).all(), "nobs drifted from the rows"
    return counts, digest


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_sequences_equal_the_python_statement_and_keep_nobs_consistent(ref, kref, seed):
    counts, _ = run_sequence(ref, kref, seed)
    print("codes over the sequence", counts.tolist())
    assert (counts[:5] >= 3).all(), counts      # every code but WILD happens


@pytest.mark.parametrize("name", sorted(mr.MUTATIONS))
def test_mutation_is_told_apart(ref, kref, name):
    """every misreading changes the bytes of some named case or of a generated sequence"""
    m = mr.MUTATIONS[name]
    hit = []
    for cname, c in sorted(CASES.items()):
        w0, r0 = mc.run_ref(ref, c)
        w1, r1 = mc.run_ref(ref, c, mutate=m)
        if r0["block"].tobytes() != r1["block"].tobytes() or mr.diff_world(w0, w1):
            hit.append(cname)
    print(name, "told apart by the cases", hit)
    if name == "first_kf_taken_as_a_slot":       # one admission stores an id no cull reads: the sequence reads it
        assert run_sequence(ref, kref, 1, mutate=m, check=False)[1] != run_sequence(ref, kref, 1, check=False)[1]
    assert hit, name
    small = [h for h in hit if h in NAMES]
    assert small, (name, "no fixture tells it apart", hit)


def test_rounding_case_is_kept_where_the_integer_test_culls(ref):
    c = CASES["cull_ratio_threshold"]
    assert np.float32(1 << 24) / np.float32((1 << 26) + 1) == np.float32(0.25) and 4 * (1 << 24) < (1 << 26) + 1
    assert mc.run_ref(ref, c)[1]["entry_code"][5] == mr.KEPT and mc.run_ref(ref, c, mutate=2)[1]["entry_code"][5] == mr.CULLED_RATIO


def test_mpcull_ref_runs_clean_under_the_host_sanitizers(tmp_path):
    """mpcull_ref.c with its stand-alone driver (tests/mpcull_ref/mpcull_ref_main.c, a main of its own), built with AddressSanitizer
    and UndefinedBehaviorSanitizer and run as a program on the CPU: any report aborts it"""
    import subprocess
    exe = str(tmp_path / "mpcull_ref_main")
    src = [os.path.join(ROOT, "tests", "mpcull_ref", f) for f in ("mpcull_ref_main.c", "mpcull_ref.c")]
    subprocess.check_call(["gcc", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe] + src)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "mpcull_ref_main: 4320 runs" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
