"""CPU: tests/newkf_ref/newkf_ref.c — the oracle of the GPU tests of the insertion of a new keyframe's row and of the observation
lists — held to an independent Python statement of the reference's lines (tests/newkf_ref/newkf_cases.py: map-point objects with an
mObservations dict, local_mapper.cpp:255-272 literally, a list as sorted(mObservations.items()), the two documented deviations), on
every fixture tests/golden/newkf_*.npz, on every named case and on sequences of 40 keyframes that alternate the insertion, the
listing with mp_ref, covis_ref, mpcull_ref (cull and admission), lba_ref (gather and apply) and cull_ref; told apart from twelve
one-line misreadings; the observation counts kept equal to a fresh count of the rows; the layout held to the header's macros; the
stand-alone driver run clean under the host sanitizers; and the host-array forms of the library held to the reference byte for
byte (a GPU test: the forms run the kernels)."""
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("newkf_ref", "mpcull_ref", "cull_ref", "covis_ref", "lba_ref", "mp_ref"):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
import covis_ref  # noqa: E402
import cull_ref  # noqa: E402
import lba_cases as lc  # noqa: E402
import lba_ref as lr  # noqa: E402
import mp_ref  # noqa: E402
import mpcull_ref as mr  # noqa: E402
import newkf_cases as nc  # noqa: E402
import newkf_ref as nr  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "newkf_*.npz")))
NAMES = [os.path.basename(p)[6:-4] for p in FIXTURES]
CASES = nc.named_cases()


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp("newkf_ref")
    return dict(nk=nr.build(d), mp=mp_ref.build(d), covis=covis_ref.build(d), mc=mr.build(d), lba=lr.build(d), kf=cull_ref.build(d))


@pytest.fixture(scope="module")
def ref(refs):
    return refs["nk"]


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_fixture_is_what_newkf_ref_gives(ref, path):
    c = nc.load_fixture(path)
    w, r = nc.run_ref(ref, c)
    assert r["block"].tobytes() == c["e_block"].tobytes()
    for k in nr.WORLD:
        assert nr.raw(w[k]) == (b"" if c["e_" + k].dtype == np.bool_ else c["e_" + k].tobytes()), k


def test_fixtures_are_the_small_named_cases():
    assert sorted(nc.fixture_names()) == sorted(NAMES) and len(NAMES) >= 30
    for name, path in zip(NAMES, FIXTURES):
        c = nc.load_fixture(path)
        assert os.path.getsize(path) < 64 * 1024, name
        for k, v in CASES[name].items():
            assert (c[k] is None) if v is None else (np.asarray(v).tobytes() == np.asarray(c[k]).tobytes()), (name, k)


@pytest.mark.parametrize("name", sorted(CASES))
def test_newkf_ref_equals_the_python_statement_on_the_named_cases(ref, name):
    c = CASES[name]
    w, r = nc.run_ref(ref, c)
    nc.against_python(c, w, r)


def test_named_cases_show_what_they_are_named_for(ref):
    def run(name):
        return nc.run_ref(ref, CASES[name])
    w, r = run("insert_every_code")
    assert r["code"].tolist() == [nr.ADDED, nr.NONE, nr.BAD_POINT, nr.WILD, nr.REPEATED, nr.WILD, nr.ADDED, nr.REPEATED, nr.BAD_POINT, nr.REPEATED]
    assert w["rows"][1].tolist() == [3, -1, -1, -1, 3, -1, 7, 3, -1, 7, -1, -1] and w["recent"][:6].tolist() == [9, 9, 1, 3, 3, 7]
    before = CASES["insert_every_code"]
    assert (w["nobs"] - before["nobs"])[[3, 7, 4, 5]].tolist() == [3, 2, 0, 0] and r["added_point"][:8].tolist() == [3, -1, -1, -1, -1, -1, 7, -1]
    assert w["flags"][3] & nr.OBSERVED and w["flags"][7] & nr.OBSERVED and w["flags"][4] == before["flags"][4]
    assert w["desc_track"][3].tobytes() == before["rec_desc"][0].tobytes() and w["desc_track"][7].tobytes() == before["rec_desc"][6].tobytes()
    assert w["desc_track"][4].tobytes() == before["desc_track"][4].tobytes()
    w, _ = run("insert_every_code_bf16")
    assert w["desc_track"][7].view(np.uint32).tolist() == (CASES["insert_every_code_bf16"]["rec_desc"][6].astype(np.uint32) << 16).tolist()
    for name in ("insert_no_record", "insert_no_track_table"):
        assert nr.raw(run(name)[0]["desc_track"]) == nr.raw(CASES[name]["desc_track"])
    for name, status in (("insert_row_in_use", nr.ROW_IN_USE), ("insert_bad_slot", nr.BAD_SLOT), ("insert_recent_cap_one_short", nr.RECENT_OVERFLOW),
                         ("insert_all_refusals", 7)):
        w, r = run(name)
        assert r["status"] == status and (r["added_point"] == -1).all() and not nr.diff_world(w, CASES[name]), name
    assert run("insert_recent_cap_one_short")[1]["n_needed"] == 7 and run("insert_recent_cap_reached")[1]["n_recent_after"] == 6
    assert run("insert_count_beyond_cap")[1]["n_recent_before"] == 6 and run("insert_count_negative")[1]["n_recent_before"] == 0
    r = run("insert_repeats_across_chunks")[1]
    assert r["code"][[10, 1030, 1090]].tolist() == [nr.ADDED, nr.REPEATED, nr.REPEATED] and r["status"] == 0
    r = run("list_all_empty_wild_repeated")[1]
    assert r["point_idx"].tolist() == [-1, -1, 5, -1, -1, -1, -1, -1] and (r["n_empty"], r["n_wild"], r["n_repeated"], r["n_first"]) == (2, 3, 2, 1)
    r = run("list_observers_0_to_300")[1]
    lens = np.diff(r["obs_start"])
    assert lens.tolist() == [300, 0, 257, 1, 256, 3, 201, 64, 65, 0, 0] and r["status"] == nr.MANY and r["max_obs"] == 300
    assert r["obs"][r["obs_start"][5]:r["obs_start"][6]].tolist() == [[0, 12], [1, 12], [1, 13]]      # point 2: twice in row 1
    for name in ("list_capacity_one_short", "list_capacity_0", "list_observers_one_short"):
        r = run(name)[1]
        assert r["status"] & nr.OVERFLOW and r["n_obs"] == 0 and r["n_obs_needed"] > r["obs_cap"] and (r["obs_start"] == 0).all(), name
    assert run("list_capacity_exact")[1]["status"] == 0 and run("list_observers_256_alone")[1]["status"] == 0
    assert run("list_observers_257_alone")[1]["status"] == nr.MANY
    r = run("list_no_index_array_past_the_table")[1]
    assert r["point_idx"].tolist() == list(range(75, 90)) + [-1] * 15 and r["n_wild"] == 15
    r = run("list_observers_in_bad_slots")[1]
    assert not set(r["obs"][:r["n_obs"], 0].tolist()) & {0, 1, 63, 199, 299}


def test_layout_is_the_headers(ref):
    from sp_orb_slam_amd import extractor as X
    for n_kp, stride, m, cap in ((0, 1, 0, 0), (1, 1, 1, 1), (5, 9, 3, 7), (1001, 1001, 1025, 8000), (16384, 16384, 262144, 4194304)):
        v, o, q = nr.layout(ref, n_kp, stride, m, cap), nr.insert_offsets(n_kp, stride), nr.list_offsets(m, cap)
        assert v[:3] == [o[k] for k in ("code", "added_point", "out_bytes")] and v[2] % 256 == 0 and v[1] % 16 == 0
        assert v[1] >= 64 + 4 * n_kp and v[2] >= v[1] + 4 * stride
        assert v[3:8] == [q[k] for k in ("point_idx", "obs_start", "ref_slot", "obs", "out_bytes")] and all(x % 16 == 0 for x in v[3:8])
        assert q["obs_start"] >= 64 + 4 * m and q["ref_slot"] >= q["obs_start"] + 4 * (m + 1) and q["obs"] >= q["ref_slot"] + 4 * m
        assert v[7] % 256 == 0 and v[7] >= q["obs"] + 8 * cap
        assert v[8:13] == [nr.ROW_IN_USE, nr.BAD_SLOT, nr.RECENT_OVERFLOW, nr.OVERFLOW, nr.MANY]
        assert v[13:19] == [4, 24, 28, 32, 4, 36]
        assert v[19:24] == [nr.MAX_OBS, 262144, 4194304, nr.REPEATED, nr.L_FIRST]
        assert X.newkf_offsets(n_kp, stride) == o and X.listobs_offsets(m, cap) == q
    assert (X.NEWKF_ROW_IN_USE, X.NEWKF_BAD_SLOT, X.NEWKF_RECENT_OVERFLOW, X.LISTOBS_OVERFLOW, X.LISTOBS_MANY) == (1, 2, 4, 1, 2)
    assert X.NEWKF_FIELDS == nr.INSERT_FIELDS and X.LISTOBS_FIELDS == nr.LIST_FIELDS
    assert (X.NEWKF_CODE_NONE, X.NEWKF_CODE_WILD, X.NEWKF_CODE_BAD_POINT, X.NEWKF_CODE_ADDED, X.NEWKF_CODE_REPEATED) == tuple(range(5))
    assert (X.LISTOBS_CODE_EMPTY, X.LISTOBS_CODE_WILD, X.LISTOBS_CODE_REPEATED, X.LISTOBS_CODE_FIRST) == tuple(range(4))
    assert C.sizeof(X.MpLife) == C.sizeof(nr.Life)


SEQ = dict(lc.SEQ, recent_cap=300, first_id=100, kmax=40)


def run_sequence(refs, seed, mutate=0, check=True):
    """40 keyframes on ONE world under the six references' names: the host sets the slot's flag; the insertion of the frame's holders;
    the listing of added_point and mp_ref on it; UpdateConnections; the map-point cull; the admission of created points, their
    listing (first_row = point_base, m = a bound) and mp_ref; the local BA's gather and apply with a random erase list; every fourth
    keyframe the keyframe cull -> (counts, the digest of every step)"""
    S = SEQ
    n, stride, n_table = S["n_slots"], S["stride"], S["n_table"]
    rng = np.random.RandomState(seed)
    w = cull_ref.new_world(n, stride, n_table, S["conn_cap"], None, None)
    w["kf_flags"][:] = 1
    w["mp_flags"][:] = 0
    extra = lr.new_world(n, stride, n_table)
    w.update(ref_slot=extra["ref_slot"], xyz=extra["xyz"], Tcw=np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (n, 1)))
    w["Tcw"][:, 3] = np.arange(n) * 0.25
    w.update(flags=w["mp_flags"], found=np.zeros(n_table, np.int32), visible=np.zeros(n_table, np.int32), first_kf=np.full(n_table, -1, np.int32),
             recent=np.full(S["recent_cap"], -1, np.int32), recent_n=np.zeros(1, np.int32), desc_track=None)
    state = {k: w[k] for k in covis_ref.STATE}
    kf_desc = np.random.RandomState(99).standard_normal((n, stride, 256)).astype(np.float32)
    kf_desc /= np.linalg.norm(kf_desc, axis=2, keepdims=True)
    next_point, digest = 0, []
    counts = dict(added=0, repeated=0, bad_point=0, wild=0, refreshed=0, listed_obs=0, culled=0, erased=0)

    def nobs_is_a_fresh_count(what):
        good = (w["flags"] & 1).astype(bool)
        fresh = cull_ref.count(refs["kf"], w["rows"], w["kf_flags"], n_table)
        assert (w["nobs"][good] == fresh[good]).all(), "nobs drifted from the rows behind " + what

    def list_and_refresh(point_idx, first_row, m, what):
        c = nc.list_case(w, point_idx, m=m, first_row=first_row, obs_cap=S["edge_cap"])
        r = nr.list_obs(refs["nk"], w, point_idx, first_row, m, S["edge_cap"], mutate)
        if check:
            nc.against_python(c, w, r)                     # every listed range equals the statement's map
            assert r["status"] == 0, (what, r["status"])
        o = nr.list_offsets(m, S["edge_cap"])               # the refresh takes the four arrays as they lie in the block
        arr = lambda k, cnt: r["block"][o[k]:o[k] + 4 * cnt].view(np.int32)   # noqa: E731
        mp = mp_ref.refresh(refs["mp"], dict(kf_flags=w["kf_flags"], kf_K=np.full(n, stride, np.int32), kf_status=np.zeros(n, np.int32), Tcw=w["Tcw"],
                                             kf_desc=kf_desc, point_idx=arr("point_idx", m), obs_start=arr("obs_start", m + 1),
                                             obs=arr("obs", 2 * S["edge_cap"]).reshape(-1, 2), ref_slot=arr("ref_slot", m), xyz=w["xyz"],
                                             flags=w["flags"], mode=3, level_scale=1.0, top_scale=1.0))
        if check:
            first = r["point_idx"] >= 0
            assert (mp["code"][~first] == 3).all(), what   # SPFE_MP_INVALID: an empty entry is never followed
            good = first & ((w["flags"][r["point_idx"].clip(0)] & 1) != 0)
            lens = np.diff(r["obs_start"])
            assert (mp["code"][good & (lens > 0)] == 6).all() and (mp["code"][good & (lens == 0)] == 2).all(), (what, mp["code"][good].tolist())
            assert (mp["code"][first & ~good] == 1).all(), what
        counts["refreshed"] += int((mp["code"] == 6).sum())
        counts["listed_obs"] += r["n_obs"]
        digest.append(r["block"].tobytes() + mp["block"].tobytes())
        return r

    for s in range(n):
        # the frame's holders at CreateNewKeyFrame: good points of the last keyframes, some twice, a culled one, wild and empty entries
        w["kf_flags"][s] = 0
        recent_rows = w["rows"][max(0, s - 5):s]
        known = np.unique(recent_rows[recent_rows >= 0])
        frame = np.full(stride, -1, np.int32)
        if len(known):
            take = rng.permutation(known)[:stride // 2]
            frame[rng.choice(stride - 9, len(take), replace=False)] = take
            free = np.flatnonzero(frame[:stride - 9] < 0)
            again = rng.choice(take, min(3, len(take), len(free)), replace=False)
            frame[free[:len(again)]] = again
            frame[stride - 9] = n_table + s
        ic = nc.insert_case(w, frame, s)
        r = nr.insert(refs["nk"], w, frame, s, None, mutate)
        if check:
            nc.against_python(ic, w, r)
            assert r["status"] == 0
            nobs_is_a_fresh_count("the insertion of keyframe %d" % s)
        for k in ("added", "repeated", "bad_point", "wild"):
            counts[k] += r["n_" + k]
        digest.append(r["block"].tobytes() + b"".join(nr.raw(w[k]) for k in nr.WORLD))
        list_and_refresh(r["added_point"], 0, stride, "keyframe %d: added_point" % s)
        covis_ref.update(refs["covis"], w["rows"], w["kf_flags"], w["mp_flags"], state, s, th=3, origin_slot=0)
        # MapPointCulling, then the admission of created points into the last 8 entries of the rows of s and of a neighbour
        c = mr.cull(refs["mc"], w, S["first_id"] + s, 2, 0.25, S["bad_cap"])
        counts["culled"] += c["n_bad"]
        if check:
            nobs_is_a_fresh_count("the map-point cull at keyframe %d" % s)
        neigh = [t for t in range(max(0, s - 4), s) if not w["kf_flags"][t] & 1]
        if neigh and next_point + 8 <= n_table:
            t = int(rng.choice(neigh))
            k2 = [k for k in range(stride - 8, stride) if w["rows"][t, k] == -1]
            k1 = [k for k in range(stride - 8, stride) if w["rows"][s, k] == -1][:len(k2)]
            blocks = [dict(point_base=next_point, k1=k1, k2=k2[:len(k1)])]
            a = mr.admit(refs["mc"], w, mr.tri_blocks(S["kmax"], blocks), S["kmax"], 1, np.asarray([t], np.int32), s, S["first_id"] + s)
            assert a["status"] == 0, a["status"]
            w["ref_slot"][next_point:next_point + len(k1)] = s                 # the host's: mpRefKF of a created point
            list_and_refresh(None, next_point, 8, "keyframe %d: created points" % s)
            next_point += len(k1)
        if check:
            nobs_is_a_fresh_count("the admission at keyframe %d" % s)
        # the local bundle adjustment
        gprm = dict(cur_slot=s, origin_slot=0, kf_cap=S["kf_cap"], free_cap=S["free_cap"], point_cap=S["point_cap"], edge_cap=S["edge_cap"])
        gc = dict(lr.copy_world(w), op="gather", ord_row=w["ord_slot"][s].copy(), **gprm)
        g = lr.gather(refs["lba"], w, gc["ord_row"], gprm)
        assert not g["status"] & lr.EDGE_OVERFLOW
        erase = np.sort(rng.choice(g["n_edges"], g["n_edges"] // 12, replace=False)) if g["n_edges"] else []
        ac = lc.apply_case(gc, lambda _g: erase, bad_cap=S["bad_cap"], seed=s, block=g["block"], status=0)
        a = lr.apply(refs["lba"], w, ac["gather"], ac["ba"], ac)
        counts["erased"] += a["n_erased"]
        if check:
            nobs_is_a_fresh_count("the local BA at keyframe %d" % s)
        if s % 4 == 3:
            cull_ref.cull(refs["kf"], {k: w[k] for k in cull_ref.WORLD}, s, th_obs=3, cov_ratio=0.9, origin_slot=0, bad_cap=0)
            if check:
                nobs_is_a_fresh_count("the keyframe cull at keyframe %d" % s)
                list_and_refresh(w["rows"][s].copy(), 0, stride, "keyframe %d: the whole row" % s)
    return counts, digest


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_sequences_equal_the_python_statement_and_keep_nobs_consistent(refs, seed):
    counts, _ = run_sequence(refs, seed)
    print("over the sequence", counts)
    assert counts["added"] >= 200 and counts["repeated"] >= 50 and counts["bad_point"] >= 3 and counts["wild"] >= 30, counts
    assert counts["refreshed"] >= 200 and counts["listed_obs"] >= 500 and counts["culled"] >= 3 and counts["erased"] >= 50, counts


@pytest.mark.parametrize("name", sorted(nr.MUTATIONS))
def test_mutation_is_told_apart(ref, name):
    """every misreading changes the bytes of some named case that is also a fixture"""
    m = nr.MUTATIONS[name]
    hit = []
    for cname, c in sorted(CASES.items()):
        w0, r0 = nc.run_ref(ref, c)
        w1, r1 = nc.run_ref(ref, c, mutate=m)
        if r0["block"].tobytes() != r1["block"].tobytes() or nr.diff_world(w0, w1):
            hit.append(cname)
    print(name, "told apart by the cases", hit)
    assert hit, name
    assert [h for h in hit if h in NAMES], (name, "no fixture tells it apart", hit)


def test_newkf_ref_runs_clean_under_the_host_sanitizers(tmp_path):
    """newkf_ref.c with its stand-alone driver (tests/newkf_ref/newkf_ref_main.c, a main of its own), built with AddressSanitizer
    and UndefinedBehaviorSanitizer and run as a program on the CPU: any report aborts it"""
    exe = str(tmp_path / "newkf_ref_main")
    src = [os.path.join(ROOT, "tests", "newkf_ref", f) for f in ("newkf_ref_main.c", "newkf_ref.c")]
    subprocess.check_call(["gcc", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe] + src)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "newkf_ref_main: 4680 runs" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(NAMES))
def test_host_array_forms_equal_the_reference(ref, name):
    """spfe_insert_keyframe and spfe_list_observations on the fixtures' host arrays: the same bytes as newkf_ref.c"""
    import newkf_gpu as ng
    from sp_orb_slam_amd import weights
    from sp_orb_slam_amd.extractor import SPExtractor
    c = CASES[name]
    bf16 = c.get("rec_desc") is not None and c["rec_desc"].dtype == np.uint16
    ext = _handle(SPExtractor, weights, bf16)
    want, _ = ng.want_of(ref, c)
    ng.same(ng.run_host(ext, c), want, c, name + ", host form")


_HANDLES = {}


def _handle(SPExtractor, weights, bf16):
    if bf16 not in _HANDLES:
        _HANDLES[bf16] = SPExtractor(nc.KMAX - 1, 64, 96, weights.synthetic(7, "trackable"), with_heat=False, desc_bf16=bf16)
    return _HANDLES[bf16]
