"""CPU: tests/cull_ref/cull_ref.c — the oracle of the GPU tests of keyframe culling — held to an independent Python statement of
the reference's lines (tests/cull_ref/cull_cases.py: objects with mObservations dicts, children sets and
mConnectedKeyFrameWeights dicts), on every fixture tests/golden/cull_*.npz and on generated sequences of 48 keyframes in which
UpdateConnections (tests/covis_ref/covis_ref.c) and the cull alternate; told apart from ten one-line misreadings; and the
observation counts kept consistent with a fresh count of the edited rows."""
import glob
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("cull_ref", "covis_ref"):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
import covis_ref  # noqa: E402
import cull_cases as cc  # noqa: E402
import cull_ref  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "cull_*.npz")))
NAMES = [os.path.basename(p)[5:-4] for p in FIXTURES]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return cull_ref.build(tmp_path_factory.mktemp("cull_ref"))


@pytest.fixture(scope="module")
def cref(tmp_path_factory):
    return covis_ref.build(tmp_path_factory.mktemp("covis_ref"))


def against_python(before, after, r, prm):
    """the world cull_ref.c left (`after`, block r) against the Python statement run on `before`"""
    pw = cc.PyWorld(before)
    decided, n_pass, stalled = pw.cull(prm["cur"], prm["th_obs"], prm["cov_ratio"], prm["origin_slot"])
    want = pw.arrays(before)
    # rows: the contract edits them after the last pass and leaves the rows of bad slots alone, so the row of a keyframe culled in
    # this call keeps the points that went bad BEFORE its own cull, where the reference had erased them
    newly_bad = set(pw.bad_points)
    for s in pw.culled:
        assert after["rows"][s].tobytes() == before["rows"][s].tobytes(), ("the row of a culled slot", s)
        for k, (got, py) in enumerate(zip(after["rows"][s].tolist(), want["rows"][s].tolist())):
            assert got == py or (py == -1 and got in newly_bad), (s, k, got, py)
        want["rows"][s] = after["rows"][s]
    for k in ("rows", "kf_flags", "mp_flags", "nobs", "conn_slot", "conn_w", "conn_n", "ord_slot", "ord_w", "ord_n", "parent",
              "first_conn"):
        assert after[k].tobytes() == want[k].tobytes(), (k, np.argwhere(after[k] != want[k])[:6].tolist())
    assert r["n_passes"] == n_pass and bool(r["status"] & cull_ref.STALLED) == stalled
    assert bool(r["status"] & cull_ref.NO_PARENT) == pw.no_parent
    assert r["culled_slot"][:r["n_culled"]].tolist() == pw.culled and r["n_culled"] == len(pw.culled)
    n = len(before["kf_flags"])
    assert r["n_reparented"] == len(pw.events)
    assert list(zip(r["event_child"][:r["n_events"]].tolist(), r["event_parent"][:r["n_events"]].tolist())) == pw.events[:n]
    assert r["n_bad"] == len(pw.bad_points) and r["bad_point"][:r["n_bad_stored"]].tolist() == pw.bad_points[:prm["bad_cap"]]
    assert r["touched_slot"][:r["n_touched"]].tolist() == sorted(pw.touched)
    for j in range(r["n_listed"]):
        s, code = int(r["entry_slot"][j]), int(r["entry_code"][j])
        if code in (cull_ref.ORIGIN, cull_ref.WILD, cull_ref.BAD):
            assert s not in decided or code == cull_ref.BAD
            continue
        assert decided[s] == (r["entry_pass"][j], r["entry_mps"][j], r["entry_red"][j]), (j, s, decided[s])
        assert code == (cull_ref.CULLED if s in pw.culled else cull_ref.DEFERRED if want["kf_flags"][s] & 4 and not before["kf_flags"][s] & 4
                        else cull_ref.STALLED_CODE if stalled and decided[s][0] == n_pass and not _dropped(decided[s], prm) else cull_ref.DROPPED)
    # (7): the table rows of the touched and the culled slots are their ord rows, the others keep their bytes
    written = set(pw.touched) | set(pw.culled)
    for t in ("best_a", "best_b"):
        nb = after[t].shape[1]
        for s in range(n):
            if s in written:
                row = want["ord_slot"][s][:nb].tolist()
                assert after[t][s].tolist() == row + [-1] * (nb - len(row)), (t, s)
            else:
                assert after[t][s].tobytes() == before[t][s].tobytes(), (t, s)


def _dropped(d, prm):
    with np.errstate(all="ignore"):
        return bool(np.float32(d[2]) / np.float32(d[1]) < np.float32(prm["cov_ratio"]))


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_fixture_is_what_cull_ref_gives(ref, path):
    c = cc.load_fixture(path)
    w, r = cull_ref.run_case(ref, c)
    assert r["block"].tobytes() == c["e_block"].tobytes()
    for k in cull_ref.WORLD:
        assert w[k].tobytes() == c["e_" + k].tobytes(), k


def test_fixtures_are_the_named_cases():
    named = cc.named_cases()
    assert sorted(named) == sorted(NAMES) and len(NAMES) >= 20
    for name, path in zip(NAMES, FIXTURES):
        c = cc.load_fixture(path)
        for k in cc.KEYS:
            assert np.asarray(named[name][k]).tobytes() == c[k].tobytes(), (name, k)


# the Python statement keeps one index a keyframe: spfe_cull_math.h (5) states the duplicate case, and its fixture is held to
# cull_ref.c alone
SINGLE = [(p, n) for p, n in zip(FIXTURES, NAMES) if n != "row_names_a_point_twice"]


@pytest.mark.parametrize("path", [p for p, _ in SINGLE], ids=[n for _, n in SINGLE])
def test_cull_ref_equals_the_python_statement_on_the_fixtures(ref, path):
    c = cc.load_fixture(path)
    before = cull_ref.case_world(c)
    w, r = cull_ref.run_case(ref, c)
    against_python(before, w, r, cull_ref.case_params(c))


def test_layout_is_the_headers(ref):
    for n, cap, bc in ((1, 1, 0), (8, 8, 8), (300, 256, 50), (65536, 4096, 262144)):
        v, o = cull_ref.layout(ref, n, cap, bc), cull_ref.offsets(n, cap, bc)
        assert v[:11] == [o[k] for k in ("entry_slot", "entry_code", "entry_pass", "entry_mps", "entry_red", "culled_slot",
                                         "touched_slot", "event_child", "event_parent", "bad_point", "out_bytes")]
        assert v[10] % 256 == 0 and v[10] >= v[9] + 4 * bc
        assert v[11:18] == [cull_ref.STALLED, cull_ref.WILD_ENTRY, cull_ref.BAD_CUT, cull_ref.EVENT_CUT, cull_ref.NO_PARENT,
                            cull_ref.KF_NOT_ERASE, cull_ref.KF_TO_BE_ERASED]


def run_sequence(ref, cref, seed, th, th_obs, cov_ratio, mutate=0, check=True):
    """48 keyframes inserted one by one: UpdateConnections, then the cull -> (culled in all, the worlds' digest)"""
    w, rng, geo = cc.sequence_world(seed)
    n = len(w["kf_flags"])
    n_table = len(w["mp_flags"])
    culled, digest, passes = 0, [], 0
    for s in range(n):
        cc.insert_keyframe(w, rng, geo, s)
        covis_ref.update(cref, w["rows"], w["kf_flags"], w["mp_flags"], {k: w[k] for k in covis_ref.STATE}, s, th, 0, w["best_a"], w["best_b"])
        before = cull_ref.copy_world(w)
        prm = dict(cur=s, th_obs=th_obs, cov_ratio=cov_ratio, origin_slot=0, bad_cap=16)
        r = cull_ref.cull(ref, w, mutate=mutate, **prm)
        if check:
            against_python(before, w, r, prm)
            good = (w["mp_flags"] & 1).astype(bool)
            fresh = cull_ref.count(ref, w["rows"], w["kf_flags"], n_table)
            assert (w["nobs"][good] == fresh[good]).all(), "nobs drifted from the rows"
        culled += r["n_culled"]
        passes = max(passes, r["n_passes"])
        digest.append(r["block"].tobytes() + b"".join(w[k].tobytes() for k in cull_ref.WORLD))
    return culled, passes, digest


@pytest.mark.parametrize("seed,th,th_obs,cov_ratio", [(1, 8, 3, 0.6), (2, 4, 4, 0.5), (3, 12, 3, 0.55), (4, 6, 5, 0.45)])
def test_sequences_equal_the_python_statement_and_keep_nobs_consistent(ref, cref, seed, th, th_obs, cov_ratio):
    culled, passes, _ = run_sequence(ref, cref, seed, th, th_obs, cov_ratio)
    print("culled", culled, "passes in one call", passes)
    assert culled >= 3, culled


def test_count_is_numpy(ref):
    w, _ = cc.generated_world(5, 40, 33, 500, 8, 8, dup=True)
    w["rows"][3, :4] = [-5, 500, 499, 0]
    want = np.zeros(500, np.int64)
    for s in range(40):
        if not w["kf_flags"][s] & 1:
            r = w["rows"][s]
            np.add.at(want, r[(r >= 0) & (r < 500)], 1)
    assert (cull_ref.count(ref, w["rows"], w["kf_flags"], 500) == want).all()


@pytest.mark.parametrize("name", sorted(cull_ref.MUTATIONS))
def test_mutation_is_told_apart(ref, cref, name):
    """every misreading changes the bytes of some fixture or of some generated sequence"""
    m = cull_ref.MUTATIONS[name]
    hit = []
    for path, fname in zip(FIXTURES, NAMES):
        c = cc.load_fixture(path)
        w0, r0 = cull_ref.run_case(ref, c)
        w1, r1 = cull_ref.run_case(ref, c, mutate=m)
        if r0["block"].tobytes() != r1["block"].tobytes() or cull_ref.diff_world(w0, w1):
            hit.append(fname)
    assert hit, name
    print(name, "told apart by", hit)


def test_stall_rule_ends_the_loop_at_cov_ratio_zero(ref):
    """cov_ratio <= 0 at ratio 0: nothing drops, nothing wins"""
    c = cc.named_cases()["nothing_above_ratio"]
    c["nobs"][:] = 1
    c["cov_ratio"] = np.float32(0.0)
    w, r = cull_ref.run_case(ref, c)
    assert r["status"] == cull_ref.STALLED and r["n_passes"] == 1 and r["entry_code"][:4].tolist() == [cull_ref.STALLED_CODE] * 4
    assert not cull_ref.diff_world(w, cull_ref.case_world(c))


def test_cull_ref_runs_clean_under_the_host_sanitizers(tmp_path):
    """cull_ref.c with its stand-alone driver (tests/cull_ref/cull_ref_main.c, a main of its own), built with AddressSanitizer and
    UndefinedBehaviorSanitizer and run as a program on the CPU: any report aborts it"""
    import subprocess
    exe = str(tmp_path / "cull_ref_main")
    src = [os.path.join(ROOT, "tests", "cull_ref", f) for f in ("cull_ref_main.c", "cull_ref.c")]
    subprocess.check_call(["gcc", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe] + src)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "cull_ref_main: 3960 runs" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
