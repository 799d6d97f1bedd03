"""CPU: tests/mp_ref/mp_ref.c, the host reference of the map-point refresh (the statement the GPU kernels of mappoint.hip are held
to bit for bit), against an independent numpy statement in float64 — the full N x N matrix of distances, np.sort, plain vector
algebra —, against its own numbered mutations, and against the recorded fixtures tests/golden/mp_*.npz."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "mp_ref"))
import mp_cases  # noqa: E402
import mp_ref  # noqa: E402

# The largest deviation of mp_ref.c's normal and dist_range from the float64 statement over the fixtures, relative to the
# largest magnitude of the vector it belongs to (measured by test_normal_and_distances_within_four_times_the_measured_deviation
# itself, which prints it): 1.11e-06 for the normal (on the 257-observation point of `codes`, whose f32 sum has 257 terms; 1.2e-07
# on the points of a few observations), 1.11e-07 for dist_range.  The outputs are f32 results of about ten f32 operations an
# observation; the bound is 4 x the measured value and absorbs a different libm sqrt path, nothing more.
MEASURED_NORMAL, MEASURED_RANGE = 1.11e-06, 1.11e-07


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return mp_ref.build(tmp_path_factory.mktemp("mp_ref"))


def centre(T):
    T = T.astype(np.float64).reshape(4, 4)
    return -T[:3, :3].T @ T[:3, 3]


def statement(c):
    """the refresh in float64 on a poisoned table -> dict like mp_ref.refresh's (no block)"""
    m, n_table, n_kf = len(c["ref_slot"]), len(c["xyz"]), len(c["kf_flags"])
    normal, dist_range, desc = mp_ref.poisoned_table(n_table)
    best_obs, n_good, code = np.full(m, -1, np.int32), np.zeros(m, np.int32), np.zeros(m, np.uint8)
    best_median = np.zeros(m, np.float32)
    for i in range(m):
        row = i if c.get("point_idx") is None else int(c["point_idx"][i])
        if not 0 <= row < n_table:
            code[i] = mp_ref.INVALID
            continue
        if not c["flags"][row] & 1:
            code[i] = mp_ref.SKIP_BAD
            continue
        obs = c["obs"][c["obs_start"][i]:c["obs_start"][i + 1]]
        if len(obs) == 0:
            code[i] = mp_ref.NO_OBS
            continue
        ok = 0 <= c["ref_slot"][i] < n_kf
        for slot, kp in obs:
            if not 0 <= slot < n_kf:
                ok = False
            elif c["kf_K"][slot] < 0:
                ok &= bool(c["kf_flags"][slot] & 1)
            else:
                ok &= 0 <= kp < c["kf_K"][slot]
        if not ok:
            code[i] = mp_ref.INVALID
            continue
        good = [o for o, (slot, _) in enumerate(obs) if not c["kf_flags"][slot] & 1]
        N = n_good[i] = len(good)
        code[i] = mp_ref.REFRESHED if not c["mode"] & 1 else mp_ref.NO_GOOD_KF if N == 0 else mp_ref.TOO_MANY if N > 256 else mp_ref.REFRESHED
        P = c["xyz"][row].astype(np.float64)
        if c["mode"] & 2:
            d = P - np.stack([centre(c["Tcw"][slot]) for slot, _ in obs])
            normal[row] = (d / np.linalg.norm(d, axis=1, keepdims=True)).sum(0) / len(obs)
            dist = np.linalg.norm(P - centre(c["Tcw"][c["ref_slot"][i]]))
            dist_range[row] = (dist * float(c["level_scale"]) / float(c["top_scale"]), dist * float(c["level_scale"]))
        if not c["mode"] & 1 or code[i] != mp_ref.REFRESHED:
            continue
        rows = np.stack([c["kf_desc"][obs[o][0], obs[o][1]] for o in good]).astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            D = np.sqrt(((rows[:, None, :] - rows[None, :, :]) ** 2).sum(-1)).astype(np.float32)   # DescriptorDistance returns a float
        D[np.arange(N), np.arange(N)] = 0
        med = np.sort(D, axis=1)[:, int(0.5 * (N - 1))]              # np.sort puts NaN last
        best, bi = np.finfo(np.float32).max, 0
        for a in range(N):
            if med[a] < best:
                best, bi = med[a], a
        best_obs[i], best_median[i], desc[row] = good[bi], best, rows[bi]
    return dict(best_obs=best_obs, n_good=n_good, code=code, best_median=best_median, normal=normal, dist_range=dist_range, desc=desc)


def test_fixtures_exist_and_cover_the_named_cases():
    assert set(mp_cases.NAMES) == set(mp_cases.CASES)


@pytest.mark.parametrize("name", sorted(mp_cases.CASES))
def test_integers_and_chosen_rows_equal_the_float64_statement(ref, name):
    """every code, count, chosen observation and chosen row; on the constructed ties too, which are exact in both"""
    c, _ = mp_cases.load(name)
    r, s = mp_ref.refresh(ref, c), statement(c)
    for k in mp_cases.OUTPUTS:
        assert np.array_equal(r[k], s[k]), (name, k, r[k], s[k])
    assert r["desc"].tobytes() == s["desc"].tobytes(), name
    chosen = r["best_obs"] >= 0
    assert np.allclose(r["best_median"][chosen], s["best_median"][chosen], rtol=3e-7, atol=0), name
    assert r["m"] == len(c["ref_slot"]) and r["n_desc_written"] == int(chosen.sum())
    assert r["n_nd_written"] == (int((r["code"] >= mp_ref.NO_GOOD_KF).sum()) if c["mode"] & 2 else 0)
    assert r["status"] == int(np.bitwise_or.reduce(c["kf_status"][c["kf_K"] >= 0]))


def deviations(r, s):
    """largest |mp_ref.c - statement| over the written rows, relative to the row's largest magnitude: (normal, dist_range)"""
    out = []
    poison = mp_ref.poisoned_table(1)[0][0, 0]
    for k in ("normal", "dist_range"):
        w = s[k][:, 0].view(np.uint32) != poison.view(np.uint32)
        assert np.array_equal(w, r[k][:, 0].view(np.uint32) != poison.view(np.uint32)), k
        a, b = r[k][w].astype(np.float64), s[k][w].astype(np.float64)
        fin = np.isfinite(b).all(1)
        assert np.array_equal(np.isfinite(a).all(1), fin)
        out.append(float((np.abs(a[fin] - b[fin]).max(1) / np.abs(b[fin]).max(1)).max()) if fin.any() else 0.0)
    return out


def test_normal_and_distances_within_four_times_the_measured_deviation(ref):
    worst = [0.0, 0.0]
    for name in sorted(mp_cases.CASES):
        c, _ = mp_cases.load(name)
        d = deviations(mp_ref.refresh(ref, c), statement(c))
        worst = [max(a, b) for a, b in zip(worst, d)]
    print("largest deviation from the float64 statement: normal %.3g, dist_range %.3g" % tuple(worst))
    assert worst[0] <= 4 * MEASURED_NORMAL and worst[1] <= 4 * MEASURED_RANGE
    assert worst[0] > 0 and worst[1] > 0                               # (something was compared)


@pytest.mark.parametrize("mutation", sorted(mp_ref.MUTATIONS))
def test_every_mutation_changes_a_fixture(ref, mutation):
    changed = []
    for name in mp_cases.NAMES:
        c, want = mp_cases.load(name)
        if mp_cases.differences(want, mp_ref.refresh(ref, c, mutate=mp_ref.MUTATIONS[mutation])):
            changed.append(name)
    print(mutation, "changes", changed)
    assert changed, mutation


@pytest.mark.parametrize("name", sorted(mp_cases.CASES))
def test_recorded_fixtures_reproduce(ref, name):
    """the stored inputs give the stored outputs, and the generator still makes the stored inputs"""
    c, want = mp_cases.load(name)
    assert mp_cases.differences(want, mp_ref.refresh(ref, c)) == []
    made = mp_cases.CASES[name]().arrays()
    for k in mp_cases.KEYS + ("kf_desc",):
        assert np.ascontiguousarray(made[k]).tobytes() == np.ascontiguousarray(c[k]).astype(np.asarray(made[k]).dtype).tobytes(), (name, k)


def test_small_counts_follow_the_rule(ref):
    """N = 1: row 0.  N = 2: both medians are the self-distance 0, so row 0.  N = 3 and 4: the median is the least distance
    to another row."""
    c, _ = mp_cases.load("counts")
    r = mp_ref.refresh(ref, c)
    assert list(r["n_good"][:5]) == [1, 2, 3, 4, 5]
    assert r["best_obs"][0] == 0 and r["best_median"][0] == 0 and r["best_obs"][1] == 0 and r["best_median"][1] == 0
    for i in (2, 3):
        obs = c["obs"][c["obs_start"][i]:c["obs_start"][i + 1]]
        rows = np.stack([c["kf_desc"][s, k] for s, k in obs]).astype(np.float64)
        D = np.sqrt(((rows[:, None] - rows[None]) ** 2).sum(-1))
        D[np.arange(len(obs)), np.arange(len(obs))] = np.inf
        assert r["best_obs"][i] == int(D.min(1).argmin()) and abs(r["best_median"][i] - D.min()) < 1e-6


def test_the_cases_hold_what_their_names_say(ref):
    r = {n: mp_ref.refresh(ref, mp_cases.load(n)[0]) for n in ("ties", "nan", "codes", "mode_desc", "mode_nd", "invalid", "permuted")}
    assert list(r["ties"]["best_obs"]) == [0, 0, 0, 0, 1] and list(r["ties"]["best_median"][:3]) == [0, 0, 0]
    assert r["ties"]["best_median"][3] == 5 and r["ties"]["best_median"][4] == 6
    n = r["nan"]
    assert n["best_obs"][0] != 2 and n["best_obs"][1] == 1 and n["best_obs"][2] == 0 and n["best_obs"][3] == 0
    assert n["best_median"][2] == np.finfo(np.float32).max and n["best_median"][3] == 0
    assert np.isnan(n["desc"][2]).all() and n["best_obs"][4] == 0 and n["best_median"][4] == np.finfo(np.float32).max
    assert list(r["codes"]["code"]) == [1, 2, 3, 4, 5, 6, 6] and r["codes"]["n_good"][4] == 257 and r["codes"]["n_good"][6] == 3
    assert list(r["mode_nd"]["code"]) == [1, 2, 3, 6, 6, 6, 6] and r["mode_nd"]["n_desc_written"] == 0
    poison = mp_ref.poisoned_table(7)
    assert r["mode_nd"]["desc"].tobytes() == poison[2].tobytes() and r["mode_desc"]["normal"].tobytes() == poison[0].tobytes()
    assert r["mode_desc"]["dist_range"].tobytes() == poison[1].tobytes() and r["mode_desc"]["n_nd_written"] == 0
    assert r["codes"]["normal"][3].tobytes() != poison[0][3].tobytes() and r["codes"]["desc"][3].tobytes() == poison[2][3].tobytes()
    assert list(r["invalid"]["code"]) == [3] * 7 + [6, 3]
    assert r["invalid"]["desc"][:7].tobytes() == mp_ref.poisoned_table(7)[2].tobytes()
    assert r["permuted"]["desc"][[4, 7]].tobytes() == mp_ref.poisoned_table(2)[2].tobytes()      # rows nobody lists
