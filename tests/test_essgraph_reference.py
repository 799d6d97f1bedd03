"""CPU: the essential graph's host reference (tests/eg_ref/eg_ref.c, built from include/spfe_essgraph_math.h: block skyline
Cholesky, fixed summation orders, its own log / acos / sin / cos / exp) against the independent float64 statement of
tests/golden/make_golden_essgraph.py (4x4 matrices, scipy's expm / logm, the full dense normal equations), whose results the
fixtures tests/golden/essgraph_*.npz record.

Every integer of the block must be equal: the generator cuts a fixture's iteration count where a trial stops moving chi2 by a
margin (see its docstring), so no count can flip on rounding.

Measured on the fixtures (x86-64, gcc 13, numpy 2 / scipy 1.15): the largest |estimate (statement) - estimate (eg_ref.c)| over
the entries of the 4x4 matrices [s R | t] is
  8.314e-14  (fixed_last)        on the graphs whose measurements agree with one another: MEASURED_DEV
  1.315e-07  (corrected_subset)  on those that keep a residual at the optimum (chain5_loop, fix_scale, duplicate_edges,
             corrected_subset): the numeric Jacobian carries logm's and the header's last-place errors times 5e8, and with a
             residual that noise moves the step: MEASURED_DEV_RESIDUAL
  9.428e-05  on rejected_trials, whose one iteration leaves chi2 at 54 (scales off by e^2 at the start): MEASURED_DEV_REJECTED
  floating_component: the pair that is not tied to the fixed vertex has seven free directions, a solved trial moves it along
             them at will (4.6e-02 between the two statements); the pinned vertices and the pair's RELATIVE similarity (measured:
             1.6e-15) are held to MEASURED_DEV.
Every bound is 4 times the measured value of the fixture's group."""
import glob
import os
import sys

import numpy as np
import pytest
from scipy.linalg import expm, logm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "eg_ref"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import eg_cases  # noqa: E402
import eg_ref  # noqa: E402
import make_golden_essgraph as stmt  # noqa: E402

from sp_orb_slam_amd.extractor import SPExtractor as X  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = stmt.NAMES
RESIDUAL = ("chain5_loop", "fix_scale", "duplicate_edges", "corrected_subset")
MEASURED_DEV = 8.314e-14
MEASURED_DEV_RESIDUAL = 1.315e-07
MEASURED_DEV_REJECTED = 9.428e-05
MEASURED_LOG = 5.1e-15        # |spfe_eg_log - logm| over the four branches, relative to max(1, |e|)
MEASURED_EXP_LOG = 1.2e-08    # |log(exp(u)) - u|: the small-angle branch takes omega = dR / 2, off by theta^3 / 6 below theta = 4.5e-3


def est_bound(name):
    return 4 * (MEASURED_DEV_RESIDUAL if name in RESIDUAL else MEASURED_DEV_REJECTED if name == "rejected_trials" else MEASURED_DEV)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return eg_ref.build(tmp_path_factory.mktemp("eg_ref"))


def load(name):
    return dict(np.load(os.path.join(GOLDEN, "essgraph_%s.npz" % name)))


def mats(sim3):
    return np.stack([eg_cases.mat_of(S) for S in sim3])


def agrees(L, name, verbose=False):
    """the acceptance of one fixture: -> None, or what differs"""
    g = load(name)
    r = eg_ref.solve(L, g)
    if [r[k] for k in eg_ref.INTS] != [int(v) for v in g["exp_ints"]]:
        return "integers %s against %s" % ([r[k] for k in eg_ref.INTS], g["exp_ints"].tolist())
    if r["rejected"] != int(g["exp_rejected"]) or r["accepted"] != int(g["exp_accepted"]):
        return "rejected / accepted"
    M, E = mats(r["sim3"]), g["exp_M"]
    if name == "floating_component":
        dev = float(np.abs(M[:2] - E[:2]).max())
        rel = float(np.abs(M[3] @ np.linalg.inv(M[2]) - E[3] @ np.linalg.inv(E[2])).max())
        if verbose:
            print("%s: relative similarity of the floating pair %.3e" % (name, rel))
        if rel > est_bound(name):
            return "floating pair %.3e" % rel
    else:
        dev = float(np.abs(M - E).max())
    if verbose:
        print("%s: |estimate - statement| %.3e" % (name, dev))
    if dev > est_bound(name):
        return "estimates %.3e" % dev
    # the poses: [R | t / s] of the block's own Sim3
    for v in range(len(M)):
        s = r["sim3"][v, 7]
        T = np.eye(4)
        T[:3, :3] = M[v, :3, :3] / s
        T[:3, 3] = M[v, :3, 3] / s
        if np.abs(r["Tiw"][v].reshape(4, 4) - T).max() > 4e-7 * max(1.0, np.abs(T).max()):
            return "Tiw of slot %d" % v
    if r["iterations"]:
        if abs(r["chi2_initial"] - float(g["exp_chi2"][0])) > 1e-9 * max(1.0, r["chi2_initial"]):
            return "chi2_initial"
        # chi2 = sum |e|^2 moves by at most 2 sqrt(chi2) sqrt(E) K d for estimates d apart, K = 10 the Lipschitz constant of an
        # error in an entry of its vertices (translations of some units)
        slack = 2 * np.sqrt(r["chi2_final"] * r["n_edges_followed"]) * 10 * est_bound(name)
        if abs(r["chi2_final"] - float(g["exp_chi2"][1])) > 1e-6 * max(1e-6, r["chi2_final"]) + 1e-18 + slack:
            return "chi2_final"
    return None


def test_fixture_set_is_complete():
    have = sorted(os.path.basename(p)[9:-4] for p in glob.glob(os.path.join(GOLDEN, "essgraph_*.npz")))
    assert have == sorted(NAMES)
    for name in NAMES:
        assert os.path.getsize(os.path.join(GOLDEN, "essgraph_%s.npz" % name)) < 32 * 1024
        assert len(load(name)["flags"]) <= 16


@pytest.mark.parametrize("name", NAMES)
def test_reference_agrees_with_the_independent_statement(ref, name):
    assert agrees(ref, name, verbose=True) is None


def test_fixtures_are_what_their_names_say(ref):
    S = {name: (load(name), eg_ref.solve(ref, load(name))) for name in NAMES}
    g, r = S["two_kf"]
    assert r["n_unknown"] == 1 and r["n_edges_followed"] == 1 and g["flags"].tolist() == [1, 0] and r["chi2_final"] < r["chi2_initial"]
    g, r = S["chain5_loop"]
    assert (g["edges"][:, 2] == 0).sum() == 1 and not np.array_equal(g["est"][4], g["meas"][4]) and r["n_unknown"] == 4
    for name, fixed in (("fixed_first", 0), ("fixed_middle", 3), ("fixed_last", 5)):
        g, r = S[name]
        assert np.flatnonzero(g["flags"]).tolist() == [fixed] and r["sim3"][fixed].tobytes() == g["est"][fixed].tobytes()
        assert r["n_unknown"] == 5 and not np.array_equal(r["sim3"], g["est"])
    g, r = S["fix_scale"]
    assert int(g["fix_scale"]) == 1 and np.abs(r["sim3"][:, 7] / g["est"][:, 7] - 1).max() < 1e-12 and r["chi2_final"] < r["chi2_initial"]
    g, r = S["duplicate_edges"]
    pairs = [tuple(sorted(e[:2])) for e in g["edges"].tolist()]
    assert len(set(pairs)) < len(pairs) and r["n_skipped"] == 0
    g, r = S["isolated_vertex"]
    assert 2 not in g["edges"][:, :2] and r["sim3"][2].tobytes() == g["est"][2].tobytes() and r["n_unknown"] == 3
    g, r = S["only_fixed"]
    assert r["status"] == eg_ref.EMPTY and r["sim3"].tobytes() == g["est"].tobytes() and r["iterations"] == 0 and r["n_edges_followed"] == 2
    g, r = S["skipped_edges"]
    assert r["n_skipped"] == 6 and r["n_edges_followed"] == 5 and r["status"] == eg_ref.OK
    g, r = S["consistent"]
    assert r["chi2_initial"] == 0.0 and r["chi2_final"] == 0.0 and (r["iterations"], r["trials"]) == (1, 1) and r["min_rho"] == 0.0
    assert r["sim3"].tobytes() == g["est"].tobytes()
    g, r = S["floating_component"]
    assert r["n_solve_failed"] >= 1 and r["lambda_final"] > 1e-16 and r["trials"] > r["iterations"]
    g, r = S["rejected_trials"]
    assert r["rejected"] >= 1 and r["accepted"] >= 1
    g, r = S["corrected_subset"]
    assert (np.abs(g["est"] - g["meas"]).max(axis=1) > 0).sum() == 4 and set(g["edges"][:, 2].tolist()) == {0, 1}
    g, r = S["envelope_overflow"]
    assert r["status"] == eg_ref.ENVELOPE_OVERFLOW and r["env_blocks"] == int(g["env_cap"]) + 1 and r["sim3"].tobytes() == g["est"].tobytes()
    g, r = S["envelope_exact"]
    assert r["status"] == eg_ref.OK and r["env_blocks"] == int(g["env_cap"]) and np.array_equal(g["edges"], S["envelope_overflow"][0]["edges"])
    # recovered poses of an echo: [R | t / s] all the same
    g, r = S["only_fixed"]
    assert np.isfinite(r["Tiw"]).all() and (r["Tiw"][:, 15] == 1).all()


def symbolic_cholesky(flags, edges):
    """brute force: the unknowns, and the boolean block pattern of L by elimination"""
    n = len(flags)
    fe = stmt.followed(edges, n)
    touched = {v for e in fe for v in e[:2]}
    unk = {}
    for v in range(n):
        if v in touched and not (int(flags[v]) & 1):
            unk[v] = len(unk)
    U = len(unk)
    A = np.eye(U, dtype=bool)
    for i, j, _ in fe:
        if i in unk and j in unk:
            A[unk[i], unk[j]] = A[unk[j], unk[i]] = True
    first_direct = [int(np.flatnonzero(A[u, :u + 1])[0]) for u in range(U)]
    Lp = np.tril(A)
    for k in range(U):
        rows = np.flatnonzero(Lp[k + 1:, k]) + k + 1
        for a in rows:
            Lp[a, rows[rows <= a]] = True
    return U, first_direct, Lp


def check_envelope(ref, flags, edges):
    U, first_direct, Lp = symbolic_cholesky(flags, edges)
    blocks, nu, first = X.essential_graph_envelope(flags, edges)
    assert (blocks, nu, first.tolist()) == (sum(u - first_direct[u] + 1 for u in range(U)), U, first_direct)
    rb, ru, rf = eg_ref.envelope(ref, flags, edges)
    assert (rb, ru, rf.tolist()) == (blocks, nu, first.tolist())
    for u in range(U):
        assert not Lp[u, :first[u]].any(), "a nonzero of L lies outside the envelope"


def test_envelope_against_a_brute_force_symbolic_cholesky(ref):
    for name in NAMES:
        g = load(name)
        check_envelope(ref, g["flags"], g["edges"])
    rng = np.random.default_rng(11)
    for _ in range(50):
        n = int(rng.integers(2, 41))
        E = int(rng.integers(0, 4 * n))
        edges = np.stack([rng.integers(-1, n + 1, E), rng.integers(-1, n + 1, E), rng.integers(-1, 3, E)], 1).astype(np.int32)
        flags = (rng.random(n) < 0.15).astype(np.uint8) | (rng.integers(0, 2, n) * 2).astype(np.uint8)   # bit 1 is ignored
        check_envelope(ref, flags, edges)


def sim_of_update(u):
    return eg_cases.sim_of(expm(stmt.generator(np.asarray(u, float))))


@pytest.mark.parametrize("sigma,theta,branch", [(0.0, 1e-4, 0), (3e-6, 2e-3, 0), (0.0, 0.7, 1), (-4e-6, 2.9, 1), (0.3, 1e-3, 2), (-0.8, 3e-3, 2),
                                                (0.5, 1.1, 3), (-1.2, 3.0, 3), (0.99e-5, 0.5, 1), (1.01e-5, 0.5, 3),
                                                (0.2, 0.99 * np.sqrt(2e-5), 2), (0.2, 1.01 * np.sqrt(2e-5), 3)])
def test_sim3_log_against_logm_in_every_branch(ref, sigma, theta, branch):
    rng = np.random.default_rng(int(1e6 * theta) + 7)
    axis = rng.normal(size=3)
    u = np.concatenate([theta * axis / np.linalg.norm(axis), rng.normal(0, 2.0, 3), [sigma]])
    S = sim_of_update(u)
    e, br = eg_ref.log(ref, S)
    assert br == branch
    want = stmt.sim_log(eg_cases.mat_of(S))
    # the published algorithm's own approximations below its thresholds: C = 1 and the sigma-free A, B are off by |sigma| at
    # most (relative, in upsilon), omega = dR / 2 = sin(theta) axis and A = 1 / 2, B = 1 / 6 by theta^2 at most
    approx = (abs(sigma) if branch in (0, 1) else 0.0) + (theta ** 2 if branch in (0, 2) else 0.0)
    dev = float(np.abs(e - want).max() / max(1.0, np.abs(want).max()))
    print("branch %d: |log - logm| %.3e" % (br, dev))
    assert dev <= 4 * MEASURED_LOG + approx
    back, _ = eg_ref.exp_update(ref, e)
    assert np.abs(eg_cases.mat_of(back) - eg_cases.mat_of(S)).max() <= (4 * MEASURED_EXP_LOG + 2 * approx) * max(1.0, np.abs(S[4:7]).max())
    back2, _ = eg_ref.exp(ref, e)   # spfe_s3o_exp (libm) and the header's own agree to the last places
    assert np.abs(back2 - back).max() <= 1e-14 * max(1.0, np.abs(back).max())


def test_the_headers_elementary_functions(ref):
    import math
    L = ref
    rng = np.random.default_rng(2)
    for _ in range(4000):
        x = float(np.exp(rng.uniform(-30, 30)))
        assert abs(eg_ref.elementary(L, x)[0] - math.log(x)) <= 4 * np.spacing(max(abs(math.log(x)), 1e-16))
        d = float(rng.uniform(-1, 1)) if rng.random() < 0.5 else 1 - float(np.exp(rng.uniform(-12, -0.1)))
        assert abs(eg_ref.elementary(L, d)[1] - math.acos(d)) <= 4 * np.spacing(math.acos(d))
        t = float(rng.uniform(0, 10))
        o = eg_ref.elementary(L, t)
        assert abs(o[2] - math.sin(t)) <= 1e-15 and abs(o[3] - math.cos(t)) <= 1e-15
        s = float(rng.uniform(-20, 20))
        assert abs(eg_ref.elementary(L, s)[4] - math.exp(s)) <= 4 * np.spacing(math.exp(s))
    assert np.isnan(eg_ref.elementary(L, -1.0)[0]) and np.isnan(eg_ref.elementary(L, 0.0)[0]) and np.isnan(eg_ref.elementary(L, 1.5)[1])
    assert eg_ref.elementary(L, 1.0)[0] == 0.0 and eg_ref.elementary(L, 1.0)[1] == 0.0


def correction_case(seed=5, n_kf=7, n_table=400):
    rng = np.random.default_rng(seed)
    S_from = np.stack([eg_cases.sim_of(eg_cases.small_motion(rng, 0.5, 2.0, 0.2)) for _ in range(n_kf)])
    S_to = np.stack([eg_cases.sim_of(eg_cases.small_motion(rng, 0.5, 2.0, 0.2)) for _ in range(n_kf)])
    xyz = rng.normal(0, 5, (n_table, 3)).astype(np.float32)
    flags = (rng.random(n_table) < 0.9).astype(np.uint8) | (rng.integers(0, 2, n_table) * 4).astype(np.uint8)
    idx = rng.permutation(n_table)[:n_table * 3 // 4].astype(np.int32)
    ref_slot = rng.integers(0, n_kf, len(idx)).astype(np.int32)
    idx[:4] = [-1, n_table, n_table + 7, -3]
    ref_slot[4:8] = [-1, n_kf, n_kf + 2, -5]
    xyz[idx[8]] = np.nan
    xyz[idx[9], 1] = np.inf
    flags[idx[4:10]] |= 1
    return S_from, S_to, ref_slot, idx, xyz, flags


def correction_agrees(L):
    S_from, S_to, ref_slot, idx, xyz, flags = correction_case()
    out, code = eg_ref.correct(L, S_from, S_to, ref_slot, idx, xyz, flags)
    want_code = np.full(len(idx), eg_ref.CORRECTED, np.uint8)
    row_ok = (idx >= 0) & (idx < len(xyz))
    want_code[~row_ok] = eg_ref.INVALID
    bad = row_ok & ((flags[np.clip(idx, 0, len(xyz) - 1)] & 1) == 0)
    want_code[bad] = eg_ref.SKIP_BAD
    want_code[row_ok & ~bad & ((ref_slot < 0) | (ref_slot >= len(S_from)))] = eg_ref.INVALID
    if not np.array_equal(code, want_code):
        return "codes"
    touched = np.zeros(len(xyz), bool)
    for i in np.flatnonzero(code == eg_ref.CORRECTED):
        row, r = idx[i], ref_slot[i]
        touched[row] = True
        X4 = np.append(xyz[row].astype(np.float64), 1.0)
        with np.errstate(invalid="ignore"):
            Y = (np.linalg.inv(eg_cases.mat_of(S_to[r])) @ eg_cases.mat_of(S_from[r]) @ X4)[:3]
        if not np.isfinite(xyz[row]).all():
            if np.isfinite(out[row]).all():
                return "a NaN row came out finite"
            continue
        # one f32 rounding of a double result that is itself good to 1e-12 here (coordinates of some units)
        if (np.abs(out[row].astype(np.float64) - Y) > np.spacing(np.abs(Y).astype(np.float32)).astype(np.float64) + 1e-12).any():
            return "row %d" % row
    if out[~touched].tobytes() != xyz[~touched].tobytes():
        return "a row that is not listed was written"
    return None


def test_point_correction_against_float64_matrices(ref):
    assert correction_agrees(ref) is None


def test_pure_host_twins_on_their_fixtures(ref):
    rng = np.random.default_rng(9)
    n = 12
    Tcw = np.stack([eg_cases.mat_of(eg_cases.sim_of(eg_cases.small_motion(rng, 0.8, 3.0))) for _ in range(n)]).astype(np.float32)
    Tcw2 = eg_cases.small_motion(rng, 0.8, 3.0).astype(np.float32)
    cur = 7
    Twc = np.linalg.inv(Tcw[cur].astype(np.float64)).astype(np.float32)
    S12m = eg_cases.small_motion(rng, 0.2, 0.5, 0.1)
    s = np.cbrt(np.linalg.det(S12m[:3, :3]))
    S12 = np.concatenate([[s], (S12m[:3, :3] / s).reshape(-1), S12m[:3, 3]])
    conn = np.array([7, 3, 11, -2, 40, 5], np.int32)
    est, meas = X.essential_graph_sim3(Tcw, S12, Tcw2, Twc, conn, cur)
    r_est, r_meas = eg_ref.sim3(ref, Tcw, S12, Tcw2, Twc, conn, cur)
    assert est.tobytes() == r_est.tobytes() and meas.tobytes() == r_meas.tobytes()
    listed = [3, 5, 7, 11]
    others = [v for v in range(n) if v not in listed]
    assert est[others].tobytes() == meas[others].tobytes() and (meas[:, 7] == 1.0).all()
    for v in range(n):   # Sim3(R, t, 1) of the pose
        assert np.abs(eg_cases.mat_of(meas[v]) - Tcw[v].astype(np.float64)).max() < 1e-6
    # the f32 cast of the corrected Sim3 is the d_Siw of the corrected poses, bit for bit
    Siw, _ = X.loop_corrected_poses(S12, Tcw2, Twc, Tcw[listed], cur_index=listed.index(cur))
    for k, v in enumerate(listed):
        M = eg_cases.mat_of(est[v])
        assert np.abs(M - Siw[k].astype(np.float64)).max() <= 4e-7 * max(1.0, np.abs(M).max())
    Scw = S12m @ Tcw2.astype(np.float64)
    assert np.abs(eg_cases.mat_of(est[cur]) - Scw).max() < 1e-5
    # the library's envelope refuses what it cannot size
    from sp_orb_slam_amd import extractor
    with pytest.raises(extractor.SpfeError):
        X.essential_graph_envelope(np.zeros(0, np.uint8), np.zeros((0, 3), np.int32))


def jacobian_is_central(L, fix_scale=0):
    """bit for bit: column d = (1 / (2 delta)) (e(+) - e(-)) of the contract's error at spfe_s3o_perturb's estimates"""
    rng = np.random.default_rng(31)
    scalar = 1.0 / (2 * 1e-9)
    for _ in range(5):
        Si, Sj = [eg_cases.sim_of(eg_cases.small_motion(rng, 0.7, 2.0, 0.2)) for _ in range(2)]
        Sji = eg_cases.sim_of(eg_cases.small_motion(rng, 0.05, 0.3, 0.05) @ eg_cases.mat_of(Sj) @ np.linalg.inv(eg_cases.mat_of(Si)))
        Ji, Jj = eg_ref.jacobian(L, Sji, Si, Sj, fix_scale)
        for d in range(7):
            ci = scalar * (eg_ref.error(L, Sji, eg_ref.perturb(L, Si, 2 * d, fix_scale)[0], Sj) -
                           eg_ref.error(L, Sji, eg_ref.perturb(L, Si, 2 * d + 1, fix_scale)[0], Sj))
            cj = scalar * (eg_ref.error(L, Sji, Si, eg_ref.perturb(L, Sj, 2 * d, fix_scale)[0]) -
                           eg_ref.error(L, Sji, Si, eg_ref.perturb(L, Sj, 2 * d + 1, fix_scale)[0]))
            if ci.tobytes() != Ji[:, d].tobytes() or cj.tobytes() != Jj[:, d].tobytes():
                return "column %d" % d
        if fix_scale and (Ji[:, 6].any() or Jj[:, 6].any()):
            return "fix_scale leaves column 6"
        # and it is the derivative: against the statement's logm at the same step, to the rounding of a difference over 2e-9
        Ms = [eg_cases.mat_of(x) for x in (Sji, Si, Sj)]
        for d in range(6 if fix_scale else 7):
            u = np.zeros(7)
            u[d] = 1e-9
            col = (stmt.sim_log(Ms[0] @ expm(stmt.generator(u)) @ Ms[1] @ np.linalg.inv(Ms[2])) -
                   stmt.sim_log(Ms[0] @ expm(stmt.generator(-u)) @ Ms[1] @ np.linalg.inv(Ms[2]))) * scalar
            if np.abs(col - Ji[:, d]).max() > 1e-5 * max(1.0, np.abs(col).max()):
                return "column %d against logm: %.3e" % (d, np.abs(col - Ji[:, d]).max())
    return None


def test_jacobians_are_central_differences(ref):
    assert jacobian_is_central(ref) is None and jacobian_is_central(ref, fix_scale=1) is None


MUTATION_SHOWS_ON = {"KIND": "chain5_loop", "SWAP": "two_kf", "TAU": "fixed_first", "ONESIDED": "jacobian", "FIXED_BLOCK": "fixed_middle",
                     "ENV_OFF": "envelope_exact", "NO_TS": "chain5_loop", "NO_INV": None}


@pytest.mark.parametrize("mutation", eg_ref.MUTATIONS)
def test_single_changes_of_the_contract_are_told_apart(tmp_path, mutation):
    """each is a one-line change of the contract, switched on by a build flag of eg_ref.c"""
    L = eg_ref.build(tmp_path, mutation)
    name = MUTATION_SHOWS_ON[mutation]
    what = correction_agrees(L) if name is None else jacobian_is_central(L) if name == "jacobian" else agrees(L, name)
    print("%s: %s" % (mutation, what))
    assert what is not None
