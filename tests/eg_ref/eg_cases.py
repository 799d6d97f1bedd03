"""Essential-graph problems for the reference and GPU tests: the small named cases the fixtures tests/golden/essgraph_*.npz record,
and the generated ones (large, threads, wide_row, lds_edge) that are built on demand and not committed.  numpy only.

A case is a dict: est / meas f64 [n][8] = q(x, y, z, w), t, s; flags uint8 [n] (bit 0 fixed); edges int32 [E][3] = (i, j, kind);
iterations, fix_scale, lambda_init; env_cap where the case sets one."""
import numpy as np

SMALL = ("two_kf", "chain5_loop", "fixed_first", "fixed_middle", "fixed_last", "fix_scale", "duplicate_edges", "isolated_vertex",
         "only_fixed", "skipped_edges", "consistent", "floating_component", "rejected_trials", "corrected_subset",
         "envelope_overflow", "envelope_exact")


def quat_of(R):
    """a unit quaternion (x, y, z, w) of a rotation matrix, w >= 0"""
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    if w > 1e-3:
        q = np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2 * np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1)
        q = np.zeros(4)
        q[i] = s / 4
        q[3] = (R[k, j] - R[j, k]) / s
        q[j] = (R[j, i] + R[i, j]) / s
        q[k] = (R[k, i] + R[i, k]) / s
    return q / np.linalg.norm(q)


def rot_of(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def rodrigues(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def mat_of(S):
    """4x4 [s R | t; 0 0 0 1] of a stored Sim3"""
    M = np.eye(4)
    M[:3, :3] = S[7] * rot_of(S[:4])
    M[:3, 3] = S[4:7]
    return M


def sim_of(M):
    s = np.cbrt(np.linalg.det(M[:3, :3]))
    return np.concatenate([quat_of(M[:3, :3] / s), M[:3, 3], [s]])


def small_motion(rng, rot, trans, scale=0.0):
    M = np.eye(4)
    M[:3, :3] = np.exp(rng.normal(0, scale) if scale else 0.0) * rodrigues(rng.normal(0, rot, 3))
    M[:3, 3] = rng.normal(0, trans, 3)
    return M


def trajectory(rng, n, step_rot=0.08, step_trans=0.5, drift_scale=0.0):
    """n world-to-camera similarities along a path"""
    Ms = [small_motion(rng, 0.3, 1.0)]
    for _ in range(1, n):
        D = small_motion(rng, step_rot, 0.1, drift_scale)
        D[:3, 3] += np.array([0.0, 0.0, step_trans])
        Ms.append(D @ Ms[-1])
    return Ms


def perturbed(rng, Ms, rot, trans, scale):
    return [small_motion(rng, rot, trans, scale) @ M for M in Ms]


def case_of(est, meas, fixed, edges, iterations=20, fix_scale=0, lambda_init=1e-16, env_cap=None):
    n = len(est)
    flags = np.zeros(n, np.uint8)
    flags[list(fixed)] = 1
    c = dict(est=np.stack([sim_of(M) if np.shape(M) == (4, 4) else np.asarray(M, float) for M in est]),
             meas=np.stack([sim_of(M) if np.shape(M) == (4, 4) else np.asarray(M, float) for M in meas]),
             flags=flags, edges=np.asarray(edges, np.int32).reshape(-1, 3), iterations=np.int32(iterations),
             fix_scale=np.int32(fix_scale), lambda_init=np.float64(lambda_init))
    if env_cap is not None:
        c["env_cap"] = np.int32(env_cap)
    return c


def chain_edges(n, kind=1):
    return [(v - 1, v, kind) for v in range(1, n)]


def small(name, seed=0, iterations=20):
    rng = np.random.default_rng(1000 + seed)
    if name == "two_kf":
        meas = trajectory(rng, 2)
        est = [meas[0], perturbed(rng, meas[1:], 0.02, 0.05, 0.02)[0]]
        return case_of(est, meas, [0], [(0, 1, 1)], iterations)
    if name == "chain5_loop":
        meas = trajectory(rng, 5, drift_scale=0.02)
        est = list(meas)
        est[4] = small_motion(rng, 0.05, 0.2, 0.05) @ meas[4]   # the corrected current keyframe
        return case_of(est, meas, [0], chain_edges(5) + [(4, 0, 0)], iterations)
    if name in ("fixed_first", "fixed_middle", "fixed_last"):
        meas = trajectory(rng, 6)
        est = perturbed(rng, meas, 0.02, 0.05, 0.02)
        fixed = {"fixed_first": 0, "fixed_middle": 3, "fixed_last": 5}[name]
        est[fixed] = meas[fixed]
        return case_of(est, meas, [fixed], chain_edges(6) + [(0, 2, 1), (1, 4, 1), (3, 5, 1), (5, 0, 1)], iterations)
    if name == "fix_scale":
        meas = trajectory(rng, 5)
        est = perturbed(rng, meas, 0.02, 0.05, 0.03)
        est[0] = meas[0]
        return case_of(est, meas, [0], chain_edges(5) + [(4, 0, 1), (1, 3, 1)], iterations, fix_scale=1)
    if name == "duplicate_edges":
        meas = trajectory(rng, 5)
        est = perturbed(rng, meas, 0.02, 0.05, 0.02)
        est[0] = meas[0]
        return case_of(est, meas, [0], chain_edges(5) + [(1, 2, 1), (2, 1, 1), (4, 0, 1), (0, 4, 1), (4, 0, 0)], iterations)
    if name == "isolated_vertex":
        meas = trajectory(rng, 5)
        est = perturbed(rng, meas, 0.02, 0.05, 0.02)
        est[0] = meas[0]
        return case_of(est, meas, [0], [(0, 1, 1), (1, 3, 1), (3, 4, 1), (4, 0, 1)], iterations)
    if name == "only_fixed":
        meas = trajectory(rng, 3)
        est = perturbed(rng, meas, 0.02, 0.05, 0.02)
        return case_of(est, meas, [0, 1, 2], chain_edges(3), iterations)
    if name == "skipped_edges":
        meas = trajectory(rng, 5)
        est = perturbed(rng, meas, 0.02, 0.05, 0.02)
        est[0] = meas[0]
        edges = [(0, 1, 1), (7, 0, 1), (1, 2, 1), (2, 2, 1), (2, 3, 1), (0, 1, 5), (3, 4, 1), (-1, 2, 0), (4, 0, 1), (1, 5, 0),
                 (2, 4, -1)]
        return case_of(est, meas, [0], edges, iterations)
    if name == "consistent":
        # identity rotations, integer translations, scale 1: every product is exact, every error exactly zero
        meas = [np.array([0, 0, 0, 1.0, 3 * v, -2 * v, v * v, 1.0]) for v in range(5)]
        return case_of(meas, meas, [0], chain_edges(5) + [(4, 0, 1), (1, 3, 1)], iterations)
    if name == "floating_component":
        meas = trajectory(rng, 4)
        est = perturbed(rng, meas, 0.02, 0.05, 0.02)
        est[0] = meas[0]
        return case_of(est, meas, [0], [(0, 1, 1), (2, 3, 1)], iterations)
    if name == "rejected_trials":
        meas = trajectory(rng, 6, step_rot=0.3)
        est = perturbed(rng, meas, 1.0, 1.0, 2.0)   # scales off by e^2: Gauss-Newton steps overshoot
        est[0] = meas[0]
        return case_of(est, meas, [0], chain_edges(6) + [(5, 0, 1), (2, 4, 1), (1, 5, 1)], iterations)
    if name == "corrected_subset":
        meas = trajectory(rng, 10, drift_scale=0.01)
        est = list(meas)
        C = small_motion(rng, 0.04, 0.3, 0.06)
        for v in (6, 7, 8, 9):
            est[v] = C @ small_motion(rng, 0.002, 0.01) @ meas[v]
        edges = [(9, 0, 0), (9, 1, 0), (8, 0, 0), (7, 1, 0)] + chain_edges(10) + [(0, 2, 1), (3, 6, 1), (5, 8, 1), (2, 7, 1)]
        return case_of(est, meas, [0], edges, iterations)
    if name in ("envelope_overflow", "envelope_exact"):
        meas = trajectory(rng, 6)
        est = perturbed(rng, meas, 0.02, 0.05, 0.02)
        est[0] = meas[0]
        edges = chain_edges(6) + [(5, 1, 1)]
        # unknowns 0 .. 4 = slots 1 .. 5; rows 0 1 2 3 hold 1, 2, 2, 2 blocks, row 4 (slot 5, adjacent to slot 1) holds 5: 12
        return case_of(est, meas, [0], edges, iterations, env_cap=11 if name == "envelope_overflow" else 12)
    raise KeyError(name)


def large(seed=0, n=1000):
    """n keyframes in a chain with 3 - 6 covisibility edges each, one loop of 8 x 8 kind-0 connections between the last and the
    first twenty, 1 % noise"""
    rng = np.random.default_rng(2000 + seed)
    true = trajectory(rng, n, step_rot=0.03, step_trans=0.3)
    # the odometry drifts: 1 % noise on every relative motion, accumulated
    meas = [true[0]]
    for v in range(1, n):
        rel = true[v] @ np.linalg.inv(true[v - 1])
        meas.append(small_motion(rng, 0.01 * 0.03, 0.01 * 0.3, 0.0005) @ rel @ meas[-1])
    est = list(meas)
    # the current keyframe and its connected ones, corrected onto the loop side
    C = true[n - 1] @ np.linalg.inv(meas[n - 1])
    for v in range(n - 20, n):
        est[v] = C @ meas[v]
    edges = []
    last8 = rng.choice(np.arange(n - 20, n), 8, replace=False)
    first8 = rng.choice(np.arange(0, 20), 8, replace=False)
    for a in last8:
        for b in first8:
            edges.append((int(a), int(b), 0))
    for v in range(1, n):
        edges.append((v - 1, v, 1))
    for v in range(n):
        for d in rng.choice(np.arange(2, 9), int(rng.integers(2, 6)), replace=False):
            if v + d < n:
                edges.append((v, int(v + d), 1))
    return case_of(est, meas, [0], edges)


def banded(n_unknown, seed=0, band=2, wide_row=False, iterations=3):
    """n_unknown free keyframes behind one fixed one, every one tied to its `band` predecessors; wide_row: the last also to the
    first unknown, so that its envelope spans all of them"""
    rng = np.random.default_rng(3000 + seed + n_unknown)
    n = n_unknown + 1
    meas = trajectory(rng, n, step_rot=0.03, step_trans=0.3)
    est = perturbed(rng, meas, 0.005, 0.02, 0.005)
    est[0] = meas[0]
    edges = [(v - d, v, 1) for v in range(1, n) for d in range(1, band + 1) if v - d >= 0]
    if wide_row:
        edges.append((n - 1, 1, 1))
    return case_of(est, meas, [0], edges, iterations)


def star(n_leaves, seed=0, iterations=2):
    """unknown 0 tied to every other unknown: the panel of block column 0 has n_leaves block rows"""
    rng = np.random.default_rng(4000 + seed + n_leaves)
    n = n_leaves + 2
    meas = trajectory(rng, n, step_rot=0.03, step_trans=0.3)
    est = perturbed(rng, meas, 0.005, 0.02, 0.005)
    est[0] = meas[0]
    edges = [(0, 1, 1)] + [(1, v, 1) for v in range(2, n)]
    return case_of(est, meas, [0], edges, iterations)


def repeated_pair(copies=2000, seed=0, iterations=2):
    """a band of 2 over 40 unknowns with ONE pair's edge given `copies` times, in both directions and interleaved with the band's
    edges: two adjacency lists of that length, spread over several chunks of the list build"""
    c = banded(40, seed, iterations=iterations)
    rng = np.random.default_rng(5000 + seed)
    extra = np.array([(7, 9, 1) if k % 2 else (9, 7, 1) for k in range(copies)], np.int32)
    edges = np.concatenate([c["edges"], extra])
    c["edges"] = np.ascontiguousarray(edges[rng.permutation(len(edges))])
    return c
