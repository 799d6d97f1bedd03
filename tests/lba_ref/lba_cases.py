"""The cases of the gather in front of the local bundle adjustment and of the application behind it, as plain numpy — no library
needed to build them — and an independent Python statement of the reference's lines (optimizer.cpp:447-499, :568-658, :660-662,
:739-773): map points as objects with an mObservations list in slot order, keyframes as mvpMapPoints lists, the mnBALocalForKF /
mnBAFixedForKF stamps as sets, and the SEQUENTIAL erase loop with its SetBadFlag cascade and mpRefKF rule.

A gather case: dict(op="gather", the WORLD arrays of lba_ref, ord_row int32 [conn_cap], the GATHER_PARAMS).
An apply case:  dict(op="apply", the WORLD arrays, gather = the gather's block (made by the Python statement), ba = the solver's block
(lba_ref.ba_block), the APPLY_PARAMS); wild=True marks a case whose blocks name things that do not exist: the Python statement
does not model those, lba_ref.c alone is the oracle there."""
import numpy as np

import lba_ref as lr



# ---- the Python statement -----------------------------------------------------------------------------------------------------------
def _observations(c):
    """p -> [(slot, keypoint)] in slot order over the keyframes that are not bad: mObservations"""
    nt = len(c["mp_flags"])
    obs = {}
    for s in range(c["rows"].shape[0]):
        if c["kf_flags"][s] & 1:
            continue
        for k, p in enumerate(c["rows"][s].tolist()):
            if 0 <= p < nt:
                obs.setdefault(p, []).append((s, k))
    return obs


def py_gather(c):
    """-> the gather's block as bytes, every byte"""
    rows, kf_flags, mp_flags = c["rows"], c["kf_flags"], c["mp_flags"]
    n_slots, stride = rows.shape
    nt = len(mp_flags)
    cur, origin = int(c["cur_slot"]), int(c["origin_slot"])
    kf_cap, free_cap, point_cap, edge_cap = (int(c[k]) for k in ("kf_cap", "free_cap", "point_cap", "edge_cap"))
    obs = _observations(c)
    status = 0
    local, n_free = [cur], int(cur != origin)                      # lLocalKeyFrames, mnBALocalForKF
    for s in c["ord_row"].tolist():
        if s == -1:
            break
        if not 0 <= s < n_slots or s == cur or s in local or kf_flags[s] & 1:
            continue
        free = s != origin
        if len(local) + 1 > kf_cap or n_free + free > free_cap:
            status |= lr.LOCAL_CUT
            break
        local.append(s)
        n_free += free
    points, stamped = [], set()                                    # lLocalMapPoints
    for s in local:
        if kf_flags[s] & 1:
            continue
        for p in rows[s].tolist():
            if 0 <= p < nt and mp_flags[p] & 1 and p not in stamped:
                stamped.add(p)
                if len(points) < point_cap:
                    points.append(p)
    if len(stamped) > point_cap:
        status |= lr.POINT_CUT
    fixed = []                                                     # lFixedCameras, mnBAFixedForKF
    for p in points:
        for s, _ in obs.get(p, []):
            if s in local or s in fixed:
                continue
            if len(local) + len(fixed) == kf_cap:
                status |= lr.FIXED_CUT
                continue
            fixed.append(s)
    kfs = local + fixed
    needed = sum(len(obs.get(p, [])) for p in points)
    o = lr.gather_offsets(kf_cap, point_cap, edge_cap)
    blk = np.zeros(o["out_bytes"], np.uint8)

    def put(key, a, dt):
        a = np.ascontiguousarray(a, dt).reshape(-1).view(np.uint8)
        blk[o[key]:o[key] + a.size] = a
    kf_slot = np.full(kf_cap, -1, np.int32)
    kf_slot[:len(kfs)] = kfs
    fx = np.zeros(kf_cap, np.uint8)
    fx[:len(kfs)] = [s == origin or i >= len(local) for i, s in enumerate(kfs)]
    T = np.zeros((kf_cap, 16), np.float32)
    T[:len(kfs)] = c["Tcw"][kfs]
    pidx = np.full(point_cap, -1, np.int32)
    pidx[:len(points)] = points
    xyz = np.zeros((point_cap, 3), np.float32)
    xyz[:len(points)] = c["xyz"][points] if points else 0
    start, ob, ed = np.full(point_cap + 1, -1, np.int32), np.full((edge_cap, 2), -1, np.int32), np.full((edge_cap, 3), -1, np.int32)
    n_obs = n_edges = 0
    if needed > edge_cap:
        status |= lr.EDGE_OVERFLOW
    else:
        for i, p in enumerate(points):
            start[i] = n_obs
            for s, k in obs.get(p, []):
                ob[n_obs] = (s, k)
                n_obs += 1
                if s in kfs:
                    ed[n_edges] = (i, kfs.index(s), k)
                    n_edges += 1
        start[len(points)] = n_obs
    for key, a, dt in (("kf_slot", kf_slot, np.int32), ("fixed", fx, np.uint8), ("Tcw", T, np.float32), ("point_idx", pidx, np.int32),
                       ("xyz", xyz, np.float32), ("obs_start", start, np.int32), ("obs", ob, np.int32), ("edges", ed, np.int32)):
        put(key, a, dt)
    blk[:40] = np.array([status, len(local), n_free, len(fixed), len(kfs), len(points), len(stamped), n_obs, n_edges, needed], np.int32).view(np.uint8)
    return blk


def py_apply(c):
    """the sequential erase loop on objects -> (the world behind it, dict(status, bad_point, remaining, ref)); nobs and ref_slot are
    the reference's for the points that stay good (it stops counting once a point is bad, and moves mpRefKF before it knows)"""
    w = lr.copy_world(c)
    k, p_cap, e_cap, b_cap = (int(c[x]) for x in lr.APPLY_PARAMS)
    g = lr.decode_gather(c["gather"], k, p_cap, e_cap)
    hdr = np.ascontiguousarray(c["ba"][:128]).view(np.int32)
    ba_status = int(hdr[lr.BA_FIELDS["status"] // 4])
    refused = bool(ba_status & (lr.BA_UNSORTED | lr.BA_COV_OVERFLOW | lr.BA_TOO_MANY_FREE | lr.BA_STOPPED_EARLY)) or \
        bool(g["status"] & lr.EDGE_OVERFLOW) or \
        [int(hdr[lr.BA_FIELDS[f] // 4]) for f in ("n_kf", "n_points", "n_edges")] != [g["n_kf"], g["n_points"], g["n_edges"]]
    if refused:
        return w, dict(status=lr.NOT_APPLIED, bad_point=[], remaining={}, ref={}, n_erased=0)
    n_kf, n, E = g["n_kf"], g["n_points"], g["n_edges"]
    o = lr.ba_offsets(n_kf, n, E)
    ba = np.ascontiguousarray(c["ba"])
    Tcw_out = ba[o["Tcw"]:o["Tcw"] + 64 * n_kf].view(np.float32).reshape(-1, 16)
    xyz_out = ba[o["xyz"]:o["xyz"] + 12 * n].view(np.float32).reshape(-1, 3)
    n_erase = int(hdr[lr.BA_FIELDS["n_erase"] // 4])
    erase = ba[o["erase"]:o["erase"] + 4 * n_erase].view(np.int32).tolist()
    points = g["point_idx"][:n].tolist()
    mobs = {p: [tuple(x) for x in g["obs"][g["obs_start"][i]:g["obs_start"][i + 1]].tolist()] for i, p in enumerate(points)}
    bad_point, n_erased = [], 0
    for e in erase:                                                 # :739-750
        i, b, kp = g["edges"][e].tolist()
        p, slot = points[i], int(g["kf_slot"][b])
        if not w["mp_flags"][p] & 1:
            continue                                                # mObservations is empty: both erases find nothing
        w["rows"][slot, kp] = -1                                    # EraseMapPointMatch
        mobs[p].remove((slot, kp))                                  # EraseObservation
        n_erased += 1
        w["nobs"][p] -= 1
        if w["ref_slot"][p] == slot and mobs[p]:
            w["ref_slot"][p] = mobs[p][0][0]
        if w["nobs"][p] <= 2:                                       # SetBadFlag
            w["mp_flags"][p] &= 0xFE
            for s2, k2 in mobs[p]:
                w["rows"][s2, k2] = -1
            mobs[p] = []
            bad_point.append(p)
    for b in range(g["n_local"]):                                   # :753-757
        w["Tcw"][g["kf_slot"][b]] = Tcw_out[b]
    for i, p in enumerate(points):                                  # :760-772
        w["xyz"][p] = xyz_out[i]
    good = [p for p in points if w["mp_flags"][p] & 1]
    return w, dict(status=lr.BAD_CUT if len(bad_point) > b_cap else 0, bad_point=bad_point, remaining={p: mobs[p] for p in good},
                   ref={p: int(w["ref_slot"][p]) for p in good}, n_erased=n_erased)


def run_ref(L, c, mutate=0):
    """the case through lba_ref.c on a copy of its world -> (world, result)"""
    w = lr.copy_world(c)
    if c["op"] == "gather":
        return w, lr.gather(L, w, c["ord_row"], c, mutate)
    return w, lr.apply(L, w, c["gather"], c["ba"], c, mutate)


def against_python(c, w, r):
    """what lba_ref.c gave (world w, result r) held to the Python statement"""
    if c["op"] == "gather":
        assert not lr.diff_world(w, c)
        want = py_gather(c)
        if r["block"].tobytes() != want.tobytes():
            k, p, e = int(c["kf_cap"]), int(c["point_cap"]), int(c["edge_cap"])
            a, b = lr.decode_gather(r["block"], k, p, e), lr.decode_gather(want, k, p, e)
            for f in lr.GATHER_FIELDS + ("kf_slot", "fixed", "point_idx", "obs_start", "obs", "edges", "Tcw", "xyz"):
                assert np.array_equal(a[f], b[f]), (f, a[f], b[f])
            assert False, "padding differs"
        return
    pw, pr = py_apply(c)
    assert r["status"] & ~lr.WILD == pr["status"] and (c.get("wild") or not r["status"] & lr.WILD), (r["status"], pr["status"])
    for key in ("rows", "kf_flags", "mp_flags", "xyz", "Tcw"):
        assert w[key].tobytes() == pw[key].tobytes(), key
    good = (w["mp_flags"] & 1).astype(bool)
    assert np.array_equal(w["nobs"][good], pw["nobs"][good]) and np.array_equal(w["ref_slot"][good], pw["ref_slot"][good])
    b_cap = int(c["bad_cap"])
    assert r["n_bad"] == len(pr["bad_point"]) and r["bad_point"][:r["n_bad_stored"]].tolist() == pr["bad_point"][:b_cap]
    assert r["n_bad_stored"] == min(b_cap, r["n_bad"]) and (r["bad_point"][r["n_bad_stored"]:] == -1).all()
    if pr["status"] & lr.NOT_APPLIED:
        assert not lr.diff_world(w, c) and r["n_erased"] == r["n_obs_after"] == 0 and r["obs_start"][0] == 0 and (r["obs_start"][1:] == -1).all()
        return
    g = lr.decode_gather(c["gather"], int(c["kf_cap"]), int(c["point_cap"]), int(c["edge_cap"]))
    at = 0
    for i, p in enumerate(g["point_idx"][:g["n_points"]].tolist()):
        assert r["obs_start"][i] == at, i
        rem = pr["remaining"].get(p, [])
        assert [tuple(x) for x in r["obs"][at:at + len(rem)].tolist()] == rem, (i, p)
        at += len(rem)
        if p in pr["ref"]:
            assert r["ref_slot"][i] == pr["ref"][p], (i, p)
    assert r["obs_start"][g["n_points"]] == at == r["n_obs_after"] and (r["obs"][at:] == -1).all()
    if not c.get("wild"):
        assert r["n_erased"] >= pr["n_erased"]      # the contract counts the erased observations of a point behind its SetBadFlag too


# ---- worlds -------------------------------------------------------------------------------------------------------------------------
def scene(seed, n_slots=12, stride=9, n_table=40, fill=0.6, bad_kf=(), bad_mp=(), used=None):
    """a random map: every row names distinct points at random keypoints (points from the first `used` table rows); nobs by count,
    ref_slot = one of the observers"""
    rng = np.random.RandomState(seed)
    w = lr.new_world(n_slots, stride, n_table)
    used = n_table if used is None else used
    for s in range(n_slots):
        m = min(int(round(fill * stride)), used)
        kps = rng.choice(stride, m, replace=False)
        w["rows"][s, kps] = rng.choice(used, m, replace=False)
    w["kf_flags"][list(bad_kf)] = 1
    w["mp_flags"][list(bad_mp)] = 2
    settle(w, rng)
    return w


def settle(w, rng=None):
    """nobs by a fresh count; ref_slot of every observed point an observer (the least one without rng)"""
    w["nobs"][:] = lr.count_nobs(w)
    w["ref_slot"][:] = -1
    n, stride = w["rows"].shape
    for s in range(n - 1, -1, -1):
        if w["kf_flags"][s] & 1:
            continue
        r = w["rows"][s]
        r = r[(r >= 0) & (r < len(w["nobs"]))]
        if rng is None:
            w["ref_slot"][r] = s
        else:
            take = rng.rand(len(r)) < 0.5
            w["ref_slot"][r[take | (w["ref_slot"][r] < 0)]] = s
    return w


def ord_for(w, cur, conn_cap, seed=0, extra=()):
    """an ord row for cur: the other slots in a random order (bad ones included: the gather skips them), `extra` entries put in
    front, -1 behind"""
    rng = np.random.RandomState(seed + 1000)
    others = [s for s in rng.permutation(w["rows"].shape[0]).tolist() if s != cur]
    row = (list(extra) + others)[:conn_cap]
    return np.array(row + [-1] * (conn_cap - len(row)), np.int32)


def gather_case(w, cur, ord_row, origin=-1, kf_cap=16, free_cap=8, point_cap=64, edge_cap=512):
    return dict(w, op="gather", ord_row=np.ascontiguousarray(ord_row, np.int32), cur_slot=cur, origin_slot=origin, kf_cap=kf_cap,
                free_cap=free_cap, point_cap=point_cap, edge_cap=edge_cap)


def apply_case(gc, erase_of, bad_cap=8, status=0, seed=0, wild=False, ba_counts=None, n_erase=None, block=None):
    """the application behind the gather case gc: erase_of(g) -> the erase list as edge indices (g: the decoded gather block); the
    solver's poses and positions are the gathered ones plus a perturbation; ba_counts overrides (n_kf, n, E) in the solver's header"""
    blk = py_gather(gc) if block is None else block
    k, p, e = int(gc["kf_cap"]), int(gc["point_cap"]), int(gc["edge_cap"])
    g = lr.decode_gather(blk, k, p, e)
    rng = np.random.RandomState(seed + 77)
    n_kf, n, E = min(max(g["n_kf"], 0), k), min(max(g["n_points"], 0), p), min(max(g["n_edges"], 0), e)   # a wild header: what fits
    T = g["Tcw"][:n_kf] + rng.randint(1, 9, (n_kf, 16)).astype(np.float32) / 8
    T[g["fixed"][:n_kf] != 0] = g["Tcw"][:n_kf][g["fixed"][:n_kf] != 0]
    X = g["xyz"][:n] + rng.randint(1, 9, (n, 3)).astype(np.float32) / 16
    erase = list(erase_of(g))
    ba = lr.ba_block(n_kf, n, E, T, X, erase, status=status, n_erase=n_erase)
    if ba_counts is not None:
        hdr = ba[:128].view(np.int32)
        for f, v in zip(("n_kf", "n_points", "n_edges"), ba_counts):
            hdr[lr.BA_FIELDS[f] // 4] = v
    c = dict({x: gc[x] for x in lr.WORLD}, op="apply", gather=blk, ba=ba, kf_cap=k, point_cap=p, edge_cap=e, bad_cap=bad_cap)
    if wild:
        c["wild"] = True
    return c


def edges_of_point(g, p, count=None, slots=None):
    """the edge indices of table row p in the decoded gather block: the first `count`, or those in `slots`"""
    i = g["point_idx"][:g["n_points"]].tolist().index(p)
    es = [e for e in range(g["n_edges"]) if g["edges"][e, 0] == i]
    if slots is not None:
        es = [e for e in es if int(g["kf_slot"][g["edges"][e, 1]]) in slots]
    return es if count is None else es[:count]


def _seen_world():
    """point 0 seen by 1 keyframe, 1 by 2, 2 by 3, 3 by 4, 4 by 200 (all at keypoint = point), and row 5 names point 5 twice"""
    w = lr.new_world(210, 8, 12)
    for p, cnt in ((0, 1), (1, 2), (2, 3), (3, 4), (4, 200)):
        w["rows"][:cnt, p] = p
    w["rows"][5, 5] = w["rows"][5, 7] = 5
    w["rows"][6, 6] = 5
    return settle(w)


def _points_world(n_points, extra_stride=0):
    """cur (slot 0) holds exactly n_points distinct points, two neighbours share every third"""
    stride = max(n_points, 1) + extra_stride
    w = lr.new_world(3, stride, max(n_points, 1) + 3)
    w["rows"][0, :n_points] = np.arange(n_points)[::-1]
    w["rows"][1, :n_points:3] = np.arange(n_points)[::-1][::3]
    w["rows"][2, :n_points:3] = np.arange(n_points)[::3][:len(range(0, n_points, 3))]
    return settle(w)


def named_cases():
    """name -> case.  Gather cases are named g_*, apply cases a_*."""
    C = {}
    # the shapes: slots, pitches, tables
    w = lr.new_world(1, 1, 1)
    w["rows"][0, 0] = 0
    C["g_one_slot_one_entry_one_point"] = gather_case(settle(w), 0, [-1], kf_cap=1, free_cap=1, point_cap=1, edge_cap=1)
    C["g_slots_300"] = gather_case(scene(1, 300, 7, 90, 0.5, bad_kf=(3, 250), bad_mp=(4, 9)), 17, ord_for(scene(1, 300, 7, 90, 0.5), 17, 40, 1),
                                   origin=0, kf_cap=24, free_cap=12, point_cap=32, edge_cap=1200)
    big = scene(2, 4100, 5, 50, 0.4, bad_kf=(7, 4099 - 1))
    C["g_slots_4100_beyond_the_scan_grid"] = gather_case(big, 4099, ord_for(big, 4099, 12, 2), kf_cap=8, free_cap=6, point_cap=16, edge_cap=9000)
    for stride in (1, 2, 3, 4, 5, 7, 1001):
        ws = scene(10 + stride, 6, stride, 30, 0.7 if stride < 100 else 0.02)
        C["g_pitch_%d" % stride] = gather_case(ws, 2, ord_for(ws, 2, 8, stride), kf_cap=4, free_cap=3, point_cap=24, edge_cap=160)
    wt = scene(3, 9, 40, 50000, 0.8, used=1000)
    wt["rows"][wt["rows"] >= 0] += 49000
    wt["rows"][4, 0], wt["rows"][5, 0], wt["rows"][4, 1] = 49999, 49999, 0
    C["g_table_50000"] = gather_case(settle(wt), 4, ord_for(wt, 4, 8, 3), kf_cap=6, free_cap=4, point_cap=40, edge_cap=400)
    # point lists: none, one, around a wavefront, a decision workgroup and a compaction chunk
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025):
        wp = _points_world(n, extra_stride=2)
        C["g_points_%d" % n] = gather_case(wp, 0, [1, 2, -1], kf_cap=3, free_cap=3, point_cap=max(n, 1), edge_cap=2 * n + 2)
    # who sees a point
    ws = _seen_world()
    C["g_seen_by_1_2_3_4_200_and_twice_in_a_row"] = gather_case(ws, 0, [1, 5, -1, 2], kf_cap=128, free_cap=3, point_cap=8, edge_cap=256)
    C["g_fixed_cut_at_kf_cap"] = gather_case(ws, 0, [1, 5, -1], kf_cap=40, free_cap=3, point_cap=8, edge_cap=256)
    # the ord row
    wo = scene(5, 14, 9, 40, 0.6, bad_kf=(3, 8))
    C["g_ord_bad_wild_repeated"] = gather_case(wo, 6, [3, 14, -2, 5, 5, 6, 8, 99999, 2, 5, 2, 1, -1, 4], origin=2, kf_cap=8, free_cap=8)
    C["g_ord_full_to_conn_cap"] = gather_case(wo, 6, ord_for(wo, 6, 13, 5), kf_cap=16, free_cap=16)
    C["g_ord_empty"] = gather_case(wo, 6, [-1] * 6)
    C["g_cur_is_origin"] = gather_case(wo, 6, ord_for(wo, 6, 13, 6), origin=6, kf_cap=8, free_cap=2)
    C["g_origin_behind_the_free_cut"] = gather_case(wo, 6, [1, 2, 4, 0, 5], origin=0, kf_cap=8, free_cap=3)
    C["g_cur_is_bad"] = gather_case(wo, 3, ord_for(wo, 3, 13, 7), kf_cap=4, free_cap=4)
    # the capacities, exact and one short
    base = dict(kf_cap=16, free_cap=8, point_cap=64, edge_cap=512)
    ord6 = [1, 2, 4, 5, 7, 9, 10, -1]
    full = lr.decode_gather(py_gather(gather_case(wo, 6, ord6, **base)), 16, 64, 512)
    assert full["status"] == 0 and full["n_local"] == 8
    for name, prm in (("g_free_cap_exact", dict(free_cap=8)), ("g_free_cap_plus_1", dict(free_cap=7)), ("g_kf_cap_exact", dict(kf_cap=full["n_kf"])),
                      ("g_kf_cap_plus_1", dict(kf_cap=full["n_kf"] - 1)), ("g_kf_cap_cuts_the_local_list", dict(kf_cap=5)),
                      ("g_point_cap_exact", dict(point_cap=full["n_points"])), ("g_point_cap_one_short", dict(point_cap=full["n_points"] - 1)),
                      ("g_edge_cap_exact", dict(edge_cap=full["n_obs"])), ("g_edge_cap_one_short", dict(edge_cap=full["n_obs"] - 1))):
        C[name] = gather_case(wo, 6, ord6, **dict(base, **prm))
    # ---- the application
    gc = gather_case(ws, 0, [1, 5, -1], kf_cap=128, free_cap=3, point_cap=8, edge_cap=256)
    C["a_erase_nothing"] = apply_case(gc, lambda g: [])
    C["a_3_to_2_goes_bad"] = apply_case(gc, lambda g: edges_of_point(g, 2, 1))
    C["a_4_to_3_stays"] = apply_case(gc, lambda g: edges_of_point(g, 3, 1))
    C["a_erase_the_reference_keyframe"] = apply_case(gc, lambda g: edges_of_point(g, 4, slots=(0, 1, 2)) + edges_of_point(g, 3, slots=(0,)))
    C["a_erase_every_observation"] = apply_case(gc, lambda g: sorted(edges_of_point(g, 2) + edges_of_point(g, 1) + edges_of_point(g, 0)))
    C["a_bad_cap_exceeded"] = apply_case(gc, lambda g: edges_of_point(g, 0) + edges_of_point(g, 1, 1) + edges_of_point(g, 2, 1) + edges_of_point(g, 3, 2),
                                         bad_cap=2)
    C["a_bad_cap_0"] = apply_case(gc, lambda g: edges_of_point(g, 2, 1), bad_cap=0)
    C["a_point_twice_in_a_row"] = apply_case(gc, lambda g: edges_of_point(g, 5, 1), wild=False)
    C["a_200_observations_half_erased"] = apply_case(gc, lambda g: edges_of_point(g, 4)[::2])
    C["a_stopped_midway_is_applied"] = apply_case(gc, lambda g: edges_of_point(g, 3, 1), status=lr.BA_STOPPED | 3)
    for name, st in (("unsorted", lr.BA_UNSORTED), ("cov_overflow", lr.BA_COV_OVERFLOW), ("too_many_free", lr.BA_TOO_MANY_FREE),
                     ("stopped_early", lr.BA_STOPPED_EARLY)):
        C["a_refused_" + name] = apply_case(gc, lambda g: edges_of_point(g, 2, 1), status=st)
    full = lr.decode_gather(py_gather(gc), 128, 8, 256)
    n3 = (full["n_kf"], full["n_points"], full["n_edges"])
    for j, name in enumerate(("n_kf", "n_points", "n_edges")):
        C["a_refused_%s_differs" % name] = apply_case(gc, lambda g: edges_of_point(g, 2, 1), ba_counts=[v - (i == j) for i, v in enumerate(n3)])
    short = gather_case(ws, 0, [1, 5, -1], kf_cap=128, free_cap=3, point_cap=8, edge_cap=100)
    C["a_refused_gather_overflowed"] = apply_case(short, lambda g: [])
    wr = scene(8, 20, 12, 60, 0.7, bad_kf=(4,), bad_mp=(7,))
    gr = gather_case(wr, 9, ord_for(wr, 9, 10, 8), origin=0, kf_cap=12, free_cap=6, point_cap=48, edge_cap=400)
    C["a_random_erases"] = apply_case(gr, lambda g: sorted(np.random.RandomState(5).choice(g["n_edges"], g["n_edges"] // 4, replace=False).tolist()))
    # what names nothing (lba_ref.c alone is the oracle)
    C["a_wild_erase_indices"] = apply_case(gc, lambda g: [-1, g["n_edges"], 1 << 30, edges_of_point(g, 3, 1)[0], edges_of_point(g, 3, 1)[0]], wild=True)
    C["a_wild_n_erase"] = apply_case(gc, lambda g: edges_of_point(g, 3, 1), n_erase=1 << 20, wild=True)
    for name, field, val in (("n_kf", 4, 129), ("n_points", 5, 9), ("n_obs", 7, 257), ("n_edges", 8, 250), ("n_local", 1, 0), ("n_points_negative", 5, -1)):
        blk = py_gather(gc).copy()
        blk[:64].view(np.int32)[field] = val
        hdr = blk[:64].view(np.int32)
        C["a_wild_count_" + name] = apply_case(gc, lambda g: [], wild=True, block=blk, ba_counts=(int(hdr[4]), int(hdr[5]), int(hdr[8])))
    blk = py_gather(gc).copy()
    o = lr.gather_offsets(128, 8, 256)
    blk[o["edges"]:o["edges"] + 36].view(np.int32)[:] = [9, 0, 0, 0, 200, 0, 1, 0, 77]
    blk[o["obs"] + 8 * 3:o["obs"] + 8 * 3 + 8].view(np.int32)[:] = [100000, 5]
    blk[o["point_idx"] + 4 * 5:o["point_idx"] + 4 * 5 + 4].view(np.int32)[:] = 12
    blk[o["obs_start"] + 4 * 3:o["obs_start"] + 4 * 3 + 4].view(np.int32)[:] = 9999
    C["a_wild_entries_in_the_gather_block"] = apply_case(gc, lambda g: [0, 1, 2, 5], wild=True, block=blk)
    return C


def fixture_names():
    """the named cases small enough to be kept under tests/golden (lba_<name>.npz)"""
    return [n for n, c in named_cases().items() if sum(np.asarray(v).nbytes for v in c.values() if not isinstance(v, (str, bool, int))) < 200 * 1024]


CASE_ARRAYS = lr.WORLD + ("ord_row", "gather", "ba")


def save_fixture(path, c, w, r):
    d = {k: np.asarray(v) for k, v in c.items()}
    d.update({"e_" + k: w[k] for k in lr.WORLD}, e_block=r["block"])
    np.savez_compressed(path, **d)


def load_fixture(path):
    z = np.load(path)
    c = {}
    for k in z.files:
        v = z[k]
        c[k] = v if k in CASE_ARRAYS or k.startswith("e_") else (str(v) if k == "op" else (bool(v) if k == "wild" else int(v)))
    return c


# ---- sequences: gather and apply alternating with the covisibility graph and the keyframe cull -----------------------------------
SEQ = dict(n_slots=40, stride=24, n_table=700, conn_cap=16, kf_cap=12, free_cap=5, point_cap=160, edge_cap=1600, bad_cap=12)


def sequence_keyframe(w, rng, s, next_point):
    """the row of the new keyframe at slot s: points of the last few keyframes re-observed, then new ones -> the next free table row"""
    stride = w["rows"].shape[1]
    recent = w["rows"][max(0, s - 5):s]
    known = np.unique(recent[(recent >= 0)])
    known = known[(w["mp_flags"][known] & 1) != 0]
    take = rng.permutation(known)[:min(len(known), stride * 2 // 3)]
    n_new = min(stride - len(take), 8, len(w["mp_flags"]) - next_point)
    pts = np.concatenate([take, np.arange(next_point, next_point + n_new)]).astype(np.int32)
    kps = rng.choice(stride, len(pts), replace=False)
    w["rows"][s, kps] = pts
    w["kf_flags"][s] = 0
    w["nobs"][pts] += 1
    w["ref_slot"][next_point:next_point + n_new] = s
    w["mp_flags"][next_point:next_point + n_new] = 3
    return next_point + n_new
