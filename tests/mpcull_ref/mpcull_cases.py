"""Cases of map-point culling and of its resident state, and an INDEPENDENT Python statement of the reference's lines
(local_mapper.cpp:281-310 and :770-787, mappoint.cpp:37-53 and :191-203, tracker.cpp:576-588 and :772-807) that mpcull_ref.c is held
to: map-point objects in a dict, keyframe rows as lists, the recent list as a Python list walked with erase, numpy.float32 division.
A case is an operation ("cull", "admit" or "stat"), a WORLD (mpcull_ref.WORLD) and the parameters of ONE call; the named cases are
what the GPU tests run, and the small ones are what the fixtures tests/golden/mpcull_*.npz record
(tests/golden/make_golden_mpcull.py), each built to show one rule of include/spfe_mpcull_math.h.  numpy only."""
import numpy as np

import mpcull_ref as mr

WORLD = mr.WORLD
PARAMS = dict(cull=("cur_kf_id", "th_obs", "found_ratio", "bad_cap"),
              admit=("kmax", "tri", "n_neigh", "neigh_slot", "cur_slot", "cur_kf_id"),
              stat=("entry", "after", "point_idx", "in_view", "outlier"))
FIXTURE_LIMIT = 40_000       # bytes of a case's arrays: larger cases are GPU cases only, not fixtures
KMAX = 101                   # the handle of the GPU tests: SPExtractor(100, ...) keeps num_features + 1 keypoints a record


# ---- the Python statement -------------------------------------------------------------------------------------------------------
class PyPoint:
    def __init__(self, flag, nobs, found, visible, first_kf, xyz):
        self.bad, self.other_bits = not flag & 1, flag & ~1
        self.nobs, self.found, self.visible, self.first_kf, self.xyz = nobs, found, visible, first_kf, xyz


class PyWorld:
    """the objects behind a world's arrays"""

    def __init__(self, w):
        self.n_table = len(w["flags"])
        self.points = {p: PyPoint(int(w["flags"][p]), int(w["nobs"][p]), int(w["found"][p]), int(w["visible"][p]), int(w["first_kf"][p]),
                                  w["xyz"][p].copy()) for p in range(self.n_table)}
        self.rows = [[int(p) for p in row] for row in w["rows"]]
        self.kf_bad = [bool(f & 1) for f in w["kf_flags"]]
        self.recent_cap = len(w["recent"])
        n = min(max(int(w["recent_n"][0]), 0), self.recent_cap)
        self.recent = [int(p) for p in w["recent"][:n]]
        self.behind = [int(p) for p in w["recent"][n:]]        # what the array holds behind the count
        self.bad_points = []

    # mappoint.cpp:157-173 with KeyFrame::EraseMapPointMatch
    def set_bad_flag(self, p):
        self.points[p].bad = True
        for s, row in enumerate(self.rows):
            if self.kf_bad[s]:
                continue
            for k, q in enumerate(row):
                if q == p:
                    row[k] = -1
        self.bad_points.append(p)

    # local_mapper.cpp:281-310
    def cull(self, cur_kf_id, th_obs, found_ratio):
        codes, lit, n_before = [], 0, len(self.recent)
        named = list(self.recent)
        while lit < len(self.recent):
            p = self.recent[lit]
            mp = self.points.get(p)
            if mp is None:
                codes.append(mr.WILD)
                del self.recent[lit]
                continue
            with np.errstate(all="ignore"):
                ratio = np.float32(mp.found) / np.float32(mp.visible)
            if mp.bad:
                codes.append(mr.ERASED_BAD)
                del self.recent[lit]
            elif ratio < np.float32(found_ratio):
                self.set_bad_flag(p)
                codes.append(mr.CULLED_RATIO)
                del self.recent[lit]
            elif cur_kf_id - mp.first_kf >= 2 and mp.nobs <= th_obs:
                self.set_bad_flag(p)
                codes.append(mr.CULLED_OBS)
                del self.recent[lit]
            elif cur_kf_id - mp.first_kf >= 3:
                codes.append(mr.RETIRED)
                del self.recent[lit]
            else:
                codes.append(mr.KEPT)
                lit += 1
        self.behind = [-1] * (n_before - len(self.recent)) + self.behind
        return named, codes

    # local_mapper.cpp:770-787, mappoint.cpp:37-50; the test of the contract's (A2) first
    def admit(self, kmax, tri, n_neigh, neigh_slot, cur_slot, cur_kf_id):
        o = mr.tri_offsets(kmax)
        blocks, status, total, seen = [], 0, 0, []
        for j in range(n_neigh):
            blk = tri[j * o["out_bytes"]:(j + 1) * o["out_bytes"]]
            i32 = blk[:64].view(np.int32)
            if i32[7] != 0:
                blocks.append(None)
                continue
            cnt, base, slot = int(i32[1]), int(i32[8]), int(neigh_slot[j])
            ok_cnt = 0 <= cnt <= kmax
            if not ok_cnt or not 0 <= slot < len(self.rows) or slot == cur_slot or slot in seen or base < 0 or base + cnt > self.n_table:
                status |= mr.BAD_RANGE
            seen.append(slot)
            total += cnt if ok_cnt else 0
            blocks.append((cnt, base, slot, blk))
        needed = len(self.recent) + total
        if needed > self.recent_cap:
            status |= mr.RECENT_OVERFLOW
        stride = len(self.rows[0])
        if not status & mr.BAD_RANGE:
            for b in blocks:
                if b is not None:
                    cnt, _, _, blk = b
                    k = np.concatenate([blk[o["new_k1"]:o["new_k1"] + 4 * cnt].view(np.int32), blk[o["new_k2"]:o["new_k2"] + 4 * cnt].view(np.int32)])
                    if ((k < 0) | (k >= stride)).any():
                        status |= mr.BAD_RANGE
        if status:
            return dict(status=status, n_admitted=0, n_displaced=0, n_needed=needed, admitted=[0] * n_neigh)
        displaced, admitted = 0, []
        for b in blocks:
            if b is None:
                admitted.append(0)
                continue
            cnt, base, slot, blk = b
            k1, k2 = blk[o["new_k1"]:o["new_k1"] + 4 * cnt].view(np.int32), blk[o["new_k2"]:o["new_k2"] + 4 * cnt].view(np.int32)
            xyz = blk[o["new_xyz"]:o["new_xyz"] + 12 * cnt].view(np.float32).reshape(cnt, 3)
            for t in range(cnt):
                p = base + t
                for s, k in ((cur_slot, int(k1[t])), (slot, int(k2[t]))):      # AddMapPoint, unconditional
                    displaced += self.rows[s][k] != -1
                    self.rows[s][k] = p
                mp = PyPoint(mr.SEARCHABLE | mr.OBSERVED, 2, 1, 1, cur_kf_id, xyz[t].copy())   # two AddObservation
                self.points[p] = mp
                self.recent.append(p)
                self.behind = self.behind[1:]
            admitted.append(cnt)
        return dict(status=mr.DISPLACED if displaced else 0, n_admitted=total, n_displaced=displaced, n_needed=needed, admitted=admitted)

    # tracker.cpp:772-807, :576-588
    def stat(self, entry, after, point_idx, in_view, outlier):
        held = view = found = 0
        for r in entry:
            mp = self.points.get(int(r))
            if mp is not None and not mp.bad:
                mp.visible += 1
                held += 1
        for r, v in zip(point_idx, in_view):
            mp = self.points.get(int(r))
            if v and mp is not None:
                mp.visible += 1
                view += 1
        for r, o in zip(after, outlier):
            mp = self.points.get(int(r))
            if mp is not None and not o:
                mp.found += 1
                found += 1
        return dict(n_visible_held=held, n_visible_view=view, n_found=found)

    def arrays(self, like):
        w = mr.copy_world(like)
        for p, mp in self.points.items():
            w["flags"][p] = (0 if mp.bad else 1) | mp.other_bits
            w["nobs"][p], w["found"][p], w["visible"][p], w["first_kf"][p] = mp.nobs, mp.found, mp.visible, mp.first_kf
            w["xyz"][p] = mp.xyz
        w["rows"][...] = np.asarray(self.rows, np.int32).reshape(w["rows"].shape)
        w["recent"][:] = self.recent + self.behind
        w["recent_n"][0] = len(self.recent)
        return w


def run_python(c):
    """the case through the Python statement -> (the world after, what the statement returned)"""
    pw = PyWorld(c)
    if c["op"] == "cull":
        named, codes = pw.cull(int(c["cur_kf_id"]), int(c["th_obs"]), np.float32(c["found_ratio"]))
        res = dict(named=named, codes=codes, bad_points=pw.bad_points)
    elif c["op"] == "admit":
        res = pw.admit(int(c["kmax"]), c["tri"], int(c["n_neigh"]), c["neigh_slot"], int(c["cur_slot"]), int(c["cur_kf_id"]))
    else:
        res = pw.stat(c["entry"], c["after"], c["point_idx"], c["in_view"], c["outlier"])
    return pw.arrays(c), res


def run_ref(L, c, mutate=0):
    """the case through mpcull_ref.c on a copy -> (the world after, the result)"""
    w = mr.copy_world(c)
    if c["op"] == "cull":
        r = mr.cull(L, w, int(c["cur_kf_id"]), int(c["th_obs"]), float(np.float32(c["found_ratio"])), int(c["bad_cap"]), mutate)
    elif c["op"] == "admit":
        r = mr.admit(L, w, c["tri"], int(c["kmax"]), int(c["n_neigh"]), c["neigh_slot"], int(c["cur_slot"]), int(c["cur_kf_id"]), mutate)
    else:
        r = mr.stat(L, w, c["entry"], c["after"], c["point_idx"], c["in_view"], c["outlier"], mutate)
    return w, r


def against_python(c, w, r):
    """the world mpcull_ref.c left (w, result r) against the Python statement on the case"""
    want, res = run_python(c)
    for k in WORLD:
        assert w[k].tobytes() == want[k].tobytes(), (k, np.argwhere(w[k] != want[k])[:6].tolist())
    if c["op"] == "cull":
        n = len(res["named"])
        assert r["n_listed"] == n and r["entry_point"][:n].tolist() == res["named"] and r["entry_code"][:n].tolist() == res["codes"]
        assert (r["entry_point"][n:] == -1).all() and (r["entry_code"][n:] == -1).all()
        bc = int(c["bad_cap"])
        assert r["n_bad"] == len(res["bad_points"]) and r["bad_point"][:r["n_bad_stored"]].tolist() == res["bad_points"][:bc]
        assert (r["bad_point"][r["n_bad_stored"]:] == -1).all() and r["n_bad_stored"] == min(bc, r["n_bad"])
        for code, key in ((mr.KEPT, "n_kept"), (mr.CULLED_RATIO, "n_culled_ratio"), (mr.CULLED_OBS, "n_culled_obs"), (mr.RETIRED, "n_retired"),
                          (mr.ERASED_BAD, "n_erased_bad"), (mr.WILD, "n_wild")):
            assert r[key] == res["codes"].count(code), key
        assert r["status"] == (mr.BAD_CUT if r["n_bad"] > bc else 0) | (mr.WILD_ENTRY if r["n_wild"] else 0)
    elif c["op"] == "admit":
        for k in ("status", "n_admitted", "n_displaced", "n_needed"):
            assert r[k] == res[k], (k, r[k], res[k])
        nn = int(c["n_neigh"])
        assert r["admitted"][:nn].tolist() == res["admitted"] and (r["admitted"][nn:] == 0).all()
        assert r["n_recent_after"] == r["n_recent_before"] + r["n_admitted"] == int(w["recent_n"][0])
    else:
        for k in mr.STAT_FIELDS:
            assert r[k] == res[k], (k, r[k], res[k])


# ---- worlds ---------------------------------------------------------------------------------------------------------------------
CUR = 50            # the current keyframe's id in the cull cases
# a point's class -> (found, visible, age, nobs) at th_obs 2, found_ratio 0.25
CLASSES = dict(kept=(3, 4, 1, 2), kept_old=(9, 10, 2, 3), ratio=(1, 5, 0, 9), obs=(4, 4, 2, 2), obs_old=(4, 4, 7, 1), retired=(4, 5, 3, 3),
               retired_old=(8, 8, 30, 5))


def set_point(w, p, cls=None, found=None, visible=None, first_kf=None, nobs=None, flag=3):
    f, v, age, n = CLASSES[cls] if cls else (found, visible, CUR - first_kf, nobs)
    w["flags"][p], w["found"][p], w["visible"][p], w["first_kf"][p], w["nobs"][p] = flag, f, v, CUR - age, n
    w["xyz"][p] = (p, -p, 0.5 * p)


def set_list(w, points):
    w["recent"][:] = -1
    w["recent"][:len(points)] = points
    w["recent_n"][0] = len(points)


def cull_case(w, cur_kf_id=CUR, th_obs=2, found_ratio=0.25, bad_cap=8):
    c = {k: w[k] for k in WORLD}
    c.update(op="cull", cur_kf_id=cur_kf_id, th_obs=th_obs, found_ratio=np.float32(found_ratio), bad_cap=bad_cap)
    return c


def admit_case(w, blocks, neigh_slot, cur_slot, cur_kf_id=CUR, kmax=KMAX):
    c = {k: w[k] for k in WORLD}
    c.update(op="admit", kmax=kmax, tri=mr.tri_blocks(kmax, blocks), n_neigh=len(blocks), neigh_slot=np.asarray(neigh_slot, np.int32),
             cur_slot=cur_slot, cur_kf_id=cur_kf_id)
    return c


def stat_case(w, entry, after, point_idx, in_view, outlier):
    c = {k: w[k] for k in WORLD}
    c.update(op="stat", entry=np.asarray(entry, np.int32), after=np.asarray(after, np.int32), point_idx=np.asarray(point_idx, np.int32),
             in_view=np.asarray(in_view, np.uint8), outlier=np.asarray(outlier, np.uint8))
    return c


def mixed_world(seed, n_list, n_slots=6, stride=37, extra_cap=3, wild=True, dup=True, bad_slots=True):
    """n_list entries over a table of n_list + 8 points of every class (some bad at entry), a few wild entries and duplicates, the
    rows filled with points of the table (a point up to a few times in a row), some slots bad"""
    rng = np.random.default_rng(seed)
    n_table = n_list + 8
    w = mr.new_world(n_slots, stride, n_table, max(1, n_list + extra_cap))
    names = sorted(CLASSES)
    for p in range(n_table):
        set_point(w, p, names[rng.integers(len(names))], flag=(3 if rng.random() > 0.1 else 2) | (0x80 if rng.random() < 0.1 else 0))
    pts = rng.permutation(n_table)[:n_list].astype(np.int32)
    if dup and n_list >= 4:
        k = max(1, n_list // 16)
        pts[rng.integers(n_list, size=k)] = pts[rng.integers(n_list, size=k)]
    if wild and n_list >= 8:
        pts[rng.integers(n_list, size=2)] = [-7, n_table]
    set_list(w, pts)
    w["rows"][...] = np.where(rng.random((n_slots, stride)) < 0.7, rng.integers(0, n_table, (n_slots, stride)), -1)
    if bad_slots and n_slots > 2:
        w["kf_flags"][rng.integers(n_slots, size=max(1, n_slots // 8))] = 1
    return w


def named_cases():
    out = {}
    # -- the list's length: both sides of a wavefront, of a decision workgroup, of a compaction chunk, several chunks
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 5000):
        out["cull_list_%d" % n] = cull_case(mixed_world(100 + n, n), bad_cap=max(4, n // 3))
    # -- duplicates: inside one chunk and on either side of a chunk boundary, culled and kept
    w = mixed_world(7, 2100, dup=False, wild=False)
    for i, (a, b, cls) in enumerate(((10, 20, "ratio"), (1000, 1030, "obs"), (5, 2050, "ratio"), (1023, 1024, "obs"), (30, 40, "kept"),
                                     (1020, 1100, "kept_old"), (100, 2099, "retired"), (63, 64, "ratio"))):
        p = int(w["recent"][a])
        set_point(w, p, cls)
        w["recent"][b] = p
        w["rows"][i % 6, 3 + i] = p
    w["recent"][[50, 51, 52]] = w["recent"][50]              # three times
    set_point(w, int(w["recent"][50]), "obs")
    out["cull_duplicates"] = cull_case(w, bad_cap=2100)
    w = mr.new_world(2, 4, 6, 8)
    for p, cls in enumerate(("ratio", "kept", "obs", "retired")):
        set_point(w, p, cls)
    set_list(w, [0, 1, 0, 1, 2, 2, 3, 3])
    w["rows"][0] = [0, 0, 2, 1]
    out["cull_duplicates_small"] = cull_case(w)
    # -- the ratio's threshold
    w = mr.new_world(1, 8, 8, 8)
    for p, (f, v) in enumerate(((1, 4), (249, 1000), (0, 0), (1, 0), (5, 3), (1 << 24, (1 << 26) + 1), (0, 1), (250, 1000))):
        set_point(w, p, found=f, visible=v, first_kf=CUR, nobs=0)
        w["rows"][0, p] = p
    set_list(w, list(range(8)))
    out["cull_ratio_threshold"] = cull_case(w)
    # -- age and observations: cur - first_kf of 1, 2, 3 and first_kf -1, nobs at th_obs and th_obs + 1
    w = mr.new_world(2, 8, 8, 9)
    for i, (fk, nobs) in enumerate(((CUR - 1, 2), (CUR - 1, 3), (CUR - 2, 2), (CUR - 2, 3), (CUR - 3, 2), (CUR - 3, 3), (-1, 2), (-1, 3))):
        set_point(w, i, found=4, visible=4, first_kf=fk, nobs=nobs)
        w["rows"][i % 2, i] = i
    set_list(w, list(range(8)))
    out["cull_age_and_observations"] = cull_case(w)
    out["cull_th_obs_zero"] = cull_case(mr.copy_world(w), th_obs=0)
    out["cull_first_kf_extremes"] = cull_case(mr.copy_world(w), cur_kf_id=2147483647)
    out["cull_first_kf_extremes"]["first_kf"][:4] = [-2147483648, 2147483647, 2147483646, 2147483645]
    # -- lists and rows: bad_cap 0 and cut, every code in one list, wild entries
    w = mr.new_world(3, 5, 12, 16)
    for p, cls in enumerate(("kept", "ratio", "obs", "retired", "kept_old", "ratio", "obs_old", "retired_old")):
        set_point(w, p, cls)
    set_point(w, 8, "kept", flag=2)                          # bad at entry
    set_point(w, 9, "ratio", flag=0x83)                      # the other bits stay
    set_list(w, [0, 1, 99, 2, 3, 8, -1, 4, 5, 12, 6, 7, 9, 1])
    w["rows"][0] = [1, 1, 2, 0, 9]                           # a culled point twice in a row
    w["rows"][1] = [5, 7, 3, 4, 8]
    w["rows"][2] = [1, 2, 5, 0, 9]
    w["kf_flags"][2] = 1                                     # a bad slot's row keeps its bytes
    out["cull_every_code"] = cull_case(w, bad_cap=16)       # point 6 is culled and in no row
    out["cull_bad_cap_0"] = cull_case(mr.copy_world(w), bad_cap=0)
    out["cull_bad_cap_cut"] = cull_case(mr.copy_world(w), bad_cap=3)
    w = mr.copy_world(w)
    w["recent_n"][0] = 99                                    # a count beyond the capacity is held to it
    out["cull_count_beyond_cap"] = cull_case(w)
    w = mr.copy_world(w)
    w["recent_n"][0] = -4
    out["cull_count_negative"] = cull_case(w)
    for n_slots, stride in ((1, 1), (2, 3), (3, 4), (5, 5), (7, 101), (65, 33), (300, 1001), (9, 1001)):
        w = mixed_world(n_slots * 1000 + stride, 200, n_slots=n_slots, stride=stride)
        out["cull_rows_%dx%d" % (n_slots, stride)] = cull_case(w, bad_cap=64)
    w = mixed_world(5, 300, n_slots=4, stride=50)
    for p in range(len(w["flags"])):
        set_point(w, p, "kept")
    out["cull_nothing_culled"] = cull_case(w)               # the row scan leaves at once

    # -- admission
    def admit_world(n_slots=8, stride=KMAX + 4, n_table=400, recent_cap=300, listed=5):
        w = mixed_world(11, listed, n_slots=n_slots, stride=stride, wild=False, dup=False, bad_slots=False)
        big = mr.new_world(n_slots, stride, n_table, recent_cap)
        for k in mr.STATE[:5] + ("xyz",):
            big[k][:len(w[k])] = w[k]
        big["rows"][...] = -1
        set_list(big, w["recent"][:listed])
        return big
    ks = lambda n, step=1, first=0: [(first + step * t) % KMAX for t in range(n)]   # noqa: E731
    out["admit_one_neighbour"] = admit_case(admit_world(), [dict(point_base=20, k1=ks(7, 3), k2=ks(7, 5, 2))], [3], 6)
    blocks, at = [], 20
    for j in range(32):
        n = (0, 1, 3, 5)[j % 4]
        blocks.append(dict(point_base=at, k1=ks(n, 1, 3 * j), k2=ks(n, 7, j)))
        at += n
    out["admit_32_neighbours"] = admit_case(admit_world(n_slots=40), blocks, list(range(1, 33)), 0)
    out["admit_n_new_0"] = admit_case(admit_world(), [dict(point_base=20)], [3], 6)
    out["admit_n_new_1"] = admit_case(admit_world(), [dict(point_base=399, k1=[KMAX + 3], k2=[0])], [7], 0)   # the last row, the last entry
    out["admit_n_new_65_and_kmax"] = admit_case(admit_world(stride=201, n_table=600),
                                                [dict(point_base=30, k1=list(range(65)), k2=ks(65, 3)),
                                                 dict(point_base=95, k1=list(range(65, 65 + KMAX)), k2=ks(KMAX, 7))], [2, 5], 1)
    out["admit_refused_and_skipped_blocks"] = admit_case(admit_world(), [dict(status=1), dict(point_base=20, k1=[1, 2], k2=[5, 6]),
                                                                        dict(point_base=22, skipped=1), dict(status=1),
                                                                        dict(point_base=22, k1=[3], k2=[9])], [99, 2, 3, 2, 4], 6)
    out["admit_all_refused"] = admit_case(admit_world(), [dict(status=1), dict(status=1)], [1, 2], 0)
    out["admit_recent_cap_reached"] = admit_case(admit_world(recent_cap=12), [dict(point_base=20, k1=ks(4), k2=ks(4)), dict(point_base=24, k1=ks(3, 1, 4), k2=ks(3))], [1, 2], 0)
    out["admit_recent_cap_one_short"] = admit_case(admit_world(recent_cap=11), [dict(point_base=20, k1=ks(4), k2=ks(4)), dict(point_base=24, k1=ks(3, 1, 4), k2=ks(3))], [1, 2], 0)
    out["admit_id_at_n_table"] = admit_case(admit_world(), [dict(point_base=20, k1=ks(4), k2=ks(4)), dict(point_base=397, k1=ks(4, 1, 4), k2=ks(4))], [1, 2], 0)
    out["admit_id_negative"] = admit_case(admit_world(), [dict(point_base=-1, k1=ks(4), k2=ks(4))], [1], 0)
    out["admit_keypoint_out_of_range"] = admit_case(admit_world(), [dict(point_base=20, k1=ks(4), k2=ks(4)), dict(point_base=24, k1=[5, KMAX + 4], k2=[1, 2])], [1, 2], 0)
    out["admit_keypoint_negative"] = admit_case(admit_world(), [dict(point_base=20, k1=[5], k2=[-1])], [1], 0)
    out["admit_neighbour_slot_out_of_range"] = admit_case(admit_world(), [dict(point_base=20, k1=[5], k2=[1])], [8], 0)
    out["admit_neighbour_is_current"] = admit_case(admit_world(), [dict(point_base=20, k1=[5], k2=[1])], [4], 4)
    out["admit_neighbour_twice"] = admit_case(admit_world(), [dict(point_base=20, k1=[5], k2=[1]), dict(point_base=21, k1=[6], k2=[2])], [3, 3], 4)
    out["admit_count_beyond_kmax"] = admit_case(admit_world(), [dict(point_base=20, k1=[5], k2=[1], n_new=KMAX + 1)], [3], 4)
    out["admit_count_negative"] = admit_case(admit_world(), [dict(point_base=20, k1=[5], k2=[1], n_new=-2)], [3], 4)
    w = admit_world()
    w["rows"][6, 3], w["rows"][3, 2], w["rows"][3, 7] = 2, 399, -9      # holders in the way: a good point, another, a wild value
    out["admit_displaced_holder"] = admit_case(w, [dict(point_base=20, k1=ks(7, 3), k2=ks(7, 5, 2))], [3], 6)

    # -- statistics
    def stat_world(n_table=700):
        w = mr.new_world(1, 1, n_table, 4)
        rng = np.random.default_rng(n_table)
        for p in range(n_table):
            set_point(w, p, "kept", flag=3 if rng.random() > 0.15 else 2)
        return w, rng

    def stat_random(n_kp, point_cap, n_listed, n_table=700):
        w, rng = stat_world(n_table)
        entry = np.where(rng.random(n_kp) < 0.5, rng.integers(-2, n_table + 2, n_kp), -1)
        after = np.where(rng.random(n_kp) < 0.8, entry, rng.integers(-1, n_table, n_kp))
        pi = np.full(point_cap, -1)
        pi[:n_listed] = rng.integers(0, n_table, n_listed)
        iv = (rng.random(point_cap) < 0.5).astype(np.uint8)           # also behind n_listed: never followed
        if n_listed >= 3:
            pi[1], iv[1] = n_table + 5, 1                             # out of range: never followed
        return stat_case(w, entry, after, pi, iv, (rng.random(n_kp) < 0.2).astype(np.uint8))
    for n_kp in (0, 1, 65, 1001):
        out["stat_n_kp_%d" % n_kp] = stat_random(n_kp, max(1, n_kp) + 200, max(1, n_kp) + 77)
    out["stat_point_cap_1"] = stat_random(0, 1, 1)
    out["stat_point_cap_8192"] = stat_random(300, 8192, 3000, n_table=2000)
    w, _ = stat_world(12)
    w["flags"][:] = 3
    w["flags"][[4, 5]] = 2                                            # holders that went bad
    out["stat_small"] = stat_case(w, entry=[3, 3, 4, -1, 12, 7, 3], after=[3, 3, 5, 8, -1, 7, 9], point_idx=[1, 3, -1, 4, -1, -1],
                                  in_view=[1, 1, 1, 0, 0, 1], outlier=[0, 1, 0, 0, 0, 0, 0])
    return out


def case_bytes(c):
    return sum(np.asarray(v).nbytes for v in c.values())


def fixture_names():
    return sorted(k for k, c in named_cases().items() if case_bytes(c) <= FIXTURE_LIMIT)


def load_fixture(path):
    z = np.load(path)
    c = {k: z[k] for k in z.files}
    c["op"] = str(c["op"])
    return c


# ---- sequences ------------------------------------------------------------------------------------------------------------------
SEQ = dict(n_slots=48, stride=60, n_table=3000, recent_cap=400, first_id=100, kmax=KMAX, frames=3, point_cap=256)


def sequence_world(seed, n_slots=SEQ["n_slots"]):
    w = mr.new_world(n_slots, SEQ["stride"], SEQ["n_table"], SEQ["recent_cap"])
    w["kf_flags"][:] = 1                                               # no keyframe yet
    return w, np.random.default_rng(seed), dict(next_point=0)


def sequence_keyframe(w, rng, geo, s):
    """the host's share of ProcessNewKeyFrame for the keyframe at slot s: its row takes some good points of the last keyframes (an
    AddObservation each: single-entry writes), before the cull"""
    w["kf_flags"][s] = 0
    good = np.flatnonzero((w["flags"] & 1) == 1)
    if len(good):
        take = rng.choice(good, size=min(len(good), 20), replace=False)
        ks = rng.choice(SEQ["stride"] // 2, size=len(take), replace=False)    # the lower half: the upper is the creation's
        w["rows"][s, ks] = take
        w["nobs"][take] += 1
    n = int(w["recent_n"][0])
    if n and rng.random() < 0.5:                                       # another stage's SetBadFlag on a listed point (the fuse walk)
        p = int(w["recent"][rng.integers(n)])
        w["flags"][p] &= 0xFE
        w["rows"][(w["rows"] == p) & (w["kf_flags"][:, None] & 1 == 0)] = -1


def sequence_admission(w, rng, geo, s, kmax=SEQ["kmax"]):
    """-> the arguments of the admission behind the keyframe at slot s: up to 4 earlier keyframes as neighbours, free entries of the
    rows' upper halves (no holder displaced), one block refused now and then"""
    neigh = [t for t in range(max(0, s - 6), s) if not w["kf_flags"][t] & 1]
    neigh = list(rng.permutation(neigh)[:4])
    if not neigh:                                                      # the first keyframe: one refused block
        return dict(tri=mr.tri_blocks(kmax, [dict(status=1)]), n_neigh=1, neigh_slot=np.asarray([(s + 1) % len(w["kf_flags"])], np.int32),
                    cur_slot=s, cur_kf_id=SEQ["first_id"] + s)
    half = SEQ["stride"] // 2
    free1 = [k for k in range(half, SEQ["stride"]) if w["rows"][s, k] == -1]
    blocks = []
    for j, t in enumerate(neigh):
        if rng.random() < 0.15:
            blocks.append(dict(status=1))
            continue
        free2 = [k for k in range(half, SEQ["stride"]) if w["rows"][t, k] == -1]
        n = int(min(rng.integers(0, 7), len(free1), len(free2)))
        k1, free1 = free1[:n], free1[n:]
        blocks.append(dict(point_base=geo["next_point"], k1=k1, k2=list(rng.permutation(free2)[:n])))
        geo["next_point"] += n
    return dict(tri=mr.tri_blocks(kmax, blocks), n_neigh=len(blocks), neigh_slot=np.asarray(neigh, np.int32), cur_slot=s,
                cur_kf_id=SEQ["first_id"] + s)


def sequence_frame(w, rng):
    """-> the arguments of the statistics of one tracked frame: holders among the recent and older points (some twice, some bad),
    a list with a -1 tail, in_view also behind it, outliers"""
    nt, cap = len(w["flags"]), SEQ["point_cap"]
    known = np.flatnonzero(w["first_kf"] >= 0)
    n_kp = int(rng.integers(20, 80))
    if not len(known):
        known = np.asarray([0])
    entry = np.where(rng.random(n_kp) < 0.6, rng.choice(known, n_kp), -1)
    n_list = int(min(cap - 5, len(known)))
    pi = np.full(cap, -1)
    pi[:n_list] = rng.choice(known, n_list, replace=False)
    iv = (rng.random(cap) < 0.7).astype(np.uint8)
    after = entry.copy()
    hit = rng.random(n_kp) < 0.25
    after[hit] = rng.choice(pi[:max(1, n_list)], int(hit.sum()))
    after[rng.random(n_kp) < 0.05] = nt + 3
    # some points are seen and seldom found: the ratio culls them
    return dict(entry=entry.astype(np.int32), after=after.astype(np.int32), point_idx=pi.astype(np.int32), in_view=iv,
                outlier=(rng.random(n_kp) < 0.45).astype(np.uint8))
