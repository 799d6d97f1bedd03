"""The named cases of the insertion of a new keyframe's row (op "insert") and of the observation lists (op "list"), and an
independent Python statement of the reference's lines that tests/test_newkf_reference.py holds newkf_ref.c to: map-point objects
with an mObservations dict, LocalMapping::ProcessNewKeyFrame :255-272 literally, a list as sorted(mObservations.items()), and the
two documented deviations applied where the reference differs.

A case is a dict: op, the world (newkf_ref.WORLD; desc_track None without a track table) and
  insert: frame int32 [n_kp], cur_slot, rec_desc (float32 or uint16 [n_kp][256], or None)
  list:   point_idx int32 [m] or None, first_row, m, obs_cap
Shapes are the smallest at which a path of newkf.hip changes: a wavefront (64), a workgroup of the multi-workgroup kernels (256),
a chunk of the one-workgroup kernels (1024), the range a wavefront orders (256 observations), the scan's grid (4096 wavefronts)."""
import numpy as np

import newkf_ref as nr

WORLD = nr.WORLD
FIXTURE_LIMIT = 40_000       # bytes of a case's arrays: larger cases are GPU cases only, not fixtures
KMAX = 301                   # the handle of the GPU tests: SPExtractor(300, ...) keeps num_features + 1 keypoints a record


# ---- the Python statement ---------------------------------------------------------------------------------------------------------
class MapPoint:
    def __init__(self, idx, bad):
        self.idx, self.bad = idx, bad
        self.mObservations = {}          # keyframe slot -> keypoint (the reference) / keypoints in row order (deviation 2)
        self.nObs = 0
        self.desc_track = None

    def isBad(self):
        return self.bad

    def IsInKeyFrame(self, kf):
        return kf in self.mObservations

    def AddObservation(self, kf, i):
        if kf in self.mObservations:
            return
        self.mObservations[kf] = [i]
        self.nObs += 1

    def GetObservations(self):
        return [(kf, k) for kf, ks in sorted(self.mObservations.items()) for k in sorted(ks)]


def the_map(w):
    """the host's object graph for the resident arrays: a MapPoint a table row, mObservations from the rows of the good slots"""
    pts = [MapPoint(p, not (int(f) & nr.SEARCHABLE)) for p, f in enumerate(w["flags"])]
    for s in range(w["rows"].shape[0]):
        if w["kf_flags"][s] & 1:
            continue
        for k, p in enumerate(w["rows"][s].tolist()):
            if 0 <= p < len(pts):
                pts[p].mObservations.setdefault(s, []).append(k)
    return pts


def python_insert(c):
    """-> (the world after, dict(status, code, added_point, counts, n_recent_*)).  local_mapper.cpp:255-272, line for line"""
    w = nr.copy_world(c)
    n_table, cap = len(w["flags"]), len(w["recent"])
    stride, cur = w["rows"].shape[1], int(c["cur_slot"])
    frame = np.asarray(c["frame"], np.int32).tolist()
    pts = [MapPoint(p, not (int(f) & nr.SEARCHABLE)) for p, f in enumerate(w["flags"])]
    vpMapPointMatches = [pts[p] if 0 <= p < n_table else None for p in frame]           # GetMapPointMatches()
    code = [nr.NONE if p == -1 else nr.WILD for p in frame]
    mlpRecentAddedMapPoints, added, row = [], [-1] * stride, [-1] * stride
    for i in range(len(vpMapPointMatches)):                                               # :258
        pMP = vpMapPointMatches[i]
        if pMP:                                                                           # :260
            if not pMP.isBad():                                                           # :261
                if not pMP.IsInKeyFrame(cur):                                             # :262
                    pMP.AddObservation(cur, i)                                            # :263
                    pMP.desc_track = i                                                    # :266 updateDescTrack(mpCurrentKeyFrame, i)
                    code[i], added[i] = nr.ADDED, pMP.idx
                else:
                    mlpRecentAddedMapPoints.append(pMP)                                   # :268
                    pMP.mObservations[cur].append(i)                                      # deviation 2: the row entry is counted
                    pMP.nObs += 1
                    code[i] = nr.REPEATED
                row[i] = pMP.idx
            else:
                code[i] = nr.BAD_POINT                                                    # deviation 1: the keyframe drops the pointer
    n_before = min(max(int(w["recent_n"][0]), 0), cap)
    needed = n_before + len(mlpRecentAddedMapPoints)
    status = (nr.ROW_IN_USE if (w["rows"][cur] >= 0).any() else 0) | (nr.BAD_SLOT if w["kf_flags"][cur] & 1 else 0) | \
        (nr.RECENT_OVERFLOW if needed > cap else 0)
    r = dict(status=status, code=np.asarray(code, np.int32), n_recent_before=n_before, n_needed=needed,
             n_recent_after=n_before if status else needed, added_point=np.asarray([-1] * stride if status else added, np.int32))
    for name, k in (("n_none", nr.NONE), ("n_wild", nr.WILD), ("n_bad_point", nr.BAD_POINT), ("n_added", nr.ADDED), ("n_repeated", nr.REPEATED)):
        r[name] = code.count(k)
    if not status:
        w["rows"][cur] = row
        for pMP in pts:
            w["nobs"][pMP.idx] += pMP.nObs
            if pMP.desc_track is not None:
                w["flags"][pMP.idx] |= nr.OBSERVED
                if c.get("rec_desc") is not None and w["desc_track"] is not None:
                    d = np.asarray(c["rec_desc"])[pMP.desc_track]
                    w["desc_track"][pMP.idx] = d if d.dtype == np.float32 else (d.astype(np.uint32) << 16).view(np.float32)
        w["recent"][n_before:needed] = [pMP.idx for pMP in mlpRecentAddedMapPoints]
        w["recent_n"][0] = needed
    return w, r


def python_list(c):
    """-> dict(point_idx, ref_slot, ranges (a list of (slot, keypoint) lists per entry), the counts)"""
    pts = the_map(c)
    n_table, m = len(pts), int(c["m"])
    idx = (np.asarray(c["point_idx"], np.int64)[:m] if c["point_idx"] is not None else int(c["first_row"]) + np.arange(m, dtype=np.int64)).tolist()
    listed, point_idx, ref_slot, ranges = set(), [], [], []
    counts = dict(n_empty=0, n_wild=0, n_repeated=0, n_first=0)
    for p in idx:
        what = "n_empty" if p == -1 else "n_wild" if not 0 <= p < n_table else "n_repeated" if p in listed else "n_first"
        counts[what] += 1
        if what == "n_first":
            listed.add(p)
            point_idx.append(p)
            ref_slot.append(int(c["ref_slot"][p]))
            ranges.append(pts[p].GetObservations())
        else:
            point_idx.append(-1)
            ref_slot.append(-1)
            ranges.append([])
    needed = sum(len(x) for x in ranges)
    max_obs = max([len(x) for x in ranges] + [0])
    overflow = needed > int(c["obs_cap"])
    return dict(counts, point_idx=point_idx, ref_slot=ref_slot, ranges=ranges, n_obs_needed=needed, max_obs=max_obs,
                status=(nr.OVERFLOW if overflow else 0) | (nr.MANY if max_obs > nr.MAX_OBS else 0), n_obs=0 if overflow else needed)


def run_ref(L, c, mutate=0):
    """the case through newkf_ref.c on a copy of its world -> (the world after, the decoded block)"""
    w = nr.copy_world(c)
    if c["op"] == "insert":
        r = nr.insert(L, w, c["frame"], int(c["cur_slot"]), c.get("rec_desc"), mutate)
    else:
        r = nr.list_obs(L, w, c["point_idx"], int(c["first_row"]), int(c["m"]), int(c["obs_cap"]), mutate)
    return w, r


def against_python(c, w, r):
    """newkf_ref.c's world and block of the case against the Python statement's"""
    if c["op"] == "insert":
        pw, pr = python_insert(c)
        for k in nr.INSERT_FIELDS:
            assert r[k] == pr[k], (k, r[k], pr[k])
        assert r["code"].tolist() == pr["code"].tolist() and r["added_point"].tolist() == pr["added_point"].tolist()
        assert not nr.diff_world(w, pw), nr.diff_world(w, pw)
        return
    pr = python_list(c)
    m, cap = int(c["m"]), int(c["obs_cap"])
    for k in ("status", "n_first", "n_empty", "n_wild", "n_repeated", "n_obs", "n_obs_needed", "max_obs"):
        assert r[k] == pr[k], (k, r[k], pr[k])
    assert r["m"] == m and r["obs_cap"] == cap and not nr.diff_world(w, c)
    assert r["point_idx"].tolist() == pr["point_idx"] and r["ref_slot"].tolist() == pr["ref_slot"]
    if r["status"] & nr.OVERFLOW:
        assert (r["obs_start"] == 0).all() and (r["obs"] == -1).all()
        return
    for i in range(m):
        got = r["obs"][r["obs_start"][i]:r["obs_start"][i + 1]]
        assert [tuple(x) for x in got.tolist()] == pr["ranges"][i], (i, got.tolist()[:6], pr["ranges"][i][:6])
    assert r["obs_start"][m] == r["n_obs"] and (r["obs"][r["n_obs"]:] == -1).all()


# ---- worlds -----------------------------------------------------------------------------------------------------------------------
def mixed_world(seed, n_slots=6, stride=37, n_table=80, recent_cap=64, density=0.5, bad_slots=True, bad_points=True, track=False,
                empty_slot=None):
    """rows that name about `density` of their entries (a point now and then twice in a row, wild entries), some slots and points
    bad, a list partly filled, ref_slot a slot a point; empty_slot: that row empty (the new keyframe's)"""
    rng = np.random.default_rng(seed)
    w = nr.new_world(n_slots, stride, n_table, recent_cap, track)
    rows = np.where(rng.random((n_slots, stride)) < density, rng.integers(0, n_table, (n_slots, stride)), -1)
    rows[rng.random((n_slots, stride)) < 0.01] = n_table + 5
    rows[rng.random((n_slots, stride)) < 0.01] = -7
    w["rows"][...] = rows
    if bad_slots and n_slots > 2:
        w["kf_flags"][rng.random(n_slots) < 0.2] = 1
    if bad_points:
        w["flags"][rng.random(n_table) < 0.15] = nr.OBSERVED
    w["flags"][rng.random(n_table) < 0.3] |= 0x80
    if empty_slot is not None:
        w["rows"][empty_slot] = -1
        w["kf_flags"][empty_slot] = 0
    counts = np.bincount(w["rows"][(w["kf_flags"] & 1) == 0].reshape(-1).clip(-1, n_table) + 1, minlength=n_table + 2)[1:n_table + 1]
    w["nobs"][:] = counts
    n = int(rng.integers(0, recent_cap // 2 + 1))
    w["recent"][:n] = rng.integers(0, n_table, n)
    w["recent_n"][0] = n
    w["ref_slot"][:] = rng.integers(0, n_slots, n_table)
    return w


def rec_desc_for(n_kp, bf16=False, seed=5):
    rng = np.random.default_rng(seed)
    if bf16:
        return rng.integers(0, 1 << 16, (max(n_kp, 1), 256)).astype(np.uint16)
    return rng.standard_normal((max(n_kp, 1), 256)).astype(np.float32)


def insert_case(w, frame, cur_slot, rec_desc=None):
    return dict(nr.copy_world(w), op="insert", frame=np.asarray(frame, np.int32), cur_slot=int(cur_slot), rec_desc=rec_desc)


def list_case(w, point_idx, m=None, first_row=0, obs_cap=None, short=0):
    """obs_cap None: exactly what the list needs, less `short`"""
    pi = None if point_idx is None else np.asarray(point_idx, np.int32)
    c = dict(nr.copy_world(w), op="list", point_idx=pi, first_row=int(first_row), m=int(len(pi) if m is None else m), obs_cap=0)
    c["obs_cap"] = int(obs_cap) if obs_cap is not None else max(python_needed(c) - short, 0)
    return c


def python_needed(c):
    n_table = len(c["ref_slot"])
    m = int(c["m"])
    idx = np.asarray(c["point_idx"], np.int64)[:m] if c["point_idx"] is not None else int(c["first_row"]) + np.arange(m, dtype=np.int64)
    listed = np.zeros(n_table + 1, bool)
    listed[idx[(idx >= 0) & (idx < n_table)]] = True
    good = c["rows"][(c["kf_flags"] & 1) == 0].reshape(-1)
    good = good[(good >= 0) & (good < n_table)]
    return int(listed[good].sum())


def frame_for(w, n_kp, seed, repeat=0.1, wild=0.03, none=0.3):
    rng = np.random.default_rng(seed)
    n_table = len(w["flags"])
    f = rng.integers(0, n_table, n_kp)
    if n_kp > 1:
        again = rng.random(n_kp) < repeat
        f[again] = f[rng.integers(0, n_kp, int(again.sum()))]
    f[rng.random(n_kp) < none] = -1
    f[rng.random(n_kp) < wild] = rng.choice([n_table, n_table + 9, -2, -(1 << 31), (1 << 31) - 1])
    return f.astype(np.int32)


def observers_world(counts, n_slots=300, stride=5, twice=(), bad=()):
    """point j is named by the first counts[j] slots (at keypoint j % stride ... one point a column block), the points of `twice`
    twice in slot 1, the slots of `bad` bad"""
    n_table = len(counts) + 3
    w = nr.new_world(n_slots, stride * len(counts), n_table, 4)
    for j, n in enumerate(counts):
        w["rows"][:n, stride * j + (j % stride)] = j
    for j in twice:
        w["rows"][1, stride * j + ((j + 1) % stride)] = j
    w["kf_flags"][list(bad)] = 1
    w["ref_slot"][:] = np.arange(n_table) % n_slots
    return w


# ---- the named cases --------------------------------------------------------------------------------------------------------------
def named_cases():
    C = {}
    # (I) the keypoint counts around a wavefront, a workgroup and the one workgroup's chunk; the row longer than the frame
    for n_kp in (0, 1, 63, 64, 65, 255, 256, 257, 1001, 1023, 1024, 1025):
        stride = max(n_kp, 1) + (0 if n_kp in (1, 64, 1001) else 3)
        w = mixed_world(100 + n_kp, n_slots=4, stride=stride, n_table=max(2, n_kp // 2 + 3), recent_cap=n_kp + 40, empty_slot=2, track=n_kp <= 257)
        rd = rec_desc_for(n_kp) if n_kp <= 257 else None
        C["insert_n_kp_%d" % n_kp] = insert_case(w, frame_for(w, n_kp, n_kp), 2, rd)
    w = mixed_world(7, n_slots=3, stride=12, n_table=10, recent_cap=8, empty_slot=1, bad_points=False, track=True)
    w["flags"][[4, 5]] = [nr.OBSERVED, 0]
    w["recent"][:3], w["recent_n"][0] = [9, 9, 1], 3
    C["insert_every_code"] = insert_case(w, [3, -1, 4, 10, 3, -5, 7, 3, 5, 7], 1, rec_desc_for(10))     # 3 three times, 7 twice
    C["insert_every_code_bf16"] = insert_case(w, [3, -1, 4, 10, 3, -5, 7, 3, 5, 7], 1, rec_desc_for(10, bf16=True))
    C["insert_no_record"] = insert_case(w, [3, -1, 4, 10, 3, -5, 7, 3, 5, 7], 1, None)
    w2 = nr.copy_world(w)
    w2["desc_track"] = None
    C["insert_no_track_table"] = insert_case(w2, [3, -1, 4, 10, 3, -5, 7, 3, 5, 7], 1, rec_desc_for(10))
    w = mixed_world(8, n_slots=2, stride=1100, n_table=40, recent_cap=700, empty_slot=0, bad_points=False)
    w["recent"][:], w["recent_n"][0] = -1, 100
    f = np.full(1100, -1, np.int32)
    f[[10, 1030, 1090]] = 36                                            # a point three times across the chunk boundary
    f[100:700] = np.arange(600) % 30                                   # 30 points twenty times each: 570 REPEATED
    C["insert_repeats_across_chunks"] = insert_case(w, f, 0)
    # refusals, each alone and all together; the list's capacity reached and one short; the count held to its range
    base = mixed_world(9, n_slots=5, stride=9, n_table=12, recent_cap=6, empty_slot=3, bad_points=False, bad_slots=False)
    base["recent"][:], base["recent_n"][0] = [1, 2, 3, 4, -1, -1], 4
    fr = [0, 5, 0, -1, 5, 7, 11]                                       # two REPEATED
    C["insert_recent_cap_reached"] = insert_case(base, fr, 3)
    C["insert_recent_cap_one_short"] = insert_case(base, fr + [7], 3)
    w = nr.copy_world(base)
    w["rows"][3, 8] = 0
    C["insert_row_in_use"] = insert_case(w, fr, 3)
    w["kf_flags"][3] = 1
    C["insert_all_refusals"] = insert_case(w, fr + [7], 3)
    w = nr.copy_world(base)
    w["kf_flags"][3] = 0x81
    C["insert_bad_slot"] = insert_case(w, fr, 3)
    w = nr.copy_world(base)
    w["rows"][3, :] = [-1, -7, -1, -(1 << 31), -1, -1, -2, -1, -1]      # negative entries are not "in use"
    w["recent_n"][0] = 99
    C["insert_count_beyond_cap"] = insert_case(w, [2, 3], 3)
    w["recent_n"][0] = -4
    C["insert_count_negative"] = insert_case(w, fr, 3)
    w = mixed_world(10, n_slots=1, stride=1, n_table=1, recent_cap=1, bad_slots=False, bad_points=False, empty_slot=0, track=True)
    w["recent_n"][0] = 0
    C["insert_1x1_table_1"] = insert_case(w, [0], 0, rec_desc_for(1))
    w = mixed_world(11, n_slots=300, stride=101, n_table=50_000, recent_cap=300, density=0.2, empty_slot=299)
    C["insert_table_50000_slots_300"] = insert_case(w, frame_for(w, 101, 3, repeat=0.2), 299)
    # (O) list lengths around a wavefront and the one workgroup's chunk, with -1, wild and repeated entries
    for m in (0, 1, 63, 64, 65, 1023, 1024, 1025):
        big = m > 100
        w = mixed_world(200 + m, n_slots=7, stride=37 if big else 11, n_table=max(3, m // 2 + 2), density=0.6)
        C["list_m_%d" % m] = list_case(w, frame_for(w, m, 50 + m, repeat=0.15, none=0.1))
    w = mixed_world(12, n_slots=6, stride=37, n_table=90)
    C["list_no_index_array"] = list_case(w, None, m=40, first_row=11)
    C["list_no_index_array_past_the_table"] = list_case(w, None, m=30, first_row=75)          # rows 90 .. 104 are wild
    C["list_no_index_array_first_row_max"] = list_case(w, None, m=5, first_row=(1 << 31) - 2)
    C["list_whole_row"] = list_case(w, w["rows"][4].copy())
    wb = mixed_world(13, n_slots=9, stride=20, n_table=30)
    wb["kf_flags"][0] = 1
    C["list_whole_row_of_a_bad_slot"] = list_case(wb, wb["rows"][0].copy())
    C["list_all_empty_wild_repeated"] = list_case(w, [-1, 90, 5, 5, -2, 5, -1, 1 << 30])
    C["list_capacity_exact"] = list_case(w, np.arange(0, 90, 3))
    C["list_capacity_one_short"] = list_case(w, np.arange(0, 90, 3), short=1)
    C["list_capacity_0"] = list_case(w, np.arange(0, 90, 3), obs_cap=0)
    C["list_capacity_large"] = list_case(w, np.arange(0, 90, 3), obs_cap=python_needed(list_case(w, np.arange(0, 90, 3))) + 77)
    # points seen by 0 .. 300 keyframes (a wavefront orders up to 256, the workgroup beyond), twice in one row, bad observers
    counts = [0, 1, 2, 64, 65, 200, 256, 257, 300]
    ow = observers_world(counts, twice=(2, 5))
    C["list_observers_0_to_300"] = list_case(ow, [8, 0, 7, 1, 6, 2, 5, 3, 4, 9, 10])
    C["list_observers_one_short"] = list_case(ow, [8, 0, 7, 1, 6, 2, 5, 3, 4], short=1)
    C["list_observers_in_bad_slots"] = list_case(observers_world(counts, twice=(2, 5, 8), bad=(0, 1, 63, 199, 299)), [8, 0, 7, 1, 6, 2, 5, 3, 4])
    C["list_observers_256_alone"] = list_case(observers_world([256]), [0])
    C["list_observers_257_alone"] = list_case(observers_world([257]), [0])
    # rows: pitches 1 .. 1001, 1 .. 300 slots, more rows than the scan has wavefronts, a table of 1 and of 50,000
    for n_slots, stride in ((1, 1), (2, 3), (7, 101), (9, 1001), (300, 5)):
        w = mixed_world(300 + stride, n_slots=n_slots, stride=stride, n_table=60, density=0.7)
        C["list_rows_%dx%d" % (n_slots, stride)] = list_case(w, frame_for(w, 50, stride, none=0.05))
    w = mixed_world(14, n_slots=4100, stride=3, n_table=500, density=0.5)
    C["list_rows_4100x3"] = list_case(w, np.arange(0, 500, 7))
    w = mixed_world(15, n_slots=1, stride=4, n_table=1, bad_slots=False)
    C["list_table_1"] = list_case(w, [0, 0, 1, -1])
    w = mixed_world(16, n_slots=40, stride=257, n_table=50_000, density=0.9)
    C["list_table_50000"] = list_case(w, np.r_[np.arange(49_990, 50_003), w["rows"][3, :100]])
    return C


def case_bytes(c):
    return sum(np.asarray(v).nbytes for v in c.values() if v is not None and not isinstance(v, str))


def fixture_names():
    C = named_cases()
    return sorted(k for k, c in C.items() if case_bytes(c) <= FIXTURE_LIMIT)


def load_fixture(path):
    z = np.load(path)
    c = {k: z[k] for k in z.files}
    c["op"] = str(c["op"])
    for k in ("desc_track", "rec_desc", "point_idx"):
        if k in c and c[k].dtype == np.bool_ and c[k].size == 1:      # how the maker stores None
            c[k] = None
    return c
