"""Cases of keyframe culling, and an INDEPENDENT Python statement of the reference's lines (local_mapper.cpp:979-1032,
keyframe.cpp:911-997 and :1004-1016, mappoint.cpp:122-173) that cull_ref.c is held to: keyframe and map-point objects with
mObservations dicts, children sets and mConnectedKeyFrameWeights dicts, sorted() by slot where the reference walks a set or a map
keyed by pointer, and the observation graph built from the rows.  A case is a WORLD (cull_ref.WORLD) and the parameters of ONE
call; the named cases are what the fixtures tests/golden/cull_*.npz record (tests/golden/make_golden_cull.py), each built to show
one rule of include/spfe_cull_math.h.  numpy only."""
import numpy as np

KEYS = ("rows", "kf_flags", "mp_flags", "nobs", "conn_slot", "conn_w", "conn_n", "ord_slot", "ord_w", "ord_n", "parent", "first_conn",
        "n_best_a", "n_best_b", "cur", "th_obs", "cov_ratio", "origin_slot", "bad_cap")
STATE = ("conn_slot", "conn_w", "conn_n", "ord_slot", "ord_w", "ord_n", "parent", "first_conn")


# ---- the Python statement -------------------------------------------------------------------------------------------------------
class PyPoint:
    def __init__(self, idx, bad, n_obs):
        self.idx, self.bad, self.n_obs, self.obs = idx, bad, n_obs, {}      # obs: keyframe slot -> index in its row


class PyKeyFrame:
    def __init__(self, slot, row, flag):
        self.slot, self.row, self.flag = slot, [int(p) for p in row], int(flag)
        self.conn, self.ord, self.parent, self.children = {}, [], None, set()

    @property
    def bad(self):
        return bool(self.flag & 1)


class PyWorld:
    """the objects behind a world's arrays.  A row must not hold a point twice (a keyframe observes a point through ONE index)."""

    def __init__(self, w):
        self.n_table = len(w["mp_flags"])
        n, cap = w["conn_slot"].shape
        self.cap = cap
        self.points = [PyPoint(p, not w["mp_flags"][p] & 1, int(w["nobs"][p])) for p in range(self.n_table)]
        self.other_bits = [int(f) & ~1 for f in w["mp_flags"]]
        self.kfs = [PyKeyFrame(s, w["rows"][s], w["kf_flags"][s]) for s in range(n)]
        for kf in self.kfs:
            s = kf.slot
            kf.conn = {int(w["conn_slot"][s, i]): int(w["conn_w"][s, i]) for i in range(int(w["conn_n"][s]))}
            kf.ord = [(int(w["ord_slot"][s, i]), int(w["ord_w"][s, i])) for i in range(int(w["ord_n"][s]))]
            kf.parent = int(w["parent"][s])
            if kf.bad:
                continue                                                 # SetBadFlag erased its observations
            for k, p in enumerate(kf.row):
                if 0 <= p < self.n_table and not self.points[p].bad:
                    assert kf.slot not in self.points[p].obs, "a row holds a point twice"
                    self.points[p].obs[kf.slot] = k
        for kf in self.kfs:
            if 0 <= kf.parent < n and kf.parent != kf.slot:
                self.kfs[kf.parent].children.add(kf.slot)
        self.events, self.culled, self.bad_points, self.touched, self.no_parent = [], [], [], set(), False

    def point_at(self, kf, k):
        p = kf.row[k]
        return self.points[p] if 0 <= p < self.n_table else None

    # mappoint.cpp:122-173
    def erase_observation(self, mp, kf):
        if kf.slot in mp.obs:
            mp.n_obs -= 1
            del mp.obs[kf.slot]
            if mp.n_obs <= 2:
                self.point_set_bad(mp)

    def point_set_bad(self, mp):
        mp.bad = True
        obs, mp.obs = mp.obs, {}
        for s, k in sorted(obs.items()):
            self.kfs[s].row[k] = -1                                     # EraseMapPointMatch
        self.bad_points.append(mp.idx)

    # keyframe.cpp:591-612, :1004-1016
    def update_best_covisibles(self, kf):
        pairs = sorted((w, k) for k, w in kf.conn.items())
        kf.ord = [(k, w) for w, k in reversed(pairs)]

    def erase_connection(self, kf, other):
        if other in kf.conn:
            del kf.conn[other]
            self.update_best_covisibles(kf)
            self.touched.add(kf.slot)

    def change_parent(self, kf, parent):
        kf.parent = parent
        if parent is not None and parent >= 0:
            self.kfs[parent].children.add(kf.slot)
        self.events.append((kf.slot, -1 if parent is None else parent))

    # keyframe.cpp:911-997
    def set_bad_flag(self, kf, origin_slot):
        if kf.slot == origin_slot:
            return
        if kf.flag & 2:
            kf.flag |= 4
            return
        for s in sorted(kf.conn):
            if 0 <= s < len(self.kfs) and s != kf.slot:
                self.erase_connection(self.kfs[s], kf.slot)
        for k in range(len(kf.row)):
            mp = self.point_at(kf, k)
            if mp is not None and not mp.bad:
                self.erase_observation(mp, kf)
        kf.conn, kf.ord = {}, []
        has_parent = 0 <= kf.parent < len(self.kfs)
        if not has_parent:
            self.no_parent = True                                       # a null dereference in the reference
        candidates = {kf.parent} if has_parent else set()
        children = set(kf.children)
        children = {s for s in children if self.kfs[s].parent == kf.slot}
        while children:
            go_on, best, pc, pp = False, -1, None, None
            for s in sorted(children):
                child = self.kfs[s]
                if child.bad:
                    continue
                for e, _ in child.ord:
                    for cand in sorted(candidates):
                        if e == cand:
                            w = child.conn.get(e, 0)
                            if w > best:
                                pc, pp, best, go_on = s, e, w, True
            if not go_on:
                break
            self.change_parent(self.kfs[pc], pp)
            candidates.add(pc)
            children.discard(pc)
        for s in sorted(children):
            self.change_parent(self.kfs[s], kf.parent if has_parent else -1)
        kf.children = set()
        kf.flag |= 1
        self.culled.append(kf.slot)

    # local_mapper.cpp:979-1032, with the stall rule of spfe_cull_math.h (3)
    def cull(self, cur, th_obs, cov_ratio, origin_slot):
        cov_ratio = np.float32(cov_ratio)
        kf_list = [s for s, _ in self.kfs[cur].ord if 0 <= s < len(self.kfs) and s != origin_slot and not self.kfs[s].bad]
        decided, n_pass, stalled = {}, 0, False
        while kf_list:
            n_pass += 1
            max_vit, ratio_max, keep = None, np.float32(0.0), []
            for s in kf_list:
                kf = self.kfs[s]
                n_mps = n_red = 0
                for k in range(len(kf.row)):
                    mp = self.point_at(kf, k)
                    if mp is not None and not mp.bad:
                        n_mps += 1
                        if mp.n_obs >= th_obs:
                            n_red += 1
                with np.errstate(all="ignore"):
                    ratio = np.float32(n_red) * np.float32(1.0) / np.float32(n_mps)
                decided[s] = (n_pass, n_mps, n_red)
                if ratio < cov_ratio:
                    continue
                keep.append(s)
                if ratio > ratio_max:
                    ratio_max, max_vit = ratio, s
            kf_list = keep
            if max_vit is None:
                stalled = bool(kf_list)
                break
            self.set_bad_flag(self.kfs[max_vit], origin_slot)
            kf_list.remove(max_vit)
        return decided, n_pass, stalled

    def arrays(self, w):
        """the world's arrays as the objects leave them (tables: not held here)"""
        out = {k: (None if w[k] is None else w[k].copy()) for k in w}
        n, cap = w["conn_slot"].shape
        for kf in self.kfs:
            s = kf.slot
            out["rows"][s] = kf.row
            out["kf_flags"][s] = kf.flag
            out["parent"][s] = kf.parent
            for name, fill in (("conn_slot", -1), ("conn_w", 0), ("ord_slot", -1), ("ord_w", 0)):
                out[name][s] = fill
            for j, k in enumerate(sorted(kf.conn)):
                out["conn_slot"][s, j], out["conn_w"][s, j] = k, kf.conn[k]
            for j, (k, wt) in enumerate(kf.ord):
                out["ord_slot"][s, j], out["ord_w"][s, j] = k, wt
            out["conn_n"][s], out["ord_n"][s] = len(kf.conn), len(kf.ord)
        for mp in self.points:
            out["mp_flags"][mp.idx] = self.other_bits[mp.idx] | (0 if mp.bad else 1)
            out["nobs"][mp.idx] = mp.n_obs
        return out


# ---- building worlds ------------------------------------------------------------------------------------------------------------
def set_links(w, s, conn, ord_=None):
    """conn: {slot: weight} of slot s; ord_: [(slot, weight)] or None = all of conn by (weight, slot) descending"""
    cap = w["conn_slot"].shape[1]
    for name, fill in (("conn_slot", -1), ("conn_w", 0), ("ord_slot", -1), ("ord_w", 0)):
        w[name][s] = fill
    for j, k in enumerate(sorted(conn)):
        w["conn_slot"][s, j], w["conn_w"][s, j] = k, conn[k]
    if ord_ is None:
        ord_ = [(k, wt) for wt, k in sorted(((wt, k) for k, wt in conn.items()), reverse=True)]
    for j, (k, wt) in enumerate(ord_):
        w["ord_slot"][s, j], w["ord_w"][s, j] = k, wt
    w["conn_n"][s], w["ord_n"][s] = len(conn), len(ord_)
    assert len(conn) <= cap and len(ord_) <= cap


def link(w, a, b, wt):
    """a symmetric link, both ord rows rebuilt from all of conn"""
    for x, y in ((a, b), (b, a)):
        n = int(w["conn_n"][x])
        conn = {int(w["conn_slot"][x, i]): int(w["conn_w"][x, i]) for i in range(n)}
        conn[y] = wt
        set_links(w, x, conn)


def base(n=8, stride=4, n_table=40, cap=8, listed=(1, 2, 3, 4), cur=5):
    """slots 0 .. n-1, a chain of parents s -> s - 1, slot 0 the origin; the current keyframe linked to `listed` with falling
    weights; every point good with 9 observations; rows empty"""
    import cull_ref
    w = cull_ref.new_world(n, stride, n_table, cap, 3, 2)
    w["nobs"][:] = 9
    w["first_conn"][:] = 0
    w["parent"][:] = np.arange(n) - 1
    for i, s in enumerate(listed):
        if 0 <= s < n:
            link(w, cur, s, 100 - 10 * i)
    set_links(w, cur, {s: 100 - 10 * i for i, s in enumerate(listed) if 0 <= s < n}, [(s, 100 - 10 * i) for i, s in enumerate(listed)])
    return w


def case(w, cur=5, th_obs=3, cov_ratio=0.75, origin_slot=0, bad_cap=8):
    c = {k: w[k] for k in ("rows", "kf_flags", "mp_flags", "nobs") + STATE}
    c.update(n_best_a=w["best_a"].shape[1], n_best_b=w["best_b"].shape[1], cur=cur, th_obs=th_obs, cov_ratio=np.float32(cov_ratio),
             origin_slot=origin_slot, bad_cap=bad_cap)
    return c


def named_cases():
    out = {}

    def rows4(w, s, first):
        w["rows"][s] = np.arange(first, first + 4)

    # nothing above the ratio: every listed keyframe has 2 of 4 points redundant
    w = base()
    for s in (1, 2, 3, 4):
        rows4(w, s, 4 * s)
        w["nobs"][4 * s:4 * s + 2] = 2
    out["nothing_above_ratio"] = case(w)

    # one culled: slot 2 at ratio 1, the others at 0.5; its child 3 has no link to slot 1 and is left over to it
    w = base()
    for s in (1, 2, 3, 4):
        rows4(w, s, 4 * s)
        if s != 2:
            w["nobs"][4 * s:4 * s + 2] = 2
    out["one_culled"] = case(w)

    # a chain: 1 and 2 share four points, 3 and 4 four others, nobs == th_obs == 4: each cull takes its partner below the ratio
    w = base()
    rows4(w, 1, 0), rows4(w, 2, 0), rows4(w, 3, 8), rows4(w, 4, 8)
    w["nobs"][:] = 4
    out["chain_each_cull_drops_the_next"] = case(w, th_obs=4)

    # a cull RAISES a ratio: slot 2 stands at 3 / 4 = cov_ratio; the cull of slot 1 makes its fourth point bad (3 -> 2): 3 / 3
    w = base(listed=(1, 2))
    rows4(w, 1, 0)
    w["rows"][2] = [3, 10, 11, 12]
    w["nobs"][3] = 3
    out["cull_raises_a_ratio"] = case(w, th_obs=4)

    # equal ratios: the first in list order, pass after pass
    w = base()
    for s in (1, 2, 3, 4):
        rows4(w, s, 4 * s)
    out["equal_ratios_first_in_list_order"] = case(w)

    # ratio exactly cov_ratio: kept, and culled as the only offer
    w = base(listed=(3,))
    rows4(w, 3, 0)
    w["nobs"][0] = 2
    out["ratio_exactly_cov_ratio_kept"] = case(w)

    # nobs == th_obs is redundant
    w = base(listed=(3,))
    rows4(w, 3, 0)
    w["nobs"][:4] = 5
    out["nobs_equal_th_obs_is_redundant"] = case(w, th_obs=5)

    # nobs 3 -> 2: the points go bad, and slot 6 (not listed) loses its entries; 4 -> 3 stays
    w = base(listed=(3,))
    rows4(w, 3, 0)
    w["rows"][6] = [1, 0, 30, 3]
    w["rows"][7] = [0, 1, 2, 3]
    w["kf_flags"][7] = 1                           # a bad slot's row keeps its bytes
    w["nobs"][:4] = [3, 3, 4, 3]
    w["mp_flags"][1] = 0x81                        # the other bits of a flag stay
    out["nobs_three_to_two_goes_bad"] = case(w)

    # a keyframe without a good point: NaN neither drops nor wins, the loop stalls after the cull of slot 2
    w = base(listed=(1, 2))
    rows4(w, 2, 0)
    w["rows"][1] = [-1, 39, 40, 41]
    w["mp_flags"][39] = 0
    out["stall_keyframe_without_good_points"] = case(w)

    # not-erase: chosen, deferred, nothing else changes; the next pass chooses slot 2
    w = base(listed=(1, 2))
    rows4(w, 1, 0), rows4(w, 2, 4)
    w["kf_flags"][1] = 2
    out["not_erase_deferred"] = case(w)

    # the origin, a bad slot and a wild slot in the list
    w = base(listed=(0, 1, 99, 2, -3))
    rows4(w, 0, 0), rows4(w, 1, 4), rows4(w, 2, 8)
    w["kf_flags"][1] = 1
    out["origin_bad_and_wild_in_the_list"] = case(w)

    # a row naming a point twice: counted twice in n_mps / n_red, nobs 4 - 2 = 2 goes bad
    w = base(listed=(3, 4))
    w["rows"][3] = [7, 7, 8, 9]
    w["rows"][4] = [7, 20, 21, 22]
    w["nobs"][7] = 4
    out["row_names_a_point_twice"] = case(w)

    # bad_cap on either side: three points go bad
    for name, cap in (("bad_cap_cuts_the_list", 2), ("bad_cap_exactly_enough", 3), ("bad_cap_zero", 0)):
        w = base(listed=(3,))
        rows4(w, 3, 0)
        w["nobs"][:4] = [3, 5, 3, 3]
        out[name] = case(w, bad_cap=cap)

    # asymmetric links: slot 6 holds 3 though 3 does not hold 6 (kept), 3 holds 7 though 7 does not hold 3 (nothing to remove)
    w = base(listed=(3,), cap=8)
    rows4(w, 3, 0)
    set_links(w, 6, {3: 11, 1: 4})
    set_links(w, 7, {1: 6})
    conn3 = {5: 100, 7: 9}
    set_links(w, 3, conn3)
    out["asymmetric_links"] = case(w)

    # a neighbour whose ord is a part of its conn: the removal rebuilds ord from ALL of conn, equal weights by slot descending
    w = base(listed=(3,))
    rows4(w, 3, 0)
    link(w, 3, 6, 30)
    set_links(w, 6, {3: 30, 1: 7, 2: 7, 4: 12}, [(3, 30), (4, 12)])
    out["ord_rebuilt_from_all_of_conn"] = case(w)

    # a child with a link to the parent (3 -> 1 by a step), and one without (4: left over to 1); the step's event comes first
    w = base(listed=(2,))
    rows4(w, 2, 0)
    w["parent"][[3, 4]] = 2
    link(w, 4, 6, 5)
    link(w, 3, 1, 8)
    out["child_with_and_without_link_to_the_parent"] = case(w)

    # a re-parented child becomes the next child's candidate: 4 -> 1 first, then 3 -> 4
    w = base(listed=(2,))
    rows4(w, 2, 0)
    w["parent"][[3, 4]] = 2
    link(w, 4, 1, 8)
    link(w, 3, 4, 6)
    out["reparented_child_is_the_next_candidate"] = case(w)

    # the maximum is the step's, not the child's: 3 (weight 9) before 4 (weight 5), though 4 is walked last
    w = base(listed=(2,))
    rows4(w, 2, 0)
    w["parent"][[3, 4]] = 2
    link(w, 3, 1, 9)
    link(w, 4, 1, 5)
    out["maximum_of_the_step_not_of_the_child"] = case(w)

    # parent(c0) == c1, both culled: 6 goes to 2 when 1 is culled, and on to 0 with the bad child 1 when 2 is
    w = base(listed=(1, 2))
    rows4(w, 1, 0), rows4(w, 2, 4)
    w["parent"][1], w["parent"][2], w["parent"][6], w["parent"][3] = 2, 0, 1, 7
    link(w, 6, 2, 5)
    out["parent_of_the_first_culled_is_culled_too"] = case(w)

    # a bad child is skipped by the steps although linked to the parent, and left over all the same
    w = base(listed=(2,))
    rows4(w, 2, 0)
    w["parent"][[3, 4]] = 2
    link(w, 3, 1, 9)
    link(w, 4, 1, 5)
    w["kf_flags"][3] = 1
    out["bad_child_left_over"] = case(w)

    # a child that is culled LATER in the call is alive when its parent is culled: 3 (child of 2, culled in the second pass) goes
    # to 1 by a step and takes its sibling 4, which links only to it; when 3 is culled, 6 goes to 1 and 4 on to 6
    w = base(listed=(2, 3))
    rows4(w, 2, 0), rows4(w, 3, 4)
    w["parent"][4], w["parent"][6] = 2, 3
    link(w, 6, 1, 5), link(w, 4, 6, 4), link(w, 3, 1, 8), link(w, 4, 3, 7)
    out["child_culled_later_is_alive"] = case(w)

    # more re-parenting events than slots: 1 -> 2 -> 3 -> 4 -> 0 are culled in that order and hand their children on, 2 + 3 + 4 + 6
    # events in 8 slots; the list is cut, parent[] is written in full
    w = base()
    for s in (1, 2, 3, 4):
        rows4(w, s, 4 * s)
    w["parent"][[1, 2, 3, 4]] = [2, 3, 4, 0]
    w["parent"][[6, 7]] = 1
    out["more_events_than_slots"] = case(w)

    # parent == -1: the children get -1 and the status bit
    w = base(listed=(2,))
    rows4(w, 2, 0)
    w["parent"][2] = -1
    w["parent"][[3, 4]] = 2
    out["no_parent"] = case(w)
    return out


def load_fixture(path):
    z = np.load(path)
    return {k: z[k] for k in z.files}


# ---- generated worlds ------------------------------------------------------------------------------------------------------------
def sequence_world(seed, n_slots=48, stride=24, window=34, step=5, cap=16, n_best_a=20, n_best_b=10):
    """an empty map of n_slots keyframes to come: every slot bad (no keyframe yet), the points good and unobserved.
    insert_keyframe puts the next keyframe's row in: distinct points of a sliding window, so that neighbours share many"""
    import cull_ref
    n_table = step * n_slots + window
    w = cull_ref.new_world(n_slots, stride, n_table, cap, n_best_a, n_best_b)
    w["kf_flags"][:] = 1
    return w, np.random.default_rng(seed), dict(window=window, step=step)


def insert_keyframe(w, rng, geo, s):
    """the row of keyframe s, its flag cleared, nobs kept up with single-entry writes (AddObservation); a few empty entries"""
    stride = w["rows"].shape[1]
    lo = geo["step"] * s
    pts = lo + rng.choice(geo["window"], size=stride, replace=False)
    pts = np.where(w["mp_flags"][pts] & 1, pts, -1)             # a bad point is not matched again
    pts[rng.random(stride) < 0.15] = -1
    w["rows"][s] = pts
    w["kf_flags"][s] = 0
    for p in pts[pts >= 0]:
        w["nobs"][p] += 1


def generated_world(seed, n, stride, n_table, cap, n_listed, n_best_a=20, n_best_b=10, share=0.7, bad_slots=0.05, dup=False):
    """a dense world for the GPU shapes: random rows over a table, consistent nobs, a random graph with symmetric links among the
    first min(n, 64) neighbours of each slot, parents below, and cur = n - 1 listing n_listed slots"""
    import cull_ref
    rng = np.random.default_rng(seed)
    w = cull_ref.new_world(n, stride, n_table, cap, n_best_a, n_best_b)
    if n_table:
        for s in range(n):
            k = min(stride, n_table)
            row = np.full(stride, -1, np.int64)
            row[:k] = rng.choice(n_table, size=k, replace=False) if not dup else rng.integers(0, n_table, k)
            row[rng.random(stride) > share] = -1
            w["rows"][s] = row
        w["mp_flags"][:] = (rng.random(n_table) > 0.1).astype(np.uint8) | (rng.integers(0, 2, n_table) << 3).astype(np.uint8)
    w["kf_flags"][:] = (rng.random(n) < bad_slots).astype(np.uint8)
    w["kf_flags"][n - 1] = 0
    w["nobs"][:] = 0
    for s in range(n):
        if not w["kf_flags"][s] & 1:
            r = w["rows"][s]
            np.add.at(w["nobs"], r[(r >= 0) & (r < n_table)], 1)
    w["first_conn"][:] = 0
    w["parent"][:] = [-1] + [int(rng.integers(max(0, s - 4), s)) for s in range(1, n)]
    conn = [dict() for _ in range(n)]
    deg = min(cap - 1, 6)
    for s in range(n - 1):
        for t in rng.choice(n - 1, size=min(deg, n - 1), replace=False):
            t = int(t)
            if t != s and len(conn[s]) < cap - 1 and len(conn[t]) < cap - 1:
                wt = int(rng.integers(1, 40))
                conn[s][t] = conn[t][s] = wt
    cur = n - 1
    listed = [int(x) for x in rng.permutation(n - 1)[:min(n_listed, cap, n - 1)]]
    for i, s in enumerate(listed):
        if len(conn[s]) < cap:
            conn[s][cur] = 1000 - i
        conn[cur][s] = 1000 - i
    for s in range(n):
        set_links(w, s, conn[s], [(t, 1000 - i) for i, t in enumerate(listed)] if s == cur else None)
    return w, cur
