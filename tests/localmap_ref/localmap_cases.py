"""Cases of the tracker's local map: the keyframe rows, flags, best covisibles, parents, the map-point flags and the frame's holders
as the arguments of localmap_ref.update and of the library's entry points; the named cases the fixtures tests/golden/localmap_*.npz
record (tests/golden/make_golden_localmap.py), each built to show one rule of include/spfe_localmap_math.h, and the generated cases
of the GPU tests.  numpy only."""
import numpy as np

KEYS = ("kf_mp_of_kp", "kf_flags", "best_cov", "parent", "mp_flags", "mp_of_kp", "max_keyframes", "point_cap")
SEARCHABLE = 1


class Case:
    """n_slots keyframes of kp_stride entries over a table of n_table points, all SEARCHABLE; every row starts empty (-1), no
    keyframe is bad, has a parent or a best covisible, and the frame holds nothing."""

    def __init__(self, n_slots, kp_stride, n_table, n_kp, n_best=20, max_keyframes=80, point_cap=None):
        self.rows = np.full((n_slots, kp_stride), -1, np.int32)
        self.kf_flags = np.zeros(n_slots, np.uint8)
        self.best_cov = np.full((n_slots, n_best), -1, np.int32)
        self.parent = np.full(n_slots, -1, np.int32)
        self.mp_flags = np.full(n_table, SEARCHABLE, np.uint8)
        self.mp_of_kp = np.full(n_kp, -1, np.int32)
        self.max_keyframes = max_keyframes
        self.point_cap = max(n_kp, 1) if point_cap is None else point_cap

    def row(self, s, points, at=0):
        self.rows[s, at:at + len(points)] = points
        return self

    def hold(self, points, at=0):
        self.mp_of_kp[at:at + len(points)] = points
        return self

    def bad_kf(self, *slots):
        self.kf_flags[list(slots)] |= 1
        return self

    def bad_mp(self, *points):
        self.mp_flags[list(points)] &= 0xFE
        return self

    def neigh(self, s, lst):
        self.best_cov[s, :] = -1
        self.best_cov[s, :len(lst)] = lst
        return self

    def parents(self, pairs):
        for c, p in pairs.items():
            self.parent[c] = p
        return self

    def arrays(self):
        return dict(kf_mp_of_kp=self.rows, kf_flags=self.kf_flags, best_cov=self.best_cov, parent=self.parent, mp_flags=self.mp_flags,
                    mp_of_kp=self.mp_of_kp, max_keyframes=self.max_keyframes, point_cap=self.point_cap)


def named_cases():
    """name -> case dict.  Slots and points are small numbers so that the expected lists can be read off the construction."""
    c = {}
    # nobody holds anything: NO_VOTES, an empty list
    c["no_holder"] = Case(4, 5, 9, 3).row(0, [0, 1]).row(1, [1, 2])
    # every held point is bad: holds nothing, NO_VOTES; the rows' other points never appear either
    c["every_held_point_bad"] = Case(3, 4, 8, 3).row(0, [0, 1, 2]).row(1, [2, 3]).hold([0, 1, 2]).bad_mp(0, 1, 2)
    # point 1 held by two keypoints: votes 2 a keyframe that has it
    c["point_held_twice"] = Case(3, 5, 8, 4, point_cap=8).row(0, [1, 4]).row(1, [2, 5]).row(2, [1, 2, 6]).hold([1, 2, 1])
    # equal greatest votes: the first slot is the reference keyframe
    c["equal_votes"] = Case(3, 4, 8, 2, point_cap=8).row(0, [0]).row(1, [0, 1]).row(2, [1, 0]).hold([0, 1])
    # holders and row entries outside the table
    c["out_of_range"] = (Case(3, 5, 6, 5, point_cap=8).row(0, [0, 6, -3, 1]).row(1, [2**31 - 1, 1, -2**31]).row(2, [5, 5])
                         .hold([0, 6, -2, 2**31 - 1, 1]))
    # a bad keyframe with votes: counted, not in V
    c["bad_keyframe_voted"] = Case(3, 4, 8, 2, point_cap=8).row(0, [0, 1, 2]).row(1, [0, 3]).row(2, [1]).hold([0, 1]).bad_kf(0)
    # best_cov: bad, marked, -1, wild, then a good one; the entry behind the pushed one is not read
    c["best_cov_skips"] = (Case(8, 4, 8, 2, n_best=7, point_cap=8).row(0, [0]).row(1, [1]).row(2, [2]).row(3, [3]).row(4, [4])
                           .hold([0, 1]).bad_kf(2).neigh(0, [2, 1, -1, 99, 3, 4, -7]).neigh(1, [0, 3, 4]))
    # two children of one keyframe: the lower slot, once; the other at the next visit of nobody
    c["two_children"] = Case(6, 3, 8, 1, point_cap=8).row(1, [0]).row(3, [3]).row(4, [4]).hold([0]).parents({3: 1, 4: 1, 5: 1}).bad_kf(3)
    # the parent of V[0] is V[1], marked: the walk goes on; V[1]'s parent is not marked and ends it before V[2]'s turn
    c["parent_marked_goes_on"] = (Case(7, 3, 8, 3, point_cap=8).row(0, [0]).row(1, [1]).row(2, [2]).row(5, [5]).row(6, [6])
                                  .hold([0, 1, 2]).parents({0: 1, 1: 5, 2: 6}).neigh(2, [4]))
    # a bad parent is pushed all the same
    c["bad_parent_pushed"] = Case(4, 3, 8, 1, point_cap=8).row(0, [0]).row(3, [3]).hold([0]).parents({0: 3}).bad_kf(3)
    # a wild parent sets the status bit and is not followed
    c["wild_parent"] = Case(3, 3, 8, 2, point_cap=8).row(0, [0]).row(1, [1]).hold([0, 1]).parents({0: 77, 1: -5})
    # max_keyframes 3: |V| = 3 does not stop the walk (3 > 3 is false), the fourth does
    c["max_keyframes_3"] = (Case(8, 3, 8, 3, max_keyframes=3, point_cap=8).row(0, [0]).row(1, [1]).row(2, [2]).row(5, [5]).row(6, [6])
                            .hold([0, 1, 2]).neigh(0, [5]).neigh(1, [6]).neigh(2, [7]))
    # the walk is over V as it stood: 1 is pushed by 0, but 1's own neighbour 2 is not
    c["walk_over_v_only"] = Case(4, 3, 8, 1, point_cap=8).row(0, [0]).row(1, [1]).row(2, [2]).hold([0]).neigh(0, [1]).neigh(1, [2])
    # point_cap below the uncut count
    c["truncated"] = (Case(3, 6, 16, 2, point_cap=5).row(0, [9, 0, 8, 7]).row(1, [6, 1, 5, 4, 3]).hold([0, 1]))
    # the rows list a held point in front of the others: the held points still come first, in keypoint order
    c["held_first"] = Case(2, 6, 16, 3, point_cap=12).row(0, [9, 2, 8, 0]).row(1, [7, 1, 9]).hold([2, 0, 1])
    # a stride of 1, a single slot, a single point
    c["one_by_one"] = Case(1, 1, 1, 1).row(0, [0]).hold([0])
    c["no_keypoints"] = Case(2, 4, 3, 0, point_cap=4).row(0, [0, 1])
    return {k: v.arrays() for k, v in c.items()}


def generated(seed, n_slots, kp_stride, n_table, n_kp, n_best=20, max_keyframes=80, point_cap=None, p_hold=0.6, chain=False,
              vote_all=False):
    """A random map: keyframe s sees a window of the table around its place, so that neighbours share points; about one keyframe in
    ten and one point in ten are bad; a few entries are outside the table, a few best_cov entries wild.  chain: every parent is the
    slot before (all in V when everything is voted, so that the walk goes on).  vote_all: the frame holds points of every window."""
    rng = np.random.default_rng(seed)
    c = Case(n_slots, kp_stride, n_table, n_kp, n_best, max_keyframes, point_cap)
    if n_table:
        c.mp_flags[rng.random(n_table) < 0.1] = 0
        c.mp_flags[rng.random(n_table) < 0.05] |= 2   # another flag bit changes nothing
    win = max(1, min(n_table, 4 * kp_stride))
    for s in range(n_slots):
        k_s = int(rng.integers(0, kp_stride + 1))
        if n_table and k_s:
            lo = int(s * max(n_table - win, 0) / max(n_slots - 1, 1))
            pts = lo + rng.integers(0, win, k_s)
            pts[rng.random(k_s) < 0.4] = -1
            wild = rng.random(k_s) < 0.02
            pts[wild] = rng.choice([n_table, n_table + 5, -2, 2**31 - 1, -2**31], int(wild.sum()))
            c.rows[s, :k_s] = pts
    c.kf_flags[rng.random(n_slots) < 0.1] = 1
    for s in range(n_slots):
        m = int(rng.integers(0, n_best + 1))
        lst = np.clip(s + rng.integers(-6, 7, m), 0, n_slots - 1)
        lst[rng.random(m) < 0.1] = -1
        lst[rng.random(m) < 0.02] = n_slots + 3
        c.best_cov[s, :m] = lst
        if s:
            c.parent[s] = s - 1 if chain else (int(rng.integers(0, s)) if rng.random() < 0.9 else -1)
    if n_kp and n_table:
        centre = int(rng.integers(0, n_table))
        span = n_table if vote_all else max(1, min(n_table, 2 * win))
        pts = (centre + rng.integers(0, span, n_kp)) % n_table
        # four holders in five hold a point that some keyframe sees (of all keyframes, or of about 40 neighbours)
        s0 = 0 if vote_all else int(rng.integers(0, max(1, n_slots - 40)))
        seen = np.unique(c.rows[s0:n_slots if vote_all else s0 + 40])
        seen = seen[(seen >= 0) & (seen < n_table)]
        if len(seen):
            pick = rng.random(n_kp) < 0.8
            pts[pick] = rng.choice(seen, int(pick.sum()))
        pts[rng.random(n_kp) > p_hold] = -1
        wild = rng.random(n_kp) < 0.02
        pts[wild] = rng.choice([n_table, -9, 2**31 - 1], int(wild.sum()))
        c.mp_of_kp[:] = pts
    return c.arrays()
