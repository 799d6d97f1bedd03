"""Cases of the map-point refresh: a small world of keyframes (poses, flags, descriptor rows of bf16-representable values, so
that f32 and bf16 records see the same numbers) and listed points given by their observations, as the arguments of
mp_ref.refresh and of the library's entry points; the named cases the fixtures tests/golden/mp_*.npz record
(tests/golden/make_golden_mappoint.py).  numpy only."""
import glob
import os

import numpy as np

import mp_ref

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KEYS = ("kf_flags", "kf_K", "kf_status", "Tcw", "obs_start", "obs", "ref_slot", "xyz", "flags", "mode", "level_scale", "top_scale")
OUTPUTS = ("best_obs", "n_good", "code")


def bf16_values(x):
    return mp_ref.widen_bf16(mp_ref.to_bf16(np.asarray(x, np.float32)))


def pose(rng):
    """a camera a few units from the origin, looking about at it: f32 [16]"""
    w = rng.normal(size=3) * 0.3
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = rng.normal(size=3) * 0.5 + (0, 0, 4)
    return T.astype(np.float32).reshape(16)


class Case:
    """n_kf keyframes of K rows each; bad: slots whose keyframe isBad(); null: slots whose record pointer is null"""

    def __init__(self, seed, n_kf=4, K=24, bad=(), null=(), status=None, mode=3, level_scale=1.0, top_scale=1.0):
        self.rng = np.random.default_rng(seed)
        self.n_kf, self.K = n_kf, K
        self.kf_desc = bf16_values(self.rng.normal(size=(n_kf, K, 256)) / 16.0)
        self.Tcw = np.stack([pose(self.rng) for _ in range(n_kf)])
        self.kf_flags = np.zeros(n_kf, np.uint8)
        self.kf_flags[list(bad)] = 1
        self.kf_K = np.full(n_kf, K, np.int32)
        self.kf_K[list(null)] = -1
        self.kf_status = np.zeros(n_kf, np.int32) if status is None else np.asarray(status, np.int32)
        self.mode, self.level_scale, self.top_scale = mode, level_scale, top_scale
        self.points = []
        self.next_kp = np.zeros(n_kf, np.int64)
        self.point_idx = None
        self.n_table = None

    def good_slots(self):
        return [k for k in range(self.n_kf) if not self.kf_flags[k] & 1 and self.kf_K[k] >= 0]

    def point(self, obs, ref=None, xyz=None, flags=1):
        """a listed point with the given (slot, keypoint) observations, as they stand"""
        obs = np.asarray(obs, np.int32).reshape(-1, 2)
        ref = (int(obs[0, 0]) if len(obs) else 0) if ref is None else ref
        xyz = self.rng.normal(size=3) * 0.7 if xyz is None else xyz
        self.points.append((obs, ref, np.asarray(xyz, np.float32), flags))
        return len(self.points) - 1

    def fresh(self, slot):
        kp = int(self.next_kp[slot] % self.K)
        self.next_kp[slot] += 1
        return kp

    def point_n(self, N, rows=None, spread=0.25, bad_obs=0, **kw):
        """a point with N observations in good keyframes (round robin, fresh keypoints while there are any) and bad_obs in bad
        ones, interleaved; rows: the N good rows (default: a base row plus noise)"""
        good, badk = self.good_slots(), [k for k in range(self.n_kf) if self.kf_flags[k] & 1]
        if rows is None:
            base = self.rng.normal(size=256) / 16.0
            rows = base + spread * self.rng.normal(size=(N, 256)) / 16.0
        rows = bf16_values(rows)
        obs = []
        for o in range(N):
            slot = good[o % len(good)]
            kp = self.fresh(slot)
            self.kf_desc[slot, kp] = rows[o]
            obs.append((slot, kp))
        for o in range(bad_obs):
            slot = badk[o % len(badk)]
            obs.insert(min(len(obs), 1 + 2 * o), (slot, self.fresh(slot) if self.kf_K[slot] >= 0 else 0))
        return self.point(obs, **kw)

    def point_reusing(self, N, **kw):
        """N observations of rows that are already there (any slot that has a record, any keypoint, repeats allowed)"""
        slots = [k for k in range(self.n_kf) if self.kf_K[k] >= 0]
        obs = [(slots[int(self.rng.integers(len(slots)))], int(self.rng.integers(self.K))) for _ in range(N)]
        return self.point(obs, **kw)

    def arrays(self):
        m = len(self.points)
        start = np.zeros(m + 1, np.int32)
        for i, p in enumerate(self.points):
            start[i + 1] = start[i] + len(p[0])
        obs = np.concatenate([p[0] for p in self.points] + [np.zeros((0, 2), np.int32)]).astype(np.int32)
        n_table = m if self.n_table is None else self.n_table
        rows = np.arange(m) if self.point_idx is None else np.asarray(self.point_idx)
        xyz = bf16_values(self.rng.normal(size=(n_table, 3)))
        flags = np.ones(n_table, np.uint8)
        for i, p in enumerate(self.points):
            if 0 <= rows[i] < n_table:
                xyz[rows[i]] = p[2]
                flags[rows[i]] = p[3]
        return dict(kf_flags=self.kf_flags, kf_K=self.kf_K, kf_status=self.kf_status, Tcw=self.Tcw, kf_desc=self.kf_desc,
                    point_idx=None if self.point_idx is None else np.asarray(self.point_idx, np.int32), obs_start=start, obs=obs,
                    ref_slot=np.array([p[1] for p in self.points], np.int32), xyz=xyz, flags=flags, mode=self.mode,
                    level_scale=np.float32(self.level_scale), top_scale=np.float32(self.top_scale))


def subcase(c, sel):
    """the case of the listed points sel alone, on the same table"""
    sel = list(sel)
    obs = [c["obs"][c["obs_start"][i]:c["obs_start"][i + 1]] for i in sel]
    start = np.concatenate([[0], np.cumsum([len(o) for o in obs])]).astype(np.int32)
    pi = np.asarray(sel, np.int32) if c.get("point_idx") is None else c["point_idx"][sel]
    return dict(c, obs_start=start, obs=np.concatenate(obs + [np.zeros((0, 2), np.int32)]).astype(np.int32), ref_slot=c["ref_slot"][sel],
                point_idx=pi)


def host_inputs(L, c):
    """what the host-array form takes for case c (no INVALID observation in it, point_idx None): the observations gathered"""
    assert c.get("point_idx") is None
    Ow = mp_ref.camera_centres(L, c["Tcw"])
    slot, kp = c["obs"][:, 0], c["obs"][:, 1]
    good = ((c["kf_flags"][slot] & 1) == 0).astype(np.uint8)
    desc = np.where(good[:, None].astype(bool), c["kf_desc"][slot, np.clip(kp, 0, c["kf_desc"].shape[1] - 1)], np.float32(0))
    return dict(obs_start=c["obs_start"], obs_desc=np.ascontiguousarray(desc, np.float32), obs_good=good, obs_Ow=Ow[slot],
                ref_Ow=Ow[c["ref_slot"]], xyz=c["xyz"], flags=c["flags"])


# ---- the named cases of the fixtures ------------------------------------------------------------------------------------------
def case_counts():
    c = Case(1)
    for N in (1, 2, 3, 4, 5, 8, 6, 4, 7, 4):
        c.point_n(N)
    return c


def case_ties():
    c = Case(2)
    r = c.rng.normal(size=(6, 256)) / 16.0
    c.point_n(2, rows=r[[0, 0]])                       # duplicate rows: the first wins
    c.point_n(5, rows=r[[1, 1, 1, 1, 1]])              # all rows identical
    c.point_n(4, rows=r[[2, 3, 3, 2]])                 # two pairs: every median is 0, row 0 stays
    e = np.zeros((5, 256))
    e[0, 0], e[1, 0], e[2, 1], e[3, 1], e[4, 2] = 3, -3, 4, -4, 10       # rows 0 .. 3 all have the median 5: row 0 stays
    c.point_n(5, rows=e)
    c.point_n(3, rows=e[[4, 0, 1]])                    # rows 1 and 2 tie at the median 6, row 0 has more: row 1
    return c


def case_nan():
    c = Case(3)
    r = c.rng.normal(size=(6, 256)) / 16.0
    r[2, 17] = np.nan
    c.point_n(5, rows=r[:5])                           # a NaN row: never wins, ranks last inside the other rows
    c.point_n(3, rows=r[[2, 0, 1]])                    # ... as row 0
    c.point_n(4, rows=np.full((4, 256), np.nan))       # all rows NaN: row 0
    c.point_n(1, rows=np.full((1, 256), np.nan))
    i = np.zeros((3, 256))
    i[0, 0], i[1, 0], i[2, 1] = 3e38, -3e38, 3e38      # every distance overflows f32: a median of +inf never wins either
    c.point_n(3, rows=i)
    return c


def case_codes():
    c = Case(4, n_kf=5, bad=(3, 4), null=(4,))
    c.point_n(3, flags=0)                              # SKIP_BAD
    c.point([])                                        # NO_OBS
    c.point([(0, 1), (5, 0)])                          # INVALID
    c.point([(3, 2), (4, 0)], ref=3)                   # NO_GOOD_KF (one bad keyframe has no record)
    c.point_reusing(257)                               # TOO_MANY, if all good ...
    c.points[-1] = (np.array([(k % 3, k % 24) for k in range(257)], np.int32), 0, c.points[-1][2], 1)
    c.point_n(4)                                       # REFRESHED
    c.point_n(3, bad_obs=2)                            # bad keyframes skipped in (a), counted in (b)
    return c


def case_invalid():
    c = Case(5, n_kf=4, bad=(2,), null=(2, 3))
    for obs, ref in (([(0, 1), (4, 0)], 0), ([(-1, 0), (1, 1)], 1), ([(0, 24)], 0), ([(1, -1)], 1), ([(0, 2), (3, 0)], 0),
                     ([(0, 3), (1, 3)], 4), ([(0, 3), (1, 3)], -1)):
        c.point(obs, ref=ref)
    c.point([(0, 5), (2, -7), (1, 5)], ref=2)          # a bad keyframe without a record: its keypoint is not tested
    c.point_n(3)
    c.point_idx = [0, 1, 2, 3, 4, 5, 6, 7, 11]         # ... and a row outside the table
    c.n_table = 10
    return c


def case_scales():
    c = Case(6, level_scale=1.2, top_scale=2.5, status=(0, 1, 0, 0))
    for N in (2, 3, 6):
        c.point_n(N)
    return c


def case_mode_desc():
    c = case_codes()
    c.mode = mp_ref.DESC
    return c


def case_mode_nd():
    c = case_codes()
    c.mode = mp_ref.NORMAL_DEPTH
    return c


def case_permuted():
    c = Case(7)
    for N in (3, 5, 2, 4, 6):
        c.point_n(N)
    c.point([(0, 1), (1, 1)])                          # listed twice, under the same row
    c.points.append(c.points[-1])
    c.point_idx = [6, 2, 0, 5, 3, 1, 1]
    c.n_table = 8
    return c


def case_wide():
    c = Case(8, n_kf=6, K=20)
    for N in (17, 40, 20, 3, 65):
        c.point_n(N, spread=1.0)
    return c


CASES = dict(counts=case_counts, ties=case_ties, nan=case_nan, codes=case_codes, invalid=case_invalid, scales=case_scales,
             mode_desc=case_mode_desc, mode_nd=case_mode_nd, permuted=case_permuted, wide=case_wide)
CONSTRUCTED_TIES = {"ties", "nan"}
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "mp_*.npz")))
NAMES = [os.path.basename(p)[3:-4] for p in FIXTURES]


def load(name):
    """fixture -> (case dict, expected dict)"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "mp_%s.npz" % name))
    c = {k: g[k] for k in KEYS}
    c["mode"] = int(c["mode"])
    c["kf_desc"] = mp_ref.widen_bf16(g["kf_desc_bf16"])
    c["point_idx"] = g["point_idx"] if "point_idx" in g.files else None
    return c, {k[2:]: g[k] for k in g.files if k.startswith("e_")}


def differences(want, r):
    """the names of the outputs of a reference run that differ from the fixture's expectation (floats by their bits)"""
    return [k for k in want if np.ascontiguousarray(r[k]).tobytes() != np.ascontiguousarray(want[k]).tobytes()]
