"""Cases of the loop detection: a table of global descriptors whose scores against the query are CONSTRUCTED (row = target x query
+ noise orthogonal to the query, so that the dot is the target to about 1e-7), the flags, the database membership, the best
covisibles and the two lists, as the arguments of loopdet_ref.detect and of the library's entry points; the named cases the
fixtures tests/golden/loopdet_*.npz record (tests/golden/make_golden_loopdet.py); the generated cases of the GPU tests.  No case
is ever dropped: check_margins asserts that no score lies within MARGIN of min_score and no acc within MARGIN of
min_score_to_retain, unless the case declares exact ties (identical rows, whose scores are identical whatever forms the sum).
numpy only."""
import numpy as np

NEIGH = 10
MARGIN = 1e-5
KEYS = ("gdesc", "kf_flags", "in_db", "best_cov", "cur_slot", "connected", "covisible", "min_score_init", "min_score_floor",
        "retain_ratio", "ties")
LOW = 0.05    # the score of a slot nobody set: far below every threshold used here


class Case:
    """n slots of dim floats; the query is the last slot unless cur says otherwise.  Every other slot starts as a db member with
    the score LOW, no best covisibles, not bad, in no list."""

    def __init__(self, seed, n, dim=64, cur=None, init=0.2, floor=0.2, ratio=0.75, ties=False):
        self.rng = np.random.default_rng(seed)
        self.n, self.dim, self.cur = n, dim, n - 1 if cur is None else cur
        q = self.rng.normal(size=dim)
        self.q = q / np.linalg.norm(q)
        self.gdesc = np.zeros((n, dim), np.float32)
        self.gdesc[self.cur] = self.q
        self.kf_flags = np.zeros(n, np.uint8)
        self.in_db = np.ones(n, np.uint8)
        self.in_db[self.cur] = 0
        self.best_cov = np.full((n, NEIGH), -1, np.int32)
        self.connected, self.covisible = [], []
        self.init, self.floor, self.ratio, self.ties = init, floor, ratio, ties
        for s in range(n):
            if s != self.cur:
                self.score(s, LOW)

    def score(self, s, target, noise=0.5):
        """slot s gets a row whose dot with the query is `target`"""
        r = self.rng.normal(size=self.dim)
        r -= (r @ self.q) * self.q
        nr = np.linalg.norm(r)
        self.gdesc[s] = target * self.q + (noise * r / nr if nr > 0 else 0)
        return self

    def scores(self, targets):
        for s, t in targets.items():
            self.score(s, t)
        return self

    def neigh(self, s, lst):
        self.best_cov[s, :] = -1
        self.best_cov[s, :len(lst)] = lst
        return self

    def bad(self, *slots):
        self.kf_flags[list(slots)] |= 1
        return self

    def arrays(self):
        return dict(gdesc=self.gdesc, kf_flags=self.kf_flags, in_db=self.in_db, best_cov=self.best_cov, cur_slot=np.int32(self.cur),
                    connected=np.asarray(self.connected, np.int64).astype(np.int32), covisible=np.asarray(self.covisible, np.int64).astype(np.int32),
                    min_score_init=np.float32(self.init), min_score_floor=np.float32(self.floor), retain_ratio=np.float32(self.ratio),
                    ties=np.bool_(self.ties))


def check_margins(c, r):
    """r: the decoded result of case c.  Every retrieved slot's score is either farther than MARGIN from min_score or — in a case
    that declares ties — equal to it; every acc farther than MARGIN from min_score_to_retain."""
    role, score = r["role"], r["score"].astype(np.float64)
    for s in np.flatnonzero(role & 1):
        d = abs(score[s] - float(r["min_score"]))
        assert np.isnan(d) or d > MARGIN or (bool(c["ties"]) and d == 0), ("score of slot %d within the margin of min_score" % s, d)
    for p, a in enumerate(r["acc_score"].astype(np.float64)):
        d = abs(a - float(r["min_score_to_retain"]))
        assert d > MARGIN, ("acc of entry %d within the margin of min_score_to_retain" % p, d)


# ---- the named cases -------------------------------------------------------------------------------------------------------
def empty_db():
    c = Case(1, 8)
    c.in_db[:] = 0
    c.scores({0: 0.6, 1: 0.5})
    c.connected, c.covisible = [0, 1], [0, 1]          # scored for the minimum all the same
    return c


def nothing_passes():
    c = Case(2, 9).scores({0: 0.1, 2: 0.15, 3: 0.19, 5: -0.3})
    c.connected, c.covisible = [7], [7]
    c.score(7, 0.7)
    return c


def all_connected():
    c = Case(3, 7).scores({s: 0.4 + 0.05 * s for s in range(6)})
    c.connected, c.covisible = list(range(6)), [0, 1, 2]
    return c


def one_pass():
    return Case(4, 10).scores({3: 0.6})


def neighbour_best():
    """the TENTH best covisible of slot 2 is the best keyframe; its second one passes too"""
    c = Case(5, 12).scores({2: 0.4, 3: 0.9, 5: 0.5})
    return c.neigh(2, [7, 5, 1, 8, 9, 10, 0, 4, 6, 3])


def shared_best():
    """entries 1 and 4 both name slot 6: the first is kept with ITS acc; slot 6 alone falls to the cut"""
    c = Case(6, 10).scores({1: 0.5, 4: 0.45, 6: 0.8})
    return c.neigh(1, [6]).neigh(4, [6, 2])


def retain_cut():
    c = Case(7, 11).scores({2: 0.9, 3: 0.8, 8: 0.3})
    return c.neigh(2, [3])


def equal_scores():
    """slot 5 holds the row of the covisible minimum (its score EQUALS min_score: it does not pass), slots 6 and 7 hold one row and
    name each other (an equal score does not take the best keyframe over, an equal acc does not raise best_acc_score)"""
    c = Case(8, 10, floor=0.0, ties=True).scores({0: 0.15, 6: 0.5})
    c.connected, c.covisible = [0], [0]
    c.gdesc[5] = c.gdesc[0]
    c.gdesc[7] = c.gdesc[6]
    return c.neigh(6, [7]).neigh(7, [6])


def nan_row():
    c = Case(9, 10, floor=0.0).scores({0: 0.1, 2: 0.6, 3: 0.5})
    c.gdesc[4, 7] = np.nan                                # a db member: never passes, never added as a neighbour
    c.gdesc[1, 0] = np.nan                                # a covisible: never lowers the minimum
    c.connected, c.covisible = [0, 1], [1, 0]
    return c.neigh(2, [4, 3])


def bad_keyframe():
    """slot 3 is bad and still retrieved; slot 1 is bad and covisible: its 0.05 does not lower the minimum, so 0.12 does not pass"""
    c = Case(10, 10, floor=0.0).scores({0: 0.15, 1: 0.05, 3: 0.7, 6: 0.12})
    c.bad(1, 3)
    c.connected, c.covisible = [0, 1], [0, 1]
    return c


def cov_min_floor():
    c = Case(11, 9).scores({0: 0.1, 5: 0.15, 6: 0.5})
    c.connected, c.covisible = [0], [0]
    return c


def cov_min_nofloor():
    c = cov_min_floor()
    c.floor = 0.0
    return c


def bad_indices():
    c = Case(12, 9).scores({2: 0.8, 3: 0.5, 4: 0.6, 0: 0.4})
    c.connected, c.covisible = [-1, 9, 2, 1 << 30, 0], [-5, 12, 0, -(1 << 31)]
    return c.neigh(4, [9, -7, 3, -1, (1 << 31) - 1])


def dup_neighbours():
    c = Case(13, 8).scores({2: 0.4, 5: 0.6})
    return c.neigh(2, [5, 5, 5])


def cur_in_db():
    """the query's own slot is flagged as a db member and named as a neighbour: it is never retrieved"""
    c = Case(14, 8, cur=3).scores({1: 0.5, 6: 0.45})
    c.in_db[3] = 1
    return c.neigh(1, [3, 6])


CASES = dict(empty_db=empty_db, nothing_passes=nothing_passes, all_connected=all_connected, one_pass=one_pass,
             neighbour_best=neighbour_best, shared_best=shared_best, retain_cut=retain_cut, equal_scores=equal_scores, nan_row=nan_row,
             bad_keyframe=bad_keyframe, cov_min_floor=cov_min_floor, cov_min_nofloor=cov_min_nofloor, bad_indices=bad_indices,
             dup_neighbours=dup_neighbours, cur_in_db=cur_in_db)


# ---- generated cases ---------------------------------------------------------------------------------------------------------
def generated(seed, n, dim=64, p_pass=0.3, cur=None):
    """a random world: a share p_pass of the slots scores in [0.25, 0.9], the others in [0, 0.15]; random best covisibles; the last
    slots before the query are connected, most of them covisible, one of those bad; a few slots outside the db, a few bad"""
    c = Case(seed, n, dim, cur=cur)
    rng = c.rng
    others = np.array([s for s in range(n) if s != c.cur], np.int64)
    for s in others:
        c.score(s, rng.uniform(0.25, 0.9) if rng.random() < p_pass else rng.uniform(0.0, 0.15))
        k = int(rng.integers(0, NEIGH + 1))
        if k and len(others) > 1:
            c.neigh(s, rng.choice(others[others != s], size=min(k, len(others) - 1), replace=False))
    if len(others):
        conn = others[-min(len(others), 6):]
        c.connected = list(conn)
        c.covisible = list(conn[::-1][:max(1, len(conn) - 1)])
        for s in conn:
            c.score(s, rng.uniform(0.4, 0.9))
        c.bad(conn[0])
        c.in_db[rng.choice(others, size=max(1, len(others) // 16), replace=False)] = 0
        c.bad(*rng.choice(others, size=max(1, len(others) // 20), replace=False))
    return c


def crowd(n, seed=77):
    """every slot but the query passes; the even ones name slot 0, the best of all, first: half of the entries share one best
    keyframe, and the retained ones among them give ONE candidate.  The odd ones name one or two odd slots: a few are retained."""
    c = Case(seed, n)
    rng = c.rng
    c.score(0, 0.95)
    for s in range(1, n - 1):
        c.score(s, rng.uniform(0.3, 0.6))
    odd = np.arange(1, n - 1, 2)
    for s in range(1, n - 1):
        if s % 2 == 0:
            c.neigh(s, [0, int(rng.choice(odd))])
        elif rng.random() < 0.7:
            c.neigh(s, rng.choice(odd[odd != s], size=int(rng.integers(1, 3)), replace=False))
    return c
