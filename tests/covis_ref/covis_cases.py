"""Cases of the covisibility graph, and an INDEPENDENT Python statement of the reference's lines (keyframe.cpp:577-612, :757-849) that
covis_ref.c is held to: observation dicts built from the rows, a dict counter, sorted() of (weight, slot) pairs reversed, and
AddConnection with its three branches.  A case is the keyframe rows, the flags, the parameters and a list of CALLS (the slot each
call updates, the state carried from call to call, starting from the preset) with EDITS of row entries in front of a call; the
named cases are what the fixtures tests/golden/covis_*.npz record (tests/golden/make_golden_covis.py), each built to show one rule
of include/spfe_covis_math.h.  numpy only."""
import numpy as np

KEYS = ("kf_mp_of_kp", "kf_flags", "mp_flags", "conn_cap", "th", "origin_slot", "n_best_a", "n_best_b", "calls", "edits")


# ---- the Python statement -------------------------------------------------------------------------------------------------------
class PyGraph:
    """mConnectedKeyFrameWeights, the two ordered vectors as one list of (slot, weight), mpParent and mbFirstConnection a slot"""

    def __init__(self, n_slots):
        self.conn = [dict() for _ in range(n_slots)]
        self.ord = [[] for _ in range(n_slots)]
        self.parent = [-1] * n_slots
        self.first = [True] * n_slots

    def update_best_covisibles(self, s):
        pairs = sorted((w, k) for k, w in self.conn[s].items())
        self.ord[s] = [(k, w) for w, k in reversed(pairs)]          # push_front of the ascending pairs

    def add_connection(self, s, kf, w):
        if kf not in self.conn[s]:
            self.conn[s][kf] = w
        elif self.conn[s][kf] != w:
            self.conn[s][kf] = w
        else:
            return False
        self.update_best_covisibles(s)
        return True


def py_update_connections(g, rows, kf_flags, mp_flags, cur, th, origin_slot):
    """KeyFrame::UpdateConnections of slot cur on PyGraph g -> the slots whose ordered vectors were rebuilt (cur included), or None
    when the counter is empty.  The rows must not hold a point twice (a keyframe observes a point through ONE index)."""
    obs = {}                                                        # MapPoint::GetObservations(): point -> {keyframe: index}
    for s, row in enumerate(rows):
        if kf_flags[s] & 1:
            continue                                                # SetBadFlag erased them
        for k, p in enumerate(row):
            if 0 <= p < len(mp_flags):
                obs.setdefault(int(p), {})[s] = k
    counter = {}
    for p in rows[cur]:
        if not 0 <= p < len(mp_flags) or not mp_flags[p] & 1:       # null or isBad()
            continue
        for s in obs.get(int(p), {}):
            if s != cur:
                counter[s] = counter.get(s, 0) + 1
    if not counter:
        return None
    nmax, kmax, pairs, rebuilt = 0, None, [], []
    for s in sorted(counter):                                       # the map's order
        if counter[s] > nmax:
            nmax, kmax = counter[s], s
        if counter[s] >= th:
            pairs.append((counter[s], s))
            if g.add_connection(s, cur, counter[s]):
                rebuilt.append(s)
    if not pairs:
        pairs.append((nmax, kmax))
        if g.add_connection(kmax, cur, nmax):
            rebuilt.append(kmax)
    pairs.sort()
    g.conn[cur] = dict(counter)
    g.ord[cur] = [(s, w) for w, s in reversed(pairs)]
    if g.first[cur] and cur != origin_slot:
        g.parent[cur] = g.ord[cur][0][0]
        g.first[cur] = False
    return rebuilt + [cur]


def py_state_arrays(g, conn_cap):
    """PyGraph as the eight state arrays (covis_ref.new_state's layout)"""
    n = len(g.conn)
    s = dict(conn_slot=np.full((n, conn_cap), -1, np.int32), conn_w=np.zeros((n, conn_cap), np.int32), conn_n=np.zeros(n, np.int32),
             ord_slot=np.full((n, conn_cap), -1, np.int32), ord_w=np.zeros((n, conn_cap), np.int32), ord_n=np.zeros(n, np.int32),
             parent=np.array(g.parent, np.int32), first_conn=np.array(g.first, np.uint8))
    for i in range(n):
        for j, k in enumerate(sorted(g.conn[i])):
            s["conn_slot"][i, j], s["conn_w"][i, j] = k, g.conn[i][k]
        for j, (k, w) in enumerate(g.ord[i]):
            s["ord_slot"][i, j], s["ord_w"][i, j] = k, w
        s["conn_n"][i], s["ord_n"][i] = len(g.conn[i]), len(g.ord[i])
    return s


def py_table_rows(g, slots, table):
    """GetBestCovisibilityKeyFrames(n_best) of the given slots into their rows of table"""
    for s in slots:
        lst = [k for k, _ in g.ord[s][:table.shape[1]]]
        table[s] = lst + [-1] * (table.shape[1] - len(lst))


# ---- the cases --------------------------------------------------------------------------------------------------------------------
class Case:
    """n_slots keyframes of kp_stride entries over a table of n_table points, all SEARCHABLE; every row starts empty (-1)."""

    def __init__(self, n_slots, kp_stride, n_table, th=2, conn_cap=8, origin_slot=-1, n_best_a=3, n_best_b=2):
        self.rows = np.full((n_slots, kp_stride), -1, np.int32)
        self.kf_flags = np.zeros(n_slots, np.uint8)
        self.mp_flags = np.ones(n_table, np.uint8)
        self.p = dict(conn_cap=conn_cap, th=th, origin_slot=origin_slot, n_best_a=n_best_a, n_best_b=n_best_b)
        self.calls, self.edits = [], []

    def row(self, s, points):
        self.rows[s, :len(points)] = points
        return self

    def bad_kf(self, *slots):
        self.kf_flags[list(slots)] |= 1
        return self

    def bad_mp(self, *points):
        self.mp_flags[list(points)] &= 0xFE
        return self

    def call(self, cur, edit=None):
        """a call for slot cur; edit: {(slot, k): point} applied to the rows in front of it"""
        for (s, k), p in (edit or {}).items():
            self.edits.append((len(self.calls), s, k, p))
        self.calls.append(cur)
        return self

    def arrays(self):
        return dict(kf_mp_of_kp=self.rows, kf_flags=self.kf_flags, mp_flags=self.mp_flags, calls=np.array(self.calls, np.int32),
                    edits=np.array(self.edits, np.int32).reshape(-1, 4), **self.p)


def named_cases():
    """name -> case dict.  Slots and points are small numbers so that the expected state can be read off the construction."""
    c = {}
    # slot 0 runs its own step 5 (ord = [1] alone, conn = {1: 3, 2: 1}); then slot 1 links 0 with the SAME weight: nothing, no re-sort
    c["equal_weight_no_resort"] = Case(3, 4, 8).row(0, [0, 1, 2, 5]).row(1, [0, 1, 2]).row(2, [5]).call(0).call(1)
    # two neighbours of weight 2: the HIGHER slot first
    c["equal_weights_slot_descending"] = Case(4, 6, 8).row(0, [0, 1]).row(1, [0, 1, 2, 3, 4, 5]).row(2, [2, 3]).row(3, [4, 5]).call(1)
    # nobody reaches th: the FIRST of the equal maxima alone
    c["first_maximum_alone"] = Case(4, 4, 8, th=5).row(0, [0]).row(1, [2, 3]).row(2, [0, 1, 2, 3]).row(3, [0, 1]).call(2)
    # a neighbour exactly at th is linked
    c["exactly_at_threshold"] = Case(3, 5, 8).row(0, [0, 1]).row(1, [0, 1, 2, 3, 4]).row(2, [2, 3, 4]).call(1)
    # the current keyframe's ord is P alone, its conn the whole counter
    c["ord_cur_is_p_alone"] = Case(3, 3, 8).row(0, [0, 1]).row(1, [0, 1, 2]).row(2, [2]).call(1)
    # slot 0 gets 2 by the maximum rule (weight 1 < th 3), then 1 at weight 3: its ord is the WHOLE map, [1, 2]
    c["neighbour_ord_whole_map"] = Case(3, 4, 8, th=3).row(0, [0, 1, 2, 3]).row(1, [0, 1, 2]).row(2, [3]).call(2).call(1)
    # the second call of slot 2 finds another best neighbour: the parent stays
    c["second_call_keeps_parent"] = (Case(3, 3, 8, th=1).row(0, [0]).row(1, [1, 2]).row(2, [0]).call(2)
                                     .call(2, {(2, 1): 1, (2, 2): 2}))
    # the origin keyframe gets no parent and keeps its first_conn byte
    c["origin_gets_no_parent"] = Case(2, 2, 4, th=1, origin_slot=0).row(0, [0, 1]).row(1, [0, 1]).call(0).call(1)
    # a bad keyframe shares the most: not counted, not linked
    c["bad_slot_not_counted"] = Case(3, 3, 8).row(0, [0, 1, 2]).row(1, [0, 1, 2]).row(2, [0, 1]).bad_kf(0).call(1)
    # the current row is not counted against itself
    c["cur_slot_not_counted"] = Case(2, 3, 8).row(0, [0, 1, 2]).row(1, [0, 1]).call(0)
    # cur_slot itself is not tested for bad: a bad keyframe is updated like any other (and links its good neighbour)
    c["bad_cur_still_updates"] = Case(2, 3, 8).row(0, [0, 1, 2]).row(1, [0, 1]).bad_kf(0).call(0).call(1)
    # THIS PROJECT'S RULE: point 0 twice in the current row counts twice everywhere; point 1 twice in row 2 counts twice there
    c["repeated_point_counts_twice"] = Case(3, 4, 8).row(0, [0, 0, 1]).row(1, [0]).row(2, [1, 1]).call(0)
    # a bad point and entries outside the table count nothing
    c["bad_point_and_wild_entries"] = (Case(3, 5, 6).row(0, [0, 1, 6, -3, 2**31 - 1]).row(1, [0, 1, 6]).row(2, [1, -2**31, 2])
                                       .bad_mp(0).call(0))
    # the weight changes between two calls: replaced (code 1), the neighbour's ord re-sorted
    c["weight_replaced"] = (Case(3, 4, 8, th=1).row(0, [0, 1, 2, 3]).row(1, [0]).row(2, [1, 2]).call(1).call(2)
                            .call(1, {(1, 1): 1, (1, 2): 2, (1, 3): 3}))
    # conn_cap 1: slot 0 is full when 2 comes (code 3, NEIGH_OVERFLOW), and 2 links it all the same
    c["neighbour_full"] = Case(3, 2, 4, th=1, conn_cap=1).row(0, [0, 1]).row(1, [0]).row(2, [1]).call(1).call(2)
    # conn_cap 1 and two sharers: CUR_OVERFLOW, nothing changes
    c["cur_overflow"] = Case(3, 2, 4, th=1, conn_cap=1).row(0, [0]).row(1, [0, 1]).row(2, [1]).call(1)
    # nobody shares anything: NO_SHARED, nothing changes
    c["no_shared"] = Case(3, 2, 4).row(0, [0]).row(1, [1]).row(2, [2, 3]).call(1).call(2)
    # one slot, one entry
    c["one_by_one"] = Case(1, 1, 1, conn_cap=1, n_best_a=1, n_best_b=1).row(0, [0]).call(0)
    # tables wider than the lists, -1 padded; three neighbours in weight order
    c["tables_padded"] = (Case(4, 6, 8, th=1, n_best_a=5, n_best_b=1).row(0, [0]).row(1, [0, 1, 2, 3, 4, 5]).row(2, [1, 2, 3])
                          .row(3, [4, 5]).call(1))
    return {k: v.arrays() for k, v in c.items()}


# the fixture that tells each mutation of covis_ref.MUTATIONS from the reference
TELLS = {"resort_on_equal_weight": "equal_weight_no_resort", "equal_weights_ascending_slot": "equal_weights_slot_descending",
         "last_maximum": "first_maximum_alone", "gt_for_ge_th": "exactly_at_threshold", "ord_cur_from_whole_map": "ord_cur_is_p_alone",
         "neighbour_ord_thresholded": "neighbour_ord_whole_map", "reparent_on_second_call": "second_call_keeps_parent",
         "parent_for_origin": "origin_gets_no_parent", "bad_slots_counted": "bad_slot_not_counted",
         "cur_slot_counted": "cur_slot_not_counted"}


def generated_rows(seed, n_slots, kp_stride, n_table, fill=0.7, window=None, p_bad_kf=0.1, p_bad_mp=0.1, wild=True):
    """A random map without a repeated point inside a row: keyframe s sees distinct points of a window of the table around its place,
    so that neighbours share points; about one keyframe and one point in ten are bad; a few entries are outside the table.
    -> rows, kf_flags, mp_flags"""
    rng = np.random.default_rng(seed)
    rows = np.full((n_slots, kp_stride), -1, np.int32)
    win = max(1, min(n_table, window or 4 * kp_stride))
    for s in range(n_slots):
        k_s = min(int(rng.integers(0, kp_stride + 1)) if fill is None else int(round(fill * kp_stride)), win)
        if k_s:
            lo = int(s * max(n_table - win, 0) / max(n_slots - 1, 1))
            pts = (lo + rng.choice(win, k_s, replace=False)).astype(np.int64)
            if wild:
                w = rng.random(k_s) < 0.03
                pts[w] = rng.choice([n_table, n_table + 5, -2, 2**31 - 1, -2**31, -1, -1], int(w.sum()))
            at = np.sort(rng.choice(kp_stride, k_s, replace=False))
            rows[s, at] = pts
    kf_flags = (rng.random(n_slots) < p_bad_kf).astype(np.uint8)
    mp_flags = np.where(rng.random(n_table) < p_bad_mp, 0, 1).astype(np.uint8)
    mp_flags[rng.random(n_table) < 0.05] |= 2     # another flag bit changes nothing
    return rows, kf_flags, mp_flags


def sequence(seed, n_kf=40, kp_stride=48, n_table=400, bad_at=(12, 25, 33)):
    """n_kf keyframes inserted one after another, each updated TWICE as LocalMapping does (local_mapper.cpp:275, :903): in front of
    the second call SearchInNeighbors has added a few points to the new row and to its neighbours'.  At the steps of bad_at the
    keyframe three slots back turns bad.  No row ever holds a point twice.  -> list of (rows, kf_flags, mp_flags, cur), the arrays
    as that call sees them (copies); slots not yet inserted are empty rows."""
    rng = np.random.default_rng(seed)
    rows = np.full((n_kf, kp_stride), -1, np.int32)
    kf_flags = np.zeros(n_kf, np.uint8)
    mp_flags = np.where(rng.random(n_table) < 0.08, 0, 1).astype(np.uint8)
    win = min(n_table, kp_stride + kp_stride // 3)
    steps = []

    def add(s, count):
        lo = int(s * max(n_table - win, 0) / max(n_kf - 1, 1))
        free = np.flatnonzero(rows[s] < 0)
        new = np.setdiff1d(lo + np.arange(win), rows[s])
        k = min(count, len(free), len(new))
        if k:
            rows[s, rng.choice(free, k, replace=False)] = rng.choice(new, k, replace=False)

    for i in range(n_kf):
        add(i, (kp_stride * 5) // 8)
        if i in bad_at:
            kf_flags[i - 3] |= 1
        steps.append((rows.copy(), kf_flags.copy(), mp_flags.copy(), i))
        for s in range(max(0, i - 3), i + 1):
            add(s, 3)
        steps.append((rows.copy(), kf_flags.copy(), mp_flags.copy(), i))
    return steps
