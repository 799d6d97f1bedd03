"""Cases of the buffer-extent tests (tests/test_gpu_extents.py) that can be held against the references on the CPU
(tests/test_extent_arena.py): mvpMapPoints arrays whose entries hold values outside [0, n) — stale indices that
include/spfe.h lets "count as none", and that a kernel must therefore never follow — and, for the loop closer's verification
forms (tests/test_gpu_loop_extents.py, tests/test_loop_extent_cases.py), the same values and keypoint indices outside their
range on the keypoints of pairs.  numpy only."""
import numpy as np

INT32_MIN = -2 ** 31
SLACK_ROWS = 64                 # rows of poison the tests keep behind every point array: n + 37 lands inside them
MIN_STALE, MIN_CONTESTED = 8, 3


def stale_values(n):
    """the out-of-range holders of the cases: just past the array, well inside the slack rows, negative ones other than -1"""
    assert 37 < SLACK_ROWS
    return (n, n + 1, n + 37, -7, INT32_MIN)


def in_range(mp, n):
    mp = np.asarray(mp)
    return (mp >= 0) & (mp < n)


def stale_entry(search, entry, K, n, seed=0, contested=4, idle=6):
    """`entry` (int32 [kmax], valid holders and -1) with stale_values(n) written to `contested` keypoints below K that are
    free on entry and that a point claims in search(entry) — the reference's run on the clean entry — and to `idle` free
    ones that nobody claims.  -> (the new entry, the contested keypoints, the idle keypoints)"""
    entry = np.asarray(entry, np.int32)
    rng = np.random.default_rng(seed)
    clean = search(entry)["mp_of_kp"][:K]
    free = entry[:K] == -1
    claimed = np.flatnonzero(free & in_range(clean, n))
    unclaimed = np.flatnonzero(free & (clean == -1))
    ck = np.sort(rng.choice(claimed, min(contested, len(claimed)), replace=False)) if len(claimed) else claimed
    ik = np.sort(rng.choice(unclaimed, min(idle, len(unclaimed)), replace=False)) if len(unclaimed) else unclaimed
    out = entry.copy()
    vals = stale_values(n)
    for j, k in enumerate(np.concatenate([ck, ik])):
        out[k] = vals[j % len(vals)]
    return out, ck, ik


def stale_counts(search, entry, K, n):
    """On the reference's run from `entry`: how many keypoints below K hold a value outside [0, n) other than -1, how many
    of those a point takes all the same (they count as none, so they are free), and whether the others are left alone.
    -> dict(stale, contested, left_alone)"""
    entry = np.asarray(entry, np.int32)
    stale = np.flatnonzero(~in_range(entry[:K], n) & (entry[:K] != -1))
    got = search(entry)["mp_of_kp"][:K]
    taken = in_range(got[stale], n)
    return dict(stale=len(stale), contested=int(taken.sum()),
                left_alone=bool(np.array_equal(got[stale][~taken], entry[stale][~taken])))


def masked(entry, n):
    """the entry with every value outside [0, n) set to -1: what the stale holders count as"""
    entry = np.asarray(entry, np.int32)
    return np.where(in_range(entry, n), entry, -1).astype(np.int32)


def restore_stale(result_mp, entry, K, n):
    """A chain's mp_of_kp computed from masked(entry) -> what it is from `entry` itself: a stale holder below K that no point
    took (the chain's result there is -1) keeps its value."""
    entry, out = np.asarray(entry, np.int32), np.array(result_mp, np.int32)
    k = np.flatnonzero(~in_range(entry[:K], n) & (out[:K] == -1))
    out[k] = entry[k]
    return out


def exact_associations(kp_from, pan_px, kp_to):
    """index into kp_to of the keypoint at kp_from[i] - pan_px, -1 without one (tools/track_scene pans by whole cells: the
    same feature sits at the same sub-pixel position one pan on)"""
    where = {(float(x), float(y)): k for k, (x, y) in enumerate(np.asarray(kp_to, np.float32))}
    moved = (np.asarray(kp_from, np.float32) - np.asarray(pan_px, np.float32)).astype(np.float32)
    return np.array([where.get((float(x), float(y)), -1) for x, y in moved], np.int32)


# ---- the loop closer's verification forms (tests/test_gpu_loop_extents.py, counted in tests/test_loop_extent_cases.py) ---------
# The holder arrays of the two keyframes are followed twice over — match12[k1] -> kf2_mp_of_kp[k2] -> xyz[3 * id] — so a stale
# holder tests something only on a keypoint that a match12 / matches12 / seed entry names: pair_holders() puts them there.
def valid_pairs(m12, mp1, mp2, K1, K2, flags):
    """the k1 below K1 whose entry names a keypoint below K2 with holders in [0, n) on both sides that name searchable points
    (flags uint8 [n], bit 0), one per k2: the pairs every form serves -> k1 ascending"""
    m12, mp1, mp2 = (np.asarray(a, np.int32) for a in (m12, mp1, mp2))
    n = len(flags)
    k1 = np.flatnonzero((m12[:K1] >= 0) & (m12[:K1] < K2))
    k1 = k1[in_range(mp1[k1], n) & in_range(mp2[m12[k1]], n)]
    k1 = k1[((flags[mp1[k1]] & 1) & (flags[mp2[m12[k1]]] & 1)).astype(bool)]
    _, first = np.unique(m12[k1], return_index=True)
    return k1[np.sort(first)]


def pair_holders(m12, mp1, mp2, K1, K2, flags, seed=0, rounds=1):
    """stale_values(n) `rounds` times in keyframe 1's holders and as often in keyframe 2's, each on a keypoint of a pair of its
    own among valid_pairs() -> (mp1, mp2 with the stale holders, the k1 of the pairs spoilt on side 1, on side 2)"""
    vals = stale_values(len(flags)) * rounds
    k1 = valid_pairs(m12, mp1, mp2, K1, K2, flags)
    assert len(k1) >= 2 * len(vals), (len(k1), "pairs")
    pick = np.random.default_rng(seed).permutation(k1)[:2 * len(vals)]
    a, b = np.sort(pick[:len(vals)]), np.sort(pick[len(vals):])
    out1, out2 = np.array(mp1, np.int32), np.array(mp2, np.int32)
    out1[a] = vals
    out2[np.asarray(m12, np.int32)[b]] = vals
    return out1, out2, a, b


def named_stale(m12, mp1, mp2, K1, K2, n):
    """how many stale holders (outside [0, n), not -1) sit on a keypoint that an entry of m12 below K1 names, and which values
    -> dict(stale, values: the set)"""
    m12, mp1, mp2 = (np.asarray(a, np.int32) for a in (m12, mp1, mp2))
    k1 = np.flatnonzero((m12[:K1] >= 0) & (m12[:K1] < K2))
    s1 = mp1[k1][~in_range(mp1[k1], n) & (mp1[k1] != -1)]
    k2 = np.unique(m12[k1])
    s2 = mp2[k2][~in_range(mp2[k2], n) & (mp2[k2] != -1)]
    return dict(stale=len(s1) + len(s2), values=set(s1.tolist()) | set(s2.tolist()))


def wild_indices(K2, kmax):
    """keypoint indices of keyframe 2 that name nothing: the first beyond its count, beyond the arrays, a negative other than -1"""
    return (K2, kmax, kmax + 37, -7)


def wild_entries(entries, m12, mp1, mp2, K1, K2, flags, values, seed=0):
    """`values` written into `entries` (m12 itself, or a seed array) at the k1 of as many valid_pairs() of m12
    -> (the new entries, their k1)"""
    k1 = valid_pairs(m12, mp1, mp2, K1, K2, flags)
    assert len(k1) >= len(values), (len(k1), "pairs")
    at = np.sort(np.random.default_rng(seed).permutation(k1)[:len(values)])
    out = np.array(entries, np.int32)
    out[at] = values
    return out, at
