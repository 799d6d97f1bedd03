"""Cases of the buffer-extent tests (tests/test_gpu_extents.py) that can be held against the references on the CPU
(tests/test_extent_arena.py): mvpMapPoints arrays whose entries hold values outside [0, n) — stale indices that
include/spfe.h lets "count as none", and that a kernel must therefore never follow.  numpy only."""
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
