"""The host's side of LoopClosingVLAD::ComputeSim3's loop with the guided match in it: the walk of tests/sim3_ref/sim3_walk.py
whose accept(i, h) is no longer a stub table but is fed from what the guided match reports for (candidate, hypothesis):
SearchBySim3Override's matches12 go to Optimizer::OptimizeSim3 (loop_closer_vlad.cpp:424-432), which returns the number of
correspondences it keeps as inliers — never more than the n_total it was given — and the candidate is accepted with 20 or more.
So n_total < 20 rejects without a call of the optimiser, and otherwise the host's optimiser decides; both walks (the literal
`while` and the replay of the device's report) see the same accept, and the guided jobs a host needs are exactly the pairs the
walk tries: `jobs_of` lists them in the order the batched call takes them.  No numpy needed."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sim3_ref"))
import sim3_walk  # noqa: E402

MIN_INLIERS = 20                 # nInliers >= 20 (loop_closer_vlad.cpp:428)
MAX_JOBS = 32                    # SPFE_GUIDED_MAX_JOBS


def accept_from(n_total, optimise=lambda i, h, n: n):
    """n_total: {(candidate, hypothesis): n_total of its guided block}; optimise(i, h, n_total) -> OptimizeSim3's inliers (the
    default keeps every correspondence).  -> accept(i, h)"""
    def accept(i, h):
        n = n_total[(i, h)]
        if n < MIN_INLIERS:
            return False                                                 # the optimiser cannot keep more than it is given
        kept = optimise(i, h, n)
        assert kept <= n
        return kept >= MIN_INLIERS
    return accept


def jobs_of(cands):
    """every (candidate, hypothesis) the walk can try: the returns below each candidate's iteration limit, candidate by candidate.
    More than MAX_JOBS go in several calls."""
    jobs = [(i, int(h)) for i, c in enumerate(cands) if c["n_matches"] >= 20 and c["N"] >= 20 for h in c["return_idx"] if h < c["limit"]]
    return [jobs[k:k + MAX_JOBS] for k in range(0, len(jobs), MAX_JOBS)]


def literal(cands, n_total, **kw):
    return sim3_walk.literal(cands, accept_from(n_total, **kw))


def walk(cands, n_total, **kw):
    return sim3_walk.walk(cands, accept_from(n_total, **kw))


# ---- SearchByProjectionLoop on toy lists: the literal sequential loop against the ordered claim as a fixed point -----------------
def loop_literal(cands, dists, ids, matched, th_dist=0.7):
    """cands[i]: the window's keypoints of point i in window order (None: refused before the window), dists[i] their
    distances.  -> (kp_of_mp, matched after the loop)"""
    m = list(matched)
    out = []
    for i, c in enumerate(cands):
        best, bk = 256.0, -1
        for k, d in zip(c or [], dists[i] or []):
            if m[k] == -1 and d < best:
                best, bk = d, k
        if bk < 0 or best > th_dist:
            out.append(-1)
            continue
        out.append(bk)
        m[bk] = ids[i]
    return out, m


def loop_fixed_point(cands, dists, ids, matched, th_dist=0.7):
    """the kernels' rounds: every unfinished point posts its index on its unblocked candidates; a point that finds itself on
    all of them is final.  -> (kp_of_mp, matched, rounds)"""
    n = len(cands)
    m = list(matched)
    blocked = [v != -1 for v in m]
    out, done, rounds = [-1] * n, [not c for c in cands], 0
    while not all(done):
        rounds += 1
        assert rounds <= n
        claim = {}
        for i in range(n):
            if not done[i]:
                for k in cands[i]:
                    if not blocked[k]:
                        claim[k] = min(claim.get(k, i), i)
        decided = []
        for i in range(n):
            if done[i]:
                continue
            free = [(k, d) for k, d in zip(cands[i], dists[i]) if not blocked[k]]
            if any(claim[k] != i for k, _ in free):
                continue
            best, bk = 256.0, -1
            for k, d in free:
                if d < best:
                    best, bk = d, k
            decided.append((i, bk if bk >= 0 and not best > th_dist else -1))
        for i, bk in decided:                                           # all decisions of a round read the same state
            done[i] = True
            out[i] = bk
            if bk >= 0:
                blocked[bk] = True
                m[bk] = ids[i]
    return out, m, rounds
