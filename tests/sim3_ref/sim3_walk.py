"""The host's side of LoopClosingVLAD::ComputeSim3's loop, twice: a literal restatement of the reference's `while`
(loop_closer_vlad.cpp:395-449) over solvers whose iterate() is Sim3Solver::iterate (sim3_solver.cpp:140-206) on a table of
per-hypothesis inlier counts, and the walk over what the library reports per candidate — N, the ordered list of returns, the
iteration limit of spfe_sim3_iteration_limit — without any solver state.  literal(...) == walk(...) is what shows that
evaluating every hypothesis up front and replaying the interleaving is exact.  OptimizeSim3 (with SearchBySim3Override in
front of it) is a stub that accepts or rejects a (candidate, hypothesis) by a table.  No numpy needed."""
ROUND = 5                        # iterate(5, ...)


class Solver:
    """Sim3Solver as far as the loop sees it: counts[h] is what CheckInliers gives hypothesis h"""

    def __init__(self, N, counts, limit, min_inliers=20):
        self.N, self.counts, self.max_its, self.min_inliers = N, counts, limit, min_inliers
        self.n_iterations, self.best = 0, 0

    def iterate(self, n):
        """-> (hypothesis returned or None, bNoMore)"""
        if self.N < self.min_inliers:
            return None, True
        cur = 0
        while self.n_iterations < self.max_its and cur < n:
            cur += 1
            h = self.n_iterations
            self.n_iterations += 1
            c = self.counts[h]
            if c >= self.best:
                self.best = c
                if c > self.min_inliers:
                    return h, False
        return None, self.n_iterations >= self.max_its


def literal(cands, accept, min_matches=20):
    """cands: per candidate dict(n_matches, N, counts, limit); accept(i, h) -> bool (OptimizeSim3 gives >= 20 inliers).
    -> (matched candidate or None, its hypothesis, the (candidate, hypothesis) pairs handed to OptimizeSim3 in order)"""
    n = len(cands)
    discarded, solvers, n_cand = [False] * n, [None] * n, 0
    for i, c in enumerate(cands):
        if c["n_matches"] < min_matches:
            discarded[i] = True
            continue
        solvers[i] = Solver(c["N"], c["counts"], c["limit"])
        n_cand += 1
    tried, match = [], None
    while n_cand > 0 and match is None:
        for i in range(n):
            if discarded[i]:
                continue
            h, no_more = solvers[i].iterate(ROUND)
            if no_more:
                discarded[i] = True
                n_cand -= 1
            if h is not None:
                tried.append((i, h))
                if accept(i, h):
                    match = (i, h)
                    break
    return (match[0], match[1], tried) if match else (None, None, tried)


def schedule(N, return_idx, limit, min_inliers=20):
    """The calls of iterate(5) of one candidate from the device's report: a list of (hypothesis returned or None, bNoMore),
    one entry per call until bNoMore.  A call starts where the last one stopped, ends at a return, after 5 hypotheses or at
    the limit; hypotheses at and beyond the limit are ignored."""
    if N < min_inliers:
        return [(None, True)]
    rets = [int(h) for h in return_idx if h < limit]
    calls, pos, r = [], 0, 0
    while True:
        end = min(pos + ROUND, limit)
        if r < len(rets) and rets[r] < end:
            calls.append((rets[r], False))        # (a return never sets bNoMore, even on the last hypothesis)
            pos, r = rets[r] + 1, r + 1
            continue
        pos = end
        calls.append((None, pos >= limit))
        if pos >= limit:
            return calls


def walk(cands, accept, min_matches=20):
    """the same result from (n_matches, N, return_idx, limit) per candidate"""
    n = len(cands)
    sched = [None if c["n_matches"] < min_matches else schedule(c["N"], c["return_idx"], c["limit"]) for c in cands]
    at = [0] * n
    live = [s is not None for s in sched]
    tried = []
    while any(live):
        for i in range(n):
            if not live[i]:
                continue
            h, no_more = sched[i][at[i]]
            at[i] += 1
            if no_more:
                live[i] = False
            if h is not None:
                tried.append((i, h))
                if accept(i, h):
                    return i, h, tried
    return None, None, tried


def returns_of(counts, min_inliers=20):
    """the prefix-maximum rule (what sim3_select_kernel reports as return_idx)"""
    best, out = 0, []
    for h, c in enumerate(counts):
        if c >= best:
            best = c
            if c > min_inliers:
                out.append(h)
    return out
