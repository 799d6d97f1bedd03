"""The host's part of the loop detection behind the block of spfe_detect_loop_candidates_device: the consistency groups of
LoopClosingVLAD::detectLoopVLAD (loop_closer_vlad.cpp:171-251), a few set intersections over a handful of candidates.  This is the
recipe of INTEGRATION.md as runnable code: keyframes are slots, `connected_of(slot)` is GetConnectedKeyFrames() of the host's
covisibility graph.  No numpy needed."""


class ConsistencyWalk:
    """mvConsistentGroups between the queries.  step() is one detectLoopVLAD behind the retrieval and returns
    mvpEnoughConsistentCandidates, in order; a loop is detected when it is not empty."""

    def __init__(self, consistency_th=3):
        self.th = consistency_th          # mnCovisibilityConsistencyTh
        self.groups = []                  # mvConsistentGroups: (set of slots, consistency)

    def step(self, cand_slot, connected_of):
        cands = [int(s) for s in cand_slot]
        if not cands:                     # :172-177: no candidates, the groups are forgotten
            self.groups = []
            return []
        enough, current = [], []
        seen = [False] * len(self.groups)
        for cand in cands:
            group = set(int(s) for s in connected_of(cand))
            group.add(cand)
            cand_enough = some = False
            for g, (previous, consistency) in enumerate(self.groups):
                if group.isdisjoint(previous):
                    continue
                some = True
                now = consistency + 1
                if not seen[g]:
                    current.append((group, now))
                    seen[g] = True
                if now >= self.th and not cand_enough:
                    enough.append(cand)
                    cand_enough = True
            if not some:                  # :232-237: the reference CLEARS what it collected so far, then starts this group at 0
                current = [(group, 0)]
        self.groups = current
        return enough
