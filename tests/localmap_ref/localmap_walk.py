"""An independent statement of the reference's lines (tracker.cpp:843-984) in Python, for tests/test_localmap_reference.py: dicts
and sets where the reference has a std::map or a std::set, sorted() by slot where it iterates one, and the observation graph built
from the rows (an entry of a row is one observation; the weight of a point saturates at 127 as the contract says).  It shares no
code with localmap_ref.c."""
import collections


def walk(c):
    rows, kf_flags, best_cov, parent = c["kf_mp_of_kp"], c["kf_flags"], c["best_cov"], c["parent"]
    mp_flags, mp_of_kp = c["mp_flags"], c["mp_of_kp"]
    n, n_table = len(rows), len(mp_flags)
    good = lambda p: 0 <= p < n_table and bool(mp_flags[p] & 1)   # noqa: E731
    bad_kf = lambda s: bool(kf_flags[s] & 1)                      # noqa: E731
    observations = collections.defaultdict(list)                  # MapPoint::GetObservations()
    total = [0] * n
    for s in range(n):
        for p in map(int, rows[s]):
            if good(p):
                observations[p].append(s)
                total[s] += 1
    # :889-903
    frame = [int(p) if good(int(p)) else None for p in mp_of_kp]
    weight = collections.Counter(p for p in frame if p is not None)
    counter = {}
    for p, w in weight.items():
        for s in observations[p]:
            counter[s] = counter.get(s, 0) + min(w, 127)
    votes = [counter.get(s, 0) for s in range(n)]
    # :906-930
    status, best, ref = 0, 0, -1
    local = []
    seen = set()
    for s in sorted(counter):
        if bad_kf(s):
            continue
        if counter[s] > best:
            best, ref = counter[s], s
        local.append(s)
        seen.add(s)
    n_voted = len(local)
    if not local:
        status |= 1
    # :932-978
    children = collections.defaultdict(set)
    for s in range(n):
        if 0 <= parent[s] < n:
            children[int(parent[s])].add(s)
    for v in list(local):
        if len(local) > c["max_keyframes"]:
            break
        for s in map(int, best_cov[v]):
            if not 0 <= s < n:
                if s != -1:
                    status |= 4
                continue
            if not bad_kf(s) and s not in seen:
                local.append(s)
                seen.add(s)
                break
        for ch in sorted(children[v]):
            if not bad_kf(ch) and ch not in seen:
                local.append(ch)
                seen.add(ch)
                break
        p = int(parent[v])
        if p < -1 or p >= n:
            status |= 4
        elif p >= 0 and p not in seen:
            local.append(p)
            seen.add(p)
            break
    # the frame's points first, then :843-866
    points, where = [], {}
    for p in frame:
        if p is not None and p not in where:
            where[p] = len(points)
            points.append(p)
    n_held = len(points)
    for s in local:
        for p in map(int, rows[s]):
            if good(p) and p not in where:
                where[p] = len(points)
                points.append(p)
    cap = c["point_cap"]
    if len(points) > cap:
        status |= 2
    return dict(n_voted=n_voted, n_local_kf=len(local), ref_slot=ref, n_held=n_held, n_points=min(len(points), cap),
                n_points_total=len(points), status=status, local_kf=local, votes=votes, total=total,
                point_idx=points[:cap] + [-1] * max(0, cap - len(points)),
                mp_of_kp_list=[-1 if p is None else where[p] for p in frame])
