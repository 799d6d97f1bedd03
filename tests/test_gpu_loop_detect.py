"""GPU: the loop detection on the device (spfe_detect_loop_candidates_device, spfe_detect_loop_candidates: loopdet.hip) against
the host reference tests/loopdet_ref/loopdet_ref.c, which shares include/spfe_loopdet_math.h with the kernels: the WHOLE output
block byte for byte, from both forms, every byte the block does not name and every byte behind it still holding the preset — on
the fixtures tests/golden/loopdet_*.npz; at the row lengths where the sum takes another shape (a slot without an element, a
partial last pass, exactly one pass, one pass and one float4, the full row); at the table sizes around one and four passes of the
one-workgroup kernels and at 5000 slots that all pass, half of them naming one best keyframe; on 300 rows of 4096; with a NaN row
in the database; a row appended by an asynchronous copy with the detection behind it on the same stream; five consecutive
queries whose candidates go through tests/loopdet_ref/loopdet_walk.py; the refusals."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("loopdet_ref", ""):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
import loopdet_cases as lc  # noqa: E402
import loopdet_ref  # noqa: E402
import loopdet_walk  # noqa: E402
import test_loopdet_reference as tlr  # noqa: E402  (the Python statement of the reference and the transcription of its walk)

from sp_orb_slam_amd import extractor as X  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import SPExtractor, SpfeError  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = loopdet_ref.FILL
GUARD = 1024          # bytes behind the block that must keep the preset
PRM = ("min_score_init", "min_score_floor", "retain_ratio")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return loopdet_ref.build(tmp_path_factory.mktemp("loopdet_ref"))


@pytest.fixture(scope="module")
def ext():
    e = SPExtractor(100, 64, 96, weights.synthetic(7, "trackable"), with_heat=False)
    yield e
    e.close()


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.reshape(-1).view(np.uint8).copy() if a.size else np.zeros(16, np.uint8)).cuda()


def upload(c):
    a = loopdet_ref.arrays(c)
    return a, {k: dev(v) for k, v in a.items()}


def call_device(ext, c, a, d, d_out, stream=None):
    n, dim = a["gdesc"].shape
    ext.detect_loop_candidates_device(d["gdesc"].data_ptr(), dim, d["kf_flags"].data_ptr(), d["in_db"].data_ptr(),
                                      d["best_cov"].data_ptr(), n, int(c["cur_slot"]),
                                      d["connected"].data_ptr() if a["connected"].size else None, len(a["connected"]),
                                      d["covisible"].data_ptr() if a["covisible"].size else None, len(a["covisible"]),
                                      d_out.data_ptr(), *[float(c[k]) for k in PRM], stream=stream)


def run_record(ext, c):
    """spfe_detect_loop_candidates_device on a block and a guard behind it filled with FILL -> the block (the guard checked)"""
    import torch
    a, d = upload(c)
    n = len(a["gdesc"])
    nb = ext.loopdet_out_bytes(n)
    assert nb == loopdet_ref.out_bytes(n)
    d_out = torch.full((nb + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    before = {k: v.clone() for k, v in d.items()}
    call_device(ext, c, a, d, d_out)
    torch.cuda.synchronize()
    assert all(torch.equal(d[k], before[k]) for k in d), "an input was written"
    raw = d_out.cpu().numpy()
    assert (raw[nb:] == FILL).all(), "bytes behind the block were written"
    return raw[:nb]


def run_host(ext, c):
    a = loopdet_ref.arrays(c)
    return ext.detect_loop_candidates(a["gdesc"], a["kf_flags"], a["in_db"], a["best_cov"], int(c["cur_slot"]), a["connected"],
                                      a["covisible"], *[float(c[k]) for k in PRM], fill=FILL)


def same(block, want, what):
    """the whole block, the bytes nobody names included"""
    n = len(want["score"])
    if block.tobytes() == want["block"].tobytes():
        return
    g = X.SPExtractor.decode_loopdet_out(block, n)
    for k in loopdet_ref.INTS:
        assert g[k] == want[k], (what, k, g[k], want[k])
    for k in loopdet_ref.SCORES:
        assert tlr.bits(g[k]) == tlr.bits(want[k]), (what, k, g[k], want[k])
    for k in loopdet_ref.LISTS + loopdet_ref.FLOATS:
        assert g[k].tobytes() == want[k].tobytes(), (what, k, np.flatnonzero(g[k].view(np.uint8) != want[k].view(np.uint8))[:8])
    diff = np.flatnonzero(block != want["block"])
    assert not len(diff), (what, "bytes the block does not name", diff[:8])


def both_forms(ext, ref, c, what):
    want = loopdet_ref.detect(ref, c)
    lc.check_margins(c, want)
    same(run_record(ext, c), want, what + ", record form")
    same(run_host(ext, c), want, what + ", host form")
    return want


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_fixtures(ext, ref, name):
    z = np.load(os.path.join(ROOT, "tests", "golden", "loopdet_%s.npz" % name))
    c = {k: z[k] for k in lc.KEYS}
    want = both_forms(ext, ref, c, name)
    for k in loopdet_ref.LISTS + loopdet_ref.FLOATS:                 # ... and the reference still gives what was recorded
        assert want[k].tobytes() == z["e_" + k].tobytes(), (name, k)
    unscored = want["role"] == 0
    assert (want["score"].view(np.uint32)[unscored] == X.LOOPDET_NO_SCORE_BITS).all()
    g = X.SPExtractor.decode_loopdet_out(run_record(ext, c), len(unscored))
    assert (g["score"].view(np.uint32)[unscored] == X.LOOPDET_NO_SCORE_BITS).all() and g["n_scored"] == int((~unscored).sum())


@pytest.mark.parametrize("dim", [4, 252, 1024, 1028, 4096])
def test_row_lengths(ext, ref, dim):
    want = both_forms(ext, ref, lc.generated(200 + dim, 37, dim).arrays(), "dim %d" % dim)
    assert want["n_pass"] >= 3 and want["n_cand"] >= 1


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1023, 1024, 1025])
def test_table_sizes(ext, ref, n):
    """around a group of four rows, one pass (1024 threads) of the one-workgroup kernels and the 256 threads of the score"""
    want = both_forms(ext, ref, lc.generated(300 + n, n, 64, p_pass=0.6).arrays(), "n_slots %d" % n)
    assert n == 1 or (want["n_pass"] > n // 3 and want["n_cand"] >= 1)
    if n >= 255:
        both_forms(ext, ref, lc.generated(400 + n, n, 64, p_pass=0.6, cur=n // 2).arrays(), "n_slots %d, the query in the middle" % n)


def test_every_slot_passes_and_half_share_a_best_keyframe(ext, ref):
    c = lc.crowd(5000).arrays()
    want = both_forms(ext, ref, c, "5000 slots")
    retained = want["acc_score"] > want["min_score_to_retain"]
    assert want["n_pass"] == 4999 and (want["best_slot"] == 0).sum() >= 2499
    assert (retained & (want["best_slot"] == 0)).sum() > 1024 and (want["cand_slot"] == 0).sum() == 1
    assert 1 < want["n_cand"] < retained.sum() and np.flatnonzero(retained).max() > 4000


def test_300_rows_of_4096(ext, ref):
    want = both_forms(ext, ref, lc.generated(500, 300, 4096).arrays(), "300 x 4096")
    assert want["n_scored"] > 250 and want["n_pass"] > 50


def test_nan_row_in_the_database(ext, ref):
    case = lc.generated(600, 300, 4096, p_pass=0.5)
    base = loopdet_ref.detect(ref, case.arrays())
    victim = int(base["pass_slot"][len(base["pass_slot"]) // 2])      # a slot that passes, and is somebody's neighbour
    case.neigh(int(base["pass_slot"][0]), [victim])
    case.gdesc[victim, 1029] = np.nan
    want = both_forms(ext, ref, case.arrays(), "NaN row")
    assert np.isnan(want["score"][victim]) and victim not in want["pass_slot"] and want["n_pass"] == base["n_pass"] - 1


def test_row_appended_on_the_stream(ext, ref):
    """the caller's per-keyframe upload: the new row by an asynchronous copy, the detection behind it on the same stream"""
    import torch
    c = lc.generated(700, 500, 4096).arrays()
    a, d = upload(c)
    n, dim = a["gdesc"].shape
    cur = int(c["cur_slot"])
    table = d["gdesc"].view(torch.float32).view(n, dim)
    table[cur].zero_()
    row = torch.from_numpy(a["gdesc"][cur].copy()).pin_memory()
    d_out = torch.full((ext.loopdet_out_bytes(n),), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        table[cur].copy_(row, non_blocking=True)
        call_device(ext, c, a, d, d_out, stream=stream.cuda_stream)
    stream.synchronize()
    same(d_out.cpu().numpy(), loopdet_ref.detect(ref, c), "appended row")


def test_five_queries_through_the_walk(ext, ref):
    """slots 0 .. 34 are the map, 35 .. 39 arrive one after the other and look at the place of slots 10 .. 14: the candidates of the
    device block, walked by loopdet_walk, are mvpEnoughConsistentCandidates of the reference's statement and its walk"""
    n, first = 40, 35
    world = lc.Case(800, n, cur=first)
    for s in range(first, n):
        world.gdesc[s] = world.gdesc[first]                                     # the same view five times
    world.scores({10: 0.5, 11: 0.7, 12: 0.8, 13: 0.6, 14: 0.45, 20: 0.3})
    conn = {s: set(t for t in (s - 2, s - 1, s + 1, s + 2) if 0 <= t < n) for s in range(n)}
    for s in range(n):
        world.neigh(s, sorted(conn[s]))
    world.in_db[first:] = 0
    walk, got, queries = loopdet_walk.ConsistencyWalk(3), [], []
    for cur in range(first, n):
        c = dict(world.arrays(), cur_slot=np.int32(cur), connected=np.array(sorted(conn[cur]), np.int32),
                 covisible=np.array(sorted(conn[cur], reverse=True), np.int32))
        want = both_forms(ext, ref, c, "query %d" % cur)
        g = X.SPExtractor.decode_loopdet_out(run_record(ext, c), n)
        got.append(walk.step(g["cand_slot"], lambda s: conn[s]))
        queries.append((tlr.statement(c)["cand_slot"], conn))
        assert g["cand_slot"].tolist() == queries[-1][0] == want["cand_slot"].tolist() and len(queries[-1][0]) >= 1
        world.in_db[cur] = 1                                                    # db_frames.push_back(mpCurrentKF)
    assert got == tlr.transcription(queries, 3)
    assert got[:3] == [[], [], []] and got[3] == got[4] and 12 in got[4]


def test_refusals(ext):
    import torch
    c = lc.generated(900, 20).arrays()
    a, d = upload(c)
    n, dim = a["gdesc"].shape
    d_out = torch.full((ext.loopdet_out_bytes(n),), FILL, dtype=torch.uint8, device="cuda")
    P = {k: v.data_ptr() for k, v in d.items()}

    def args(**over):
        v = dict(d_gdesc=P["gdesc"], dim=dim, d_kf_flags=P["kf_flags"], d_in_db=P["in_db"], d_best_cov=P["best_cov"], n_slots=n,
                 cur_slot=int(c["cur_slot"]), d_connected=P["connected"], n_conn=len(a["connected"]), d_covisible=P["covisible"],
                 n_cov=len(a["covisible"]), d_out=d_out.data_ptr())
        v.update(over)
        return v
    bad = [dict(n_slots=0), dict(n_slots=X.LOOPDET_MAX_KEYFRAMES + 1), dict(dim=0), dict(dim=2), dict(dim=6), dict(dim=-4),
           dict(dim=X.GLOBAL_DESC_DIM + 4), dict(cur_slot=-1), dict(cur_slot=n), dict(n_conn=-1), dict(n_conn=n + 1), dict(n_cov=-1),
           dict(n_cov=n + 1), dict(d_gdesc=None), dict(d_kf_flags=None), dict(d_in_db=None), dict(d_best_cov=None), dict(d_out=None),
           dict(d_connected=None), dict(d_covisible=None), dict(d_gdesc=P["gdesc"] + 4), dict(d_out=d_out.data_ptr() + 1)]
    for over in bad:
        with pytest.raises(SpfeError):
            ext.detect_loop_candidates_device(**args(**over))
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == FILL).all(), "a refused call wrote"
    ext.detect_loop_candidates_device(**args(d_connected=None, n_conn=0, d_covisible=None, n_cov=0))     # null lists of no entries
    torch.cuda.synchronize()
    assert X.SPExtractor.decode_loopdet_out(d_out.cpu().numpy(), n)["n_scored"] > 0
    # the host form
    out = np.full(ext.loopdet_out_bytes(n), FILL, np.uint8)
    for over in (dict(cur_slot=n), dict(cur_slot=-1)):
        with pytest.raises(SpfeError):
            ext.detect_loop_candidates(a["gdesc"], a["kf_flags"], a["in_db"], a["best_cov"], over["cur_slot"], a["connected"],
                                       a["covisible"], out=out)
    with pytest.raises(SpfeError):
        ext.detect_loop_candidates(a["gdesc"][:, :6], a["kf_flags"], a["in_db"], a["best_cov"], 0, a["connected"], a["covisible"], out=out)
    with pytest.raises(SpfeError):
        ext.detect_loop_candidates(a["gdesc"], a["kf_flags"], a["in_db"], a["best_cov"], 0, np.zeros(n + 1, np.int32), a["covisible"],
                                   out=out)
    assert (out == FILL).all()
