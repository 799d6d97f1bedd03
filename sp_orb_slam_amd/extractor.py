"""Host-side mirror of the reference extractor interface over the C ABI.

`SPExtractor` keeps the call shape of the reference class
(/root/reference/orb_slam2/include/orb_slam/cv/sp_extractor.h:49-88):
construct once with the number of features, call it with a CV_8UC1 image and an
(ignored) mask, get keypoints + a K x 256 float32 descriptor matrix, then read
the side outputs the tracker copies right after the call
(/root/reference/orb_slam2/src/type/frame.cpp:296-314): getCov2Inv(),
dense_dust_, heat_, occ_grid_.  Everything is computed by libspfe.so
(hand-written HIP for gfx950); there is NO CPU path: importing works anywhere,
constructing an extractor without the library or without a GPU raises.
"""
import ctypes as C
import os
import threading

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libspfe.so")

SPFE_FLAG_HEAT = 1
SPFE_FLAG_ASYNC_COV = 2
SPFE_FLAG_DESC_BF16 = 4   # records / results carry bf16 descriptors (RNE of the f32 ones)
SPFE_FLAG_LAZY_HEAT_INV = 8   # with SPFE_FLAG_HEAT: host calls bring back `heat` only; fetch_heat_inv() on demand
SPFE_PRECISION_F32 = 0
SPFE_PRECISION_BF16 = 1
NUM_PARAMS = 1300865
ABI_VERSION = 5           # SPFE_ABI_VERSION of include/spfe.h these ctypes structures mirror
_ERRORS = {-1: "SPFE_EINVAL", -2: "SPFE_EEMPTY", -3: "SPFE_EHIP", -4: "SPFE_EWEIGHTS"}

class SpfeError(RuntimeError):
    pass


class _Config(C.Structure):
    _fields_ = [("height", C.c_int), ("width", C.c_int), ("num_features", C.c_int),
                ("max_batch", C.c_int), ("device", C.c_int), ("precision", C.c_int),
                ("flags", C.c_uint), ("weights", C.c_void_p), ("weights_path", C.c_char_p)]


class _Result(C.Structure):
    _fields_ = [("K", C.c_int), ("n_candidates", C.c_int), ("status", C.c_int),
                ("reserved", C.c_int), ("kp_xy", C.c_void_p),
                ("kp_response", C.c_void_p), ("desc", C.c_void_p), ("cov2", C.c_void_p),
                ("cov2_inv", C.c_void_p), ("occ_grid", C.c_void_p), ("dense_dust", C.c_void_p),
                ("semi_dust", C.c_void_p), ("heat", C.c_void_p), ("heat_inv", C.c_void_p),
                ("desc_bf16", C.c_void_p)]


class RecordLayout(C.Structure):
    _fields_ = [("bytes", C.c_size_t), ("kmax", C.c_int), ("off_hdr", C.c_size_t),
                ("off_xy", C.c_size_t), ("off_resp", C.c_size_t), ("off_cov", C.c_size_t),
                ("off_cinv", C.c_size_t), ("off_desc", C.c_size_t), ("off_occ", C.c_size_t),
                ("off_dd", C.c_size_t), ("off_sd", C.c_size_t), ("desc_elem_bytes", C.c_int)]


class _DustParams(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("max_iterations", C.c_int), ("huber_delta", C.c_double), ("inlier_chi2", C.c_double)]


DUST_MAX_POINTS = 512
DUST_OFF_UV = 128
DUST_OFF_INLIER = 128 + DUST_MAX_POINTS * 8
DUST_OUT_BYTES = 128 + DUST_MAX_POINTS * 9


class _PoseParams(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("schedule", C.c_int),
                ("iterations", C.c_int)]


POSE_DUST_POST = 0          # SPFE_POSE_DUST_POST: Optimizer::PoseOptimizationDustPost
POSE_OPTIMIZATION = 1       # SPFE_POSE_OPTIMIZATION: Optimizer::PoseOptimization (monocular)
POSE_OFF_OUTLIER = 128
POSE_STATUS_COV_OVERFLOW = 1
TRACK_OK, TRACK_FAIL_INLIERS, TRACK_FAIL_MATCHES, TRACK_FAIL_RATIO, TRACK_FAIL_COV = 0, 1, 2, 3, 4
TRACK_FAIL_LOCAL_INLIERS = 5   # SPFE_TRACK_FAIL_LOCAL_INLIERS: TrackLocalMap's mnMatchesInliers < th_ninlier
POSE_OFF_N_INLIERS = 64 + 36
TRACK_FAIL_MOTION_INLIERS = 6  # SPFE_TRACK_FAIL_MOTION_INLIERS: TrackWithMotionModel's nmatchesMap < th_nmatch_opt
TRACK_FAIL_REFKF_INLIERS = 7   # SPFE_TRACK_FAIL_REFKF_INLIERS: trackReferenceKeyFrameANN's nmatchesMap < th_nmatch_opt
POSE_OFF_WIDENED = 64 + 40     # the motion-model chain: the search with the doubled window stands
POSE_OFF_N_OUTLIERS = 64 + 44  # the motion-model and reference-keyframe chains: keypoints the discard loop emptied


class _ProjParams(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("mode", C.c_int),
                ("th", C.c_float), ("th_dist", C.c_float), ("view_cos_limit", C.c_float), ("adaptive", C.c_int),
                ("c2_thresh", C.c_float)]


PROJ_LOCAL_MAP, PROJ_LAST_FRAME = 0, 1      # SPFE_PROJ_LOCAL_MAP / SPFE_PROJ_LAST_FRAME
PROJ_SEARCHABLE, PROJ_OBSERVED = 1, 2       # map point flags
PROJ_MAX_POINTS = 8192
PROJ_MAX_RADIUS = 32
PROJ_MAX_CELLS_AXIS = 2 * PROJ_MAX_RADIUS // 8 + 3
PROJ_MAX_CAND = PROJ_MAX_CELLS_AXIS ** 2
PROJ_OFF_KP = 64
PROJ_OFF_UV = PROJ_OFF_KP + PROJ_MAX_POINTS * 4
PROJ_OFF_COS = PROJ_OFF_UV + PROJ_MAX_POINTS * 8
PROJ_OFF_VIEW = PROJ_OFF_COS + PROJ_MAX_POINTS * 4
PROJ_OUT_BYTES = (PROJ_OFF_VIEW + PROJ_MAX_POINTS + 255) // 256 * 256


class _TriParams(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("fx1", "fy1", "cx1", "cy1", "fx2", "fy2", "cx2", "cy2", "ratio", "epipole_r2")] + \
        [(n, C.c_double) for n in ("chi2_line", "chi2_reproj", "cos_parallax_max", "min_baseline_depth_ratio")]


TRI_MAX_NEIGHBOURS = 32
TRI_NONE, TRI_NEW, TRI_PARALLAX, TRI_DEGENERATE, TRI_DEPTH, TRI_REPROJ = range(6)   # SPFE_TRI_VERDICT_*
TRI_STATUS_COV_OVERFLOW = 1
# the int32 fields of the output block, in the order of their SPFE_TRI_OFF_* offsets (4 bytes apart from 0)
TRI_FIELDS = ("n_matches", "n_new", "n_rej_parallax", "n_rej_depth", "n_rej_reproj", "n_rej_degenerate", "skipped", "status",
              "point_base")
TRI_OFF_MATCH12 = 64


def tri_offsets(kmax):
    """SPFE_TRI_OFF_VERDICT / NEW_XYZ / NEW_K1 / NEW_K2 (kmax) and SPFE_TRI_OUT_BYTES(kmax)"""
    return dict(verdict=64 + 4 * kmax, new_xyz=64 + 8 * kmax, new_k1=64 + 20 * kmax, new_k2=64 + 24 * kmax,
                out_bytes=(64 + 28 * kmax + 255) // 256 * 256)


class _FuseParams(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "th", "th_dist")] + \
        [("chi2", C.c_double), ("view_cos", C.c_double), ("min_factor", C.c_float), ("max_factor", C.c_float)]


FUSE_MAX_TARGETS = 128
# SPFE_FUSE_*: the reason codes of reason[i]
(FUSE_SKIP_BAD, FUSE_SKIP_IN_KF, FUSE_BEHIND, FUSE_OUTSIDE, FUSE_RANGE, FUSE_ANGLE, FUSE_NO_CANDIDATE, FUSE_TOO_FAR,
 FUSE_PROPOSED) = range(1, 10)
FUSE_REASONS = ("skip_bad", "skip_in_kf", "behind", "outside", "range", "angle", "no_candidate", "too_far", "proposed")
FUSE_FIELDS = ("n_fused", "n", "status")   # the int32 fields of the output block, 4 bytes apart from 0
FUSE_OFF_KP_OF_MP = 64


def fuse_offsets(cap):
    """SPFE_FUSE_OFF_BEST_DIST / HOLDER / FUSED_IDX / REASON (cap) and SPFE_FUSE_OUT_BYTES(cap)"""
    return dict(best_dist=64 + 4 * cap, holder=64 + 8 * cap, fused_idx=64 + 12 * cap, reason=64 + 16 * cap,
                out_bytes=(64 + 17 * cap + 255) // 256 * 256)


class _LoopFuseParams(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "th", "th_dist")] + \
        [("view_cos", C.c_double), ("min_factor", C.c_float), ("max_factor", C.c_float)]


LOOPFUSE_STRIP = 64   # SPFE_LOOPFUSE_STRIP: a search workgroup serves one target and this many consecutive points


class _Sim3Params(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("fx1", "fy1", "cx1", "cy1", "fx2", "fy2", "cx2", "cy2", "max_err1", "max_err2")] + \
        [("min_inliers", C.c_int), ("fix_scale", C.c_int)]


SIM3_MAX_CANDIDATES = 16
SIM3_MAX_HYPOTHESES = 512
SIM3_FIELDS = ("N", "n_returns", "best_h", "best_count", "n_hyp")   # the int32 fields of the output block, 4 bytes apart from 0
SIM3_OFF_K1 = 64


def sim3_offsets(kmax, hyp_cap):
    """SPFE_SIM3_OFF_COUNT / RETURN_IDX / T12 / INLIERS, SPFE_SIM3_WORDS(kmax) and SPFE_SIM3_OUT_BYTES(kmax, hyp_cap)"""
    words = (kmax + 63) // 64
    inl = (64 + 4 * kmax + 60 * hyp_cap + 7) // 8 * 8
    return dict(k1=SIM3_OFF_K1, count=64 + 4 * kmax, return_idx=64 + 4 * kmax + 4 * hyp_cap, T12=64 + 4 * kmax + 8 * hyp_cap,
                inliers=inl, words=words, out_bytes=(inl + 8 * hyp_cap * words + 255) // 256 * 256)


class _GuidedParams(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("fx1", "fy1", "cx1", "cy1", "fx2", "fy2", "cx2", "cy2", "th", "th_dist", "min_factor",
                                         "max_factor")]


GUIDED_MAX_JOBS = 32
# SPFE_GUIDED_*: the reason codes of reason1[i1] / reason2[i2]
(GUIDED_NO_POINT, GUIDED_ALREADY, GUIDED_SKIP_BAD, GUIDED_BEHIND, GUIDED_OUTSIDE, GUIDED_RANGE, GUIDED_NO_CANDIDATE,
 GUIDED_TOO_FAR, GUIDED_MATCHED) = range(1, 10)
GUIDED_REASONS = ("no_point", "already", "skip_bad", "behind", "outside", "range", "no_candidate", "too_far", "matched")
GUIDED_FIELDS = ("n_found", "n_total", "n_seed", "status")   # the int32 fields of the output block, 4 bytes apart from 0
GUIDED_OFF_MATCH1 = 64
GUIDED_STATUS_NOT_EVALUATED = 0x100


def guided_offsets(kmax):
    """SPFE_GUIDED_OFF_MATCH2 / DIST1 / DIST2 / MATCHES12 / REASON1 / REASON2 (kmax) and SPFE_GUIDED_OUT_BYTES(kmax)"""
    return dict(match1=GUIDED_OFF_MATCH1, match2=64 + 4 * kmax, dist1=64 + 8 * kmax, dist2=64 + 12 * kmax, matches12=64 + 16 * kmax,
                reason1=64 + 20 * kmax, reason2=64 + 21 * kmax, out_bytes=(64 + 22 * kmax + 255) // 256 * 256)


class _LoopProjParams(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "th", "th_dist")] + \
        [("view_cos", C.c_double), ("min_factor", C.c_float), ("max_factor", C.c_float)]


# SPFE_LOOPPROJ_*: the reason codes of the loop-point search
(LOOPPROJ_SKIP_BAD, LOOPPROJ_ALREADY_FOUND, LOOPPROJ_BEHIND, LOOPPROJ_OUTSIDE, LOOPPROJ_RANGE, LOOPPROJ_ANGLE, LOOPPROJ_NO_CANDIDATE,
 LOOPPROJ_TOO_FAR, LOOPPROJ_MATCHED) = range(1, 10)
LOOPPROJ_REASONS = ("skip_bad", "already_found", "behind", "outside", "range", "angle", "no_candidate", "too_far", "matched")
LOOPPROJ_FIELDS = ("n_matched", "n", "status")   # the int32 fields of the output block, 4 bytes apart from 0
LOOPPROJ_OFF_KP_OF_MP = 64


def loop_proj_offsets(cap):
    """SPFE_LOOPPROJ_OFF_BEST_DIST / MATCHED_IDX / REASON (cap) and SPFE_LOOPPROJ_OUT_BYTES(cap)"""
    return dict(best_dist=64 + 4 * cap, matched_idx=64 + 8 * cap, reason=64 + 12 * cap, out_bytes=(64 + 13 * cap + 255) // 256 * 256)


class _Sim3OptParams(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("fx1", "fy1", "cx1", "cy1", "fx2", "fy2", "cx2", "cy2", "th2")] + \
        [(n, C.c_int) for n in ("fix_scale", "iterations", "min_kept", "min_inliers")]


# SPFE_SIM3OPT_*: verdict[k1] of the Sim3 optimisation
(SIM3OPT_NONE, SIM3OPT_SKIPPED, SIM3OPT_REMOVED, SIM3OPT_OUTLIER, SIM3OPT_INLIER, SIM3OPT_KEPT) = range(6)
SIM3OPT_VERDICTS = ("none", "skipped", "removed", "outlier", "inlier", "kept")
# the int32 fields of the output block, 4 bytes apart from 0 (iterations and trials are pairs)
SIM3OPT_FIELDS = ("n_corr", "n_bad", "n_in", "accepted", "iterations0", "iterations1", "trials0", "trials1", "status")
SIM3OPT_OFF_S12, SIM3OPT_OFF_T12, SIM3OPT_OFF_SCW, SIM3OPT_OFF_MATCHES12 = 64, 168, 224, 320
SIM3OPT_STATUS_NOT_EVALUATED = 0x100


def sim3opt_offsets(kmax):
    """SPFE_SIM3OPT_OFF_MATCHED / VERDICT (kmax) and SPFE_SIM3OPT_OUT_BYTES(kmax)"""
    return dict(S12=SIM3OPT_OFF_S12, T12=SIM3OPT_OFF_T12, Scw=SIM3OPT_OFF_SCW, matches12=SIM3OPT_OFF_MATCHES12,
                matched=320 + 4 * kmax, verdict=320 + 8 * kmax, out_bytes=(320 + 9 * kmax + 255) // 256 * 256)


class BaParams(C.Structure):
    """spfe_ba_params"""
    _fields_ = [(n, C.c_float) for n in ("fx", "fy", "cx", "cy")] + [("schedule", C.c_int), ("iterations", C.c_int * 2),
                                                                      ("robust", C.c_int), ("inv_sigma2", C.c_float)]


# SPFE_BA_*: limits, schedules, verdict[e], status bits
BA_MAX_KEYFRAMES, BA_MAX_FREE, BA_MAX_POINTS, BA_MAX_EDGES = 128, 64, 16384, 131072
BA_LOCAL, BA_FULL = 0, 1
(BA_SKIPPED, BA_INLIER, BA_LEVEL1_KEPT, BA_ERASE) = range(4)
BA_VERDICTS = ("skipped", "inlier", "level1_kept", "erase")
BA_STATUS_UNSORTED, BA_STATUS_COV_OVERFLOW, BA_STATUS_STOPPED_EARLY, BA_STATUS_STOPPED, BA_STATUS_TOO_MANY_FREE = \
    0x100, 0x200, 0x400, 0x800, 0x1000
# the int32 fields of the output block, 4 bytes apart from 0 (iterations and trials are pairs)
BA_FIELDS = ("n_kf", "n_free", "n_points", "n_edges", "n_served", "iterations0", "iterations1", "trials0", "trials1", "n_level1",
             "n_erase", "status")


def ba_offsets(n_kf, n, E):
    """SPFE_BA_OFF_* and SPFE_BA_OUT_BYTES(n_kf, n, E)"""
    verdict = 128 + 64 * n_kf + 12 * n
    erase = verdict + (E + 3) // 4 * 4
    return dict(iterations=20, trials=28, n_level1=36, n_erase=40, status=44, chi2=64, tcw=128, xyz=128 + 64 * n_kf,
                verdict=verdict, erase=erase, bytes=(erase + 4 * E + 255) // 256 * 256, **{"lambda": 80})


class MpParams(C.Structure):
    """spfe_mp_params"""
    _fields_ = [("mode", C.c_int), ("level_scale", C.c_float), ("top_scale", C.c_float)]


# SPFE_MP_*: limits, mode bits, code[i], scheduling constants
MP_MAX_POINTS, MP_MAX_EDGES, MP_MAX_OBS = 262144, 4194304, 256
MP_DESC, MP_NORMAL_DEPTH = 1, 2
(MP_SKIP_BAD, MP_NO_OBS, MP_INVALID, MP_NO_GOOD_KF, MP_TOO_MANY, MP_REFRESHED) = range(1, 7)
MP_CODES = ("skip_bad", "no_obs", "invalid", "no_good_kf", "too_many", "refreshed")
MP_CHUNK, MP_WAVE_OBS = 16, 16
MP_FIELDS = ("m", "n_desc_written", "n_nd_written", "status")   # the int32 fields of the output block, 4 bytes apart from 0


def mp_offsets(m):
    """SPFE_MP_OFF_* and SPFE_MP_OUT_BYTES(m)"""
    return dict(best_obs=16, n_good=16 + 4 * m, best_median=16 + 8 * m, code=16 + 12 * m, out_bytes=(16 + 13 * m + 255) // 256 * 256)


class EssGraphParams(C.Structure):
    """spfe_essgraph_params"""
    _fields_ = [("iterations", C.c_int), ("fix_scale", C.c_int), ("lambda_init", C.c_double)]


# SPFE_ESSGRAPH_*: limits, statuses; SPFE_EGC_*: the codes of the map-point correction
ESSGRAPH_MAX_KEYFRAMES, ESSGRAPH_MAX_EDGES, ESSGRAPH_MAX_BLOCKS = 16384, 262144, 786432
ESSGRAPH_OK, ESSGRAPH_EMPTY, ESSGRAPH_ENVELOPE_OVERFLOW = 0, 1, 2
ESSGRAPH_FIELDS = ("status", "n_unknown", "n_edges_followed", "n_skipped", "env_blocks", "iterations", "trials", "n_solve_failed")
EGC_SKIP_BAD, EGC_INVALID, EGC_CORRECTED = 1, 2, 3


def essgraph_offsets(n):
    """SPFE_ESSGRAPH_OFF_* and SPFE_ESSGRAPH_OUT_BYTES(n)"""
    return dict(chi2=32, sim3=64, tiw=64 + 64 * n, out_bytes=(64 + 128 * n + 255) // 256 * 256)


class LoopdetParams(C.Structure):
    """spfe_loopdet_params"""
    _fields_ = [("min_score_init", C.c_float), ("min_score_floor", C.c_float), ("retain_ratio", C.c_float)]


# SPFE_LOOPDET_*: limits, role bits, status bits, the bits of a score that was not formed
LOOPDET_NEIGH, LOOPDET_MAX_KEYFRAMES, GLOBAL_DESC_DIM = 10, 65536, 4096
LOOPDET_ROLE_DB, LOOPDET_ROLE_COV = 1, 2
LOOPDET_BAD_LIST_INDEX, LOOPDET_BAD_NEIGHBOUR = 1, 2
LOOPDET_NO_SCORE_BITS = 0x7FC00000
LOOPDET_FIELDS = ("status", "n_scored", "n_pass", "n_cand")   # the int32 fields of the output block, 4 bytes apart from 0
LOOPDET_SCORES = ("cov_min_score", "min_score", "best_acc_score", "min_score_to_retain")   # the f32 fields behind them


def loopdet_offsets(n):
    """SPFE_LOOPDET_OFF_* and SPFE_LOOPDET_OUT_BYTES(n)"""
    return dict(score=32, pass_slot=32 + 4 * n, acc_score=32 + 8 * n, best_slot=32 + 12 * n, cand_slot=32 + 16 * n,
                cand_acc=32 + 20 * n, first_pos=32 + 24 * n, role=32 + 28 * n, out_bytes=(32 + 29 * n + 255) // 256 * 256)


class LocalmapParams(C.Structure):
    """spfe_localmap_params"""
    _fields_ = [("max_keyframes", C.c_int), ("point_cap", C.c_int)]


# SPFE_LOCALMAP_*: limits, status bits, the int32 fields of the block's header (4 bytes apart from 0)
LOCALMAP_MAX_KEYFRAMES, LOCALMAP_MAX_STRIDE, LOCALMAP_MAX_BEST, LOCALMAP_MAX_WEIGHT = 65536, 16384, 32, 127
LOCALMAP_NO_VOTES, LOCALMAP_TRUNCATED, LOCALMAP_BAD_SLOT = 1, 2, 4
LOCALMAP_FIELDS = ("n_voted", "n_local_kf", "ref_slot", "n_held", "n_points", "n_points_total", "status")


def localmap_offsets(n_slots, point_cap, n_kp):
    """SPFE_LOCALMAP_OFF_* and SPFE_LOCALMAP_OUT_BYTES(n_slots, point_cap, n_kp)"""
    s, p, k = int(n_slots), int(point_cap), int(n_kp)
    return dict(local_kf=32, votes=32 + 4 * s, total=32 + 8 * s, point_idx=32 + 12 * s, mp_of_kp_list=32 + 12 * s + 4 * p,
                out_bytes=(32 + 12 * s + 4 * p + 4 * k + 255) // 256 * 256)


class CovisGraph(C.Structure):
    """spfe_covis_graph: the eight state arrays (device pointers, or host pointers in spfe_update_connections), n_slots, conn_cap"""
    _fields_ = [("d_conn_slot", C.c_void_p), ("d_conn_w", C.c_void_p), ("d_conn_n", C.c_void_p), ("d_ord_slot", C.c_void_p),
                ("d_ord_w", C.c_void_p), ("d_ord_n", C.c_void_p), ("d_parent", C.c_void_p), ("d_first_conn", C.c_void_p),
                ("n_slots", C.c_int), ("conn_cap", C.c_int)]


class CovisParams(C.Structure):
    """spfe_covis_params"""
    _fields_ = [("th", C.c_int), ("origin_slot", C.c_int)]


# SPFE_COVIS_*: the limit, status bits, the codes of a linked neighbour, the int32 fields of the block's header (4 bytes apart from 0),
# the state arrays in the order of spfe_covis_graph
COVIS_MAX_CONN = 4096
COVIS_NO_SHARED, COVIS_CUR_OVERFLOW, COVIS_NEIGH_OVERFLOW = 1, 2, 4
COVIS_CODE_SAME, COVIS_CODE_REPLACED, COVIS_CODE_INSERTED, COVIS_CODE_FULL = 0, 1, 2, 3
COVIS_FIELDS = ("status", "n_counter", "n_linked", "n_changed", "n_overflow", "max_slot", "max_count", "parent_set")
COVIS_STATE = ("conn_slot", "conn_w", "conn_n", "ord_slot", "ord_w", "ord_n", "parent", "first_conn")


def covis_offsets(n_slots, conn_cap):
    """SPFE_COVIS_OFF_* and SPFE_COVIS_OUT_BYTES(n_slots, conn_cap)"""
    s, c = int(n_slots), int(conn_cap)
    return dict(counter=32, linked_slot=32 + 4 * s, linked_code=32 + 4 * s + 4 * c, out_bytes=(32 + 4 * s + 8 * c + 255) // 256 * 256)


def covis_graph(ptrs, n_slots, conn_cap):
    """spfe_covis_graph from the eight pointers (ints, None = null) in the order of COVIS_STATE, or a dict by those names"""
    if isinstance(ptrs, dict):
        ptrs = [ptrs[k] for k in COVIS_STATE]
    assert len(ptrs) == 8
    return CovisGraph(*[C.c_void_p(p or 0) for p in ptrs], int(n_slots), int(conn_cap))


class CullParams(C.Structure):
    """spfe_cull_params"""
    _fields_ = [("th_obs", C.c_int), ("cov_ratio", C.c_float), ("origin_slot", C.c_int), ("bad_cap", C.c_int)]


# SPFE_KF_* and SPFE_CULL_*: the flag bits of d_kf_flags, the status bits, the codes of a list entry, the int32 fields of the block's
# header (4 bytes apart from 0)
KF_BAD, KF_NOT_ERASE, KF_TO_BE_ERASED = 1, 2, 4
CULL_STALLED, CULL_WILD_ENTRY, CULL_BAD_CUT, CULL_EVENT_CUT, CULL_NO_PARENT = 1, 2, 4, 8, 16
(CULL_CODE_DROPPED, CULL_CODE_CULLED, CULL_CODE_DEFERRED, CULL_CODE_STALLED, CULL_CODE_ORIGIN, CULL_CODE_WILD,
 CULL_CODE_BAD) = range(7)
CULL_FIELDS = ("status", "n_listed", "n_passes", "n_culled", "n_deferred", "n_touched", "n_reparented", "n_events", "n_bad",
               "n_bad_stored")


def cull_offsets(n_slots, conn_cap, bad_cap):
    """SPFE_CULL_OFF_* and SPFE_CULL_OUT_BYTES(n_slots, conn_cap, bad_cap)"""
    s, c, b = int(n_slots), int(conn_cap), int(bad_cap)
    return dict(entry_slot=64, entry_code=64 + 4 * c, entry_pass=64 + 8 * c, entry_mps=64 + 12 * c, entry_red=64 + 16 * c,
                culled_slot=64 + 20 * c, touched_slot=64 + 24 * c, event_child=64 + 24 * c + 4 * s, event_parent=64 + 24 * c + 8 * s,
                bad_point=64 + 24 * c + 12 * s, out_bytes=(64 + 24 * c + 12 * s + 4 * b + 255) // 256 * 256)


class MpLife(C.Structure):
    """spfe_mp_life: the seven state arrays of map-point culling (device pointers, or host pointers in the host-array forms),
    n_table, recent_cap"""
    _fields_ = [("d_mp_flags", C.c_void_p), ("d_mp_nobs", C.c_void_p), ("d_mp_found", C.c_void_p), ("d_mp_visible", C.c_void_p),
                ("d_mp_first_kf", C.c_void_p), ("d_recent", C.c_void_p), ("d_recent_n", C.c_void_p), ("n_table", C.c_int),
                ("recent_cap", C.c_int)]


class MpCullParams(C.Structure):
    """spfe_mpcull_params"""
    _fields_ = [("cur_kf_id", C.c_int), ("th_obs", C.c_int), ("found_ratio", C.c_float), ("bad_cap", C.c_int)]


# SPFE_ADMIT_*, SPFE_MPSTAT_*, SPFE_MPCULL_*: status bits, the codes of a list entry, the int32 fields of the blocks' headers (4 bytes
# apart from 0), the state arrays in the order of spfe_mp_life
MP_LIFE_STATE = ("flags", "nobs", "found", "visible", "first_kf", "recent", "recent_n")
ADMIT_RECENT_OVERFLOW, ADMIT_BAD_RANGE, ADMIT_DISPLACED = 1, 2, 4
ADMIT_FIELDS = ("status", "n_admitted", "n_recent_before", "n_recent_after", "n_displaced", "n_needed")
ADMIT_OFF_ADMITTED, ADMIT_OUT_BYTES = 32, 256
MPSTAT_FIELDS = ("n_visible_held", "n_visible_view", "n_found")
MPSTAT_OUT_BYTES = 256
MPCULL_BAD_CUT, MPCULL_WILD_ENTRY = 1, 2
(MPCULL_CODE_KEPT, MPCULL_CODE_CULLED_RATIO, MPCULL_CODE_CULLED_OBS, MPCULL_CODE_RETIRED, MPCULL_CODE_ERASED_BAD,
 MPCULL_CODE_WILD) = range(6)
MPCULL_FIELDS = ("status", "n_listed", "n_kept", "n_culled_ratio", "n_culled_obs", "n_retired", "n_erased_bad", "n_wild", "n_bad",
                 "n_bad_stored")


def mpcull_offsets(recent_cap, bad_cap):
    """SPFE_MPCULL_OFF_* and SPFE_MPCULL_OUT_BYTES(recent_cap, bad_cap)"""
    r, b = int(recent_cap), int(bad_cap)
    return dict(entry_point=64, entry_code=64 + 4 * r, bad_point=64 + 8 * r, out_bytes=(64 + 8 * r + 4 * b + 255) // 256 * 256)


def mp_life(ptrs, n_table, recent_cap):
    """spfe_mp_life from the seven pointers (ints, None = null) in the order of MP_LIFE_STATE, or a dict by those names"""
    if isinstance(ptrs, dict):
        ptrs = [ptrs.get(k) for k in MP_LIFE_STATE]
    assert len(ptrs) == 7
    return MpLife(*[C.c_void_p(p or 0) for p in ptrs], int(n_table), int(recent_cap))


# SPFE_NEWKF_*, SPFE_LISTOBS_*: status bits, the codes of a keypoint and of a list entry, the int32 fields of the blocks' headers (4
# bytes apart from 0)
NEWKF_ROW_IN_USE, NEWKF_BAD_SLOT, NEWKF_RECENT_OVERFLOW = 1, 2, 4
NEWKF_CODE_NONE, NEWKF_CODE_WILD, NEWKF_CODE_BAD_POINT, NEWKF_CODE_ADDED, NEWKF_CODE_REPEATED = range(5)
NEWKF_FIELDS = ("status", "n_none", "n_wild", "n_bad_point", "n_added", "n_repeated", "n_recent_before", "n_recent_after", "n_needed")
LISTOBS_OVERFLOW, LISTOBS_MANY = 1, 2
LISTOBS_CODE_EMPTY, LISTOBS_CODE_WILD, LISTOBS_CODE_REPEATED, LISTOBS_CODE_FIRST = range(4)
LISTOBS_FIELDS = ("status", "m", "n_first", "n_empty", "n_wild", "n_repeated", "n_obs", "n_obs_needed", "max_obs", "obs_cap")


def _pad16(v):
    return (int(v) + 15) // 16 * 16


def newkf_offsets(n_kp, kp_stride):
    """SPFE_NEWKF_OFF_* and SPFE_NEWKF_OUT_BYTES(n_kp, kp_stride)"""
    added = 64 + _pad16(4 * int(n_kp))
    return dict(code=64, added_point=added, out_bytes=(added + 4 * int(kp_stride) + 255) // 256 * 256)


def listobs_offsets(m, obs_cap):
    """SPFE_LISTOBS_OFF_* and SPFE_LISTOBS_OUT_BYTES(m, obs_cap)"""
    m = int(m)
    start = 64 + _pad16(4 * m)
    ref = start + _pad16(4 * (m + 1))
    obs = ref + _pad16(4 * m)
    return dict(point_idx=64, obs_start=start, ref_slot=ref, obs=obs, out_bytes=(obs + 8 * int(obs_cap) + 255) // 256 * 256)


class LbaGatherParams(C.Structure):
    """spfe_lba_gather_params"""
    _fields_ = [("cur_slot", C.c_int), ("origin_slot", C.c_int), ("kf_cap", C.c_int), ("free_cap", C.c_int), ("point_cap", C.c_int),
                ("edge_cap", C.c_int)]


class LbaApplyParams(C.Structure):
    """spfe_lba_apply_params"""
    _fields_ = [("kf_cap", C.c_int), ("point_cap", C.c_int), ("edge_cap", C.c_int), ("bad_cap", C.c_int)]


# SPFE_LBA_*: the status bits of the gather and of the application, the int32 fields of the two headers (4 bytes apart from 0)
LBA_LOCAL_CUT, LBA_POINT_CUT, LBA_FIXED_CUT, LBA_EDGE_OVERFLOW = 1, 2, 4, 8
LBA_NOT_APPLIED, LBA_BAD_CUT, LBA_WILD = 1, 2, 4
LBA_GATHER_FIELDS = ("status", "n_local", "n_free", "n_fixed", "n_kf", "n_points", "n_points_all", "n_obs", "n_edges", "n_obs_needed")
LBA_APPLY_FIELDS = ("status", "n_erased", "n_bad", "n_bad_stored", "n_ref_moved", "n_obs_after")


def _pad16(v):
    return (int(v) + 15) // 16 * 16


def lba_gather_offsets(kf_cap, point_cap, edge_cap):
    """SPFE_LBA_OFF_* and SPFE_LBA_GATHER_BYTES(kf_cap, point_cap, edge_cap): kf_slot, fixed, Tcw, point_idx, xyz, obs_start, obs,
    edges — fixed, Tcw, xyz and edges are where spfe_local_ba_records_device takes d_fixed, d_Tcw, d_xyz and d_edges"""
    k, p, e = int(kf_cap), int(point_cap), int(edge_cap)
    o = dict(kf_slot=64)
    o["fixed"] = 64 + _pad16(4 * k)
    o["Tcw"] = o["fixed"] + _pad16(k)
    o["point_idx"] = o["Tcw"] + 64 * k
    o["xyz"] = o["point_idx"] + _pad16(4 * p)
    o["obs_start"] = o["xyz"] + _pad16(12 * p)
    o["obs"] = o["obs_start"] + _pad16(4 * (p + 1))
    o["edges"] = o["obs"] + _pad16(8 * e)
    o["out_bytes"] = (o["edges"] + 12 * e + 255) // 256 * 256
    return o


def lba_apply_offsets(point_cap, edge_cap, bad_cap):
    """SPFE_LBA_APPLY_OFF_* and SPFE_LBA_APPLY_BYTES(point_cap, edge_cap, bad_cap): bad_point, and obs_start / obs / ref_slot where
    spfe_refresh_map_points_device takes d_obs_start, d_obs and d_ref_slot"""
    p, e, b = int(point_cap), int(edge_cap), int(bad_cap)
    o = dict(bad_point=64)
    o["obs_start"] = 64 + _pad16(4 * b)
    o["obs"] = o["obs_start"] + _pad16(4 * (p + 1))
    o["ref_slot"] = o["obs"] + _pad16(8 * e)
    o["out_bytes"] = (o["ref_slot"] + 4 * p + 255) // 256 * 256
    return o


class _Staging(C.Structure):
    _fields_ = [("src_height", C.c_int), ("src_width", C.c_int), ("channels", C.c_int), ("rgb", C.c_int),
                ("map_x", C.c_void_p), ("map_y", C.c_void_p)]


# The C ABI: name -> (restype, argtypes), in the order and the groups of include/spfe.h.  load_library() applies it;
# tests/test_abi.py checks it against the header's declarations.
_vp, _int, _long, _size, _float, _str, _P = C.c_void_p, C.c_int, C.c_long, C.c_size_t, C.c_float, C.c_char_p, C.POINTER
_SIGNATURES = {
    # the extractor and its synchronous host calls
    "spfe_create": (_int, [_P(_Config), _P(_vp)]),
    "spfe_destroy": (None, [_vp]),
    "spfe_extract": (_int, [_vp, _vp, _int, _P(_Result)]),
    "spfe_extract_batch": (_int, [_vp, _P(_vp), _int, _int, _P(_Result)]),
    "spfe_extract_begin": (_int, [_vp, _P(_vp), _int, _int]),
    "spfe_extract_maps": (_int, [_vp, _P(_P(_float)), _P(_P(_float))]),
    "spfe_extract_rows": (_int, [_vp, _int, _P(_int), _P(_P(_float))]),
    "spfe_extract_finish": (_int, [_vp, _P(_Result)]),
    # pipelined host path
    "spfe_submit_batch": (_int, [_vp, _P(_vp), _int, _int, _P(_long)]),
    "spfe_collect_batch": (_int, [_vp, _long, _P(_Result)]),
    "spfe_postprocess": (_int, [_vp, _vp, _vp, _int, _P(_Result)]),
    # device-resident batch path
    "spfe_get_record_layout": (_int, [_vp, _P(RecordLayout)]),
    "spfe_record_bytes": (_size, [_vp]),
    "spfe_extract_batch_device": (_int, [_vp, _vp, _int, _vp, _vp]),
    "spfe_last_ticket": (_long, [_vp]),
    "spfe_wait_records": (_int, [_vp, _long, _vp]),
    # multi-GPU: all-gather of the records
    "spfe_comm_unique_id": (_int, [_vp, _size]),
    "spfe_comm_init": (_int, [_vp, _vp, _int, _int]),
    "spfe_comm_destroy": (_int, [_vp]),
    "spfe_allgather_records": (_int, [_vp, _long, _vp, _vp, _int]),
    "spfe_comm_wait": (_int, [_vp, _vp]),
    "spfe_comm_stream": (_vp, [_vp]),
    "spfe_comm_count": (_int, [_vp, _P(_int)]),
    "spfe_view_record": (_int, [_vp, _vp, _P(_Result)]),
    "spfe_debug_read": (_long, [_vp, _str, _int, _vp, _size]),
    # descriptor matching and patch-wise association
    "spfe_match": (_int, [_vp, _vp, _int, _vp, _int, _int, _vp, _vp]),
    "spfe_match_knn2": (_int, [_vp, _vp, _int, _vp, _int, _vp, _vp]),
    "spfe_match_records_device": (_int, [_vp, _vp, _vp, _int, _int, _vp, _vp]),
    "spfe_match_out_bytes": (_size, [_vp]),
    "spfe_match_patches": (_int, [_vp, _vp, _vp, _int, _vp, _vp, _int, _float, _vp]),
    "spfe_match_patches_record_device": (_int, [_vp, _vp, _vp, _int, _vp, _float, _vp, _vp]),
    # direct "dust" alignment
    "spfe_align_dust": (_int, [_vp, _vp, _vp, _int, _vp, _P(_DustParams), _vp, _vp, _vp, _P(_int), _P(_int)]),
    "spfe_align_dust_record_device": (_int, [_vp, _vp, _vp, _int, _vp, _P(_DustParams), _vp, _vp]),
    "spfe_track_dust_record_device": (_int, [_vp, _vp, _vp, _vp, _int, _vp, _P(_DustParams), _int, _float, _vp, _vp, _vp]),
    "spfe_align_dust_batch_device": (_int, [_vp, _vp, _int, _vp, _vp, _vp, _P(_DustParams), _vp, _vp]),
    # covariance-weighted pose refinement
    "spfe_refine_pose": (_int, [_vp, _vp, _vp, _vp, _int, _vp, _P(_PoseParams), _vp, _vp, _vp, _P(_int)]),
    "spfe_pose_out_bytes": (_size, [_vp]),
    "spfe_pose_lds_edge_capacity": (_int, [_vp]),
    "spfe_refine_pose_record_device": (_int, [_vp, _vp, _vp, _vp, _vp, _P(_PoseParams), _vp, _vp]),
    "spfe_refine_pose_batch_device": (_int, [_vp, _vp, _int, _vp, _vp, _size, _vp, _P(_PoseParams), _vp, _vp]),
    "spfe_track_dust_refine_record_device": (_int, [_vp, _vp, _vp, _vp, _int, _vp, _P(_DustParams), _P(_PoseParams), _int, _int,
                                                    _float, _float, _vp, _vp, _vp, _vp]),
    # local-map tracking: window search by projection and the pose gate
    "spfe_search_projection": (_int, [_vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _vp, _int, _vp, _vp, _P(_ProjParams), _vp, _vp, _vp,
                                      _vp, _P(_int), _P(_int)]),
    "spfe_proj_out_bytes": (_size, [_vp]),
    "spfe_search_projection_record_device": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _int, _vp, _vp, _P(_ProjParams), _vp, _vp]),
    "spfe_search_projection_batch_device": (_int, [_vp, _vp, _int, _vp, _vp, _vp, _vp, _vp, _size, _vp, _vp, _P(_ProjParams), _vp,
                                                   _vp]),
    "spfe_track_local_map_record_device": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _int, _vp, _vp, _P(_ProjParams), _P(_PoseParams),
                                                  _int, _vp, _vp, _vp]),
    # the tracker's fallback steps: TrackWithMotionModel and trackReferenceKeyFrameANN
    "spfe_track_motion_model_record_device": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _vp, _vp, _P(_ProjParams), _P(_PoseParams),
                                                     _int, _int, _vp, _vp, _vp]),
    "spfe_track_reference_kf_record_device": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _int, _vp, _vp, _P(_PoseParams), _int, _vp,
                                                     _vp]),
    # the mapper: new map points between the current keyframe and its neighbours
    "spfe_tri_out_bytes": (_size, [_vp]),
    "spfe_create_map_points_pair_record_device": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _P(_TriParams), _int, _vp, _vp]),
    "spfe_create_map_points_record_device": (_int, [_vp, _vp, _P(_vp), _int, _vp, _vp, _vp, _vp, _vp, _P(_TriParams), _int, _vp,
                                                    _vp]),
    # the mapper: the search of SPMatcher::Fuse
    "spfe_fuse_search": (_int, [_vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _P(_FuseParams), _vp, _vp,
                                _vp, _vp, _vp, _P(_int)]),
    "spfe_fuse_record_device": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _P(_FuseParams), _vp, _vp]),
    "spfe_fuse_targets_record_device": (_int, [_vp, _P(_vp), _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int,
                                               _P(_FuseParams), _vp, _vp]),
    # the loop closer: masked match and Sim3 RANSAC of the loop candidates
    "spfe_loop_match_record_device": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "spfe_sim3_ransac_device": (_int, [_vp, _int, _vp, _vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _int, _P(_Sim3Params), _vp, _vp]),
    "spfe_sim3_ransac": (_int, [_vp, _int, _vp, _vp, _int, _vp, _vp, _vp, _int, _vp, _vp, _vp, _int, _P(_Sim3Params), _vp]),
    "spfe_loop_verify_records_device": (_int, [_vp, _vp, _P(_vp), _int, _vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _int,
                                               _P(_Sim3Params), _vp, _vp, _vp, _vp]),
    "spfe_sim3_iteration_limit": (_int, [_int, C.c_double, _int, _int]),
    # the loop closer: SearchAndFuse and the corrected poses of CorrectLoop
    "spfe_loop_fuse_search": (_int, [_vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _P(_LoopFuseParams),
                                     _vp, _vp, _vp, _vp, _vp, _P(_int)]),
    "spfe_loop_fuse_record_device": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _P(_LoopFuseParams), _vp,
                                            _vp]),
    "spfe_loop_fuse_targets_record_device": (_int, [_vp, _P(_vp), _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int,
                                                    _P(_LoopFuseParams), _vp, _vp]),
    "spfe_loop_corrected_poses_device": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _int, _vp, _vp, _vp]),
    "spfe_loop_corrected_poses": (_int, [_vp, _vp, _vp, _vp, _int, _int, _vp, _vp]),
    # the loop closer: the guided match of a returning hypothesis (SearchBySim3Override)
    "spfe_search_by_sim3": (_int, [_vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _vp, _vp, _int, _vp, _vp, _vp,
                                   _vp, _P(_GuidedParams), _vp]),
    "spfe_search_by_sim3_record_device": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _vp,
                                                 _P(_GuidedParams), _vp, _vp]),
    "spfe_loop_guided_match_records_device": (_int, [_vp, _vp, _P(_vp), _int, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp,
                                                     _vp, _vp, _vp, _int, _P(_GuidedParams), _vp, _vp]),
    # the loop closer: the loop's map points projected into the current keyframe (SearchByProjectionLoop)
    "spfe_search_loop_points": (_int, [_vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _P(_LoopProjParams),
                                       _vp, _vp, _vp, _vp, _vp]),
    "spfe_search_loop_points_record_device": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int,
                                                     _P(_LoopProjParams), _vp, _vp]),
    # the loop closer: the Sim3 optimisation of a hypothesis (OptimizeSim3)
    "spfe_sim3opt_lds_edge_capacity": (_int, [_vp, _int]),
    "spfe_ba_lds_free_capacity": (_int, [_vp]),
    "spfe_bundle_adjust": (_int, [_vp, _vp, _vp, _vp, _int, _vp, _vp, _int, _vp, _int, _P(BaParams), _vp, _vp]),
    "spfe_local_ba_records_device": (_int, [_vp, _vp, _int, _vp, _int, _vp, _vp, _vp, _int, _P(BaParams), _vp, _vp, _vp]),
    "spfe_optimize_sim3": (_int, [_vp, _vp, _int, _vp, _vp, _int, _vp, _vp, _vp, _int, _vp, _vp, _vp, _vp, _P(_Sim3OptParams), _vp]),
    "spfe_optimize_sim3_record_device": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _vp, _P(_Sim3OptParams),
                                                _vp, _vp]),
    "spfe_loop_optimize_sim3_records_device": (_int, [_vp, _vp, _P(_vp), _int, _vp, _int, _vp, _vp, _vp, _vp, _int, _vp, _vp, _vp,
                                                      _int, _vp, _P(_Sim3OptParams), _vp, _vp]),
    # the map-point table: descriptor, normal and depth refreshed from the records, and the gather into a point list
    "spfe_mp_lds_obs_capacity": (_int, [_vp, _int]),
    "spfe_refresh_map_points_device": (_int, [_vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _vp, _int, _int, _vp, _vp, _vp, _vp, _vp, _int,
                                              _P(MpParams), _vp, _vp]),
    "spfe_refresh_map_points": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _int, _P(MpParams), _vp, _vp, _vp, _vp]),
    "spfe_gather_map_points_device": (_int, [_vp, _vp, _int, _vp, _vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # the loop closer: the essential graph over Sim3, its start values and the map-point correction
    "spfe_essential_graph_envelope": (_int, [_int, _vp, _vp, _int, _vp, _P(_int), _P(_int)]),
    "spfe_essgraph_lds_panel_capacity": (_int, [_vp]),
    "spfe_essential_graph_sim3_device": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _vp, _vp, _int, _vp]),
    "spfe_essential_graph_sim3": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _int, _vp, _vp, _int]),
    "spfe_optimize_essential_graph_device": (_int, [_vp, _vp, _vp, _vp, _int, _vp, _int, _int, _P(EssGraphParams), _vp, _vp]),
    "spfe_optimize_essential_graph": (_int, [_vp, _vp, _vp, _vp, _int, _vp, _int, _int, _P(EssGraphParams), _vp]),
    "spfe_correct_map_points_device": (_int, [_vp, _vp, _vp, _int, _vp, _vp, _int, _vp, _vp, _int, _vp, _vp]),
    "spfe_correct_map_points": (_int, [_vp, _vp, _vp, _int, _vp, _vp, _int, _vp, _vp, _int, _vp]),
    # the loop closer: the detection, NetVLAD retrieval and the scoring of its candidates
    "spfe_detect_loop_candidates_device": (_int, [_vp, _vp, _int, _vp, _vp, _vp, _int, _int, _vp, _int, _vp, _int, _P(LoopdetParams),
                                                  _vp, _vp]),
    "spfe_detect_loop_candidates": (_int, [_vp, _vp, _int, _vp, _vp, _vp, _int, _int, _vp, _int, _vp, _int, _P(LoopdetParams), _vp]),
    # the tracker's local map: keyframe votes, expansion, ordered point list
    "spfe_localmap_lds_point_capacity": (_int, [_vp]),
    "spfe_update_local_map_resident": (_int, [_vp, _vp, _int, _vp, _vp, _int, _vp, _int, _vp, _int, _vp, _int, _P(LocalmapParams),
                                              _vp, _vp]),
    "spfe_count_shared_points_resident": (_int, [_vp, _vp, _int, _int, _vp, _int, _vp, _vp, _int, _vp, _vp, _vp]),
    "spfe_local_map_rows_resident": (_int, [_vp, _vp, _int, _vp, _int, _vp, _vp]),
    "spfe_update_local_map": (_int, [_vp, _vp, _int, _vp, _vp, _int, _vp, _int, _vp, _int, _vp, _int, _P(LocalmapParams), _vp]),
    # the covisibility graph
    "spfe_covis_reset_slots_resident": (_int, [_vp, _P(CovisGraph), _int, _int, _vp]),
    "spfe_update_connections_resident": (_int, [_vp, _P(CovisGraph), _vp, _int, _vp, _vp, _int, _int, _P(CovisParams), _vp, _int, _vp,
                                                _int, _vp, _vp]),
    "spfe_update_connections": (_int, [_vp, _P(CovisGraph), _vp, _int, _vp, _vp, _int, _int, _P(CovisParams), _vp, _int, _vp, _int,
                                       _vp]),
    # keyframe culling
    "spfe_count_observations_resident": (_int, [_vp, _vp, _int, _vp, _int, _vp, _int, _vp]),
    "spfe_cull_keyframes_resident": (_int, [_vp, _P(CovisGraph), _vp, _int, _vp, _vp, _vp, _int, _int, _P(CullParams), _vp, _int, _vp,
                                            _int, _vp, _vp]),
    "spfe_cull_keyframes": (_int, [_vp, _P(CovisGraph), _vp, _int, _vp, _vp, _vp, _int, _int, _P(CullParams), _vp, _int, _vp, _int,
                                   _vp]),
    # map-point culling and its resident state
    "spfe_mp_life_reset_resident": (_int, [_vp, _P(MpLife), _int, _int, _int, _vp]),
    "spfe_admit_map_points_resident": (_int, [_vp, _P(MpLife), _vp, _int, _vp, _int, _int, _vp, _int, _int, _vp, _vp, _vp]),
    "spfe_track_statistics_resident": (_int, [_vp, _P(MpLife), _vp, _vp, _int, _vp, _int, _vp, _vp, _vp, _vp]),
    "spfe_cull_map_points_resident": (_int, [_vp, _P(MpLife), _vp, _int, _vp, _int, _P(MpCullParams), _vp, _vp]),
    "spfe_admit_map_points": (_int, [_vp, _P(MpLife), _vp, _int, _vp, _int, _int, _vp, _int, _int, _vp, _vp]),
    "spfe_track_statistics": (_int, [_vp, _P(MpLife), _vp, _vp, _int, _vp, _int, _vp, _vp, _vp]),
    "spfe_cull_map_points": (_int, [_vp, _P(MpLife), _vp, _int, _vp, _int, _P(MpCullParams), _vp]),
    "spfe_insert_keyframe_resident": (_int, [_vp, _P(MpLife), _vp, _int, _int, _vp, _int, _vp, _int, _vp, _vp, _vp, _vp]),
    "spfe_list_observations_resident": (_int, [_vp, _vp, _int, _int, _vp, _int, _vp, _int, _vp, _int, _int, _vp, _vp]),
    "spfe_insert_keyframe": (_int, [_vp, _P(MpLife), _vp, _int, _int, _vp, _int, _vp, _int, _vp, _vp, _vp]),
    "spfe_list_observations": (_int, [_vp, _vp, _int, _int, _vp, _int, _vp, _int, _vp, _int, _int, _vp]),
    "spfe_gather_local_ba_resident": (_int, [_vp, _vp, _int, _vp, _int, _vp, _int, _vp, _vp, _int, _vp, _P(LbaGatherParams), _vp, _vp]),
    "spfe_apply_local_ba_resident": (_int, [_vp, _vp, _vp, _vp, _int, _vp, _int, _vp, _vp, _vp, _vp, _int, _vp, _P(LbaApplyParams), _vp,
                                            _vp]),
    "spfe_gather_local_ba": (_int, [_vp, _vp, _int, _vp, _int, _vp, _int, _vp, _vp, _int, _vp, _P(LbaGatherParams), _vp]),
    "spfe_apply_local_ba": (_int, [_vp, _vp, _vp, _vp, _int, _vp, _int, _vp, _vp, _vp, _vp, _int, _vp, _P(LbaApplyParams), _vp]),
    # input staging
    "spfe_set_staging": (_int, [_vp, _P(_Staging)]),
    "spfe_extract_staged": (_int, [_vp, _vp, _int, _P(_Result)]),
    "spfe_extract_batch_staged": (_int, [_vp, _P(_vp), _int, _int, _P(_Result)]),
    "spfe_stage_batch_device": (_int, [_vp, _vp, _int, _vp, _vp]),
    # stage timing, the maps, probes and versions
    "spfe_stage_times": (_int, [_vp, _P(_float), _int]),
    "spfe_stage_reset": (_int, [_vp]),
    "spfe_stage_name": (_str, [_int]),
    "spfe_fetch_heat_inv": (_int, [_vp, _int, _P(_vp)]),
    "spfe_set_map_buffers": (_int, [_vp, _vp, _vp]),
    "spfe_math_probe": (_int, [_vp, _vp, _vp, _int]),
    "spfe_last_error": (_str, []),
    "spfe_version": (_str, []),
    "spfe_abi_version": (_int, []),
    "spfe_check_abi": (_int, [_int, _size, _size, _size]),
}
ABI_SYMBOLS = list(_SIGNATURES)   # every symbol include/spfe.h declares (tests check that the library exports all)

_lib = None
_lib_lock = threading.Lock()


def _bind_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels ship their own libamdhip64.so.7 (+ HSA
    runtime) under torch/lib; libspfe.so needs the same SONAME.  Whichever copy the dynamic loader
    sees first serves both, and a torch imported AFTER libspfe had pulled in /opt/rocm's copy finds
    no devices.  So when a torch wheel with a bundled runtime is installed (it is the plumbing the
    multi-GPU driver uses), load that copy first; torch itself is not imported here."""
    import importlib.util
    import sys

    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load_library():
    """dlopen libspfe.so (built by __graft_entry__.build()).  Raises if missing."""
    global _lib
    if _lib is not None:
        return _lib
    with _lib_lock:      # threads that create their first handles at the same moment: one of them loads, the others wait
        return _load_library_locked()


def _load_library_locked():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SpfeError("libspfe.so not built at %s — run `python -c 'import __graft_entry__ as g; "
                        "g.build()'` (there is no CPU fallback)" % LIB_PATH)
    _bind_hip_runtime()
    L = C.CDLL(LIB_PATH)
    # the structures above mirror include/spfe.h by hand: a library built from another header revision is refused here,
    # not discovered as overrun arrays later
    if not hasattr(L, "spfe_check_abi"):
        raise SpfeError("libspfe.so at %s predates spfe_check_abi (ABI < %d): rebuild it" % (LIB_PATH, ABI_VERSION))
    for name, (restype, argtypes) in _SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    if L.spfe_check_abi(ABI_VERSION, C.sizeof(_Config), C.sizeof(_Result), C.sizeof(RecordLayout)) != 0:
        raise SpfeError(L.spfe_last_error().decode())
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        msg = load_library().spfe_last_error().decode()
        if rc == -2:
            # the reference throws std::runtime_error("input image is empty")
            # (sp_extractor.cpp:364-365)
            raise RuntimeError("input image is empty")
        raise SpfeError("%s: %s" % (_ERRORS.get(rc, rc), msg))


KEYPOINT_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("size", np.float32),
                           ("angle", np.float32), ("response", np.float32),
                           ("octave", np.int32), ("class_id", np.int32)])


def _as_np(ptr, shape, dtype):
    n = int(np.prod(shape))
    if n == 0 or not ptr:
        return np.zeros(shape, dtype)
    buf = (C.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype).reshape(shape).copy()


class FrameResult:
    """Deep copies of everything one extractor call produced for one frame."""

    def __init__(self, r, H, W, with_heat):
        hc, wc = H // 8, W // 8
        K = r.K
        self.K = K
        self.n_candidates = r.n_candidates
        self.status = r.status
        xy = _as_np(r.kp_xy, (K, 2), np.float32)
        resp = _as_np(r.kp_response, (K,), np.float32)
        kps = np.zeros(K, KEYPOINT_DTYPE)
        # cv::KeyPoint(x, y, 1.0f): angle -1, octave 0, class_id -1 (sp_extractor.cpp:231-232)
        kps["x"], kps["y"] = xy[:, 0], xy[:, 1]
        kps["size"], kps["angle"], kps["octave"], kps["class_id"] = 1.0, -1.0, 0, -1
        kps["response"] = resp  # :271
        self.keypoints = kps
        self.kp_xy = xy
        self.response = resp
        if r.desc:
            self.descriptors = _as_np(r.desc, (K, 256), np.float32)
            self.descriptors_bf16 = None
        else:   # SPFE_FLAG_DESC_BF16: the record carries bf16 rows; `descriptors` is their exact widening to f32
            self.descriptors_bf16 = _as_np(r.desc_bf16, (K, 256), np.uint16)
            self.descriptors = (self.descriptors_bf16.astype(np.uint32) << 16).view(np.float32)
        self.cov2 = _as_np(r.cov2, (K, 2), np.float32)
        self.cov2_inv = _as_np(r.cov2_inv, (K, 2), np.float32)
        self.occ_grid = _as_np(r.occ_grid, (hc, wc), np.int16)
        self.dense_dust = _as_np(r.dense_dust, (hc, wc), np.float32)
        self.semi_dust = _as_np(r.semi_dust, (hc, wc), np.float32)
        self.heat = _as_np(r.heat, (H, W), np.float32) if with_heat and r.heat else None
        self.heat_inv = _as_np(r.heat_inv, (H, W), np.float32) if with_heat and r.heat_inv else None


class SPExtractor:
    """MI355X SuperPoint extractor with the reference's call signature.

    Reference constructor: SPExtractor(int nfeatures) reading camera::height,
    camera::width and common::model_path from globals (sp_extractor.cpp:342-359);
    here they are explicit arguments.
    """

    def __init__(self, nfeatures, height, width, weights, max_batch=1, device=0, with_heat=True,
                 async_cov=False, precision="f32", desc_bf16=False, lazy_heat_inv=False):
        self._h = C.c_void_p()
        self._lib = load_library()
        self.nfeatures, self.height, self.width = int(nfeatures), int(height), int(width)
        self.max_batch, self.with_heat = int(max_batch), bool(with_heat)
        cfg = _Config()
        cfg.height, cfg.width, cfg.num_features = self.height, self.width, self.nfeatures
        if precision not in ("f32", "bf16"):
            raise SpfeError("precision must be 'f32' or 'bf16'")
        self.precision = precision
        cfg.max_batch, cfg.device = self.max_batch, int(device)
        cfg.precision = SPFE_PRECISION_BF16 if precision == "bf16" else SPFE_PRECISION_F32
        cfg.flags = (SPFE_FLAG_HEAT if with_heat else 0) | (SPFE_FLAG_ASYNC_COV if async_cov else 0) | \
            (SPFE_FLAG_DESC_BF16 if desc_bf16 else 0) | (SPFE_FLAG_LAZY_HEAT_INV if lazy_heat_inv and with_heat else 0)
        self.desc_bf16 = bool(desc_bf16)
        self.async_cov = bool(async_cov)
        keep = None
        if isinstance(weights, (str, bytes, os.PathLike)):
            cfg.weights, cfg.weights_path = None, os.fsencode(weights)
        else:
            keep = np.ascontiguousarray(weights, np.float32)
            if keep.size != NUM_PARAMS:
                raise SpfeError("weight blob has %d params, expected %d" % (keep.size, NUM_PARAMS))
            cfg.weights, cfg.weights_path = keep.ctypes.data, None
        _check(self._lib.spfe_create(C.byref(cfg), C.byref(self._h)))
        del keep
        self.layout = RecordLayout()
        _check(self._lib.spfe_get_record_layout(self._h, C.byref(self.layout)))
        # BaseExtractor(n, 1.0, 1, 1, 1): one pyramid level (base_extractor.h:12-47)
        self.nlevels, self.scaleFactor = 1, 1.0
        self.semi_dust_ = self.dense_dust_ = self.heat_ = self.heat_inv_ = self.occ_grid_ = None
        self.mask_ = None  # never written by the reference either
        self._cov2 = self._cov2_inv = None
        self.last = None

    # -- BaseExtractor getters (base_extractor.h:58-72) --
    def GetLevels(self):
        return 1

    def GetScaleFactor(self):
        return 1.0

    def GetScaleFactors(self):
        return [1.0]

    def GetInverseScaleFactors(self):
        return [1.0]

    def GetScaleSigmaSquares(self):
        return [1.0]

    def GetInverseScaleSigmaSquares(self):
        return [1.0]

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.spfe_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check_image(self, image):
        if image is None or getattr(image, "size", 0) == 0:
            raise RuntimeError("input image is empty")  # sp_extractor.cpp:364-365
        img = np.asarray(image)
        if img.dtype != np.uint8 or img.ndim != 2:
            raise SpfeError("image must be CV_8UC1 (2-D uint8)")  # assert at :368
        if img.shape != (self.height, self.width):
            raise SpfeError("image is %s, extractor was built for %s" %
                            (img.shape, (self.height, self.width)))
        if img.strides[1] != 1:
            img = np.ascontiguousarray(img)
        return img

    def _publish(self, fr):
        self.last = fr
        self.semi_dust_, self.dense_dust_ = fr.semi_dust, fr.dense_dust
        self.heat_, self.heat_inv_, self.occ_grid_ = fr.heat, fr.heat_inv, fr.occ_grid
        self._cov2, self._cov2_inv = fr.cov2, fr.cov2_inv

    def __call__(self, image, mask=None):
        """operator()(image, mask, keypoints, descriptors) — mask is ignored (:361-363)."""
        img = self._check_image(image)
        r = _Result()
        _check(self._lib.spfe_extract(self._h, img.ctypes.data, img.strides[0], C.byref(r)))
        fr = FrameResult(r, self.height, self.width, self.with_heat)
        self._publish(fr)
        return fr.keypoints, fr.descriptors

    def extract_batch(self, images):
        """n independent frames in one call; returns a list of FrameResult."""
        imgs = [self._check_image(im) for im in images]
        n = len(imgs)
        if n == 0:
            raise RuntimeError("input image is empty")
        strides = {im.strides[0] for im in imgs}
        if len(strides) != 1:
            imgs = [np.ascontiguousarray(im) for im in imgs]
        ptrs = (C.c_void_p * n)(*[im.ctypes.data for im in imgs])
        res = (_Result * n)()
        _check(self._lib.spfe_extract_batch(self._h, ptrs, imgs[0].strides[0], n, res))
        out = [FrameResult(res[i], self.height, self.width, self.with_heat) for i in range(n)]
        self._publish(out[-1])
        return out

    # -- the synchronous call in three parts (spfe.h: spfe_extract_begin / _maps / _finish) --
    def extract_begin(self, images):
        """Enqueue what extract_batch(images) runs and return at once; extract_finish() delivers the results."""
        imgs = [np.ascontiguousarray(self._check_image(im)) for im in images]
        if not imgs:
            raise RuntimeError("input image is empty")
        ptrs = (C.c_void_p * len(imgs))(*[im.ctypes.data for im in imgs])
        _check(self._lib.spfe_extract_begin(self._h, ptrs, imgs[0].strides[0], len(imgs)))
        self._open_n = len(imgs)

    def extract_maps(self):
        """Block until the open call's H x W maps are in host memory: (heat [n,H,W], heat_inv [n,H,W] or None) as views of
        the library's buffers — or (None, None) when the maps travel with the record in this call."""
        ph, pi = C.POINTER(C.c_float)(), C.POINTER(C.c_float)()
        _check(self._lib.spfe_extract_maps(self._h, C.byref(ph), None))      # heat arrives first ...
        _check(self._lib.spfe_extract_maps(self._h, None, C.byref(pi)))      # ... heat_inv behind it
        n = getattr(self, "_open_n", 0)
        view = lambda p: np.ctypeslib.as_array(p, shape=(n, self.height, self.width)) if p else None
        return view(ph), view(pi)

    def extract_rows(self, frame=0):
        """Block until the open call's descriptor rows of `frame` are in host memory: [K, 256] f32 view of the library's
        buffer, or None when the rows travel with the record in this call."""
        k, p = C.c_int(0), C.POINTER(C.c_float)()
        _check(self._lib.spfe_extract_rows(self._h, int(frame), C.byref(k), C.byref(p)))
        if not p:
            return None
        return np.ctypeslib.as_array(p, shape=(max(k.value, 1), 256))[:k.value]

    def extract_finish(self):
        """The rest of the call begun by extract_begin(); returns what extract_batch would have."""
        n = max(getattr(self, "_open_n", 0), 1)
        res = (_Result * n)()
        self._open_n = 0
        _check(self._lib.spfe_extract_finish(self._h, res))
        out = [FrameResult(res[i], self.height, self.width, self.with_heat) for i in range(n)]
        self._publish(out[-1])
        return out

    def set_map_buffers(self, heat=None, heat_inv=None):
        """spfe_set_map_buffers: the synchronous calls' H x W maps straight into these float32 arrays ([max_batch, H, W],
        C-contiguous; the extractor keeps them alive and the library page-locks them while set); None = the library's buffer."""
        for a in (heat, heat_inv):
            if a is not None and (a.dtype != np.float32 or not a.flags["C_CONTIGUOUS"] or
                                  a.size != self.max_batch * self.height * self.width):
                raise SpfeError("map buffers must be C-contiguous float32 [max_batch, H, W]")
        _check(self._lib.spfe_set_map_buffers(self._h, heat.ctypes.data if heat is not None else None,
                                              heat_inv.ctypes.data if heat_inv is not None else None))
        self._map_buffers = (heat, heat_inv)

    # -- direct "dust" alignment (optimizer_dust.cpp:170-294) --
    @staticmethod
    def _dust_params(fx, fy, cx, cy, max_iterations, huber_delta, inlier_chi2):
        return _DustParams(float(fx), float(fy), float(cx), float(cy), int(max_iterations), float(huber_delta),
                           float(inlier_chi2))

    def align_dust(self, dense_dust, points_xyz, Tcw, fx, fy, cx, cy, max_iterations=40, huber_delta=0.9,
                   inlier_chi2=0.9):
        """Optimizer::PoseOptimizationDust(pFrame, mps, is_visible): -> dict(Tcw [4,4] f32, inlier bool[n],
        uv f32 [n,2] (dust_proj_u/v), n_inlier, iterations)."""
        dust = np.ascontiguousarray(dense_dust, np.float32)
        if dust.shape != (self.height // 8, self.width // 8):
            raise SpfeError("dense_dust must be [H/8, W/8]")
        pts = np.ascontiguousarray(points_xyz, np.float32).reshape(-1, 3)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
        n = len(pts)
        Tout = np.zeros(16, np.float32)
        inl = np.zeros(max(n, 1), np.uint8)
        uv = np.zeros((max(n, 1), 2), np.float32)
        ni, it = C.c_int(0), C.c_int(0)
        prm = self._dust_params(fx, fy, cx, cy, max_iterations, huber_delta, inlier_chi2)
        _check(self._lib.spfe_align_dust(self._h, dust.ctypes.data, pts.ctypes.data, n, T.ctypes.data, C.byref(prm),
                                         Tout.ctypes.data, inl.ctypes.data, uv.ctypes.data, C.byref(ni), C.byref(it)))
        return dict(Tcw=Tout.reshape(4, 4), inlier=inl[:n].astype(bool), uv=uv[:n], n_inlier=ni.value,
                    iterations=it.value)

    def align_dust_record_device(self, d_record, d_points_xyz, n, d_Tcw, d_out, fx, fy, cx, cy, max_iterations=40,
                                 huber_delta=0.9, inlier_chi2=0.9, stream=None):
        prm = self._dust_params(fx, fy, cx, cy, max_iterations, huber_delta, inlier_chi2)
        _check(self._lib.spfe_align_dust_record_device(self._h, C.c_void_p(d_record), C.c_void_p(d_points_xyz), int(n),
                                                       C.c_void_p(d_Tcw), C.byref(prm), C.c_void_p(d_out),
                                                       C.c_void_p(stream or 0)))

    def track_dust_record_device(self, d_record, d_points_xyz, d_mp_desc, n, d_Tcw, d_dust_out, d_kp_idx, fx, fy, cx, cy,
                                 min_inliers=0, max_dist=0.75, max_iterations=40, huber_delta=0.9, inlier_chi2=0.9, stream=None):
        """Tracking::trackFrameDustKFLocal's chain behind the extraction (tracker_dust.cpp:92-172) on a resident record:
        PoseOptimizationDust, then the patch-wise association of the in_view points at their projections
        (spfe_track_dust_record_device); nothing leaves HBM in between."""
        prm = self._dust_params(fx, fy, cx, cy, max_iterations, huber_delta, inlier_chi2)
        _check(self._lib.spfe_track_dust_record_device(self._h, C.c_void_p(d_record), C.c_void_p(d_points_xyz),
                                                       C.c_void_p(d_mp_desc), int(n), C.c_void_p(d_Tcw), C.byref(prm),
                                                       int(min_inliers), float(max_dist), C.c_void_p(d_dust_out),
                                                       C.c_void_p(d_kp_idx), C.c_void_p(stream or 0)))

    def align_dust_batch_device(self, d_records, n_frames, d_points_xyz, d_n_points, d_Tcw, d_out, fx, fy, cx, cy,
                                max_iterations=40, huber_delta=0.9, inlier_chi2=0.9, stream=None):
        """n_frames independent solves in one launch (spfe_align_dust_batch_device): frame f uses record f of `d_records`,
        the points at d_points_xyz + f * DUST_MAX_POINTS * 3 floats (d_n_points[f] of them), pose d_Tcw + 16 f, and writes
        d_out + f * DUST_OUT_BYTES."""
        prm = self._dust_params(fx, fy, cx, cy, max_iterations, huber_delta, inlier_chi2)
        _check(self._lib.spfe_align_dust_batch_device(self._h, C.c_void_p(d_records), int(n_frames), C.c_void_p(d_points_xyz),
                                                      C.c_void_p(d_n_points), C.c_void_p(d_Tcw), C.byref(prm),
                                                      C.c_void_p(d_out), C.c_void_p(stream or 0)))

    @staticmethod
    def decode_dust_out(host_block, n):
        b = np.ascontiguousarray(host_block, np.uint8)
        cnt = b[64:72].view(np.int32)
        return dict(Tcw=b[:64].view(np.float32).reshape(4, 4).copy(), n_inlier=int(cnt[0]), iterations=int(cnt[1]),
                    uv=b[DUST_OFF_UV:DUST_OFF_UV + n * 8].view(np.float32).reshape(n, 2).copy(),
                    inlier=b[DUST_OFF_INLIER:DUST_OFF_INLIER + n].astype(bool))

    # -- covariance-weighted pose refinement (optimizer_dust.cpp:35-167, optimizer.cpp:231-443) --
    @staticmethod
    def _pose_params(fx, fy, cx, cy, schedule, iterations):
        return _PoseParams(float(fx), float(fy), float(cx), float(cy), int(schedule), int(iterations))

    def pose_out_bytes(self):
        return int(self._lib.spfe_pose_out_bytes(self._h))

    def pose_lds_edge_capacity(self):
        """The most edges whose data the device forms stage in LDS (spfe_pose_lds_edge_capacity)."""
        return int(self._lib.spfe_pose_lds_edge_capacity(self._h))

    def refine_pose(self, obs_xy, inv_sigma2, points_xyz, Tcw, fx, fy, cx, cy, schedule=POSE_DUST_POST, iterations=10):
        """PoseOptimizationDustPost / PoseOptimization over n edges given in edge order (spfe_refine_pose): -> dict(Tcw [4,4]
        f32, outlier bool[n], iterations int[4] (per optimize() call), n_good)."""
        obs = np.ascontiguousarray(obs_xy, np.float32).reshape(-1, 2)
        w = np.ascontiguousarray(inv_sigma2, np.float32).reshape(-1, 2)
        pts = np.ascontiguousarray(points_xyz, np.float32).reshape(-1, 3)
        n = len(obs)
        if len(w) != n or len(pts) != n:
            raise SpfeError("obs_xy, inv_sigma2 and points_xyz must have one row per edge")
        T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
        Tout = np.zeros(16, np.float32)
        out = np.zeros(max(n, 1), np.uint8)
        its = np.zeros(4, np.int32)
        ng = C.c_int(0)
        prm = self._pose_params(fx, fy, cx, cy, schedule, iterations)
        _check(self._lib.spfe_refine_pose(self._h, obs.ctypes.data, w.ctypes.data, pts.ctypes.data, n, T.ctypes.data,
                                          C.byref(prm), Tout.ctypes.data, out.ctypes.data, its.ctypes.data, C.byref(ng)))
        return dict(Tcw=Tout.reshape(4, 4), outlier=out[:n].astype(bool), iterations=its, n_good=ng.value)

    def refine_pose_record_device(self, d_record, d_mp_of_kp, d_points_xyz, d_Tcw, d_out, fx, fy, cx, cy,
                                  schedule=POSE_DUST_POST, iterations=10, stream=None):
        """The same on a resident record (spfe_refine_pose_record_device): d_mp_of_kp int32 [kmax] = mvpMapPoints (-1 or a
        row of d_points_xyz); d_out receives pose_out_bytes() bytes (decode_pose_out)."""
        prm = self._pose_params(fx, fy, cx, cy, schedule, iterations)
        _check(self._lib.spfe_refine_pose_record_device(self._h, C.c_void_p(d_record), C.c_void_p(d_mp_of_kp),
                                                        C.c_void_p(d_points_xyz), C.c_void_p(d_Tcw), C.byref(prm),
                                                        C.c_void_p(d_out), C.c_void_p(stream or 0)))

    def refine_pose_batch_device(self, d_records, n_frames, d_mp_of_kp, d_points_xyz, points_stride, d_Tcw, d_out, fx, fy,
                                 cx, cy, schedule=POSE_DUST_POST, iterations=10, stream=None):
        """n_frames solves in one launch (spfe_refine_pose_batch_device): frame f uses record f, d_mp_of_kp + f * kmax,
        d_points_xyz + f * points_stride floats, d_Tcw + 16 f, and writes d_out + f * pose_out_bytes()."""
        prm = self._pose_params(fx, fy, cx, cy, schedule, iterations)
        _check(self._lib.spfe_refine_pose_batch_device(self._h, C.c_void_p(d_records), int(n_frames), C.c_void_p(d_mp_of_kp),
                                                       C.c_void_p(d_points_xyz), int(points_stride), C.c_void_p(d_Tcw),
                                                       C.byref(prm), C.c_void_p(d_out), C.c_void_p(stream or 0)))

    def track_dust_refine_record_device(self, d_record, d_points_xyz, d_mp_desc, n, d_Tcw, d_dust_out, d_kp_idx, d_pose_out,
                                        fx, fy, cx, cy, th_ninlier, th_nmatch, th_ratio, max_dist=0.75, max_iterations=40,
                                        huber_delta=0.9, inlier_chi2=0.9, iterations=10, stream=None):
        """Tracking::trackFrameDustKFLocal behind the extraction (tracker_dust.cpp:22-228) on a resident record: alignment,
        th_ninlier, association, th_nmatch, PoseOptimizationDustPost, the ratio test (spfe_track_dust_refine_record_device).
        EuRoC's thresholds: th_ninlier 20, th_nmatch 20, th_ratio 0.35."""
        dprm = self._dust_params(fx, fy, cx, cy, max_iterations, huber_delta, inlier_chi2)
        pprm = self._pose_params(fx, fy, cx, cy, POSE_DUST_POST, iterations)
        _check(self._lib.spfe_track_dust_refine_record_device(
            self._h, C.c_void_p(d_record), C.c_void_p(d_points_xyz), C.c_void_p(d_mp_desc), int(n), C.c_void_p(d_Tcw),
            C.byref(dprm), C.byref(pprm), int(th_ninlier), int(th_nmatch), float(th_ratio), float(max_dist),
            C.c_void_p(d_dust_out), C.c_void_p(d_kp_idx), C.c_void_p(d_pose_out), C.c_void_p(stream or 0)))

    @staticmethod
    def decode_pose_out(host_block, kmax):
        """The spfe_pose_out_bytes block: dict(Tcw, n_initial, n_good, iterations int[4], status, verdict, n_matches,
        n_inliers, widened, n_outliers, outlier bool[kmax] per keypoint); n_inliers, widened and n_outliers are what the
        block holds there: only the chains named in include/spfe.h write them."""
        b = np.ascontiguousarray(host_block, np.uint8)
        c = b[64:100].view(np.int32)
        return dict(Tcw=b[:64].view(np.float32).reshape(4, 4).copy(), n_initial=int(c[0]), n_good=int(c[1]),
                    iterations=c[2:6].copy(), status=int(c[6]), verdict=int(c[7]), n_matches=int(c[8]),
                    n_inliers=int(b[POSE_OFF_N_INLIERS:POSE_OFF_N_INLIERS + 4].view(np.int32)[0]),
                    widened=int(b[POSE_OFF_WIDENED:POSE_OFF_WIDENED + 4].view(np.int32)[0]),
                    n_outliers=int(b[POSE_OFF_N_OUTLIERS:POSE_OFF_N_OUTLIERS + 4].view(np.int32)[0]),
                    outlier=b[POSE_OFF_OUTLIER:POSE_OFF_OUTLIER + kmax].astype(bool))

    # -- window search by projection and TrackLocalMap (sp_matcher.cpp:344-432, :1439-1543; tracker.cpp:561-615) --
    @staticmethod
    def _proj_params(fx, fy, cx, cy, mode, th, th_dist, view_cos_limit, adaptive, c2_thresh):
        return _ProjParams(float(fx), float(fy), float(cx), float(cy), int(mode), float(th), float(th_dist),
                           float(view_cos_limit), 1 if adaptive else 0, float(c2_thresh))

    def proj_out_bytes(self):
        return int(self._lib.spfe_proj_out_bytes(self._h))

    def search_projection(self, kp_xy, occ_grid, kp_desc, xyz, normal, desc, flags, mp_of_kp, Tcw, fx, fy, cx, cy,
                          mode=PROJ_LOCAL_MAP, th=1.0, th_dist=0.7, view_cos_limit=0.5, adaptive=True, c2_thresh=81.0):
        """SearchByProjection on host arrays (spfe_search_projection): -> dict(mp_of_kp int32[K] (the updated copy),
        kp_of_mp int32[n], in_view bool[n], proj_uv f32[n,2], view_cos f32[n], n_matches, n_to_match)."""
        kp = np.ascontiguousarray(kp_xy, np.float32).reshape(-1, 2)
        K = len(kp)
        occ = np.ascontiguousarray(occ_grid, np.int16)
        kd = np.ascontiguousarray(kp_desc, np.float32).reshape(-1, 256)
        P = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n = len(P)
        N = np.ascontiguousarray(normal if normal is not None else np.zeros((n, 3)), np.float32).reshape(-1, 3)
        D = np.ascontiguousarray(desc, np.float32).reshape(-1, 256)
        F = np.ascontiguousarray(flags, np.uint8).reshape(-1)
        m = np.ascontiguousarray(mp_of_kp, np.int32).reshape(-1).copy()
        if len(kd) != K or len(m) != K or len(N) != n or len(D) != n or len(F) != n:
            raise SpfeError("one row per keypoint in kp_xy / kp_desc / mp_of_kp, one per point in xyz / normal / desc / flags")
        if occ.shape != (self.height // 8, self.width // 8):
            raise SpfeError("occ_grid must be [height / 8, width / 8]")
        T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
        kp_of_mp = np.full(max(n, 1), -1, np.int32)
        in_view = np.zeros(max(n, 1), np.uint8)
        uv = np.zeros((max(n, 1), 2), np.float32)
        vc = np.zeros(max(n, 1), np.float32)
        nm, nt = C.c_int(0), C.c_int(0)
        prm = self._proj_params(fx, fy, cx, cy, mode, th, th_dist, view_cos_limit, adaptive, c2_thresh)
        _check(self._lib.spfe_search_projection(self._h, kp.ctypes.data, occ.ctypes.data, kd.ctypes.data, K, P.ctypes.data,
                                                N.ctypes.data, D.ctypes.data, F.ctypes.data, n, m.ctypes.data, T.ctypes.data,
                                                C.byref(prm), kp_of_mp.ctypes.data, in_view.ctypes.data, uv.ctypes.data,
                                                vc.ctypes.data, C.byref(nm), C.byref(nt)))
        return dict(mp_of_kp=m, kp_of_mp=kp_of_mp[:n], in_view=in_view[:n].astype(bool), proj_uv=uv[:n], view_cos=vc[:n],
                    n_matches=nm.value, n_to_match=nt.value)

    def search_projection_record_device(self, d_record, d_xyz, d_normal, d_desc, d_flags, n, d_mp_of_kp, d_Tcw, d_out, fx,
                                        fy, cx, cy, mode=PROJ_LOCAL_MAP, th=1.0, th_dist=0.7, view_cos_limit=0.5,
                                        adaptive=True, c2_thresh=81.0, stream=None):
        """The same on a resident record (spfe_search_projection_record_device): d_mp_of_kp int32 [kmax] is updated in
        place; d_out receives proj_out_bytes() bytes (decode_proj_out)."""
        prm = self._proj_params(fx, fy, cx, cy, mode, th, th_dist, view_cos_limit, adaptive, c2_thresh)
        _check(self._lib.spfe_search_projection_record_device(
            self._h, C.c_void_p(d_record), C.c_void_p(d_xyz), C.c_void_p(d_normal), C.c_void_p(d_desc), C.c_void_p(d_flags),
            int(n), C.c_void_p(d_mp_of_kp), C.c_void_p(d_Tcw), C.byref(prm), C.c_void_p(d_out), C.c_void_p(stream or 0)))

    def search_projection_batch_device(self, d_records, n_frames, d_xyz, d_normal, d_desc, d_flags, d_n_points,
                                       points_stride, d_mp_of_kp, d_Tcw, d_out, fx, fy, cx, cy, mode=PROJ_LOCAL_MAP, th=1.0,
                                       th_dist=0.7, view_cos_limit=0.5, adaptive=True, c2_thresh=81.0, stream=None):
        """n_frames searches in the same launches (spfe_search_projection_batch_device): frame f uses record f, the point
        arrays at f * points_stride rows, d_n_points[f] of them, d_mp_of_kp + f * kmax, d_Tcw + 16 f, and writes
        d_out + f * proj_out_bytes()."""
        prm = self._proj_params(fx, fy, cx, cy, mode, th, th_dist, view_cos_limit, adaptive, c2_thresh)
        _check(self._lib.spfe_search_projection_batch_device(
            self._h, C.c_void_p(d_records), int(n_frames), C.c_void_p(d_xyz), C.c_void_p(d_normal), C.c_void_p(d_desc),
            C.c_void_p(d_flags), C.c_void_p(d_n_points), int(points_stride), C.c_void_p(d_mp_of_kp), C.c_void_p(d_Tcw),
            C.byref(prm), C.c_void_p(d_out), C.c_void_p(stream or 0)))

    def track_local_map_record_device(self, d_record, d_xyz, d_normal, d_desc, d_flags, n, d_mp_of_kp, d_Tcw, d_proj_out,
                                      d_pose_out, fx, fy, cx, cy, th_ninlier, th=1.0, th_dist=0.7, view_cos_limit=0.5,
                                      adaptive=True, c2_thresh=81.0, iterations=10, stream=None):
        """Tracking::TrackLocalMap on a resident record (spfe_track_local_map_record_device): the LOCAL_MAP search,
        PoseOptimization over the updated d_mp_of_kp from d_Tcw, mnMatchesInliers >= th_ninlier.  d_pose_out:
        decode_pose_out (verdict TRACK_OK / TRACK_FAIL_LOCAL_INLIERS / TRACK_FAIL_COV, n_matches, n_inliers)."""
        jprm = self._proj_params(fx, fy, cx, cy, PROJ_LOCAL_MAP, th, th_dist, view_cos_limit, adaptive, c2_thresh)
        pprm = self._pose_params(fx, fy, cx, cy, POSE_OPTIMIZATION, iterations)
        _check(self._lib.spfe_track_local_map_record_device(
            self._h, C.c_void_p(d_record), C.c_void_p(d_xyz), C.c_void_p(d_normal), C.c_void_p(d_desc), C.c_void_p(d_flags),
            int(n), C.c_void_p(d_mp_of_kp), C.c_void_p(d_Tcw), C.byref(jprm), C.byref(pprm), int(th_ninlier),
            C.c_void_p(d_proj_out), C.c_void_p(d_pose_out), C.c_void_p(stream or 0)))

    # -- the tracker's fallback steps (tracker.cpp:480-559, :372-417) --
    def track_motion_model_record_device(self, d_record, d_xyz, d_desc, d_flags, n, d_mp_of_kp, d_Tcw, d_proj_out, d_pose_out,
                                         fx, fy, cx, cy, th=15.0, th_nmatch_proj=20, th_nmatch_opt=10, th_dist=0.7,
                                         iterations=10, stream=None):
        """Tracking::TrackWithMotionModel on a resident record (spfe_track_motion_model_record_device): d_mp_of_kp cleared,
        the LAST_FRAME search with radius th, on fewer than th_nmatch_proj matches (decided on the device) the search with
        2 th alone, PoseOptimization from d_Tcw, the outliers discarded, n_inliers >= th_nmatch_opt.  d_proj_out:
        decode_proj_out, the search that stands; d_pose_out: decode_pose_out (verdict TRACK_OK / TRACK_FAIL_MOTION_INLIERS /
        TRACK_FAIL_COV, n_matches, n_inliers, widened, n_outliers).  The defaults are src/config.cpp's."""
        jprm = self._proj_params(fx, fy, cx, cy, PROJ_LAST_FRAME, th, th_dist, 0.5, True, 81.0)
        pprm = self._pose_params(fx, fy, cx, cy, POSE_OPTIMIZATION, iterations)
        _check(self._lib.spfe_track_motion_model_record_device(
            self._h, C.c_void_p(d_record), C.c_void_p(d_xyz), C.c_void_p(d_desc), C.c_void_p(d_flags), int(n),
            C.c_void_p(d_mp_of_kp), C.c_void_p(d_Tcw), C.byref(jprm), C.byref(pprm), int(th_nmatch_proj), int(th_nmatch_opt),
            C.c_void_p(d_proj_out), C.c_void_p(d_pose_out), C.c_void_p(stream or 0)))

    def track_reference_kf_record_device(self, d_record, d_kf_record, d_kf_mp_of_kp, d_xyz, d_flags, n, d_mp_of_kp, d_Tcw,
                                         d_pose_out, fx, fy, cx, cy, th_nmatch_opt=10, iterations=10, stream=None):
        """Tracking::trackReferenceKeyFrameANN on a resident record and the keyframe's record
        (spfe_track_reference_kf_record_device): the cross-check match of the frame's rows against the keyframe's rows that
        hold a point (d_kf_mp_of_kp int32 [kmax]: index into d_xyz / d_flags, or -1), the matched keypoints take those points,
        PoseOptimization from d_Tcw, the outliers discarded, n_inliers >= th_nmatch_opt.  d_pose_out: decode_pose_out
        (verdict TRACK_OK / TRACK_FAIL_REFKF_INLIERS / TRACK_FAIL_COV, n_matches, n_inliers, n_outliers)."""
        pprm = self._pose_params(fx, fy, cx, cy, POSE_OPTIMIZATION, iterations)
        _check(self._lib.spfe_track_reference_kf_record_device(
            self._h, C.c_void_p(d_record), C.c_void_p(d_kf_record), C.c_void_p(d_kf_mp_of_kp), C.c_void_p(d_xyz),
            C.c_void_p(d_flags), int(n), C.c_void_p(d_mp_of_kp), C.c_void_p(d_Tcw), C.byref(pprm), int(th_nmatch_opt),
            C.c_void_p(d_pose_out), C.c_void_p(stream or 0)))

    # -- the mapper: CreateNewMapPointsOverride on keyframe records (local_mapper.cpp:558-814, sp_matcher.cpp:183-262) --
    @staticmethod
    def _tri_params(intr1, intr2, ratio, epipole_r2, chi2_line, chi2_reproj, cos_parallax_max, min_baseline_depth_ratio):
        return _TriParams(*[float(v) for v in tuple(intr1) + tuple(intr2)], float(ratio), float(epipole_r2), float(chi2_line),
                          float(chi2_reproj), float(cos_parallax_max), float(min_baseline_depth_ratio))

    def tri_out_bytes(self):
        return int(self._lib.spfe_tri_out_bytes(self._h))

    def create_map_points_pair_record_device(self, d_record1, d_record2, d_mp1_of_kp, d_mp2_of_kp, d_Tcw1, d_Tcw2, d_out, intr1,
                                             intr2=None, point_base=0, ratio=0.7, epipole_r2=100.0, chi2_line=3.84,
                                             chi2_reproj=5.991, cos_parallax_max=0.9998, min_baseline_depth_ratio=0.01,
                                             stream=None):
        """New map points between the current keyframe's record (1) and ONE neighbour's (2)
        (spfe_create_map_points_pair_record_device): the free keypoints (d_mp*_of_kp int32 [kmax] < 0) are matched 2-NN with the
        0.7 ratio test, gated on the epipole and the epipolar line, triangulated and gated; the keypoints of new point t get
        point_base + t in both arrays.  intr = (fx, fy, cx, cy).  d_out: tri_out_bytes() bytes (decode_tri_out)."""
        prm = self._tri_params(intr1, intr2 or intr1, ratio, epipole_r2, chi2_line, chi2_reproj, cos_parallax_max,
                               min_baseline_depth_ratio)
        _check(self._lib.spfe_create_map_points_pair_record_device(
            self._h, C.c_void_p(d_record1), C.c_void_p(d_record2), C.c_void_p(d_mp1_of_kp), C.c_void_p(d_mp2_of_kp),
            C.c_void_p(d_Tcw1), C.c_void_p(d_Tcw2), C.byref(prm), int(point_base), C.c_void_p(d_out), C.c_void_p(stream or 0)))

    def create_map_points_record_device(self, d_record1, d_records2, d_mp1_of_kp, d_mp2_of_kp, d_Tcw1, d_Tcw2, d_median_depth,
                                        d_out, intr1, intr2=None, point_base=0, ratio=0.7, epipole_r2=100.0, chi2_line=3.84,
                                        chi2_reproj=5.991, cos_parallax_max=0.9998, min_baseline_depth_ratio=0.01, stream=None):
        """The loop over the neighbours as one call (spfe_create_map_points_record_device): d_records2 is a sequence of device
        pointers, one record per neighbour; neighbour j uses d_mp2_of_kp + j * kmax, d_Tcw2 + 16 j, d_median_depth[j] (f32) and
        writes d_out + j * tri_out_bytes(); it is skipped on the device when baseline / median depth is below
        min_baseline_depth_ratio, sees d_mp1_of_kp as the neighbours before it left it, and its ids run on behind theirs."""
        n = len(d_records2)
        ptrs = (C.c_void_p * max(n, 1))(*[int(p) for p in d_records2])
        prm = self._tri_params(intr1, intr2 or intr1, ratio, epipole_r2, chi2_line, chi2_reproj, cos_parallax_max,
                               min_baseline_depth_ratio)
        _check(self._lib.spfe_create_map_points_record_device(
            self._h, C.c_void_p(d_record1), ptrs, n, C.c_void_p(d_mp1_of_kp), C.c_void_p(d_mp2_of_kp), C.c_void_p(d_Tcw1),
            C.c_void_p(d_Tcw2), C.c_void_p(d_median_depth), C.byref(prm), int(point_base), C.c_void_p(d_out),
            C.c_void_p(stream or 0)))

    @staticmethod
    def decode_tri_out(host_block, kmax):
        """One neighbour's spfe_tri_out_bytes block: dict(the TRI_FIELDS ints, match12 int32[kmax], verdict int32[kmax],
        new_xyz f32[n_new,3], new_k1, new_k2 int32[n_new]).  A block with status != 0 holds nothing but the status, a skipped
        one nothing but the ints: the arrays are then returned as they lie in the block."""
        b = np.ascontiguousarray(host_block, np.uint8)
        o = tri_offsets(kmax)
        out = {k: int(v) for k, v in zip(TRI_FIELDS, b[:4 * len(TRI_FIELDS)].view(np.int32))}
        live = out["status"] == 0 and out["skipped"] == 0
        n = min(max(out["n_new"], 0), kmax) if live else 0
        out.update(match12=b[TRI_OFF_MATCH12:TRI_OFF_MATCH12 + 4 * kmax].view(np.int32).copy(),
                   verdict=b[o["verdict"]:o["verdict"] + 4 * kmax].view(np.int32).copy(),
                   new_xyz=b[o["new_xyz"]:o["new_xyz"] + 12 * n].view(np.float32).reshape(n, 3).copy(),
                   new_k1=b[o["new_k1"]:o["new_k1"] + 4 * n].view(np.int32).copy(),
                   new_k2=b[o["new_k2"]:o["new_k2"] + 4 * n].view(np.int32).copy())
        return out

    # -- the mapper: the search of SPMatcher::Fuse in SearchInNeighbors (sp_matcher.cpp:965-1104, local_mapper.cpp:816-904) --
    @staticmethod
    def _fuse_params(fx, fy, cx, cy, th, th_dist, chi2, view_cos, min_factor, max_factor):
        return _FuseParams(float(fx), float(fy), float(cx), float(cy), float(th), float(th_dist), float(chi2), float(view_cos),
                           float(min_factor), float(max_factor))

    @staticmethod
    def fuse_out_bytes(n_cap):
        return fuse_offsets(int(n_cap))["out_bytes"]

    def fuse_search(self, kp_xy, occ_grid, kp_desc, kf_mp_of_kp, Tcw, point_id, xyz, normal, dist_range, desc, flags, fx, fy,
                    cx, cy, th=3.0, th_dist=0.3, chi2=5.99, view_cos=0.5, min_factor=0.8, max_factor=1.2):
        """The search of Fuse on host arrays (spfe_fuse_search): -> dict(n_fused, kp_of_mp int32[n], best_dist f32[n],
        holder int32[n], reason uint8[n], fused_idx int32[n_fused])."""
        kp = np.ascontiguousarray(kp_xy, np.float32).reshape(-1, 2)
        K = len(kp)
        occ = np.ascontiguousarray(occ_grid, np.int16)
        kd = np.ascontiguousarray(kp_desc, np.float32).reshape(-1, 256)
        m = np.ascontiguousarray(kf_mp_of_kp, np.int32).reshape(-1)
        ids = np.ascontiguousarray(point_id, np.int32).reshape(-1)
        n = len(ids)
        P = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        N = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
        R = np.ascontiguousarray(dist_range, np.float32).reshape(-1, 2)
        D = np.ascontiguousarray(desc, np.float32).reshape(-1, 256)
        F = np.ascontiguousarray(flags, np.uint8).reshape(-1)
        if len(kd) != K or len(m) != K or len(P) != n or len(N) != n or len(R) != n or len(D) != n or len(F) != n:
            raise SpfeError("one row per keypoint in kp_xy / kp_desc / kf_mp_of_kp, one per point in the point arrays")
        if occ.shape != (self.height // 8, self.width // 8):
            raise SpfeError("occ_grid must be [height / 8, width / 8]")
        T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
        cap = max(n, 1)
        kom, bd, hol = np.full(cap, -1, np.int32), np.zeros(cap, np.float32), np.full(cap, -1, np.int32)
        rs, fi = np.zeros(cap, np.uint8), np.zeros(cap, np.int32)
        nf = C.c_int(0)
        prm = self._fuse_params(fx, fy, cx, cy, th, th_dist, chi2, view_cos, min_factor, max_factor)
        _check(self._lib.spfe_fuse_search(self._h, kp.ctypes.data, occ.ctypes.data, kd.ctypes.data, K, m.ctypes.data,
                                          T.ctypes.data, ids.ctypes.data, P.ctypes.data, N.ctypes.data, R.ctypes.data,
                                          D.ctypes.data, F.ctypes.data, n, C.byref(prm), kom.ctypes.data, bd.ctypes.data,
                                          hol.ctypes.data, rs.ctypes.data, fi.ctypes.data, C.byref(nf)))
        return dict(n_fused=nf.value, kp_of_mp=kom[:n], best_dist=bd[:n], holder=hol[:n], reason=rs[:n],
                    fused_idx=fi[:nf.value].copy())

    def fuse_record_device(self, d_record, d_kf_mp_of_kp, d_Tcw, d_point_id, d_xyz, d_normal, d_dist_range, d_desc, d_flags, n,
                           d_out, fx, fy, cx, cy, n_cap=None, th=3.0, th_dist=0.3, chi2=5.99, view_cos=0.5, min_factor=0.8,
                           max_factor=1.2, stream=None):
        """The search of Fuse of n points into ONE resident record (spfe_fuse_record_device): d_kf_mp_of_kp int32 [kmax] is
        read only; d_out receives fuse_out_bytes(n_cap) bytes (decode_fuse_out); n_cap defaults to max(n, 1)."""
        prm = self._fuse_params(fx, fy, cx, cy, th, th_dist, chi2, view_cos, min_factor, max_factor)
        _check(self._lib.spfe_fuse_record_device(
            self._h, C.c_void_p(d_record), C.c_void_p(d_kf_mp_of_kp), C.c_void_p(d_Tcw), C.c_void_p(d_point_id), C.c_void_p(d_xyz),
            C.c_void_p(d_normal), C.c_void_p(d_dist_range), C.c_void_p(d_desc), C.c_void_p(d_flags), int(n),
            int(max(n, 1) if n_cap is None else n_cap), C.byref(prm), C.c_void_p(d_out), C.c_void_p(stream or 0)))

    def fuse_targets_record_device(self, d_records, d_kf_mp_of_kp, d_Tcw, d_point_id, d_xyz, d_normal, d_dist_range, d_desc,
                                   d_flags, n, d_out, fx, fy, cx, cy, n_cap=None, th=3.0, th_dist=0.3, chi2=5.99, view_cos=0.5,
                                   min_factor=0.8, max_factor=1.2, stream=None):
        """The loop over the targets as one call (spfe_fuse_targets_record_device): d_records is a sequence of device
        pointers, one record per target; target j uses d_kf_mp_of_kp + j * kmax, d_Tcw + 16 j, the one point list, and
        writes d_out + j * fuse_out_bytes(n_cap)."""
        nt = len(d_records)
        ptrs = (C.c_void_p * max(nt, 1))(*[int(p) for p in d_records])
        prm = self._fuse_params(fx, fy, cx, cy, th, th_dist, chi2, view_cos, min_factor, max_factor)
        _check(self._lib.spfe_fuse_targets_record_device(
            self._h, ptrs, nt, C.c_void_p(d_kf_mp_of_kp), C.c_void_p(d_Tcw), C.c_void_p(d_point_id), C.c_void_p(d_xyz),
            C.c_void_p(d_normal), C.c_void_p(d_dist_range), C.c_void_p(d_desc), C.c_void_p(d_flags), int(n),
            int(max(n, 1) if n_cap is None else n_cap), C.byref(prm), C.c_void_p(d_out), C.c_void_p(stream or 0)))

    @staticmethod
    def decode_fuse_out(host_block, n_cap):
        """One target's block over the capacity n_cap: dict(n_fused, n, status, kp_of_mp int32[n], best_dist f32[n],
        holder int32[n], reason uint8[n], fused_idx int32[n_fused])."""
        b = np.ascontiguousarray(host_block, np.uint8)
        o = fuse_offsets(int(n_cap))
        out = {k: int(v) for k, v in zip(FUSE_FIELDS, b[:4 * len(FUSE_FIELDS)].view(np.int32))}
        n, nf = min(max(out["n"], 0), n_cap), min(max(out["n_fused"], 0), n_cap)
        out.update(kp_of_mp=b[FUSE_OFF_KP_OF_MP:FUSE_OFF_KP_OF_MP + 4 * n].view(np.int32).copy(),
                   best_dist=b[o["best_dist"]:o["best_dist"] + 4 * n].view(np.float32).copy(),
                   holder=b[o["holder"]:o["holder"] + 4 * n].view(np.int32).copy(),
                   fused_idx=b[o["fused_idx"]:o["fused_idx"] + 4 * nf].view(np.int32).copy(),
                   reason=b[o["reason"]:o["reason"] + n].copy())
        return out

    # -- the loop closer: SearchAndFuse (sp_matcher.cpp:1106-1219, loop_closer_vlad.cpp:701-726) and the corrected poses --
    @staticmethod
    def _loop_fuse_params(fx, fy, cx, cy, th, th_dist, view_cos, min_factor, max_factor):
        return _LoopFuseParams(float(fx), float(fy), float(cx), float(cy), float(th), float(th_dist), float(view_cos),
                               float(min_factor), float(max_factor))

    def loop_fuse_search(self, kp_xy, occ_grid, kp_desc, kf_mp_of_kp, Scw, point_id, xyz, normal, dist_range, desc, flags, fx, fy,
                         cx, cy, th=4.0, th_dist=0.7, view_cos=0.5, min_factor=0.8, max_factor=1.2):
        """The search of Fuse under a similarity on host arrays (spfe_loop_fuse_search): -> dict(n_fused, kp_of_mp int32[n],
        best_dist f32[n], holder int32[n], reason uint8[n], fused_idx int32[n_fused])."""
        kp = np.ascontiguousarray(kp_xy, np.float32).reshape(-1, 2)
        K = len(kp)
        occ = np.ascontiguousarray(occ_grid, np.int16)
        kd = np.ascontiguousarray(kp_desc, np.float32).reshape(-1, 256)
        m = np.ascontiguousarray(kf_mp_of_kp, np.int32).reshape(-1)
        ids = np.ascontiguousarray(point_id, np.int32).reshape(-1)
        n = len(ids)
        P = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        N = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
        R = np.ascontiguousarray(dist_range, np.float32).reshape(-1, 2)
        D = np.ascontiguousarray(desc, np.float32).reshape(-1, 256)
        F = np.ascontiguousarray(flags, np.uint8).reshape(-1)
        if len(kd) != K or len(m) != K or len(P) != n or len(N) != n or len(R) != n or len(D) != n or len(F) != n:
            raise SpfeError("one row per keypoint in kp_xy / kp_desc / kf_mp_of_kp, one per point in the point arrays")
        if occ.shape != (self.height // 8, self.width // 8):
            raise SpfeError("occ_grid must be [height / 8, width / 8]")
        S = np.ascontiguousarray(Scw, np.float32).reshape(16)
        cap = max(n, 1)
        kom, bd, hol = np.full(cap, -1, np.int32), np.zeros(cap, np.float32), np.full(cap, -1, np.int32)
        rs, fi = np.zeros(cap, np.uint8), np.zeros(cap, np.int32)
        nf = C.c_int(0)
        prm = self._loop_fuse_params(fx, fy, cx, cy, th, th_dist, view_cos, min_factor, max_factor)
        _check(self._lib.spfe_loop_fuse_search(self._h, kp.ctypes.data, occ.ctypes.data, kd.ctypes.data, K, m.ctypes.data,
                                               S.ctypes.data, ids.ctypes.data, P.ctypes.data, N.ctypes.data, R.ctypes.data,
                                               D.ctypes.data, F.ctypes.data, n, C.byref(prm), kom.ctypes.data, bd.ctypes.data,
                                               hol.ctypes.data, rs.ctypes.data, fi.ctypes.data, C.byref(nf)))
        return dict(n_fused=nf.value, kp_of_mp=kom[:n], best_dist=bd[:n], holder=hol[:n], reason=rs[:n],
                    fused_idx=fi[:nf.value].copy())

    def loop_fuse_record_device(self, d_record, d_kf_mp_of_kp, d_Scw, d_point_id, d_xyz, d_normal, d_dist_range, d_desc, d_flags,
                                n, d_out, fx, fy, cx, cy, n_cap=None, th=4.0, th_dist=0.7, view_cos=0.5, min_factor=0.8,
                                max_factor=1.2, stream=None):
        """The loop's fuse search of n points into ONE resident record (spfe_loop_fuse_record_device): d_Scw f32 [16],
        d_kf_mp_of_kp int32 [kmax] read only; d_out receives fuse_out_bytes(n_cap) bytes (decode_fuse_out)."""
        prm = self._loop_fuse_params(fx, fy, cx, cy, th, th_dist, view_cos, min_factor, max_factor)
        _check(self._lib.spfe_loop_fuse_record_device(
            self._h, C.c_void_p(d_record), C.c_void_p(d_kf_mp_of_kp), C.c_void_p(d_Scw), C.c_void_p(d_point_id), C.c_void_p(d_xyz),
            C.c_void_p(d_normal), C.c_void_p(d_dist_range), C.c_void_p(d_desc), C.c_void_p(d_flags), int(n),
            int(max(n, 1) if n_cap is None else n_cap), C.byref(prm), C.c_void_p(d_out), C.c_void_p(stream or 0)))

    def loop_fuse_targets_record_device(self, d_records, d_kf_mp_of_kp, d_Scw, d_point_id, d_xyz, d_normal, d_dist_range, d_desc,
                                        d_flags, n, d_out, fx, fy, cx, cy, n_cap=None, th=4.0, th_dist=0.7, view_cos=0.5,
                                        min_factor=0.8, max_factor=1.2, stream=None):
        """SearchAndFuse's loop over the connected keyframes as one call (spfe_loop_fuse_targets_record_device): target j uses
        d_kf_mp_of_kp + j * kmax, d_Scw + 16 j (the d_Siw of loop_corrected_poses_device), the one point list, and writes
        d_out + j * fuse_out_bytes(n_cap)."""
        nt = len(d_records)
        ptrs = (C.c_void_p * max(nt, 1))(*[int(p) for p in d_records])
        prm = self._loop_fuse_params(fx, fy, cx, cy, th, th_dist, view_cos, min_factor, max_factor)
        _check(self._lib.spfe_loop_fuse_targets_record_device(
            self._h, ptrs, nt, C.c_void_p(d_kf_mp_of_kp), C.c_void_p(d_Scw), C.c_void_p(d_point_id), C.c_void_p(d_xyz),
            C.c_void_p(d_normal), C.c_void_p(d_dist_range), C.c_void_p(d_desc), C.c_void_p(d_flags), int(n),
            int(max(n, 1) if n_cap is None else n_cap), C.byref(prm), C.c_void_p(d_out), C.c_void_p(stream or 0)))

    def loop_corrected_poses_device(self, d_opt_block, d_Tcw2, d_Twc, d_Tiw, n_targets, cur_index, d_Siw, d_Tiw_corrected,
                                    stream=None):
        """The corrected poses of CorrectLoop on the device (spfe_loop_corrected_poses_device): S12 is read out of the optimise
        block d_opt_block; d_Siw / d_Tiw_corrected f32 [n_targets][16]."""
        _check(self._lib.spfe_loop_corrected_poses_device(
            self._h, C.c_void_p(d_opt_block), C.c_void_p(d_Tcw2), C.c_void_p(d_Twc), C.c_void_p(d_Tiw), int(n_targets),
            int(cur_index), C.c_void_p(d_Siw), C.c_void_p(d_Tiw_corrected), C.c_void_p(stream or 0)))

    @staticmethod
    def loop_corrected_poses(S12, Tcw2, Twc, Tiw, cur_index=-1):
        """The same on the host (spfe_loop_corrected_poses; a pure function): S12 f64 [13], Tcw2 / Twc f32 4x4, Tiw f32
        [T, 4, 4] -> (Siw f32 [T, 4, 4], Tiw_corrected f32 [T, 4, 4])."""
        S = np.ascontiguousarray(S12, np.float64).reshape(13)
        T2 = np.ascontiguousarray(Tcw2, np.float32).reshape(16)
        Tw = np.ascontiguousarray(Twc, np.float32).reshape(16)
        Ti = np.ascontiguousarray(Tiw, np.float32).reshape(-1, 16)
        nt = len(Ti)
        Siw, Tc = np.zeros((max(nt, 1), 4, 4), np.float32), np.zeros((max(nt, 1), 4, 4), np.float32)
        _check(load_library().spfe_loop_corrected_poses(S.ctypes.data, T2.ctypes.data, Tw.ctypes.data, Ti.ctypes.data, nt,
                                                        int(cur_index), Siw.ctypes.data, Tc.ctypes.data))
        return Siw[:nt], Tc[:nt]

    # -- the loop closer: the front half of ComputeSim3 (loop_closer_vlad.cpp:345-449, sp_matcher_loop.cpp:334-376) --
    @staticmethod
    def _sim3_params(intr1, intr2, max_err1, max_err2, min_inliers, fix_scale):
        return _Sim3Params(*[float(v) for v in tuple(intr1) + tuple(intr1 if intr2 is None else intr2)], float(max_err1), float(max_err2),
                           int(min_inliers), int(bool(fix_scale)))

    def sim3_out_bytes(self, n_hyp, kmax=None):
        return sim3_offsets(self.layout.kmax if kmax is None else int(kmax), int(n_hyp))["out_bytes"]

    def loop_match_record_device(self, d_record1, d_record2, d_kf1_mp_of_kp, d_kf2_mp_of_kp, d_match12, d_n_matches, stream=None):
        """SearchByBruteForce between the current keyframe's record (1) and a candidate's (2), both of this handle
        (spfe_loop_match_record_device): cross-check between the rows whose d_kf*_mp_of_kp (int32 [kmax]) is >= 0;
        d_match12 int32 [kmax] receives the candidate's keypoint per k1 or -1, d_n_matches (int32) their number."""
        _check(self._lib.spfe_loop_match_record_device(
            self._h, C.c_void_p(d_record1), C.c_void_p(d_record2), C.c_void_p(d_kf1_mp_of_kp), C.c_void_p(d_kf2_mp_of_kp),
            C.c_void_p(d_match12), C.c_void_p(d_n_matches), C.c_void_p(stream or 0)))

    def sim3_ransac_device(self, K1, d_match12, d_kf1_mp_of_kp, d_kf2_mp_of_kp, d_xyz, d_flags, n, d_Tcw1, d_Tcw2, d_rand_u32,
                           n_hyp, d_out, intr1, intr2=None, max_err1=9.0, max_err2=9.0, min_inliers=20, fix_scale=False,
                           stream=None):
        """The Sim3Solver of one candidate on device arrays (spfe_sim3_ransac_device): the index arrays are int32 [kmax],
        d_rand_u32 uint32 [n_hyp][3]; d_out receives sim3_out_bytes(n_hyp) bytes (decode_sim3_out)."""
        prm = self._sim3_params(intr1, intr2, max_err1, max_err2, min_inliers, fix_scale)
        _check(self._lib.spfe_sim3_ransac_device(
            self._h, int(K1), C.c_void_p(d_match12), C.c_void_p(d_kf1_mp_of_kp), C.c_void_p(d_kf2_mp_of_kp), C.c_void_p(d_xyz),
            C.c_void_p(d_flags), int(n), C.c_void_p(d_Tcw1), C.c_void_p(d_Tcw2), C.c_void_p(d_rand_u32), int(n_hyp), C.byref(prm),
            C.c_void_p(d_out), C.c_void_p(stream or 0)))

    def sim3_ransac(self, match12, kf1_mp_of_kp, kf2_mp_of_kp, xyz, flags, Tcw1, Tcw2, rand_u32, intr1, intr2=None, max_err1=9.0,
                    max_err2=9.0, min_inliers=20, fix_scale=False, fill=0):
        """The same on host arrays (spfe_sim3_ransac), synchronous: -> (raw block over kmax = max(K1, K2, 1) on a background
        of `fill`, that kmax); decode_sim3_out(block, kmax, n_hyp) unpacks it."""
        m = np.ascontiguousarray(match12, np.int32)
        a = np.ascontiguousarray(kf1_mp_of_kp, np.int32)
        b = np.ascontiguousarray(kf2_mp_of_kp, np.int32)
        assert len(m) == len(a)
        p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        f = np.ascontiguousarray(flags, np.uint8)
        assert len(p) == len(f)
        r = np.ascontiguousarray(rand_u32, np.uint32).reshape(-1, 3)
        T1 = np.ascontiguousarray(Tcw1, np.float32).reshape(16)
        T2 = np.ascontiguousarray(Tcw2, np.float32).reshape(16)
        kcap = max(len(a), len(b), 1)
        out = np.full(sim3_offsets(kcap, len(r))["out_bytes"], fill, np.uint8)
        prm = self._sim3_params(intr1, intr2, max_err1, max_err2, min_inliers, fix_scale)
        ptr = lambda v: v.ctypes.data if v.size else None   # noqa: E731
        _check(self._lib.spfe_sim3_ransac(self._h, len(a), ptr(m), ptr(a), len(b), ptr(b), ptr(p), ptr(f), len(f), T1.ctypes.data,
                                          T2.ctypes.data, ptr(r), len(r), C.byref(prm), out.ctypes.data))
        return out, kcap

    def loop_verify_records_device(self, d_record1, d_records2, d_kf1_mp_of_kp, d_kf2_mp_of_kp, d_xyz, d_flags, n, d_Tcw1, d_Tcw2,
                                   d_rand_u32, n_hyp, d_match12, d_n_matches, d_out, intr1, intr2=None, max_err1=9.0,
                                   max_err2=9.0, min_inliers=20, fix_scale=False, stream=None):
        """Match and Sim3 hypotheses of every loop candidate as one call (spfe_loop_verify_records_device): d_records2 is a
        sequence of device pointers; candidate j uses d_kf2_mp_of_kp + j * kmax, d_Tcw2 + 16 j, d_rand_u32 + j * 3 * n_hyp and
        writes d_match12 + j * kmax, d_n_matches + j, d_out + j * sim3_out_bytes(n_hyp)."""
        nc = len(d_records2)
        ptrs = (C.c_void_p * max(nc, 1))(*[int(p) for p in d_records2])
        prm = self._sim3_params(intr1, intr2, max_err1, max_err2, min_inliers, fix_scale)
        _check(self._lib.spfe_loop_verify_records_device(
            self._h, C.c_void_p(d_record1), ptrs, nc, C.c_void_p(d_kf1_mp_of_kp), C.c_void_p(d_kf2_mp_of_kp), C.c_void_p(d_xyz),
            C.c_void_p(d_flags), int(n), C.c_void_p(d_Tcw1), C.c_void_p(d_Tcw2), C.c_void_p(d_rand_u32), int(n_hyp), C.byref(prm),
            C.c_void_p(d_match12), C.c_void_p(d_n_matches), C.c_void_p(d_out), C.c_void_p(stream or 0)))

    @staticmethod
    def sim3_iteration_limit(N, probability=0.99, min_inliers=20, max_iterations=300):
        """Sim3Solver::SetRansacParameters' iteration limit for N pairs (spfe_sim3_iteration_limit; host only)."""
        return int(load_library().spfe_sim3_iteration_limit(int(N), float(probability), int(min_inliers), int(max_iterations)))

    @staticmethod
    def decode_sim3_out(host_block, kmax, n_hyp):
        """One candidate's block: dict(the SIM3_FIELDS ints, k1 int32[N], count int32[n_hyp], return_idx int32[n_returns],
        T12 f32[n_hyp,13] (s, R, t), inliers bool[n_hyp,N] over the pairs, vbInliers bool[n_hyp,kmax] over k1).  A candidate
        with too few pairs (best_h < 0) was not evaluated: T12, inliers and vbInliers are None."""
        b = np.ascontiguousarray(host_block, np.uint8)
        o = sim3_offsets(int(kmax), int(n_hyp))
        out = {k: int(v) for k, v in zip(SIM3_FIELDS, b[:4 * len(SIM3_FIELDS)].view(np.int32))}
        N, nr = min(max(out["N"], 0), kmax), min(max(out["n_returns"], 0), n_hyp)
        out.update(k1=b[o["k1"]:o["k1"] + 4 * N].view(np.int32).copy(),
                   count=b[o["count"]:o["count"] + 4 * n_hyp].view(np.int32).copy(),
                   return_idx=b[o["return_idx"]:o["return_idx"] + 4 * nr].view(np.int32).copy(), T12=None, inliers=None,
                   vbInliers=None)
        if out["best_h"] >= 0:
            out["T12"] = b[o["T12"]:o["T12"] + 52 * n_hyp].view(np.float32).reshape(n_hyp, 13).copy()
            w = b[o["inliers"]:o["inliers"] + 8 * n_hyp * o["words"]].reshape(n_hyp, -1)
            out["inliers"] = np.unpackbits(w, axis=1, bitorder="little")[:, :N].astype(bool)
            out["vbInliers"] = np.zeros((n_hyp, kmax), bool)
            out["vbInliers"][:, out["k1"]] = out["inliers"]
        return out

    # -- the loop closer: SearchBySim3Override of a returning hypothesis (sp_matcher_loop.cpp:7-220) --
    @staticmethod
    def _guided_params(intr1, intr2, th, th_dist, min_factor, max_factor):
        return _GuidedParams(*[float(v) for v in tuple(intr1) + tuple(intr1 if intr2 is None else intr2)], float(th), float(th_dist),
                             float(min_factor), float(max_factor))

    def guided_out_bytes(self, kmax=None):
        return guided_offsets(self.layout.kmax if kmax is None else int(kmax))["out_bytes"]

    def search_by_sim3(self, kf1, kf2, xyz, flags, dist_range, desc, Tcw1, Tcw2, T12, seed12, intr1, intr2=None, th=7.5,
                       th_dist=0.7, min_factor=0.8, max_factor=1.2, fill=0):
        """The guided match on host arrays (spfe_search_by_sim3), synchronous.  kf1 / kf2: dict(kp_xy [K][2], occ [H/8][W/8],
        kp_desc [K][256] f32, kf_mp int32 [K]); T12 f32 [13] (s, R, t); seed12 int32 [K1].  -> (raw block over kmax =
        max(K1, K2, 1) on a background of `fill`, that kmax); decode_guided_out(block, kmax, K1, K2) unpacks it."""
        side = []
        for kf in (kf1, kf2):
            kp = np.ascontiguousarray(kf["kp_xy"], np.float32).reshape(-1, 2)
            occ = np.ascontiguousarray(kf["occ"], np.int16)
            assert occ.shape == (self.height // 8, self.width // 8)
            kd = np.ascontiguousarray(kf["kp_desc"], np.float32).reshape(-1, 256)
            m = np.ascontiguousarray(kf["kf_mp"], np.int32).reshape(-1)
            assert len(kd) == len(kp) == len(m)
            side.append((kp, occ, kd, m))
        p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        f = np.ascontiguousarray(flags, np.uint8).reshape(-1)
        r = np.ascontiguousarray(dist_range, np.float32).reshape(-1, 2)
        d = np.ascontiguousarray(desc, np.float32).reshape(-1, 256)
        assert len(p) == len(f) == len(r) == len(d)
        T1 = np.ascontiguousarray(Tcw1, np.float32).reshape(16)
        T2 = np.ascontiguousarray(Tcw2, np.float32).reshape(16)
        T = np.ascontiguousarray(T12, np.float32).reshape(13)
        sd = np.ascontiguousarray(seed12, np.int32).reshape(-1)
        K1, K2 = len(side[0][0]), len(side[1][0])
        assert len(sd) == K1
        kcap = max(K1, K2, 1)
        out = np.full(guided_offsets(kcap)["out_bytes"], fill, np.uint8)
        prm = self._guided_params(intr1, intr2, th, th_dist, min_factor, max_factor)
        ptr = lambda v: v.ctypes.data if v.size else None   # noqa: E731
        (kp1, occ1, kd1, m1), (kp2, occ2, kd2, m2) = side
        _check(self._lib.spfe_search_by_sim3(self._h, ptr(kp1), occ1.ctypes.data, ptr(kd1), K1, ptr(m1), ptr(kp2), occ2.ctypes.data,
                                             ptr(kd2), K2, ptr(m2), ptr(p), ptr(f), ptr(r), ptr(d), len(f), T1.ctypes.data,
                                             T2.ctypes.data, T.ctypes.data, ptr(sd), C.byref(prm), out.ctypes.data))
        return out, kcap

    def search_by_sim3_record_device(self, d_record1, d_record2, d_kf1_mp_of_kp, d_kf2_mp_of_kp, d_xyz, d_flags, d_dist_range,
                                     d_desc, n, d_Tcw1, d_Tcw2, d_T12, d_seed12, d_out, intr1, intr2=None, th=7.5, th_dist=0.7,
                                     min_factor=0.8, max_factor=1.2, stream=None):
        """The guided match between two resident records (spfe_search_by_sim3_record_device): d_T12 f32 [13], d_seed12 int32
        [kmax]; d_out receives guided_out_bytes() bytes (decode_guided_out)."""
        prm = self._guided_params(intr1, intr2, th, th_dist, min_factor, max_factor)
        _check(self._lib.spfe_search_by_sim3_record_device(
            self._h, C.c_void_p(d_record1), C.c_void_p(d_record2), C.c_void_p(d_kf1_mp_of_kp), C.c_void_p(d_kf2_mp_of_kp),
            C.c_void_p(d_xyz), C.c_void_p(d_flags), C.c_void_p(d_dist_range), C.c_void_p(d_desc), int(n), C.c_void_p(d_Tcw1),
            C.c_void_p(d_Tcw2), C.c_void_p(d_T12), C.c_void_p(d_seed12), C.byref(prm), C.c_void_p(d_out), C.c_void_p(stream or 0)))

    def loop_guided_match_records_device(self, d_record1, d_records2, jobs, d_kf1_mp_of_kp, d_kf2_mp_of_kp, d_xyz, d_flags,
                                         d_dist_range, d_desc, n, d_Tcw1, d_Tcw2, d_match12, d_verify_out, n_hyp, d_out, intr1,
                                         intr2=None, th=7.5, th_dist=0.7, min_factor=0.8, max_factor=1.2, stream=None):
        """The guided matches of several returning hypotheses as one call behind loop_verify_records_device
        (spfe_loop_guided_match_records_device): d_records2 is a sequence of device pointers, jobs a sequence of (candidate,
        hypothesis); T12 and the seed are read from the verify blocks on the device; job q writes d_out + q *
        guided_out_bytes()."""
        nc = len(d_records2)
        ptrs = (C.c_void_p * max(nc, 1))(*[int(p) for p in d_records2])
        jb = np.ascontiguousarray(jobs, np.int32).reshape(-1, 2)
        prm = self._guided_params(intr1, intr2, th, th_dist, min_factor, max_factor)
        _check(self._lib.spfe_loop_guided_match_records_device(
            self._h, C.c_void_p(d_record1), ptrs, nc, jb.ctypes.data if jb.size else None, len(jb), C.c_void_p(d_kf1_mp_of_kp),
            C.c_void_p(d_kf2_mp_of_kp), C.c_void_p(d_xyz), C.c_void_p(d_flags), C.c_void_p(d_dist_range), C.c_void_p(d_desc), int(n),
            C.c_void_p(d_Tcw1), C.c_void_p(d_Tcw2), C.c_void_p(d_match12), C.c_void_p(d_verify_out), int(n_hyp), C.byref(prm),
            C.c_void_p(d_out), C.c_void_p(stream or 0)))

    @staticmethod
    def decode_guided_out(host_block, kmax, K1, K2):
        """One job's block: dict(n_found, n_total, n_seed, status, match1 int32[K1], dist1 f32[K1], reason1 uint8[K1], match2
        int32[K2], dist2 f32[K2], reason2 uint8[K2], matches12 int32[kmax])."""
        b = np.ascontiguousarray(host_block, np.uint8)
        o = guided_offsets(int(kmax))
        out = {k: int(v) for k, v in zip(GUIDED_FIELDS, b[:4 * len(GUIDED_FIELDS)].view(np.int32))}
        out.update(match1=b[o["match1"]:o["match1"] + 4 * K1].view(np.int32).copy(),
                   match2=b[o["match2"]:o["match2"] + 4 * K2].view(np.int32).copy(),
                   dist1=b[o["dist1"]:o["dist1"] + 4 * K1].view(np.float32).copy(),
                   dist2=b[o["dist2"]:o["dist2"] + 4 * K2].view(np.float32).copy(),
                   matches12=b[o["matches12"]:o["matches12"] + 4 * kmax].view(np.int32).copy(),
                   reason1=b[o["reason1"]:o["reason1"] + K1].copy(), reason2=b[o["reason2"]:o["reason2"] + K2].copy())
        return out

    # -- the loop closer: SearchByProjectionLoop behind the accepted candidate (sp_matcher_loop.cpp:222-332) --
    @staticmethod
    def _loop_proj_params(fx, fy, cx, cy, th, th_dist, view_cos, min_factor, max_factor):
        return _LoopProjParams(float(fx), float(fy), float(cx), float(cy), float(th), float(th_dist), float(view_cos), float(min_factor),
                               float(max_factor))

    @staticmethod
    def loop_proj_out_bytes(n_cap):
        return loop_proj_offsets(int(n_cap))["out_bytes"]

    def search_loop_points(self, kp_xy, occ_grid, kp_desc, Scw, matched, point_id, xyz, normal, dist_range, desc, flags, fx, fy, cx, cy,
                           th=10.0, th_dist=0.7, view_cos=0.5, min_factor=0.8, max_factor=1.2):
        """The loop-point search on host arrays (spfe_search_loop_points), synchronous: -> dict(n_matched, kp_of_mp int32[n],
        best_dist f32[n], reason uint8[n], matched_idx int32[n_matched], matched int32[K]: the array after the call; the
        argument is not changed)."""
        kp = np.ascontiguousarray(kp_xy, np.float32).reshape(-1, 2)
        K = len(kp)
        occ = np.ascontiguousarray(occ_grid, np.int16)
        assert occ.shape == (self.height // 8, self.width // 8)
        kd = np.ascontiguousarray(kp_desc, np.float32).reshape(-1, 256)
        m = np.array(matched, np.int32).reshape(-1)[:K].copy()
        assert len(kd) >= K and len(m) == K
        S = np.ascontiguousarray(Scw, np.float32).reshape(16)
        ids = np.ascontiguousarray(point_id, np.int32).reshape(-1)
        n = len(ids)
        P = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        N = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
        R = np.ascontiguousarray(dist_range, np.float32).reshape(-1, 2)
        D = np.ascontiguousarray(desc, np.float32).reshape(-1, 256)
        F = np.ascontiguousarray(flags, np.uint8).reshape(-1)
        assert len(P) == n and len(N) == n and len(R) == n and len(D) == n and len(F) == n
        cap = max(n, 1)
        kom, bd, rs, mi = np.full(cap, -1, np.int32), np.zeros(cap, np.float32), np.zeros(cap, np.uint8), np.zeros(cap, np.int32)
        nm = C.c_int(0)
        prm = self._loop_proj_params(fx, fy, cx, cy, th, th_dist, view_cos, min_factor, max_factor)
        ptr = lambda v: v.ctypes.data if v.size else None   # noqa: E731
        _check(self._lib.spfe_search_loop_points(self._h, ptr(kp), occ.ctypes.data, ptr(kd), K, S.ctypes.data, ptr(m), ptr(ids), ptr(P),
                                                 ptr(N), ptr(R), ptr(D), ptr(F), n, C.byref(prm), kom.ctypes.data, bd.ctypes.data,
                                                 rs.ctypes.data, mi.ctypes.data, C.byref(nm)))
        return dict(n_matched=nm.value, kp_of_mp=kom[:n], best_dist=bd[:n], reason=rs[:n], matched_idx=mi[:nm.value].copy(), matched=m)

    def search_loop_points_record_device(self, d_record, d_Scw, d_matched, d_point_id, d_xyz, d_normal, d_dist_range, d_desc, d_flags,
                                         n, d_out, fx, fy, cx, cy, th=10.0, th_dist=0.7, view_cos=0.5, min_factor=0.8,
                                         max_factor=1.2, n_cap=None, stream=None):
        """The loop-point search of n points into ONE resident record (spfe_search_loop_points_record_device): d_matched int32
        [kmax] is in/out; d_out receives loop_proj_out_bytes(n_cap) bytes (decode_loop_proj_out); n_cap defaults to max(n, 1)."""
        prm = self._loop_proj_params(fx, fy, cx, cy, th, th_dist, view_cos, min_factor, max_factor)
        _check(self._lib.spfe_search_loop_points_record_device(
            self._h, C.c_void_p(d_record), C.c_void_p(d_Scw), C.c_void_p(d_matched), C.c_void_p(d_point_id), C.c_void_p(d_xyz),
            C.c_void_p(d_normal), C.c_void_p(d_dist_range), C.c_void_p(d_desc), C.c_void_p(d_flags), int(n),
            int(max(n, 1) if n_cap is None else n_cap), C.byref(prm), C.c_void_p(d_out), C.c_void_p(stream or 0)))

    @staticmethod
    def decode_loop_proj_out(host_block, n_cap):
        """The block over the capacity n_cap: dict(n_matched, n, status, kp_of_mp int32[n], best_dist f32[n], reason uint8[n],
        matched_idx int32[n_matched])."""
        b = np.ascontiguousarray(host_block, np.uint8)
        o = loop_proj_offsets(int(n_cap))
        out = {k: int(v) for k, v in zip(LOOPPROJ_FIELDS, b[:4 * len(LOOPPROJ_FIELDS)].view(np.int32))}
        n, nm = min(max(out["n"], 0), n_cap), min(max(out["n_matched"], 0), n_cap)
        out.update(kp_of_mp=b[LOOPPROJ_OFF_KP_OF_MP:LOOPPROJ_OFF_KP_OF_MP + 4 * n].view(np.int32).copy(),
                   best_dist=b[o["best_dist"]:o["best_dist"] + 4 * n].view(np.float32).copy(),
                   matched_idx=b[o["matched_idx"]:o["matched_idx"] + 4 * nm].view(np.int32).copy(),
                   reason=b[o["reason"]:o["reason"] + n].copy())
        return out

    # -- the loop closer: Optimizer::OptimizeSim3 behind the guided match (optimizer.cpp:1062-1252) --
    @staticmethod
    def _sim3opt_params(intr1, intr2, th2, fix_scale, iterations, min_kept, min_inliers):
        return _Sim3OptParams(*[float(v) for v in tuple(intr1) + tuple(intr1 if intr2 is None else intr2)], float(th2), int(fix_scale),
                              int(iterations), int(min_kept), int(min_inliers))

    def sim3opt_out_bytes(self, kmax=None):
        return sim3opt_offsets(self.layout.kmax if kmax is None else int(kmax))["out_bytes"]

    def sim3opt_lds_edge_capacity(self, kmax=None):
        """The most served correspondences whose edge data a solve over kmax keypoints (default: the handle's records) stages in
        LDS (spfe_sim3opt_lds_edge_capacity)."""
        return int(self._lib.spfe_sim3opt_lds_edge_capacity(self._h, 0 if kmax is None else int(kmax)))

    def optimize_sim3(self, kp_xy1, kf1_mp_of_kp, kp_xy2, kf2_mp_of_kp, xyz, flags, Tcw1, Tcw2, T12, matches12, intr1, intr2=None,
                      th2=10.0, fix_scale=0, iterations=5, min_kept=10, min_inliers=20, fill=0):
        """The Sim3 optimisation on host arrays (spfe_optimize_sim3), synchronous.  -> (raw block over kmax = max(K1, K2, 1) on
        a background of `fill`, that kmax); decode_sim3opt_out(block, kmax) unpacks it."""
        kp1 = np.ascontiguousarray(kp_xy1, np.float32).reshape(-1, 2)
        kp2 = np.ascontiguousarray(kp_xy2, np.float32).reshape(-1, 2)
        m1 = np.ascontiguousarray(kf1_mp_of_kp, np.int32).reshape(-1)
        m2 = np.ascontiguousarray(kf2_mp_of_kp, np.int32).reshape(-1)
        m12 = np.ascontiguousarray(matches12, np.int32).reshape(-1)
        p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        f = np.ascontiguousarray(flags, np.uint8).reshape(-1)
        K1, K2 = len(kp1), len(kp2)
        assert len(m1) == len(m12) == K1 and len(m2) == K2 and len(p) == len(f)
        T1 = np.ascontiguousarray(Tcw1, np.float32).reshape(16)
        T2 = np.ascontiguousarray(Tcw2, np.float32).reshape(16)
        T = np.ascontiguousarray(T12, np.float32).reshape(13)
        kcap = max(K1, K2, 1)
        out = np.full(sim3opt_offsets(kcap)["out_bytes"], fill, np.uint8)
        prm = self._sim3opt_params(intr1, intr2, th2, fix_scale, iterations, min_kept, min_inliers)
        ptr = lambda v: v.ctypes.data if v.size else None   # noqa: E731
        _check(self._lib.spfe_optimize_sim3(self._h, ptr(kp1), K1, ptr(m1), ptr(kp2), K2, ptr(m2), ptr(p), ptr(f), len(f),
                                            T1.ctypes.data, T2.ctypes.data, T.ctypes.data, ptr(m12), C.byref(prm), out.ctypes.data))
        return out, kcap

    def optimize_sim3_record_device(self, d_record1, d_record2, d_kf1_mp_of_kp, d_kf2_mp_of_kp, d_xyz, d_flags, n, d_Tcw1, d_Tcw2,
                                    d_T12, d_matches12, d_out, intr1, intr2=None, th2=10.0, fix_scale=0, iterations=5, min_kept=10,
                                    min_inliers=20, stream=None):
        """The Sim3 optimisation between two resident records (spfe_optimize_sim3_record_device): d_T12 f32 [13], d_matches12
        int32 [kmax]; d_out receives sim3opt_out_bytes() bytes (decode_sim3opt_out)."""
        prm = self._sim3opt_params(intr1, intr2, th2, fix_scale, iterations, min_kept, min_inliers)
        _check(self._lib.spfe_optimize_sim3_record_device(
            self._h, C.c_void_p(d_record1), C.c_void_p(d_record2), C.c_void_p(d_kf1_mp_of_kp), C.c_void_p(d_kf2_mp_of_kp),
            C.c_void_p(d_xyz), C.c_void_p(d_flags), int(n), C.c_void_p(d_Tcw1), C.c_void_p(d_Tcw2), C.c_void_p(d_T12),
            C.c_void_p(d_matches12), C.byref(prm), C.c_void_p(d_out), C.c_void_p(stream or 0)))

    def loop_optimize_sim3_records_device(self, d_record1, d_records2, jobs, d_kf1_mp_of_kp, d_kf2_mp_of_kp, d_xyz, d_flags, n,
                                          d_Tcw1, d_Tcw2, d_verify_out, n_hyp, d_guided_out, d_out, intr1, intr2=None, th2=10.0,
                                          fix_scale=0, iterations=5, min_kept=10, min_inliers=20, stream=None):
        """The solves of several hypotheses as one launch behind loop_guided_match_records_device
        (spfe_loop_optimize_sim3_records_device), with the same d_records2, jobs, d_verify_out, n_hyp and that call's d_out as
        d_guided_out: T12 and matches12 are read on the device; job q writes d_out + q * sim3opt_out_bytes()."""
        nc = len(d_records2)
        ptrs = (C.c_void_p * max(nc, 1))(*[int(p) for p in d_records2])
        jb = np.ascontiguousarray(jobs, np.int32).reshape(-1, 2)
        prm = self._sim3opt_params(intr1, intr2, th2, fix_scale, iterations, min_kept, min_inliers)
        _check(self._lib.spfe_loop_optimize_sim3_records_device(
            self._h, C.c_void_p(d_record1), ptrs, nc, jb.ctypes.data if jb.size else None, len(jb), C.c_void_p(d_kf1_mp_of_kp),
            C.c_void_p(d_kf2_mp_of_kp), C.c_void_p(d_xyz), C.c_void_p(d_flags), int(n), C.c_void_p(d_Tcw1), C.c_void_p(d_Tcw2),
            C.c_void_p(d_verify_out), int(n_hyp), C.c_void_p(d_guided_out), C.byref(prm), C.c_void_p(d_out), C.c_void_p(stream or 0)))

    @staticmethod
    def decode_sim3opt_out(host_block, kmax):
        """One solve's block: dict(n_corr, n_bad, n_in, accepted, iterations int32[2], trials int32[2], status, S12 f64[13],
        T12_out f32[13], Scw f32[4,4], matches12_out / matched int32[kmax], verdict uint8[kmax])."""
        b = np.ascontiguousarray(host_block, np.uint8)
        kmax = int(kmax)
        o = sim3opt_offsets(kmax)
        f = b[:4 * len(SIM3OPT_FIELDS)].view(np.int32)
        out = dict(n_corr=int(f[0]), n_bad=int(f[1]), n_in=int(f[2]), accepted=int(f[3]), iterations=f[4:6].copy(),
                   trials=f[6:8].copy(), status=int(f[8]))
        out.update(S12=b[o["S12"]:o["S12"] + 104].view(np.float64).copy(), T12_out=b[o["T12"]:o["T12"] + 52].view(np.float32).copy(),
                   Scw=b[o["Scw"]:o["Scw"] + 64].view(np.float32).reshape(4, 4).copy(),
                   matches12_out=b[o["matches12"]:o["matches12"] + 4 * kmax].view(np.int32).copy(),
                   matched=b[o["matched"]:o["matched"] + 4 * kmax].view(np.int32).copy(),
                   verdict=b[o["verdict"]:o["verdict"] + kmax].copy())
        return out

    # -- the mapper: Optimizer::LocalBundleAdjustment / BundleAdjustment (optimizer.cpp:445-774, :51-229) --
    @staticmethod
    def _ba_params(intr, schedule, iterations, robust, inv_sigma2):
        return BaParams(*[float(v) for v in intr], int(schedule), (C.c_int * 2)(int(iterations[0]), int(iterations[1])), int(robust),
                        float(inv_sigma2))

    def ba_lds_free_capacity(self):
        """The most free keyframes of a problem whose reduced camera system is kept in LDS (spfe_ba_lds_free_capacity)."""
        return int(self._lib.spfe_ba_lds_free_capacity(self._h))

    def bundle_adjust(self, edges, obs_xy, inv_sigma2, Tcw, fixed, xyz, intr, schedule=BA_LOCAL, iterations=(5, 10), robust=1,
                      inv_sigma2_full=1.0, stop=None, fill=0, out=None):
        """Bundle adjustment on host arrays (spfe_bundle_adjust), synchronous: edges int32 [E][3] (point, keyframe slot,
        keypoint) sorted by point, obs_xy / inv_sigma2 f32 [E][2], Tcw f32 [n_kf][16], fixed uint8 [n_kf], xyz f32 [n][3];
        stop: None or an int read when the call starts.  -> the raw block (on a background of `fill`, or `out` itself);
        decode_ba_out(block, n_kf, n, E) unpacks it."""
        e = np.ascontiguousarray(edges, np.int32).reshape(-1, 3)
        o = np.ascontiguousarray(obs_xy, np.float32).reshape(-1, 2)
        w = None if inv_sigma2 is None else np.ascontiguousarray(inv_sigma2, np.float32).reshape(-1, 2)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(-1, 16)
        f = np.ascontiguousarray(fixed, np.uint8).reshape(-1)
        p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        E, n_kf, n = len(e), len(T), len(p)
        assert len(o) == E and len(f) == n_kf and (w is None or len(w) == E)
        if out is None:
            out = np.full(ba_offsets(n_kf, n, E)["bytes"], fill, np.uint8)
        prm = self._ba_params(intr, schedule, iterations, robust, inv_sigma2_full)
        st = None if stop is None else np.array([int(stop)], np.int32)
        ptr = lambda v: v.ctypes.data if v is not None and v.size else None   # noqa: E731
        _check(self._lib.spfe_bundle_adjust(self._h, ptr(e), ptr(o), ptr(w), E, ptr(T), ptr(f), n_kf, ptr(p), n, C.byref(prm),
                                            ptr(st), out.ctypes.data))
        return out

    def local_ba_records_device(self, d_records, d_edges, E, d_Tcw, d_fixed, d_xyz, n, d_out, intr, schedule=BA_LOCAL,
                                iterations=(5, 10), robust=1, inv_sigma2_full=1.0, d_stop=None, stream=None):
        """Bundle adjustment on resident keyframe records (spfe_local_ba_records_device): d_records is a list of device
        pointers, the observations and cov2_inv are read from the records; d_out receives ba_offsets(len(d_records), n,
        E)["bytes"] bytes (decode_ba_out).  One launch, no host synchronisation."""
        nk = len(d_records)
        ptrs = (C.c_void_p * max(nk, 1))(*[int(p) for p in d_records])
        prm = self._ba_params(intr, schedule, iterations, robust, inv_sigma2_full)
        _check(self._lib.spfe_local_ba_records_device(
            self._h, ptrs, nk, C.c_void_p(d_edges or 0), int(E), C.c_void_p(d_Tcw), C.c_void_p(d_fixed), C.c_void_p(d_xyz or 0), int(n),
            C.byref(prm), C.c_void_p(d_stop or 0), C.c_void_p(d_out), C.c_void_p(stream or 0)))

    @staticmethod
    def decode_ba_out(host_block, n_kf, n, E):
        """The block of one problem: dict of the BA_FIELDS counts (iterations / trials as int32[2]), chi2_entry, chi2_exit,
        lambda_, Tcw_out f32 [n_kf,16], xyz_out f32 [n,3], verdict uint8 [E], erase_idx int32 [n_erase]."""
        b = np.ascontiguousarray(host_block, np.uint8)
        o = ba_offsets(int(n_kf), int(n), int(E))
        f = b[:4 * len(BA_FIELDS)].view(np.int32)
        d = b[o["chi2"]:o["chi2"] + 24].view(np.float64)
        out = dict(n_kf=int(f[0]), n_free=int(f[1]), n_points=int(f[2]), n_edges=int(f[3]), n_served=int(f[4]), iterations=f[5:7].copy(),
                   trials=f[7:9].copy(), n_level1=int(f[9]), n_erase=int(f[10]), status=int(f[11]), chi2_entry=float(d[0]),
                   chi2_exit=float(d[1]), lambda_=float(d[2]))
        ne = max(0, min(out["n_erase"], int(E)))
        out.update(Tcw_out=b[o["tcw"]:o["xyz"]].view(np.float32).reshape(n_kf, 16).copy(),
                   xyz_out=b[o["xyz"]:o["verdict"]].view(np.float32).reshape(n, 3).copy(),
                   verdict=b[o["verdict"]:o["verdict"] + E].copy(),
                   erase_idx=b[o["erase"]:o["erase"] + 4 * ne].view(np.int32).copy())
        return out

    # -- the map-point table: ComputeDistinctiveDescriptors / UpdateNormalAndDepth (mappoint.cpp:237-302, :322-364) --
    def mp_lds_obs_capacity(self, desc_elem_bytes=None):
        """The most good rows of a point that the workgroup path stages in LDS (spfe_mp_lds_obs_capacity); default: this
        handle's row format."""
        if desc_elem_bytes is None:
            desc_elem_bytes = 2 if self.desc_bf16 else 4
        cap = int(self._lib.spfe_mp_lds_obs_capacity(self._h, int(desc_elem_bytes)))
        if cap < 0:
            _check(cap)
        return cap

    @staticmethod
    def mp_out_bytes(m):
        return mp_offsets(int(m))["out_bytes"]

    def refresh_map_points_device(self, d_kf_records, d_kf_flags, d_Tcw, n_kf, d_point_idx, d_obs_start, d_obs, d_ref_slot, m, E,
                                  d_xyz, d_flags, d_normal, d_dist_range, d_desc, n_table, d_out, mode=MP_DESC | MP_NORMAL_DEPTH,
                                  level_scale=1.0, top_scale=1.0, stream=None):
        """The refresh of m listed points of the table from resident keyframe records (spfe_refresh_map_points_device):
        d_kf_records is a DEVICE array of n_kf record pointers; d_point_idx may be None (row i).  normal, dist_range and desc
        are written in place at the listed rows; d_out receives mp_out_bytes(m) bytes (decode_mp_out).  Two launches, no host
        synchronisation."""
        prm = MpParams(int(mode), float(level_scale), float(top_scale))
        v = lambda p: C.c_void_p(p or 0)   # noqa: E731
        _check(self._lib.spfe_refresh_map_points_device(
            self._h, v(d_kf_records), v(d_kf_flags), v(d_Tcw), int(n_kf), v(d_point_idx), v(d_obs_start), v(d_obs), v(d_ref_slot), int(m),
            int(E), v(d_xyz), v(d_flags), v(d_normal), v(d_dist_range), v(d_desc), int(n_table), C.byref(prm), v(d_out), v(stream)))

    def refresh_map_points(self, obs_start, obs_desc, obs_good, obs_Ow, ref_Ow, xyz, flags, normal, dist_range, desc, out=None,
                           mode=MP_DESC | MP_NORMAL_DEPTH, level_scale=1.0, top_scale=1.0, fill=0):
        """The refresh on host arrays (spfe_refresh_map_points), synchronous, the observations already gathered: obs_start
        int32 [m + 1], obs_desc f32 [E][256], obs_good uint8 [E], obs_Ow f32 [E][3], ref_Ow f32 [m][3], xyz f32 [m][3], flags
        uint8 [m].  normal f32 [m][3], dist_range f32 [m][2] and desc f32 [m][256] are written IN PLACE (C-contiguous float32
        arrays; rows that are not written keep their bytes).  -> the raw block (on a background of `fill`, or `out` itself)."""
        s = np.ascontiguousarray(obs_start, np.int32).reshape(-1)
        m = len(s) - 1
        d = np.ascontiguousarray(obs_desc, np.float32).reshape(-1, 256)
        g = np.ascontiguousarray(obs_good, np.uint8).reshape(-1)
        ow = np.ascontiguousarray(obs_Ow, np.float32).reshape(-1, 3)
        rw = np.ascontiguousarray(ref_Ow, np.float32).reshape(-1, 3)
        p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        f = np.ascontiguousarray(flags, np.uint8).reshape(-1)
        E = len(d)
        assert len(g) == E and len(ow) == E and len(rw) == m and len(p) == m and len(f) == m
        for a, w in ((normal, 3), (dist_range, 2), (desc, 256)):
            assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"] and a.size == m * w
        if out is None:
            out = np.full(mp_offsets(m)["out_bytes"], fill, np.uint8)
        prm = MpParams(int(mode), float(level_scale), float(top_scale))
        ptr = lambda v: v.ctypes.data if v is not None and v.size else None   # noqa: E731
        _check(self._lib.spfe_refresh_map_points(self._h, s.ctypes.data, ptr(d), ptr(g), ptr(ow), E, ptr(rw), ptr(p), ptr(f), m,
                                                 C.byref(prm), ptr(normal), ptr(dist_range), ptr(desc), out.ctypes.data))
        return out

    def gather_map_points_device(self, d_idx, n, d_xyz, d_flags, d_normal, d_dist_range, d_desc, n_table, d_point_id, d_list_xyz,
                                 d_list_normal, d_list_dist_range, d_list_desc, d_list_flags, stream=None):
        """Table rows d_idx int32 [n] -> the point list of the searches (spfe_gather_map_points_device): point_id, xyz, normal,
        dist_range, desc, flags, contiguous.  An index outside [0, n_table) gives a row of zeros (flags 0).  One launch."""
        v = lambda p: C.c_void_p(p or 0)   # noqa: E731
        _check(self._lib.spfe_gather_map_points_device(
            self._h, v(d_idx), int(n), v(d_xyz), v(d_flags), v(d_normal), v(d_dist_range), v(d_desc), int(n_table), v(d_point_id),
            v(d_list_xyz), v(d_list_normal), v(d_list_dist_range), v(d_list_desc), v(d_list_flags), v(stream)))

    # -- the loop closer: OptimizeEssentialGraph and the map corrections (optimizer.cpp:776-1060, loop_closer_vlad.cpp:575-606) --
    @staticmethod
    def essential_graph_envelope(flags, edges):
        """The symbolic step on the host (spfe_essential_graph_envelope; a pure function): flags uint8 [n], edges int32 [E][3]
        -> (n_blocks, n_unknown, first int32 [n_unknown])."""
        f = np.ascontiguousarray(flags, np.uint8).reshape(-1)
        e = np.ascontiguousarray(edges, np.int32).reshape(-1, 3)
        first = np.zeros(max(len(f), 1), np.int32)
        nu, nb = C.c_int(0), C.c_int(0)
        rc = load_library().spfe_essential_graph_envelope(len(f), f.ctypes.data if f.size else None, e.ctypes.data if e.size else None,
                                                          len(e), first.ctypes.data, C.byref(nu), C.byref(nb))
        if rc < 0:
            _check(rc)
        return nb.value, nu.value, first[:nu.value].copy()

    def essgraph_lds_panel_capacity(self):
        """The most block rows of a column panel the factorisation stages in LDS (spfe_essgraph_lds_panel_capacity)."""
        return int(self._lib.spfe_essgraph_lds_panel_capacity(self._h))

    def essential_graph_sim3_device(self, d_Tcw, d_opt_block, d_Tcw2, d_Twc, d_conn_slot, n_conn, cur_slot, d_Scw_est, d_Scw_meas, n,
                                    stream=None):
        """The graph's start values on the device (spfe_essential_graph_sim3_device): d_Scw_est / d_Scw_meas f64 [n][8]."""
        v = lambda p: C.c_void_p(p or 0)   # noqa: E731
        _check(self._lib.spfe_essential_graph_sim3_device(self._h, v(d_Tcw), v(d_opt_block), v(d_Tcw2), v(d_Twc), v(d_conn_slot),
                                                          int(n_conn), int(cur_slot), v(d_Scw_est), v(d_Scw_meas), int(n), v(stream)))

    @staticmethod
    def essential_graph_sim3(Tcw, S12, Tcw2, Twc, conn_slot, cur_slot=-1):
        """The same on the host (spfe_essential_graph_sim3; a pure function) -> (Scw_est, Scw_meas) f64 [n][8]."""
        T = np.ascontiguousarray(Tcw, np.float32).reshape(-1, 16)
        S = np.ascontiguousarray(S12, np.float64).reshape(13)
        T2 = np.ascontiguousarray(Tcw2, np.float32).reshape(16)
        Tw = np.ascontiguousarray(Twc, np.float32).reshape(16)
        cs = np.ascontiguousarray(conn_slot, np.int32).reshape(-1)
        n = len(T)
        est, meas = np.zeros((max(n, 1), 8)), np.zeros((max(n, 1), 8))
        _check(load_library().spfe_essential_graph_sim3(T.ctypes.data if n else None, S.ctypes.data, T2.ctypes.data, Tw.ctypes.data,
                                                        cs.ctypes.data if cs.size else None, len(cs), int(cur_slot), est.ctypes.data,
                                                        meas.ctypes.data, n))
        return est[:n], meas[:n]

    def optimize_essential_graph_device(self, d_Scw_est, d_Scw_meas, d_flags, n, d_edges, E, env_cap, d_out, iterations=20,
                                        fix_scale=0, lambda_init=1e-16, stream=None):
        """The pose graph over Sim3 on device arrays (spfe_optimize_essential_graph_device): d_out receives
        essgraph_offsets(n)["out_bytes"] bytes (decode_essgraph_out).  No host synchronisation."""
        prm = EssGraphParams(int(iterations), int(fix_scale), float(lambda_init))
        v = lambda p: C.c_void_p(p or 0)   # noqa: E731
        _check(self._lib.spfe_optimize_essential_graph_device(self._h, v(d_Scw_est), v(d_Scw_meas), v(d_flags), int(n), v(d_edges), int(E),
                                                              int(env_cap), C.byref(prm), v(d_out), v(stream)))

    def optimize_essential_graph(self, Scw_est, Scw_meas, flags, edges, env_cap=ESSGRAPH_MAX_BLOCKS, iterations=20, fix_scale=0,
                                 lambda_init=1e-16, fill=0, out=None):
        """The same on host arrays (spfe_optimize_essential_graph), synchronous: Scw_est / Scw_meas f64 [n][8] = q(x, y, z, w),
        t, s; flags uint8 [n] (bit 0 fixed); edges int32 [E][3] = (i, j, kind).  -> the raw block (on a background of `fill`, or
        `out` itself); decode_essgraph_out(block, n) unpacks it."""
        a = np.ascontiguousarray(Scw_est, np.float64).reshape(-1, 8)
        m = np.ascontiguousarray(Scw_meas, np.float64).reshape(-1, 8)
        f = np.ascontiguousarray(flags, np.uint8).reshape(-1)
        e = np.ascontiguousarray(edges, np.int32).reshape(-1, 3)
        n = len(a)
        assert len(m) == n and len(f) == n
        if out is None:
            out = np.full(essgraph_offsets(n)["out_bytes"], fill, np.uint8)
        prm = EssGraphParams(int(iterations), int(fix_scale), float(lambda_init))
        ptr = lambda v: v.ctypes.data if v is not None and v.size else None   # noqa: E731
        _check(self._lib.spfe_optimize_essential_graph(self._h, ptr(a), ptr(m), ptr(f), n, ptr(e), len(e), int(env_cap), C.byref(prm),
                                                       out.ctypes.data))
        return out

    @staticmethod
    def decode_essgraph_out(host_block, n):
        """The block of one optimisation: dict of the ESSGRAPH_FIELDS counts, chi2_initial, chi2_final, lambda_final, sim3 f64
        [n,8], Tiw f32 [n,16]."""
        b = np.ascontiguousarray(host_block, np.uint8)
        n = int(n)
        o = essgraph_offsets(n)
        f = b[:4 * len(ESSGRAPH_FIELDS)].view(np.int32)
        d = b[o["chi2"]:o["chi2"] + 24].view(np.float64)
        out = {k: int(v) for k, v in zip(ESSGRAPH_FIELDS, f)}
        out.update(chi2_initial=float(d[0]), chi2_final=float(d[1]), lambda_final=float(d[2]),
                   sim3=b[o["sim3"]:o["tiw"]].view(np.float64).reshape(n, 8).copy(),
                   Tiw=b[o["tiw"]:o["tiw"] + 64 * n].view(np.float32).reshape(n, 16).copy())
        return out

    def correct_map_points_device(self, d_S_from, d_S_to, n_kf, d_ref_slot, d_point_idx, m, d_xyz, d_flags, n_table, d_code,
                                  stream=None):
        """The map-point correction in place in the table (spfe_correct_map_points_device); d_point_idx may be None (row i).
        One launch, no host synchronisation; a row may be listed once."""
        v = lambda p: C.c_void_p(p or 0)   # noqa: E731
        _check(self._lib.spfe_correct_map_points_device(self._h, v(d_S_from), v(d_S_to), int(n_kf), v(d_ref_slot), v(d_point_idx), int(m),
                                                        v(d_xyz), v(d_flags), int(n_table), v(d_code), v(stream)))

    def correct_map_points(self, S_from, S_to, ref_slot, point_idx, xyz, flags, code=None):
        """The same on host arrays (spfe_correct_map_points), synchronous: xyz f32 [n_table][3] is corrected IN PLACE
        (C-contiguous float32).  -> code uint8 [m].  A row listed twice is refused."""
        a = np.ascontiguousarray(S_from, np.float64).reshape(-1, 8)
        b = np.ascontiguousarray(S_to, np.float64).reshape(-1, 8)
        r = np.ascontiguousarray(ref_slot, np.int32).reshape(-1)
        i = None if point_idx is None else np.ascontiguousarray(point_idx, np.int32).reshape(-1)
        f = np.ascontiguousarray(flags, np.uint8).reshape(-1)
        assert xyz.dtype == np.float32 and xyz.flags["C_CONTIGUOUS"] and xyz.size == 3 * len(f) and len(a) == len(b)
        m = len(r)
        if code is None:
            code = np.zeros(max(m, 1), np.uint8)
        ptr = lambda v: v.ctypes.data if v is not None and v.size else None   # noqa: E731
        _check(self._lib.spfe_correct_map_points(self._h, ptr(a), ptr(b), len(a), ptr(r), ptr(i), m, ptr(xyz), ptr(f), len(f),
                                                 code.ctypes.data))
        return code[:m]

    # -- the loop closer: the detection (loop_closer_vlad.cpp:42-118, :150-165) --
    @staticmethod
    def loopdet_out_bytes(n_slots):
        return loopdet_offsets(int(n_slots))["out_bytes"]

    def detect_loop_candidates_device(self, d_gdesc, dim, d_kf_flags, d_in_db, d_best_cov, n_slots, cur_slot, d_connected, n_conn,
                                      d_covisible, n_cov, d_out, min_score_init=0.2, min_score_floor=0.2, retain_ratio=0.75,
                                      stream=None):
        """The loop detection of the keyframe at cur_slot on the resident table (spfe_detect_loop_candidates_device): d_gdesc
        f32 [n_slots][dim], d_kf_flags / d_in_db uint8 [n_slots], d_best_cov int32 [n_slots][10], the two lists int32 (None when
        their count is 0).  d_out receives loopdet_out_bytes(n_slots) bytes (decode_loopdet_out).  Three launches, no host
        synchronisation."""
        prm = LoopdetParams(float(min_score_init), float(min_score_floor), float(retain_ratio))
        v = lambda p: C.c_void_p(p or 0)   # noqa: E731
        _check(self._lib.spfe_detect_loop_candidates_device(
            self._h, v(d_gdesc), int(dim), v(d_kf_flags), v(d_in_db), v(d_best_cov), int(n_slots), int(cur_slot), v(d_connected),
            int(n_conn), v(d_covisible), int(n_cov), C.byref(prm), v(d_out), v(stream)))

    def detect_loop_candidates(self, gdesc, kf_flags, in_db, best_cov, cur_slot, connected, covisible, min_score_init=0.2,
                               min_score_floor=0.2, retain_ratio=0.75, fill=0, out=None):
        """The same on host arrays (spfe_detect_loop_candidates), synchronous: gdesc f32 [n_slots][dim].  -> the raw block (on a
        background of `fill`, or `out` itself); decode_loopdet_out(block, n_slots) unpacks it."""
        g = np.ascontiguousarray(gdesc, np.float32)
        assert g.ndim == 2
        n, dim = g.shape
        f = np.ascontiguousarray(kf_flags, np.uint8).reshape(-1)
        d = np.ascontiguousarray(in_db, np.uint8).reshape(-1)
        bc = np.ascontiguousarray(best_cov, np.int32).reshape(-1, LOOPDET_NEIGH)
        cn = np.ascontiguousarray(connected, np.int32).reshape(-1)
        cv = np.ascontiguousarray(covisible, np.int32).reshape(-1)
        assert len(f) == n and len(d) == n and len(bc) == n
        if out is None:
            out = np.full(loopdet_offsets(n)["out_bytes"], fill, np.uint8)
        prm = LoopdetParams(float(min_score_init), float(min_score_floor), float(retain_ratio))
        ptr = lambda v: v.ctypes.data if v is not None and v.size else None   # noqa: E731
        _check(self._lib.spfe_detect_loop_candidates(self._h, ptr(g), dim, ptr(f), ptr(d), ptr(bc), n, int(cur_slot), ptr(cn), len(cn),
                                                     ptr(cv), len(cv), C.byref(prm), out.ctypes.data))
        return out

    @staticmethod
    def decode_loopdet_out(host_block, n_slots):
        """The block of one detection: dict of the LOOPDET_FIELDS counts and the LOOPDET_SCORES (numpy float32), score f32
        [n_slots], pass_slot / best_slot int32 [n_pass], acc_score f32 [n_pass], cand_slot int32 [n_cand], cand_acc f32 [n_cand],
        first_pos int32 [n_slots], role uint8 [n_slots]."""
        b = np.ascontiguousarray(host_block, np.uint8)
        n = int(n_slots)
        o = loopdet_offsets(n)
        out = {k: int(v) for k, v in zip(LOOPDET_FIELDS, b[:16].view(np.int32))}
        out.update({k: v for k, v in zip(LOOPDET_SCORES, b[16:32].view(np.float32).copy())})
        npass, nc = max(0, min(out["n_pass"], n)), max(0, min(out["n_cand"], n))
        at = lambda k, cnt, t: b[o[k]:o[k] + 4 * cnt].view(t).copy()   # noqa: E731
        out.update(score=at("score", n, np.float32), pass_slot=at("pass_slot", npass, np.int32),
                   acc_score=at("acc_score", npass, np.float32), best_slot=at("best_slot", npass, np.int32),
                   cand_slot=at("cand_slot", nc, np.int32), cand_acc=at("cand_acc", nc, np.float32),
                   first_pos=at("first_pos", n, np.int32), role=b[o["role"]:o["role"] + n].copy())
        return out

    # -- the tracker's local map (tracker.cpp:834-984) --
    @staticmethod
    def localmap_out_bytes(n_slots, point_cap, n_kp):
        return localmap_offsets(n_slots, point_cap, n_kp)["out_bytes"]

    def localmap_lds_point_capacity(self):
        """Points whose weight table the vote kernel holds in LDS (spfe_localmap_lds_point_capacity)."""
        cap = int(self._lib.spfe_localmap_lds_point_capacity(self._h))
        if cap < 0:
            _check(cap)
        return cap

    def update_local_map_resident(self, d_kf_mp_of_kp, kp_stride, d_kf_flags, d_best_cov, n_best, d_parent, n_slots, d_mp_flags,
                                  n_table, d_mp_of_kp, n_kp, d_out, point_cap, max_keyframes=80, stream=None):
        """UpdateLocalMap on the resident arrays (spfe_update_local_map_resident): d_kf_mp_of_kp int32 [n_slots][kp_stride],
        d_kf_flags uint8 [n_slots], d_best_cov int32 [n_slots][n_best], d_parent int32 [n_slots], d_mp_flags uint8 [n_table],
        d_mp_of_kp int32 [n_kp] (None when n_kp is 0).  d_out receives localmap_out_bytes(n_slots, point_cap, n_kp) bytes
        (decode_localmap_out).  Seven launches, no host synchronisation."""
        prm = LocalmapParams(int(max_keyframes), int(point_cap))
        v = lambda p: C.c_void_p(p or 0)   # noqa: E731
        _check(self._lib.spfe_update_local_map_resident(
            self._h, v(d_kf_mp_of_kp), int(kp_stride), v(d_kf_flags), v(d_best_cov), int(n_best), v(d_parent), int(n_slots),
            v(d_mp_flags), int(n_table), v(d_mp_of_kp), int(n_kp), C.byref(prm), v(d_out), v(stream)))

    def count_shared_points_resident(self, d_kf_mp_of_kp, kp_stride, n_slots, d_mp_flags, n_table, d_mp_of_kp, d_outlier, n_kp,
                                     d_votes, d_total, stream=None):
        """Votes and total per slot alone (spfe_count_shared_points_resident): d_outlier uint8 [n_kp] or None; d_votes and d_total
        int32 [n_slots].  Three launches."""
        v = lambda p: C.c_void_p(p or 0)   # noqa: E731
        _check(self._lib.spfe_count_shared_points_resident(
            self._h, v(d_kf_mp_of_kp), int(kp_stride), int(n_slots), v(d_mp_flags), int(n_table), v(d_mp_of_kp), v(d_outlier),
            int(n_kp), v(d_votes), v(d_total), v(stream)))

    def local_map_rows_resident(self, d_point_idx, point_cap, d_mp_of_kp_list, n_kp, d_mp_of_kp_rows, stream=None):
        """List positions back into table rows (spfe_local_map_rows_resident).  One launch."""
        v = lambda p: C.c_void_p(p or 0)   # noqa: E731
        _check(self._lib.spfe_local_map_rows_resident(self._h, v(d_point_idx), int(point_cap), v(d_mp_of_kp_list), int(n_kp),
                                                      v(d_mp_of_kp_rows), v(stream)))

    def update_local_map(self, kf_mp_of_kp, kf_flags, best_cov, parent, mp_flags, mp_of_kp, point_cap, max_keyframes=80, fill=0,
                         out=None):
        """The same on host arrays (spfe_update_local_map), synchronous: kf_mp_of_kp int32 [n_slots][kp_stride], best_cov int32
        [n_slots][n_best].  -> the raw block (every byte written); decode_localmap_out unpacks it."""
        rows = np.ascontiguousarray(kf_mp_of_kp, np.int32)
        bc = np.ascontiguousarray(best_cov, np.int32)
        assert rows.ndim == 2 and bc.ndim == 2
        n, stride = rows.shape
        f = np.ascontiguousarray(kf_flags, np.uint8).reshape(-1)
        par = np.ascontiguousarray(parent, np.int32).reshape(-1)
        mf = np.ascontiguousarray(mp_flags, np.uint8).reshape(-1)
        mk = np.ascontiguousarray(mp_of_kp, np.int32).reshape(-1)
        assert len(f) == n and len(par) == n and len(bc) == n
        if out is None:
            out = np.full(localmap_offsets(n, point_cap, len(mk))["out_bytes"], fill, np.uint8)
        prm = LocalmapParams(int(max_keyframes), int(point_cap))
        ptr = lambda v: v.ctypes.data if v is not None and v.size else None   # noqa: E731
        _check(self._lib.spfe_update_local_map(self._h, ptr(rows), stride, ptr(f), ptr(bc), bc.shape[1], ptr(par), n, ptr(mf), len(mf),
                                               ptr(mk), len(mk), C.byref(prm), out.ctypes.data))
        return out

    @staticmethod
    def decode_localmap_out(host_block, n_slots, point_cap, n_kp):
        """The block of one call: dict of the LOCALMAP_FIELDS, local_kf int32 [n_local_kf], votes / total int32 [n_slots],
        point_idx int32 [point_cap] (whole: -1 behind n_points), mp_of_kp_list int32 [n_kp]."""
        b = np.ascontiguousarray(host_block, np.uint8)
        n, cap, k = int(n_slots), int(point_cap), int(n_kp)
        o = localmap_offsets(n, cap, k)
        out = {name: int(v) for name, v in zip(LOCALMAP_FIELDS, b[:28].view(np.int32))}
        at = lambda key, cnt: b[o[key]:o[key] + 4 * cnt].view(np.int32).copy()   # noqa: E731
        out.update(local_kf=at("local_kf", max(0, min(out["n_local_kf"], n))), votes=at("votes", n), total=at("total", n),
                   point_idx=at("point_idx", cap), mp_of_kp_list=at("mp_of_kp_list", k))
        return out

    # -- the covisibility graph (keyframe.cpp:577-612, :757-849) --
    @staticmethod
    def covis_out_bytes(n_slots, conn_cap):
        return covis_offsets(n_slots, conn_cap)["out_bytes"]

    def covis_reset_slots_resident(self, graph, first_slot, n, stream=None):
        """The preset of the slots [first_slot, first_slot + n) of the resident graph state (spfe_covis_reset_slots_resident): counts
        0, rows -1 / 0, parent -1, first_conn 1.  graph: a CovisGraph of device pointers (covis_graph).  One launch."""
        _check(self._lib.spfe_covis_reset_slots_resident(self._h, C.byref(graph), int(first_slot), int(n), C.c_void_p(stream or 0)))

    def update_connections_resident(self, graph, d_kf_mp_of_kp, kp_stride, d_kf_flags, d_mp_flags, n_table, cur_slot, d_out, th=15,
                                    origin_slot=-1, d_best_cov_a=None, n_best_a=20, d_best_cov_b=None, n_best_b=10, stream=None):
        """KeyFrame::UpdateConnections of the keyframe at cur_slot on the resident arrays (spfe_update_connections_resident): graph a
        CovisGraph of device pointers, d_kf_mp_of_kp int32 [n_slots][kp_stride], d_kf_flags uint8 [n_slots], d_mp_flags uint8
        [n_table], the two best_cov tables int32 [n_slots][n_best] or None.  d_out receives covis_out_bytes(n_slots, conn_cap)
        bytes (decode_covis_out).  Five launches, no host synchronisation."""
        prm = CovisParams(int(th), int(origin_slot))
        v = lambda p: C.c_void_p(p or 0)   # noqa: E731
        _check(self._lib.spfe_update_connections_resident(
            self._h, C.byref(graph), v(d_kf_mp_of_kp), int(kp_stride), v(d_kf_flags), v(d_mp_flags), int(n_table), int(cur_slot),
            C.byref(prm), v(d_best_cov_a), int(n_best_a), v(d_best_cov_b), int(n_best_b), v(d_out), v(stream)))

    def update_connections(self, state, kf_mp_of_kp, kf_flags, mp_flags, cur_slot, th=15, origin_slot=-1, best_cov_a=None,
                           best_cov_b=None, fill=0, out=None):
        """The same on host arrays (spfe_update_connections), synchronous: state is a dict of the COVIS_STATE arrays (C-contiguous,
        conn / ord rows int32 [n_slots][conn_cap], first_conn uint8), best_cov_a / best_cov_b int32 [n_slots][n_best] or None; all
        of them are updated IN PLACE.  -> the raw block (every byte written); decode_covis_out unpacks it."""
        rows = np.ascontiguousarray(kf_mp_of_kp, np.int32)
        assert rows.ndim == 2
        n, stride = rows.shape
        f = np.ascontiguousarray(kf_flags, np.uint8).reshape(-1)
        mf = np.ascontiguousarray(mp_flags, np.uint8).reshape(-1)
        cap = state["conn_slot"].shape[1]
        for k in COVIS_STATE:
            a = state[k]
            assert a.flags["C_CONTIGUOUS"] and a.dtype == (np.uint8 if k == "first_conn" else np.int32) and a.shape[0] == n, k
        for tab in (best_cov_a, best_cov_b):
            assert tab is None or (tab.dtype == np.int32 and tab.flags["C_CONTIGUOUS"] and tab.ndim == 2 and tab.shape[0] == n)
        assert len(f) == n
        if out is None:
            out = np.full(covis_offsets(n, cap)["out_bytes"], fill, np.uint8)
        g = covis_graph([state[k].ctypes.data for k in COVIS_STATE], n, cap)
        prm = CovisParams(int(th), int(origin_slot))
        ptr = lambda v: v.ctypes.data if v is not None and v.size else None   # noqa: E731
        _check(self._lib.spfe_update_connections(self._h, C.byref(g), ptr(rows), stride, ptr(f), ptr(mf), len(mf), int(cur_slot),
                                                 C.byref(prm), ptr(best_cov_a), 1 if best_cov_a is None else best_cov_a.shape[1],
                                                 ptr(best_cov_b), 1 if best_cov_b is None else best_cov_b.shape[1], out.ctypes.data))
        return out

    @staticmethod
    def decode_covis_out(host_block, n_slots, conn_cap):
        """The block of one call: dict of the COVIS_FIELDS, counter int32 [n_slots], linked_slot / linked_code int32 [n_linked]."""
        b = np.ascontiguousarray(host_block, np.uint8)
        n, cap = int(n_slots), int(conn_cap)
        o = covis_offsets(n, cap)
        out = {name: int(v) for name, v in zip(COVIS_FIELDS, b[:32].view(np.int32))}
        at = lambda key, cnt: b[o[key]:o[key] + 4 * cnt].view(np.int32).copy()   # noqa: E731
        nl = max(0, min(out["n_linked"], cap))
        out.update(counter=at("counter", n), linked_slot=at("linked_slot", nl), linked_code=at("linked_code", nl))
        return out

    # -- keyframe culling (local_mapper.cpp:979-1032, keyframe.cpp:911-997) --
    @staticmethod
    def cull_out_bytes(n_slots, conn_cap, bad_cap):
        return cull_offsets(n_slots, conn_cap, bad_cap)["out_bytes"]

    def count_observations_resident(self, d_kf_mp_of_kp, kp_stride, d_kf_flags, n_slots, d_mp_nobs, n_table, stream=None):
        """MapPoint::Observations() of every point from the rows (spfe_count_observations_resident): d_mp_nobs int32 [n_table], the
        whole array written.  Two launches."""
        v = lambda p: C.c_void_p(p or 0)   # noqa: E731
        _check(self._lib.spfe_count_observations_resident(self._h, v(d_kf_mp_of_kp), int(kp_stride), v(d_kf_flags), int(n_slots),
                                                          v(d_mp_nobs), int(n_table), v(stream)))

    def cull_keyframes_resident(self, graph, d_kf_mp_of_kp, kp_stride, d_kf_flags, d_mp_flags, d_mp_nobs, n_table, cur_slot, d_out,
                                th_obs=3, cov_ratio=0.9, origin_slot=-1, bad_cap=0, d_best_cov_a=None, n_best_a=20,
                                d_best_cov_b=None, n_best_b=10, stream=None):
        """The cull loop over the covisible keyframes of cur_slot with SetBadFlag on the resident arrays
        (spfe_cull_keyframes_resident).  WRITES d_kf_mp_of_kp, d_kf_flags, d_mp_flags, d_mp_nobs, the graph state and the tables.
        d_out receives cull_out_bytes(n_slots, conn_cap, bad_cap) bytes (decode_cull_out).  Four launches, no host
        synchronisation."""
        prm = CullParams(int(th_obs), float(cov_ratio), int(origin_slot), int(bad_cap))
        v = lambda p: C.c_void_p(p or 0)   # noqa: E731
        _check(self._lib.spfe_cull_keyframes_resident(
            self._h, C.byref(graph), v(d_kf_mp_of_kp), int(kp_stride), v(d_kf_flags), v(d_mp_flags), v(d_mp_nobs), int(n_table),
            int(cur_slot), C.byref(prm), v(d_best_cov_a), int(n_best_a), v(d_best_cov_b), int(n_best_b), v(d_out), v(stream)))

    def cull_keyframes(self, state, kf_mp_of_kp, kf_flags, mp_flags, mp_nobs, cur_slot, th_obs=3, cov_ratio=0.9, origin_slot=-1,
                       bad_cap=0, best_cov_a=None, best_cov_b=None, fill=0, out=None):
        """The same on host arrays (spfe_cull_keyframes), synchronous: state is a dict of the COVIS_STATE arrays, kf_mp_of_kp int32
        [n_slots][kp_stride], kf_flags uint8 [n_slots], mp_flags uint8 [n_table], mp_nobs int32 [n_table], the tables int32
        [n_slots][n_best] or None; ALL of them must be C-contiguous arrays of those types and are updated IN PLACE.  -> the raw
        block (every byte written); decode_cull_out unpacks it."""
        rows = kf_mp_of_kp
        assert rows.ndim == 2 and rows.dtype == np.int32 and rows.flags["C_CONTIGUOUS"]
        n, stride = rows.shape
        cap = state["conn_slot"].shape[1]
        for k in COVIS_STATE:
            a = state[k]
            assert a.flags["C_CONTIGUOUS"] and a.dtype == (np.uint8 if k == "first_conn" else np.int32) and a.shape[0] == n, k
        for arr, dt in ((kf_flags, np.uint8), (mp_flags, np.uint8), (mp_nobs, np.int32)):
            assert arr.dtype == dt and arr.flags["C_CONTIGUOUS"] and arr.ndim == 1
        assert len(kf_flags) == n and len(mp_nobs) == len(mp_flags)
        for tab in (best_cov_a, best_cov_b):
            assert tab is None or (tab.dtype == np.int32 and tab.flags["C_CONTIGUOUS"] and tab.ndim == 2 and tab.shape[0] == n)
        if out is None:
            out = np.full(cull_offsets(n, cap, bad_cap)["out_bytes"], fill, np.uint8)
        g = covis_graph([state[k].ctypes.data for k in COVIS_STATE], n, cap)
        prm = CullParams(int(th_obs), float(cov_ratio), int(origin_slot), int(bad_cap))
        ptr = lambda v: v.ctypes.data if v is not None and v.size else None   # noqa: E731
        _check(self._lib.spfe_cull_keyframes(self._h, C.byref(g), ptr(rows), stride, ptr(kf_flags), ptr(mp_flags), ptr(mp_nobs),
                                             len(mp_flags), int(cur_slot), C.byref(prm), ptr(best_cov_a),
                                             1 if best_cov_a is None else best_cov_a.shape[1], ptr(best_cov_b),
                                             1 if best_cov_b is None else best_cov_b.shape[1], out.ctypes.data))
        return out

    @staticmethod
    def decode_cull_out(host_block, n_slots, conn_cap, bad_cap):
        """The block of one call: dict of the CULL_FIELDS, entry_slot / entry_code / entry_pass / entry_mps / entry_red int32
        [n_listed], culled_slot [n_culled], touched_slot [n_touched], event_child / event_parent [n_events], bad_point
        [n_bad_stored]."""
        b = np.ascontiguousarray(host_block, np.uint8)
        n, cap, bc = int(n_slots), int(conn_cap), int(bad_cap)
        o = cull_offsets(n, cap, bc)
        out = {name: int(v) for name, v in zip(CULL_FIELDS, b[:40].view(np.int32))}
        at = lambda key, cnt: b[o[key]:o[key] + 4 * cnt].view(np.int32).copy()   # noqa: E731
        nl = max(0, min(out["n_listed"], cap))
        for k in ("entry_slot", "entry_code", "entry_pass", "entry_mps", "entry_red"):
            out[k] = at(k, nl)
        out.update(culled_slot=at("culled_slot", max(0, min(out["n_culled"], cap))),
                   touched_slot=at("touched_slot", max(0, min(out["n_touched"], n))),
                   event_child=at("event_child", max(0, min(out["n_events"], n))),
                   event_parent=at("event_parent", max(0, min(out["n_events"], n))),
                   bad_point=at("bad_point", max(0, min(out["n_bad_stored"], bc))))
        return out

    # -- map-point culling and its resident state (local_mapper.cpp:281-310, :770-787, tracker.cpp:772-807) --
    @staticmethod
    def mpcull_out_bytes(recent_cap, bad_cap):
        return mpcull_offsets(recent_cap, bad_cap)["out_bytes"]

    def mp_life_reset_resident(self, life, first_row, n_rows, reset_list=False, stream=None):
        """The preset of the table rows [first_row, first_row + n_rows) of the state and, with reset_list, of the recent list
        (spfe_mp_life_reset_resident).  life: an MpLife of device pointers (mp_life).  One launch."""
        _check(self._lib.spfe_mp_life_reset_resident(self._h, C.byref(life), int(first_row), int(n_rows), int(bool(reset_list)),
                                                     C.c_void_p(stream or 0)))

    def admit_map_points_resident(self, life, d_tri_out, n_neigh, d_neigh_slot, cur_slot, cur_kf_id, d_kf_mp_of_kp, kp_stride, n_slots,
                                  d_xyz, d_out, stream=None):
        """The points of one create_map_points_record_device call (its d_out, n_neigh blocks) into the rows, the table's xyz and
        the state, all or nothing (spfe_admit_map_points_resident).  d_out receives ADMIT_OUT_BYTES (decode_admit_out).  Two
        launches, no host synchronisation."""
        v = lambda p: C.c_void_p(p or 0)   # noqa: E731
        _check(self._lib.spfe_admit_map_points_resident(self._h, C.byref(life), v(d_tri_out), int(n_neigh), v(d_neigh_slot), int(cur_slot),
                                                        int(cur_kf_id), v(d_kf_mp_of_kp), int(kp_stride), int(n_slots), v(d_xyz),
                                                        v(d_out), v(stream)))

    def track_statistics_resident(self, life, d_mp_of_kp_entry, d_mp_of_kp_after, n_kp, d_point_idx, point_cap, d_proj_out, d_pose_out,
                                  d_out, stream=None):
        """IncreaseVisible / IncreaseFound of one tracked frame on the resident counters (spfe_track_statistics_resident), behind
        track_local_map_record_device and local_map_rows_resident.  d_out receives MPSTAT_OUT_BYTES.  One launch."""
        v = lambda p: C.c_void_p(p or 0)   # noqa: E731
        _check(self._lib.spfe_track_statistics_resident(self._h, C.byref(life), v(d_mp_of_kp_entry), v(d_mp_of_kp_after), int(n_kp),
                                                        v(d_point_idx), int(point_cap), v(d_proj_out), v(d_pose_out), v(d_out),
                                                        v(stream)))

    def cull_map_points_resident(self, life, d_kf_mp_of_kp, kp_stride, d_kf_flags, n_slots, cur_kf_id, d_out, th_obs=2,
                                 found_ratio=0.25, bad_cap=0, stream=None):
        """The cull loop over the recent list (spfe_cull_map_points_resident).  WRITES d_mp_flags, d_recent, d_recent_n and
        d_kf_mp_of_kp.  d_out receives mpcull_out_bytes(recent_cap, bad_cap) bytes (decode_mpcull_out).  Four launches, no host
        synchronisation."""
        prm = MpCullParams(int(cur_kf_id), int(th_obs), float(found_ratio), int(bad_cap))
        v = lambda p: C.c_void_p(p or 0)   # noqa: E731
        _check(self._lib.spfe_cull_map_points_resident(self._h, C.byref(life), v(d_kf_mp_of_kp), int(kp_stride), v(d_kf_flags),
                                                       int(n_slots), C.byref(prm), v(d_out), v(stream)))

    @staticmethod
    def _host_life(state):
        """state: dict of the MP_LIFE_STATE arrays (C-contiguous; flags uint8, the others int32, recent_n of one entry)"""
        for k in MP_LIFE_STATE:
            a = state[k]
            assert a.flags["C_CONTIGUOUS"] and a.dtype == (np.uint8 if k == "flags" else np.int32) and a.ndim == 1, k
        n_table = len(state["flags"])
        assert all(len(state[k]) == n_table for k in ("nobs", "found", "visible", "first_kf")) and len(state["recent_n"]) == 1
        return mp_life([state[k].ctypes.data for k in MP_LIFE_STATE], n_table, len(state["recent"]))

    def admit_map_points(self, state, tri_out, n_neigh, neigh_slot, cur_slot, cur_kf_id, kf_mp_of_kp, xyz, fill=0):
        """The same on host arrays (spfe_admit_map_points), synchronous: state as in _host_life, tri_out the n_neigh blocks as
        downloaded (uint8), kf_mp_of_kp int32 [n_slots][kp_stride] and xyz float32 [n_table][3] updated IN PLACE.  -> the raw block."""
        rows = kf_mp_of_kp
        assert rows.ndim == 2 and rows.dtype == np.int32 and rows.flags["C_CONTIGUOUS"]
        assert xyz.dtype == np.float32 and xyz.flags["C_CONTIGUOUS"] and xyz.shape == (len(state["flags"]), 3)
        tri = np.ascontiguousarray(tri_out, np.uint8)
        assert tri.size >= int(n_neigh) * self.tri_out_bytes()
        ns = np.ascontiguousarray(neigh_slot, np.int32)
        assert len(ns) >= int(n_neigh)
        out = np.full(ADMIT_OUT_BYTES, fill, np.uint8)
        life = self._host_life(state)
        _check(self._lib.spfe_admit_map_points(self._h, C.byref(life), tri.ctypes.data, int(n_neigh), ns.ctypes.data, int(cur_slot),
                                               int(cur_kf_id), rows.ctypes.data, rows.shape[1], rows.shape[0], xyz.ctypes.data,
                                               out.ctypes.data))
        return out

    def track_statistics(self, state, mp_of_kp_entry, mp_of_kp_after, point_idx, in_view, outlier, fill=0):
        """The same on host arrays (spfe_track_statistics), synchronous: found and visible of state updated IN PLACE; in_view uint8
        [point_cap], outlier uint8 [n_kp].  -> the raw block."""
        e, a = np.ascontiguousarray(mp_of_kp_entry, np.int32), np.ascontiguousarray(mp_of_kp_after, np.int32)
        pi, iv, ol = np.ascontiguousarray(point_idx, np.int32), np.ascontiguousarray(in_view, np.uint8), np.ascontiguousarray(outlier, np.uint8)
        assert len(e) == len(a) == len(ol) and len(pi) == len(iv)
        out = np.full(MPSTAT_OUT_BYTES, fill, np.uint8)
        life = self._host_life(state)
        ptr = lambda v: v.ctypes.data if v.size else None   # noqa: E731
        _check(self._lib.spfe_track_statistics(self._h, C.byref(life), ptr(e), ptr(a), len(e), ptr(pi), len(pi), ptr(iv), ptr(ol),
                                               out.ctypes.data))
        return out

    def cull_map_points(self, state, kf_mp_of_kp, kf_flags, cur_kf_id, th_obs=2, found_ratio=0.25, bad_cap=0, fill=0):
        """The same on host arrays (spfe_cull_map_points), synchronous: state and kf_mp_of_kp updated IN PLACE.  -> the raw block
        (every byte written); decode_mpcull_out unpacks it."""
        rows = kf_mp_of_kp
        assert rows.ndim == 2 and rows.dtype == np.int32 and rows.flags["C_CONTIGUOUS"]
        assert kf_flags.dtype == np.uint8 and kf_flags.flags["C_CONTIGUOUS"] and len(kf_flags) == rows.shape[0]
        life = self._host_life(state)
        out = np.full(mpcull_offsets(len(state["recent"]), bad_cap)["out_bytes"], fill, np.uint8)
        prm = MpCullParams(int(cur_kf_id), int(th_obs), float(found_ratio), int(bad_cap))
        _check(self._lib.spfe_cull_map_points(self._h, C.byref(life), rows.ctypes.data, rows.shape[1], kf_flags.ctypes.data, rows.shape[0],
                                              C.byref(prm), out.ctypes.data))
        return out

    # -- a new keyframe on resident state: the insertion of its row, the observation lists (local_mapper.cpp:255-272) --
    @staticmethod
    def newkf_out_bytes(n_kp, kp_stride):
        return newkf_offsets(n_kp, kp_stride)["out_bytes"]

    @staticmethod
    def listobs_out_bytes(m, obs_cap):
        return listobs_offsets(m, obs_cap)["out_bytes"]

    def insert_keyframe_resident(self, life, d_frame_mp_of_kp, n_kp, cur_slot, d_kf_mp_of_kp, kp_stride, d_kf_flags, n_slots, d_out,
                                 d_kf_record=None, d_desc_track=None, stream=None):
        """ProcessNewKeyFrame without its refresh (spfe_insert_keyframe_resident): the frame's holders into row cur_slot, nobs, the
        flags, the recent list and — with both d_kf_record and d_desc_track — the track descriptors, all or nothing.  life: an
        MpLife of device pointers (found, visible and first_kf may be null).  d_out receives newkf_out_bytes(n_kp, kp_stride)
        bytes (decode_newkf_out).  Four launches, no host synchronisation."""
        v = lambda p: C.c_void_p(p or 0)   # noqa: E731
        _check(self._lib.spfe_insert_keyframe_resident(self._h, C.byref(life), v(d_frame_mp_of_kp), int(n_kp), int(cur_slot),
                                                       v(d_kf_mp_of_kp), int(kp_stride), v(d_kf_flags), int(n_slots), v(d_kf_record),
                                                       v(d_desc_track), v(d_out), v(stream)))

    def list_observations_resident(self, d_point_idx, first_row, m, d_kf_mp_of_kp, kp_stride, d_kf_flags, n_slots, d_mp_ref_slot,
                                   n_table, obs_cap, d_out, stream=None):
        """The observations of m listed points from one scan of the rows (spfe_list_observations_resident): d_point_idx int32 [m],
        or None: entry i names row first_row + i.  d_out receives listobs_out_bytes(m, obs_cap) bytes (decode_listobs_out);
        refresh_map_points_device takes pointers into it (listobs_offsets) with E = obs_cap.  Six launches, no host
        synchronisation."""
        v = lambda p: C.c_void_p(p or 0)   # noqa: E731
        _check(self._lib.spfe_list_observations_resident(self._h, v(d_point_idx), int(first_row), int(m), v(d_kf_mp_of_kp),
                                                         int(kp_stride), v(d_kf_flags), int(n_slots), v(d_mp_ref_slot), int(n_table),
                                                         int(obs_cap), v(d_out), v(stream)))

    def insert_keyframe(self, state, frame_mp_of_kp, cur_slot, kf_mp_of_kp, kf_flags, kf_record=None, desc_track=None, fill=0):
        """The same on host arrays (spfe_insert_keyframe), synchronous: state a dict of flags, nobs, recent, recent_n (found,
        visible, first_kf optional), kf_mp_of_kp int32 [n_slots][kp_stride] and desc_track float32 [n_table][256] updated IN PLACE;
        kf_record: the record's bytes (uint8, layout.bytes) or None.  -> the raw block (every byte written)."""
        rows = kf_mp_of_kp
        assert rows.ndim == 2 and rows.dtype == np.int32 and rows.flags["C_CONTIGUOUS"]
        assert kf_flags.dtype == np.uint8 and kf_flags.flags["C_CONTIGUOUS"] and len(kf_flags) == rows.shape[0]
        frame = np.ascontiguousarray(frame_mp_of_kp, np.int32)
        n_table = len(state["flags"])
        ptrs = []
        for k in MP_LIFE_STATE:
            a = state.get(k)
            if a is not None:
                assert a.flags["C_CONTIGUOUS"] and a.dtype == (np.uint8 if k == "flags" else np.int32) and a.ndim == 1, k
            ptrs.append(a.ctypes.data if a is not None else None)
        life = mp_life(ptrs, n_table, len(state["recent"]))
        rec = None
        if kf_record is not None:
            rec = np.ascontiguousarray(kf_record, np.uint8)
            assert rec.size >= self.layout.bytes
        if desc_track is not None:
            assert desc_track.dtype == np.float32 and desc_track.flags["C_CONTIGUOUS"] and desc_track.shape == (n_table, 256)
        out = np.full(newkf_offsets(len(frame), rows.shape[1])["out_bytes"], fill, np.uint8)
        _check(self._lib.spfe_insert_keyframe(self._h, C.byref(life), frame.ctypes.data if frame.size else None, len(frame), int(cur_slot),
                                              rows.ctypes.data, rows.shape[1], kf_flags.ctypes.data, rows.shape[0],
                                              rec.ctypes.data if rec is not None else None,
                                              desc_track.ctypes.data if desc_track is not None else None, out.ctypes.data))
        return out

    def list_observations(self, point_idx, first_row, m, kf_mp_of_kp, kf_flags, mp_ref_slot, obs_cap, fill=0):
        """The same on host arrays (spfe_list_observations), synchronous.  point_idx int32 [m] or None.  -> the raw block (every
        byte written); decode_listobs_out unpacks it."""
        rows = kf_mp_of_kp
        assert rows.ndim == 2 and rows.dtype == np.int32 and rows.flags["C_CONTIGUOUS"]
        assert kf_flags.dtype == np.uint8 and kf_flags.flags["C_CONTIGUOUS"] and len(kf_flags) == rows.shape[0]
        rs = np.ascontiguousarray(mp_ref_slot, np.int32)
        pi = None if point_idx is None else np.ascontiguousarray(point_idx, np.int32)
        assert pi is None or len(pi) >= int(m)
        out = np.full(listobs_offsets(m, obs_cap)["out_bytes"], fill, np.uint8)
        _check(self._lib.spfe_list_observations(self._h, pi.ctypes.data if pi is not None and pi.size else None, int(first_row), int(m),
                                                rows.ctypes.data, rows.shape[1], kf_flags.ctypes.data, rows.shape[0], rs.ctypes.data,
                                                len(rs), int(obs_cap), out.ctypes.data))
        return out

    @staticmethod
    def decode_newkf_out(host_block, n_kp, kp_stride):
        """The block of an insertion: dict of the NEWKF_FIELDS, code int32 [n_kp], added_point int32 [kp_stride]."""
        b = np.ascontiguousarray(host_block, np.uint8)
        o = newkf_offsets(n_kp, kp_stride)
        out = {name: int(v) for name, v in zip(NEWKF_FIELDS, b[:36].view(np.int32))}
        out["code"] = b[o["code"]:o["code"] + 4 * int(n_kp)].view(np.int32).copy()
        out["added_point"] = b[o["added_point"]:o["added_point"] + 4 * int(kp_stride)].view(np.int32).copy()
        return out

    @staticmethod
    def decode_listobs_out(host_block, m, obs_cap):
        """The block of a listing: dict of the LISTOBS_FIELDS, point_idx int32 [m], obs_start int32 [m + 1], ref_slot int32 [m],
        obs int32 [obs_cap][2]."""
        b = np.ascontiguousarray(host_block, np.uint8)
        m, e = int(m), int(obs_cap)
        o = listobs_offsets(m, e)
        out = {name: int(v) for name, v in zip(LISTOBS_FIELDS, b[:40].view(np.int32))}
        at = lambda k, n: b[o[k]:o[k] + 4 * n].view(np.int32).copy()   # noqa: E731
        out.update(point_idx=at("point_idx", m), obs_start=at("obs_start", m + 1), ref_slot=at("ref_slot", m),
                   obs=at("obs", 2 * e).reshape(e, 2))
        return out

    # -- the local bundle adjustment on resident state: gather and application (optimizer.cpp:447-499, :568-658, :739-773) --
    def gather_local_ba_resident(self, d_ord_slot, conn_cap, d_kf_mp_of_kp, kp_stride, d_kf_flags, n_slots, d_mp_flags, d_xyz, n_table,
                                 d_Tcw, cur_slot, d_out, origin_slot=-1, kf_cap=128, free_cap=64, point_cap=4096, edge_cap=32768,
                                 stream=None):
        """The problem of the local bundle adjustment of the keyframe at cur_slot from the resident arrays
        (spfe_gather_local_ba_resident): d_out receives lba_gather_offsets(kf_cap, point_cap, edge_cap)["out_bytes"] bytes
        (decode_lba_gather), in which the solver's d_edges, d_Tcw, d_fixed and d_xyz lie.  Ten launches, no host synchronisation."""
        prm = LbaGatherParams(int(cur_slot), int(origin_slot), int(kf_cap), int(free_cap), int(point_cap), int(edge_cap))
        v = lambda p: C.c_void_p(p or 0)   # noqa: E731
        _check(self._lib.spfe_gather_local_ba_resident(self._h, v(d_ord_slot), int(conn_cap), v(d_kf_mp_of_kp), int(kp_stride), v(d_kf_flags),
                                                       int(n_slots), v(d_mp_flags), v(d_xyz), int(n_table), v(d_Tcw), C.byref(prm), v(d_out),
                                                       v(stream)))

    def apply_local_ba_resident(self, d_gather, d_ba_out, d_kf_mp_of_kp, kp_stride, d_kf_flags, n_slots, d_mp_flags, d_mp_nobs,
                                d_mp_ref_slot, d_xyz, n_table, d_Tcw, kf_cap, point_cap, edge_cap, d_out, bad_cap=0, stream=None):
        """The solver's block applied to the resident arrays (spfe_apply_local_ba_resident).  WRITES d_kf_mp_of_kp, d_mp_flags,
        d_mp_nobs, d_mp_ref_slot, d_xyz and d_Tcw.  d_out receives lba_apply_offsets(point_cap, edge_cap, bad_cap)["out_bytes"] bytes
        (decode_lba_apply), in which the refresh's d_obs_start, d_obs and d_ref_slot lie.  Five launches, no host synchronisation."""
        prm = LbaApplyParams(int(kf_cap), int(point_cap), int(edge_cap), int(bad_cap))
        v = lambda p: C.c_void_p(p or 0)   # noqa: E731
        _check(self._lib.spfe_apply_local_ba_resident(self._h, v(d_gather), v(d_ba_out), v(d_kf_mp_of_kp), int(kp_stride), v(d_kf_flags),
                                                      int(n_slots), v(d_mp_flags), v(d_mp_nobs), v(d_mp_ref_slot), v(d_xyz), int(n_table),
                                                      v(d_Tcw), C.byref(prm), v(d_out), v(stream)))

    def gather_local_ba(self, ord_row, kf_mp_of_kp, kf_flags, mp_flags, xyz, Tcw, cur_slot, origin_slot=-1, kf_cap=128, free_cap=64,
                        point_cap=4096, edge_cap=32768, fill=0):
        """The same on host arrays (spfe_gather_local_ba), synchronous: ord_row int32 [conn_cap] is row cur_slot of the graph's
        ord_slot.  -> the raw block (every byte written); decode_lba_gather unpacks it."""
        rows = kf_mp_of_kp
        ordr = np.ascontiguousarray(ord_row, np.int32)
        assert rows.ndim == 2 and rows.dtype == np.int32 and rows.flags["C_CONTIGUOUS"]
        assert kf_flags.dtype == np.uint8 and len(kf_flags) == rows.shape[0] and mp_flags.dtype == np.uint8
        assert xyz.dtype == np.float32 and xyz.flags["C_CONTIGUOUS"] and xyz.shape == (len(mp_flags), 3)
        assert Tcw.dtype == np.float32 and Tcw.flags["C_CONTIGUOUS"] and Tcw.shape == (rows.shape[0], 16)
        prm = LbaGatherParams(int(cur_slot), int(origin_slot), int(kf_cap), int(free_cap), int(point_cap), int(edge_cap))
        out = np.full(lba_gather_offsets(kf_cap, point_cap, edge_cap)["out_bytes"], fill, np.uint8)
        _check(self._lib.spfe_gather_local_ba(self._h, ordr.ctypes.data, len(ordr), rows.ctypes.data, rows.shape[1], kf_flags.ctypes.data,
                                              rows.shape[0], mp_flags.ctypes.data, xyz.ctypes.data, len(mp_flags), Tcw.ctypes.data,
                                              C.byref(prm), out.ctypes.data))
        return out

    def apply_local_ba(self, gather, ba_out, kf_mp_of_kp, kf_flags, mp_flags, mp_nobs, mp_ref_slot, xyz, Tcw, kf_cap, point_cap, edge_cap,
                       bad_cap=0, fill=0):
        """The same on host arrays (spfe_apply_local_ba), synchronous: the two blocks as downloaded (uint8), the rows, flags, counts,
        reference slots, positions and poses updated IN PLACE.  -> the raw block; decode_lba_apply unpacks it."""
        rows = kf_mp_of_kp
        g, b = np.ascontiguousarray(gather, np.uint8), np.ascontiguousarray(ba_out, np.uint8)
        assert len(g) == lba_gather_offsets(kf_cap, point_cap, edge_cap)["out_bytes"] and len(b) >= 128
        assert rows.ndim == 2 and rows.dtype == np.int32 and rows.flags["C_CONTIGUOUS"]
        nt = len(mp_flags)
        assert kf_flags.dtype == np.uint8 and len(kf_flags) == rows.shape[0] and mp_flags.dtype == np.uint8
        assert mp_nobs.dtype == np.int32 and mp_ref_slot.dtype == np.int32 and len(mp_nobs) == len(mp_ref_slot) == nt
        assert xyz.dtype == np.float32 and xyz.flags["C_CONTIGUOUS"] and xyz.shape == (nt, 3)
        assert Tcw.dtype == np.float32 and Tcw.flags["C_CONTIGUOUS"] and Tcw.shape == (rows.shape[0], 16)
        prm = LbaApplyParams(int(kf_cap), int(point_cap), int(edge_cap), int(bad_cap))
        out = np.full(lba_apply_offsets(point_cap, edge_cap, bad_cap)["out_bytes"], fill, np.uint8)
        _check(self._lib.spfe_apply_local_ba(self._h, g.ctypes.data, b.ctypes.data, rows.ctypes.data, rows.shape[1], kf_flags.ctypes.data,
                                             rows.shape[0], mp_flags.ctypes.data, mp_nobs.ctypes.data, mp_ref_slot.ctypes.data, xyz.ctypes.data,
                                             nt, Tcw.ctypes.data, C.byref(prm), out.ctypes.data))
        return out

    @staticmethod
    def decode_lba_gather(host_block, kf_cap, point_cap, edge_cap):
        """The gather's block: dict of the LBA_GATHER_FIELDS, kf_slot int32 [kf_cap], fixed uint8 [kf_cap], Tcw f32 [kf_cap][16],
        point_idx int32 [point_cap], xyz f32 [point_cap][3], obs_start int32 [point_cap + 1], obs int32 [edge_cap][2], edges int32
        [edge_cap][3]."""
        b = np.ascontiguousarray(host_block, np.uint8)
        k, p, e = int(kf_cap), int(point_cap), int(edge_cap)
        o = lba_gather_offsets(k, p, e)
        out = {name: int(v) for name, v in zip(LBA_GATHER_FIELDS, b[:40].view(np.int32))}
        at = lambda key, nbytes, dt: b[o[key]:o[key] + nbytes].view(dt).copy()   # noqa: E731
        out.update(kf_slot=at("kf_slot", 4 * k, np.int32), fixed=at("fixed", k, np.uint8), Tcw=at("Tcw", 64 * k, np.float32).reshape(-1, 16),
                   point_idx=at("point_idx", 4 * p, np.int32), xyz=at("xyz", 12 * p, np.float32).reshape(-1, 3),
                   obs_start=at("obs_start", 4 * (p + 1), np.int32), obs=at("obs", 8 * e, np.int32).reshape(-1, 2),
                   edges=at("edges", 12 * e, np.int32).reshape(-1, 3))
        return out

    @staticmethod
    def decode_lba_apply(host_block, point_cap, edge_cap, bad_cap):
        """The application's block: dict of the LBA_APPLY_FIELDS, bad_point int32 [bad_cap], obs_start int32 [point_cap + 1], obs
        int32 [edge_cap][2], ref_slot int32 [point_cap]."""
        b = np.ascontiguousarray(host_block, np.uint8)
        p, e, bc = int(point_cap), int(edge_cap), int(bad_cap)
        o = lba_apply_offsets(p, e, bc)
        out = {name: int(v) for name, v in zip(LBA_APPLY_FIELDS, b[:24].view(np.int32))}
        at = lambda key, cnt: b[o[key]:o[key] + 4 * cnt].view(np.int32).copy()   # noqa: E731
        out.update(bad_point=at("bad_point", bc), obs_start=at("obs_start", p + 1), obs=at("obs", 2 * e).reshape(-1, 2), ref_slot=at("ref_slot", p))
        return out

    @staticmethod
    def decode_admit_out(host_block):
        """The block of an admission: dict of the ADMIT_FIELDS, admitted int32 [32] per neighbour."""
        b = np.ascontiguousarray(host_block, np.uint8)
        out = {name: int(v) for name, v in zip(ADMIT_FIELDS, b[:24].view(np.int32))}
        out["admitted"] = b[ADMIT_OFF_ADMITTED:ADMIT_OFF_ADMITTED + 128].view(np.int32).copy()
        return out

    @staticmethod
    def decode_mpstat_out(host_block):
        b = np.ascontiguousarray(host_block, np.uint8)
        return {name: int(v) for name, v in zip(MPSTAT_FIELDS, b[:12].view(np.int32))}

    @staticmethod
    def decode_mpcull_out(host_block, recent_cap, bad_cap):
        """The block of one cull: dict of the MPCULL_FIELDS, entry_point / entry_code int32 [recent_cap], bad_point [bad_cap]."""
        b = np.ascontiguousarray(host_block, np.uint8)
        r, bc = int(recent_cap), int(bad_cap)
        o = mpcull_offsets(r, bc)
        out = {name: int(v) for name, v in zip(MPCULL_FIELDS, b[:40].view(np.int32))}
        at = lambda key, cnt: b[o[key]:o[key] + 4 * cnt].view(np.int32).copy()   # noqa: E731
        out.update(entry_point=at("entry_point", r), entry_code=at("entry_code", r), bad_point=at("bad_point", bc))
        return out

    @staticmethod
    def decode_mp_out(host_block, m):
        """The block of a refresh: dict of the MP_FIELDS counts, best_obs int32 [m], n_good int32 [m], best_median f32 [m],
        code uint8 [m]."""
        b = np.ascontiguousarray(host_block, np.uint8)
        m = int(m)
        o = mp_offsets(m)
        f = b[:16].view(np.int32)
        return dict(m=int(f[0]), n_desc_written=int(f[1]), n_nd_written=int(f[2]), status=int(f[3]),
                    best_obs=b[o["best_obs"]:o["n_good"]].view(np.int32).copy(),
                    n_good=b[o["n_good"]:o["best_median"]].view(np.int32).copy(),
                    best_median=b[o["best_median"]:o["code"]].view(np.float32).copy(), code=b[o["code"]:o["code"] + m].copy())

    @staticmethod
    def decode_proj_out(host_block, n=None):
        """The spfe_proj_out_bytes block: dict(n_matches, n_to_match, n, kp_of_mp int32[n], proj_uv f32[n,2],
        view_cos f32[n], in_view bool[n]); n defaults to the count the block itself names."""
        b = np.ascontiguousarray(host_block, np.uint8)
        c = b[:12].view(np.int32)
        if n is None:
            n = int(c[2])
        return dict(n_matches=int(c[0]), n_to_match=int(c[1]), n=int(c[2]),
                    kp_of_mp=b[PROJ_OFF_KP:PROJ_OFF_KP + 4 * n].view(np.int32).copy(),
                    proj_uv=b[PROJ_OFF_UV:PROJ_OFF_UV + 8 * n].view(np.float32).reshape(n, 2).copy(),
                    view_cos=b[PROJ_OFF_COS:PROJ_OFF_COS + 4 * n].view(np.float32).copy(),
                    in_view=b[PROJ_OFF_VIEW:PROJ_OFF_VIEW + n].astype(bool))

    # -- pipelined host path: up to 3 batches in flight --
    def submit_batch(self, images):
        """Copy `images` (list of uint8 [H, W]) into pinned staging, enqueue H2D + the whole path + D2H of the
        records, return a ticket immediately (spfe_submit_batch)."""
        imgs = [self._check_image(im) for im in images]
        n = len(imgs)
        if n == 0:
            raise RuntimeError("input image is empty")
        if len({im.strides[0] for im in imgs}) != 1:
            imgs = [np.ascontiguousarray(im) for im in imgs]
        ptrs = (C.c_void_p * n)(*[im.ctypes.data for im in imgs])
        t = C.c_long(-1)
        _check(self._lib.spfe_submit_batch(self._h, ptrs, imgs[0].strides[0], n, C.byref(t)))
        self._pipe_n = getattr(self, "_pipe_n", {})
        self._pipe_n[t.value] = n
        return t.value

    def collect_batch(self, ticket, copy=True):
        """Block until batch `ticket` is back in host memory; list of FrameResult (deep copies).  copy=False
        returns the raw spfe_result array instead (pointers into the library's pinned buffers, valid until
        three further submits) — what a C++ caller gets."""
        n = self._pipe_n.pop(ticket)
        res = (_Result * n)()
        _check(self._lib.spfe_collect_batch(self._h, int(ticket), res))
        if not copy:
            return res
        out = [FrameResult(res[i], self.height, self.width, self.with_heat) for i in range(n)]
        self._publish(out[-1])
        return out

    def postprocess(self, semi, coarse):
        """Tail + selection + descriptors + covariance from host semi/coarse maps
        ([n,hc,wc,65], [n,hc,wc,256], or a single frame without the n axis)."""
        semi = np.ascontiguousarray(semi, np.float32)
        coarse = np.ascontiguousarray(coarse, np.float32)
        hc, wc = self.height // 8, self.width // 8
        semi = semi.reshape(-1, hc, wc, 65)
        coarse = coarse.reshape(-1, hc, wc, 256)
        n = semi.shape[0]
        res = (_Result * n)()
        _check(self._lib.spfe_postprocess(self._h, semi.ctypes.data, coarse.ctypes.data, n, res))
        out = [FrameResult(res[i], self.height, self.width, self.with_heat) for i in range(n)]
        self._publish(out[-1])
        return out

    # -- side outputs (sp_extractor.h:61-73) --
    def getCov(self):
        return self._cov2

    def getCov2Inv(self):
        return self._cov2_inv

    def getHeatMap(self):
        return self.heat_

    def getMask(self):
        return self.mask_

    # -- device-resident path --
    def record_bytes(self):
        return int(self._lib.spfe_record_bytes(self._h))

    def extract_batch_device(self, d_images, n, d_records=None, stream=None):
        """Enqueue n frames already in device memory (raw device pointers as ints)."""
        if not d_images:
            raise RuntimeError("input image is empty")
        _check(self._lib.spfe_extract_batch_device(self._h, C.c_void_p(d_images), int(n),
                                                   C.c_void_p(d_records or 0),
                                                   C.c_void_p(stream or 0)))
        return int(self._lib.spfe_last_ticket(self._h))

    def last_ticket(self):
        """Ticket of the most recent extract_batch_device call on this handle (spfe_last_ticket)."""
        return int(self._lib.spfe_last_ticket(self._h))

    def wait_records(self, ticket, stream=None):
        """Order `stream` after the covariance stage of call `ticket` (async_cov mode)."""
        _check(self._lib.spfe_wait_records(self._h, int(ticket), C.c_void_p(stream or 0)))

    # -- multi-GPU: RCCL all-gather of the records, inside the library (no torch) --
    @staticmethod
    def comm_unique_id():
        """128-byte RCCL unique id (rank 0 creates it and ships it to every rank)."""
        buf = (C.c_ubyte * 128)()
        _check(load_library().spfe_comm_unique_id(buf, 128))
        return bytes(buf)

    def comm_init(self, unique_id, rank, world):
        if len(unique_id) != 128:
            raise ValueError("unique id must be 128 bytes")
        _check(self._lib.spfe_comm_init(self._h, C.c_char_p(bytes(unique_id)), int(rank), int(world)))

    def comm_destroy(self):
        _check(self._lib.spfe_comm_destroy(self._h))

    def comm_stream(self):
        """hipStream_t (int) of the library's communication stream, 0 before comm_init."""
        return int(self._lib.spfe_comm_stream(self._h) or 0)

    def comm_count(self):
        """Number of ranks in the communicator as RCCL reports it (ncclCommCount)."""
        n = C.c_int(0)
        _check(self._lib.spfe_comm_count(self._h, C.byref(n)))
        return n.value

    def allgather_records(self, ticket, d_local, d_all, frames_per_rank):
        """ncclAllGather of this rank's `frames_per_rank` records (device pointers as ints) on the library's
        communication stream, ordered after the records of call `ticket`."""
        _check(self._lib.spfe_allgather_records(self._h, int(ticket), C.c_void_p(d_local), C.c_void_p(d_all),
                                                int(frames_per_rank)))

    def comm_wait(self, stream=None):
        """Order `stream` after the last all-gather."""
        _check(self._lib.spfe_comm_wait(self._h, C.c_void_p(stream or 0)))

    def view_record(self, host_record):
        """Decode ONE record (bytes-like / uint8 array copied from the device)."""
        rec = np.ascontiguousarray(np.frombuffer(host_record, np.uint8)
                                   if not isinstance(host_record, np.ndarray) else host_record)
        r = _Result()
        _check(self._lib.spfe_view_record(self._h, rec.ctypes.data, C.byref(r)))
        return FrameResult(r, self.height, self.width, False)

    # -- input staging --
    def set_staging(self, src_height, src_width, channels=3, rgb=False, map_x=None, map_y=None):
        """Configure the raw-frame front end: cv::remap(m1, m2, INTER_LINEAR) (data_loader.cc:519-521),
        crop (system.cpp:160-161), cvtColor to gray (mono_tracker.cpp:18-28).  Maps: f32
        [src_height, src_width] (cv::initUndistortRectifyMap, CV_32FC1) or None."""
        st = _Staging(src_height, src_width, channels, 1 if rgb else 0, None, None)
        keep = []
        if map_x is not None or map_y is not None:
            mx = np.ascontiguousarray(map_x, np.float32)
            my = np.ascontiguousarray(map_y, np.float32)
            if mx.shape != (src_height, src_width) or my.shape != (src_height, src_width):
                raise SpfeError("maps must be [src_height, src_width]")
            keep = [mx, my]
            st.map_x, st.map_y = mx.ctypes.data, my.ctypes.data
        _check(self._lib.spfe_set_staging(self._h, C.byref(st)))
        self._staging = (src_height, src_width, channels)
        del keep

    def _check_raw(self, src):
        if src is None or getattr(src, "size", 0) == 0:
            raise RuntimeError("input image is empty")  # sp_extractor.cpp:364-365
        hs, ws, cn = self._staging
        src = np.asarray(src)
        want = (hs, ws) if cn == 1 else (hs, ws, cn)
        if src.dtype != np.uint8 or src.shape != want:
            raise SpfeError("raw frame must be uint8 %s, got %s %s" % (want, src.dtype, src.shape))
        return np.ascontiguousarray(src)

    def extract_staged(self, src):
        """Raw camera frame -> Frame (remap + crop + gray on the GPU, then the extraction path)."""
        return self.extract_batch_staged([src])[0]

    def extract_batch_staged(self, srcs):
        srcs = [self._check_raw(s) for s in srcs]
        n = len(srcs)
        hs, ws, cn = self._staging
        ptrs = (C.c_void_p * n)(*[s.ctypes.data for s in srcs])
        res = (_Result * n)()
        _check(self._lib.spfe_extract_batch_staged(self._h, ptrs, ws * cn, n, res))
        frames = [FrameResult(res[i], self.height, self.width, self.with_heat) for i in range(n)]
        self._publish(frames[-1])
        return frames

    def stage_batch_device(self, d_src, n, d_gray, stream=None):
        _check(self._lib.spfe_stage_batch_device(self._h, d_src, n, d_gray, stream))

    # -- descriptor matching --
    def match(self, query, train, cross_check=True):
        """cv::BFMatcher(NORM_L2, crossCheck).match(query) with `train` added, as
        SPMatcher::SearchByBruteForce calls it (sp_matcher.cpp:1642-1674).
        query [nq,256], train [nt,256] f32 -> (train_idx int32 [nq], -1 = no match; distance f32 [nq])."""
        q = np.ascontiguousarray(query, np.float32).reshape(-1, 256)
        t = np.ascontiguousarray(train, np.float32).reshape(-1, 256)
        idx = np.empty(len(q), np.int32)
        dist = np.empty(len(q), np.float32)
        _check(self._lib.spfe_match(self._h, q.ctypes.data if len(q) else None, len(q),
                                    t.ctypes.data if len(t) else None, len(t), 1 if cross_check else 0,
                                    idx.ctypes.data, dist.ctypes.data))
        return idx, dist

    def match_knn2(self, query, train):
        """knnMatch(query, matches, 2) against `train`, exact: -> (train_idx [nq, 2] int32, distance [nq, 2] f32)."""
        q = np.ascontiguousarray(query, np.float32).reshape(-1, 256)
        t = np.ascontiguousarray(train, np.float32).reshape(-1, 256)
        idx = np.full((max(len(q), 1), 2), -1, np.int32)
        dist = np.zeros((max(len(q), 1), 2), np.float32)
        _check(self._lib.spfe_match_knn2(self._h, q.ctypes.data, len(q), t.ctypes.data, len(t), idx.ctypes.data,
                                         dist.ctypes.data))
        return idx[:len(q)], dist[:len(q)]

    def match_patches(self, mp_desc, mp_uv, occ_grid, kp_desc, max_dist=0.75):
        """Patch-wise association of projected map points (tracker_dust.cpp:113-172): map point i at
        dust-map position mp_uv[i] (cells) takes the nearest keypoint of its 2 x 2 cells below max_dist,
        earlier map points first.  -> int32 [n_points] keypoint index or -1."""
        m = np.ascontiguousarray(mp_desc, np.float32).reshape(-1, 256)
        uv = np.ascontiguousarray(mp_uv, np.float32).reshape(-1, 2)
        occ = np.ascontiguousarray(occ_grid, np.int16)
        kd = np.ascontiguousarray(kp_desc, np.float32).reshape(-1, 256)
        if occ.shape != (self.height // 8, self.width // 8):
            raise SpfeError("occ_grid must be [height/8, width/8]")
        out = np.empty(len(m), np.int32)
        _check(self._lib.spfe_match_patches(self._h, m.ctypes.data if len(m) else None, uv.ctypes.data if len(m) else None,
                                            len(m), occ.ctypes.data, kd.ctypes.data if len(kd) else None, len(kd),
                                            max_dist, out.ctypes.data if len(m) else np.empty(1, np.int32).ctypes.data))
        return out

    def match_patches_record_device(self, d_mp_desc, d_mp_uv, n_points, d_record, d_kp_idx, max_dist=0.75,
                                    stream=None):
        _check(self._lib.spfe_match_patches_record_device(self._h, d_mp_desc, d_mp_uv, n_points, d_record, max_dist,
                                                          d_kp_idx, stream))

    def match_out_bytes(self):
        return int(self._lib.spfe_match_out_bytes(self._h))

    def match_records_device(self, d_query_records, d_train_records, n_pairs, d_out, cross_check=True,
                             stream=None):
        """Device pointers (ints) to n_pairs query / train records and to n_pairs * match_out_bytes()
        bytes of output; enqueues on `stream` (int hipStream_t, None = the handle's stream)."""
        _check(self._lib.spfe_match_records_device(self._h, d_query_records, d_train_records, n_pairs,
                                                   1 if cross_check else 0, d_out, stream))

    def decode_match_out(self, host_block, n_query=None):
        """uint8[match_out_bytes()] copied from the device -> (train_idx, distance)."""
        b = np.ascontiguousarray(host_block, np.uint8)
        kmax = self.match_out_bytes() // 8
        idx = b[:kmax * 4].view(np.int32)
        dist = b[kmax * 4:kmax * 8].view(np.float32)
        n = kmax if n_query is None else n_query
        return idx[:n].copy(), dist[:n].copy()

    def fetch_heat_inv(self, frame=0):
        """heat_inv (sp_extractor.cpp:468) of a frame of the last synchronous host call, copied back on demand
        (spfe_fetch_heat_inv; the companion of lazy_heat_inv=True)."""
        p = C.c_void_p()
        _check(self._lib.spfe_fetch_heat_inv(self._h, int(frame), C.byref(p)))
        return _as_np(p.value, (self.height, self.width), np.float32)

    def debug_read(self, name, frame=0):
        shapes = {"semi": (self.height // 8, self.width // 8, 65),
                  "coarse": (self.height // 8, self.width // 8, 256),
                  "head": (self.height // 8, self.width // 8, 512),
                  "feat": (self.height // 8, self.width // 8, 128),
                  "heat_log": (self.height, self.width), "heat_inv": (self.height, self.width),
                  "heat": (self.height, self.width),
                  "cell_score": (self.height // 8, self.width // 8)}
        div = [1, 2, 2, 4, 4, 8, 8, 8]
        ch = [64, 64, 64, 64, 128, 128, 128, 128]
        for i in range(8):
            shapes["act%d" % i] = (self.height // div[i], self.width // div[i], ch[i])
        shapes["coarse_sparse"] = shapes["coarse"]   # the descriptor map as the last call left it (only the rows it read)
        if name.startswith("cov_"):   # covariance scratch (int32): counters [4], nxt / workers / npop [kmax]
            out = np.empty(4 if name == "cov_counters" else self.nfeatures + 1, np.int32)
        elif name in ("db_total", "da_gathered", "conv1b_tile_rows", "conv1b_split_rows", "select_huge", "two_chains", "twin_failed"):   # gathered descriptor head: number of listed cells of the last call /
            out = np.empty(1, np.int32)             # whether convDa ran on those cells only
        elif name == "split_streams":   # [outcome of the queue probe, the last call ran as two half batches] (spfe_schedule.hip)
            out = np.empty(2, np.int32)
        elif name == "db_list":       # ... and the list (global cell indices b * C + cell), max_batch * min(4 kmax, C) entries
            C_ = (self.height // 8) * (self.width // 8)
            out = np.empty(self.max_batch * min(4 * (self.nfeatures + 1), C_), np.int32)
        else:
            out = (np.empty((self.height, self.width), np.uint8) if name == "image"   # the staged gray frame
                   else np.empty(shapes[name], np.float32))
        n = self._lib.spfe_debug_read(self._h, name.encode(), frame, out.ctypes.data, out.nbytes)
        if n < 0:
            _check(int(n))
        return out

    def stage_reset(self):
        _check(self._lib.spfe_stage_reset(self._h))

    def stage_times(self):
        buf = (C.c_float * 32)()
        n = self._lib.spfe_stage_times(self._h, buf, 32)
        if n < 0:
            _check(n)
        return {self._lib.spfe_stage_name(i).decode(): buf[i] for i in range(n)}


def math_probe(x):
    """Device spfe_expf(x), spfe_logf(|x|) for a float32 array (test hook)."""
    x = np.ascontiguousarray(x, np.float32)
    e = np.empty_like(x)
    l = np.empty_like(x)
    _check(load_library().spfe_math_probe(x.ctypes.data, e.ctypes.data, l.ctypes.data, x.size))
    return e, l
