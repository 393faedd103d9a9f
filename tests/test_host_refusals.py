"""The host-pointer entry points refuse a bad argument before they touch the
device: every row below is a call through the C ABI that must come back as
ORBPL_ERR_ARG with exactly this orbpl_last_error() text, on a machine with or
without a GPU (a refusal issued after the first HIP call would surface as
ORBPL_ERR_HIP where there is no device).

Per entry point: a NULL required pointer, a negative count, and a count one
past its capacity (2048 keypoints, 80 key lines, 256 bf-knn queries, 2304 pose
edges, 10 neighbours, 64 keyframes, min_inliers 4, vocabulary node ids below
2^21 - 1).

Not in the table, because the library issues them only after it has staged the
inputs: orbm_search_by_projection_kf's nlevels refusal (it comes from the
device form the host form ends in), and orbpl_stereo_matches' refusals about
the two extractors (they need the extractors' device pyramids).
"""
import ctypes as C

import numpy as np
import pytest

from _pkg import load_pkg

orbpl = load_pkg()

# every non-NULL pointer of a bad call points here: zeros, larger than any
# array the refusals' own loops read (2049 rows of 64 bytes)
_Z = np.zeros(1 << 18, np.uint8)
Z = _Z.ctypes.data
CAM = orbpl.Camera(525.0, 525.0, 319.5, 239.5, 0.0, 0.0, 0.0, 0.0, 0.0, 40.0, 3.0, 640, 480)
_KEEP = []

CAP_KP = "keypoint count exceeds the matcher capacity (2048)"
CAP_KL = "more key lines than LineExtractor keeps (80)"
NODE = "vocabulary node id >= 2^21 - 1"


def ref(obj):
    _KEEP.append(obj)
    return C.addressof(obj)


def cam():
    return ref(CAM)


def cur(n=0, Tcw=Z, kps_un=Z, desc=Z, uright=Z):
    return ref(orbpl.MatchCurrent(n, Tcw, kps_un, desc, uright))


def last(n=0, kps_un=Z):
    return ref(orbpl.MatchLast(n, Z, kps_un, Z, Z, Z, Z, Z))


def pose(n=0, nl=0, kps_un=Z, kl_obs=Z, nlevels=8):
    return ref(orbpl.PoseProblem(n, kps_un, Z, Z, Z, nl, kl_obs, Z, Z, Z, Z, nlevels))


def ints(*v):
    a = np.array(v, np.int32)
    _KEEP.append(a)
    return a.ctypes.data


def u8(*v):
    a = np.array(v, np.uint8)
    _KEEP.append(a)
    return a.ctypes.data


def octaves(*v):
    a = np.zeros(len(v), orbpl.KP_DTYPE)
    a["octave"] = v
    _KEEP.append(a)
    return a.ctypes.data


def kfdb(nkf=0, nq_words=0, cand=Z, kf_off=Z, q_words=Z):
    return ref(orbpl.KfdbProblem(nkf, kf_off, Z, Z, Z, Z, nq_words, q_words, Z, cand, Z, Z))


def pnp(n=0, min_inliers=4, iterations=Z, p2d=Z, n_draws=0):
    return ref(orbpl.PnpProblem(525.0, 525.0, 319.5, 239.5, n, p2d, None, Z, min_inliers, 1, Z,
                                n_draws, Z, iterations, Z, Z, Z, Z, Z, Z, Z, Z, Z))


def kf(n=0, nl=0, Tcw=Z, kps=Z, kps_un=Z, klines=Z, feat_node=Z):
    return orbpl.LmKeyFrame(0, Tcw, n, kps, kps_un, Z, Z, Z, feat_node, Z, Z, nl, klines, Z, Z)


def kfp(**kw):
    return ref(kf(**kw))


def lm_problem(n_neigh=0, neigh=Z, points=Z, **kw):
    p = orbpl.LmProblem()
    p.cur, p.n_neigh, p.neigh = kf(**kw), n_neigh, neigh
    p.points = p.kf1_point_record = points
    p.lines = p.kf1_line_record = Z
    return ref(p)


def lm_neigh(**kw):
    return ref((orbpl.LmKeyFrame * 1)(kf(**kw)))


# name -> a call whose arguments are all acceptable (every count 0, every
# pointer non-NULL); a row replaces some of them by position
GOOD = {
    "orbpl_frame_prepare": lambda: [cam(), Z, 0, Z, Z, Z, Z, Z, Z],
    "orbm_search_by_projection_last": lambda: [cam(), Z, 8, cur(), last(), 7.0, 0, 1, Z, Z],
    "orbpl_pose_optimization": lambda: [cam(), pose(), Z, Z, Z, Z],
    "orbpl_pose_optimization_ex": lambda: [cam(), pose(), 0, Z, Z, Z, Z],
    "orbpl_frame_is_in_frustum": lambda: [cam(), 1.2, 8, Z, 0, Z, Z, Z, Z, 0.5, Z, Z, Z, Z, Z, Z],
    "orbm_search_by_projection_local": lambda: [cam(), Z, 8, cur(), 0, Z, Z, Z, Z, Z, Z, Z, Z, Z,
                                                1.0, 0.8, Z, Z],
    "orbpl_line_frame_prepare": lambda: [cam(), Z, 0, Z, Z, Z, Z, Z, Z],
    "orbl_search_by_projection_last": lambda: [cam(), Z, 0, Z, Z, 0, Z, Z, Z, Z, Z, Z, Z],
    "orbm_search_by_bow": lambda: [0, Z, Z, Z, Z, 0, Z, Z, Z, 0.7, 1, Z, Z],
    "orbm_search_by_projection_kf": lambda: [cam(), Z, 8, cur(), Z, 0, Z, Z, Z, Z, Z, Z, Z, 10.0,
                                             100, 1, Z, Z],
    "orbpl_stereo_matches": lambda: [cam(), Z, Z, 0, Z, Z, 0, Z, Z, 0, Z, Z],
    "orbl_frame_is_in_frustum": lambda: [Z, 0, Z, Z],
    "orbl_search_by_projection_list": lambda: [cam(), Z, 0, Z, Z, Z, 0, Z, Z, Z, Z, Z, Z],
    "orbl_search_by_projection_pairs": lambda: [cam(), Z, 0, 0, Z, Z, Z, 0, Z, Z, Z, Z, Z, Z, Z, Z,
                                                Z, 0, Z, Z, Z, Z],
    "orbl_match_bf_knn": lambda: [0, Z, 0, Z, Z, Z],
    "orbl_stereo_line_depths": lambda: [cam(), Z, Z, 0, Z, Z, 0, Z, Z],
    "orbkf_detect_reloc": lambda: [kfdb(), 1, 0],
    "orbpnp_iterate": lambda: [pnp(), 1, 1],
    "orblm_create_new_map_features": lambda: [cam(), Z, Z, 8, lm_problem(), 1],
    "orbm_search_for_triangulation": lambda: [cam(), Z, Z, 8, kfp(), kfp(), Z, 0, 0, Z, Z, Z],
    "orbl_search_for_triangulation": lambda: [0, Z, 0, Z, Z, Z],
}

_P = C.POINTER(C.c_int)


def _as_int_ptr(v):
    return C.cast(C.c_void_p(v), _P)


# (entry point, case, {argument position: value}, the refusal)
ROWS = [
    ("orbpl_frame_prepare", "null_camera", {0: None}, "bad argument"),
    ("orbpl_frame_prepare", "negative_n", {2: -1}, "bad argument"),
    ("orbpl_frame_prepare", "null_keypoints", {1: None, 2: 1}, "bad argument"),
    ("orbpl_frame_prepare", "null_output", {2: 1, 7: None}, "bad argument"),

    ("orbm_search_by_projection_last", "null_current", {3: None}, "NULL argument"),
    ("orbm_search_by_projection_last", "null_nmatches", {9: None}, "NULL argument"),
    ("orbm_search_by_projection_last", "negative_n", {3: lambda: cur(-1)}, CAP_KP),
    ("orbm_search_by_projection_last", "negative_nl", {4: lambda: last(-1)}, CAP_KP),
    ("orbm_search_by_projection_last", "n_2049", {3: lambda: cur(2049)}, CAP_KP),
    ("orbm_search_by_projection_last", "nl_2049", {4: lambda: last(2049)}, CAP_KP),
    ("orbm_search_by_projection_last", "nlevels_0", {2: 0}, "nlevels out of range"),
    ("orbm_search_by_projection_last", "nlevels_17", {2: 17}, "nlevels out of range"),
    ("orbm_search_by_projection_last", "null_current_arrays", {3: lambda: cur(1, desc=None)},
     "NULL frame arrays"),
    ("orbm_search_by_projection_last", "null_pose", {3: lambda: cur(0, Tcw=None)},
     "NULL frame arrays"),
    ("orbm_search_by_projection_last", "current_octave_8",
     {3: lambda: cur(2, kps_un=octaves(7, 8))}, "keypoint octave outside the pyramid"),
    ("orbm_search_by_projection_last", "current_octave_negative",
     {3: lambda: cur(2, kps_un=octaves(0, -1))}, "keypoint octave outside the pyramid"),
    ("orbm_search_by_projection_last", "last_octave_8",
     {4: lambda: last(2, kps_un=octaves(7, 8))}, "keypoint octave outside the pyramid"),
    ("orbm_search_by_projection_last", "last_octave_negative",
     {4: lambda: last(2, kps_un=octaves(0, -1))}, "keypoint octave outside the pyramid"),

    ("orbpl_pose_optimization", "null_pose", {2: None}, "NULL argument"),
    ("orbpl_pose_optimization", "negative_n", {1: lambda: pose(-1, 0)},
     "too many edges (max 2304)"),
    ("orbpl_pose_optimization", "edges_2305", {1: lambda: pose(2305, 0)},
     "too many edges (max 2304)"),
    ("orbpl_pose_optimization_ex", "null_problem", {1: None}, "NULL argument"),
    ("orbpl_pose_optimization_ex", "null_n_inliers", {6: None}, "NULL argument"),
    ("orbpl_pose_optimization_ex", "unknown_flag", {2: 2}, "unknown pose flag"),
    ("orbpl_pose_optimization_ex", "negative_n", {1: lambda: pose(-1, 0)},
     "too many edges (max 2304)"),
    ("orbpl_pose_optimization_ex", "negative_nl", {1: lambda: pose(0, -1)},
     "too many edges (max 2304)"),
    ("orbpl_pose_optimization_ex", "edges_2305", {1: lambda: pose(2304, 1)},
     "too many edges (max 2304)"),
    ("orbpl_pose_optimization_ex", "null_point_arrays", {1: lambda: pose(1, 0, kps_un=None)},
     "NULL point arrays"),
    ("orbpl_pose_optimization_ex", "null_outlier", {1: lambda: pose(1, 0), 4: None},
     "NULL point arrays"),
    ("orbpl_pose_optimization_ex", "null_line_arrays", {1: lambda: pose(0, 1, kl_obs=None)},
     "NULL line arrays"),
    ("orbpl_pose_optimization_ex", "nlevels_17", {1: lambda: pose(nlevels=17)},
     "nlevels out of range"),

    ("orbpl_frame_is_in_frustum", "null_pose", {3: None}, "bad argument"),
    ("orbpl_frame_is_in_frustum", "negative_n", {4: -1}, "bad argument"),
    ("orbpl_frame_is_in_frustum", "nlevels_17", {2: 17}, "bad argument"),
    ("orbpl_frame_is_in_frustum", "null_xyz", {4: 1, 5: None}, "NULL map point arrays"),
    ("orbpl_frame_is_in_frustum", "null_output", {4: 1, 15: None}, "NULL map point arrays"),

    ("orbm_search_by_projection_local", "null_nmatches", {17: None}, "bad argument"),
    ("orbm_search_by_projection_local", "negative_nmp", {4: -1}, "bad argument"),
    ("orbm_search_by_projection_local", "negative_n", {3: lambda: cur(-1)}, CAP_KP),
    ("orbm_search_by_projection_local", "n_2049", {3: lambda: cur(2049)}, CAP_KP),
    ("orbm_search_by_projection_local", "null_frame_arrays", {3: lambda: cur(1, desc=None)},
     "NULL frame arrays"),
    ("orbm_search_by_projection_local", "null_match", {3: lambda: cur(1), 16: None},
     "NULL frame arrays"),
    ("orbm_search_by_projection_local", "null_map_point_arrays", {4: 1, 12: None},
     "NULL map point arrays"),
    ("orbm_search_by_projection_local", "level_out_of_range",
     {4: 2, 5: lambda: u8(1, 1), 9: lambda: ints(0, 8)}, "level out of range"),
    ("orbm_search_by_projection_local", "nlevels_0", {2: 0}, "nlevels out of range"),
    ("orbm_search_by_projection_local", "octave_8", {3: lambda: cur(2, kps_un=octaves(7, 8))},
     "keypoint octave outside the pyramid"),
    ("orbm_search_by_projection_local", "octave_negative",
     {3: lambda: cur(2, kps_un=octaves(0, -1))}, "keypoint octave outside the pyramid"),

    ("orbpl_line_frame_prepare", "null_camera", {0: None}, "bad argument"),
    ("orbpl_line_frame_prepare", "negative_n", {2: -1}, "bad argument"),
    ("orbpl_line_frame_prepare", "null_key_lines", {1: None, 2: 1}, "bad argument"),
    ("orbpl_line_frame_prepare", "n_81", {2: 81}, CAP_KL),

    ("orbl_search_by_projection_last", "null_pose", {1: None}, "bad argument"),
    ("orbl_search_by_projection_last", "negative_ncur", {2: -1}, "bad argument"),
    ("orbl_search_by_projection_last", "negative_nlast", {5: -1}, "bad argument"),
    ("orbl_search_by_projection_last", "ncur_81", {2: 81}, CAP_KL),
    ("orbl_search_by_projection_last", "nlast_81", {5: 81}, CAP_KL),
    ("orbl_search_by_projection_last", "null_current_arrays", {2: 1, 4: None}, "NULL line arrays"),
    ("orbl_search_by_projection_last", "null_last_arrays", {5: 1, 9: None}, "NULL line arrays"),

    ("orbm_search_by_bow", "null_nmatches", {12: None}, "bad argument"),
    ("orbm_search_by_bow", "negative_nkf", {0: -1}, "bad argument"),
    ("orbm_search_by_bow", "negative_nf", {5: -1}, "bad argument"),
    ("orbm_search_by_bow", "nkf_2049", {0: 2049}, "more than 2048 features"),
    ("orbm_search_by_bow", "nf_2049", {5: 2049}, "more than 2048 features"),
    ("orbm_search_by_bow", "null_keyframe_arrays", {0: 1, 3: None}, "NULL feature arrays"),
    ("orbm_search_by_bow", "null_match", {5: 1, 11: None}, "NULL feature arrays"),
    ("orbm_search_by_bow", "keyframe_node_id", {0: 2, 1: lambda: ints(5, (1 << 21) - 1)}, NODE),
    ("orbm_search_by_bow", "frame_node_id", {5: 1, 6: lambda: ints((1 << 21) - 1)}, NODE),

    ("orbm_search_by_projection_kf", "null_current", {3: None}, "NULL argument"),
    ("orbm_search_by_projection_kf", "negative_n", {3: lambda: cur(-1)}, CAP_KP),
    ("orbm_search_by_projection_kf", "negative_nkf", {5: -1}, CAP_KP),
    ("orbm_search_by_projection_kf", "n_2049", {3: lambda: cur(2049)}, CAP_KP),
    ("orbm_search_by_projection_kf", "nkf_2049", {5: 2049}, CAP_KP),
    ("orbm_search_by_projection_kf", "null_pose", {3: lambda: cur(0, Tcw=None)},
     "NULL feature arrays"),
    ("orbm_search_by_projection_kf", "null_has_mp", {3: lambda: cur(1), 4: None},
     "NULL feature arrays"),
    ("orbm_search_by_projection_kf", "null_keyframe_arrays", {5: 1, 12: None},
     "NULL feature arrays"),

    ("orbpl_stereo_matches", "null_extractor", {1: None}, "bad argument"),
    ("orbpl_stereo_matches", "negative_n", {6: -1}, "bad argument"),
    ("orbpl_stereo_matches", "negative_nr", {9: -1}, "bad argument"),
    ("orbpl_stereo_matches", "n_4097", {6: 4097}, "more than 4096 keypoints"),
    ("orbpl_stereo_matches", "null_keypoints", {6: 1, 4: None}, "NULL keypoint arrays"),

    ("orbl_frame_is_in_frustum", "null_pose", {0: None}, "bad argument"),
    ("orbl_frame_is_in_frustum", "negative_n", {1: -1}, "bad argument"),
    ("orbl_frame_is_in_frustum", "null_lines", {1: 1, 2: None}, "bad argument"),

    ("orbl_search_by_projection_list", "null_nmatches", {11: None}, "bad argument"),
    ("orbl_search_by_projection_list", "negative_ncur", {2: -1}, "bad argument"),
    ("orbl_search_by_projection_list", "negative_nml", {6: -1}, "bad argument"),
    ("orbl_search_by_projection_list", "ncur_81", {2: 81}, CAP_KL),
    ("orbl_search_by_projection_list", "null_current_arrays", {2: 1, 10: None},
     "NULL line arrays"),
    ("orbl_search_by_projection_list", "null_map_line_arrays", {6: 1, 7: None},
     "NULL line arrays"),

    ("orbl_search_by_projection_pairs", "null_wiped", {21: None}, "bad argument"),
    ("orbl_search_by_projection_pairs", "null_nproj", {15: None}, "bad argument"),
    ("orbl_search_by_projection_pairs", "negative_ncur", {3: -1}, "bad argument"),
    ("orbl_search_by_projection_pairs", "negative_nml", {7: -1}, "bad argument"),
    ("orbl_search_by_projection_pairs", "negative_pair_cap", {17: -1}, "bad argument"),
    ("orbl_search_by_projection_pairs", "mode_2", {2: 2}, "bad argument"),
    ("orbl_search_by_projection_pairs", "ncur_81", {3: 81}, CAP_KL),
    ("orbl_search_by_projection_pairs", "null_current_arrays", {3: 1, 5: None},
     "NULL line arrays"),
    ("orbl_search_by_projection_pairs", "null_projection_output", {7: 1, 13: None},
     "NULL line arrays"),
    ("orbl_search_by_projection_pairs", "null_pairs", {16: None, 17: 1}, "NULL line arrays"),

    ("orbl_match_bf_knn", "null_nmatches", {5: None}, "bad argument"),
    ("orbl_match_bf_knn", "negative_nq", {0: -1}, "bad argument"),
    ("orbl_match_bf_knn", "negative_nt", {2: -1}, "bad argument"),
    ("orbl_match_bf_knn", "nq_257", {0: 257}, "more than 256 query descriptors"),
    ("orbl_match_bf_knn", "null_queries", {0: 1, 1: None}, "NULL descriptor arrays"),
    ("orbl_match_bf_knn", "null_output", {2: 1, 4: None}, "NULL descriptor arrays"),

    ("orbl_stereo_line_depths", "null_camera", {0: None}, "bad argument"),
    ("orbl_stereo_line_depths", "negative_nl", {3: -1}, "bad argument"),
    ("orbl_stereo_line_depths", "negative_nr", {6: -1}, "bad argument"),
    ("orbl_stereo_line_depths", "nl_81", {3: 81}, CAP_KL),
    ("orbl_stereo_line_depths", "nr_81", {6: 81}, CAP_KL),
    ("orbl_stereo_line_depths", "null_left_lines", {3: 1, 1: None}, "NULL line arrays"),
    ("orbl_stereo_line_depths", "null_left_descriptors", {3: 1, 2: None}, "NULL line arrays"),
    ("orbl_stereo_line_depths", "null_output", {3: 1, 8: None}, "NULL line arrays"),
    ("orbl_stereo_line_depths", "null_right_lines", {6: 1, 4: None}, "NULL line arrays"),
    ("orbl_stereo_line_depths", "null_right_descriptors", {6: 1, 5: None}, "NULL line arrays"),

    ("orbkf_detect_reloc", "scoring_1", {2: 1},
     "only the vocabulary's L1 scoring (L1_NORM = 0) is built"),
    ("orbkf_detect_reloc", "negative_nq", {1: -1}, "bad argument"),
    ("orbkf_detect_reloc", "null_problems", {0: None}, "bad argument"),
    ("orbkf_detect_reloc", "negative_nkf", {0: lambda: kfdb(nkf=-1)},
     "more than 64 keyframes in a database"),
    ("orbkf_detect_reloc", "nkf_65", {0: lambda: kfdb(nkf=65)},
     "more than 64 keyframes in a database"),
    ("orbkf_detect_reloc", "query_words_4097", {0: lambda: kfdb(nq_words=4097)},
     "more than 4096 entries in the query's BowVector"),
    ("orbkf_detect_reloc", "null_candidates", {0: lambda: kfdb(cand=None)}, "NULL output"),
    ("orbkf_detect_reloc", "null_query", {0: lambda: kfdb(nq_words=1, q_words=None)},
     "NULL query BowVector"),
    ("orbkf_detect_reloc", "null_keyframe_arrays", {0: lambda: kfdb(nkf=1, kf_off=None)},
     "NULL keyframe arrays"),
    ("orbkf_detect_reloc", "keyframe_words_4097",
     {0: lambda: kfdb(nkf=1, kf_off=ints(0, 4097))},
     "a keyframe's BowVector has a negative length or more than 4096 entries"),

    ("orbpnp_iterate", "negative_nsolvers", {1: -1}, "bad argument"),
    ("orbpnp_iterate", "null_problems", {0: None}, "bad argument"),
    ("orbpnp_iterate", "negative_n", {0: lambda: pnp(n=-1)}, "more than 2048 correspondences"),
    ("orbpnp_iterate", "n_2049", {0: lambda: pnp(n=2049)}, "more than 2048 correspondences"),
    ("orbpnp_iterate", "min_inliers_3", {0: lambda: pnp(min_inliers=3)},
     "min_inliers below the minimal set of 4"),
    ("orbpnp_iterate", "null_state", {0: lambda: pnp(iterations=None)}, "NULL state or output"),
    ("orbpnp_iterate", "null_correspondences", {0: lambda: pnp(n=1, p2d=None)},
     "NULL correspondence arrays"),
    ("orbpnp_iterate", "negative_iterations", {0: lambda: pnp(iterations=ints(-1))},
     "negative iteration count"),
    ("orbpnp_iterate", "hypotheses_321", {0: lambda: pnp(n=4), 2: 321},
     "more hypotheses in one call than ORBPNP_MAX_ITERATIONS"),
    ("orbpnp_iterate", "too_few_draws", {0: lambda: pnp(n=4, n_draws=3)},
     "fewer draws than 4 per hypothesis"),

    ("orblm_create_new_map_features", "null_camera", {0: None}, "NULL camera or scale tables"),
    ("orblm_create_new_map_features", "nlevels_1", {3: 1}, "nlevels outside [2, 16]"),
    ("orblm_create_new_map_features", "negative_n", {5: -1}, "bad argument"),
    ("orblm_create_new_map_features", "null_problems", {4: None}, "bad argument"),
    ("orblm_create_new_map_features", "negative_neighbours", {4: lambda: lm_problem(n_neigh=-1)},
     "more than 10 neighbours"),
    ("orblm_create_new_map_features", "neighbours_11", {4: lambda: lm_problem(n_neigh=11)},
     "more than 10 neighbours"),
    ("orblm_create_new_map_features", "null_neighbours",
     {4: lambda: lm_problem(n_neigh=1, neigh=None)}, "NULL neighbour list"),
    ("orblm_create_new_map_features", "null_keyframe_pose", {4: lambda: lm_problem(Tcw=None)},
     "NULL keyframe pose"),
    ("orblm_create_new_map_features", "negative_features", {4: lambda: lm_problem(n=-1)},
     "keyframe with more than 2048 features"),
    ("orblm_create_new_map_features", "features_2049", {4: lambda: lm_problem(n=2049)},
     "keyframe with more than 2048 features"),
    ("orblm_create_new_map_features", "null_keyframe_arrays",
     {4: lambda: lm_problem(n=1, kps=None)}, "NULL keyframe arrays"),
    ("orblm_create_new_map_features", "octave_out_of_range",
     {3: 2, 4: lambda: lm_problem(n=2, kps_un=octaves(1, 2))},
     "keypoint octave outside [0, nlevels)"),
    ("orblm_create_new_map_features", "node_id",
     {4: lambda: lm_problem(n=2, feat_node=ints(0, (1 << 21) - 1))}, NODE),
    ("orblm_create_new_map_features", "negative_lines", {4: lambda: lm_problem(nl=-1)},
     "keyframe with more than 256 lines"),
    ("orblm_create_new_map_features", "lines_257", {4: lambda: lm_problem(nl=257)},
     "keyframe with more than 256 lines"),
    ("orblm_create_new_map_features", "null_line_arrays",
     {4: lambda: lm_problem(nl=1, klines=None)}, "NULL keyframe line arrays"),
    ("orblm_create_new_map_features", "null_outputs", {4: lambda: lm_problem(n=1, points=None)},
     "NULL output arrays"),
    ("orblm_create_new_map_features", "neighbour_features_2049",
     {4: lambda: lm_problem(n_neigh=1, neigh=lm_neigh(n=2049))},
     "keyframe with more than 2048 features"),

    ("orbm_search_for_triangulation", "null_scale_tables", {1: None}, "NULL camera or scale tables"),
    ("orbm_search_for_triangulation", "nlevels_17", {3: 17}, "nlevels outside [2, 16]"),
    ("orbm_search_for_triangulation", "null_keyframe", {4: None}, "bad argument"),
    ("orbm_search_for_triangulation", "null_npairs", {10: None}, "bad argument"),
    ("orbm_search_for_triangulation", "negative_features", {4: lambda: kfp(n=-1)},
     "keyframe with more than 2048 features"),
    ("orbm_search_for_triangulation", "features_2049", {5: lambda: kfp(n=2049)},
     "keyframe with more than 2048 features"),
    ("orbm_search_for_triangulation", "null_keyframe_arrays", {5: lambda: kfp(n=1, kps=None)},
     "NULL keyframe arrays"),
    ("orbm_search_for_triangulation", "null_pairs", {4: lambda: kfp(n=1), 9: None}, "NULL pairs"),

    ("orbl_search_for_triangulation", "null_npairs", {5: None}, "bad argument"),
    ("orbl_search_for_triangulation", "negative_nl1", {0: -1}, "bad argument"),
    ("orbl_search_for_triangulation", "negative_nl2", {2: -1}, "bad argument"),
    ("orbl_search_for_triangulation", "nl1_257", {0: 257}, "more than 256 lines"),
    ("orbl_search_for_triangulation", "nl2_257", {2: 257}, "more than 256 lines"),
    ("orbl_search_for_triangulation", "null_descriptors", {0: 1, 1: None}, "NULL line arrays"),
    ("orbl_search_for_triangulation", "null_pairs", {0: 1, 4: None}, "NULL line arrays"),
]


def test_every_host_entry_point_has_null_negative_and_capacity_rows():
    for name in GOOD:
        cases = " ".join(c for n, c, _, _ in ROWS if n == name)
        assert "null" in cases and "negative" in cases, name
    ids = [f"{n}-{c}" for n, c, _, _ in ROWS]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("name,case,change,message", ROWS, ids=[f"{n}-{c}" for n, c, _, _ in ROWS])
def test_refused_before_any_device_call(name, case, change, message):
    L = orbpl.lib()
    fn = getattr(L, name)
    args = GOOD[name]()
    for pos, v in change.items():
        args[pos] = v() if callable(v) else v
    for pos, t in enumerate(fn.argtypes):
        if t is _P:
            args[pos] = None if args[pos] is None else _as_int_ptr(args[pos])
    rc = fn(*args)
    text = L.orbpl_last_error().decode()
    assert (rc, text) == (orbpl.ORBPL_ERR_ARG, message)


def test_stereo_tracker_refuses_more_than_1024_rows():
    """k_stereo's row table holds 1024 rows: a stereo tracker for a taller
    image is refused at creation, before any device call. The level count needs no refusal of its own: the stereo level table holds the
    extractor's 16 (orbx_create refuses 17 for every tracker)."""
    L = orbpl.lib()
    p = orbpl.OrbParams(500, 1.1, 12, 20, 7)
    tall = orbpl.Camera(525.0, 525.0, 319.5, 239.5, 0.0, 0.0, 0.0, 0.0, 0.0, 40.0, 3.0, 640, 1025)
    h = C.c_void_p()
    rc = L.orbpl_tracker_create_ex(C.byref(p), C.byref(tall), 1, 0, orbpl.Tracker.TRACK_STEREO,
                                   C.byref(h))
    assert (rc, L.orbpl_last_error().decode()) == (
        orbpl.ORBPL_ERR_ARG, "stereo tracking supports images up to 1024 rows")
    assert not h.value
