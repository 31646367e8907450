"""ctypes binding of libsvo_hip.so (include/svo_abi.h).  No compute happens in Python."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

MEM_HOST, MEM_DEVICE = 0, 1

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


class SvoError(RuntimeError):
    pass


class Config(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("max_keypoints", C.c_int32),
                ("max_batch", C.c_int32), ("num_slots", C.c_int32), ("fast_threshold", C.c_int32),
                ("num_features_tracking", C.c_int32), ("iterations", C.c_int32),
                ("reproj_err", C.c_float), ("confidence", C.c_float),
                ("feature_match_error", C.c_double), ("inlier_rate", C.c_double),
                ("min_move2", C.c_double), ("max_move2", C.c_double),
                ("P1", C.c_double * 12), ("P2", C.c_double * 12),
                ("track_mode", C.c_int32), ("orb_nfeatures", C.c_int32), ("orb_scale_factor", C.c_float),
                ("orb_nlevels", C.c_int32), ("orb_ini_th", C.c_int32), ("orb_min_th", C.c_int32),
                ("lk_accum", C.c_int32), ("fast_keep_strongest", C.c_int32)]


MODE_LK, MODE_ORB = 0, 1
DETECTOR_FAST, DETECTOR_GFTT = 0, 1                                                         # svo_set_lk_detector
INTERP_NEAREST, INTERP_LINEAR = 0, 1                                                        # svo_resize / svo_ingest_create
LK_ACCUM_EXACT, LK_ACCUM_SSE2, LK_ACCUM_SIMD128, LK_ACCUM_SSE2_LEGACY = 0, 1, 2, 3          # svo_config.lk_accum


class PnPResult(C.Structure):
    _fields_ = [("rvec", C.c_double * 3), ("tvec", C.c_double * 3), ("R", C.c_double * 9),
                ("n_inliers", C.c_int32), ("ransac_iters", C.c_int32), ("best_iter", C.c_int32),
                ("lm_iters", C.c_int32), ("ok", C.c_int32), ("_pad", C.c_int32)]


class RefineResult(C.Structure):
    """svo_refine_result: the outcome of the pose refinement stage for one pair."""
    _fields_ = [("rvec", C.c_double * 3), ("tvec", C.c_double * 3), ("R", C.c_double * 9),
                ("pnp_rvec", C.c_double * 3), ("pnp_tvec", C.c_double * 3), ("info", C.c_double * 36),
                ("cost_first", C.c_double), ("cost_last", C.c_double),
                ("n_points", C.c_int32), ("n_active", C.c_int32), ("iters", C.c_int32), ("views", C.c_int32),
                ("status", C.c_int32), ("_pad", C.c_int32)]


ORB_MATCHER_BRUTE, ORB_MATCHER_GUIDED = 0, 1                                               # svo_set_orb_matcher
REFINE_OFF, REFINE_REPROJ, REFINE_BA = 0, 1, 2                          # svo_set_pose_refine
REFINE_APPLIED, REFINE_KEPT_PNP, REFINE_SKIPPED = 0, 1, 2              # svo_refine_result.status


class StepResult(C.Structure):
    _fields_ = [("ok", C.c_int32), ("fail_stage", C.c_int32), ("n_prev_kps", C.c_int32),
                ("n_cur_kps", C.c_int32), ("n_tracked", C.c_int32), ("n_inliers", C.c_int32),
                ("ransac_iters", C.c_int32), ("lm_iters", C.c_int32),
                ("rvec", C.c_double * 3), ("tvec", C.c_double * 3), ("R", C.c_double * 9),
                ("T_rel_inv", C.c_double * 16), ("pose", C.c_double * 16)]


STEP_DTYPE = np.dtype([("ok", "<i4"), ("fail_stage", "<i4"), ("n_prev_kps", "<i4"),
                       ("n_cur_kps", "<i4"), ("n_tracked", "<i4"), ("n_inliers", "<i4"),
                       ("ransac_iters", "<i4"), ("lm_iters", "<i4"), ("rvec", "<f8", 3),
                       ("tvec", "<f8", 3), ("R", "<f8", 9), ("T_rel_inv", "<f8", 16),
                       ("pose", "<f8", 16)])
assert STEP_DTYPE.itemsize == C.sizeof(StepResult)


WINDOW_MAX_FRAMES = 8
_WINDOW_COLS = ("counts", "poses", "ids", "X", "seen", "active", "obs_left", "obs_right")


class WindowTable(C.Structure):
    """svo_window_table: the columns of a sliding-window landmark table as raw pointers."""
    _fields_ = [(k, C.c_void_p) for k in _WINDOW_COLS]


class WindowResult(C.Structure):
    """svo_window_result: the outcome of svo_window_ba."""
    _fields_ = [(k, C.c_int32) for k in ("status", "n_frames", "n_landmarks", "n_usable", "n_obs", "n_active", "iters", "_pad")] + [
        ("frame_active", C.c_int32 * WINDOW_MAX_FRAMES), ("cost_first", C.c_double), ("cost_last", C.c_double), ("info", C.c_double * (42 * 42))]

    def as_dict(self):
        d = {k: getattr(self, k) for k in ("status", "n_frames", "n_landmarks", "n_usable", "n_obs", "n_active", "iters", "cost_first", "cost_last")}
        d["frame_active"] = np.array(self.frame_active, np.int32)
        d["info"] = np.array(self.info, np.float64).reshape(42, 42)
        return d


KF_NONE, KF_SHORT, KF_PAIR_FAILED, KF_REJECTED, KF_APPLIED = 0, 1, 2, 3, 4


class KeyframeResult(C.Structure):
    """svo_keyframe_result: what keyframe mode did in the last add_frame step."""
    _fields_ = [(k, C.c_int32) for k in ("status", "switched", "kf_index", "gap", "n_rows", "n_join", "n_inliers", "ransac_iters",
                                         "lm_iters", "_pad")] + [
        ("rvec", C.c_double * 3), ("tvec", C.c_double * 3), ("pose_K", C.c_double * 16), ("pose_pair", C.c_double * 16)]

    def as_dict(self):
        d = {k: getattr(self, k) for k in ("status", "switched", "kf_index", "gap", "n_rows", "n_join", "n_inliers", "ransac_iters", "lm_iters")}
        d["rvec"], d["tvec"] = np.array(self.rvec, np.float64), np.array(self.tvec, np.float64)
        d["pose_K"], d["pose_pair"] = np.array(self.pose_K, np.float64).reshape(4, 4), np.array(self.pose_pair, np.float64).reshape(4, 4)
        return d


def library_path():
    return os.path.join(_HERE, "libsvo_hip.so")


def build_library(force=False):
    """hipcc --offload-arch=gfx950 build of csrc/ into libsvo_hip.so (cross-compiles without a GPU)."""
    args = ["make", "-C", os.path.join(_HERE, "csrc"), "-j8"]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return library_path()


def load_library():
    """dlopen libsvo_hip.so; raises SvoError when it is missing (there is no CPU fallback)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise SvoError(f"{path} is missing: run __graft_entry__.build() (hipcc) first; "
                       "this package has no CPU fallback")
    lib = C.CDLL(path)
    if lib.svo_config_bytes() != C.sizeof(Config):
        raise SvoError(f"{path}: svo_config is {lib.svo_config_bytes()} bytes, this binding's Config {C.sizeof(Config)} "
                       "(stale build? run __graft_entry__.build())")
    lib.svo_last_error.restype = C.c_char_p
    lib.svo_last_error.argtypes = [C.c_void_p]
    lib.svo_create.argtypes = [C.POINTER(Config), C.c_int, C.POINTER(C.c_void_p)]
    lib.svo_destroy.argtypes = [C.c_void_p]
    lib.svo_destroy.restype = None
    lib.svo_default_config.argtypes = [C.POINTER(Config), C.c_int, C.c_int]
    lib.svo_default_config.restype = None
    lib.svo_track_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_int]
    lib.svo_get_frame_keypoints.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.svo_get_last_tracks.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_int, C.POINTER(C.c_int)]
    lib.svo_get_batch_tracks.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.POINTER(C.c_int)]
    lib.svo_chain_relative.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    lib.svo_host_alloc.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
    lib.svo_host_free.argtypes = [C.c_void_p, C.c_void_p]
    lib.svo_upload_frames.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int]
    lib.svo_upload_frames_at.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int]
    lib.svo_wait_stream.argtypes = [C.c_void_p, C.c_void_p]
    lib.svo_signal_stream.argtypes = [C.c_void_p, C.c_void_p]
    lib.svo_signal_stream_inputs.argtypes = [C.c_void_p, C.c_void_p]
    lib.svo_wait_upload.argtypes = [C.c_void_p, C.c_int]
    lib.svo_track_uploaded.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    lib.svo_track_uploaded_async.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    lib.svo_collect_results.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.svo_results_ready.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    lib.svo_set_pose.argtypes = [C.c_void_p, C.c_void_p]
    # stream sets (additive entry points: a library without them is a stale build, and that is an error, not a fallback)
    lib.svo_streams_create.argtypes = [C.c_void_p, C.c_int]
    lib.svo_streams_count.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    lib.svo_streams_step.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int,
                                     C.c_void_p, C.c_int]
    lib.svo_streams_reset.argtypes = [C.c_void_p, C.c_int]
    lib.svo_streams_get_pose.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.svo_streams_set_pose.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.svo_streams_get_tracks.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.POINTER(C.c_int)]
    # cv::resize and the ingest stage (additive entry points, like the stream sets)
    lib.svo_scale_projection.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_void_p]
    lib.svo_resize.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64,
                               C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int]
    lib.svo_ingest_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double]
    lib.svo_ingest_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                    C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.svo_ingest_add_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.svo_ingest_track_batch.argtypes = lib.svo_track_batch.argtypes
    lib.svo_ingest_streams_step.argtypes = lib.svo_streams_step.argtypes
    lib.svo_ingest_upload_frames_at.argtypes = lib.svo_upload_frames_at.argtypes
    # FAST corner buckets (additive entry points, like the stream sets)
    lib.svo_set_fast_buckets.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.svo_get_fast_buckets.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.svo_bucket_corners.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    # Shi-Tomasi corners (additive entry points, like the stream sets)
    lib.svo_set_lk_detector.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double]
    lib.svo_get_lk_detector.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double),
                                        C.POINTER(C.c_double)]
    lib.svo_min_eigen_map.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    lib.svo_gftt_detect.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                    C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.svo_set_pose_refine.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int]
    lib.svo_get_pose_refine.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                        C.POINTER(C.c_double), C.POINTER(C.c_int)]
    lib.svo_refine_pose.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.POINTER(RefineResult), C.c_void_p, C.c_int]
    lib.svo_get_refine_result.argtypes = [C.c_void_p, C.c_int, C.POINTER(RefineResult), C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.svo_set_pose_refine_ba.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int]
    lib.svo_refine_ba.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.POINTER(RefineResult), C.c_void_p, C.c_void_p, C.c_int]
    lib.svo_get_refine_points.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    # guided ORB matcher (additive entry points, like the stream sets)
    lib.svo_set_orb_matcher.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double]
    lib.svo_get_orb_matcher.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                        C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.svo_orb_stereo_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.svo_orb_track_frames.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int, C.POINTER(C.c_int)]
    lib.svo_get_frame_stereo.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.svo_set_track_carry.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int]
    lib.svo_get_track_carry.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int)]
    lib.svo_carry_merge.argtypes = ([C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int] + [C.c_void_p] * 5 + [C.c_int] +
                                    [C.c_void_p] * 2 + [C.c_int, C.c_int64] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 2 + [C.c_int])
    lib.svo_get_frame_track_ids.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.svo_get_last_track_ids.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.svo_streams_get_track_ids.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.svo_streams_get_frame_tracks.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.svo_set_window_ba.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int]
    lib.svo_get_window_ba.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double),
                                      C.POINTER(C.c_int)]
    lib.svo_get_window.argtypes = [C.c_void_p, C.POINTER(WindowTable), C.c_int]
    lib.svo_get_window_result.argtypes = [C.c_void_p, C.c_void_p]
    lib.svo_window_ba.argtypes = [C.c_void_p, C.POINTER(WindowTable), C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int,
                                  C.c_void_p, C.c_int]
    lib.svo_window_update.argtypes = ([C.c_void_p, C.c_int, C.POINTER(WindowTable), C.POINTER(WindowTable), C.c_int] + [C.c_void_p] * 6 +
                                      [C.c_int, C.c_void_p, C.c_void_p, C.c_int])
    lib.svo_set_keyframe.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.svo_get_keyframe.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.svo_get_keyframe_result.argtypes = [C.c_void_p, C.POINTER(KeyframeResult)]
    lib.svo_get_keyframe_matches.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_int, C.POINTER(C.c_int)]
    lib.svo_get_keyframe_table.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.svo_keyframe_join.argtypes = ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4 +
                                      [C.c_int, C.c_void_p, C.c_int])
    _LIB = lib
    return lib


def _interp(interp):
    """SVO_INTERP_* of "nearest" / "linear" (or the constant itself)."""
    if isinstance(interp, str):
        if interp not in ("nearest", "linear"):
            raise ValueError(f"interp must be 'nearest' or 'linear', not {interp!r}")
        return INTERP_LINEAR if interp == "linear" else INTERP_NEAREST
    return int(interp)


def scale_projection(P, inv_x, inv_y, interp="nearest"):
    """svo_scale_projection: the 3 x 4 projection matrix of an image resized by (inv_x, inv_y) -- what a context that tracks
    resized frames is created with.  Host arithmetic only (no device, no context)."""
    P = np.ascontiguousarray(P, np.float64).reshape(12)
    out = np.zeros(12)
    rc = load_library().svo_scale_projection(C.c_void_p(P.ctypes.data), float(inv_x), float(inv_y), _interp(interp),
                                             C.c_void_p(out.ctypes.data))
    if rc != 0:
        raise SvoError(f"svo_scale_projection failed ({rc}): inv must be in (0, 1], interp nearest or linear")
    return out.reshape(3, 4)


def device_count():
    """svo_device_count: HIP devices visible to this process (0 when there is none)."""
    n = C.c_int(0)
    load_library().svo_device_count(C.byref(n))
    return n.value


def default_config(width, height, **overrides):
    cfg = Config()
    load_library().svo_default_config(C.byref(cfg), int(width), int(height))
    for k, v in overrides.items():
        if k in ("P1", "P2"):
            arr = getattr(cfg, k)
            for i, x in enumerate(np.asarray(v, np.float64).reshape(12)):
                arr[i] = float(x)
        else:
            setattr(cfg, k, v)
    return cfg


def _ptr(a):
    """Raw pointer + memory kind of a numpy array (host) or a torch tensor (host or cuda)."""
    if a is None:
        return None, MEM_HOST
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return C.c_void_p(a.ctypes.data), MEM_HOST
    # torch tensor
    assert a.is_contiguous()
    return C.c_void_p(a.data_ptr()), (MEM_DEVICE if a.is_cuda else MEM_HOST)


def _pose_ptr(pose0):
    """Pointer to the 16 doubles of a pose (it keeps its array alive), or None."""
    if pose0 is None:
        return None
    return np.ascontiguousarray(pose0, np.float64).reshape(16).ctypes.data_as(C.c_void_p)


def _records(n, results):
    """(out object, pointer, memory kind) of n step records: a fresh host array, or the caller's cuda tensor."""
    if results is None:
        out = np.zeros(n, dtype=STEP_DTYPE)
        return out, C.c_void_p(out.ctypes.data), MEM_HOST
    return results, C.c_void_p(results.data_ptr()), MEM_DEVICE


class Context:
    """One svo_ctx: owns every device buffer of the hot path on one GPU."""

    def __init__(self, width, height, device=0, **cfg_overrides):
        self.lib = load_library()
        self.cfg = default_config(width, height, **cfg_overrides)
        h = C.c_void_p()
        rc = self.lib.svo_create(C.byref(self.cfg), int(device), C.byref(h))
        if rc != 0:
            raise SvoError(f"svo_create failed with {rc} (no usable HIP device?) -- there is no CPU fallback")
        self.h = h
        self.width, self.height = int(width), int(height)

    def close(self):
        if getattr(self, "h", None):
            self.lib.svo_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, allow_soft=False):
        if rc < 0 or (rc > 0 and not allow_soft):
            raise SvoError(f"svo call failed ({rc}): {self.lib.svo_last_error(self.h).decode()}")
        return rc

    # ---- misc -------------------------------------------------------------------------------
    def sync(self):
        self._check(self.lib.svo_sync(self.h))

    def set_stream(self, stream_handle):
        self._check(self.lib.svo_set_stream(self.h, C.c_void_p(stream_handle)))
        self._stream_handle = int(stream_handle or 0)

    def wait_stream(self, stream_handle):
        """The context's stream waits ON THE DEVICE for everything queued on `stream_handle` so far (svo_wait_stream, ABI v7):
        call it before handing the library a device buffer another stream is still filling."""
        self._check(self.lib.svo_wait_stream(self.h, C.c_void_p(stream_handle)))

    def signal_stream(self, stream_handle):
        """`stream_handle` waits ON THE DEVICE for everything the context has queued so far, the side-stream pose stage of
        an overlap-mode batch included (svo_signal_stream): what a consumer of device-resident results on another stream
        calls instead of svo_sync()."""
        self._check(self.lib.svo_signal_stream(self.h, C.c_void_p(stream_handle)))

    def signal_stream_inputs(self, stream_handle):
        """`stream_handle` waits ON THE DEVICE until the kernels that read the caller's frames have run (the front end);
        the side-stream pose stage is NOT waited for (svo_signal_stream_inputs, ABI v9)."""
        self._check(self.lib.svo_signal_stream_inputs(self.h, C.c_void_p(stream_handle)))

    def _order_in(self, t):
        """Tensors torch has just produced (an output's zero fill is a kernel on TORCH's current stream; an input may still
        be being written there) are ordered before the library's kernels on the device -- no host synchronisation."""
        import torch
        other = torch.cuda.current_stream(t.device).cuda_stream
        if other and other == getattr(self, "_stream_handle", 0):
            return False                   # the context was handed this very stream (set_stream): already in order
        self.wait_stream(other)
        return True

    def _order_out(self, t):
        """... and what the library wrote into them before whatever torch's current stream does next."""
        import torch
        other = torch.cuda.current_stream(t.device).cuda_stream
        if other and other == getattr(self, "_stream_handle", 0):
            return                         # (and a signal would make the next front end wait for this batch's pose stage)
        self.signal_stream(other)

    @property
    def num_levels(self):
        return self.lib.svo_num_levels(self.h)

    def set_overlap(self, on=True):
        """Pose stage of batch k on a side stream, overlapped with batch k+1's front end."""
        self._check(self.lib.svo_set_overlap(self.h, int(on)))

    def wait_results(self):
        self._check(self.lib.svo_wait_results(self.h))

    def enable_timing(self, on=True):
        self._check(self.lib.svo_enable_timing(self.h, int(on)))

    def get_timing(self):
        names = (C.c_char_p * 64)()
        ms = (C.c_float * 64)()
        n = self.lib.svo_get_timing(self.h, names, ms, 64)
        return [(names[i].decode(), float(ms[i])) for i in range(n)]

    # ---- stage API --------------------------------------------------------------------------
    def _img(self, img, shape=None):
        """(pointer, row pitch in bytes, memory kind) of a u8 image of the context's size (or of `shape`); rows may be padded
        (pitch >= width)."""
        shape = shape or (self.height, self.width)
        assert tuple(img.shape) == tuple(shape), (tuple(img.shape), shape)
        if isinstance(img, np.ndarray):
            assert img.dtype == np.uint8 and img.strides[1] == 1
            return C.c_void_p(img.ctypes.data), int(img.strides[0]), MEM_HOST
        assert img.element_size() == 1 and img.stride(1) == 1
        return C.c_void_p(img.data_ptr()), int(img.stride(0)), (MEM_DEVICE if img.is_cuda else MEM_HOST)

    def fast_detect(self, img, threshold=20, nonmax=True, cap=None):
        cap = cap or self.cfg.max_keypoints
        p, pitch, mem = self._img(img)
        out = np.zeros(cap, dtype=KP_DTYPE)
        n = C.c_int(0)
        self._check(self.lib.svo_fast_detect(self.h, p, pitch, mem, int(threshold), int(bool(nonmax)),
                                             C.c_void_p(out.ctypes.data), cap, C.byref(n)))
        return out[:n.value].copy()

    def build_pyramid(self, slot, img):
        p, pitch, mem = self._img(img)
        self._check(self.lib.svo_build_pyramid(self.h, int(slot), p, pitch, mem))

    def read_pyramid_level(self, slot, level):
        w, h = C.c_int(0), C.c_int(0)
        self._check(self.lib.svo_read_pyramid_level(self.h, slot, level, None, 0, MEM_HOST,
                                                    C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), np.uint8)
        self._check(self.lib.svo_read_pyramid_level(self.h, slot, level, C.c_void_p(out.ctypes.data),
                                                    w.value, MEM_HOST, C.byref(w), C.byref(h)))
        return out

    def lk_track(self, slot_prev, slot_next, pts):
        """pts: (n,2) float32 numpy (host) or torch cuda tensor -> (next_pts, status), same kind."""
        if isinstance(pts, np.ndarray):
            pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
            n = pts.shape[0]
            out = np.zeros((n, 2), np.float32)
            st = np.zeros(n, np.uint8)
        else:
            import torch
            n = pts.shape[0]
            out = torch.zeros((n, 2), dtype=torch.float32, device=pts.device)
            st = torch.zeros(n, dtype=torch.uint8, device=pts.device)
            self._order_in(st)
        pi, mem = _ptr(pts)
        po, _ = _ptr(out)
        ps, _ = _ptr(st)
        self._check(self.lib.svo_lk_track(self.h, slot_prev, slot_next, pi, n, po, ps, mem))
        if mem == MEM_DEVICE:
            self._order_out(st)
        return out, st

    def circular_match(self, slots, t1_left):
        """slots = (prevL, prevR, curL, curR); returns the four compacted (M,2) arrays."""
        if isinstance(t1_left, np.ndarray):
            t1_left = np.ascontiguousarray(t1_left, np.float32).reshape(-1, 2)
            n = t1_left.shape[0]
            outs = [np.zeros((max(n, 1), 2), np.float32) for _ in range(4)]
        else:
            import torch
            n = t1_left.shape[0]
            outs = [torch.zeros((max(n, 1), 2), dtype=torch.float32, device=t1_left.device) for _ in range(4)]
            self._order_in(outs[0])
        pi, mem = _ptr(t1_left)
        m = C.c_int(0)
        self._check(self.lib.svo_circular_match(self.h, *[int(s) for s in slots], pi, n,
                                                *[_ptr(o)[0] for o in outs], C.byref(m), mem))
        return [o[:m.value] for o in outs]

    def triangulate(self, P1, P2, x1, x2):
        P1 = np.ascontiguousarray(P1, np.float64).reshape(12)
        P2 = np.ascontiguousarray(P2, np.float64).reshape(12)
        if isinstance(x1, np.ndarray):
            x1 = np.ascontiguousarray(x1, np.float32).reshape(-1, 2)
            x2 = np.ascontiguousarray(x2, np.float32).reshape(-1, 2)
            out = np.zeros((x1.shape[0], 3), np.float32)
        else:
            import torch
            out = torch.zeros((x1.shape[0], 3), dtype=torch.float32, device=x1.device)
            self._order_in(out)
        p1, mem = _ptr(x1)
        p2, _ = _ptr(x2)
        self._check(self.lib.svo_triangulate(self.h, C.c_void_p(P1.ctypes.data), C.c_void_p(P2.ctypes.data),
                                             p1, p2, x1.shape[0], _ptr(out)[0], mem))
        if mem == MEM_DEVICE:
            self._order_out(out)
        return out

    def pnp_ransac(self, obj, img, K, iterations=500, reproj_err=0.5, confidence=0.99):
        K = np.ascontiguousarray(K, np.float64).reshape(9)
        if isinstance(obj, np.ndarray):
            obj = np.ascontiguousarray(obj, np.float32).reshape(-1, 3)
            img = np.ascontiguousarray(img, np.float32).reshape(-1, 2)
            mask = np.zeros(max(obj.shape[0], 1), np.uint8)
        else:
            import torch
            mask = torch.zeros(max(obj.shape[0], 1), dtype=torch.uint8, device=obj.device)
            self._order_in(mask)
        n = obj.shape[0]
        res = PnPResult()
        po, mem = _ptr(obj)
        conf = float(np.float32(confidence))      # a float at reference src/tracking.cpp:481
        self._check(self.lib.svo_pnp_ransac(self.h, po, _ptr(img)[0], n, C.c_void_p(K.ctypes.data),
                                            int(iterations), C.c_float(reproj_err), C.c_double(conf),
                                            C.byref(res), _ptr(mask)[0], mem))
        if mem == MEM_DEVICE:
            self._order_out(mask)
            mask = mask.cpu().numpy()
        return dict(ok=res.ok, rvec=np.array(res.rvec), tvec=np.array(res.tvec),
                    R=np.array(res.R).reshape(3, 3), n_inliers=res.n_inliers,
                    ransac_iters=res.ransac_iters, best_iter=res.best_iter, lm_iters=res.lm_iters,
                    mask=np.asarray(mask[:n]).copy())

    # ---- robust two-view pose refinement after solvePnPRansac (svo_set_pose_refine) -----------
    def set_pose_refine(self, mode, rounds=4, iters=10, sigma_px=1.0, min_inliers=6):
        """"reproj": every fused entry point refines each pair's PnP pose on both cameras' t2 observations; "ba": it adjusts the
        pose and the triangulated points together on the observations of both times; "off": as before."""
        names = {"off": REFINE_OFF, "none": REFINE_OFF, "reproj": REFINE_REPROJ, "ba": REFINE_BA}
        m = names[mode] if isinstance(mode, str) and mode in names else mode
        if isinstance(m, str):
            raise SvoError(f"pose refinement mode must be 'reproj', 'ba' or 'off', not {mode!r}")
        if m == REFINE_BA:                 # (svo_set_pose_refine refuses every mode but OFF and REPROJ: the mode has its own setter)
            self._check(self.lib.svo_set_pose_refine_ba(self.h, int(rounds), int(iters), float(sigma_px), int(min_inliers)))
            return
        self._check(self.lib.svo_set_pose_refine(self.h, int(m), int(rounds), int(iters), float(sigma_px), int(min_inliers)))

    def pose_refine(self):
        """(mode name, rounds, iters, sigma_px, min_inliers) as set."""
        m, r, i, n = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        sg = C.c_double()
        self._check(self.lib.svo_get_pose_refine(self.h, C.byref(m), C.byref(r), C.byref(i), C.byref(sg), C.byref(n)))
        return {REFINE_REPROJ: "reproj", REFINE_BA: "ba"}.get(m.value, "off"), r.value, i.value, sg.value, n.value

    @staticmethod
    def _refine_dict(res, active):
        return dict(status=res.status, rvec=np.array(res.rvec), tvec=np.array(res.tvec), R=np.array(res.R).reshape(3, 3),
                    pnp_rvec=np.array(res.pnp_rvec), pnp_tvec=np.array(res.pnp_tvec), info=np.array(res.info).reshape(6, 6),
                    cost_first=res.cost_first, cost_last=res.cost_last, n_points=res.n_points, n_active=res.n_active,
                    iters=res.iters, views=res.views, active=active)

    def refine_pose(self, obj, img_left, img_right, P1, P2, rvec0, tvec0):
        """svo_refine_pose: the refinement stage on a caller's points (numpy arrays, or cuda tensors) with the current settings;
        img_right None: one view."""
        P1 = np.ascontiguousarray(P1, np.float64).reshape(12)
        P2 = np.ascontiguousarray(P2, np.float64).reshape(12)
        r0 = np.ascontiguousarray(rvec0, np.float64).reshape(3)
        t0 = np.ascontiguousarray(tvec0, np.float64).reshape(3)
        if isinstance(obj, np.ndarray):
            obj = np.ascontiguousarray(obj, np.float32).reshape(-1, 3)
            img_left = np.ascontiguousarray(img_left, np.float32).reshape(-1, 2)
            if img_right is not None:
                img_right = np.ascontiguousarray(img_right, np.float32).reshape(-1, 2)
            act = np.zeros(max(obj.shape[0], 1), np.uint8)
        else:
            import torch
            for name, t, cols in (("obj", obj, 3), ("img_left", img_left, 2), ("img_right", img_right, 2)):
                if t is None:
                    continue
                if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == cols and t.is_contiguous()
                        and t.device == obj.device and t.shape[0] == obj.shape[0]):
                    raise SvoError(f"refine_pose: {name} must be a contiguous float32 tensor of shape (n, {cols}) on the device of obj")
            act = torch.zeros(max(obj.shape[0], 1), dtype=torch.uint8, device=obj.device)
            self._order_in(act)
        n = obj.shape[0]
        if img_left.shape[0] != n or (img_right is not None and img_right.shape[0] != n):
            raise SvoError("refine_pose: obj, img_left and img_right must have the same number of points")
        res = RefineResult()
        po, mem = _ptr(obj)
        self._check(self.lib.svo_refine_pose(self.h, po, _ptr(img_left)[0], _ptr(img_right)[0], n, C.c_void_p(P1.ctypes.data),
                                             C.c_void_p(P2.ctypes.data), C.c_void_p(r0.ctypes.data), C.c_void_p(t0.ctypes.data),
                                             C.byref(res), _ptr(act)[0], mem))
        if mem == MEM_DEVICE:
            self._order_out(act)
            act = act.cpu().numpy()
        return self._refine_dict(res, np.asarray(act[:n]).copy())

    def refine_result(self, pair=0, cap=None):
        """svo_get_refine_result: the record and the active flags of pair `pair` of the most recent fused launch."""
        res = RefineResult()
        cap = int(self.cfg.max_keypoints) if cap is None else int(cap)      # a pair never has more points
        act = np.zeros(max(cap, 1), np.uint8)
        n = C.c_int(0)
        self._check(self.lib.svo_get_refine_result(self.h, int(pair), C.byref(res), C.c_void_p(act.ctypes.data), cap, C.byref(n)))
        return self._refine_dict(res, act[:n.value].copy())

    def refine_ba(self, obj, img1_left, img1_right, img2_left, img2_right, P1, P2, rvec0, tvec0):
        """svo_refine_ba: the stage's bundle-adjustment mode on a caller's points (numpy arrays, or cuda tensors) with the
        current settings; img2_right None: three views.  The dict of refine_pose plus 'X', the (n, 3) float64 points that stand."""
        P1 = np.ascontiguousarray(P1, np.float64).reshape(12)
        P2 = np.ascontiguousarray(P2, np.float64).reshape(12)
        r0 = np.ascontiguousarray(rvec0, np.float64).reshape(3)
        t0 = np.ascontiguousarray(tvec0, np.float64).reshape(3)
        obs = [("img1_left", img1_left), ("img1_right", img1_right), ("img2_left", img2_left), ("img2_right", img2_right)]
        if any(o is None for _, o in obs[:3]):
            raise SvoError("refine_ba: only img2_right may be None")
        if isinstance(obj, np.ndarray):
            obj = np.ascontiguousarray(obj, np.float32).reshape(-1, 3)
            obs = [(k, None if o is None else np.ascontiguousarray(o, np.float32).reshape(-1, 2)) for k, o in obs]
            act = np.zeros(max(obj.shape[0], 1), np.uint8)
            X = np.zeros((max(obj.shape[0], 1), 3), np.float64)
        else:
            import torch
            for name, t, cols in [("obj", obj, 3)] + [(k, o, 2) for k, o in obs]:
                if t is None:
                    continue
                if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == cols and t.is_contiguous()
                        and t.device == obj.device and t.shape[0] == obj.shape[0]):
                    raise SvoError(f"refine_ba: {name} must be a contiguous float32 tensor of shape (n, {cols}) on the device of obj")
            act = torch.zeros(max(obj.shape[0], 1), dtype=torch.uint8, device=obj.device)
            X = torch.zeros((max(obj.shape[0], 1), 3), dtype=torch.float64, device=obj.device)
            self._order_in(X)
        n = obj.shape[0]
        if any(o is not None and o.shape[0] != n for _, o in obs):
            raise SvoError("refine_ba: obj and the observation lists must have the same number of points")
        res = RefineResult()
        po, mem = _ptr(obj)
        self._check(self.lib.svo_refine_ba(self.h, po, *[_ptr(o)[0] for _, o in obs], n, C.c_void_p(P1.ctypes.data),
                                           C.c_void_p(P2.ctypes.data), C.c_void_p(r0.ctypes.data), C.c_void_p(t0.ctypes.data),
                                           C.byref(res), _ptr(act)[0], _ptr(X)[0], mem))
        if mem == MEM_DEVICE:
            self._order_out(X)
            act, X = act.cpu().numpy(), X.cpu().numpy()
        out = self._refine_dict(res, np.asarray(act[:n]).copy())
        out["X"] = np.asarray(X[:n]).copy()
        return out

    def refine_points(self, pair=0, cap=None):
        """svo_get_refine_points: the (n, 3) float64 points that stand of pair `pair` of the most recent fused launch, which
        must have run in "ba" mode."""
        cap = int(self.cfg.max_keypoints) if cap is None else int(cap)
        X = np.zeros((max(cap, 1), 3), np.float64)
        n = C.c_int(0)
        self._check(self.lib.svo_get_refine_points(self.h, int(pair), C.c_void_p(X.ctypes.data), cap, C.byref(n)))
        return X[:n.value].copy()

    # ---- ORB path ---------------------------------------------------------------------------
    def orb_extract(self, img, cap=None):
        """ORBextractor::operator(): (keypoints, descriptors (n,32) uint8, per-level counts)."""
        cap = cap or self.cfg.max_keypoints
        p, pitch, mem = self._img(img)
        kps = np.zeros(cap, dtype=KP_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        per = np.zeros(8, np.int32)
        n = C.c_int(0)
        self._check(self.lib.svo_orb_extract(self.h, p, pitch, mem, C.c_void_p(kps.ctypes.data),
                                             C.c_void_p(desc.ctypes.data), cap, C.byref(n), C.c_void_p(per.ctypes.data)))
        return kps[:n.value].copy(), desc[:n.value].copy(), per

    def orb_read_level(self, level):
        w, h = C.c_int(0), C.c_int(0)
        self._check(self.lib.svo_orb_read_level(self.h, level, None, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), np.uint8)
        self._check(self.lib.svo_orb_read_level(self.h, level, C.c_void_p(out.ctypes.data), C.byref(w), C.byref(h)))
        return out

    def orb_read_candidates(self, level, cap=8192):
        out = np.zeros((cap, 4), np.float32)
        n = C.c_int(0)
        self._check(self.lib.svo_orb_read_candidates(self.h, level, C.c_void_p(out.ctypes.data), cap, C.byref(n)))
        return out[:min(n.value, cap), :3].copy()

    def match_hamming(self, query, train):
        if isinstance(query, np.ndarray):
            query = np.ascontiguousarray(query, np.uint8).reshape(-1, 32)
            train = np.ascontiguousarray(train, np.uint8).reshape(-1, 32)
            idx = np.zeros(max(len(query), 1), np.int32)
            dist = np.zeros(max(len(query), 1), np.float32)
        else:
            import torch
            idx = torch.zeros(max(len(query), 1), dtype=torch.int32, device=query.device)
            dist = torch.zeros(max(len(query), 1), dtype=torch.float32, device=query.device)
            self._order_in(dist)
        pq, mem = _ptr(query)
        self._check(self.lib.svo_match_hamming(self.h, pq, len(query), _ptr(train)[0], len(train), _ptr(idx)[0],
                                               _ptr(dist)[0], mem))
        if mem == MEM_DEVICE:
            self._order_out(dist)
        return idx[:len(query)], dist[:len(query)]

    # ---- guided ORB matcher (svo_set_orb_matcher / svo_orb_stereo_frame / svo_orb_track_frames) ----
    def set_orb_matcher(self, mode, th_stereo=75, th_track=100, ratio=0.9, radius=0.0, max_disparity=0.0):
        """ORB mode: the matcher of the frames ingested by later calls -- "brute" (the reference's, the default) or "guided":
        epipolar stereo search with a sub-pixel SAD slide, temporal ratio-test match with a sub-pixel step (radius 0: the whole
        image; max_disparity 0: P1[0])."""
        if isinstance(mode, str):
            if mode not in ("brute", "guided"):
                raise ValueError(f"matcher must be 'brute' or 'guided', not {mode!r}")
            mode = ORB_MATCHER_GUIDED if mode == "guided" else ORB_MATCHER_BRUTE
        self._check(self.lib.svo_set_orb_matcher(self.h, int(mode), int(th_stereo), int(th_track), float(ratio), float(radius),
                                                 float(max_disparity)))

    def get_orb_matcher(self):
        """("brute" | "guided", th_stereo, th_track, ratio, radius, max_disparity) as set."""
        m, a, b = C.c_int(0), C.c_int(0), C.c_int(0)
        r, rad, d = C.c_double(0), C.c_double(0), C.c_double(0)
        self._check(self.lib.svo_get_orb_matcher(self.h, C.byref(m), C.byref(a), C.byref(b), C.byref(r), C.byref(rad), C.byref(d)))
        return ("guided" if m.value == ORB_MATCHER_GUIDED else "brute"), a.value, b.value, r.value, rad.value, d.value

    def orb_stereo_frame(self, left, right, slot=0, cap=None):
        """svo_orb_stereo_frame: extraction of both images into stage slot 0 / 1 + stage S.  Returns (left keypoints, uR float32,
        sad int32); uR -1 / sad -1: no stereo match."""
        cap = cap or self.cfg.max_keypoints
        pl, pitch, mem = self._img(left)
        pr, pitch_r, mem_r = self._img(right)
        if pitch != pitch_r or mem != mem_r:
            raise SvoError("orb_stereo_frame: left and right must share the row pitch and the memory kind")
        kps = np.zeros(cap, dtype=KP_DTYPE)
        uR = np.zeros(cap, np.float32)
        sad = np.zeros(cap, np.int32)
        n = C.c_int(0)
        self._check(self.lib.svo_orb_stereo_frame(self.h, pl, pr, pitch, mem, int(slot), C.c_void_p(kps.ctypes.data),
                                                  C.c_void_p(uR.ctypes.data), C.c_void_p(sad.ctypes.data), cap, C.byref(n)))
        return kps[:n.value].copy(), uR[:n.value].copy(), sad[:n.value].copy()

    def orb_track_frames(self, slot_prev=0, slot_cur=1, cap=None):
        """svo_orb_track_frames: stage T between two stage slots.  Returns (t1_left, t1_right, t2_left (m, 2) float32,
        idx_prev, idx_cur int32)."""
        cap = cap or self.cfg.max_keypoints
        pts = [np.zeros((cap, 2), np.float32) for _ in range(3)]
        idx = [np.zeros(cap, np.int32) for _ in range(2)]
        n = C.c_int(0)
        self._check(self.lib.svo_orb_track_frames(self.h, int(slot_prev), int(slot_cur), *[C.c_void_p(a.ctypes.data) for a in pts + idx],
                                                  cap, C.byref(n)))
        return tuple(a[:n.value].copy() for a in pts + idx)

    def get_frame_stereo(self, cap=None):
        """svo_get_frame_stereo: (uR, sad) of the current frame of add_frame (its keypoints: get_frame_keypoints)."""
        cap = cap or self.cfg.max_keypoints
        uR = np.zeros(cap, np.float32)
        sad = np.zeros(cap, np.int32)
        n = C.c_int(0)
        self._check(self.lib.svo_get_frame_stereo(self.h, C.c_void_p(uR.ctypes.data), C.c_void_p(sad.ctypes.data), cap, C.byref(n)))
        return uR[:n.value].copy(), sad[:n.value].copy()

    # ---- FAST corner buckets (svo_set_fast_buckets / svo_bucket_corners) ---------------------------
    def set_fast_buckets(self, cell_w, cell_h, per_cell):
        """LK mode: keep the per_cell strongest FAST corners of every cell_w x cell_h pixel cell of the frames detected by
        later calls (per_cell = 0: off, the default).  fast_keep_strongest, if set, runs on the survivors."""
        self._check(self.lib.svo_set_fast_buckets(self.h, int(cell_w), int(cell_h), int(per_cell)))

    def fast_buckets(self):
        """(cell_w, cell_h, per_cell) as set; (0, 0, 0) while off."""
        cw, ch, k = C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(self.lib.svo_get_fast_buckets(self.h, C.byref(cw), C.byref(ch), C.byref(k)))
        return cw.value, ch.value, k.value

    def bucket_corners(self, kps, width, height, cell_w, cell_h, per_cell, cap=None):
        """svo_bucket_corners on a raster-ordered corner list: a numpy KP_DTYPE array (returns the kept records), or a cuda
        uint8 tensor of n * KP_DTYPE.itemsize bytes (returns (records tensor of the same size, int32 count tensor), both
        filled in stream order without a host synchronisation)."""
        if isinstance(kps, np.ndarray):
            kps = np.ascontiguousarray(kps, KP_DTYPE)
            n = int(kps.shape[0])
            cap = n if cap is None else int(cap)
            out = np.zeros(max(cap, 1), dtype=KP_DTYPE)
            m = C.c_int(0)
            self._check(self.lib.svo_bucket_corners(self.h, C.c_void_p(kps.ctypes.data), n, int(width), int(height), int(cell_w),
                                                    int(cell_h), int(per_cell), C.c_void_p(out.ctypes.data), cap,
                                                    C.cast(C.byref(m), C.c_void_p), MEM_HOST))
            return out[:m.value].copy()
        import torch
        assert kps.is_cuda and kps.is_contiguous() and kps.element_size() == 1 and kps.numel() % KP_DTYPE.itemsize == 0
        n = kps.numel() // KP_DTYPE.itemsize
        cap = n if cap is None else int(cap)
        out = torch.zeros(max(cap, 1) * KP_DTYPE.itemsize, dtype=torch.uint8, device=kps.device)
        m = torch.zeros(1, dtype=torch.int32, device=kps.device)
        ordered = self._order_in(out)
        self._check(self.lib.svo_bucket_corners(self.h, C.c_void_p(kps.data_ptr()), n, int(width), int(height), int(cell_w),
                                                int(cell_h), int(per_cell), C.c_void_p(out.data_ptr()), cap,
                                                C.c_void_p(m.data_ptr()), MEM_DEVICE))
        if ordered:
            self._order_out(out)
        return out, m

    # ---- track carry (svo_set_track_carry / svo_carry_merge and the id read-backs) -------------------
    def set_track_carry(self, on=True, min_distance=3.0, max_age=0):
        """LK mode, add_frame / streams_step and their ingest twins: keep the points the circular LK tracked into a frame,
        under persistent ids, as the head of the list the next pair tracks from; the frame's detections closer than
        min_distance to one of them are dropped.  max_age = 0: unlimited.  While on, the batch entry points refuse."""
        self._check(self.lib.svo_set_track_carry(self.h, 1 if on else 0, float(min_distance), int(max_age)))

    def track_carry(self):
        """(on, min_distance, max_age) as set; (False, 0.0, 0) while off."""
        on, md, ma = C.c_int(0), C.c_double(0), C.c_int(0)
        self._check(self.lib.svo_get_track_carry(self.h, C.byref(on), C.byref(md), C.byref(ma)))
        return bool(on.value), md.value, ma.value

    def carry_merge(self, width, height, min_distance, max_age, trk_xy, trk_resp, trk_id, trk_age, trk_keep, det_xy, det_resp,
                    next_id=0, cap=None):
        """svo_carry_merge.  numpy inputs: returns a dict of numpy arrays xy, resp, id, age, src (n_out entries) and the int
        n_carried.  torch cuda inputs: returns the same keys as `cap`-entry tensors plus n_out / n_carried as int32 tensors,
        all filled in stream order without a host synchronisation."""
        host = isinstance(trk_xy, np.ndarray)
        if host:
            conv = lambda a, dt, shape: np.ascontiguousarray(a, dt).reshape(shape)
            new = lambda shape, dt: np.zeros(shape, dt)
            f32, i64, i32, u8 = np.float32, np.int64, np.int32, np.uint8
            ptr = lambda a: C.c_void_p(a.ctypes.data)
        else:
            import torch
            dev = trk_xy.device
            conv = lambda a, dt, shape: a.to(dt).contiguous().reshape(shape)
            new = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
            f32, i64, i32, u8 = torch.float32, torch.int64, torch.int32, torch.uint8
            ptr = lambda a: C.c_void_p(a.data_ptr())
        txy, tr, ti, ta, tk = (conv(trk_xy, f32, (-1, 2)), conv(trk_resp, f32, (-1,)), conv(trk_id, i64, (-1,)),
                               conv(trk_age, i32, (-1,)), conv(trk_keep, u8, (-1,)))
        dxy, dr = conv(det_xy, f32, (-1, 2)), conv(det_resp, f32, (-1,))
        n_trk, n_det = int(txy.shape[0]), int(dxy.shape[0])
        assert tr.shape[0] == ti.shape[0] == ta.shape[0] == tk.shape[0] == n_trk and dr.shape[0] == n_det
        cap = n_trk + n_det if cap is None else int(cap)
        m = max(cap, 1)
        out = {"xy": new((m, 2), f32), "resp": new((m,), f32), "id": new((m,), i64), "age": new((m,), i32), "src": new((m,), i32)}
        if host:
            n_out, n_car = C.c_int(0), C.c_int(0)
            pn, pc = C.cast(C.byref(n_out), C.c_void_p), C.cast(C.byref(n_car), C.c_void_p)
        else:
            n_out, n_car = new((1,), i32), new((1,), i32)
            pn, pc = ptr(n_out), ptr(n_car)
            ordered = self._order_in(n_car)
        self._check(self.lib.svo_carry_merge(self.h, int(width), int(height), float(min_distance), int(max_age), ptr(txy), ptr(tr),
                                             ptr(ti), ptr(ta), ptr(tk), n_trk, ptr(dxy), ptr(dr), n_det, int(next_id),
                                             ptr(out["xy"]), ptr(out["resp"]), ptr(out["id"]), ptr(out["age"]), ptr(out["src"]), cap,
                                             pn, pc, MEM_HOST if host else MEM_DEVICE))
        if host:
            res = {k: v[:n_out.value].copy() for k, v in out.items()}
            res["n_carried"] = n_car.value
            return res
        if ordered:
            self._order_out(n_car)
        out["n_out"], out["n_carried"] = n_out, n_car
        return out

    # ---- sliding window: the landmark table over carried tracks (svo_window_update) -----------------
    def window_update(self, table, frames, t1_left, t1_right, t2_left, t2_right, ids, tri, pose_a, pose_b, cap=None):
        """svo_window_update: one tracked pair a -> b moves a landmark table on.  table: None (a cleared table) or a dict as
        this method returns it; frames: the window length W; the four track lists, ids (ascending) and tri (the float32
        triangulation in frame a) of the pair; pose_a / pose_b: the 4 x 4 chain pose before the step and the step's.  numpy
        inputs: returns dict(n, m, poses (8, 12), ids, X, seen, active, obs_left (m, 8, 2), obs_right), m rows each; raises
        SvoError when the result needs more than `cap` rows (default: rows in + tracks).  torch cuda inputs: the table carries
        `counts` (int32[4]: n, m, rows needed, 0) in place of n and m, every column has `cap` rows, and everything is
        filled in stream order without a host synchronisation."""
        host = isinstance(t1_left, np.ndarray)
        F = WINDOW_MAX_FRAMES
        if host:
            conv = lambda a, dt, shape: np.ascontiguousarray(a, dt).reshape(shape)
            new = lambda shape, dt: np.zeros(shape, dt)
            f32, f64, i64, i32, u32 = np.float32, np.float64, np.int64, np.int32, np.uint32
            ptr = lambda a: a.ctypes.data
        else:
            import torch
            dev = t1_left.device
            conv = lambda a, dt, shape: a.to(dt).contiguous().reshape(shape)
            new = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
            f32, f64, i64, i32, u32 = torch.float32, torch.float64, torch.int64, torch.int32, torch.int32   # masks travel as int32 bits
            ptr = lambda a: a.data_ptr()
        obs = [conv(a, f32, (-1, 2)) for a in (t1_left, t1_right, t2_left, t2_right)]
        tid, tx = conv(ids, i64, (-1,)), conv(tri, f32, (-1, 3))
        n_trk = int(tid.shape[0])
        assert all(int(o.shape[0]) == n_trk for o in obs) and int(tx.shape[0]) == n_trk
        pa, pb = conv(pose_a, f64, (16,)), conv(pose_b, f64, (16,))
        shapes = {"poses": ((F, 12), f64), "ids": ((-1,), i64), "X": ((-1, 3), f64), "seen": ((-1,), u32), "active": ((-1,), u32),
                  "obs_left": ((-1, F, 2), f32), "obs_right": ((-1, F, 2), f32)}
        if table is None:
            m_in = 0
            tin = {k: new(tuple(1 if d < 0 else d for d in sh), dt) for k, (sh, dt) in shapes.items()}
            tin["counts"] = new((4,), i32)
        else:
            tin = {k: conv(table[k], dt, sh) for k, (sh, dt) in shapes.items()}
            if host:
                m_in = int(table["m"])
                tin["counts"] = np.array([int(table["n"]), m_in, 0, 0], np.int32)
            else:
                m_in = int(tin["ids"].shape[0])
                tin["counts"] = conv(table["counts"], i32, (4,))
        cap = m_in + n_trk if cap is None else int(cap)
        rows = max(cap, 1)
        if int(tin["ids"].shape[0]) < rows:                       # both tables have `cap` rows of room
            grown = {k: new((rows,) + tuple(tin[k].shape[1:]), dt) for k, (sh, dt) in shapes.items() if k != "poses"}
            for k, g in grown.items():
                g[:tin[k].shape[0]] = tin[k]
            tin.update(grown)
        out = {k: new((F, 12) if k == "poses" else (rows,) + tuple(tin[k].shape[1:]), dt) for k, (sh, dt) in shapes.items()}
        out["counts"] = new((4,), i32)
        ti, to = (WindowTable(*[ptr(t[k]) for k in _WINDOW_COLS]) for t in (tin, out))
        if not host:
            ordered = self._order_in(out["counts"])
        rc = self.lib.svo_window_update(self.h, int(frames), C.byref(ti), C.byref(to), cap, *[ptr(o) for o in obs], ptr(tid), ptr(tx),
                                        n_trk, ptr(pa), ptr(pb), MEM_HOST if host else MEM_DEVICE)
        self._check(rc)
        if not host:
            if ordered:
                self._order_out(out["counts"])
            return out
        m = int(out["counts"][1])
        res = {k: (v if k == "poses" else v[:m].copy()) for k, v in out.items() if k != "counts"}
        res["n"], res["m"] = int(out["counts"][0]), m
        return res

    def set_window_ba(self, frames=5, rounds=4, iters=5, sigma_px=1.0, min_obs=10):
        """LK mode, add_frame / ingest_add_frame with track carry on: keep a landmark table over the last `frames` frames of the
        chain and adjust its poses and points together after every step (svo_set_window_ba); frames = 0 switches it off."""
        self._check(self.lib.svo_set_window_ba(self.h, int(frames), int(rounds), int(iters), float(sigma_px), int(min_obs)))

    def window_ba(self):
        """(frames, rounds, iters, sigma_px, min_obs) as set; all 0 while off."""
        f, r, i, s, m = C.c_int(0), C.c_int(0), C.c_int(0), C.c_double(0), C.c_int(0)
        self._check(self.lib.svo_get_window_ba(self.h, C.byref(f), C.byref(r), C.byref(i), C.byref(s), C.byref(m)))
        return f.value, r.value, i.value, s.value, m.value

    def window(self):
        """The online chain's landmark table after the last add_frame step: a dict as window_update returns it (numpy)."""
        F = WINDOW_MAX_FRAMES
        counts = np.zeros(4, np.int32)
        self._check(self.lib.svo_get_window(self.h, C.byref(WindowTable(counts.ctypes.data, *([None] * 7))), 0))
        m, rows = int(counts[1]), max(int(counts[1]), 1)
        t = {"counts": counts, "poses": np.zeros((F, 12)), "ids": np.zeros(rows, np.int64), "X": np.zeros((rows, 3)),
             "seen": np.zeros(rows, np.uint32), "active": np.zeros(rows, np.uint32), "obs_left": np.zeros((rows, F, 2), np.float32),
             "obs_right": np.zeros((rows, F, 2), np.float32)}
        self._check(self.lib.svo_get_window(self.h, C.byref(WindowTable(*[t[k].ctypes.data for k in _WINDOW_COLS])), rows))
        res = {k: (v if k == "poses" else v[:m].copy()) for k, v in t.items() if k != "counts"}
        res["n"], res["m"] = int(counts[0]), m
        return res

    def window_result(self):
        """The last add_frame step's optimiser outcome (svo_get_window_result) as a dict."""
        res = WindowResult()
        self._check(self.lib.svo_get_window_result(self.h, C.addressof(res)))
        return res.as_dict()

    def window_solve(self, table, P1, P2, rounds=4, iters=5, sigma_px=1.0, min_obs=10):
        """svo_window_ba: the sliding-window bundle adjustment on a landmark table (a dict as window_update returns it).  numpy:
        returns (result dict -- status, counts, frame_active (8), cost_first / cost_last, info (42, 42) -- and the table as it
        stands afterwards: poses, X and active replaced when status is REFINE_APPLIED, the input otherwise; the input dict is not
        modified).  torch cuda: the table's poses / X / active tensors are overwritten IN PLACE in stream order and the result
        comes back as a uint8 tensor holding a WindowResult (WindowResult.from_buffer_copy after a synchronisation)."""
        host = isinstance(table["X"], np.ndarray)
        F = WINDOW_MAX_FRAMES
        P1c, P2c = np.ascontiguousarray(P1, np.float64).reshape(12), np.ascontiguousarray(P2, np.float64).reshape(12)
        if host:
            m = int(table["m"])
            t = {"counts": np.array([int(table["n"]), m, 0, 0], np.int32), "poses": np.array(table["poses"], np.float64).reshape(F, 12),
                 "ids": np.ascontiguousarray(table["ids"][:m], np.int64), "X": np.array(table["X"][:m], np.float64).reshape(-1, 3),
                 "seen": np.ascontiguousarray(table["seen"][:m], np.uint32), "active": np.array(table["active"][:m], np.uint32),
                 "obs_left": np.ascontiguousarray(table["obs_left"][:m], np.float32).reshape(-1, F, 2),
                 "obs_right": np.ascontiguousarray(table["obs_right"][:m], np.float32).reshape(-1, F, 2)}
            if m == 0:
                t.update({k: np.zeros((1,) + t[k].shape[1:], t[k].dtype) for k in _WINDOW_COLS[2:]})
            tt = WindowTable(*[t[k].ctypes.data for k in _WINDOW_COLS])
            res = WindowResult()
            self._check(self.lib.svo_window_ba(self.h, C.byref(tt), max(m, 1), P1c.ctypes.data, P2c.ctypes.data, int(rounds), int(iters),
                                               float(sigma_px), int(min_obs), C.addressof(res), MEM_HOST))
            out = dict(table, poses=t["poses"], X=t["X"][:m], active=t["active"][:m])
            return res.as_dict(), out
        import torch
        for k in _WINDOW_COLS:
            assert table[k].is_cuda and table[k].is_contiguous(), k
        res = torch.zeros(C.sizeof(WindowResult), dtype=torch.uint8, device=table["X"].device)
        ordered = self._order_in(res)
        tt = WindowTable(*[table[k].data_ptr() for k in _WINDOW_COLS])
        self._check(self.lib.svo_window_ba(self.h, C.byref(tt), int(table["ids"].shape[0]), P1c.ctypes.data, P2c.ctypes.data, int(rounds),
                                           int(iters), float(sigma_px), int(min_obs), res.data_ptr(), MEM_DEVICE))
        if ordered:
            self._order_out(res)
        return res, table

    # ---- keyframe-relative pose on the online chain (svo_set_keyframe / svo_keyframe_join and the read-backs) ----------
    def set_keyframe(self, on=True, min_tracks=60, max_gap=0):
        """LK mode, add_frame / ingest_add_frame with track carry on: localise every frame by solvePnPRansac against the
        points triangulated at a keyframe several frames back as well, and report that pose where it passes the pair's own
        gates (svo_set_keyframe).  min_tracks: joined tracks a solve needs; max_gap: frames a keyframe serves at most (0: no
        limit).  While on, set_window_ba(on), set_track_carry(False) and streams_step refuse."""
        if on and (int(min_tracks) < 4 or int(max_gap) < 0 or int(max_gap) == 1):
            raise ValueError("min_tracks must be >= 4 and max_gap 0 (no limit) or >= 2")
        self._check(self.lib.svo_set_keyframe(self.h, 1 if on else 0, int(min_tracks), int(max_gap)))

    def keyframe(self):
        """(on, min_tracks, max_gap) as set; (False, 0, 0) while off."""
        on, mt, mg = C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(self.lib.svo_get_keyframe(self.h, C.byref(on), C.byref(mt), C.byref(mg)))
        return bool(on.value), mt.value, mg.value

    def keyframe_result(self):
        """The last add_frame step's svo_keyframe_result as a dict (poses 4 x 4)."""
        res = KeyframeResult()
        self._check(self.lib.svo_get_keyframe_result(self.h, C.byref(res)))
        return res.as_dict()

    def keyframe_matches(self):
        """The last step's joined lists: dict(ids, X (n, 3), xy (n, 2), trk (the track's index in last_tracks()), mask (the
        keyframe solve's inliers; zeros when nothing was solved))."""
        n = C.c_int(0)
        self._check(self.lib.svo_get_keyframe_matches(self.h, None, None, None, None, None, 0, C.byref(n)))
        m = max(n.value, 1)
        out = {"ids": np.zeros(m, np.int64), "X": np.zeros((m, 3), np.float32), "xy": np.zeros((m, 2), np.float32),
               "trk": np.zeros(m, np.int32), "mask": np.zeros(m, np.uint8)}
        self._check(self.lib.svo_get_keyframe_matches(self.h, *[C.c_void_p(out[k].ctypes.data) for k in ("ids", "X", "xy", "trk", "mask")],
                                                      m, C.byref(n)))
        return {k: v[:n.value].copy() for k, v in out.items()}

    def keyframe_table(self):
        """The chain's keyframe table after the last step: (ids, X (n, 3) float32 in the keyframe's camera frame)."""
        n = C.c_int(0)
        self._check(self.lib.svo_get_keyframe_table(self.h, None, None, 0, C.byref(n)))
        m = max(n.value, 1)
        ids, X = np.zeros(m, np.int64), np.zeros((m, 3), np.float32)
        self._check(self.lib.svo_get_keyframe_table(self.h, C.c_void_p(ids.ctypes.data), C.c_void_p(X.ctypes.data), m, C.byref(n)))
        return ids[:n.value].copy(), X[:n.value].copy()

    def keyframe_join(self, tab_ids, tab_X, trk_ids, trk_xy, cap=None):
        """svo_keyframe_join: the tracks whose id has a row in the table, in track order.  numpy inputs: returns a dict of
        numpy arrays X (n, 3), xy (n, 2), trk, row (n entries).  torch cuda inputs: the same keys as `cap`-entry tensors plus
        n_out as an int32 tensor, all filled in stream order without a host synchronisation."""
        host = isinstance(tab_ids, np.ndarray)
        if host:
            conv = lambda a, dt, shape: np.ascontiguousarray(a, dt).reshape(shape)
            new = lambda shape, dt: np.zeros(shape, dt)
            f32, i64, i32 = np.float32, np.int64, np.int32
            ptr = lambda a: C.c_void_p(a.ctypes.data)
        else:
            import torch
            dev = tab_ids.device
            conv = lambda a, dt, shape: a.to(dt).contiguous().reshape(shape)
            new = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
            f32, i64, i32 = torch.float32, torch.int64, torch.int32
            ptr = lambda a: C.c_void_p(a.data_ptr())
        ti, tx, ki, kx = conv(tab_ids, i64, (-1,)), conv(tab_X, f32, (-1, 3)), conv(trk_ids, i64, (-1,)), conv(trk_xy, f32, (-1, 2))
        n_rows, n_trk = int(ti.shape[0]), int(ki.shape[0])
        if int(tx.shape[0]) != n_rows or int(kx.shape[0]) != n_trk:
            raise ValueError("tab_X / trk_xy must have one row per id")
        cap = min(n_rows, n_trk) if cap is None else int(cap)
        m = max(cap, 1)
        out = {"X": new((m, 3), f32), "xy": new((m, 2), f32), "trk": new((m,), i32), "row": new((m,), i32)}
        if host:
            n_out = C.c_int(0)
            pn = C.cast(C.byref(n_out), C.c_void_p)
        else:
            n_out = new((1,), i32)
            pn = ptr(n_out)
            ordered = self._order_in(n_out)
        self._check(self.lib.svo_keyframe_join(self.h, ptr(ti), ptr(tx), n_rows, ptr(ki), ptr(kx), n_trk, ptr(out["X"]), ptr(out["xy"]),
                                               ptr(out["trk"]), ptr(out["row"]), cap, pn, MEM_HOST if host else MEM_DEVICE))
        if host:
            return {k: v[:n_out.value].copy() for k, v in out.items()}
        if ordered:
            self._order_out(n_out)
        out["n_out"] = n_out
        return out

    def _ids(self, fn, *head, cap=65536):
        ids, ages, n = np.zeros(cap, np.int64), np.zeros(cap, np.int32), C.c_int(0)
        self._check(fn(self.h, *head, C.c_void_p(ids.ctypes.data), C.c_void_p(ages.ctypes.data), cap, C.byref(n)))
        return ids[:n.value].copy(), ages[:n.value].copy()

    def frame_track_ids(self, cap=65536):
        """(ids, ages) of the list frame_keypoints() returns (track carry on)."""
        return self._ids(self.lib.svo_get_frame_track_ids, cap=cap)

    def last_track_ids(self, cap=65536):
        """(ids, ages at t1) of the tracks last_tracks() returns, in their order (track carry on)."""
        return self._ids(self.lib.svo_get_last_track_ids, cap=cap)

    def streams_track_ids(self, item, cap=65536):
        """(ids, ages at t1) of the tracks streams_tracks(item) returns, in their order (track carry on)."""
        return self._ids(self.lib.svo_streams_get_track_ids, int(item), cap=cap)

    def streams_frame_tracks(self, stream_id, cap=65536):
        """(keypoint records, ids, ages) of the list stream `stream_id` keeps for its next pair (track carry on)."""
        kps = np.zeros(cap, dtype=KP_DTYPE)
        ids, ages = self._ids(self.lib.svo_streams_get_frame_tracks, int(stream_id), C.c_void_p(kps.ctypes.data), cap=cap)
        return kps[:len(ids)].copy(), ids, ages

    # ---- Shi-Tomasi corners (svo_set_lk_detector / svo_min_eigen_map / svo_gftt_detect) ------------
    def set_lk_detector(self, detector, max_corners=500, quality_level=0.01, min_distance=20.0):
        """LK mode: the detector of the frames detected by later calls -- "fast" (the default; the other arguments are
        ignored) or "gftt", cv::goodFeaturesToTrack(img, max_corners, quality_level, min_distance)."""
        if isinstance(detector, str):
            if detector not in ("fast", "gftt"):
                raise ValueError(f"detector must be 'fast' or 'gftt', not {detector!r}")
            detector = DETECTOR_GFTT if detector == "gftt" else DETECTOR_FAST
        self._check(self.lib.svo_set_lk_detector(self.h, int(detector), int(max_corners), float(quality_level), float(min_distance)))

    def lk_detector(self):
        """("fast" | "gftt", max_corners, quality_level, min_distance) as set; ("fast", 0, 0.0, 0.0) while FAST."""
        d, n, q, m = C.c_int(0), C.c_int(0), C.c_double(0), C.c_double(0)
        self._check(self.lib.svo_get_lk_detector(self.h, C.byref(d), C.byref(n), C.byref(q), C.byref(m)))
        return ("gftt" if d.value == DETECTOR_GFTT else "fast"), n.value, q.value, m.value

    def _img_any(self, img):
        """(pointer, width, height, row pitch, memory kind, is numpy) of a u8 image of any size; rows may be padded."""
        h, w = (int(v) for v in img.shape)
        p, pitch, mem = self._img(img, (h, w))
        return p, w, h, pitch, mem, isinstance(img, np.ndarray)

    def min_eigen_map(self, img):
        """svo_min_eigen_map: the minimal-eigenvalue map (float32, h x w) of a u8 image of any size -- numpy in, numpy out;
        cuda tensor in, cuda tensor out (stream order, no host synchronisation)."""
        p, w, h, pitch, mem, is_np = self._img_any(img)
        if mem == MEM_HOST:
            out = np.zeros((h, w), np.float32)
            self._check(self.lib.svo_min_eigen_map(self.h, p, w, h, pitch, MEM_HOST, C.c_void_p(out.ctypes.data), w))
            if is_np:
                return out
            import torch
            return torch.from_numpy(out)
        import torch
        out = torch.zeros((h, w), dtype=torch.float32, device=img.device)
        ordered = self._order_in(out)
        self._check(self.lib.svo_min_eigen_map(self.h, p, w, h, pitch, MEM_DEVICE, C.c_void_p(out.data_ptr()), w))
        if ordered:
            self._order_out(out)
        return out

    def gftt_detect(self, img, max_corners=500, quality_level=0.01, min_distance=20.0, cap=None):
        """svo_gftt_detect on a u8 image of any size.  numpy (host) image: returns (KP_DTYPE records in selection order,
        float32 strengths).  cuda tensor: returns (uint8 tensor of cap * KP_DTYPE.itemsize bytes, float32 tensor of cap
        strengths, int32 count tensor), filled in stream order without a host synchronisation; a count above cap means
        more candidates than cap and no list."""
        p, w, h, pitch, mem, is_np = self._img_any(img)
        cap = int(self.cfg.max_keypoints if cap is None else cap)
        if mem == MEM_HOST:
            out = np.zeros(max(cap, 1), dtype=KP_DTYPE)
            strength = np.zeros(max(cap, 1), np.float32)
            n = C.c_int(0)
            self._check(self.lib.svo_gftt_detect(self.h, p, w, h, pitch, MEM_HOST, int(max_corners), float(quality_level),
                                                 float(min_distance), C.c_void_p(out.ctypes.data), C.c_void_p(strength.ctypes.data),
                                                 cap, C.cast(C.byref(n), C.c_void_p)))
            return out[:n.value].copy(), strength[:n.value].copy()
        import torch
        out = torch.zeros(max(cap, 1) * KP_DTYPE.itemsize, dtype=torch.uint8, device=img.device)
        strength = torch.zeros(max(cap, 1), dtype=torch.float32, device=img.device)
        n = torch.zeros(1, dtype=torch.int32, device=img.device)
        ordered = self._order_in(out)
        self._check(self.lib.svo_gftt_detect(self.h, p, w, h, pitch, MEM_DEVICE, int(max_corners), float(quality_level),
                                             float(min_distance), C.c_void_p(out.data_ptr()), C.c_void_p(strength.data_ptr()),
                                             cap, C.c_void_p(n.data_ptr())))
        if ordered:
            self._order_out(out)
        return out, strength, n

    # ---- cv::resize and the ingest stage (svo_resize / svo_ingest_*) -------------------------------
    def resize(self, src, dw, dh, interp="nearest", fx=0, fy=0, out=None):
        """cv::resize of one (h, w) image or a stack (n, h, w) of them, numpy (host) or torch cuda, rows may be padded:
        factor form (fx, fy > 0; dw x dh must be cvRound(size * f)) or size form (fx = fy = 0).  Returns an array of the
        same kind, or fills `out` (same kind; rows may be padded, the padding is not written)."""
        single = src.ndim == 2
        s3 = src[None] if single else src
        n, sh, sw = (int(v) for v in s3.shape)
        is_np = isinstance(s3, np.ndarray)
        if out is None:
            if is_np:
                o3 = np.zeros((n, int(dh), int(dw)), np.uint8)
            else:
                import torch
                o3 = torch.zeros((n, int(dh), int(dw)), dtype=torch.uint8, device=s3.device)
        else:
            o3 = out[None] if single else out
            assert isinstance(o3, np.ndarray) == is_np and tuple(o3.shape) == (n, int(dh), int(dw))
        if is_np:
            assert s3.dtype == np.uint8 and o3.dtype == np.uint8 and s3.strides[2] == 1 and o3.strides[2] == 1
            ps, pd, mem = C.c_void_p(s3.ctypes.data), C.c_void_p(o3.ctypes.data), MEM_HOST
            sp, ss, dp, ds = s3.strides[1], s3.strides[0], o3.strides[1], o3.strides[0]
        else:
            assert s3.element_size() == 1 and o3.element_size() == 1 and s3.stride(2) == 1 and o3.stride(2) == 1
            assert s3.is_cuda == o3.is_cuda
            ps, pd = C.c_void_p(s3.data_ptr()), C.c_void_p(o3.data_ptr())
            mem = MEM_DEVICE if s3.is_cuda else MEM_HOST
            sp, ss, dp, ds = s3.stride(1), s3.stride(0), o3.stride(1), o3.stride(0)
        ordered = self._order_in(s3) if mem == MEM_DEVICE else False
        self._check(self.lib.svo_resize(self.h, ps, sw, sh, int(sp), int(ss), pd, int(dw), int(dh), int(dp), int(ds), n,
                                        _interp(interp), float(fx), float(fy), mem))
        if ordered:
            self._order_out(o3)
        res = o3 if out is None else out
        return res[0] if (single and out is None) else res

    def ingest_create(self, src_width, src_height, interp="nearest", fx=0, fy=0):
        """The ingest stage: frames of src_width x src_height are resized on the device to the context's size (factor form,
        or fx = fy = 0 for the size form).  Once per context."""
        self._check(self.lib.svo_ingest_create(self.h, int(src_width), int(src_height), _interp(interp), float(fx), float(fy)))
        self.src_width, self.src_height = int(src_width), int(src_height)

    def ingest_info(self):
        """(src_width, src_height, interp, inv_x, inv_y) of the ingest stage; inv_x / inv_y go to scale_projection."""
        sw, sh, it = C.c_int(0), C.c_int(0), C.c_int(0)
        ix, iy = C.c_double(0), C.c_double(0)
        self._check(self.lib.svo_ingest_info(self.h, C.byref(sw), C.byref(sh), C.byref(it), C.byref(ix), C.byref(iy)))
        return sw.value, sh.value, it.value, ix.value, iy.value

    def _src_shape(self):
        """The frame shape the ingest calls assert against (before ingest_create: the library answers SVO_ERR_STATE)."""
        return (getattr(self, "src_height", self.height), getattr(self, "src_width", self.width))

    def ingest_add_frame(self, left, right):
        """add_frame on source-size frames (svo_ingest_add_frame)."""
        return self._add_frame(self.lib.svo_ingest_add_frame, self._src_shape(), left, right)

    def ingest_track_batch(self, left_frames, right_frames, pose0=None, results=None):
        """track_batch on source-size frames: torch cuda uint8 tensors (F, src_height, src_width), rows may be padded; they are
        read by the resize kernel on the context's stream."""
        return self._track_batch(self.lib.svo_ingest_track_batch, self._src_shape(), left_frames, right_frames, pose0, results)

    def ingest_streams_step(self, ids, lefts, rights, results=None):
        """streams_step on source-size frames (svo_ingest_streams_step)."""
        return self._streams_step(self.lib.svo_ingest_streams_step, self._src_shape(), ids, lefts, rights, results)

    def ingest_upload_frames(self, buf, left, right, first_slot=0):
        """upload_frames on source-size host frames (F, src_height, pitch): copied and resized into device frame buffer
        `buf` on the copy stream (svo_ingest_upload_frames_at); wait_upload / track_uploaded(_async) follow as usual."""
        self._upload_frames(self.lib.svo_ingest_upload_frames_at, self._src_shape(), buf, left, right, first_slot)

    # ---- fused API --------------------------------------------------------------------------
    def add_frame(self, left, right):
        return self._add_frame(self.lib.svo_add_frame, (self.height, self.width), left, right)

    def _add_frame(self, fn, shape, left, right):
        """svo_add_frame / svo_ingest_add_frame on one frame pair of `shape`."""
        pl, pitch, mem = self._img(left, shape)
        pr, pitch_r, mem_r = self._img(right, shape)
        assert pitch == pitch_r and mem == mem_r
        res = StepResult()
        if mem == MEM_DEVICE:
            # ORB mode reads level 0 IN PLACE until the end of the front end, and the frames may still be being written on
            # torch's stream: order them before the library's kernels.  The call returns with the record on the host,
            # i.e. after everything that reads the frames, so nothing is left to order afterwards.
            self._order_in(left)
        rc = self._check(fn(self.h, pl, pr, pitch, mem, C.byref(res)), allow_soft=True)
        return rc, np.frombuffer(bytes(res), dtype=STEP_DTYPE)[0].copy()

    def reset(self):
        self._check(self.lib.svo_reset(self.h))

    def get_pose(self):
        pose = np.zeros(16)
        self._check(self.lib.svo_get_pose(self.h, C.c_void_p(pose.ctypes.data)))
        return pose.reshape(4, 4)

    def track_batch(self, left_frames, right_frames, pose0=None, results=None):
        """left/right_frames: torch cuda uint8 tensors (F, h, pitch>=w) viewed as (F, h, w).
        Returns a numpy structured array of F-1 step results (or fills the given cuda tensor)."""
        return self._track_batch(self.lib.svo_track_batch, None, left_frames, right_frames, pose0, results)

    def _track_batch(self, fn, shape, left_frames, right_frames, pose0, results):
        """svo_track_batch / svo_ingest_track_batch on F frames per eye (of `shape`, where one is given)."""
        F = left_frames.shape[0]
        assert left_frames.is_cuda and right_frames.is_cuda
        assert shape is None or (tuple(left_frames.shape[1:]) == tuple(shape) and left_frames.shape == right_frames.shape)
        assert left_frames.stride(2) == 1 and left_frames.stride() == right_frames.stride()
        pitch, fstride = left_frames.stride(1), left_frames.stride(0)
        out, rp, rmem = _records(F - 1, results)
        # The frames (read in place until the end of the front end in ORB mode) and a device result buffer (its zero fill) may
        # still be in flight on torch's current stream, and with device results the call returns while the kernels run:
        # torch's stream is ordered before the launch, and the kernels that READ THE FRAMES before whatever torch's stream
        # does next (freeing or overwriting them) -- svo_signal_stream_inputs, not svo_signal_stream: making torch's stream
        # wait for the side-stream pose stage after every batch would chain batch k + 1's front end behind batch k's pose
        # stage through that stream and end their overlap.  The RECORDS of a device result buffer are complete after
        # signal_stream(consumer) / sync(), as before.  Two event operations each, no host synchronisation; skipped when
        # the context runs ON torch's current stream (set_stream).
        ordered = self._order_in(left_frames)
        self._check(fn(self.h, C.c_void_p(left_frames.data_ptr()), C.c_void_p(right_frames.data_ptr()), int(pitch), int(fstride),
                       int(F), _pose_ptr(pose0), rp, rmem))
        if results is not None and ordered:
            import torch
            self.signal_stream_inputs(torch.cuda.current_stream(left_frames.device).cuda_stream)
        return out

    # ---- host-resident frame batches (svo_upload_frames / svo_track_uploaded) -----------------
    def host_frames(self, n_frames, pitch=None, source_size=False):
        """(n_frames, height, pitch) uint8 numpy view over page-locked host memory (svo_host_alloc);
        release it with host_free(view).  source_size: frames of the ingest stage's source size (ingest_upload_frames)."""
        height, width = self._src_shape() if source_size else (self.height, self.width)
        pitch = pitch or width
        nbytes = int(n_frames) * height * int(pitch)
        p = C.c_void_p()
        self._check(self.lib.svo_host_alloc(self.h, nbytes, C.byref(p)))
        buf = (C.c_uint8 * nbytes).from_address(p.value)
        view = np.frombuffer(buf, dtype=np.uint8).reshape(int(n_frames), height, int(pitch))
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[view.ctypes.data] = p
        return view

    def host_free(self, view):
        p = self._pinned.pop(view.ctypes.data)
        self._check(self.lib.svo_host_free(self.h, p))

    def upload_frames(self, buf, left, right, first_slot=0):
        """left/right: (F, height, pitch) uint8 host arrays (ideally from host_frames); asynchronous.  first_slot: the frame
        slot of the device buffer the first of them goes to (svo_upload_frames_at: a stream whose halo frame is carried on
        the device uploads its new frames into slots 1..)."""
        self._upload_frames(self.lib.svo_upload_frames_at, None, buf, left, right, first_slot)

    def _upload_frames(self, fn, shape, buf, left, right, first_slot):
        """svo_upload_frames_at / svo_ingest_upload_frames_at on F host frames per eye (of `shape`, where one is given)."""
        assert left.shape == right.shape and left.strides == right.strides and left.strides[2] == 1
        assert shape is None or tuple(left.shape[1:]) == tuple(shape), (tuple(left.shape), shape)
        self._check(fn(self.h, int(buf), int(first_slot), C.c_void_p(left.ctypes.data), C.c_void_p(right.ctypes.data),
                       int(left.strides[1]), int(left.strides[0]), int(left.shape[0])))

    def wait_upload(self, buf):
        self._check(self.lib.svo_wait_upload(self.h, int(buf)))

    def track_uploaded(self, buf, n_frames, pose0=None):
        out = np.zeros(int(n_frames) - 1, dtype=STEP_DTYPE)
        self._check(self.lib.svo_track_uploaded(self.h, int(buf), int(n_frames), _pose_ptr(pose0), C.c_void_p(out.ctypes.data), MEM_HOST))
        return out

    def track_uploaded_async(self, buf, n_frames, pose0=None, continue_chain=False, carry_frame=False):
        """svo_track_uploaded without waiting for the GPU; the records are fetched by collect_results()
        (up to two batches outstanding, collected in launch order).  carry_frame (with continue_chain): frame 0 of this
        batch is the previous batch's last frame -- its features are carried over on the device, not computed again."""
        flags = (1 if continue_chain else 0) | (2 if continue_chain and carry_frame else 0)
        self._check(self.lib.svo_track_uploaded_async(self.h, int(buf), int(n_frames), _pose_ptr(pose0), flags))

    def collect_results(self, n_pairs):
        out = np.zeros(int(n_pairs), dtype=STEP_DTYPE)
        self._check(self.lib.svo_collect_results(self.h, C.c_void_p(out.ctypes.data), int(n_pairs)))
        return out

    def results_ready(self):
        """Pairs of the oldest outstanding async batch when its records are complete, else 0 (svo_results_ready)."""
        n = C.c_int(0)
        self._check(self.lib.svo_results_ready(self.h, C.byref(n)))
        return n.value

    def set_pose(self, pose):
        pose = np.ascontiguousarray(pose, np.float64).reshape(16)
        self._check(self.lib.svo_set_pose(self.h, C.c_void_p(pose.ctypes.data)))

    def chain_relative(self, T_rel_inv, ok, pose0=None):
        """poses[p] = pose0 * prod_{q<=p, ok[q]} T[q] (svo_chain_relative).  numpy arrays or torch cuda
        tensors: T (n, 16) float64, ok (n,) int32.  Returns (n, 16) of the same kind."""
        if isinstance(T_rel_inv, np.ndarray):
            T = np.ascontiguousarray(T_rel_inv, np.float64).reshape(-1, 16)
            okc = np.ascontiguousarray(ok, np.int32)
            out = np.zeros_like(T)
            tp, op_, up, mem = C.c_void_p(T.ctypes.data), C.c_void_p(okc.ctypes.data), C.c_void_p(out.ctypes.data), MEM_HOST
        else:
            import torch
            T = T_rel_inv.reshape(-1, 16).contiguous()
            okc = ok.to(torch.int32).contiguous()
            assert T.is_cuda and okc.is_cuda and T.dtype == torch.float64
            out = torch.zeros_like(T)
            self._order_in(out)
            tp, op_, up, mem = C.c_void_p(T.data_ptr()), C.c_void_p(okc.data_ptr()), C.c_void_p(out.data_ptr()), MEM_DEVICE
        self._check(self.lib.svo_chain_relative(self.h, tp, op_, int(T.shape[0]), _pose_ptr(pose0), up, mem))
        if mem == MEM_DEVICE:
            self._order_out(out)        # device tensors: complete in stream order, for torch's current stream too
        return out

    def frame_keypoints(self, side=0, with_descriptors=False, cap=65536):
        """Keypoints detected on the frame last given to add_frame (svo_get_frame_keypoints)."""
        kps = np.zeros(cap, dtype=KP_DTYPE)
        desc = np.zeros((cap, 32), np.uint8) if with_descriptors else None
        n = C.c_int(0)
        self._check(self.lib.svo_get_frame_keypoints(self.h, int(side), C.c_void_p(kps.ctypes.data),
                                                     C.c_void_p(desc.ctypes.data) if with_descriptors else None, cap, C.byref(n)))
        return (kps[:n.value].copy(), desc[:n.value].copy()) if with_descriptors else kps[:n.value].copy()

    def batch_tracks(self, pair, cap=65536):
        """(t1_left, t1_right, t2_right, t2_left, inlier) of pair `pair` of the last track_batch launch."""
        pts = [np.zeros((cap, 2), np.float32) for _ in range(4)]
        inl = np.zeros(cap, np.uint8)
        n = C.c_int(0)
        self._check(self.lib.svo_get_batch_tracks(self.h, int(pair), *[C.c_void_p(p.ctypes.data) for p in pts],
                                                  C.c_void_p(inl.ctypes.data), cap, C.byref(n)))
        return [p[:n.value].copy() for p in pts] + [inl[:n.value].copy()]

    def last_tracks(self, cap=65536):
        """(t1_left, t1_right, t2_right, t2_left, inlier) of the pair last tracked by add_frame."""
        pts = [np.zeros((cap, 2), np.float32) for _ in range(4)]
        inl = np.zeros(cap, np.uint8)
        n = C.c_int(0)
        self._check(self.lib.svo_get_last_tracks(self.h, *[C.c_void_p(p.ctypes.data) for p in pts], C.c_void_p(inl.ctypes.data),
                                                 cap, C.byref(n)))
        return [p[:n.value].copy() for p in pts] + [inl[:n.value].copy()]

    # ---- stream sets: many independent live streams through one launch set (svo_streams_*) ------
    def streams_create(self, n_streams):
        self._check(self.lib.svo_streams_create(self.h, int(n_streams)))

    def streams_count(self):
        n = C.c_int(0)
        self._check(self.lib.svo_streams_count(self.h, C.byref(n)))
        return n.value

    def _frame_stack(self, frames, shape):
        """(array, pointer, pitch, frame stride, memory kind) of m equal-size u8 frames of `shape`: a stacked (m, h, w) numpy array or
        torch tensor (rows may be padded), or a list of (h, w) images, which is stacked."""
        if isinstance(frames, (list, tuple)):
            if isinstance(frames[0], np.ndarray):
                frames = np.stack([np.ascontiguousarray(f, np.uint8) for f in frames])
            else:
                import torch
                frames = torch.stack(list(frames))
        assert tuple(frames.shape[1:]) == tuple(shape), (tuple(frames.shape), shape)
        if isinstance(frames, np.ndarray):
            assert frames.dtype == np.uint8 and frames.strides[2] == 1
            return frames, C.c_void_p(frames.ctypes.data), int(frames.strides[1]), int(frames.strides[0]), MEM_HOST
        assert frames.element_size() == 1 and frames.stride(2) == 1
        return (frames, C.c_void_p(frames.data_ptr()), int(frames.stride(1)), int(frames.stride(0)),
                MEM_DEVICE if frames.is_cuda else MEM_HOST)

    def streams_step(self, ids, lefts, rights, results=None):
        """Advances the streams `ids` (distinct, any order, any subset) by one stereo frame each: lefts[i] / rights[i] is the
        next frame of stream ids[i].  Frames: numpy (host) or torch cuda, stacked (m, h, w) or a list of (h, w) images.
        Returns the m step records in the caller's order as a numpy structured array, or -- results = a cuda uint8 / record
        tensor of m * STEP_DTYPE.itemsize bytes -- fills that tensor in stream order without a host synchronisation."""
        return self._streams_step(self.lib.svo_streams_step, (self.height, self.width), ids, lefts, rights, results)

    def _streams_step(self, fn, shape, ids, lefts, rights, results):
        """svo_streams_step / svo_ingest_streams_step on one frame of `shape` per named stream."""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        m = int(ids.shape[0])
        fl, pl, pitch, fstride, mem = self._frame_stack(lefts, shape) if m else (None, None, shape[1], 0, MEM_HOST)
        fr, pr, pitch_r, fstride_r, mem_r = self._frame_stack(rights, shape) if m else (None, None, shape[1], 0, MEM_HOST)
        assert (pitch, fstride, mem) == (pitch_r, fstride_r, mem_r)
        assert m == 0 or (fl.shape[0] == m and fr.shape[0] == m)
        out, rp, rmem = _records(m, results)
        ordered = False
        if mem == MEM_DEVICE:
            ordered = self._order_in(fl)     # the frames (and a device result buffer) may still be in flight on torch's stream
        self._check(fn(self.h, C.c_void_p(ids.ctypes.data), m, pl, pr, pitch, fstride, mem, rp, rmem))
        if results is not None and ordered:
            self._order_out(fl)              # frames and records: before whatever torch's stream does next
        return out

    def streams_reset(self, id=-1):
        self._check(self.lib.svo_streams_reset(self.h, int(id)))

    def streams_get_pose(self, id):
        pose = np.zeros(16)
        self._check(self.lib.svo_streams_get_pose(self.h, int(id), C.c_void_p(pose.ctypes.data)))
        return pose.reshape(4, 4)

    def streams_set_pose(self, id, pose):
        pose = np.ascontiguousarray(pose, np.float64).reshape(16)
        self._check(self.lib.svo_streams_set_pose(self.h, int(id), C.c_void_p(pose.ctypes.data)))

    def streams_tracks(self, item, cap=65536):
        """(t1_left, t1_right, t2_right, t2_left, inlier) of item `item` of the last streams_step (empty for an init item)."""
        pts = [np.zeros((cap, 2), np.float32) for _ in range(4)]
        inl = np.zeros(cap, np.uint8)
        n = C.c_int(0)
        self._check(self.lib.svo_streams_get_tracks(self.h, int(item), *[C.c_void_p(p.ctypes.data) for p in pts],
                                                    C.c_void_p(inl.ctypes.data), cap, C.byref(n)))
        return [p[:n.value].copy() for p in pts] + [inl[:n.value].copy()]
