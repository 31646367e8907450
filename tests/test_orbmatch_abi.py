"""CPU test: the guided ORB matcher's entry points are additive -- declared in include/svo_abi.h and exported by the library,
with the ABI version and svo_config exactly as they were (detected by symbol, like the Shi-Tomasi detector)."""
import ctypes
import os
import re

import pytest

import conftest

SIGS = {
    "svo_set_orb_matcher": "svo_ctx *ctx, int mode, int th_stereo, int th_track, double ratio, double radius, double max_disparity",
    "svo_get_orb_matcher": "const svo_ctx *ctx, int *mode, int *th_stereo, int *th_track, double *ratio, double *radius, double *max_disparity",
    "svo_orb_stereo_frame": "svo_ctx *ctx, const uint8_t *left, const uint8_t *right, int pitch, int mem, int slot, svo_keypoint *kps, "
                            "float *uR, int32_t *sad, int cap, int *n_out",
    "svo_orb_track_frames": "svo_ctx *ctx, int slot_prev, int slot_cur, svo_pt2f *t1_left, svo_pt2f *t1_right, svo_pt2f *t2_left, "
                            "int32_t *idx_prev, int32_t *idx_cur, int cap, int *n_out",
    "svo_get_frame_stereo": "svo_ctx *ctx, float *uR, int32_t *sad, int cap, int *n_out",
}


def _norm(s):
    return re.sub(r"\s+", " ", s).strip()


def test_orbmatch_symbols_declared_and_exported(pkg):
    hdr = open(os.path.join(conftest.ROOT, "include", "svo_abi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    pkg.build_library()
    lib = ctypes.CDLL(pkg.library_path())
    for s, args in SIGS.items():
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % s, code, flags=re.S)
        assert m, s
        assert _norm(m.group(1)) == _norm(args), s             # struct-free: scalars and pointers to plain arrays only
        assert hasattr(lib, s), s
    assert re.search(r"#define\s+SVO_ORB_MATCHER_BRUTE\s+0\b", code) and re.search(r"#define\s+SVO_ORB_MATCHER_GUIDED\s+1\b", code)
    assert "#define SVO_ABI_VERSION 9" in hdr and lib.svo_abi_version() == 9


def test_config_struct_unchanged_and_binding_argtypes(pkg):
    from importlib import import_module
    b = import_module(conftest.entry.PKG_NAME + ".binding")
    C = ctypes
    lib = b.load_library()
    assert lib.svo_config_bytes() == ctypes.sizeof(b.Config) == 296
    assert [f[0] for f in b.Config._fields_][-2:] == ["lk_accum", "fast_keep_strongest"]
    for m in ("set_orb_matcher", "get_orb_matcher", "orb_stereo_frame", "orb_track_frames", "get_frame_stereo"):
        assert callable(getattr(b.Context, m))
    assert (b.ORB_MATCHER_BRUTE, b.ORB_MATCHER_GUIDED) == (0, 1) == (pkg.ORB_MATCHER_BRUTE, pkg.ORB_MATCHER_GUIDED)
    assert lib.svo_set_orb_matcher.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double]
    assert lib.svo_get_orb_matcher.argtypes == [C.c_void_p] + [C.POINTER(C.c_int)] * 3 + [C.POINTER(C.c_double)] * 3
    assert lib.svo_orb_stereo_frame.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    assert lib.svo_orb_track_frames.argtypes == [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.POINTER(C.c_int)]
    assert lib.svo_get_frame_stereo.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]


def test_null_context_is_an_argument_error(pkg):
    from importlib import import_module
    lib = import_module(conftest.entry.PKG_NAME + ".binding").load_library()
    assert lib.svo_set_orb_matcher(None, 1, 75, 100, 0.9, 0.0, 0.0) == -1
    assert lib.svo_get_orb_matcher(None, None, None, None, None, None, None) == -1
    assert lib.svo_orb_stereo_frame(None, None, None, 8, 0, 0, None, None, None, 0, None) == -1
    assert lib.svo_orb_track_frames(None, 0, 1, None, None, None, None, None, 0, None) == -1
    assert lib.svo_get_frame_stereo(None, None, None, 0, None) == -1


def test_binding_fails_loudly_without_gpu(pkg):
    import torch
    if torch.cuda.is_available():
        return
    with pytest.raises(pkg.SvoError):
        pkg.Context(64, 64, track_mode=pkg.MODE_ORB).set_orb_matcher("guided")
