"""CPU test: the Shi-Tomasi detector's entry points are additive -- declared in include/svo_abi.h and exported by the library,
with the ABI version and svo_config exactly as they were (detected by symbol, like the FAST buckets)."""
import ctypes
import os
import re

import pytest

import conftest

SYMS = ["svo_set_lk_detector", "svo_get_lk_detector", "svo_min_eigen_map", "svo_gftt_detect"]


def test_gftt_symbols_declared_and_exported(pkg):
    hdr = open(os.path.join(conftest.ROOT, "include", "svo_abi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    pkg.build_library()
    lib = ctypes.CDLL(pkg.library_path())
    for s in SYMS:
        assert re.search(r"\bint\s+%s\s*\(" % s, code), s
        assert hasattr(lib, s), s
    assert re.search(r"#define\s+SVO_DETECTOR_FAST\s+0\b", code) and re.search(r"#define\s+SVO_DETECTOR_GFTT\s+1\b", code)
    assert "#define SVO_ABI_VERSION 9" in hdr and lib.svo_abi_version() == 9


def test_config_struct_unchanged(pkg):
    from importlib import import_module
    b = import_module(conftest.entry.PKG_NAME + ".binding")
    assert b.load_library().svo_config_bytes() == ctypes.sizeof(b.Config) == 296
    assert [f[0] for f in b.Config._fields_][-2:] == ["lk_accum", "fast_keep_strongest"]
    for m in ("set_lk_detector", "lk_detector", "min_eigen_map", "gftt_detect"):
        assert callable(getattr(b.Context, m))
    assert (b.DETECTOR_FAST, b.DETECTOR_GFTT) == (0, 1)


def test_null_context_is_an_argument_error(pkg):
    from importlib import import_module
    lib = import_module(conftest.entry.PKG_NAME + ".binding").load_library()
    assert lib.svo_set_lk_detector(None, 1, 500, 0.01, 20.0) == -1
    assert lib.svo_get_lk_detector(None, None, None, None, None) == -1
    assert lib.svo_min_eigen_map(None, None, 8, 8, 8, 0, None, 8) == -1
    assert lib.svo_gftt_detect(None, None, 8, 8, 8, 0, 0, 0.01, 0.0, None, None, 0, None) == -1


def test_binding_fails_loudly_without_gpu(pkg):
    import torch
    if torch.cuda.is_available():
        return
    with pytest.raises(pkg.SvoError):
        pkg.Context(64, 64).set_lk_detector("gftt")
