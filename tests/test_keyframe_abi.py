"""CPU test: the keyframe entry points are additive -- declared in include/svo_abi.h and exported by the library, with the ABI
version and svo_config exactly as they were (detected by symbol, like track carry and the sliding window) -- and the binding
mirrors the result struct and checks its arguments before it calls the library."""
import ctypes
import os
import re

import numpy as np
import pytest

import conftest

SYMS = ["svo_set_keyframe", "svo_get_keyframe", "svo_get_keyframe_result", "svo_get_keyframe_matches", "svo_get_keyframe_table",
        "svo_keyframe_join"]
STATUS = ["NONE", "SHORT", "PAIR_FAILED", "REJECTED", "APPLIED"]


def _binding():
    from importlib import import_module
    return import_module(conftest.entry.PKG_NAME + ".binding")


def test_keyframe_symbols_declared_and_exported(pkg):
    hdr = open(os.path.join(conftest.ROOT, "include", "svo_abi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    pkg.build_library()
    lib = ctypes.CDLL(pkg.library_path())
    for s in SYMS:
        assert re.search(r"\bint\s+%s\s*\(" % s, code), s
        assert hasattr(lib, s), s
    assert "#define SVO_ABI_VERSION 9" in hdr and lib.svo_abi_version() == 9
    for k, name in enumerate(STATUS):
        assert re.search(r"#define\s+SVO_KF_%s\s+%d\b" % (name, k), code), name
        assert getattr(pkg, "KF_" + name) == k
    for rule in ("K1", "K2", "K3", "K4", "K5", "K6", "K7", "K8"):    # the rules are stated where C1-C8 and T1-T7 are
        assert re.search(r"^ \*   %s " % rule, hdr, flags=re.M), rule


def test_result_struct_and_binding(pkg):
    b = _binding()
    assert b.load_library().svo_config_bytes() == ctypes.sizeof(b.Config) == 296
    hdr = open(os.path.join(conftest.ROOT, "include", "svo_abi.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} svo_keyframe_result;", hdr).group(1)
    names = [n for n in re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)]
    assert names == [f[0] for f in b.KeyframeResult._fields_]
    assert ctypes.sizeof(b.KeyframeResult) == 10 * 4 + (3 + 3 + 16 + 16) * 8 == 344
    for m in ("set_keyframe", "keyframe", "keyframe_result", "keyframe_matches", "keyframe_table", "keyframe_join"):
        assert callable(getattr(b.Context, m))
    r = b.KeyframeResult(status=4, kf_index=-1)
    r.pose_K[5] = 2.5
    d = r.as_dict()
    assert d["status"] == 4 and d["kf_index"] == -1 and d["pose_K"].shape == d["pose_pair"].shape == (4, 4) and d["pose_K"][1, 1] == 2.5


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the binding called {name} with arguments it should have refused")


def test_binding_argument_checks(pkg):
    """refused in Python, before the library is reached (no context, no device)"""
    b = _binding()
    c = object.__new__(b.Context)
    c.lib, c.h = _NoLibrary(), None
    for bad in [dict(min_tracks=3), dict(min_tracks=0), dict(max_gap=-1), dict(max_gap=1)]:
        with pytest.raises(ValueError):
            c.set_keyframe(True, **bad)
    ids, X, xy = np.arange(4, dtype=np.int64), np.zeros((4, 3), np.float32), np.zeros((4, 2), np.float32)
    with pytest.raises(ValueError):
        c.keyframe_join(ids, X[:3], ids, xy)
    with pytest.raises(ValueError):
        c.keyframe_join(ids, X, ids, xy[:2])
