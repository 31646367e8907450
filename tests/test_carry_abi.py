"""CPU test: the track-carry entry points are additive -- declared in include/svo_abi.h and exported by the library, with the
ABI version and svo_config exactly as they were (detected by symbol, like the buckets and the stream sets)."""
import ctypes
import os
import re

import conftest

SYMS = ["svo_set_track_carry", "svo_get_track_carry", "svo_carry_merge", "svo_get_frame_track_ids", "svo_get_last_track_ids",
        "svo_streams_get_track_ids", "svo_streams_get_frame_tracks"]


def test_carry_symbols_declared_and_exported(pkg):
    hdr = open(os.path.join(conftest.ROOT, "include", "svo_abi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    pkg.build_library()
    lib = ctypes.CDLL(pkg.library_path())
    for s in SYMS:
        assert re.search(r"\bint\s+%s\s*\(" % s, code), s
        assert hasattr(lib, s), s
    assert "#define SVO_ABI_VERSION 9" in hdr and lib.svo_abi_version() == 9


def test_config_struct_unchanged(pkg):
    from importlib import import_module
    b = import_module(conftest.entry.PKG_NAME + ".binding")
    assert b.load_library().svo_config_bytes() == ctypes.sizeof(b.Config) == 296
    assert [f[0] for f in b.Config._fields_][-2:] == ["lk_accum", "fast_keep_strongest"]
    for m in ("set_track_carry", "track_carry", "carry_merge", "frame_track_ids", "last_track_ids", "streams_track_ids",
              "streams_frame_tracks"):
        assert callable(getattr(b.Context, m))
