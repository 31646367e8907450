"""CPU test: the FAST corner bucket entry points are additive -- declared in include/svo_abi.h and exported by the library,
with the ABI version and svo_config exactly as they were (detected by symbol, like the stream sets and the ingest stage)."""
import ctypes
import os
import re

import conftest

SYMS = ["svo_set_fast_buckets", "svo_get_fast_buckets", "svo_bucket_corners"]


def test_bucket_symbols_declared_and_exported(pkg):
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
    # 296 bytes: the layout of ABI v9 (tests/test_abi_symbols.py pins the binding's Config against the library)
    assert b.load_library().svo_config_bytes() == ctypes.sizeof(b.Config) == 296
    assert [f[0] for f in b.Config._fields_][-2:] == ["lk_accum", "fast_keep_strongest"]
    for m in ("set_fast_buckets", "fast_buckets", "bucket_corners"):
        assert callable(getattr(b.Context, m))
