"""CPU test: the sliding-window entry point is additive -- declared in include/svo_abi.h and exported by the library, with the
ABI version and svo_config exactly as they were (detected by symbol, like track carry)."""
import ctypes
import os
import re

import conftest

SYMS = ["svo_window_update", "svo_window_ba", "svo_set_window_ba", "svo_get_window_ba", "svo_get_window", "svo_get_window_result"]


def test_window_symbols_declared_and_exported(pkg):
    hdr = open(os.path.join(conftest.ROOT, "include", "svo_abi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    pkg.build_library()
    lib = ctypes.CDLL(pkg.library_path())
    for s in SYMS:
        assert re.search(r"\bint\s+%s\s*\(" % s, code), s
        assert hasattr(lib, s), s
    assert "#define SVO_ABI_VERSION 9" in hdr and lib.svo_abi_version() == 9
    assert re.search(r"#define\s+SVO_WINDOW_MAX_FRAMES\s+8\b", code)


def test_table_struct_and_binding(pkg):
    from importlib import import_module
    b = import_module(conftest.entry.PKG_NAME + ".binding")
    assert b.load_library().svo_config_bytes() == ctypes.sizeof(b.Config) == 296
    assert ctypes.sizeof(b.WindowTable) == 8 * ctypes.sizeof(ctypes.c_void_p) and b.WINDOW_MAX_FRAMES == 8
    hdr = open(os.path.join(conftest.ROOT, "include", "svo_abi.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} svo_window_table;", hdr).group(1)
    assert re.findall(r"\*\s*(\w+)", body) == [f[0] for f in b.WindowTable._fields_]
    assert all(callable(getattr(b.Context, m)) for m in ("window_update", "window_solve", "set_window_ba", "window_ba", "window", "window_result"))
    res = re.search(r"typedef struct \{([^}]*)\} svo_window_result;", hdr).group(1)
    assert ctypes.sizeof(b.WindowResult) == 8 * 4 + 8 * 4 + 2 * 8 + 42 * 42 * 8 and "info[42 * 42]" in res
