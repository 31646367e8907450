"""CPU test: the stream-set surface (svo_streams_*) is declared in include/svo_abi.h, exported by the built library and
bound by binding.Context -- additively: the ABI version and sizeof(svo_config) are what they were before it existed.
No compute call is made without a GPU."""
import ctypes
import os
import re
from importlib import import_module

import conftest

STREAM_SYMBOLS = ["svo_streams_create", "svo_streams_count", "svo_streams_step", "svo_streams_reset",
                  "svo_streams_get_pose", "svo_streams_set_pose", "svo_streams_get_tracks"]
STREAM_METHODS = ["streams_create", "streams_step", "streams_reset", "streams_get_pose", "streams_set_pose",
                  "streams_tracks"]
# svo_config_bytes() of the commit before the stream set was added: no svo_config field came with it
PARENT_CONFIG_BYTES = 296


def _declared_symbols():
    hdr = open(os.path.join(conftest.ROOT, "include", "svo_abi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return set(re.findall(r"\b(svo_[a-z_0-9]+)\s*\(", hdr))


def test_header_declares_the_stream_set_surface():
    missing = [s for s in STREAM_SYMBOLS if s not in _declared_symbols()]
    assert not missing, missing
    hdr = open(os.path.join(conftest.ROOT, "include", "svo_abi.h")).read()
    assert re.search(r"#define\s+SVO_ABI_VERSION\s+9\b", hdr)


def test_library_exports_the_stream_set_surface(pkg):
    pkg.build_library()
    lib = ctypes.CDLL(pkg.library_path())
    missing = [s for s in STREAM_SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing
    assert lib.svo_abi_version() == 9
    assert lib.svo_config_bytes() == PARENT_CONFIG_BYTES


def test_binding_has_the_stream_set_methods(pkg):
    b = import_module(conftest.entry.PKG_NAME + ".binding")
    missing = [m for m in STREAM_METHODS if not callable(getattr(b.Context, m, None))]
    assert not missing, missing
    assert ctypes.sizeof(b.Config) == PARENT_CONFIG_BYTES
    lib = b.load_library()
    assert all(getattr(lib, s).argtypes is not None for s in STREAM_SYMBOLS)
