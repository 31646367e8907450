"""CPU tests: the bundle-adjustment surface of the pose stage (SVO_REFINE_BA, svo_refine_ba, svo_get_refine_points) is
declared in include/svo_abi.h, exported by the built library and bound by binding.Context -- additively: the ABI version and
sizeof(svo_config), sizeof(svo_step_result) and sizeof(svo_refine_result) are what they were before it existed.  No compute
call is made without a GPU."""
import ctypes
import os
import re
import subprocess
from importlib import import_module

import pytest

import conftest

BA_SYMBOLS = ["svo_set_pose_refine_ba", "svo_refine_ba", "svo_get_refine_points"]
BA_METHODS = ["refine_ba", "refine_points"]
PARENT_CONFIG_BYTES, PARENT_STEP_BYTES, PARENT_REFINE_BYTES = 296, 408, 496


def _header():
    return open(os.path.join(conftest.ROOT, "include", "svo_abi.h")).read()


def test_header_declares_the_ba_surface():
    hdr = _header()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(svo_[a-z_0-9]+)\s*\(", code))
    missing = [s for s in BA_SYMBOLS if s not in declared]
    assert not missing, missing
    assert re.search(r"#define\s+SVO_ABI_VERSION\s+9\b", hdr)
    for name, value in (("SVO_REFINE_OFF", 0), ("SVO_REFINE_REPROJ", 1), ("SVO_REFINE_BA", 2)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", hdr), name
    # the argument order: four observation lists, X_out before mem
    proto = re.search(r"int\s+svo_refine_ba\s*\(([^;]*)\)\s*;", code, flags=re.S).group(1)
    names = re.findall(r"(\w+)\s*(?:\[\d+\])?\s*(?:,|$)", re.sub(r"\s+", " ", proto))
    assert names == ["ctx", "obj", "img1_left", "img1_right", "img2_left", "img2_right", "n", "P1", "P2", "rvec0", "tvec0", "res",
                     "active", "X_out", "mem"], names


def test_library_exports_the_ba_surface(pkg):
    pkg.build_library()
    lib = ctypes.CDLL(pkg.library_path())
    missing = [s for s in BA_SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing
    assert lib.svo_abi_version() == 9
    assert lib.svo_config_bytes() == PARENT_CONFIG_BYTES


def test_struct_sizes_are_unchanged(pkg, tmp_path):
    b = import_module(conftest.entry.PKG_NAME + ".binding")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "svo_abi.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %d\\n", sizeof(svo_config), sizeof(svo_step_result), sizeof(svo_refine_result), SVO_REFINE_BA);\n'
                   "    return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(conftest.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [PARENT_CONFIG_BYTES, PARENT_STEP_BYTES, PARENT_REFINE_BYTES, 2]
    assert (ctypes.sizeof(b.Config), ctypes.sizeof(b.StepResult), ctypes.sizeof(b.RefineResult)) == tuple(got[:3])


def test_null_context_is_refused_by_every_entry(pkg):
    pkg.build_library()
    lib = ctypes.CDLL(pkg.library_path())
    res = (ctypes.c_double * 62)()
    assert lib.svo_set_pose_refine_ba(None, 4, 10, ctypes.c_double(1.0), 6) == -1
    assert lib.svo_refine_ba(None, None, None, None, None, None, 0, None, None, None, None, res, None, None, 0) == -1
    assert lib.svo_get_refine_points(None, 0, None, 0, None) == -1


def test_binding_has_the_ba_methods_and_raises_without_a_gpu(pkg):
    b = import_module(conftest.entry.PKG_NAME + ".binding")
    missing = [m for m in BA_METHODS if not callable(getattr(b.Context, m, None))]
    assert not missing, missing
    assert (b.REFINE_OFF, b.REFINE_REPROJ, b.REFINE_BA) == (0, 1, 2) and pkg.REFINE_BA == 2
    lib = b.load_library()
    assert all(getattr(lib, s).argtypes is not None for s in BA_SYMBOLS)
    assert len(lib.svo_refine_ba.argtypes) == 15 and len(lib.svo_get_refine_points.argtypes) == 5
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(b.SvoError):                 # no device: no context -- there is no CPU fallback
            b.Context(416, 128).set_pose_refine("ba")
