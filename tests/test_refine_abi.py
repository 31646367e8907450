"""CPU tests: the pose refinement surface (svo_set_pose_refine, svo_get_pose_refine, svo_refine_pose, svo_get_refine_result) is
declared in include/svo_abi.h, exported by the built library and bound by binding.Context -- additively: the ABI version,
sizeof(svo_config) and sizeof(svo_step_result) are what they were before it existed -- and svo_refine_result has the layout
the binding assumes.  No compute call is made without a GPU."""
import ctypes
import os
import re
import subprocess
from importlib import import_module

import pytest

import conftest

REFINE_SYMBOLS = ["svo_set_pose_refine", "svo_get_pose_refine", "svo_refine_pose", "svo_get_refine_result"]
REFINE_METHODS = ["set_pose_refine", "pose_refine", "refine_pose", "refine_result"]
PARENT_CONFIG_BYTES = 296
PARENT_STEP_BYTES = 408          # 8 int32 + (3 + 3 + 9 + 16 + 16) doubles
REFINE_BYTES = 496               # (3 + 3 + 9 + 3 + 3 + 36 + 2) doubles + 6 int32


def _header():
    return open(os.path.join(conftest.ROOT, "include", "svo_abi.h")).read()


def test_header_declares_the_refine_surface():
    hdr = _header()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(svo_[a-z_0-9]+)\s*\(", code))
    missing = [s for s in REFINE_SYMBOLS if s not in declared]
    assert not missing, missing
    assert re.search(r"#define\s+SVO_ABI_VERSION\s+9\b", hdr)
    for name, value in (("SVO_REFINE_OFF", 0), ("SVO_REFINE_REPROJ", 1), ("SVO_REFINE_APPLIED", 0), ("SVO_REFINE_KEPT_PNP", 1),
                        ("SVO_REFINE_SKIPPED", 2)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", hdr), name
    assert "svo_refine_result;" in code


def test_library_exports_the_refine_surface(pkg):
    pkg.build_library()
    lib = ctypes.CDLL(pkg.library_path())
    missing = [s for s in REFINE_SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing
    assert lib.svo_abi_version() == 9
    assert lib.svo_config_bytes() == PARENT_CONFIG_BYTES


def test_struct_sizes_match_the_header(pkg, tmp_path):
    """The C compiler's view of the header against the binding's ctypes structures, field offsets included."""
    b = import_module(conftest.entry.PKG_NAME + ".binding")
    fields = [f[0] for f in b.RefineResult._fields_]
    src = tmp_path / "sizes.c"
    prints = "".join(f'    printf("{f} %zu\\n", offsetof(svo_refine_result, {f}));\n' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "svo_abi.h"\nint main(void) {\n'
                   '    printf("config %zu\\nstep %zu\\nrefine %zu\\n", sizeof(svo_config), sizeof(svo_step_result), sizeof(svo_refine_result));\n'
                   + prints + "    return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(conftest.ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["config"]) == PARENT_CONFIG_BYTES == ctypes.sizeof(b.Config)
    assert int(got["step"]) == PARENT_STEP_BYTES == ctypes.sizeof(b.StepResult) == b.STEP_DTYPE.itemsize
    assert int(got["refine"]) == REFINE_BYTES == ctypes.sizeof(b.RefineResult)
    for f in fields:
        assert int(got[f]) == getattr(b.RefineResult, f).offset, f


def test_null_context_is_refused_by_every_entry(pkg):
    pkg.build_library()
    lib = ctypes.CDLL(pkg.library_path())
    res = (ctypes.c_double * 62)()
    assert lib.svo_set_pose_refine(None, 1, 4, 10, ctypes.c_double(1.0), 6) == -1
    assert lib.svo_get_pose_refine(None, None, None, None, None, None) == -1
    assert lib.svo_refine_pose(None, None, None, None, 0, None, None, None, None, res, None, 0) == -1
    assert lib.svo_get_refine_result(None, 0, res, None, 0, None) == -1


def test_binding_has_the_refine_methods_and_raises_without_a_gpu(pkg):
    b = import_module(conftest.entry.PKG_NAME + ".binding")
    missing = [m for m in REFINE_METHODS if not callable(getattr(b.Context, m, None))]
    assert not missing, missing
    assert (b.REFINE_OFF, b.REFINE_REPROJ) == (0, 1) and (b.REFINE_APPLIED, b.REFINE_KEPT_PNP, b.REFINE_SKIPPED) == (0, 1, 2)
    assert pkg.RefineResult is b.RefineResult
    lib = b.load_library()
    assert all(getattr(lib, s).argtypes is not None for s in REFINE_SYMBOLS)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(b.SvoError):                 # no device: no context, so no refinement -- there is no CPU fallback
            b.Context(416, 128).set_pose_refine("reproj")
