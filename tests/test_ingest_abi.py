"""CPU tests: the resize / ingest surface (svo_resize, svo_scale_projection, svo_ingest_*) is declared in include/svo_abi.h,
exported by the built library and bound by binding.Context -- additively: the ABI version and sizeof(svo_config) are what
they were before it existed -- and svo_scale_projection, which needs no device, satisfies the projection identity it is
defined by.  No compute call is made without a GPU."""
import ctypes
import os
import re
import sys
from importlib import import_module

import numpy as np
import pytest

import conftest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _resize_ref as RR   # noqa: E402
import _rigs               # noqa: E402

INGEST_SYMBOLS = ["svo_scale_projection", "svo_resize", "svo_ingest_create", "svo_ingest_info", "svo_ingest_add_frame",
                  "svo_ingest_track_batch", "svo_ingest_streams_step", "svo_ingest_upload_frames_at"]
INGEST_METHODS = ["resize", "ingest_create", "ingest_add_frame", "ingest_track_batch", "ingest_streams_step",
                  "ingest_upload_frames"]
PARENT_CONFIG_BYTES = 296


def _header():
    return open(os.path.join(conftest.ROOT, "include", "svo_abi.h")).read()


def test_header_declares_the_ingest_surface():
    hdr = _header()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(svo_[a-z_0-9]+)\s*\(", code))
    missing = [s for s in INGEST_SYMBOLS if s not in declared]
    assert not missing, missing
    assert re.search(r"#define\s+SVO_ABI_VERSION\s+9\b", hdr)
    assert re.search(r"#define\s+SVO_INTERP_NEAREST\s+0\b", hdr) and re.search(r"#define\s+SVO_INTERP_LINEAR\s+1\b", hdr)


def test_library_exports_the_ingest_surface(pkg):
    pkg.build_library()
    lib = ctypes.CDLL(pkg.library_path())
    missing = [s for s in INGEST_SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing
    assert lib.svo_abi_version() == 9
    assert lib.svo_config_bytes() == PARENT_CONFIG_BYTES


def test_binding_has_the_ingest_methods(pkg):
    b = import_module(conftest.entry.PKG_NAME + ".binding")
    missing = [m for m in INGEST_METHODS if not callable(getattr(b.Context, m, None))]
    assert not missing, missing
    assert callable(getattr(b, "scale_projection", None)) and callable(getattr(pkg, "scale_projection", None))
    assert (b.INTERP_NEAREST, b.INTERP_LINEAR) == (0, 1)
    assert ctypes.sizeof(b.Config) == PARENT_CONFIG_BYTES
    lib = b.load_library()
    assert all(getattr(lib, s).argtypes is not None for s in INGEST_SYMBOLS)


def _matrices():
    fx, cx, cy, tx = 718.856, 607.193, 185.216, -0.537              # the KITTI rig of svo_default_config
    kitti = (np.array([[fx, 0, cx, 0], [0, fx, cy, 0], [0, 0, 1, 0.0]]),
             np.array([[fx, 0, cx, fx * tx], [0, fx, cy, 0], [0, 0, 1, 0.0]]))
    return {"kitti": kitti, "R1": _rigs.matrices("R1"), "R3": _rigs.matrices("R3")}


@pytest.mark.parametrize("rig", ["kitti", "R1", "R3"])
@pytest.mark.parametrize("f", [0.5, 0.6])
def test_scale_projection_identity(pkg, rig, f):
    """Projecting with P and mapping the pixel to the resized image == projecting with svo_scale_projection(P), to 1e-9 px
    (the double rounding of a 3x3 by 3x4 product on coordinates below 1e4); nearest and linear differ by exactly (ox, oy)."""
    rng = np.random.default_rng(5)
    X = np.c_[rng.uniform(-8, 8, 300), rng.uniform(-3, 3, 300), rng.uniform(2, 60, 300), np.ones(300)]
    for P in _matrices()[rig]:
        uvw = X @ P.T
        assert (uvw[:, 2] > 0).all()
        u, v = uvw[:, 0] / uvw[:, 2], uvw[:, 1] / uvw[:, 2]
        assert np.abs(u).max() < 1e4 and np.abs(v).max() < 1e4
        outs = {}
        for interp in ("nearest", "linear"):
            Po = pkg.scale_projection(P, f, f, interp)
            assert Po.shape == (3, 4)
            o = X @ Po.T
            uo, vo = o[:, 0] / o[:, 2], o[:, 1] / o[:, 2]
            if interp == "nearest":
                ue, ve = u * f, v * f                               # destination pixel dx shows source pixel dx / f
            else:
                ue, ve = (u + 0.5) * f - 0.5, (v + 0.5) * f - 0.5   # pixel centres
            print(rig, f, interp, "max |du|, |dv| =", np.abs(uo - ue).max(), np.abs(vo - ve).max())
            assert np.abs(uo - ue).max() <= 1e-9 and np.abs(vo - ve).max() <= 1e-9
            assert np.allclose(Po, RR.scale_projection(P, f, f, interp), rtol=0, atol=1e-12)
            outs[interp] = (Po, uo, vo)
        d = outs["linear"][0] - outs["nearest"][0]
        ox = 0.5 * (f - 1)
        # the two interpolations see every point exactly (ox, oy) apart
        assert np.abs(outs["linear"][1] - outs["nearest"][1] - ox).max() <= 1e-9
        assert np.abs(outs["linear"][2] - outs["nearest"][2] - ox).max() <= 1e-9
        expect = np.zeros((3, 4))
        expect[0] = ox * P[2]
        expect[1] = ox * P[2]
        assert np.allclose(d, expect, rtol=0, atol=1e-12)
        # rectified rigs (third row (0, 0, 1, 0)): the offset lands in the principal point alone -- (ox, oy) up to the one
        # rounding of inv * c + o, nothing else differs
        if rig != "R3":
            assert np.count_nonzero(d) == 2 and abs(d[0, 2] - ox) <= 1e-12 and abs(d[1, 2] - ox) <= 1e-12


def test_scale_projection_arguments(pkg):
    P = _matrices()["kitti"][0]
    lib = pkg.load_library()
    out = np.zeros(12)
    pp, po = ctypes.c_void_p(np.ascontiguousarray(P).ctypes.data), ctypes.c_void_p(out.ctypes.data)
    assert lib.svo_scale_projection(pp, 0.5, 0.5, 0, po) == 0
    for bad in [(0.0, 0.5, 0), (0.5, 1.5, 0), (-0.5, 0.5, 1), (0.5, 0.5, 2)]:
        assert lib.svo_scale_projection(pp, bad[0], bad[1], bad[2], po) == -1, bad
    assert lib.svo_scale_projection(None, 0.5, 0.5, 0, po) == -1
    assert np.array_equal(pkg.scale_projection(P, 1.0, 1.0, "linear"), P)
