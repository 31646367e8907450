"""csrc/block_cut.h (no GPU): the one helper that cuts a device block into 256-byte-aligned sub-ranges gives the offsets the
three hand-written chains it replaced gave -- svo_bucket_corners' stage, gftt_plan's scratch, the refinement block -- which
are written out below in closed form as they stood.  A stand-alone C++ program that includes nothing but the header, built
with the address and undefined-behaviour sanitizers where the compiler has their runtimes, and run directly."""
import ctypes
import importlib
import os
import subprocess

import conftest

PROGRAM = r"""
#include "block_cut.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
using svo::BlockCut;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); failures++; } } while (0)
static size_t up(size_t v) { return (v + 255) / 256 * 256; }

// ---- the chains as they were written by hand ----------------------------------------------------------------------------
static void bucket_stage(size_t n, size_t ncells, bool host, bool dev_cells)
{
    const size_t o_xy = 256, o_resp = o_xy + up(8 * n), o_cells = o_resp + up(4 * n),
                 o_in = o_cells + (dev_cells ? up(4 * 4 * ncells) : 0), o_out = o_in + (host ? up(KP * n) : 0),
                 bytes = o_out + (host ? up(KP * n) : 0);
    BlockCut cut;
    CHECK(cut.add(256) == 0);
    CHECK(cut.add(8 * n) == o_xy);
    CHECK(cut.add(4 * n) == o_resp);
    CHECK(cut.add(dev_cells ? 4 * 4 * ncells : 0) == o_cells);
    CHECK(cut.add(host ? KP * n : 0) == o_in);
    CHECK(cut.add(host ? KP * n : 0) == o_out);
    CHECK(cut.total() == bytes);
}

static void gftt(size_t n, size_t w, size_t h, size_t cap, size_t ncells, bool dev_cells, bool with_lists, size_t extra)
{
    size_t ks = 64;
    while (ks < cap) ks <<= 1;
    const size_t mpitch = (w + 63) / 64 * 64;
    const size_t o_max = 0, o_cnt = up(4 * n), o_map = o_cnt + up(4 * n), o_keys = o_map + (with_lists ? up(4 * mpitch * h * n) : 0),
                 o_cells = o_keys + (with_lists ? up(8 * ks * n) : 0), o_extra = o_cells + (dev_cells ? up(4 * 4 * ncells * n) : 0),
                 bytes = o_extra + up(extra);
    CHECK(svo::align_up(w, 64) == mpitch);
    BlockCut cut;
    CHECK(cut.add(4 * n) == o_max);
    CHECK(cut.add(4 * n) == o_cnt);
    CHECK(cut.add(with_lists ? 4 * mpitch * h * n : 0) == o_map);
    CHECK(cut.add(with_lists ? 8 * ks * n : 0) == o_keys);
    CHECK(cut.add(dev_cells ? 4 * 4 * ncells * n : 0) == o_cells);
    CHECK(cut.add(extra) == o_extra);
    CHECK(cut.total() == bytes);
}

static void refine(size_t max_batch, size_t max_keypoints)
{
    const size_t f = up(REC * (max_batch + 1)), X = up(f + (max_batch + 1) * max_keypoints), xl = up(X + 4 * 3 * max_keypoints),
                 xr = up(xl + 8 * max_keypoints), end = up(xr + 8 * max_keypoints);
    BlockCut cut;
    CHECK(cut.add(REC * (max_batch + 1)) == 0);
    CHECK(cut.add((max_batch + 1) * max_keypoints) == f);
    CHECK(cut.add(4 * 3 * max_keypoints) == X);
    CHECK(cut.add(8 * max_keypoints) == xl);
    CHECK(cut.add(8 * max_keypoints) == xr);
    CHECK(cut.total() == end);
}

int main()
{
    // aligned, in call order, not overlapping; a zero-byte range consumes nothing
    const size_t sizes[] = {1, 0, 255, 256, 257, 0, 0, 100000, 3, 0, 65536, 7};
    BlockCut cut;
    CHECK(cut.total() == 0);
    size_t prev_end = 0;
    for (size_t b : sizes) {
        const size_t before = cut.total(), at = cut.add(b);
        CHECK(at % 256 == 0 && cut.total() % 256 == 0);
        CHECK(at == before && at >= prev_end);                   // starts where the block ended: behind every earlier range
        CHECK(cut.total() >= at + b && cut.total() < at + b + 256);
        if (b == 0) CHECK(cut.total() == before);
        if (b) prev_end = at + b;
    }
    CHECK(svo::align_up(0, 256) == 0 && svo::align_up(1, 256) == 256 && svo::align_up(256, 256) == 256 && svo::align_up(257, 64) == 320);
    for (size_t n : {(size_t)0, (size_t)1, (size_t)100000})
        for (int host = 0; host < 2; host++) {
            bucket_stage(n, 3072, host, false);                  // cells in LDS
            bucket_stage(n, 16384, host, true);                  // cells in device memory
        }
    for (size_t n : {(size_t)1, (size_t)4})
        for (int lists = 0; lists < 2; lists++) {
            gftt(n, 64, 48, 8192, 0, false, lists, 0);
            gftt(n, 64, 48, 500, 3072, true, lists, 64 * 48 + 12345);
        }
    for (size_t b : {(size_t)1, (size_t)256})
        for (size_t k : {(size_t)64, (size_t)16384}) refine(b, k);
    if (failures) return 1;
    printf("block cut ok\n");
    return 0;
}
"""


def _sanitizer_flags():
    """-fsanitize=address,undefined where g++ has both runtimes (the probe of test_oracle_sanitizers.py: the file name comes
    back as a path only when the library exists)"""
    for lib in ("libasan.so", "libubsan.so"):
        path = subprocess.check_output(["g++", "-print-file-name=" + lib]).decode().strip()
        if not (os.path.isabs(path) and os.path.exists(path)):
            return []
    return ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def test_block_cut_offsets_equal_the_hand_written_chains(tmp_path):
    binding = importlib.import_module(conftest.entry.load_package().__name__ + ".binding")
    src, exe = tmp_path / "block_cut_test.cpp", tmp_path / "block_cut_test"
    src.write_text(PROGRAM)
    csrc = os.path.join(conftest.ROOT, "stereo-visual-odometry_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", csrc, f"-DKP={binding.KP_DTYPE.itemsize}",
                           f"-DREC={ctypes.sizeof(binding.RefineResult)}"] + _sanitizer_flags() + ["-o", str(exe), str(src)])
    r = subprocess.run([str(exe)], capture_output=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1"))
    out = r.stdout.decode() + r.stderr.decode()
    assert r.returncode == 0 and "block cut ok" in out and "runtime error" not in out, out[-4000:]
