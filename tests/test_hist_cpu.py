"""CPU: the value histogram (include/vr/vr_hist.h) -- the reference helper tests/hist_ref.py
pinned by closed forms, vr_hist_edges and vr_hist_window against it bit for bit, the refusals,
the binding's symbol list and structs, and the host helper header under AddressSanitizer + UBSan
in a stand-alone program.  No GPU: nothing here creates a context."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hist_ref
import vr_amd
from harness import run_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
EDGE_CASES = [(-1.3, 2.7, 1000), (0.0, 65535.0, 4096)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- closed forms that pin the reference -----------------------------------------------------------
def test_bytes_over_their_codes_are_a_bincount():
    v = np.random.default_rng(1).integers(0, 256, size=(5, 6, 7), dtype=np.uint8)
    bins, info = hist_ref.histogram(v, 0, 256, 256)
    assert np.array_equal(bins, np.bincount(v.ravel(), minlength=256).astype(np.uint64))
    assert (info["voxels"], info["below"], info["above"], info["nan"]) == (v.size, 0, 0, 0)
    assert info["vmin"] == v.min() and info["vmax"] == v.max()


@pytest.mark.parametrize("lo,hi,nbins", EDGE_CASES)
def test_edge_values_fill_every_bin_with_two(lo, hi, nbins):
    e = hist_ref.edges(lo, hi, nbins)
    assert e.dtype == np.float32 and e[0] == F(lo) and np.all(np.diff(e) > 0)
    v = hist_ref.edge_values(lo, hi, nbins)
    assert v.size == 2 * nbins + 2
    bins, info = hist_ref.histogram(v, lo, hi, nbins)
    assert np.all(bins == 2) and info["below"] == 1 and info["above"] == 1 and info["nan"] == 0
    # the f32 floor((v - lo) * (nbins / (hi - lo))) estimate is not this rule
    ok = v[(v >= F(lo)) & (v <= F(hi))]
    est = np.floor((ok - F(lo)) * (F(nbins) / (F(hi) - F(lo)))).astype(np.int64)
    ref = np.searchsorted(e, ok, side="right") - 1
    assert np.count_nonzero(np.clip(est, 0, nbins - 1) != ref) > 0


def test_duplicate_edges_the_last_one_takes_the_value():
    lo, hi = F(1), np.nextafter(F(1), F(2))
    e = hist_ref.edges(lo, hi, 4)
    assert list(e) == [lo, lo, lo, hi]
    v = np.array([lo, lo, hi, np.nextafter(lo, F(0)), np.nextafter(hi, F(2))], F)
    bins, info = hist_ref.histogram(v, lo, hi, 4)
    assert list(bins) == [0, 0, 2, 1] and info["below"] == 1 and info["above"] == 1


def test_special_values():
    den = np.finfo(np.float32).smallest_subnormal
    v = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, den, -den, 1.0, 0.5], F)
    bins, info = hist_ref.histogram(v, 0, 1, 2)
    assert list(bins) == [3, 2]
    assert (info["voxels"], info["below"], info["above"], info["nan"]) == (9, 2, 1, 1)
    assert info["vmin"] == -np.inf and info["vmax"] == np.inf
    bins, info = hist_ref.histogram(np.array([np.nan, np.nan], F), 0, 1, 2)
    assert not bins.any() and info["nan"] == 2 and info["vmin"] == np.inf and info["vmax"] == -np.inf


def test_box():
    v = np.arange(4 * 5 * 6, dtype=np.float32).reshape(4, 5, 6)  # [z, y, x]
    bins, info = hist_ref.histogram(v, 0, 120, 120, box=((1, 2, 0), (3, 4, 2)))
    want = np.zeros(120, np.uint64)
    for z in (0, 1):
        for y in (2, 3):
            for x in (1, 2):
                want[(z * 5 + y) * 6 + x] = 1
    assert np.array_equal(bins, want) and info["voxels"] == 8
    assert info["vmin"] == 13 and info["vmax"] == 50


# ---- vr_hist_edges, vr_hist_window -----------------------------------------------------------------
@pytest.mark.parametrize("lo,hi,nbins", EDGE_CASES + [(-60, 60, 7), (0, 1, 1), (-3e38, 3e38, 4096),
                                                     (1, float(np.nextafter(F(1), F(2))), 4)])
def test_hist_edges_equal_the_reference(lo, hi, nbins):
    assert np.array_equal(bits(vr_amd.hist_edges(lo, hi, nbins)), bits(hist_ref.edges(lo, hi, nbins)))


def test_hist_edges_errors():
    L = vr_amd.lib()
    buf = np.full(8, 77, F)
    p = buf.ctypes.data_as(C.POINTER(C.c_float))
    assert L.vr_hist_edges(0.0, 1.0, 8, p) == 0 and buf[0] == 0
    buf[:] = 77
    assert L.vr_hist_edges(0.0, 1.0, 8, None) == -22
    for lo, hi, n in ((1.0, 1.0, 8), (2.0, 1.0, 8), (float("nan"), 1.0, 8), (0.0, float("inf"), 8),
                      (float("-inf"), 0.0, 8), (0.0, 1.0, 0), (0.0, 1.0, vr_amd.HIST_MAX_BINS + 1)):
        assert L.vr_hist_edges(lo, hi, n, p) == -22, (lo, hi, n)
    assert np.all(buf == 77)
    with pytest.raises(ValueError, match="vr_hist_edges"):
        vr_amd.hist_edges(1, 0, 4)


def _bins(kind):
    if kind == "mixed":
        b = (np.arange(64, dtype=np.uint64) * 37) % 11
        b[20] += 1000
        return b
    if kind == "single":
        b = np.zeros(16, np.uint64)
        b[5] = 9
        return b
    if kind == "last":
        b = np.zeros(16, np.uint64)
        b[15] = 1 << 33
        return b
    return np.random.default_rng(7).integers(0, 1 << 20, size=4096).astype(np.uint64)


@pytest.mark.parametrize("kind,lo,hi", [("mixed", -1, 3), ("single", 0, 16), ("last", 0, 16),
                                        ("random", -1000, 1000)])
@pytest.mark.parametrize("p", [(0.0, 1.0), (0.01, 0.99), (0.3, 0.31), (0.5, 1.0), (0.0, 1e-12)])
def test_hist_window_equals_the_reference(kind, lo, hi, p):
    b = _bins(kind)
    got = vr_amd.hist_window(b, lo, hi, *p)
    ref = hist_ref.window(b, lo, hi, *p)
    assert np.array_equal(bits(got), bits(ref))
    assert got[0] < got[1]
    if p == (0.0, 1.0):  # the bins that hold a count, from the first one's edge to the last one's end
        e = hist_ref.edges(lo, hi, b.size)
        nz = np.nonzero(b)[0]
        assert got[0] == e[nz[0]]
        assert got[1] == (F(hi) if nz[-1] == b.size - 1 else e[nz[-1] + 1])


def test_hist_window_errors():
    L = vr_amd.lib()
    b = _bins("single")
    bp = b.ctypes.data_as(C.POINTER(C.c_uint64))
    v0, v1 = C.c_float(-7), C.c_float(-7)

    def call(bins=bp, n=16, lo=0.0, hi=16.0, p0=0.0, p1=1.0, o0=True, o1=True):
        return L.vr_hist_window(bins, n, lo, hi, p0, p1, C.byref(v0) if o0 else None,
                                C.byref(v1) if o1 else None)

    zero = np.zeros(16, np.uint64)
    for bad in (dict(bins=None), dict(o0=False), dict(o1=False), dict(n=0),
                dict(n=vr_amd.HIST_MAX_BINS + 1), dict(lo=16.0), dict(lo=17.0), dict(hi=float("nan")),
                dict(hi=float("inf")), dict(lo=float("-inf")), dict(p0=-0.01), dict(p1=1.01),
                dict(p0=0.5, p1=0.5), dict(p0=0.6, p1=0.5), dict(p0=float("nan")), dict(p1=float("nan")),
                dict(bins=zero.ctypes.data_as(C.POINTER(C.c_uint64)))):
        assert call(**bad) == -22, bad
    assert v0.value == -7 and v1.value == -7
    for p in ((-0.01, 1.0), (0.0, 1.01), (0.5, 0.5), (0.6, 0.5), (float("nan"), 1.0)):
        assert hist_ref.window(b, 0, 16, *p) is None
    assert hist_ref.window(zero, 0, 16, 0, 1) is None and hist_ref.window(b, 16, 16, 0, 1) is None
    assert call() == 0 and (v0.value, v1.value) == (5.0, 6.0)
    with pytest.raises(ValueError, match="vr_hist_window"):
        vr_amd.hist_window(b, 0, 16, 0.5, 0.5)


def test_null_context_calls_are_refused():
    L = vr_amd.lib()
    req = vr_amd.vr_hist_request()
    req.lo, req.hi, req.nbins = 0.0, 1.0, 4
    bins = np.full(4, 77, np.uint64)
    info = vr_amd.vr_hist_info()
    info.voxels = 77
    assert L.vr_histogram(None, C.byref(req), bins.ctypes.data_as(C.POINTER(C.c_uint64)),
                          C.byref(info)) == -22
    assert L.vr_set_value_range(None, 0.0, 1.0) == -22
    assert np.all(bins == 77) and info.voxels == 77


# ---- the binding -------------------------------------------------------------------------------------
def test_every_declared_name_is_exported_and_listed():
    src = open(os.path.join(ROOT, "include", "vr", "vr_hist.h")).read()
    assert f"#define VR_HIST_MAX_BINS {vr_amd.HIST_MAX_BINS}" in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b(vr_[a-z0-9_]+)\s*\(", src))
    assert names == set(vr_amd.HIST_SYMBOLS) and len(names) == 4
    out = subprocess.run(["nm", "-D", "--defined-only", vr_amd.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not names - exported
    L = vr_amd.lib()
    assert all(getattr(L, n).argtypes is not None for n in names)
    assert vr_amd.ABI_VERSION == 9 and L.vr_abi_version() == 9  # an addition: the ABI stays
    assert vr_amd.KNOBS["hist_agg"] == 12 and vr_amd.KNOB_AUTO["hist_agg"] == -1
    assert "VR_KNOB_HIST_AGG = 12" in open(os.path.join(ROOT, "include", "vr", "vr_debug.h")).read()


def test_struct_layouts_match_header(tmp_path):
    test = r"""
#include "vr/vr_hist.h"
#include <stdio.h>
#include <stddef.h>
int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu  %zu %zu %zu %zu %zu %zu %zu\n",
  sizeof(vr_hist_request), offsetof(vr_hist_request, lo), offsetof(vr_hist_request, hi),
  offsetof(vr_hist_request, nbins), offsetof(vr_hist_request, use_box),
  offsetof(vr_hist_request, box_min), offsetof(vr_hist_request, box_max),
  sizeof(vr_hist_info), offsetof(vr_hist_info, voxels), offsetof(vr_hist_info, below),
  offsetof(vr_hist_info, above), offsetof(vr_hist_info, nan), offsetof(vr_hist_info, vmin),
  offsetof(vr_hist_info, vmax)); return 0; }
"""
    tmp = str(tmp_path / "vr_hist_layout")
    with open(tmp + ".c", "w") as f:
        f.write(test)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), tmp + ".c", "-o", tmp], check=True)
    out = subprocess.run([tmp], capture_output=True, text=True, check=True).stdout.split()
    R, I = vr_amd.vr_hist_request, vr_amd.vr_hist_info
    assert [int(x) for x in out] == [
        C.sizeof(R), R.lo.offset, R.hi.offset, R.nbins.offset, R.use_box.offset, R.box_min.offset,
        R.box_max.offset, C.sizeof(I), I.voxels.offset, I.below.offset, I.above.offset, I.nan.offset,
        I.vmin.offset, I.vmax.offset]
    assert C.sizeof(R) == 40 and C.sizeof(I) == 40


# ---- the host helper header, stand-alone, under AddressSanitizer + UBSan -----------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ missing")
def test_host_helpers_under_sanitizers(tmp_path):
    stdout = run_sanitized(tmp_path, "hist")
    seen = boxes = 0
    for line in stdout.splitlines():
        w = line.replace(":", " ").split()
        if w[0] == "box":
            # the request-check table: the box rule and the brick range, restated here (no size bound:
            # the voxel count and the brick count saturate at 2^64 - 1)
            use = int(w[1])
            lo, hi, dims = ([int(x) for x in w[a:a + 3]] for a in (2, 5, 9))
            ok, voxels, nwork = int(w[12]), int(w[13]), int(w[14])
            if not use:
                lo, hi = [0, 0, 0], dims
            assert ok == int(use <= 1 and all(lo[a] < hi[a] <= dims[a] for a in range(3))), line
            if ok:
                assert voxels == min((hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2]), 2 ** 64 - 1), line
                cells = (7, 8, 8)
                nb = [(hi[a] + 1) // cells[a] - (lo[a] + 2) // cells[a] + 1 for a in range(3)]
                assert nwork == min(nb[0] * nb[1] * nb[2], 2 ** 64 - 1), line
            else:
                assert voxels == 0 and nwork == 0, line
            boxes += 1
        elif w[0] == "edges":
            lo, hi, n = float.fromhex(w[1]), float.fromhex(w[2]), int(w[3])
            e = hist_ref.edges(lo, hi, n).view(np.uint32)
            step = n // 8 or 1
            assert [int(x, 16) for x in w[4:]] == [int(x) for x in e[::step]] + [int(e[-1])]
            seen += 1
        elif w[0] == "window":
            lo, hi, n, p0, p1 = float.fromhex(w[1]), float.fromhex(w[2]), int(w[3]), float(w[4]), float(w[5])
            b = {64: _bins("mixed"), 16: _bins("single")}[n]
            if w[5] == "1" and w[4] == "0.5":
                b = _bins("last")
            ref = hist_ref.window(b, lo, hi, p0, p1)
            assert int(w[6]) == 1 and [int(w[7], 16), int(w[8], 16)] == [int(x) for x in bits(ref)]
            seen += 1
    assert seen == 9 and boxes == 18
