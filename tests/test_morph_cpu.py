"""CPU: the exact distance transform and ball morphology (include/vr/vr_morph.h) -- the reference
tests/morph_ref.py pinned against the definitions pair by pair and against scipy where it is
installed; the second library's symbols and structs; the refusals that need no device; and the host
helper header under AddressSanitizer + UBSan in a stand-alone program (the kernels of both
libraries: tests/test_kernel_inventory_cpu.py).
No GPU: nothing here creates a context."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import morph_ref as R
import morph_scenes as S
import vr_amd
from harness import run_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference, pinned before anything is compared with it ----------------------------------------
@pytest.mark.parametrize("shape", [(5, 6, 7), (1, 1, 9), (4, 1, 1), (3, 5, 2), (1, 1, 1)])  # (bz, by, bx)
def test_reference_equals_the_definition_pair_by_pair(shape):
    rng = np.random.default_rng(sum(shape))
    for density in (0.0, 0.03, 0.3, 0.9, 1.0):
        m = rng.random(shape) < density
        for t in (m, ~m):
            assert np.array_equal(R.edt2(t), R.brute_edt2(t))
        for r2 in (0, 1, 2, 3, 5, 9, 100):
            assert np.array_equal(R.dilate(m, r2), R.brute_dilate(m, r2)), (density, r2)
            assert np.array_equal(R.erode(m, r2), R.brute_erode(m, r2)), (density, r2)
            for op, want in ((R.DILATE, R.brute_dilate(m, r2)), (R.ERODE, R.brute_erode(m, r2)),
                             (R.OPEN, R.brute_dilate(R.brute_erode(m, r2), r2)),
                             (R.CLOSE, R.brute_erode(R.brute_dilate(m, r2), r2))):
                out, info = R.morph(m.astype(np.uint8), op, r2)
                assert out.dtype == np.uint8 and np.array_equal(out, want.astype(np.uint8)), (density, op, r2)
                assert info == {"voxels": m.size, "in_set": int(m.sum()), "out_set": int(want.sum())}
            if r2 == 0:
                assert all(np.array_equal(R.morph(m, op, 0)[0], m.astype(np.uint8)) for op in range(4))


@pytest.mark.parametrize("name", list(S.SHAPES))
@pytest.mark.parametrize("target", [R.TO_SET, R.TO_UNSET])
def test_reference_equals_scipy(name, target):
    ndi = pytest.importorskip("scipy.ndimage")
    m = S.mask(name) != 0
    t = m if target == R.TO_SET else ~m
    d, info = S.reference_edt(name, target)
    assert d.dtype == np.uint32 and d.shape == m.shape == S.SHAPES[name][::-1]
    assert info["voxels"] == m.size and info["target_voxels"] == int(t.sum())
    if not t.any():
        assert np.all(d == R.NONE) and (info["max_dist2"], info["max_index"]) == (R.NONE, 0)
        return
    idx = ndi.distance_transform_edt(~t, return_distances=False, return_indices=True)
    off = idx.astype(np.int64) - np.indices(m.shape)
    want = (off * off).sum(axis=0)  # the squared offset to scipy's nearest target voxel: an exact integer
    assert np.array_equal(d.astype(np.int64), want)
    assert info["max_dist2"] == int(want.max()) and info["max_index"] == int(np.argmax(want.reshape(-1)))


def test_the_corner_scene_and_the_sentinel():
    d, info = S.reference_edt("corner", R.TO_SET)
    bx, by, bz = S.SHAPES["corner"]
    assert info["max_dist2"] == S.diagonal2("corner") == (bx - 1) ** 2 + (by - 1) ** 2 + (bz - 1) ** 2
    assert info["max_index"] == bx * by * bz - 1 and info["target_voxels"] == 1  # the far corner
    assert 3 * 32767 ** 2 < R.NONE == vr_amd.EDT_NONE and vr_amd.MORPH_MAX_EXTENT == 32768
    assert int(S.reference_edt("far200", R.TO_SET)[1]["max_dist2"]) > 1000  # distances into the thousands
    assert sorted(int(S.mask(n).sum()) for n in ("thin_x", "thin_y", "thin_z")) == [3, 3, 3]
    assert int(S.mask("far200").sum()) == 30 and not S.mask("empty").any() and S.mask("full").all()
    # the grid's border erodes nothing: a full mask stays full under erosion and closing
    for op in (R.ERODE, R.CLOSE):
        assert S.reference_morph("full", op, 100)[0].all()
    assert not S.reference_morph("empty", R.DILATE, 100)[0].any()


@pytest.mark.parametrize("name", S.SMALL)
def test_ops_equal_scipy_with_the_ball_footprint(name):
    ndi = pytest.importorskip("scipy.ndimage")
    m = S.mask(name) != 0
    for r2 in (0, 1, 2, 3, 9, 100):
        fp = R.ball(r2)
        dil = ndi.binary_dilation(m, structure=fp, border_value=0)
        ero = ndi.binary_erosion(m, structure=fp, border_value=1)
        assert np.array_equal(S.reference_morph(name, R.DILATE, r2)[0], dil.astype(np.uint8)), r2
        assert np.array_equal(S.reference_morph(name, R.ERODE, r2)[0], ero.astype(np.uint8)), r2
        opened = ndi.binary_dilation(ero, structure=fp, border_value=0)
        closed = ndi.binary_erosion(dil, structure=fp, border_value=1)
        assert np.array_equal(S.reference_morph(name, R.OPEN, r2)[0], opened.astype(np.uint8)), r2
        assert np.array_equal(S.reference_morph(name, R.CLOSE, r2)[0], closed.astype(np.uint8)), r2


def test_the_cases_cover_every_op_width_and_radius():
    cases = S.morph_cases()
    assert {c[1] for c in cases} == {0, 1, 2, 3} and {c[0] for c in cases} == set(S.SHAPES)
    for name in S.SMALL:
        assert {c[2] for c in cases if c[0] == name} == {0, 1, 2, 3, 9, 100, S.diagonal2(name) + 1}
    lab = S.as_labels(S.mask("rows129"))
    assert lab.dtype == np.uint32 and np.array_equal(lab != 0, S.mask("rows129") != 0)
    assert ((lab & 0xFF) == 0).all() and lab.max() > 0xFFFF  # set iff non-zero: no single byte says it


# ---- the binding ---------------------------------------------------------------------------------------
def test_every_declared_name_is_exported_and_listed():
    src = open(os.path.join(ROOT, "include", "vr", "vr_morph.h")).read()
    assert '#include "vr_mesh.h"' in src and "#define VR_ENOSPC" not in src  # reused, not redefined
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b(vr_[a-z0-9_]+)\s*\(", src))
    assert names == set(vr_amd.MORPH_SYMBOLS) and len(names) == 5
    assert os.path.dirname(vr_amd.MORPH_LIB_PATH) == os.path.dirname(vr_amd.LIB_PATH)
    nm = lambda path: {l.split()[-1] for l in subprocess.run(
        ["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout.splitlines()
        if " T " in l}
    assert not names - nm(vr_amd.MORPH_LIB_PATH)
    assert not names & nm(vr_amd.LIB_PATH)  # the first library holds none of them
    L = vr_amd.morph_lib()
    assert all(getattr(L, n).argtypes is not None for n in names)
    assert vr_amd.ABI_VERSION == 9 and vr_amd.lib().vr_abi_version() == 9  # an addition: the ABI stays
    for m in ("distance_transform", "distance_transform_device", "morph", "morph_device", "morph_last_kernel_name"):
        assert callable(getattr(vr_amd.OffscreenPass, m))
    # the second library takes the scaffold from the first, found beside it
    dyn = subprocess.run(["readelf", "-d", vr_amd.MORPH_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libvr_amd.so" in dyn and "$ORIGIN" in dyn


def test_struct_layouts_match_header(tmp_path):
    fields = {"vr_edt_info": ["voxels", "target_voxels", "max_dist2", "max_index"],
              "vr_morph_info": ["voxels", "in_set", "out_set"]}
    body = "".join(f'  printf("%zu ", sizeof({s}));\n' +
                   "".join(f'  printf("%zu ", offsetof({s}, {f}));\n' for f in fs) for s, fs in fields.items())
    test = '#include "vr/vr_morph.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n' + body + \
           '  printf("%d %u %d %d %d %d %d %d %u\\n", VR_ENOSPC, VR_EDT_NONE, VR_EDT_TO_SET, VR_EDT_TO_UNSET, ' \
           'VR_MORPH_DILATE, VR_MORPH_ERODE, VR_MORPH_OPEN, VR_MORPH_CLOSE, VR_MORPH_MAX_EXTENT); return 0; }\n'
    tmp = str(tmp_path / "vr_morph_layout")
    with open(tmp + ".c", "w") as f:
        f.write(test)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), tmp + ".c", "-o", tmp], check=True)
    out = [int(x) for x in subprocess.run([tmp], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for s, fs in fields.items():
        T = getattr(vr_amd, s)
        want += [C.sizeof(T)] + [getattr(T, f).offset for f in fs]
    assert out == want + [-28, vr_amd.EDT_NONE, vr_amd.EDT_TO_SET, vr_amd.EDT_TO_UNSET, vr_amd.MORPH_DILATE,
                          vr_amd.MORPH_ERODE, vr_amd.MORPH_OPEN, vr_amd.MORPH_CLOSE, vr_amd.MORPH_MAX_EXTENT]
    assert [C.sizeof(getattr(vr_amd, s)) for s in fields] == [24, 24]


def test_argument_errors_without_a_device():
    """Everything a NULL context refuses: -22, the outputs untouched."""
    L = vr_amd.morph_lib()
    ei, mi = vr_amd.vr_edt_info(), vr_amd.vr_morph_info()
    C.memset(C.byref(ei), 0x77, 24)
    C.memset(C.byref(mi), 0x77, 24)
    ext = (C.c_uint32 * 3)(2, 2, 1)
    mask = np.full(4, 1, np.uint8)
    dist = np.full(4, 0x77777777, np.uint32)
    out = np.full(4, 0x77, np.uint8)
    for t in (0, 1, 2):
        assert L.vr_edt_squared(None, ext, mask.ctypes.data, 1, t, dist.ctypes.data, 4, C.byref(ei)) == -22
        assert L.vr_edt_squared_device(None, ext, mask.ctypes.data, 1, t, dist.ctypes.data, 4, C.byref(ei), None) == -22
    assert b"NULL" in vr_amd.lib().vr_last_error(None)  # the message is the first library's, as every family's
    for op in (0, 1, 2, 3, 4):
        assert L.vr_mask_morph(None, ext, op, 1, mask.ctypes.data, 1, out.ctypes.data, 4, C.byref(mi)) == -22
        assert L.vr_mask_morph_device(None, ext, op, 1, mask.ctypes.data, 1, out.ctypes.data, 4, C.byref(mi), None) == -22
    assert L.vr_edt_squared(None, ext, mask.ctypes.data, 1, 0, dist.ctypes.data, 3, C.byref(ei)) == -22  # (not -28)
    assert L.vr_mask_morph(None, ext, 0, 0xFFFFFFFF, mask.ctypes.data, 1, out.ctypes.data, 4, C.byref(mi)) == -22
    assert L.vr_edt_squared(None, None, None, 0, 0, None, 0, None) == -22
    assert L.vr_edt_squared_device(None, None, None, 0, 0, None, 0, None, None) == -22
    assert L.vr_mask_morph(None, None, 0, 0, None, 0, None, 0, None) == -22
    assert L.vr_mask_morph_device(None, None, 0, 0, None, 0, None, 0, None, None) == -22
    assert L.vr_morph_last_kernel_name(None) == b""
    assert bytes(ei) == b"\x77" * 24 and bytes(mi) == b"\x77" * 24
    assert np.all(dist == 0x77777777) and np.all(out == 0x77) and np.all(mask == 1)


# ---- the host helper header, stand-alone, under AddressSanitizer + UBSan ---------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ missing")
def test_host_helpers_under_sanitizers(tmp_path):
    """Every refusal that needs no device, -22 and -28 alike, on csrc/vr_morph_host.h itself (the
    library's entry points refuse a NULL context before they reach it)."""
    stdout = run_sanitized(tmp_path, "morph")
    # the grid rule and the tiling, restated here
    seen = refused = 0
    for line in stdout.splitlines():
        w = line.replace(":", " ").split()
        if w[0] != "grid":
            continue
        ext = [int(x) for x in w[1:4]]
        ok, voxels = int(w[4]), int(w[5])
        n = ext[0] * ext[1] * ext[2]
        want = all(1 <= e <= 32768 for e in ext) and n <= 2 ** 32 - 1
        assert ok == int(want), line
        refused += not want
        if ok:
            assert voxels == n, line
            for axis, (wd, tiles) in ((1, (int(w[6]), int(w[7]))), (2, (int(w[8]), int(w[9])))):
                col = ext[axis]
                words = 32768 if col > 16384 else 16384
                assert wd == max(v for v in (1, 2, 4, 8, 16, 32, 64) if v * col <= words), line
                line_len, slabs = (ext[0], ext[2]) if axis == 1 else (ext[0] * ext[1], 1)
                assert tiles == slabs * -(-line_len // wd), line
        seen += 1
    assert seen == 31 and refused == 11
