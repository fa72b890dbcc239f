"""CPU: the components of a mask (include/vr/vr_maskcc.h) -- the reference tests/maskcc_ref.py pinned
against a breadth-first search and against scipy; the scenes hold what they are for; the third
library's symbols and structs; the refusals that need no device; and the host helper header
under AddressSanitizer + UBSan in a stand-alone program (the kernels of every library:
tests/test_kernel_inventory_cpu.py).  No GPU: nothing here creates a context."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import label_ref
import maskcc_ref as R
import maskcc_scenes as S
import vr_amd
from harness import run_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def structure(connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    return ndi.generate_binary_structure(3, 1 if connectivity == 6 else 3)


# ---- the reference, pinned before anything is compared with it ------------------------------------------
@pytest.mark.parametrize("name", S.SMALL)
def test_reference_equals_a_breadth_first_search(name):
    m = S.mask(name) != 0
    for conn in (6, 26):
        labels, rec, info = S.reference_label(name, conn)
        assert labels.dtype == np.uint32 and np.array_equal(labels, label_ref.bfs_label(m, conn)), (name, conn)
        assert info["voxels"] == m.size and info["in_voxels"] == int(m.sum()) == int(rec["voxels"].sum())
        assert np.array_equal(rec["label"], np.unique(labels[labels != 0])) and not rec["reserved"].any()
        # the complement, which hole filling labels
        assert np.array_equal(S.reference_label(name, conn, True)[0], label_ref.bfs_label(~m, conn)), (name, conn)


@pytest.mark.parametrize("name", S.NAMES)
def test_reference_counts_equal_scipy(name):
    ndi = pytest.importorskip("scipy.ndimage")
    m = S.mask(name) != 0
    assert m.shape == S.shape(name)[::-1]
    for conn in (6, 26):
        labels, rec, info = S.reference_label(name, conn)
        got, count = ndi.label(m, structure=structure(conn))
        assert count == info["components"] == len(rec), (name, conn)
        # the same partition: scipy's label is constant on each of ours, and there are as many
        assert np.array_equal(got != 0, labels != 0)
        pairs = np.unique(np.stack([labels[m].astype(np.int64), got[m].astype(np.int64)]), axis=1)
        assert pairs.shape[1] == count


@pytest.mark.parametrize("name", S.FILL)
def test_reference_fill_equals_scipy(name):
    ndi = pytest.importorskip("scipy.ndimage")
    m = S.mask(name) != 0
    for conn in (6, 26):
        out, info = S.reference_select(name, R.FILL_HOLES, conn)
        want = ndi.binary_fill_holes(m, structure=structure(conn))
        assert out.dtype == np.uint8 and out.tobytes() == want.astype(np.uint8).tobytes(), (name, conn)
        assert info["in_set"] == int(m.sum()) and info["out_set"] == int(want.sum())
        # a hole is exactly a record whose bounding box touches no face: selection is a function of the records
        labels, rec, linfo = S.reference_label(name, conn, True)
        holes = R.holes_from_records(rec, m.shape)
        assert info["kept"] == holes.size and info["components"] == linfo["components"]
        assert np.array_equal(out != 0, m | np.isin(labels, holes))


def test_the_scenes_hold_what_they_are_for():
    comps = lambda name, conn: S.reference_label(name, conn)[2]["components"]
    for n in S.ROW_LENGTHS:
        assert S.shape(f"row{n}") == (n, 4, 2)
    m = S.mask("row129")[0]
    assert m[0, 60:64].all() and not m[0, 64] and m[1, 64:71].all() and not m[1, 63] and m[2, 62:67].all() and m[3].all()
    for name in ("diag_y", "diag_zy", "diag_yz", "diag_z", "corner_pair"):  # touching by a diagonal alone
        assert (comps(name, 6), comps(name, 26)) == (2, 1), name
    for name in ("diag_y", "diag_zy", "diag_yz", "diag_z"):  # ... across the word boundary
        xs = np.nonzero(S.mask(name))[2]
        assert {63, 64} <= set(xs.tolist())
    assert [S.shape(n) for n in ("line_x", "line_y", "line_z")] == [(257, 1, 1), (1, 300, 1), (1, 1, 257)]
    assert not S.mask("none").any() and S.mask("all").all()
    assert S.shape("corner_pair") == (2, 2, 2) and S.shape("checker") == (17, 9, 5)
    n = int(S.mask("checker").sum())
    assert comps("checker", 6) == n > 64 and comps("checker", 26) == 1
    for name in ("pillars", "comb", "serpentine", "spiral"):  # one component, merged late
        assert comps(name, 6) == comps(name, 26) == 1, name
    p = np.array(S.mask("pillars"))
    p[5, 19, 1:8] = 0
    p[5, 19, 1] = p[5, 19, 7] = 1
    assert label_ref.table(label_ref.label_array(p != 0, 26))[1]["components"] == 2  # the bar alone joins them
    assert int((S.mask("comb")[0, 0] != 0).sum()) == 40
    assert S.shape("serpentine") == (130, 33, 4) and S.shape("spiral") == (65, 65, 1)
    s = np.array(S.mask("serpentine"))
    s[0, 16, 64] = 0  # a chain: one cut, two pieces
    assert label_ref.table(label_ref.label_array(s != 0, 6))[1]["components"] == 2
    assert S.shape("chunk130") == (130, 9, 8) and 8192 < 130 * 9 * 8 < 2 * 8192 and S.shape("chunk70") == (70, 33, 19)
    assert [S.shape(n) for n in S.RANDOM] == [(64, 64, 64)] * 3 + [(128, 96, 80)]
    for name, d in zip(S.RANDOM, (0.05, 0.5, 0.95, 0.35)):
        assert abs(float(S.mask(name).mean()) - d) < 0.01
    # the holes
    for (name, conn), filled in S.FILLED.items():
        out, info = S.reference_select(name, R.FILL_HOLES, conn)
        assert info["out_set"] - info["in_set"] == filled, (name, conn)
    for conn in (6, 26):
        out, info = S.reference_select("shells", R.FILL_HOLES, conn)
        assert out[1:10, 1:10, 1:10].all() and info["out_set"] == 9 ** 3 and info["kept"] == 2  # solid
        for name in S.THIN:  # a grid with an extent of 1 has no holes
            out, info = S.reference_select(name, R.FILL_HOLES, conn)
            assert info["kept"] == 0 and out.tobytes() == S.mask(name).tobytes()
    # a tie for the largest goes to the smallest label
    out, info = S.reference_select("checker", R.KEEP_LARGEST, 6)
    assert info["kept"] == 1 and info["out_set"] == 1 and out.reshape(-1)[0] == 1


# ---- the binding ---------------------------------------------------------------------------------------
def test_every_declared_name_is_exported_and_listed():
    src = open(os.path.join(ROOT, "include", "vr", "vr_maskcc.h")).read()
    assert '#include "vr_label.h"' in src and '#include "vr_mesh.h"' in src
    assert "#define VR_ENOSPC" not in src and "typedef struct vr_label_component" not in src  # reused, not redefined
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b(vr_[a-z0-9_]+)\s*\(", src))
    assert names == set(vr_amd.MASKCC_SYMBOLS) and len(names) == 5
    assert os.path.dirname(vr_amd.MASKCC_LIB_PATH) == os.path.dirname(vr_amd.LIB_PATH)
    nm = lambda path: {l.split()[-1] for l in subprocess.run(
        ["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout.splitlines()
        if " T " in l}
    assert not names - nm(vr_amd.MASKCC_LIB_PATH)
    assert not names & nm(vr_amd.LIB_PATH) and not names & nm(vr_amd.MORPH_LIB_PATH)  # the other two hold none
    L = vr_amd.maskcc_lib()
    assert all(getattr(L, n).argtypes is not None for n in names)
    assert vr_amd.ABI_VERSION == 9 and vr_amd.lib().vr_abi_version() == 9  # an addition: the ABI stays
    for m in ("mask_label", "mask_label_device", "mask_select", "mask_select_device", "maskcc_last_kernel_name"):
        assert callable(getattr(vr_amd.OffscreenPass, m))
    # the third library takes the scaffold from the first, found beside it
    dyn = subprocess.run(["readelf", "-d", vr_amd.MASKCC_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libvr_amd.so" in dyn and "$ORIGIN" in dyn and "libvr_amd_morph" not in dyn


def test_struct_layouts_match_header(tmp_path):
    fields = {"vr_mask_select_request": ["rule", "connectivity", "min_voxels", "seed", "reserved"],
              "vr_mask_select_info": ["voxels", "in_set", "out_set", "components", "kept"]}
    body = "".join(f'  printf("%zu ", sizeof({s}));\n' +
                   "".join(f'  printf("%zu ", offsetof({s}, {f}));\n' for f in fs) for s, fs in fields.items())
    test = '#include "vr/vr_maskcc.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n' + body + \
           '  printf("%zu %zu %d %d %d %d %d %u\\n", sizeof(vr_label_component), sizeof(vr_label_info), VR_ENOSPC, ' \
           'VR_MASK_KEEP_LARGEST, VR_MASK_KEEP_MIN_VOXELS, VR_MASK_KEEP_SEED, VR_MASK_FILL_HOLES, ' \
           'VR_MASKCC_MAX_EXTENT); return 0; }\n'
    tmp = str(tmp_path / "vr_maskcc_layout")
    with open(tmp + ".c", "w") as f:
        f.write(test)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), tmp + ".c", "-o", tmp], check=True)
    out = [int(x) for x in subprocess.run([tmp], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for s, fs in fields.items():
        T = getattr(vr_amd, s)
        want += [C.sizeof(T)] + [getattr(T, f).offset for f in fs]
    assert out == want + [C.sizeof(vr_amd.vr_label_component), C.sizeof(vr_amd.vr_label_info), -28,
                          vr_amd.MASK_KEEP_LARGEST, vr_amd.MASK_KEEP_MIN_VOXELS, vr_amd.MASK_KEEP_SEED,
                          vr_amd.MASK_FILL_HOLES, vr_amd.MASKCC_MAX_EXTENT]
    assert [C.sizeof(getattr(vr_amd, s)) for s in fields] == [32, 40]
    assert (R.KEEP_LARGEST, R.KEEP_MIN_VOXELS, R.KEEP_SEED, R.FILL_HOLES) == (0, 1, 2, 3)


def test_argument_errors_without_a_device():
    """Everything a NULL context refuses: -22, the outputs and infos untouched."""
    L = vr_amd.maskcc_lib()
    li, si = vr_amd.vr_label_info(), vr_amd.vr_mask_select_info()
    C.memset(C.byref(li), 0x77, 40)
    C.memset(C.byref(si), 0x77, 40)
    ext = (C.c_uint32 * 3)(2, 2, 1)
    mask = np.full(4, 1, np.uint8)
    labels = np.full(4, 0x77777777, np.uint32)
    comps = np.full(4 * 64, 0x77, np.uint8)
    out = np.full(4, 0x77, np.uint8)
    for conn in (6, 26, 7):
        assert L.vr_mask_label(None, ext, mask.ctypes.data, 1, conn, labels.ctypes.data, 4, comps.ctypes.data, 4,
                               C.byref(li)) == -22
        assert L.vr_mask_label_device(None, ext, mask.ctypes.data, 1, conn, labels.ctypes.data, 4, comps.ctypes.data,
                                      4, C.byref(li), None) == -22
    assert b"NULL" in vr_amd.lib().vr_last_error(None)  # the message is the first library's, as every family's
    for rule in (0, 1, 2, 3, 4):
        req = vr_amd.mask_select_request(rule, 6, 1, (1, 1, 0))
        assert L.vr_mask_select(None, ext, C.byref(req), mask.ctypes.data, 1, out.ctypes.data, 4, C.byref(si)) == -22
        assert L.vr_mask_select_device(None, ext, C.byref(req), mask.ctypes.data, 1, out.ctypes.data, 4, C.byref(si),
                                       None) == -22
    req = vr_amd.mask_select_request(0)
    assert L.vr_mask_label(None, ext, mask.ctypes.data, 1, 6, labels.ctypes.data, 3, comps.ctypes.data, 4,
                           C.byref(li)) == -22  # (not -28)
    assert L.vr_mask_select(None, ext, C.byref(req), mask.ctypes.data, 1, out.ctypes.data, 3, C.byref(si)) == -22
    assert L.vr_mask_label(None, None, None, 0, 0, None, 0, None, 0, None) == -22
    assert L.vr_mask_label_device(None, None, None, 0, 0, None, 0, None, 0, None, None) == -22
    assert L.vr_mask_select(None, None, None, None, 0, None, 0, None) == -22
    assert L.vr_mask_select_device(None, None, None, None, 0, None, 0, None, None) == -22
    assert L.vr_maskcc_last_kernel_name(None) == b""
    assert bytes(li) == b"\x77" * 40 and bytes(si) == b"\x77" * 40
    assert np.all(labels == 0x77777777) and np.all(comps == 0x77) and np.all(out == 0x77) and np.all(mask == 1)


# ---- the host helper header, stand-alone, under AddressSanitizer + UBSan ---------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ missing")
def test_host_helpers_under_sanitizers(tmp_path):
    """Every refusal that needs no device, -22 and -28 alike, and the launch geometry, on
    csrc/vr_maskcc_host.h itself (the library's entry points refuse a NULL context before they
    reach it)."""
    stdout = run_sanitized(tmp_path, "maskcc")
    # the grid rule and the geometry, restated here
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
            rows, row_words, row_grid, nwords, nchunks, sweep_grid, nbytes = (int(x) for x in w[6:13])
            assert rows == ext[1] * ext[2] and row_words == -(-ext[0] // 64), line
            assert row_grid == min(-(-rows // 4), 8192) and sweep_grid == min(-(-n // 256), 8192), line
            assert nwords == -(-n // 64) and nchunks == -(-n // 8192), line
            assert nbytes == -(-(12 * nwords + 4 * nchunks) // 8) * 8 + 64, line  # about 3/16 byte a voxel
        seen += 1
    assert seen == 37 and refused == 11
