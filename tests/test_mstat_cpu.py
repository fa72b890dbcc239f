"""CPU: the volume under a mask or a label array (include/vr/vr_mstat.h) -- the reference
tests/mstat_ref.py pinned against a voxel-by-voxel restatement, np.bincount and scipy.ndimage; the
scenes hold what they are for; the fourth library's symbols and structs; the refusals that
need no device; and the host helper header under AddressSanitizer + UBSan in a stand-alone program
(the kernels of every library: tests/test_kernel_inventory_cpu.py).  No GPU: nothing here creates a
context."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import edge_shapes as E
import hist_ref
import label_ref
import label_scenes
import mstat_ref as R
import mstat_scenes as S
import vr_amd
from harness import run_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ---- the reference, pinned before anything is compared with it ------------------------------------------
def slow_region(v, lab, label, int_storage):
    """One record, voxel by voxel, with exact rational sums."""
    r = R.empty_records([label])[0]
    s = s2 = Fraction(0)
    special = []
    for l in range(v.size):
        if lab[l] != label:
            continue
        r["voxels"] += 1
        f = v[l]
        if f != f:
            r["nan"] += 1
            continue
        if r["min_index"] == R.NONE or f < r["vmin"]:
            r["vmin"], r["min_index"] = f, l
        if r["max_index"] == R.NONE or f > r["vmax"]:
            r["vmax"], r["max_index"] = f, l
        if math.isinf(f):
            special.append(float(f))
        else:
            s += Fraction(float(f))
            s2 += Fraction(float(f)) ** 2
    if special:
        r["sum"] = sum(special)  # +-inf, or NaN for opposite ones
        r["sum2"] = float("inf")
    else:
        r["sum"], r["sum2"] = float(s), float(s2)  # (Fraction -> float rounds once, as fsum does)
    return r


def test_reference_equals_a_voxel_by_voxel_restatement():
    v, lab = S.specials()
    table = list(S.SPECIAL_TABLE)
    got, info = R.regions(v, lab, table, False)
    for i, label in enumerate(table):
        want = slow_region(v.reshape(-1), lab.reshape(-1), label, False)
        a, b = R.normalised(got[i:i + 1]), R.normalised(want)
        if math.isnan(want["sum"]):
            assert math.isnan(got[i]["sum"]) and got[i]["sum2"] == math.inf
            a["sum"] = b["sum"] = 0.0
        assert a.tobytes() == b.tobytes(), (label, got[i], want)
    assert info == {"voxels": v.size, "set": int((lab != 0).sum()), "unlisted": int((lab == S.UNLISTED).sum()),
                    "regions": len(table)}
    # integer storage, a box of the noise volume: the labels of a window
    vol = E.box_volume("plain8")
    box = ((5, 5, 5), (14, 12, 9))
    labels, rec, linfo = label_ref.label(vol, 50.0, 100.0, 6, box)
    sub = R.crop(vol, box[0], labels.shape)
    got, info = R.regions(sub, labels, rec["label"], True)
    for i in range(0, len(rec), 3):
        want = slow_region(sub.reshape(-1), labels.reshape(-1), rec["label"][i], True)
        assert R.same_records(got[i:i + 1], want)
    assert np.array_equal(got["voxels"], rec["voxels"]) and info["unlisted"] == 0 and info["set"] == linfo["in_voxels"]


def test_reference_equals_bincount_and_scipy():
    vol = label_scenes.noise()
    labels, rec, linfo = label_scenes.reference("noise", 0.3, 0.6, 6)
    got, info = R.regions(vol, labels, rec["label"], False)
    lab = labels.reshape(-1)
    d = vol.reshape(-1).astype(np.float64)
    inv = np.searchsorted(rec["label"], lab[lab != 0])
    assert np.array_equal(got["voxels"], np.bincount(inv, minlength=len(rec)))
    assert np.array_equal(got["voxels"], rec["voxels"]) and not got["nan"].any()
    s = np.bincount(inv, weights=d[lab != 0], minlength=len(rec))
    s2 = np.bincount(inv, weights=d[lab != 0] ** 2, minlength=len(rec))
    assert np.allclose(got["sum"], s, rtol=1e-13, atol=0) and np.allclose(got["sum2"], s2, rtol=1e-13, atol=0)
    ndi = pytest.importorskip("scipy.ndimage")
    idx = rec["label"]
    assert np.array_equal(got["vmin"], ndi.minimum(vol, labels, idx).astype(F))
    assert np.array_equal(got["vmax"], ndi.maximum(vol, labels, idx).astype(F))
    lin = lambda pos: np.array([np.ravel_multi_index(p, vol.shape) for p in pos], np.uint32)
    assert np.array_equal(got["min_index"], lin(ndi.minimum_position(vol, labels, idx)))
    assert np.array_equal(got["max_index"], lin(ndi.maximum_position(vol, labels, idx)))


def test_reference_mask_and_window():
    vol = E.box_volume("plain8")
    m = S.byte_mask(vol.shape)
    rec, bins, hinfo = R.mask_stats(vol, m, True, (16, 10.0, 80.0))
    sel = vol[m != 0]
    assert rec["label"] == 1 and rec["voxels"] == hinfo["voxels"] == int(m.sum()) and rec["nan"] == hinfo["nan"] == 0
    assert rec["sum"] == float(sel.astype(np.int64).sum()) and rec["sum2"] == float((sel.astype(np.int64) ** 2).sum())
    assert rec["vmin"] == hinfo["vmin"] == sel.min() and rec["vmax"] == hinfo["vmax"] == sel.max()
    assert vol.reshape(-1)[rec["min_index"]] == sel.min() and not (vol.reshape(-1)[:rec["min_index"]][m.reshape(-1)[:rec["min_index"]] != 0] == sel.min()).any()
    assert int(bins.sum()) + hinfo["below"] + hinfo["above"] == int(m.sum()) and hinfo["below"] > 0 < hinfo["above"]
    assert np.array_equal(bins, hist_ref.histogram(sel, 10.0, 80.0, 16)[0])
    out, info = R.window(vol, m, 20.0, 50.0)
    assert np.array_equal(out != 0, (m != 0) & (vol >= 20) & (vol <= 50)) and info["in_set"] == int(m.sum())
    out, info = R.window(vol, None, 20.0, 50.0)
    assert info["in_set"] == vol.size and info["out_set"] == int(((vol >= 20) & (vol <= 50)).sum())
    # the bound: n and A alone
    v = np.array([1.5, -2.25, np.nan, 3.0], F)
    assert R.sum_bounds(v) == (2 * 2.0 ** -52 * 6.75, 2 * 2.0 ** -52 * (2.25 + 5.0625 + 9.0))
    assert R.sum_bounds(v[:1]) == (0.0, 0.0)


def test_the_scenes_hold_what_they_are_for():
    # a label crossing every seam voxel, in both geometries: the 26-connected window of the box volume
    for layout in E.BOX_LAYOUTS:
        labels, rec, info = E.box_label_reference(layout, E.WHOLE, 26)
        for a in range(3):
            for s in E.seams(E.BOX_DIMS[a], E.geometry(layout)[a]):
                assert E.crossing(labels, a, s) >= 1, (layout, a, s)
    v, lab = S.specials()
    assert v.shape == S.SPECIAL_DIMS[::-1] and v.dtype == F
    assert np.isnan(v).sum() == 15 and np.isposinf(v).sum() == 2 and np.isneginf(v).sum() == 1
    assert np.signbit(v[v == 0]).sum() == 3 and (v == S.DENORMAL).sum() == 1 and 0 < S.DENORMAL < np.finfo(F).tiny
    rec, info = R.regions(v, lab, S.SPECIAL_TABLE, False)
    r = {int(x["label"]): x for x in rec}
    assert r[8]["voxels"] == 0 and r[8]["min_index"] == R.NONE and r[8]["vmin"] == np.inf and r[8]["sum"] == 0.0  # empty
    assert info["unlisted"] == 9 and info["set"] == int((lab != 0).sum()) and info["regions"] == 10
    assert r[45]["voxels"] == 2 and r[45]["sum"] == 0.0 and not np.signbit(r[45]["sum"]) and not np.signbit(r[45]["sum2"])
    assert r[3]["voxels"] == 16 and r[7]["nan"] == 2 and r[7]["voxels"] == 11
    assert r[20]["voxels"] == r[20]["nan"] == 13 and r[20]["max_index"] == R.NONE and r[20]["vmax"] == -np.inf
    assert math.isnan(r[21]["sum"]) and r[21]["vmax"] == np.inf and r[21]["vmin"] == -np.inf and r[21]["sum2"] == np.inf
    assert r[30]["vmax"] == np.inf == r[30]["sum"] and abs(r[30]["vmin"]) < 1
    z = r[40]  # -0.0 == 0: both extremes at the first voxel, which holds the -0.0
    assert z["vmin"] == z["vmax"] == 0 and z["min_index"] == z["max_index"] == np.ravel_multi_index((2, 1, 3), v.shape)
    t = r[50]  # a tie for each extreme goes to the smaller index
    assert t["vmax"] == F(0.95) and t["max_index"] == np.ravel_multi_index((2, 3, 4), v.shape)
    assert t["vmin"] == F(-0.95) and t["min_index"] == np.ravel_multi_index((2, 3, 2), v.shape)
    assert r[60]["vmax"] == S.DENORMAL and r[60]["sum"] == float(S.DENORMAL) and r[60]["sum2"] == float(S.DENORMAL) ** 2 > 0
    # the arrays
    w = S.word_mask((5, 6, 7))
    assert w.dtype == np.uint32 and w[w != 0].min() >= 2 and 0 < (w != 0).mean() < 1
    assert (w[w != 0] & 0xFF == 0).any()  # an element whose first byte is zero is set
    for layout, (dtype, knobs, storage, tag, add) in S.LAYOUTS.items():
        vol = S.volume((5, 11, 15), layout)
        assert np.array_equal(vol.astype(dtype).astype(F), vol) and (vol.min() < 0) == (add < 0)
    assert set(E.LAYOUTS) < set(S.LAYOUTS) and all(S.LAYOUTS[k][:3] == E.LAYOUTS[k][:3] for k in E.LAYOUTS)
    # beyond one workgroup
    c = S.checker_labels()
    n = int((c != 0).sum())
    assert c.shape == S.BIG_DIMS[::-1] and 150000 < n == np.unique(c[c != 0]).size
    assert np.array_equal(c, label_ref.label_array(label_scenes.checker(S.BIG_DIMS, np.uint8) != 0, 6))
    u = S.big_volume("u16")
    assert u.min() == 0 and u.max() == 65535 and float((u.astype(np.int64) ** 2).sum()) > 2.0 ** 48
    f = S.big_volume("f32")
    assert (f != np.rint(f)).mean() > 0.99 and f.min() < -3000 and f.max() > 3000
    bx, by, bz = S.BIG_DIMS
    assert -(-bx // 64) * -(-by // 4) * bz > 1 and bx % 64 and by % 4


def test_the_thin_grid_makes_a_workgroup_walk_many_tiles():
    """More tiles than a launch has workgroups, and on its labels a lane of the label pass meets every
    case of its rule: it merges, sends the smaller part on, and replaces what it keeps."""
    bx, by, bz = S.THIN_DIMS
    lab = S.thin_labels()
    assert lab.shape == (bz, by, bx) and lab.dtype == np.uint32
    assert all(o + e <= d for o, e, d in zip(S.THIN_ORIGIN, S.THIN_DIMS, S.THIN_VOLUME_DIMS))
    ev = S.lane_events(lab)
    print(ev)
    assert ev["tiles"] == 36000 > 8 * S.MAX_GRID and ev["most_tiles_a_workgroup"] == 9
    assert min(ev["first"], ev["merge"], ev["flush_smaller"], ev["replace"]) > 100, ev
    assert list(S.table_of(lab)["label"]) == [1, 2, 3, 4, 5, 9] and (lab == 0).sum() == 100 * bx * by
    # the other grids of the suite never reach those cases: every workgroup walks one tile
    ev = S.lane_events(S.checker_labels(), step=1)
    assert ev["tiles"] < S.MAX_GRID and ev["merge"] == ev["flush_smaller"] == ev["replace"] == 0
    src = open(os.path.join(ROOT, "volumetric-renderer_amd", "csrc", "vr_mstat_host.h")).read()
    assert re.search(r"kMstatMaxGrid = %d;" % S.MAX_GRID, src) and "kMstatTileX = 64, kMstatTileY = 4;" in src


# ---- the binding ---------------------------------------------------------------------------------------
def test_every_declared_name_is_exported_and_listed():
    src = open(os.path.join(ROOT, "include", "vr", "vr_mstat.h")).read()
    for h in ("vr_hist.h", "vr_label.h", "vr_mesh.h", "vr_morph.h"):
        assert f'#include "{h}"' in src
    assert "#define VR_ENOSPC" not in src and "typedef struct vr_morph_info" not in src  # reused, not redefined
    assert "2^-52" in src  # the bound on the f32 sums is the header's
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b(vr_[a-z0-9_]+)\s*\(", src))
    assert names == set(vr_amd.MSTAT_SYMBOLS) and len(names) == 7
    assert os.path.dirname(vr_amd.MSTAT_LIB_PATH) == os.path.dirname(vr_amd.LIB_PATH)
    nm = lambda path: {l.split()[-1] for l in subprocess.run(
        ["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout.splitlines()
        if " T " in l}
    assert not names - nm(vr_amd.MSTAT_LIB_PATH)
    for other in (vr_amd.LIB_PATH, vr_amd.MORPH_LIB_PATH, vr_amd.MASKCC_LIB_PATH):  # the other three hold none
        assert not names & nm(other)
    L = vr_amd.mstat_lib()
    assert all(getattr(L, n).argtypes is not None for n in names)
    assert vr_amd.ABI_VERSION == 9 and vr_amd.lib().vr_abi_version() == 9  # an addition: the ABI stays
    for m in ("mask_stats", "mask_stats_device", "label_stats", "label_stats_device", "mask_window",
              "mask_window_device", "mstat_last_kernel_name"):
        assert callable(getattr(vr_amd.OffscreenPass, m))
    # the fourth library takes the scaffold from the first, found beside it, and nothing from its siblings
    dyn = subprocess.run(["readelf", "-d", vr_amd.MSTAT_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libvr_amd.so" in dyn and "$ORIGIN" in dyn and "libvr_amd_morph" not in dyn and "libvr_amd_maskcc" not in dyn


def test_struct_layouts_match_header(tmp_path):
    fields = {"vr_mstat_region": ["label", "reserved", "voxels", "nan", "vmin", "vmax", "min_index", "max_index",
                                  "sum", "sum2", "reserved2"],
              "vr_mstat_info": ["voxels", "set", "unlisted", "regions"]}
    body = "".join(f'  printf("%zu ", sizeof({s}));\n' +
                   "".join(f'  printf("%zu ", offsetof({s}, {f}));\n' for f in fs) for s, fs in fields.items())
    test = '#include "vr/vr_mstat.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n' + body + \
           '  printf("%zu %zu %zu %d %u %u\\n", sizeof(vr_label_component), sizeof(vr_morph_info), ' \
           'sizeof(vr_hist_info), VR_ENOSPC, VR_MSTAT_NONE, VR_MSTAT_MAX_EXTENT); return 0; }\n'
    tmp = str(tmp_path / "vr_mstat_layout")
    with open(tmp + ".c", "w") as f:
        f.write(test)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), tmp + ".c", "-o", tmp], check=True)
    out = [int(x) for x in subprocess.run([tmp], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for s, fs in fields.items():
        T = getattr(vr_amd, s)
        want += [C.sizeof(T)] + [getattr(T, f).offset for f in fs]
    assert out == want + [64, 24, 40, -28, vr_amd.MSTAT_NONE, vr_amd.MSTAT_MAX_EXTENT]
    assert [C.sizeof(getattr(vr_amd, s)) for s in fields] == [64, 32]
    # the numpy record is the structure, and the reference's
    D = vr_amd.MSTAT_REGION_DTYPE
    assert D == R.REGION_DTYPE and D.itemsize == 64
    assert [D.fields[f][1] for f in fields["vr_mstat_region"]] == [getattr(vr_amd.vr_mstat_region, f).offset
                                                                   for f in fields["vr_mstat_region"]]
    assert R.NONE == vr_amd.MSTAT_NONE == 0xFFFFFFFF


def test_argument_errors_without_a_device():
    """Everything a NULL context refuses: -22, the outputs and infos untouched."""
    L = vr_amd.mstat_lib()
    reg, mi, wi, hi = vr_amd.vr_mstat_region(), vr_amd.vr_mstat_info(), vr_amd.vr_morph_info(), vr_amd.vr_hist_info()
    for s, n in ((reg, 64), (mi, 32), (wi, 24), (hi, 40)):
        C.memset(C.byref(s), 0x77, n)
    ext, org = (C.c_uint32 * 3)(2, 2, 1), (C.c_uint32 * 3)(0, 0, 0)
    mask = np.full(4, 1, np.uint8)
    labels = np.full(4, 3, np.uint32)
    table = np.zeros(1, vr_amd.LABEL_COMPONENT_DTYPE)
    table["label"] = 3
    regs = np.full(64, 0x77, np.uint8)
    out = np.full(4, 0x77, np.uint8)
    bins = np.full(8, 0x7777777777777777, np.uint64)
    req = vr_amd.vr_hist_request()
    req.lo, req.hi, req.nbins = 0.0, 1.0, 8
    assert L.vr_mask_stats(None, ext, org, mask.ctypes.data, 1, None, None, None, C.byref(reg)) == -22
    assert b"NULL" in vr_amd.lib().vr_last_error(None)  # the message is the first library's, as every family's
    assert L.vr_mask_stats(None, ext, org, mask.ctypes.data, 1, C.byref(req), bins.ctypes.data, C.byref(hi),
                           C.byref(reg)) == -22
    assert L.vr_mask_stats_device(None, ext, org, mask.ctypes.data, 1, C.byref(req), bins.ctypes.data, C.byref(hi),
                                  C.byref(reg), None) == -22
    assert L.vr_label_stats(None, ext, org, labels.ctypes.data, table.ctypes.data, 1, regs.ctypes.data, 1, C.byref(mi)) == -22
    assert L.vr_label_stats(None, ext, org, labels.ctypes.data, table.ctypes.data, 1, regs.ctypes.data, 0,
                            C.byref(mi)) == -22  # (not -28)
    assert L.vr_label_stats_device(None, ext, org, labels.ctypes.data, table.ctypes.data, 1, regs.ctypes.data, 1,
                                   C.byref(mi), None) == -22
    assert L.vr_mask_window(None, ext, org, mask.ctypes.data, 1, 0.0, 1.0, out.ctypes.data, 4, C.byref(wi)) == -22
    assert L.vr_mask_window(None, ext, org, None, 1, 0.0, 1.0, out.ctypes.data, 3, C.byref(wi)) == -22  # (not -28)
    assert L.vr_mask_window_device(None, ext, org, mask.ctypes.data, 1, 0.0, 1.0, out.ctypes.data, 4, C.byref(wi), None) == -22
    assert L.vr_mask_stats(None, None, None, None, 0, None, None, None, None) == -22
    assert L.vr_mask_stats_device(None, None, None, None, 0, None, None, None, None, None) == -22
    assert L.vr_label_stats(None, None, None, None, None, 0, None, 0, None) == -22
    assert L.vr_label_stats_device(None, None, None, None, None, 0, None, 0, None, None) == -22
    assert L.vr_mask_window(None, None, None, None, 0, 0.0, 0.0, None, 0, None) == -22
    assert L.vr_mask_window_device(None, None, None, None, 0, 0.0, 0.0, None, 0, None, None) == -22
    assert L.vr_mstat_last_kernel_name(None) == b""
    assert bytes(reg) == b"\x77" * 64 and bytes(mi) == b"\x77" * 32 and bytes(wi) == b"\x77" * 24 and bytes(hi) == b"\x77" * 40
    assert np.all(regs == 0x77) and np.all(out == 0x77) and np.all(bins == 0x7777777777777777)
    assert np.all(mask == 1) and np.all(labels == 3)


# ---- the host helper header, stand-alone, under AddressSanitizer + UBSan ---------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ missing")
def test_host_helpers_under_sanitizers(tmp_path):
    """Every refusal that needs no device, -22 and -28 alike, the launch geometry and the brick
    addressing the kernels share, on csrc/vr_mstat_host.h itself (the library's entry points refuse a
    NULL context before they reach it)."""
    stdout = run_sanitized(tmp_path, "mstat")
    # the four geometries over the extents 1 .. 15 per axis: (1 + .. + 15)^3 voxels each
    assert f"addressing {4 * 120 ** 3} voxels" in stdout
    # the grid rule and the geometry, restated here
    seen = refused = 0
    for line in stdout.splitlines():
        w = line.replace(":", " ").split()
        if w[0] != "grid":
            continue
        ext = [int(x) for x in w[1:4]]
        nrec, ok, voxels = int(w[4]), int(w[5]), int(w[6])
        n = ext[0] * ext[1] * ext[2]
        want = all(1 <= e <= 32768 for e in ext) and n <= 2 ** 32 - 1
        assert ok == int(want), line
        refused += not want
        if ok:
            assert voxels == n, line
            tiles_x, tiles_y, tiles, grid, rec_grid, nbytes = (int(x) for x in w[7:13])
            assert tiles_x == -(-ext[0] // 64) and tiles_y == -(-ext[1] // 4) and tiles == tiles_x * tiles_y * ext[2], line
            assert grid == min(tiles, 4096) and rec_grid == min(max(-(-nrec // 256), 1), 4096), line
            assert nbytes == 64 + 4096 * 12 + nrec * 116, line  # 48 KiB and 116 bytes a record
        seen += 1
    assert seen == 38 and refused == 11
