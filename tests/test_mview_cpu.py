"""CPU: the view of a mask or a label array (include/vr/vr_mview.h) -- the reference tests/mview_ref.py
pinned against hit_ref's ENTRY records and MAX counters, closed-form normals and a voxel-by-voxel
occupancy; the scenes hold what they are for; the fifth library's symbols and structs; the refusals
that need no device; and the host helper header under AddressSanitizer + UBSan in a stand-alone
program (the kernels and their scratch memory: tests/test_kernel_inventory_cpu.py).  No GPU: nothing here creates a context."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hit_scenes
import mpr_ref
import mview_ref as R
import mview_scenes as S
import vr_amd
from harness import run_sanitized
from range_scenes import FULL, volume

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ---- the reference, pinned before anything is compared with it ------------------------------------------
@pytest.mark.parametrize("i", range(len(hit_scenes.PARITY)))
def test_all_set_is_entry_and_all_zero_walks_the_whole_ray(i):
    """An all-set full-volume byte mask hits at the first in-slab sample: hit_ref's ENTRY pos, depth and
    step on every pixel.  An all-zero one walks every ray to its end: the steps and samples of hit_ref's
    MAX, which does the same."""
    volname = hit_scenes.PARITY[i][0]
    walk = hit_scenes.reference(*hit_scenes.PARITY[i])
    shape = volume(volname).shape
    rec, info, tr = R.hit_image(S.parity_scene(i), np.ones(shape, np.uint8))
    e = walk.records["entry"]
    assert np.array_equal(tr["covered"], walk.covered)
    for f in ("pos", "depth", "step"):
        assert np.array_equal(rec[f].view(np.uint32), e[f].view(np.uint32)), f
    hit = rec["step"] != R.MISS
    assert np.all(rec["element"][hit] == 1) and np.all(rec["element"][~hit] == 0) and np.all(rec["index"][~hit] == R.MISS)
    st = walk.stats["entry"]
    assert (info["covered"], info["hits"], info["steps"], info["samples"]) == (
        st["rays"], st["shaded_samples"], st["steps"], st["samples"])
    assert info["pixels"] == rec.size and info["voxels"] == int(np.prod(shape))
    # the index is the voxel of the position
    nz, ny, nx = shape
    v, _ = R.voxel_of(rec["pos"][hit], (nx, ny, nz))
    assert np.array_equal(rec["index"][hit], v[:, 0] + nx * (v[:, 1] + ny * v[:, 2]))
    zrec, zinfo, _ = R.hit_image(S.parity_scene(i), np.zeros(shape, np.uint8))
    assert zrec.tobytes() == R.miss_records(zrec.shape).tobytes()
    mx = walk.stats["max"]
    assert (zinfo["covered"], zinfo["hits"], zinfo["steps"], zinfo["samples"]) == (mx["rays"], 0, mx["steps"], mx["samples"])


def test_normals_in_closed_form():
    nz, ny, nx = volume("g20").shape
    half = nx // 2
    lo = np.zeros((nz, ny, nx), np.uint8)
    lo[:, :, :half] = 1  # the half space x < half: its face points to +x
    hi = (1 - lo).astype(np.uint8)
    inner = np.array([[half - 1, 5, 7], [half - 1, 1, nz - 2]])
    assert np.array_equal(R.normals(lo, (0, 0, 0), inner), [[9, 0, 0]] * 2)
    assert np.array_equal(R.normals(hi, (0, 0, 0), inner + [1, 0, 0]), [[-9, 0, 0]] * 2)
    assert np.array_equal(R.normals(lo, (0, 0, 0), np.array([[half - 1, 0, 0]])), [[4, -4, -4]])  # a corner of the volume
    # in an image: every hit on the face, away from the volume's border, has the face's normal
    for mask, want, x in ((lo, 9, half - 1), (hi, -9, half)):
        n = 0
        for i in (0, 1, 4):  # the g20 scenes: the full box sees one side, the cut box the other
            assert hit_scenes.PARITY[i][0] == "g20"
            rec, info, _ = R.hit_image(S.parity_scene(i), mask)
            h = rec[rec["step"] != R.MISS]
            g = np.stack([h["index"] % nx, h["index"] // nx % ny, h["index"] // (nx * ny)], -1).astype(int)
            face = (g[:, 0] == x) & (g[:, 1] >= 1) & (g[:, 1] <= ny - 2) & (g[:, 2] >= 1) & (g[:, 2] <= nz - 2)
            assert np.all(h["normal"][face] == (want, 0, 0))
            n += int(face.sum())
        assert n >= 30, (want, n)
    # a lone voxel has no neighbour: (0, 0, 0), and an image of it says so
    lone = np.zeros((nz, ny, nx), np.uint8)
    lone[11, 9, 10] = 1
    assert np.array_equal(R.normals(lone, (0, 0, 0), np.array([[10, 9, 11]])), [[0, 0, 0]])
    rec, info, _ = R.hit_image(S.parity_scene(0, step=None), lone)
    h = rec[rec["step"] != R.MISS]
    assert info["hits"] == len(h) >= 1 and np.all(h["normal"] == 0) and np.all(h["index"] == 10 + nx * (9 + ny * 11))
    # label selection: the neighbours that match are those of the label
    lab = np.where(lo != 0, np.uint32(7), np.uint32(256))
    assert np.array_equal(R.normals(lab, (0, 0, 0), inner, 7), [[9, 0, 0]] * 2)
    assert np.array_equal(R.normals(lab, (0, 0, 0), inner), [[0, 0, 0]] * 2)  # ANY: every neighbour is set


def test_occupancy_equals_a_voxel_by_voxel_loop():
    for ext, origin_label in ((S.GRID_EXT, None), ((9, 8, 2), None), ((33, 5, 70), 65536), ((1, 19, 17), None)):
        a = S.byte_mask(ext, 0.02) if origin_label is None else S.word_mask(ext)
        words, info, cells = R.occupancy(a, origin_label)
        bx, by, bz = ext
        c = [-(-n // 8) for n in ext]
        want = np.zeros(-(-c[0] * c[1] * c[2] // 32), np.uint32)
        n = 0
        for k in range(bz):
            for j in range(by):
                for i in range(bx):
                    e = int(a[k, j, i])
                    if (e == origin_label) if origin_label is not None else (e != 0):
                        m = i // 8 + c[0] * (j // 8 + c[1] * (k // 8))
                        want[m >> 5] |= np.uint32(1 << (m & 31))
                        n += 1
        assert np.array_equal(words, want) and words.dtype == np.uint32
        assert info == dict(voxels=bx * by * bz, cells=c[0] * c[1] * c[2], cells_set=int(sum(bin(int(w)).count("1") for w in want)),
                            matching=n)
        assert len(words) == vr_amd.mview_occupancy_words(ext) and cells.shape == (c[2], c[1], c[0])
    assert 0 < R.occupancy(S.byte_mask(S.GRID_EXT, 0.02))[1]["cells_set"] <= 45
    w, info, _ = R.occupancy(S.corner_voxel(S.GRID_EXT))
    assert list(w) == [1, 0] and info["cells_set"] == info["matching"] == 1


def test_slice_reference_on_closed_forms():
    """An axial plane whose pixels are the voxel centres of one layer shows that layer of the array."""
    nx, ny, nz = S.GRID_VOLUME
    a = S.word_mask(S.GRID_EXT)
    k = 9
    pl = mpr_ref.axis_plane(2, (k + 0.5) / nz, nx, ny)
    img, info = R.slice_image(S.GRID_VOLUME, a, pl, origin=S.GRID_ORIGIN)
    want = np.zeros((ny, nx), np.uint32)
    ox, oy, oz = S.GRID_ORIGIN
    want[oy:oy + S.GRID_EXT[1], ox:ox + S.GRID_EXT[0]] = a[k - oz]
    assert np.array_equal(img, want)
    assert info == dict(voxels=a.size, pixels=nx * ny, covered=nx * ny, hits=int((want != 0).sum()), steps=nx * ny,
                        samples=nx * ny)
    # a label alone; and a slab of five layers ends at its first match in s order
    img7, _ = R.slice_image(S.GRID_VOLUME, a, pl, origin=S.GRID_ORIGIN, label=256)
    assert np.array_equal(img7, np.where(want == 256, want, 0))
    pl5 = mpr_ref.axis_plane(2, (k + 0.5) / nz, nx, ny, 5, 1.0 / nz)
    img5, info5 = R.slice_image(S.GRID_VOLUME, a, pl5, origin=S.GRID_ORIGIN)
    first = np.zeros((ny, nx), np.uint32)
    count = np.zeros((ny, nx), np.int64)
    for kk in range(k - 2, k + 3):
        layer = np.zeros((ny, nx), np.uint32)
        layer[oy:oy + S.GRID_EXT[1], ox:ox + S.GRID_EXT[0]] = a[kk - oz]
        count += first == 0
        first = np.where(first == 0, layer, first)
    assert np.array_equal(img5, first) and info5["steps"] == info5["samples"] == int(count.sum())


# ---- the scenes hold what they are for (the reference's own output) ---------------------------------------
def test_the_parity_scenes_hit_miss_and_pass_set_cells():
    """Scenes 0 .. 4 (5 looks from inside the near plane and covers no pixel; 6 is one pixel): at least
    30 hits, 30 covered pixels that miss, and 30 hit rays that took a sample in a cell whose bit is set
    but whose voxel does not match before they hit."""
    for i in range(5):
        rec, info, tr = S.parity_reference(i)
        hit = rec["step"] != R.MISS
        assert info["hits"] >= 30 and info["covered"] - info["hits"] >= 30, (i, info)
        assert int(((tr["near"] > 0) & hit).sum()) >= 30, i
        assert np.unique(rec["step"][hit]).size >= 20  # hits deep in the volume, not at the entry alone
    for i in (5, 6):
        assert S.parity_reference(i)[1]["covered"] == (0, 1)[i - 5]


def test_the_grid_scene_hits_in_every_face_cell_layer_and_clamps():
    m = S.byte_mask(S.GRID_EXT, 0.5)
    rec, info, tr = R.hit_image(S.grid_scene("diag", FULL, 45, 35), m, S.GRID_ORIGIN)
    hit = rec["step"] != R.MISS
    assert info["hits"] >= 30 and info["covered"] - info["hits"] >= 30
    for (a, side), inside in S.face_cells(S.GRID_EXT, rec["index"][hit]).items():
        assert inside.sum() >= 1, (a, side)  # side 1: the cut cell layer at the grid's far face
    assert all(e % 8 for e in S.GRID_EXT) and all(o % 8 for o in S.GRID_ORIGIN)
    assert all(o + e < d for o, e, d in zip(S.GRID_ORIGIN, S.GRID_EXT, S.GRID_VOLUME))
    c = [-(-e // 8) for e in S.GRID_EXT]
    assert c == [5, 3, 3] and c[0] * c[1] * c[2] == 45 > 32 and 32 % c[0]  # a cell row crosses the word boundary
    # under the open box a ray that enters through a far face samples at exactly 1.0: its voxel is clamped
    v = volume("g13")
    rec, info, tr = R.hit_image(S.parity_scene(3, box=S.OPEN), S.byte_mask(v.shape[::-1], 0.5))
    cl = tr["clamped"] & (rec["step"] != R.MISS)
    assert cl.sum() >= 1 and np.all((rec["pos"][cl] == 1.0).any(-1)) and np.all(rec["step"][cl] == 0)
    # more than one workgroup in the occupancy pass
    assert vr_amd.mview_occupancy_words(S.BIG_DIMS) == 24


# ---- the binding ---------------------------------------------------------------------------------------
def test_every_declared_name_is_exported_and_listed():
    src = open(os.path.join(ROOT, "include", "vr", "vr_mview.h")).read()
    for h in ("vr_mesh.h", "vr_mpr.h"):
        assert f'#include "{h}"' in src
    assert "#define VR_ENOSPC" not in src and "typedef struct vr_mpr_plane" not in src  # reused, not redefined
    assert "SAMPLES" in src and "1 / max(dims)" in src  # the walk samples, and the header says so
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b(vr_[a-z0-9_]+)\s*\(", src))
    assert names == set(vr_amd.MVIEW_SYMBOLS) and len(names) == 8
    assert os.path.dirname(vr_amd.MVIEW_LIB_PATH) == os.path.dirname(vr_amd.LIB_PATH)
    assert vr_amd.FAMILY_LIBS["mview"] == ("VR_AMD_MVIEW_LIB", "libvr_amd_mview.so")
    nm = lambda path: {l.split()[-1] for l in subprocess.run(
        ["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout.splitlines()
        if " T " in l}
    assert not names - nm(vr_amd.MVIEW_LIB_PATH)
    for other in (vr_amd.LIB_PATH, vr_amd.MORPH_LIB_PATH, vr_amd.MASKCC_LIB_PATH, vr_amd.MSTAT_LIB_PATH):
        assert not names & nm(other)
    L = vr_amd.mview_lib()
    assert all(getattr(L, n).argtypes is not None for n in names)
    assert vr_amd.ABI_VERSION == 9 and vr_amd.lib().vr_abi_version() == 9  # an addition: the ABI stays
    for m in ("mask_occupancy_device", "mask_hit_render", "mask_hit_render_device", "mask_pick", "mask_slice",
              "mask_slice_device", "mview_last_kernel_name"):
        assert callable(getattr(vr_amd.OffscreenPass, m))
    # the fifth library takes the scaffold from the first, found beside it, and nothing from its siblings
    dyn = subprocess.run(["readelf", "-d", vr_amd.MVIEW_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libvr_amd.so" in dyn and "$ORIGIN" in dyn
    assert not any(f"libvr_amd_{f}" in dyn for f in ("morph", "maskcc", "mstat"))


def test_struct_layouts_match_header(tmp_path):
    fields = {"vr_mask_hit": ["pos", "depth", "element", "step", "index", "normal", "reserved"],
              "vr_mview_info": ["voxels", "pixels", "covered", "hits", "steps", "samples"],
              "vr_mview_occ_info": ["voxels", "cells", "cells_set", "matching"],
              "vr_mview_source": ["ext", "origin", "elem_bytes", "select", "label", "reserved", "array", "occupancy"]}
    body = "".join(f'  printf("%zu ", sizeof({s}));\n' +
                   "".join(f'  printf("%zu ", offsetof({s}, {f}));\n' for f in fs) for s, fs in fields.items())
    test = '#include "vr/vr_mview.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n' + body + \
           '  printf("%d %u %u %d %d %zu\\n", VR_ENOSPC, VR_MVIEW_MAX_EXTENT, VR_MVIEW_CELL, VR_MVIEW_ANY, ' \
           'VR_MVIEW_LABEL, sizeof(vr_mpr_plane)); return 0; }\n'
    tmp = str(tmp_path / "vr_mview_layout")
    with open(tmp + ".c", "w") as f:
        f.write(test)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), tmp + ".c", "-o", tmp], check=True)
    out = [int(x) for x in subprocess.run([tmp], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for s, fs in fields.items():
        T = getattr(vr_amd, s)
        want += [C.sizeof(T)] + [getattr(T, f).offset for f in fs]
    assert out == want + [-28, vr_amd.MVIEW_MAX_EXTENT, vr_amd.MVIEW_CELL, vr_amd.MVIEW_ANY, vr_amd.MVIEW_LABEL,
                          C.sizeof(vr_amd.vr_mpr_plane)]
    assert [C.sizeof(getattr(vr_amd, s)) for s in fields] == [32, 48, 32, C.sizeof(vr_amd.vr_mview_source)]
    assert C.sizeof(vr_amd.vr_mview_source) == 40 + 2 * C.sizeof(C.c_void_p)
    # the numpy record is the structure, and the reference's
    D = vr_amd.MVIEW_HIT_DTYPE
    assert D == R.HIT_DTYPE and D.itemsize == 32
    assert [D.fields[f][1] for f in fields["vr_mask_hit"]] == [getattr(vr_amd.vr_mask_hit, f).offset
                                                               for f in fields["vr_mask_hit"]]
    assert R.MISS == vr_amd.MVIEW_MISS == 0xFFFFFFFF and R.CELL == vr_amd.MVIEW_CELL
    miss = R.miss_records(1)
    assert miss.tobytes() == np.array([0, 0, 0, 0x7F800000, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0], np.uint32).tobytes()


def test_argument_errors_without_a_device():
    """Everything a NULL context refuses: -22, the outputs and infos untouched; and the pure word count."""
    L = vr_amd.mview_lib()
    info, oinfo, hit = vr_amd.vr_mview_info(), vr_amd.vr_mview_occ_info(), vr_amd.vr_mask_hit()
    for s, n in ((info, 48), (oinfo, 32), (hit, 32)):
        C.memset(C.byref(s), 0x77, n)
    mask = np.full(4, 1, np.uint8)
    out = np.full(64, 0x77, np.uint8)
    src = vr_amd.mview_source((2, 2, 1), mask.ctypes.data, 1)
    cam, p = vr_amd.vr_camera(), vr_amd.default_params()
    pl = vr_amd.axis_plane(vr_amd.AXIS_AXIAL, 0.5, 2, 2)
    assert L.vr_mask_occupancy_device(None, C.byref(src), out.ctypes.data, 1, C.byref(oinfo), None) == -22
    assert b"NULL" in vr_amd.lib().vr_last_error(None)  # the message is the first library's, as every family's
    assert L.vr_mask_occupancy_device(None, C.byref(src), out.ctypes.data, 0, C.byref(oinfo), None) == -22  # (not -28)
    assert L.vr_mask_hit_render_device(None, C.byref(cam), C.byref(p), C.byref(src), None, out.ctypes.data, 2,
                                       C.byref(info), None) == -22
    assert L.vr_mask_hit_render(None, C.byref(cam), C.byref(p), C.byref(src), None, out.ctypes.data, 0, C.byref(info)) == -22
    assert L.vr_mask_pick(None, C.byref(cam), C.byref(p), C.byref(src), 0, 0, C.byref(hit)) == -22
    assert L.vr_mask_slice_device(None, C.byref(pl), C.byref(src), out.ctypes.data, 4, C.byref(info), None) == -22
    assert L.vr_mask_slice(None, C.byref(pl), C.byref(src), out.ctypes.data, 0, C.byref(info)) == -22
    assert L.vr_mask_occupancy_device(None, None, None, 0, None, None) == -22
    assert L.vr_mask_hit_render_device(None, None, None, None, None, None, 0, None, None) == -22
    assert L.vr_mask_hit_render(None, None, None, None, None, None, 0, None) == -22
    assert L.vr_mask_pick(None, None, None, None, 0, 0, None) == -22
    assert L.vr_mask_slice_device(None, None, None, None, 0, None, None) == -22
    assert L.vr_mask_slice(None, None, None, None, 0, None) == -22
    assert L.vr_mview_last_kernel_name(None) == b""
    assert bytes(info) == b"\x77" * 48 and bytes(oinfo) == b"\x77" * 32 and bytes(hit) == b"\x77" * 32
    assert np.all(out == 0x77) and np.all(mask == 1)
    # vr_mview_occupancy_words is pure
    W = vr_amd.mview_occupancy_words
    assert [W((e, e, 1)) for e in (1, 8, 9)] == [1, 1, 1] and W((32768, 1, 1)) == 128 and W(S.GRID_EXT) == 2
    assert W((32768, 32768, 1)) == 2 ** 19 and W((32768, 32767, 4)) == 2 ** 19  # the largest: 2 MiB of words
    assert W((32768, 32768, 4)) == 0 and W((0, 8, 8)) == 0 and W((32769, 1, 1)) == 0 and W((65535, 65537, 1)) == 0
    assert L.vr_mview_occupancy_words(None) == 0


# ---- the host helper header, stand-alone, under AddressSanitizer + UBSan ---------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ missing")
def test_host_helpers_under_sanitizers(tmp_path):
    """Every refusal that needs no device at its boundary, with its text, vr_mview_occupancy_words and
    the cell geometry of every grid of 1 .. 20 voxels per axis, on csrc/vr_mview_host.h itself (the
    library's entry points refuse a NULL context before they reach it)."""
    stdout = run_sanitized(tmp_path, "mview")
    assert "source rules checked" in stdout and "call rules checked" in stdout
    # the word counts and the geometry totals, restated here
    seen = 0
    for line in stdout.splitlines():
        w = line.replace(":", " ").split()
        if w[0] != "words":
            continue
        ext = [int(x) for x in w[1:4]]
        ok = all(1 <= e <= 32768 for e in ext) and ext[0] * ext[1] * ext[2] <= 2 ** 32 - 1
        c = [-(-e // 8) for e in ext]
        assert int(w[4]) == (-(-c[0] * c[1] * c[2] // 32) if ok else 0), line
        seen += 1
    assert seen == 10
    n = range(1, 21)
    cells = sum(-(-a // 8) * -(-b // 8) * -(-c // 8) for a in n for b in n for c in n)
    words = sum(-(-(-(-a // 8) * -(-b // 8) * -(-c // 8)) // 32) for a in n for b in n for c in n)
    assert f"geometry {210 ** 3} voxels {cells} cells {words} words" in stdout
