"""CPU: connected components and region growing (include/vr/vr_label.h) -- the reference helper
tests/label_ref.py pinned against a plain breadth-first search, scipy where it is installed and
the counts beside the scenes; the binding's symbols and structs; the refusals that need no device;
the C++ shim; and the host helper header under AddressSanitizer + UBSan in a stand-alone program
(the label_* kernels: tests/test_kernel_inventory_cpu.py).
No GPU: nothing here creates a context."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import label_ref
import label_scenes as S
import vr_amd
from harness import run_sanitized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.dirname(vr_amd.LIB_PATH)
SMALL = [k for k in S.CASES]


# ---- the reference, pinned before anything is compared with it ----------------------------------------
@pytest.mark.parametrize("name,lo,hi,conn,box", SMALL)
def test_reference_equals_a_breadth_first_search(name, lo, hi, conn, box):
    labels, rec, info = S.reference(name, lo, hi, conn, box)
    assert S.pinned(info) == S.CASES[(name, lo, hi, conn, box)]
    v, origin = label_ref.crop(S.SCENES[name](), box)
    inm = label_ref.in_window(v, lo, hi)
    assert np.array_equal(labels, label_ref.bfs_label(inm, conn))
    assert np.array_equal(labels != 0, inm)
    # the records, restated voxel by voxel
    assert list(rec["label"]) == sorted(set(labels[labels != 0].tolist())) and not rec["reserved"].any()
    for r in rec[:: max(1, len(rec) // 25)]:
        z, y, x = np.nonzero(labels == r["label"])
        x, y, z = x + origin[0], y + origin[1], z + origin[2]
        assert r["voxels"] == x.size
        assert r["bbox_min"].tolist() == [x.min(), y.min(), z.min()]
        assert r["bbox_max"].tolist() == [x.max() + 1, y.max() + 1, z.max() + 1]
        assert r["sum"].tolist() == [x.sum(), y.sum(), z.sum()]
        # the label: 1 + the smallest box-linear index of the component
        assert r["label"] == 1 + int(np.flatnonzero(labels.reshape(-1) == r["label"])[0])
    assert info["voxels"] == labels.size and info["in_voxels"] == int(inm.sum()) == int(rec["voxels"].sum())
    if len(rec):
        big = rec[rec["voxels"] == rec["voxels"].max()]
        assert (info["largest_voxels"], info["largest_label"]) == (int(big["voxels"][0]), int(big["label"].min()))


def _scipy_canonical(inm, conn):
    ndi = pytest.importorskip("scipy.ndimage")
    lab, n = ndi.label(inm, structure=ndi.generate_binary_structure(3, 1 if conn == 6 else 3))
    flat = lab.reshape(-1)
    idx = np.flatnonzero(flat)
    first = np.zeros(n + 1, np.int64)
    u, fi = np.unique(flat[idx], return_index=True)
    first[u] = idx[fi] + 1  # scipy's labels renumbered to 1 + the smallest index
    return first[flat].astype(np.uint32).reshape(lab.shape), n


@pytest.mark.parametrize("name,lo,hi,conn,box", list(S.CASES) + list(S.LONG_CASES))
def test_reference_equals_scipy(name, lo, hi, conn, box):
    pins = {**S.CASES, **S.LONG_CASES}
    v, _ = label_ref.crop(S.SCENES[name](), box)
    want, n = _scipy_canonical(label_ref.in_window(v, lo, hi), conn)
    labels, rec, info = S.reference(name, lo, hi, conn, box)
    assert S.pinned(info) == pins[(name, lo, hi, conn, box)]
    assert info["components"] == n == len(rec) and np.array_equal(labels, want)


def test_the_pinned_scene_counts():
    """The figures beside the scenes: the snake is one path of 1979 voxels, the checkerboard the most
    components a volume holds, the noise windows' components and how many cross a brick boundary."""
    assert int(S.snake().sum()) == 1979 and int(S.checker().sum()) == 3392
    for (name, lo, hi, conn), n in S.STRADDLE.items():
        labels, rec, info = S.reference(name, lo, hi, conn, None)
        assert S.straddling(labels) == n >= 10 and info["components"] >= 100
    assert S.NOISE26 == (0.9, 1.0)
    rec = S.reference("noise", 0.7, 1.0, 6)[1]
    assert len(rec) == 448 and int(rec["voxels"].max()) == 213 and int((rec["voxels"] >= 10).sum()) == 43
    assert S.reference("noise", 0.3, 0.6, 6)[2]["components"] == 447
    # the snake under 6 is a path: two ends with one neighbour, everything else with two
    s = S.snake() > 0
    nb = np.zeros(s.shape, int)
    for a in range(3):
        for d in (1, -1):
            sh = np.roll(s, d, axis=a)
            idx = [slice(None)] * 3
            idx[a] = 0 if d == 1 else -1
            sh[tuple(idx)] = False
            nb += sh
    assert sorted(np.bincount(nb[s]).tolist()) == [0, 2, 1977]


def test_window_rule_of_the_reference():
    v = np.array([-0.0, 0.0, np.nan, np.inf, -np.inf, 0.25, 1.0], np.float32)
    assert label_ref.in_window(v, 0.0, 0.0).tolist() == [True, True, False, False, False, False, False]
    assert label_ref.in_window(v, -np.inf, np.inf).tolist() == [True, True, False, True, True, True, True]
    assert label_ref.in_window(v, 0.25, np.inf).tolist() == [False, False, False, True, False, True, True]
    # specials: everything but the NaNs; and +inf is in [0.25, +inf]
    sp = S.SCENES["specials"]()
    assert S.reference("specials", -S.INF, S.INF, 6)[2]["in_voxels"] == sp.size - int(np.isnan(sp).sum())
    lab = S.reference("specials", 0.25, S.INF, 6)[0]
    assert np.all(lab[np.isposinf(sp)] != 0) and not lab[np.isnan(sp) | np.isneginf(sp)].any()


def test_region_grow_of_the_reference():
    ref = S.reference("noise", 0.7, 1.0, 6, S.BOX)
    labels, rec, _ = ref
    big = rec[int(np.argmax(rec["voxels"]))]
    l = int(np.flatnonzero(labels.reshape(-1) == big["label"])[-1])
    bz, by, bx = labels.shape
    seed = (l % bx + S.BOX[0][0], (l // bx) % by + S.BOX[0][1], l // (bx * by) + S.BOX[0][2])
    mask, comp = label_ref.region_grow(None, seed, 0.7, 1.0, 6, S.BOX, labelled=ref)
    assert int(mask.sum()) == comp["voxels"] == int(big["voxels"]) and comp["label"] == int(big["label"])
    z, y, x = np.argwhere(labels == 0)[0]
    mask, comp = label_ref.region_grow(None, (x + 3, y + 2, z + 5), 0.7, 1.0, 6, S.BOX, labelled=ref)
    assert not mask.any() and comp["voxels"] == 0 and comp["label"] == 0


# ---- the binding ---------------------------------------------------------------------------------------
def test_every_declared_name_is_exported_and_listed():
    src = open(os.path.join(ROOT, "include", "vr", "vr_label.h")).read()
    assert '#include "vr_mesh.h"' in src and "#define VR_ENOSPC" not in src  # reused, not redefined
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b(vr_[a-z0-9_]+)\s*\(", src))
    assert names == set(vr_amd.LABEL_SYMBOLS) and len(names) == 5
    out = subprocess.run(["nm", "-D", "--defined-only", vr_amd.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not names - exported
    L = vr_amd.lib()
    assert all(getattr(L, n).argtypes is not None for n in names)
    assert vr_amd.ABI_VERSION == 9 and L.vr_abi_version() == 9  # an addition: the ABI stays
    assert vr_amd.LABEL_COMPONENT_DTYPE == label_ref.COMPONENT_DTYPE and vr_amd.LABEL_COMPONENT_DTYPE.itemsize == 64
    for m in ("label_count", "label", "label_device", "region_grow", "region_grow_device"):
        assert callable(getattr(vr_amd.OffscreenPass, m))


def test_struct_layouts_match_header(tmp_path):
    fields = {"vr_label_request": ["lo", "hi", "connectivity", "use_box", "box_min", "box_max"],
              "vr_label_component": ["label", "reserved", "voxels", "bbox_min", "bbox_max", "sum"],
              "vr_label_info": ["voxels", "in_voxels", "components", "largest_voxels", "largest_label", "reserved"]}
    body = "".join(f'  printf("%zu ", sizeof({s}));\n' +
                   "".join(f'  printf("%zu ", offsetof({s}, {f}));\n' for f in fs) for s, fs in fields.items())
    test = '#include "vr/vr_label.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n' + body + \
           '  printf("%d\\n", VR_ENOSPC); return 0; }\n'
    tmp = str(tmp_path / "vr_label_layout")
    with open(tmp + ".c", "w") as f:
        f.write(test)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), tmp + ".c", "-o", tmp], check=True)
    out = [int(x) for x in subprocess.run([tmp], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for s, fs in fields.items():
        T = getattr(vr_amd, s)
        want += [C.sizeof(T)] + [getattr(T, f).offset for f in fs]
    assert out == want + [-28]
    assert [C.sizeof(getattr(vr_amd, s)) for s in fields] == [40, 64, 40]
    D = vr_amd.LABEL_COMPONENT_DTYPE
    assert [D.fields[n][1] for n in fields["vr_label_component"]] == [0, 4, 8, 16, 28, 40]


def test_argument_errors_without_a_device():
    """Everything a NULL context refuses: -22, the outputs untouched."""
    L = vr_amd.lib()
    req = vr_amd.label_request(0.5, 1.0)
    info = vr_amd.vr_label_info()
    comp = vr_amd.vr_label_component()
    C.memset(C.byref(info), 0x77, 40)
    C.memset(C.byref(comp), 0x77, 64)
    lab = np.full(4, 0x77777777, np.uint32)
    rec = np.full(16, 0x77777777, np.uint32)
    mask = np.full(4, 0x77, np.uint8)
    seed = (C.c_uint32 * 3)(0, 0, 0)
    assert L.vr_label_count(None, C.byref(req), C.byref(info)) == -22
    assert b"NULL" in L.vr_last_error(None)
    assert L.vr_label_components(None, C.byref(req), lab.ctypes.data, 4, rec.ctypes.data, 1, C.byref(info)) == -22
    assert L.vr_label_components_device(None, C.byref(req), lab.ctypes.data, 4, rec.ctypes.data, 1,
                                        C.byref(info), None) == -22
    assert L.vr_region_grow(None, C.byref(req), seed, mask.ctypes.data, 4, C.byref(comp)) == -22
    assert L.vr_region_grow_device(None, C.byref(req), seed, mask.ctypes.data, 4, C.byref(comp), None) == -22
    assert L.vr_label_count(None, None, None) == -22
    assert L.vr_label_components(None, None, None, 0, None, 0, None) == -22
    assert L.vr_region_grow(None, None, None, None, 0, None) == -22
    assert bytes(info) == b"\x77" * 40 and bytes(comp) == b"\x77" * 64
    assert np.all(lab == 0x77777777) and np.all(rec == 0x77777777) and np.all(mask == 0x77)
    r = vr_amd.label_request(-float("inf"), 2.5, 26, ((1, 2, 3), (4, 5, 6)))
    assert (r.lo, r.hi, r.connectivity, r.use_box, list(r.box_min), list(r.box_max)) == \
        (-float("inf"), 2.5, 26, 1, [1, 2, 3], [4, 5, 6])


# ---- the shim ----------------------------------------------------------------------------------------
def test_shim_compiles_with_label_components_and_grow_region(tmp_path):
    src = str(tmp_path / "vr_shim_label.cpp")
    exe = str(tmp_path / "vr_shim_label")
    with open(src, "w") as f:
        f.write(r"""
#include <vr/offscreen_pass_hip.hpp>
#include <cstdio>
int main(int argc, char **)
{
    static_assert(sizeof(vr_label_request) == 40 && sizeof(vr_label_component) == 64 && sizeof(vr_label_info) == 40 &&
                      VR_ENOSPC == -28, "vr_label.h");
    if (argc > 1) {  // never taken in the CPU test: needs a device
        Vol::Rendering::Hip::OffscreenPass pass(8, 8);
        const uint32_t lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};
        const auto l = pass.label_components(0.5f, 1.0f, 26, lo, hi);
        const auto r = pass.grow_region(lo, 0.5f, 1.0f, 6, lo, hi);
        return l.labels.size() == l.info.voxels && l.components.size() == l.info.components && r.mask.size() == 1 ? 0 : 1;
    }
    vr_label_request req{};
    vr_label_info info{};
    vr_label_component c{};
    uint32_t lab[1] = {0}, seed[3] = {0, 0, 0};
    uint8_t m[1] = {0};
    std::printf("%d %d %d %d %d\n", vr_label_count(nullptr, &req, &info),
                vr_label_components(nullptr, &req, lab, 1, &c, 1, &info),
                vr_label_components_device(nullptr, &req, lab, 1, &c, 1, &info, nullptr),
                vr_region_grow(nullptr, &req, seed, m, 1, &c),
                vr_region_grow_device(nullptr, &req, seed, m, 1, &c, nullptr));
    return 0;
}
""")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src,
                        "-o", exe, "-L", LIBDIR, "-lvr_amd", "-Wl,-rpath," + LIBDIR],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip() == "-22 -22 -22 -22 -22"


# ---- the host helper header, stand-alone, under AddressSanitizer + UBSan ---------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ missing")
def test_host_helpers_under_sanitizers(tmp_path):
    stdout = run_sanitized(tmp_path, "label")
    # the request-check table: the box rule, the 2^32 - 1 bound and the brick range, restated here
    seen = refused_for_size = 0
    for line in stdout.splitlines():
        w = line.replace(":", " ").split()
        if w[0] != "box":
            continue
        use = int(w[1])
        lo, hi, dims = ([int(x) for x in w[a:a + 3]] for a in (2, 5, 9))
        ok, voxels, nwork = int(w[12]), int(w[13]), int(w[14])
        if not use:
            lo, hi = [0, 0, 0], dims
        box_ok = use <= 1 and all(lo[a] < hi[a] <= dims[a] for a in range(3))
        n = (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2]) if box_ok else 0
        assert ok == int(box_ok and n <= 2 ** 32 - 1), line
        refused_for_size += box_ok and not ok
        if ok:
            assert voxels == n, line
            cells = (7, 8, 8)
            nb = [(hi[a] + 1) // cells[a] - (lo[a] + 2) // cells[a] + 1 for a in range(3)]
            assert nwork == min(nb[0] * nb[1] * nb[2], 2 ** 64 - 1), line
        seen += 1
    assert seen == 26 and refused_for_size == 7
