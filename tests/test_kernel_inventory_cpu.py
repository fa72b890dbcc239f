"""CPU: the kernels of every library, once -- libvr_amd.so and the library of each mask family
(MASK_FAMILIES in the Makefile).  LIBRARIES is the one place a library's kernel count, the tag its
names carry and the tags they must not carry are written; the exact name sets, the golden lists of
tests/golden/kernels_before_*.txt and the scratch-memory rule of the Makefile's comment are each
checked here and nowhere else.  A new family adds a row, its name set, and nothing to the others.
No GPU: the code objects are read from the built libraries."""
import functools
import itertools
import os
import re
import subprocess

import pytest

import vr_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = "vr::(anonymous namespace)::"
TYPES = ["unsigned char", "signed char", "unsigned short", "short", "float",
         "vr::Quad8<unsigned char>", "vr::Quad8<signed char>"]

# library: (kernels, the tag every demangled name carries, the tags none may carry beyond the other rows' own)
LIBRARIES = {
    "base": (662 + 24, None, ()),          # libvr_amd.so: tests/golden/kernels_before_morph.txt
    "morph": (8, "morph_", ("label_", "mesh_")),
    "maskcc": (14, "mcc_", ("label_", "mesh_")),
    "mstat": (31, "mstat_", ()),
    "mview": (10, "mview_", ()),
    # the launch_mmesh_* instantiations of csrc/vr_mmesh_kernels.hip (bits<u8, u32>, classify, scan,
    # vertex<last, local>, smooth<last, local>, triangle), and the .kd symbols of libvr_amd_mmesh.so as
    # built at the commit that added the family
    "mmesh": (9, "mmesh_", ()),
}
FAMILIES = [k for k in LIBRARIES if k != "base"]
PATHS = dict(vr_amd.FAMILY_LIB_PATHS, base=vr_amd.LIB_PATH)


def golden(name):
    return open(os.path.join(ROOT, "tests", "golden", f"kernels_before_{name}.txt")).read().split()


def _demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return [d for d in out.split("\n") if d]


@functools.lru_cache(maxsize=None)
def _demangled_kernels(path):
    """(the sorted .kd symbols of the library's code object, their demangled names)"""
    kd = sorted(name[:-3].decode() for name, _ in vr_amd.code_object_symbols(path) if name.endswith(b".kd"))
    return kd, _demangle(kd)


@functools.lru_cache(maxsize=None)
def base_kernel_names():
    """The identifiers of libvr_amd.so's kernels ("march_kernel", "label_flatten_kernel", ...)."""
    base = set(re.findall(r"::(\w+_kernel)\b", "\n".join(_demangle(golden("morph")))))
    assert len(base) > 30
    # (the names the family tests looked for by hand)
    assert {"march_kernel", "mip_kernel", "iso_kernel", "proj_kernel", "mpr_kernel", "hist_kernel", "hit_kernel",
            "label_flatten_kernel"} <= base
    return base


def same(built, want):
    norm = lambda s: s.replace("> >", ">>")
    built, want = {norm(d) for d in built}, {norm(w) for w in want}
    assert built - want == set() and want - built == set()


# ---- the exact names ----------------------------------------------------------------------------------------
def want_morph():  # test_morph_cpu.py::test_morph_kernels_are_exactly_the_expected_ones
    want = {f"void {NS}morph_edt_x_kernel<{eb}>(vr::MorphArgs, unsigned long)" for eb in (1, 4)}
    want |= {f"void {NS}morph_edt_axis_kernel<{fin}, {words}>(vr::MorphArgs, vr::MorphAxis)"
             for fin in (0, 1, 2) for words in (16384, 32768)}
    return want


def want_maskcc():  # test_maskcc_cpu.py::test_maskcc_kernels_are_exactly_the_expected_ones
    want = {f"void {NS}mcc_rows_kernel<{eb}, {inv}>(vr::MccArgs, unsigned long)" for eb in (1, 4) for inv in (0, 1)}
    want |= {f"void {NS}mcc_link_kernel<{conn}>(vr::MccArgs, unsigned long)" for conn in (6, 26)}
    want |= {f"void {NS}mcc_select_kernel<{fill}>(vr::MccArgs)" for fill in (0, 1)}
    want |= {f"{NS}mcc_{k}_kernel(vr::MccArgs)" for k in ("flatten", "scan", "table_init", "largest", "keep")}
    want |= {f"{NS}mcc_accum_kernel(vr::MccArgs, unsigned long)"}
    return want


def want_mstat():  # test_mstat_cpu.py::test_mstat_kernels_are_exactly_the_expected_ones
    types = [("float", 0), ("unsigned short", 1), ("short", 1), ("unsigned char", 2), ("signed char", 2),
             ("unsigned char", 3), ("signed char", 3)]  # the seven base layouts: (element type, geometry)
    tail = "(vr::MstatArgs, unsigned int, unsigned int, unsigned long)"
    want = {f"void {NS}mstat_mask_kernel<{t}, {k}, {h}>{tail}" for t, k in types for h in ("true", "false")}
    want |= {f"void {NS}mstat_labels_kernel<{t}, {k}>{tail}" for t, k in types}
    want |= {f"void {NS}mstat_window_kernel<{t}, {k}>{tail}" for t, k in types}
    want |= {f"void {NS}mstat_finalize_kernel<{f}>(vr::MstatArgs)" for f in ("true", "false")}
    want |= {f"{NS}mstat_gather_kernel(vr::MstatArgs)"}
    return want


def want_mview():  # test_mview_cpu.py::test_mview_kernels_are_exactly_the_expected_ones (the pick is a hit kernel: no fourth body)
    elems = ("unsigned char", "unsigned int")
    want = {f"void {NS}mview_occupancy_kernel<{t}>(vr::MviewOccArgs)" for t in elems}
    want |= {f"void {NS}mview_hit_kernel<{t}, {o}>(vr::MarchParams, vr::MviewHitArgs)" for t in elems for o in ("true", "false")}
    want |= {f"void {NS}mview_slice_kernel<{t}, {o}>(vr::MviewSliceArgs)" for t in elems for o in ("true", "false")}
    return want


def want_mmesh():  # new: the family had no kernel list
    want = {f"void {NS}mmesh_bits_kernel<{t}>(vr::MmeshArgs)" for t in ("unsigned char", "unsigned int")}
    want |= {f"void {NS}mmesh_{k}_kernel<{last}>(vr::MmeshArgs)" for k in ("vertex", "smooth") for last in ("true", "false")}
    want |= {f"{NS}mmesh_{k}_kernel(vr::MmeshArgs)" for k in ("classify", "scan", "triangle")}
    return want


WANT = {"morph": want_morph, "maskcc": want_maskcc, "mstat": want_mstat, "mview": want_mview, "mmesh": want_mmesh}


def test_every_library_has_a_row():
    assert set(PATHS) == set(LIBRARIES) and set(WANT) == set(FAMILIES)


# test_{morph,maskcc,mstat,mview}_cpu.py::test_<family>_kernels_are_exactly_the_expected_ones, and the counts
# and tags of test_maskcc_cpu.py::test_the_other_two_libraries_keep_exactly_their_kernels,
# test_mstat_cpu.py::test_the_other_three_libraries_keep_exactly_their_kernels and the loop that closed
# test_mview_cpu.py::test_mview_kernels_are_exactly_the_expected_ones
@pytest.mark.parametrize("family", FAMILIES)
def test_a_family_library_holds_exactly_its_kernels(family):
    count, tag, never = LIBRARIES[family]
    want = WANT[family]()
    assert len(want) == count
    kd, dem = _demangled_kernels(PATHS[family])
    assert set(dem) == want and len(kd) == count
    assert all(f"{NS}{tag}" in d for d in dem)
    others = tuple(LIBRARIES[f][1] for f in FAMILIES if f != family)
    assert not [d for d in dem if any(t in d for t in never + others)]


# test_morph_cpu.py::test_the_first_library_keeps_exactly_its_kernels, and the libvr_amd.so half of the three
# "the other libraries keep theirs" tests: the parent's list, and no family's tag
def test_the_first_library_keeps_exactly_its_kernels():
    """A kernel family lives in a library of its own: libvr_amd.so's kernel list is the one it had
    before the first family left."""
    count, _, _ = LIBRARIES["base"]
    before = golden("morph")
    assert len(before) == count
    kd, dem = _demangled_kernels(PATHS["base"])
    assert kd == sorted(before)
    assert not [d for d in dem + before if any(LIBRARIES[f][1] in d for f in FAMILIES)]


# test_{hit,mesh,label}_cpu.py::test_every_kernel_that_existed_before_is_still_there and the chain half of
# test_morph_cpu.py::test_the_first_library_keeps_exactly_its_kernels
def test_the_golden_lists_are_a_chain_and_the_library_holds_them():
    hit, mesh, label, morph = (golden(n) for n in ("hit", "mesh", "label", "morph"))
    kd = set(_demangled_kernels(PATHS["base"])[0])
    assert len(hit) == 527 and not any("hit_kernel" in n for n in hit)
    assert set(hit) - kd == set()
    assert len(mesh) == 632 and not any("mesh_" in n for n in mesh)
    assert set(mesh) - kd == set()
    assert len(label) == 632 + 30 and not any("label_" in n for n in label)
    assert set(mesh) < set(label) and all("mesh_" in n for n in set(label) - set(mesh))
    assert set(label) - kd == set() and all("label_" in n for n in kd - set(label))
    assert len(morph) == LIBRARIES["base"][0] and set(label) < set(morph)
    assert all("label_" in n for n in set(morph) - set(label)) and not any("morph_" in n for n in morph)


# test_hit_cpu.py::test_hit_kernels_are_exactly_the_expected_105
def test_hit_kernels_are_exactly_the_expected_105():
    want = {f"void {NS}hit_kernel<{t}, {kind}, {count}, {k}>(vr::MarchParams, vr::HitArgs)"
            for t, kind, (count, k) in itertools.product(TYPES, range(5), (("false", 1), ("false", 2),
                                                                             ("true", 1)))}
    assert len(want) == 7 * 5 * 3 == 105
    _, dem = _demangled_kernels(PATHS["base"])
    built = {d for d in dem if "hit_kernel<" in d}
    assert built - want == set() and want - built == set()
    # the name stays out of the other families' matches
    assert not any(f"::{fam}<" in d for d in built
                   for fam in ("march_kernel", "mip_kernel", "iso_kernel", "proj_kernel", "mpr_kernel",
                               "hist_kernel"))


# test_mesh_cpu.py::test_mesh_kernels_are_exactly_the_expected_30
def test_mesh_kernels_are_exactly_the_expected_30():
    want = {f"void {NS}mesh_classify_kernel<{t}>(vr::MeshArgs)" for t in TYPES}
    want |= {f"void {NS}mesh_quad_kernel<{t}>(vr::MeshArgs)" for t in TYPES}
    want |= {f"void {NS}mesh_vertex_kernel<{t}, {n}>(vr::MeshArgs)" for t in TYPES for n in ("false", "true")}
    want |= {f"{NS}mesh_scan_bricks_kernel(vr::MeshArgs)", f"{NS}mesh_scan_chunks_kernel(vr::MeshArgs)"}
    assert len(want) == 7 * 4 + 2 == 30
    _, dem = _demangled_kernels(PATHS["base"])
    same([d for d in dem if "mesh_" in d], want)


# test_label_cpu.py::test_label_kernels_are_exactly_the_expected_ones
def test_label_kernels_are_exactly_the_expected_ones():
    want = {f"void {NS}label_local_kernel<{t}, {c}>(vr::LabelArgs)" for t in TYPES for c in (6, 26)}
    geoms = ["vr::BrickGeom<8, 8, 8, 0>", "vr::BrickGeom<7, 8, 8, 0>"]  # every layout but plain 8-bit; plain 8-bit
    want |= {f"void {NS}label_seam_kernel<{c}, {g}>(vr::LabelArgs)" for c in (6, 26) for g in geoms}
    want |= {f"{NS}label_{k}_kernel(vr::LabelArgs)" for k in ("flatten", "scan_chunks", "table_init", "accum",
                                                                "largest", "grow")}
    assert len(want) == 14 + 4 + 6 == 24
    _, dem = _demangled_kernels(PATHS["base"])
    built = [d for d in dem if "label_" in d]
    same(built, want)
    forbidden = ("mesh_", "march_kernel", "mip_kernel", "iso_kernel", "proj_kernel", "mpr_kernel", "hist_kernel",
                 "hit_kernel")
    assert not [d for d in built if any(f in d for f in forbidden)]


# the "no existing kernel's name" halves of the four family tests.  mstat's form ("::name" opens no
# identifier of the family, which covers mview's "::name<" and "::name(") holds for every family; morph's and
# maskcc's form (the name occurs nowhere in the string) for the three whose names embed no base name --
# mview_hit_kernel and mmesh_classify_kernel embed one on purpose.
@pytest.mark.parametrize("family", FAMILIES)
def test_no_family_kernel_reuses_a_base_kernel_name(family):
    base = base_kernel_names()
    _, dem = _demangled_kernels(PATHS[family])
    assert not [d for d in dem if any(f"::{b}" in d for b in base)]
    if family in ("morph", "maskcc", "mstat"):
        assert not [d for d in dem if any(b in d for b in base)]


# test_mview_cpu.py::test_no_kernel_uses_scratch_memory, for every family the Makefile's comment promises it of
@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="hipcc missing")
@pytest.mark.parametrize("family", FAMILIES)
def test_no_kernel_uses_scratch_memory(tmp_path, family):
    """The compiler's resource-usage remarks of the kernel unit, compiled with the Makefile's flags."""
    count, tag, _ = LIBRARIES[family]
    mk = open(os.path.join(ROOT, "volumetric-renderer_amd", "Makefile")).read()
    flags = re.search(r"^HIPFLAGS = (.*?\\\n.*?)$", mk, re.M).group(1).replace("\\\n", " ")
    flags = flags.replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags +
                       ["-c", os.path.join(ROOT, "volumetric-renderer_amd", "csrc", f"vr_{family}_kernels.hip"),
                        "-o", str(tmp_path / f"{family}.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == count and all(tag in n for n in names), names
    assert scratch == [0] * count, dict(zip(names, scratch))
