"""CPU: the y-major copy's kernel family in the variant table (csrc/vr_variant.h) -- the names the
host can report for layout code ST_F32 | 0x400 against the march_y_kernel instantiations the
library carries, both ways.  (The layout's index map is proven by static_asserts in
csrc/vr_internal.h at build time.)"""
import itertools
import subprocess

import vr_amd

ST_F32, YMAJOR = 4, 0x400
NS = "void vr::(anonymous namespace)::"
FLAGS = (0, 1)
FIELDS = ("layout", "mode", "shade", "count", "skip", "field", "field_half", "pipeline", "tf_n",
          "pair", "mip_inflight")


def expected(mode, shade, count, skip, field, half, pipeline, tf_n, pair, inflight):
    if mode != vr_amd.MODE_COMPOSITE or count or skip or pair or not pipeline or tf_n > 256:
        return None
    if shade:
        return f"{NS}march_y_kernel<vr::F32HY, true>(vr::MarchParams)" if field and half else None
    return None if field else f"{NS}march_y_kernel<vr::F32Y, false>(vr::MarchParams)"


def test_ymajor_names_are_the_built_kernels():
    reachable = set()
    for case in itertools.product((vr_amd.MODE_COMPOSITE, vr_amd.MODE_MIP, vr_amd.MODE_ISO), FLAGS,
                                  FLAGS, FLAGS, FLAGS, FLAGS, FLAGS, (256, 257), (0, 2, 4), (0, 2)):
        got = vr_amd.variant_name(**dict(zip(FIELDS, (ST_F32 | YMAJOR,) + case)))
        assert got == expected(*case), case
        if got:
            reachable.add(got)
    kd = sorted(name[:-3].decode() for name, _ in vr_amd.code_object_symbols()
                if name.endswith(b".kd"))
    dem = subprocess.run(["c++filt"], input="\n".join(kd), capture_output=True, text=True,
                         check=True).stdout.split("\n")
    built = {d for d in dem if "::march_y_kernel<" in d}
    assert len(built) == 2 and built == reachable
    # its tags belong to this family alone, and no other layout code reaches it
    assert not any("F32Y" in d or "F32HY" in d for d in dem if "::march_y_kernel<" not in d)
    for layout in (0, 1, 2, 3, 4, 0x10, 0x11, 0x24, 0x84, 0x104, 0x204, 0x400, 0x404 | 0x20):
        for shade, field, half in itertools.product(FLAGS, FLAGS, FLAGS):
            n = vr_amd.variant_name(layout=layout, mode=0, shade=shade, count=0, skip=0, field=field,
                                    field_half=half, pipeline=1, tf_n=256, pair=0, mip_inflight=0)
            assert "march_y_kernel" not in (n or ""), (layout, n)


def test_abi_9_struct_is_unchanged_and_the_copy_has_a_code():
    import ctypes as C
    assert C.sizeof(vr_amd.vr_memory_info) == 12 * 8
    assert vr_amd.DERIVED[6] == "ymajor_copy"
    assert vr_amd.lib().vr_debug_ymajor_copy_bytes(None) == 0
