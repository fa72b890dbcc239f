"""CPU: the y-major difference field's names in the ABI (vr.h VR_DERIVED_YMAJOR_FIELD, vr_debug.h
VR_KNOB_FIELD_ORDER and vr_debug_ymajor_field_bytes), and the y-major index maps checked on the
host over the GPU tests' brick grids (tools/ymajor_maps_check.hip: what the builders place is what
the march addresses, inside the allocations)."""
import ctypes as C
import os
import subprocess

import vr_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_derived_code_symbol_and_struct():
    assert vr_amd.DERIVED[7] == "ymajor_field" and vr_amd.DERIVED[6] == "ymajor_copy"
    assert "vr_debug_ymajor_field_bytes" in vr_amd.DEBUG_SYMBOLS
    lib = C.CDLL(vr_amd.LIB_PATH)  # a fresh handle: the symbol itself, not the binding's table
    fn = lib.vr_debug_ymajor_field_bytes
    fn.restype, fn.argtypes = C.c_uint64, [C.c_void_p]
    assert fn(None) == 0 and vr_amd.lib().vr_debug_ymajor_field_bytes(None) == 0
    assert C.sizeof(vr_amd.vr_memory_info) == 96
    assert vr_amd.ABI_VERSION == 9 and vr_amd.lib().vr_abi_version() == 9


def test_field_order_knob_values():
    assert vr_amd.KNOBS["field_order"] == 11 and vr_amd.KNOB_AUTO["field_order"] == -1
    lib = vr_amd.lib()
    # without a context the knob calls refuse before they look at the value ...
    assert lib.vr_debug_set_knob(None, 11, 0) != 0
    # ... so the accepted values are read from the header and the library's table
    hdr = open(os.path.join(ROOT, "include", "vr", "vr_debug.h")).read()
    assert "VR_KNOB_FIELD_ORDER = 11" in hdr
    src = open(os.path.join(ROOT, "volumetric-renderer_amd", "csrc", "vr_api.hip")).read()
    assert "case VR_KNOB_FIELD_ORDER: return &c->knobs.field_order;" in src
    # no case of its own in knob_value_ok: the default range -1 .. 1
    ok = src[src.index("bool knob_value_ok"):src.index("#ifdef VR_EXPERIMENTS")]
    assert "VR_KNOB_FIELD_ORDER" not in ok and "default: return v >= -1 && v <= 1;" in ok


def test_index_maps_on_the_host(tmp_path):
    exe = str(tmp_path / "ymajor_maps_check")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17",
                        os.path.join(ROOT, "tools", "ymajor_maps_check.hip"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, "40", "24", "56", "9", "7", "17", "56", "24", "40", "32", "28", "24"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.count(", ok") == 4, r.stdout
