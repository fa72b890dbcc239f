"""CPU: which kernel a launch runs (csrc/vr_variant.h) -- resolve_variant against a restatement
of the launch chains it replaced, and the names it can yield against the kernels the library
carries.  No device: vr_debug_variant_name is pure."""
import itertools
import subprocess

import vr_amd

ST_F32, QUAD, ALT, HALF, PLAIN, STENCIL = 4, 0x10, 0x20, 0x80, 0x100, 0x200
LAYOUTS = [0, 1, 2, 3, ST_F32, 0 | QUAD, 1 | QUAD, ST_F32 | ALT, ST_F32 | HALF, ST_F32 | PLAIN,
           ST_F32 | STENCIL]  # ST_F32 | HALF names a variant only: no launch takes it
BASE_TYPES = {0: "unsigned char", 1: "signed char", 2: "unsigned short", 3: "short", 4: "float",
              0 | QUAD: "vr::Quad8<unsigned char>", 1 | QUAD: "vr::Quad8<signed char>"}
ALT_TYPES = {ST_F32 | ALT: "vr::F32Alt", ST_F32 | PLAIN: "vr::F32P", ST_F32 | STENCIL: "vr::F32S"}
K_TF_LDS = 256
NS = "void vr::(anonymous namespace)::"


def b(*flags):
    return "".join(", true" if f else ", false" for f in flags)


# The chains of csrc/vr_kernels.hip at commit daa9d5a ("Add maximum-intensity projection as a
# second render mode"), function by function; None = hipErrorInvalidValue.
def launch_march_t(vt, shade, count, skip, gf=False, pipe=False):
    return f"{NS}march_kernel<{vt}{b(shade, count, skip, gf, pipe)}>(vr::MarchParams)"


def launch_pair_t(vt, shade, gf, pair):
    return f"{NS}march_pair_kernel<{vt}{b(shade, gf)}, {4 if pair == 4 else 2}>(vr::MarchParams)"


def launch_march_vt(vt, shade, count, p):
    zpair = vt == "float"  # kZPair<VT> of the types this chain is called with
    if p["pair"]:
        if not shade:
            return launch_pair_t(vt, False, False, p["pair"])
        if zpair and p["grad"]:
            return launch_pair_t(vt, True, True, p["pair"])
        return launch_pair_t(vt, True, False, p["pair"])
    if p["pipelined"] and not count and not p["skip_empty"] and p["tf_n"] <= K_TF_LDS:
        if not shade:
            return launch_march_t(vt, False, False, False, False, True)
        if zpair and p["grad"]:
            return launch_march_t(vt, True, False, False, True, True)
        return launch_march_t(vt, True, False, False, False, True)
    if zpair and shade and p["grad"]:
        if p["skip_empty"]:
            return launch_march_t(vt, True, count, True, True)
        return launch_march_t(vt, True, count, False, True)
    if p["skip_empty"]:
        return launch_march_t(vt, shade, count, True)
    return launch_march_t(vt, shade, count, False)


def launch_march_half_field(vt, count, p):
    if p["pair"]:
        return launch_pair_t(vt, True, True, p["pair"])
    if p["pipelined"] and not count and not p["skip_empty"] and p["tf_n"] <= K_TF_LDS:
        return launch_march_t(vt, True, False, False, True, True)
    if p["skip_empty"]:
        return launch_march_t(vt, True, count, True, True)
    return launch_march_t(vt, True, count, False, True)


def launch_march_alt(vt, shade, p):
    if p["pipelined"] and p["tf_n"] <= K_TF_LDS:
        return launch_march_t(vt, shade, False, False, False, True)
    return launch_march_t(vt, shade, False, False)


def launch_march(storage, shade, count, p):
    if storage in BASE_TYPES and storage != ST_F32:
        return launch_march_vt(BASE_TYPES[storage], shade, count, p)
    if storage == ST_F32:
        if shade and p["grad"] and p["grad_half"]:
            return launch_march_half_field("vr::F32H", count, p)
        return launch_march_vt("float", shade, count, p)
    if storage in ALT_TYPES:
        if count or p["pair"] or p["skip_empty"] or p["grad"]:
            return None
        return launch_march_alt(ALT_TYPES[storage], shade, p)
    return None


def launch_mip(storage, count, K, p):
    if storage not in BASE_TYPES:
        return None
    skip = p["skip_empty"]  # (skip without brick ranges is the launch's own check, not a fact)
    if count:
        K = 1
    elif K not in (1, 2, 4):
        return None
    return f"{NS}mip_kernel<{BASE_TYPES[storage]}{b(count, skip)}, {K}>(vr::MarchParams, vr::MipArgs)"


def parent_name(layout, mode, shade, count, skip, field, half, pipelined, tf_n, pair, inflight):
    p = dict(pair=pair, pipelined=pipelined, skip_empty=skip, grad=field, grad_half=half, tf_n=tf_n)
    if mode == vr_amd.MODE_MIP:
        return launch_mip(layout, count, inflight, p)
    return launch_march(layout, shade, count, p)


FLAGS = (0, 1)
PRODUCT = list(itertools.product(LAYOUTS, (vr_amd.MODE_COMPOSITE, vr_amd.MODE_MIP), FLAGS, FLAGS,
                                 FLAGS, FLAGS, FLAGS, FLAGS, (256, 257), (0, 2, 4), (0, 1, 2, 4)))
FIELDS = ("layout", "mode", "shade", "count", "skip", "field", "field_half", "pipeline", "tf_n",
          "pair", "mip_inflight")
_names = None


def resolved_names():
    global _names
    if _names is None:
        _names = [vr_amd.variant_name(**dict(zip(FIELDS, case))) for case in PRODUCT]
    return _names


def test_resolve_variant_equals_the_parent_chains():
    assert len(PRODUCT) == 33792
    for case, got in zip(PRODUCT, resolved_names()):
        assert got == parent_name(*case), dict(zip(FIELDS, case))


def test_reachable_names_are_the_built_kernels():
    """Every name the host can report exists as a kernel, every kernel carried is reachable."""
    reachable = {n for n in resolved_names() if n is not None}
    kd = sorted(name[:-3].decode() for name, _ in vr_amd.code_object_symbols()
                if name.endswith(b".kd"))
    dem = subprocess.run(["c++filt"], input="\n".join(kd), capture_output=True, text=True,
                         check=True).stdout.split("\n")
    built = {fam: {d for d in dem if f"::{fam}<" in d}
             for fam in ("march_kernel", "march_pair_kernel", "mip_kernel")}
    assert {fam: len(s) for fam, s in built.items()} == {
        "march_kernel": 92, "march_pair_kernel": 32, "mip_kernel": 56}
    everything = set().union(*built.values())
    assert reachable - everything == set()
    assert everything - reachable == set()


def test_variant_name_rejects_null_arguments():
    import ctypes as C
    L = vr_amd.lib()
    buf = C.create_string_buffer(8)
    assert L.vr_debug_variant_name(None, buf, 8) == -22
    assert L.vr_debug_variant_name(C.byref(vr_amd.vr_variant_facts(layout=4)), None, 8) == -22
    assert L.vr_debug_last_kernel_name(None) == b""
