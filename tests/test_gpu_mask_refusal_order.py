"""GPU: which refusal wins where a mask call (vr_morph.h, vr_maskcc.h, vr_mstat.h) has more than one
reason to refuse, on a single-device context and on a multi-device one (two members on device 0, as
tests/test_gpu_members.py makes it).  One host form and one device form of each family, a grid of
4 x 3 x 2 in a volume of 8 x 8 x 8, each case one call that is refused on the host before any launch:

  a bad argument and a short buffer together   -22, the info untouched at its 0x77 fill
  a short buffer alone                         -28, the info {voxels = 24} and zeros
  vr_mstat.h only: a short buffer on a context without a volume (a fresh one holds the one-voxel
  placeholder, which the grid lies beyond), and with origin + ext beyond the volume: -22 both, what
  needs the volume outranks the capacity.

Every case leaves a text in vr_last_error."""
import ctypes as C

import numpy as np
import pytest

import vr_amd

pytestmark = pytest.mark.gpu

EXT = (4, 3, 2)
VOXELS = 24
DIMS = (8, 8, 8)
EINVAL, ENOSPC = -22, -28


@pytest.fixture(scope="module", params=["single", "members"])
def passes(gpu, request):
    """(a context holding the 8 x 8 x 8 volume, a fresh one of the same kind)"""
    kw = {"device": 0} if request.param == "single" else {"members": (0, 0), "exchange": vr_amd.EXCHANGE_COPY}
    rp, fresh = vr_amd.OffscreenPass(32, 24, **kw), vr_amd.OffscreenPass(32, 24, **kw)
    rp.generate_volume(DIMS, np.float32, seed=11)
    yield rp, fresh
    fresh.close()
    rp.close()


@pytest.fixture(scope="module")
def arrays(gpu):
    """The mask and an output of four bytes a voxel, on the host and on the device."""
    import torch
    hm, ho = np.ones(VOXELS, np.uint8), np.zeros(VOXELS, np.uint32)
    dm = torch.ones(VOXELS, dtype=torch.uint8, device="cuda")
    do = torch.zeros(VOXELS, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return {"host": (hm.ctypes.data, ho.ctypes.data), "device": (dm.data_ptr(), do.data_ptr()), "keep": (hm, ho, dm, do)}


def _u3(v):
    return (C.c_uint32 * 3)(*v)


def _edt(ctx, form, mask, out, cap, info, bad=False, origin=None):
    L, target = vr_amd.morph_lib(), 2 if bad else vr_amd.EDT_TO_SET  # enum vr_edt_target ends at 1
    if form == "device":
        return L.vr_edt_squared_device(ctx, _u3(EXT), mask, 1, target, out, cap, C.byref(info), None)
    return L.vr_edt_squared(ctx, _u3(EXT), mask, 1, target, out, cap, C.byref(info))


def _select(ctx, form, mask, out, cap, info, bad=False, origin=None):
    L = vr_amd.maskcc_lib()
    req = vr_amd.mask_select_request(9 if bad else vr_amd.MASK_KEEP_LARGEST)  # enum vr_mask_rule ends at 3
    if form == "device":
        return L.vr_mask_select_device(ctx, _u3(EXT), C.byref(req), mask, 1, out, cap, C.byref(info), None)
    return L.vr_mask_select(ctx, _u3(EXT), C.byref(req), mask, 1, out, cap, C.byref(info))


def _window(ctx, form, mask, out, cap, info, bad=False, origin=(1, 2, 3)):
    L = vr_amd.mstat_lib()
    lo, hi = (1.0, 0.0) if bad else (0.0, 1.0)  # a window needs lo <= hi
    if form == "device":
        return L.vr_mask_window_device(ctx, _u3(EXT), _u3(origin), mask, 1, lo, hi, out, cap, C.byref(info), None)
    return L.vr_mask_window(ctx, _u3(EXT), _u3(origin), mask, 1, lo, hi, out, cap, C.byref(info))


FAMILIES = {"morph": (_edt, vr_amd.vr_edt_info), "maskcc": (_select, vr_amd.vr_mask_select_info),
            "mstat": (_window, vr_amd.vr_morph_info)}


def _refused(rp, call, info_type, form, arrays, **kw):
    """One call with a buffer one voxel short: (its return code, the info's bytes)."""
    info = info_type()
    C.memset(C.byref(info), 0x77, C.sizeof(info))
    mask, out = arrays[form]
    rc = call(rp._ctx, form, C.c_void_p(mask), C.c_void_p(out), VOXELS - 1, info, **kw)
    assert vr_amd.lib().vr_last_error(rp._ctx) != b"", (rc, form)
    return rc, bytes(info)


def _voxels_alone(info_type):
    info = info_type()
    info.voxels = VOXELS
    return bytes(info)


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_a_bad_argument_outranks_a_short_buffer(passes, arrays, family, form):
    call, info_type = FAMILIES[family]
    rc, info = _refused(passes[0], call, info_type, form, arrays, bad=True)
    assert rc == EINVAL and info == b"\x77" * C.sizeof(info_type)


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_a_short_buffer_alone_reports_the_voxels(passes, arrays, family, form):
    call, info_type = FAMILIES[family]
    rc, info = _refused(passes[0], call, info_type, form, arrays)
    assert rc == ENOSPC and info == _voxels_alone(info_type)


@pytest.mark.parametrize("form", ["host", "device"])
def test_mstat_no_volume_outranks_a_short_buffer(passes, arrays, form):
    rc, info = _refused(passes[1], _window, vr_amd.vr_morph_info, form, arrays, origin=(0, 0, 0))
    assert rc == EINVAL and info == b"\x77" * C.sizeof(vr_amd.vr_morph_info)


@pytest.mark.parametrize("form", ["host", "device"])
def test_mstat_a_grid_beyond_the_volume_outranks_a_short_buffer(passes, arrays, form):
    rc, info = _refused(passes[0], _window, vr_amd.vr_morph_info, form, arrays, origin=(4, 5, 7))  # 7 + 2 > 8
    assert rc == EINVAL and info == b"\x77" * C.sizeof(vr_amd.vr_morph_info)
