"""GPU: the volume under a mask or a label array (include/vr/vr_mstat.h, lib/libvr_amd_mstat.so)
against tests/mstat_ref.py -- records, bins and infos byte for byte on every base layout and on
volumes whose last voxel lies on or beside each brick seam; boxes with origin = box_min; the chain
behind vr_label_components_device; NaN, infinities, -0.0 and ties; more than one workgroup; the
refusals; and the context's state.  The sums of a non-integer f32 volume are held to the header's
bound, computed here from n and A."""
import ctypes as C
import math

import numpy as np
import pytest

import edge_shapes as E
import hist_ref
import hit_scenes
import label_ref
import label_scenes
import mstat_ref as R
import mstat_scenes as S
import synth
import vr_amd
from gpu_kit import GUARD32, context_untouched, device_bytes, ext_of, unchanged
from gpu_kit import stream  # noqa: F401

pytestmark = pytest.mark.gpu

INF = float("inf")
F = np.float32
DT = vr_amd.MSTAT_REGION_DTYPE


def dims_id(v):
    return "x".join(str(a) for a in v) if isinstance(v[0], int) else "%s-%s" % (dims_id(v[0]), dims_id(v[1]))


def make_pass(vol, layout):
    dtype, knobs, storage, tag, _ = S.LAYOUTS[layout]
    rp = vr_amd.OffscreenPass(16, 16)
    for k, v in knobs.items():
        rp.set_knob(k, v)
    rp.volume_dataset_changed(synth.dataset(np.asarray(vol).astype(dtype)))
    assert rp.volume_info()[2] == storage
    return rp


def stats_device(rp, stream, mask, origin=(0, 0, 0), hist=None, odd=False):
    keep, ptr = device_bytes(mask, odd)
    got = rp.mask_stats_device(ext_of(mask), ptr, mask.dtype.itemsize, origin, hist, stream=stream.cuda_stream)
    assert unchanged(keep, mask, odd)  # the mask is only read
    return got


def region_record(d):
    r = np.zeros(1, DT)
    for k, v in d.items():
        r[k] = v
    return r


def labels_device(rp, stream, labels, table, origin=(0, 0, 0), rcap=None):
    """vr_label_stats_device -> (records, info): the table and the records at odd addresses, guard
    bytes past every buffer, the inputs unchanged."""
    import torch
    n = len(table)
    kl, lp = device_bytes(labels)
    kt, tp = device_bytes(table, odd=True)
    out = torch.full((n * 64 + 17,), 0x77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    info = rp.label_stats_device(ext_of(labels), lp, tp, n, out.data_ptr() + 1, n if rcap is None else rcap, origin,
                                 stream=stream.cuda_stream)
    # (complete on return: no synchronisation of ours before the copies on another stream)
    h = out.cpu().numpy()
    assert h[0] == 0x77 and np.all(h[1 + n * 64:] == 0x77)
    assert unchanged(kl, labels) and unchanged(kt, table, odd=True)
    return np.frombuffer(h[1:1 + n * 64].tobytes(), DT), info


def window_device(rp, stream, mask, shape, lo, hi, origin=(0, 0, 0), odd=False):
    import torch
    n = shape[0] * shape[1] * shape[2]
    keep, ptr = device_bytes(mask, odd) if mask is not None else (None, 0)
    o = torch.full((n + 9,), 0x77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    info = rp.mask_window_device(shape[::-1], ptr, mask.dtype.itemsize if mask is not None else 1, lo, hi,
                                 o.data_ptr() + 1, n, origin, stream=stream.cuda_stream)
    h = o.cpu().numpy()
    assert h[0] == 0x77 and np.all(h[n + 1:] == 0x77)
    assert mask is None or unchanged(keep, mask, odd)
    return h[1:n + 1].reshape(shape), info


def check_stats(got, want, what, exact=True, values=None):
    """A vr_mask_stats* result against the reference's (record, bins, hist info).  exact: the sums
    byte for byte; else within the header's bound of the fsum value, from the region's `values`."""
    wrec, wbins, whinfo = want
    rec = region_record(got["region"])
    print(what, got["region"])
    if exact:
        assert R.same_records(rec, wrec), (what, rec, wrec)
    else:
        assert R.same_but_sums(rec, wrec), (what, rec, wrec)
        b1, b2 = R.sum_bounds(values)
        e1, e2 = abs(float(rec["sum"][0]) - float(wrec["sum"])), abs(float(rec["sum2"][0]) - float(wrec["sum2"]))
        print(what, "sum error", e1, "bound", b1, "sum2 error", e2, "bound", b2)
        assert e1 <= b1 and e2 <= b2, (what, e1, b1, e2, b2)
    if wbins is not None:
        assert got["bins"].dtype == np.uint64 and got["bins"].tobytes() == wbins.tobytes(), what
        assert hist_ref.same_info(got["hist_info"], whinfo), (what, got["hist_info"], whinfo)
        assert got["hist_info"]["voxels"] == got["region"]["voxels"] and got["hist_info"]["nan"] == got["region"]["nan"]
    else:
        assert "bins" not in got


# ---- 1. whole volumes, every layout ------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(S.LAYOUTS))
@pytest.mark.parametrize("dims", E.VOLUMES, ids=dims_id)
def test_whole_volumes_on_every_layout(gpu, stream, dims, layout):
    vol = S.volume(dims, layout)
    tag = S.LAYOUTS[layout][3]
    ints = layout != "f32"  # (the fill is integers: the f32 sums are exact too, whatever the order)
    hist = (S.HIST[0],) + S.shifted(layout, *S.HIST[1:])
    lo, hi = S.shifted(layout, *S.WINDOW)
    rp = make_pass(vol, layout)
    try:
        assert tuple(rp.volume_info()[0]) == dims
        what = (dims, layout)
        # a 1-byte mask at an odd address, with and without the histogram
        m1 = S.byte_mask(vol.shape)
        check_stats(stats_device(rp, stream, m1, hist=hist, odd=True), R.mask_stats(vol, m1, ints, hist), what)
        assert rp.mstat_last_kernel_name() == "mstat_finalize_kernel<%s>" % ("int" if ints else "f32")
        check_stats(stats_device(rp, stream, m1, odd=True), R.mask_stats(vol, m1, ints), what)
        # a 4-byte mask whose elements are at least 2: the device and the host form
        m4 = S.word_mask(vol.shape)
        want = R.mask_stats(vol, m4, ints, hist)
        check_stats(stats_device(rp, stream, m4, hist=hist), want, what)
        check_stats(rp.mask_stats(m4, hist=hist), want, what)
        # the window under both masks and under none
        for m, odd in ((m1, True), (m4, False), (None, False)):
            wout, winfo = R.window(vol, m, lo, hi)
            out, info = window_device(rp, stream, m, vol.shape, lo, hi, odd=odd)
            assert info == winfo and out.tobytes() == wout.tobytes(), (what, info, winfo)
            assert rp.mstat_last_kernel_name() == "mstat_window_kernel<%s>" % tag
            host = rp.mask_window(m, lo, hi, shape=vol.shape)
            assert host["info"] == winfo and host["mask"].tobytes() == wout.tobytes(), what
        # the label array and the records of label_components
        for conn in (6, 26):
            labels, table, linfo = rp.label(lo, hi, conn)
            wrec, winfo = R.regions(vol, labels, table["label"], ints)
            rec, info = labels_device(rp, stream, labels, table)
            print(what, conn, info)
            assert info == winfo and info["unlisted"] == 0 and info["set"] == linfo["in_voxels"], (what, info, winfo)
            assert R.same_records(rec, wrec), (what, conn)
            assert np.array_equal(rec["voxels"], table["voxels"])
            hrec, hinfo = rp.label_stats(labels, table)
            assert hinfo == winfo and R.same_records(hrec, wrec), (what, conn)
            if len(table):
                assert rp.mstat_last_kernel_name() == "mstat_finalize_kernel<%s>" % ("int" if ints else "f32")
            else:
                assert rp.mstat_last_kernel_name() == "mstat_labels_kernel<%s>" % tag
    finally:
        rp.close()


# ---- 2. boxes ------------------------------------------------------------------------------------------------
_box_pass = {}


@pytest.fixture(scope="module")
def box_pass(gpu):
    """One context per layout for the whole module (the volumes are never modified)."""
    def get(layout):
        if layout not in _box_pass:
            _box_pass[layout] = make_pass(E.box_volume(layout), layout)
        return _box_pass[layout]
    yield get
    for rp in _box_pass.values():
        rp.close()
    _box_pass.clear()


@pytest.mark.parametrize("layout", E.BOX_LAYOUTS)
@pytest.mark.parametrize("box", E.BOXES, ids=dims_id)
def test_boxes_with_origin_at_box_min(gpu, stream, box_pass, box, layout):
    rp = box_pass(layout)
    full = E.box_volume(layout)
    s = E.box_scale(layout)
    ints = layout != "f32"
    shape = tuple(box[1][a] - box[0][a] for a in (2, 1, 0))
    vol = R.crop(full, box[0], shape)
    what = (layout, box)
    hist = (32, 0.25 * s, 0.75 * s)
    lo, hi = E.BOX_WINDOW[0] * s, E.BOX_WINDOW[1] * s
    m1, m4 = S.byte_mask(shape, 0.7), S.word_mask(shape)
    for m, odd in ((m1, True), (m4, False)):
        got = stats_device(rp, stream, m, box[0], hist, odd)
        check_stats(got, R.mask_stats(vol, m, ints, hist), what, exact=ints, values=vol[m != 0])
        wout, winfo = R.window(vol, m, lo, hi)
        out, info = window_device(rp, stream, m, shape, lo, hi, box[0], odd)
        assert info == winfo and out.tobytes() == wout.tobytes(), (what, info, winfo)
    wout, winfo = R.window(vol, None, lo, hi)
    out, info = window_device(rp, stream, None, shape, lo, hi, box[0])
    assert info == winfo and out.tobytes() == wout.tobytes(), (what, info, winfo)
    # the box's own components: the window's mask is labels != 0, and every record within the bound
    labels, table, linfo = E.box_label_reference(layout, box, 6)
    assert out.tobytes() == (labels != 0).astype(np.uint8).tobytes()
    rec, info = labels_device(rp, stream, labels, table, box[0])
    wrec, winfo = R.regions(vol, labels, table["label"], ints)
    assert info == winfo and info["unlisted"] == 0
    if ints:
        assert R.same_records(rec, wrec), what
    else:
        assert R.same_but_sums(rec, wrec), what
        for i in range(len(rec)):
            b1, b2 = R.sum_bounds(vol[labels == rec["label"][i]])
            assert abs(rec["sum"][i] - wrec["sum"][i]) <= b1 and abs(rec["sum2"][i] - wrec["sum2"][i]) <= b2, (what, i)


# ---- 3. the chain --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", E.BOX_LAYOUTS)
def test_the_chain_behind_the_labeller(gpu, stream, box_pass, layout):
    import torch
    rp = box_pass(layout)
    full = E.box_volume(layout)
    s = E.box_scale(layout)
    ints = layout != "f32"
    box = label_scenes.BOX
    lo, hi = 0.5 * s, 1.0 * s
    labels, table, linfo = label_ref.label(full, lo, hi, 6, box)
    n, nc = linfo["voxels"], linfo["components"]
    shape = labels.shape
    vol = R.crop(full, box[0], shape)
    assert nc > 8
    dl = torch.full((n + 8,), GUARD32, dtype=torch.int32, device="cuda")
    dc = torch.full((nc * 16 + 8,), GUARD32, dtype=torch.int32, device="cuda")
    dr = torch.full((nc * 16 + 8,), GUARD32, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    st = stream.cuda_stream
    assert rp.label_device(dl.data_ptr(), n, dc.data_ptr(), nc, lo, hi, 6, box, stream=st) == linfo
    info = rp.label_stats_device(shape[::-1], dl.data_ptr(), dc.data_ptr(), nc, dr.data_ptr(), nc, box[0], stream=st)
    hr = dr.cpu().numpy().view(np.uint32)
    rec = np.frombuffer(hr[:nc * 16].tobytes(), DT)
    assert np.all(hr[nc * 16:] == GUARD32)
    assert info == {"voxels": n, "set": linfo["in_voxels"], "unlisted": 0, "regions": nc}
    assert np.array_equal(rec["voxels"], table["voxels"]) and int(rec["voxels"].sum()) == linfo["in_voxels"]
    assert np.array_equal(rec["label"], table["label"])
    wrec, winfo = R.regions(vol, labels, table["label"], ints)
    assert R.same_but_sums(rec, wrec) and (not ints or R.same_records(rec, wrec))
    # every second record dropped from the table: its voxels are unlisted, the kept regions unchanged
    kept = np.ascontiguousarray(table[::2])
    krec, kinfo = labels_device(rp, stream, labels, kept, box[0])
    assert kinfo == {"voxels": n, "set": linfo["in_voxels"], "unlisted": int(table["voxels"][1::2].sum()),
                     "regions": len(kept)}
    assert R.same_but_sums(krec, rec[::2]) and (not ints or krec.tobytes() == rec[::2].tobytes())
    # the region grown from the largest component, windowed with its own window: the mask as it is
    big = table[np.argmax(table["voxels"])]
    at = int(big["label"]) - 1
    seed = tuple(c + o for c, o in zip((at % shape[2], (at // shape[2]) % shape[1], at // (shape[2] * shape[1])), box[0]))
    a = torch.full((n + 8,), 0x77, dtype=torch.uint8, device="cuda")
    b = torch.full((n + 8,), 0x77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    comp = rp.region_grow_device(seed, a.data_ptr(), n, lo, hi, 6, box, stream=st)
    assert comp["voxels"] == int(big["voxels"])
    winfo = rp.mask_window_device(shape[::-1], a.data_ptr(), 1, lo, hi, b.data_ptr(), n, box[0], stream=st)
    assert winfo == {"voxels": n, "in_set": comp["voxels"], "out_set": comp["voxels"]} and torch.equal(a, b)
    got = rp.mask_stats_device(shape[::-1], a.data_ptr(), 1, box[0], stream=st)["region"]
    r = rec[np.argmax(table["voxels"])]
    assert (got["voxels"], got["vmin"], got["vmax"], got["min_index"], got["max_index"]) == \
        (r["voxels"], r["vmin"], r["vmax"], r["min_index"], r["max_index"])
    # no mask, the whole volume: the window is labels != 0
    wl, wt, wi = label_ref.label(full, lo, hi, 6, None)
    out, info = window_device(rp, stream, None, full.shape, lo, hi)
    assert out.tobytes() == (wl != 0).astype(np.uint8).tobytes() and info["out_set"] == wi["in_voxels"]
    assert info["in_set"] == info["voxels"] == full.size


# ---- 4. specials ---------------------------------------------------------------------------------------------
def test_special_values(gpu, stream):
    v, lab = S.specials()
    table = np.zeros(len(S.SPECIAL_TABLE), vr_amd.LABEL_COMPONENT_DTYPE)
    table["label"] = S.SPECIAL_TABLE
    wrec, winfo = R.regions(v, lab, S.SPECIAL_TABLE, False)
    rp = make_pass(v, "f32")
    try:
        assert np.array_equal(rp.read_volume().view(np.uint32), v.view(np.uint32))  # NaN, -0.0 and the denormal are stored
        rec, info = labels_device(rp, stream, lab, table)
        print(rec, info)
        assert info == winfo
        assert R.same_but_sums(rec, wrec), (rec, wrec)
        for i, label in enumerate(S.SPECIAL_TABLE):
            vals = v[lab == label]
            for k, b in zip(("sum", "sum2"), R.sum_bounds(vals)):
                g, w = float(rec[k][i]), float(wrec[k][i])
                if math.isnan(w) or math.isinf(w):
                    assert (math.isnan(g) and math.isnan(w)) or g == w, (label, k, g, w)
                else:
                    assert abs(g - w) <= b, (label, k, g, w, b)
        r = {int(x["label"]): x for x in rec}
        assert r[8]["voxels"] == 0 and r[8]["sum"] == 0.0 and not np.signbit(r[8]["sum"])  # empty: +0.0
        assert r[45]["voxels"] == 2 and r[45]["sum"] == 0.0 and not np.signbit(r[45]["sum"])  # -0.0 alone: +0.0
        assert r[20]["nan"] == r[20]["voxels"] == 13 and r[20]["min_index"] == vr_amd.MSTAT_NONE  # all NaN
        assert r[60]["sum"] == float(S.DENORMAL) and r[60]["vmax"] == S.DENORMAL  # the denormal is not flushed
        # each region as a mask: the same record with label 1; the histogram counts its NaNs apart
        for i, label in enumerate(S.SPECIAL_TABLE):
            m = (lab == label).astype(np.uint8)
            hist = (8, -1.0, 1.0)
            got = stats_device(rp, stream, m, hist=hist, odd=True)
            want = R.mask_stats(v, m, False, hist)
            g, w = region_record(got["region"]), np.array([want[0]])
            assert R.same_but_sums(g, w), (label, g, w)
            assert got["bins"].tobytes() == want[1].tobytes() and hist_ref.same_info(got["hist_info"], want[2]), label
        # an empty mask, and a window with infinite bounds: everything but the NaNs
        got = stats_device(rp, stream, np.zeros(v.shape, np.uint8), hist=(4, 0.0, 1.0))
        assert R.same_records(region_record(got["region"]), R.empty_records([1])) and not got["bins"].any()
        assert got["hist_info"]["voxels"] == 0 and got["hist_info"]["vmin"] == np.inf
        for lo, hi in ((-INF, INF), (0.0, 0.0), (np.float32(S.DENORMAL), INF), (-INF, -INF)):
            wout, wi = R.window(v, None, lo, hi)
            out, info = window_device(rp, stream, None, v.shape, lo, hi)
            assert info == wi and out.tobytes() == wout.tobytes(), (lo, hi)
        assert R.window(v, None, -INF, INF)[1]["out_set"] == v.size - 15
        assert R.window(v, None, 0.0, 0.0)[1]["out_set"] == 20  # -0.0 is in
    finally:
        rp.close()


# ---- 5. beyond one workgroup ---------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["u16", "f32"])
def test_beyond_one_workgroup(gpu, stream, layout):
    vol = S.big_volume(layout)
    ints = layout == "u16"
    rp = make_pass(vol, layout)
    try:
        hist = (256, 0.0, 65535.0) if ints else (256, -2000.0, 2000.0)
        for i, density in enumerate(S.BIG_DENSITIES):
            m = S.byte_mask(vol.shape, density, seed=i)
            want = R.mask_stats(vol, m, ints, hist)
            got = stats_device(rp, stream, m, hist=hist, odd=True)
            check_stats(got, want, (layout, density), exact=ints, values=vol[m != 0])
            if ints:  # two calls write identical bytes
                again = stats_device(rp, stream, m, hist=hist, odd=True)
                assert again["region"] == got["region"] and again["bins"].tobytes() == got["bins"].tobytes()
        # about 150 000 one-voxel regions, and one region that covers the grid
        lab = S.checker_labels()
        table = S.table_of(lab)
        wrec, winfo = R.regions(vol, lab, table["label"], ints)
        rec, info = labels_device(rp, stream, lab, table)
        assert info == winfo and len(rec) > 150000
        assert R.same_records(rec, wrec)  # (one term a sum: bytes on f32 too)
        if ints:
            assert labels_device(rp, stream, lab, table)[0].tobytes() == rec.tobytes()
        one = np.full(vol.shape, 5, np.uint32)
        table = S.table_of(one)
        wrec, winfo = R.regions(vol, one, table["label"], ints)
        rec, info = labels_device(rp, stream, one, table)
        assert info == winfo and info["set"] == vol.size
        if ints:
            assert R.same_records(rec, wrec)
        else:
            b1, b2 = R.sum_bounds(vol)
            assert R.same_but_sums(rec, wrec)
            assert abs(rec["sum"][0] - wrec["sum"][0]) <= b1 and abs(rec["sum2"][0] - wrec["sum2"][0]) <= b2
        # a few large regions crossed by specks: slabs of z, every 37th voxel another label
        mix = (1 + np.arange(vol.size, dtype=np.uint32) // (vol.size // 3 + 1)).reshape(vol.shape)
        mix.reshape(-1)[::37] = 9
        table = S.table_of(mix)
        wrec, winfo = R.regions(vol, mix, table["label"], ints)
        rec, info = labels_device(rp, stream, mix, table)
        assert info == winfo and R.same_but_sums(rec, wrec) and (not ints or R.same_records(rec, wrec))
    finally:
        rp.close()


@pytest.mark.parametrize("layout", ["u16", "f32"])
def test_more_tiles_than_workgroups(gpu, stream, layout):
    """36 000 tiles on at most 4096 workgroups: every workgroup strides over 8 or 9 tiles, a lane gathers
    several voxels before the wave combines, and a lane of the label pass arrives at a run with sums it
    keeps -- the same label, a smaller part, a larger one (tests/test_mstat_cpu.py counts the cases on
    these labels).  A grid in a box at (1, 1, 1)."""
    full = S.thin_volume(layout)
    ints = layout == "u16"
    shape = S.THIN_DIMS[::-1]
    org = S.THIN_ORIGIN
    vol = R.crop(full, org, shape)
    rp = make_pass(full, layout)

    def check_records(lab):
        table = S.table_of(lab)
        wrec, winfo = R.regions(vol, lab, table["label"], ints)
        rec, info = labels_device(rp, stream, lab, table, org)
        print(layout, info, rec[["label", "voxels", "sum"]])
        assert info == winfo, (info, winfo)
        if ints:
            assert R.same_records(rec, wrec), (rec, wrec)
            assert labels_device(rp, stream, lab, table, org)[0].tobytes() == rec.tobytes()  # two calls, the same bytes
        else:
            assert R.same_but_sums(rec, wrec), (rec, wrec)
            for i in range(len(rec)):
                b1, b2 = R.sum_bounds(vol[lab == rec["label"][i]])
                e1, e2 = abs(rec["sum"][i] - wrec["sum"][i]), abs(rec["sum2"][i] - wrec["sum2"][i])
                print(layout, int(rec["label"][i]), "sum error", e1, "bound", b1, "sum2 error", e2, "bound", b2)
                assert e1 <= b1 and e2 <= b2, (i, e1, b1, e2, b2)

    try:
        check_records(S.thin_labels())          # five large labels crossed by specks
        check_records(np.full(shape, 7, np.uint32))  # one piece
        hist = (256, 0.0, 65535.0) if ints else (256, -2000.0, 2000.0)
        m = S.byte_mask(shape, 0.5)
        got = stats_device(rp, stream, m, org, hist, odd=True)
        check_stats(got, R.mask_stats(vol, m, ints, hist), (layout, "thin"), exact=ints, values=vol[m != 0])
        if ints:
            again = stats_device(rp, stream, m, org, hist, odd=True)
            assert again["region"] == got["region"] and again["bins"].tobytes() == got["bins"].tobytes()
        lo, hi = (20000.0, 40000.0) if ints else (-500.0, 700.0)
        for mm, odd in ((m, True), (None, False)):
            wout, winfo = R.window(vol, mm, lo, hi)
            out, info = window_device(rp, stream, mm, shape, lo, hi, org, odd)
            assert info == winfo and out.tobytes() == wout.tobytes(), (layout, info, winfo)
    finally:
        rp.close()


# ---- 6. errors -----------------------------------------------------------------------------------------------
def test_every_error_leaves_the_outputs_untouched(gpu, box_pass):
    import torch
    L = vr_amd.mstat_lib()
    rp = box_pass("f32")
    nx, ny, nz = E.BOX_DIMS
    shape = (5, 6, 7)
    n = 5 * 6 * 7
    lab = S.word_mask(shape)
    tab = S.table_of(lab)
    nt = len(tab)
    assert nt > 2
    ext, org = (C.c_uint32 * 3)(7, 6, 5), (C.c_uint32 * 3)(1, 2, 3)
    keep, mp = device_bytes(lab)
    kt, tp = device_bytes(tab)
    o = torch.full((n + 8,), 0x77, dtype=torch.uint8, device="cuda")
    dr = torch.full((nt * 16 + 4,), GUARD32, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    reg, mi, wi, hi = vr_amd.vr_mstat_region(), vr_amd.vr_mstat_info(), vr_amd.vr_morph_info(), vr_amd.vr_hist_info()
    bins = np.full(8, 0x7777777777777777, np.uint64)
    vp = C.c_void_p
    e3 = lambda a, b, c: (C.c_uint32 * 3)(a, b, c)

    def fresh():
        for s, k in ((reg, 64), (mi, 32), (wi, 24), (hi, 40)):
            C.memset(C.byref(s), 0x77, k)

    def req(lo=0.0, hi_=1.0, nbins=8, use_box=0):
        r = vr_amd.vr_hist_request()
        r.lo, r.hi, r.nbins, r.use_box = lo, hi_, nbins, use_box
        return C.byref(r)

    def stats(ext=ext, org=org, mask=mp, eb=4, hist=None, b=None, h=None, region=C.byref(reg)):
        return L.vr_mask_stats_device(rp._ctx, ext, org, vp(mask), eb, hist, b, h, region, None)

    def labels(ext=ext, org=org, labels=mp, table=tp, ntable=nt, regions=dr.data_ptr(), rcap=nt, info=C.byref(mi)):
        return L.vr_label_stats_device(rp._ctx, ext, org, vp(labels), vp(table), ntable, vp(regions), rcap, info, None)

    def window(ext=ext, org=org, mask=mp, eb=4, lo=0.0, hi_=1.0, out=o.data_ptr(), cap=n, info=C.byref(wi)):
        return L.vr_mask_window_device(rp._ctx, ext, org, vp(mask), eb, lo, hi_, vp(out), cap, info, None)

    fresh()
    # rcap / mcap one short: -28 before any kernel, the voxels set and nothing else
    assert labels(rcap=nt - 1) == -28 and b"smaller" in vr_amd.lib().vr_last_error(rp._ctx)
    assert (mi.voxels, mi.set, mi.unlisted, mi.regions) == (n, 0, 0, 0)
    assert window(cap=n - 1) == -28 and (wi.voxels, wi.in_set, wi.out_set) == (n, 0, 0)
    hl, ht = np.ascontiguousarray(lab), np.ascontiguousarray(tab)
    hr = np.full(nt * 64, 0x77, np.uint8)
    ho = np.full(n, 0x77, np.uint8)
    assert L.vr_label_stats(rp._ctx, ext, org, hl.ctypes.data, ht.ctypes.data, nt, hr.ctypes.data, nt - 1, C.byref(mi)) == -28
    assert L.vr_mask_window(rp._ctx, ext, org, hl.ctypes.data, 4, 0.0, 1.0, ho.ctypes.data, n - 1, C.byref(wi)) == -28
    fresh()
    bp, hp = bins.ctypes.data, C.byref(hi)
    nan = float("nan")
    bad = [stats(ext=None), stats(org=None), stats(mask=None), stats(region=None),
           stats(hist=req(), b=None, h=hp), stats(hist=req(), b=bp, h=None), stats(hist=None, b=bp, h=hp),
           stats(hist=None, b=bp), stats(hist=None, h=hp),
           stats(ext=e3(7, 0, 5)), stats(ext=e3(32769, 1, 1)), stats(ext=e3(32768, 32768, 4)),
           stats(org=e3(nx - 6, 2, 3)), stats(org=e3(1, ny - 5, 3)), stats(org=e3(1, 2, nz - 4)),
           stats(org=e3(0xFFFFFFFF, 0, 0)), stats(ext=e3(nx + 1, 1, 1), org=e3(0, 0, 0)),
           stats(eb=2), stats(eb=0), stats(mask=mp + 1), stats(mask=mp + 2),
           stats(hist=req(use_box=1), b=bp, h=hp), stats(hist=req(lo=1.0, hi_=1.0), b=bp, h=hp),
           stats(hist=req(lo=nan), b=bp, h=hp), stats(hist=req(hi_=INF), b=bp, h=hp),
           stats(hist=req(nbins=0), b=bp, h=hp), stats(hist=req(nbins=4097), b=bp, h=hp),
           labels(ext=None), labels(org=None), labels(labels=None), labels(table=None), labels(regions=None),
           labels(info=None), labels(ext=e3(0, 6, 5)), labels(org=e3(nx - 6, 0, 0)), labels(labels=mp + 2),
           labels(ntable=1 << 32, rcap=1 << 32), labels(ntable=1 << 32, rcap=0),
           labels(regions=mp + 4 * n - 1), labels(regions=tp + 64 * nt - 1), labels(regions=tp - 63, rcap=nt),
           window(ext=None), window(org=None), window(out=None), window(info=None), window(ext=e3(7, 6, 32769)),
           window(org=e3(1, 2, nz - 4)), window(eb=3), window(mask=None, eb=0), window(mask=mp + 3),
           window(lo=nan), window(hi_=nan), window(lo=1.0, hi_=0.5), window(lo=INF, hi_=-INF, cap=0),
           window(out=mp + 4 * n - 1), window(mask=o.data_ptr(), eb=1, out=o.data_ptr() + 3, cap=n)]
    assert bad == [-22] * len(bad), bad
    assert bytes(reg) == b"\x77" * 64 and bytes(mi) == b"\x77" * 32 and bytes(wi) == b"\x77" * 24 and bytes(hi) == b"\x77" * 40
    torch.cuda.synchronize()
    assert np.all(o.cpu().numpy() == 0x77) and np.all(dr.cpu().numpy().view(np.uint32) == GUARD32)
    assert np.all(bins == 0x7777777777777777) and np.all(hr == 0x77) and np.all(ho == 0x77)
    assert unchanged(keep, lab) and unchanged(kt, tab)
    # the grid may end on the volume's last voxel, and an empty table is a table
    assert stats(org=e3(nx - 7, ny - 6, nz - 5)) == 0 and reg.label == 1
    assert labels(ntable=0, rcap=0) == 0 and (mi.voxels, mi.set, mi.unlisted, mi.regions) == (n, int((lab != 0).sum()),
                                                                                                int((lab != 0).sum()), 0)
    assert np.all(dr.cpu().numpy().view(np.uint32) == GUARD32)
    # a table that is not ascending: VR_OK, the guards intact
    rev = np.ascontiguousarray(tab[::-1])
    krev, rp_ = device_bytes(rev)
    assert labels(table=rp_) == 0 and (mi.voxels, mi.set, mi.regions) == (n, int((lab != 0).sum()), nt)
    h = dr.cpu().numpy().view(np.uint32)
    assert np.all(h[nt * 16:] == GUARD32) and unchanged(krev, rev)
    assert np.array_equal(np.frombuffer(h[:nt * 16].tobytes(), DT)["label"], rev["label"])
    # no volume: a fresh context refuses
    empty = vr_amd.OffscreenPass(16, 16)
    try:
        fresh()
        rc = L.vr_mask_stats_device(empty._ctx, e3(1, 1, 1), e3(4000, 0, 0), vp(mp), 4, None, None, None, C.byref(reg), None)
        assert rc == -22 and bytes(reg) == b"\x77" * 64
    finally:
        empty.close()
    # the binding refuses what is no label array
    with pytest.raises(ValueError):
        rp.label_stats(np.zeros((2, 2, 2), np.uint8), tab)
    with pytest.raises(ValueError):
        rp.mask_stats(np.zeros((2, 2), np.uint8))


# ---- 7. state ------------------------------------------------------------------------------------------------
def test_the_calls_leave_the_context_as_it_was(gpu, stream):
    vol = label_scenes.noise()
    rp = hit_scenes.hit_pass(32, 24, np.asarray(vol), synth.tf_color(), 0.5)
    try:
        with context_untouched(rp) as state:
            assert rp.mstat_last_kernel_name() == ""  # a fresh context
            labels, table, linfo = rp.label(0.7, 1.0, 6)
            state.rebase()  # (the label family's name: the calls after it leave it alone)
            m = S.byte_mask(vol.shape)
            rp.timing_enable(True)
            rp.timing_reset()
            got = stats_device(rp, stream, m, hist=(16, 0.0, 1.0))
            assert rp.timing_read()[1] == 1  # each call's passes are one interval
            assert rp.mstat_last_kernel_name() == "mstat_finalize_kernel<f32>"
            check_stats(got, R.mask_stats(vol, m, False, (16, 0.0, 1.0)), "state", exact=False, values=vol[m != 0])
            rp.timing_reset()
            rec, info = labels_device(rp, stream, labels, table)
            assert rp.timing_read()[1] == 1 and np.array_equal(rec["voxels"], table["voxels"])
            rp.timing_reset()
            out, info = window_device(rp, stream, m, vol.shape, 0.7, 1.0)
            assert rp.timing_read()[1] == 1 and rp.mstat_last_kernel_name() == "mstat_window_kernel<f32>"
            assert out.tobytes() == R.window(vol, m, 0.7, 1.0)[0].tobytes()
            rp.timing_enable(False)
            rp.timing_reset()
            rp.mask_stats(m)
            assert rp.timing_read()[1] == 0
    finally:
        rp.close()


def test_a_multi_device_context_computes_on_its_lowest_device(gpu, stream):
    vol = E.box_volume("plain8")
    grp = vr_amd.OffscreenPass(16, 16, exchange=vr_amd.EXCHANGE_COPY, members=[0, 0])
    try:
        grp.volume_dataset_changed(synth.dataset(vol.astype(np.uint8)))
        box = label_scenes.BOX
        labels, table, linfo = label_ref.label(vol, 50.0, 100.0, 6, box)
        sub = R.crop(vol, box[0], labels.shape)
        wrec, winfo = R.regions(sub, labels, table["label"], True)
        rec, info = labels_device(grp, stream, labels, table, box[0])
        assert info == winfo and R.same_records(rec, wrec)
        hrec, hinfo = grp.label_stats(labels, table, box[0])
        assert hinfo == winfo and R.same_records(hrec, wrec)
        m = S.byte_mask(labels.shape)
        hist = (16, 10.0, 80.0)
        want = R.mask_stats(sub, m, True, hist)
        check_stats(stats_device(grp, stream, m, box[0], hist, odd=True), want, "group")
        check_stats(grp.mask_stats(m, box[0], hist), want, "group")
        wout, wi = R.window(sub, m, 50.0, 100.0)
        out, info = window_device(grp, stream, m, labels.shape, 50.0, 100.0, box[0], odd=True)
        assert info == wi and out.tobytes() == wout.tobytes()
        host = grp.mask_window(m, 50.0, 100.0, box[0])
        assert host["info"] == wi and host["mask"].tobytes() == wout.tobytes()
        assert grp.mstat_last_kernel_name() == "mstat_window_kernel<quad_u8>"  # (a small 8-bit volume: yz-quads)
    finally:
        grp.close()
