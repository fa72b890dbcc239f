"""GPU: the components of a mask (include/vr/vr_maskcc.h, lib/libvr_amd_maskcc.so) against
tests/maskcc_ref.py -- labels byte for byte, records and infos field by field: both connectivities,
both element widths, the host and the device forms, a 1-byte mask at an odd address, guard words past
every buffer; the window labelling of vr_label.h as the oracle at volume size; every selection rule
and hole filling; the refusals; and the calls chained behind vr_region_grow_device and
vr_mask_morph_device on a context that renders the same frame before and after."""
import ctypes as C

import numpy as np
import pytest

import hit_scenes
import label_ref
import label_scenes
import maskcc_ref as R
import maskcc_scenes as S
import morph_ref
import synth
import vr_amd
from gpu_kit import GUARD32, context_untouched, device_bytes, ext_of

pytestmark = pytest.mark.gpu

INF = float("inf")
DT = vr_amd.LABEL_COMPONENT_DTYPE


@pytest.fixture(scope="module")
def rp(gpu):
    p = vr_amd.OffscreenPass(16, 16)  # the calls read no volume: the placeholder will do
    yield p
    p.close()


def label_device(rp, m, conn, ncomps, odd=False, ccap=None):
    """vr_mask_label_device on a stream of its own -> (labels, records, info); the records at an odd
    address, guard words past every buffer, the mask unchanged."""
    import torch
    keep, ptr = device_bytes(m, odd)
    dl = torch.full((m.size + 8,), GUARD32, dtype=torch.int32, device="cuda")
    dc = torch.full((ncomps * 64 + 17,), 0x77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    info = rp.mask_label_device(ext_of(m), ptr, m.dtype.itemsize, dl.data_ptr(), m.size + 3, dc.data_ptr() + 1,
                                ncomps if ccap is None else ccap, conn, stream=stream.cuda_stream)
    # (complete on return: no synchronisation of ours before the copies on another stream)
    hl = dl.cpu().numpy().view(np.uint32)
    hc = dc.cpu().numpy()
    assert np.all(hl[m.size:] == GUARD32) and hc[0] == 0x77 and np.all(hc[1 + ncomps * 64:] == 0x77)
    assert keep.cpu().numpy()[(1 if odd else 0):][:m.nbytes].tobytes() == m.tobytes()  # the mask is only read
    return hl[:m.size].reshape(m.shape), np.frombuffer(hc[1:1 + ncomps * 64].tobytes(), DT), info


def select_device(rp, m, rule, conn=6, min_voxels=0, seed=(0, 0, 0), odd=False):
    import torch
    keep, ptr = device_bytes(m, odd)
    o = torch.full((m.size + 9,), 0x77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    info = rp.mask_select_device(ext_of(m), rule, ptr, m.dtype.itemsize, o.data_ptr() + 1, m.size, conn, min_voxels,
                                 seed, stream=stream.cuda_stream)
    h = o.cpu().numpy()
    assert h[0] == 0x77 and np.all(h[m.size + 1:] == 0x77)
    assert keep.cpu().numpy()[(1 if odd else 0):][:m.nbytes].tobytes() == m.tobytes()
    return h[1:m.size + 1].reshape(m.shape), info


def same_records(got, want):
    return got.dtype == want.dtype and got.tobytes() == want.tobytes()


# ---- 1. labels, records and info -------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.NAMES)
def test_labels_equal_the_reference(rp, name):
    m = S.mask(name)
    lab4 = S.as_labels(m)
    for conn in (6, 26):
        want, wrec, winfo = S.reference_label(name, conn)
        for mm in (m, lab4):  # both element widths, the host form
            labels, rec, info = rp.mask_label(mm, conn)
            print(name, conn, mm.dtype, info)
            assert info == winfo, (name, conn, mm.dtype, info, winfo)
            assert labels.dtype == np.uint32 and labels.tobytes() == want.tobytes(), (name, conn, mm.dtype)
            assert same_records(rec, wrec), (name, conn, mm.dtype)
        # the device form: a 1-byte mask at an odd address, then a 4-byte one; two calls, identical bytes
        nc = winfo["components"]
        l1, r1, i1 = label_device(rp, m, conn, nc, odd=True)
        l2, r2, i2 = label_device(rp, lab4, conn, nc)
        l3, r3, i3 = label_device(rp, m, conn, nc, odd=True)
        assert i1 == i2 == i3 == winfo
        assert l1.tobytes() == l2.tobytes() == l3.tobytes() == want.tobytes(), (name, conn)
        assert same_records(r1, wrec) and same_records(r2, wrec) and same_records(r3, wrec), (name, conn)
    assert rp.maskcc_last_kernel_name() == ("mcc_largest_kernel" if winfo["components"] else "mcc_scan_kernel")


@pytest.mark.parametrize("name,lo,hi", [("noise", 0.7, 1.0), ("long_checker", 1.0, 1.0)])
def test_the_window_labelling_is_the_oracle_at_volume_size(gpu, name, lo, hi):
    """vr_label_components_device over the whole volume writes labels L; vr_mask_label_device on L
    as a 4-byte mask writes the same label bytes, the same records and the same info."""
    import torch
    vol = np.asarray(label_scenes.SCENES[name]())
    rp = vr_amd.OffscreenPass(16, 16)
    try:
        rp.volume_dataset_changed(synth.dataset(vol))
        bz, by, bx = vol.shape
        n = vol.size
        stream = torch.cuda.Stream()
        for conn in (6, 26):
            key = (name, lo, hi, conn, None)
            pinned = label_scenes.CASES.get(key, label_scenes.LONG_CASES.get(key))  # (where the scenes pin one)
            nc = rp.label_count(lo, hi, conn)["components"]
            dl = torch.full((n + 8,), GUARD32, dtype=torch.int32, device="cuda")
            dc = torch.full((nc * 16 + 16,), GUARD32, dtype=torch.int32, device="cuda")
            ml = torch.full((n + 8,), GUARD32, dtype=torch.int32, device="cuda")
            mc = torch.full((nc * 16 + 16,), GUARD32, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            winfo = rp.label_device(dl.data_ptr(), n, dc.data_ptr(), nc, lo, hi, conn, None, stream=stream.cuda_stream)
            assert winfo["components"] == nc > 0 and (pinned is None or label_scenes.pinned(winfo) == pinned)
            info = rp.mask_label_device((bx, by, bz), dl.data_ptr(), 4, ml.data_ptr(), n, mc.data_ptr(), nc, conn,
                                        stream=stream.cuda_stream)
            assert info == winfo, (conn, info, winfo)
            assert torch.equal(ml, dl) and torch.equal(mc, dc), conn  # labels, records and guards alike
    finally:
        rp.close()


# ---- 2. selection ------------------------------------------------------------------------------------------
def check_select(rp, name, rule, conn=6, min_voxels=0, seed=(0, 0, 0), device=True):
    m = S.mask(name)
    want, winfo = S.reference_select(name, rule, conn, min_voxels, tuple(seed))
    got = rp.mask_select(m, rule, conn, min_voxels, seed)
    what = (name, rule, conn, min_voxels, seed)
    print(what, got["info"])
    assert got["info"] == winfo, (what, got["info"], winfo)
    assert got["mask"].dtype == np.uint8 and got["mask"].tobytes() == want.tobytes(), what
    if device:
        d1, i1 = select_device(rp, m, rule, conn, min_voxels, seed, odd=True)
        d4, i4 = select_device(rp, S.as_labels(m), rule, conn, min_voxels, seed)
        assert i1 == i4 == winfo and d1.tobytes() == d4.tobytes() == want.tobytes(), what
    return winfo


KEEP_SCENES = ("row129", "row257", "checker", "chunk130", "chunk70", "rand64_05", "rand64_50", "shells", "line_y",
               "none", "all", "morph_sparse70")


@pytest.mark.parametrize("name", KEEP_SCENES)
def test_the_keep_rules_equal_the_reference(rp, name):
    for conn in (6, 26):
        linfo = S.reference_label(name, conn)[2]
        i = check_select(rp, name, R.KEEP_LARGEST, conn)
        assert i["out_set"] == linfo["largest_voxels"] and i["kept"] == (1 if linfo["components"] else 0)
        big = linfo["largest_voxels"]
        for mv in (0, 1, 2, big, big + 1):
            i = check_select(rp, name, R.KEEP_MIN_VOXELS, conn, min_voxels=mv, device=mv == 2)
            if mv <= 1:
                assert i["kept"] == i["components"] and i["out_set"] == i["in_set"]
            if mv == big + 1:
                assert i["kept"] == 0 and i["out_set"] == 0
        on, off, last = S.seeds(name)
        for seed in (on, off, last):
            if seed is not None:
                i = check_select(rp, name, R.KEEP_SEED, conn, seed=seed)
                assert i["kept"] == int(S.mask(name)[seed[2], seed[1], seed[0]] != 0)
    assert rp.maskcc_last_kernel_name() == "mcc_select_kernel<0>"


def test_a_tie_for_the_largest_goes_to_the_smallest_label(rp):
    got = rp.mask_select(S.mask("checker"), vr_amd.MASK_KEEP_LARGEST, 6)
    assert got["info"]["kept"] == 1 and got["info"]["out_set"] == 1 and got["info"]["components"] > 64
    assert got["mask"].reshape(-1)[0] == 1
    # min_voxels beyond 32 bits keeps nothing
    got = rp.mask_select(S.mask("all"), vr_amd.MASK_KEEP_MIN_VOXELS, 6, min_voxels=1 << 40)
    assert got["info"]["kept"] == 0 and not got["mask"].any()


@pytest.mark.parametrize("name", S.FILL)
def test_fill_holes_equals_the_reference(rp, name):
    for conn in (6, 26):
        i = check_select(rp, name, R.FILL_HOLES, conn)
        if (name, conn) in S.FILLED:
            assert i["out_set"] - i["in_set"] == S.FILLED[(name, conn)]
        if name in S.THIN:
            assert i["kept"] == 0 and i["out_set"] == i["in_set"]
    assert rp.maskcc_last_kernel_name() == "mcc_select_kernel<1>"


# ---- 3. errors -------------------------------------------------------------------------------------------
def test_every_error_leaves_the_outputs_untouched(rp):
    import torch
    L = vr_amd.maskcc_lib()
    name = "chunk130"
    m = S.mask(name)
    n = m.size
    want, wrec, winfo = S.reference_label(name, 6)
    nc = winfo["components"]
    ext = (C.c_uint32 * 3)(*ext_of(m))
    keep, mp = device_bytes(S.as_labels(m))
    dl = torch.full((n + 4,), GUARD32, dtype=torch.int32, device="cuda")
    dc = torch.full((nc * 16 + 4,), GUARD32, dtype=torch.int32, device="cuda")
    o = torch.full((n + 4,), 0x77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    li, si = vr_amd.vr_label_info(), vr_amd.vr_mask_select_info()
    vp = C.c_void_p

    def fresh():
        C.memset(C.byref(li), 0x77, 40)
        C.memset(C.byref(si), 0x77, 40)

    def label(ext=ext, mask=mp, eb=4, conn=6, labels=dl.data_ptr(), lcap=n, comps=dc.data_ptr(), ccap=nc,
              info=C.byref(li)):
        return L.vr_mask_label_device(rp._ctx, ext, vp(mask), eb, conn, vp(labels), lcap, vp(comps), ccap, info, None)

    def select(ext=ext, rule=0, conn=6, seed=(0, 0, 0), mask=mp, eb=4, out=o.data_ptr(), cap=n, info=C.byref(si),
               req=True):
        r = vr_amd.mask_select_request(rule, conn, 1, seed)
        return L.vr_mask_select_device(rp._ctx, ext, C.byref(r) if req else None, vp(mask), eb, vp(out), cap, info, None)

    fresh()
    # lcap / mcap one short: -28 before any kernel, the voxels set and nothing else
    assert label(lcap=n - 1) == -28 and b"smaller" in vr_amd.lib().vr_last_error(rp._ctx)
    assert (li.voxels, li.in_voxels, li.components, li.largest_voxels, li.largest_label) == (n, 0, 0, 0, 0)
    assert select(cap=n - 1) == -28 and (si.voxels, si.in_set, si.out_set, si.components, si.kept) == (n, 0, 0, 0, 0)
    hl = np.full(n, GUARD32, np.uint32)
    hc = np.full(nc * 64, 0x77, np.uint8)
    ho = np.full(n, 0x77, np.uint8)
    req = vr_amd.mask_select_request(0)
    assert L.vr_mask_label(rp._ctx, ext, m.ctypes.data, 1, 6, hl.ctypes.data, n - 1, hc.ctypes.data, nc, C.byref(li)) == -28
    assert L.vr_mask_select(rp._ctx, ext, C.byref(req), m.ctypes.data, 1, ho.ctypes.data, n - 1, C.byref(si)) == -28
    fresh()
    e3 = lambda a, b, c: (C.c_uint32 * 3)(a, b, c)
    bx, by, bz = ext_of(m)
    bad = [label(ext=None), label(mask=None), label(labels=None), label(comps=None), label(info=None),
           label(ext=e3(130, 0, 8)), label(ext=e3(32769, 1, 1)), label(ext=e3(32768, 32768, 4)),
           label(eb=2), label(eb=0), label(conn=0), label(conn=18), label(conn=7, lcap=0),
           label(mask=mp + 1), label(mask=mp + 2), label(labels=dl.data_ptr() + 2),
           label(labels=mp, lcap=n), label(labels=mp + 4 * (n - 1), lcap=n), label(comps=mp + 4 * n - 1, ccap=1),
           label(mask=dl.data_ptr() + 4, labels=dl.data_ptr()),
           select(ext=None), select(req=False), select(mask=None), select(out=None), select(info=None),
           select(ext=e3(0, 9, 8)), select(eb=3), select(rule=4), select(rule=0xFFFFFFFF), select(conn=8),
           select(rule=2, seed=(bx, 0, 0)), select(rule=2, seed=(0, by, 0)), select(rule=2, seed=(0, 0, bz)),
           select(rule=2, seed=(0, 0, bz), cap=0), select(mask=mp + 3), select(out=mp + 4 * n - 1),
           select(mask=o.data_ptr(), eb=1, out=o.data_ptr() + 3, cap=n)]
    assert bad == [-22] * len(bad), bad
    assert bytes(li) == b"\x77" * 40 and bytes(si) == b"\x77" * 40
    torch.cuda.synchronize()
    assert np.all(dl.cpu().numpy().view(np.uint32) == GUARD32) and np.all(dc.cpu().numpy().view(np.uint32) == GUARD32)
    assert np.all(o.cpu().numpy() == 0x77) and np.all(hl == GUARD32) and np.all(hc == 0x77) and np.all(ho == 0x77)
    assert keep.cpu().numpy()[:4 * n].tobytes() == S.as_labels(m).tobytes()
    # a seed outside the grid is KEEP_SEED's error alone
    assert select(rule=0, seed=(bx, by, bz)) == 0 and select(rule=3, seed=(bx, by, bz)) == 0
    # ccap one below the count: complete labels, a complete info, untouched records -- device and host
    o.fill_(0x77)
    assert nc > 1 and label(ccap=nc - 1) == -28 and b"record" in vr_amd.lib().vr_last_error(rp._ctx)
    assert vr_amd.OffscreenPass._label_info(li) == winfo
    assert dl.cpu().numpy().view(np.uint32)[:n].tobytes() == want.tobytes()
    assert np.all(dc.cpu().numpy().view(np.uint32) == GUARD32)
    fresh()
    assert L.vr_mask_label(rp._ctx, ext, m.ctypes.data, 1, 6, hl.ctypes.data, n, hc.ctypes.data, nc - 1, C.byref(li)) == -28
    assert vr_amd.OffscreenPass._label_info(li) == winfo and hl.tobytes() == want.tobytes() and np.all(hc == 0x77)
    assert label(ccap=nc) == 0 and np.frombuffer(dc.cpu().numpy()[:nc * 16].tobytes(), DT).tobytes() == wrec.tobytes()
    # the binding refuses what is no mask
    with pytest.raises(ValueError):
        rp.mask_label(np.zeros((2, 2), np.uint8))
    with pytest.raises(ValueError):
        rp.mask_select(np.zeros((2, 2, 2), np.float32), 0)


# ---- 4. the chain, on a context that renders ------------------------------------------------------------
@pytest.mark.parametrize("name,lo,hi,r2,pieces,holes", [("specials", 0.25, INF, 2, 1, 2), ("noise", 0.45, 1.0, 1, 48, 0)])
def test_the_chain_from_a_click_to_a_distance_stays_on_the_device(gpu, name, lo, hi, r2, pieces, holes):
    """pick -> grow -> open -> keep the clicked piece -> fill its holes -> distance, with no host copy
    in between, between two renders of the same frame.  The opening cuts `specials`' region nowhere
    but leaves two cavities to fill; it cuts `noise`'s into 48 pieces, of which the clicked one stays."""
    import torch
    vol = label_scenes.SCENES[name]()
    labels, rec, linfo = label_scenes.reference(name, lo, hi, 6)
    bz, by, bx = labels.shape
    n = labels.size
    ext = (bx, by, bz)
    # the click: the deepest voxel of the largest component, which this opening cannot remove
    big = (labels == linfo["largest_label"]).astype(np.uint8)
    deep = morph_ref.edt(big, morph_ref.TO_UNSET)[1]
    assert deep["max_dist2"] > r2
    l = deep["max_index"]
    seed = (l % bx, (l // bx) % by, l // (bx * by))
    # the chain of references
    grown, comp = label_ref.region_grow(vol, seed, lo, hi, 6, None, labelled=(labels, rec, linfo))
    opened, open_info = morph_ref.morph(grown, morph_ref.OPEN, r2)
    kept, kept_info = R.select(opened, R.KEEP_SEED, 6, seed=seed)
    filled, fill_info = R.select(kept, R.FILL_HOLES, 6)
    dist, dist_info = morph_ref.edt(filled, morph_ref.TO_UNSET)
    assert (kept_info["components"], kept_info["kept"], fill_info["kept"]) == (pieces, 1, holes)
    assert 0 < kept_info["out_set"] <= open_info["out_set"] < comp["voxels"]

    rp = hit_scenes.hit_pass(32, 24, np.asarray(vol), synth.tf_color(), 0.5)
    try:
        with context_untouched(rp) as state:
            assert rp.maskcc_last_kernel_name() == ""  # a fresh context
            a = torch.full((n + 16,), 0x77, dtype=torch.uint8, device="cuda")
            b = torch.full((n + 16,), 0x77, dtype=torch.uint8, device="cuda")
            dd = torch.full((n + 8,), GUARD32, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            stream = torch.cuda.Stream()
            s = stream.cuda_stream
            rp.timing_enable(True)
            assert rp.region_grow_device(seed, a.data_ptr(), n, lo, hi, 6, None, stream=s) == comp
            state.rebase()  # (the label family's name: the calls after it leave the name alone)
            assert rp.morph_device(ext, vr_amd.MORPH_OPEN, r2, a.data_ptr(), 1, b.data_ptr(), n, stream=s) == open_info
            rp.timing_reset()
            assert rp.mask_select_device(ext, vr_amd.MASK_KEEP_SEED, b.data_ptr(), 1, a.data_ptr(), n, 6, seed=seed,
                                         stream=s) == kept_info
            assert rp.timing_read()[1] == 3  # the labelling passes, the records, the selection
            ms = rp.maskcc_pass_ms()  # (the bench's split of those intervals, kernel by kernel)
            assert list(ms) == list(rp.MASKCC_PASSES) and all(v > 0.0 for v in ms.values()), ms
            assert rp.maskcc_last_kernel_name() == "mcc_select_kernel<0>"
            rp.timing_reset()
            assert rp.mask_select_device(ext, vr_amd.MASK_FILL_HOLES, a.data_ptr(), 1, b.data_ptr(), n, 6,
                                         stream=s) == fill_info
            assert rp.timing_read()[1] == 3
            assert rp.maskcc_last_kernel_name() == "mcc_select_kernel<1>"
            assert rp.distance_transform_device(ext, b.data_ptr(), 1, dd.data_ptr(), n, to_set=False, stream=s) == dist_info
            ha, hb, hd = a.cpu().numpy(), b.cpu().numpy(), dd.cpu().numpy().view(np.uint32)
            assert ha[:n].tobytes() == kept.tobytes() and hb[:n].tobytes() == filled.tobytes()
            assert hd[:n].tobytes() == dist.tobytes()
            assert np.all(ha[n:] == 0x77) and np.all(hb[n:] == 0x77) and np.all(hd[n:] == GUARD32)
            # the labels of the filled piece: two intervals, and one where there is no component
            dl = torch.full((n + 8,), GUARD32, dtype=torch.int32, device="cuda")
            dc = torch.full((16 + 16,), GUARD32, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            rp.timing_reset()
            flab, frec, finfo = R.label(filled, 6)
            assert rp.mask_label_device(ext, b.data_ptr(), 1, dl.data_ptr(), n, dc.data_ptr(), 1, 6, stream=s) == finfo
            assert rp.timing_read()[1] == 2 and finfo["components"] == 1
            assert dl.cpu().numpy().view(np.uint32)[:n].tobytes() == flab.tobytes()
            assert rp.maskcc_last_kernel_name() == "mcc_largest_kernel"
            rp.timing_reset()
            assert rp.mask_label(np.zeros((3, 4, 5), np.uint8))[2]["components"] == 0
            assert rp.timing_read()[1] == 1 and rp.maskcc_last_kernel_name() == "mcc_scan_kernel"
            ms = rp.maskcc_pass_ms()
            assert all((v > 0.0) == (k in ("rows", "link", "flatten", "scan")) for k, v in ms.items()), ms
            rp.timing_enable(False)
            rp.timing_reset()
            rp.mask_select(S.mask("hole_block"), vr_amd.MASK_FILL_HOLES, 6)
            assert rp.timing_read()[1] == 0 and not any(rp.maskcc_pass_ms().values())
    finally:
        rp.close()


def test_a_multi_device_context_computes_on_its_lowest_device(gpu):
    grp = vr_amd.OffscreenPass(16, 16, exchange=vr_amd.EXCHANGE_COPY, members=[0, 0])
    try:
        name = "chunk130"
        m = S.mask(name)
        for conn in (6, 26):
            want, wrec, winfo = S.reference_label(name, conn)
            labels, rec, info = grp.mask_label(m, conn)
            assert info == winfo and labels.tobytes() == want.tobytes() and same_records(rec, wrec)
            l1, r1, i1 = label_device(grp, m, conn, winfo["components"], odd=True)
            assert i1 == winfo and l1.tobytes() == want.tobytes() and same_records(r1, wrec)
            for rule in (R.KEEP_LARGEST, R.FILL_HOLES):
                check_select(grp, name, rule, conn)
        assert grp.maskcc_last_kernel_name() == "mcc_select_kernel<1>"
    finally:
        grp.close()
