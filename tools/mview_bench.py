"""The view of a device mask or label array against the volume's own hit image and MPR slab (GPU;
measurement tool).

On the C3 volume (512^3 f32 from vr_generate_volume) and on C4 (1024^3 u8) one process times, on a
1024 x 1024 framebuffer with the fill_oblique camera,

    hit_iso           vr_hit_render_device, VR_HIT_ISO at the window's lower bound: the trilinear
                      first-hit kernel of the same surface, the yardstick
    hit_max           vr_hit_render_device, VR_HIT_MAX: a trilinear kernel that walks every ray to its end
    occupancy         vr_mask_occupancy_device of the byte mask
    mask_hit          vr_mask_hit_render_device of the byte mask of the window [0.3 of the data range,
                      +inf] (vr_mask_window_device with no mask), occupancy NULL
    mask_hit_occ      the same with its occupancy words
    label_hit         the same mask as a 4-byte array whose set elements are 7, VR_MVIEW_LABEL 7, no words
    label_hit_occ     with its words
    mpr_slab          vr_mpr_render_device of a 1024 x 1024 oblique slab of 64 samples, VR_MPR_MAX
    mask_slice        vr_mask_slice_device of the byte mask on the same plane, no words
    mask_slice_occ    with its words

A round runs --frames calls of a row after --warmup warm-up calls and takes the kernel time from
vr_timing_read (HIP events around each call's kernel and, for this family, the memset of its
counters); the rows alternate inside every round, and a row's figure is the median over --rounds
rounds.  What can be checked without a reference at this size is checked: records, pixels and infos
are the same bytes with and without the words, for the byte mask and for the label; every hit's
element is the mask's; the words' `matching` is the window's count; picks equal the image's records.
--host also times, once on C3, the host path the calls replace: the mask read back.

    python tools/mview_bench.py --host      # the next free profiles/rNN/mview

writes <out>/c3.json and <out>/c4.json and prints one JSON line per configuration.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("volumetric-renderer_amd", "tools", "tests", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, sub))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import synth  # noqa: E402
import vr_amd  # noqa: E402

CONFIGS = {"c3": (512, np.float32), "c4": (1024, np.uint8)}
LO_F = 0.3
INF = float("inf")
W = H = 1024
NSAMPLES = 64
LABEL = 7
DT = vr_amd.MVIEW_HIT_DTYPE


def next_free_out():
    prof = os.path.join(ROOT, "profiles")
    taken = [int(m.group(1)) for m in (re.fullmatch(r"r(\d+)", d) for d in os.listdir(prof)) if m]
    return os.path.join(prof, f"r{max(taken, default=0) + 1:02d}", "mview")


def write(res, args, name):
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, f"{name}.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1, default=lambda o: o.item())
        f.write("\n")
    return path


def run(name, args):
    n, dtype = CONFIGS[name]
    rp = vr_amd.OffscreenPass(W, H)
    lo, hi = rp.generate_volume((n,) * 3, dtype, seed=2024)
    rp.transfer_function_changed(synth.tf_color())
    wlo = float(np.float32(lo + LO_F * (hi - lo)))
    rp.isovalue_changed(wlo)
    nvox, ext = n ** 3, (n, n, n)
    stream = torch.cuda.current_stream().cuda_stream
    cam = synth.camera("fill_oblique").to_vr_camera()
    p = vr_amd.default_params()
    mask = torch.empty(nvox, dtype=torch.uint8, device="cuda")
    winfo = rp.mask_window_device(ext, 0, 1, wlo, INF, mask.data_ptr(), nvox, stream=stream)
    labels = mask.to(torch.int32) * LABEL
    nw = vr_amd.mview_occupancy_words(ext)
    occ_m = torch.zeros(nw, dtype=torch.int32, device="cuda")
    occ_l = torch.zeros(nw, dtype=torch.int32, device="cuda")
    src_m = lambda occ: vr_amd.mview_source(ext, mask.data_ptr(), 1, occupancy_ptr=occ_m.data_ptr() if occ else 0)
    src_l = lambda occ: vr_amd.mview_source(ext, labels.data_ptr(), 4, label=LABEL,
                                            occupancy_ptr=occ_l.data_ptr() if occ else 0)
    rec = [torch.zeros(W * H * 8, dtype=torch.int32, device="cuda") for _ in range(2)]
    pix = [torch.zeros(W * H, dtype=torch.int32, device="cuda") for _ in range(2)]
    vrec = torch.zeros(W * H * 6, dtype=torch.int32, device="cuda")
    img = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    plane = vr_amd.mpr_plane((0.5, 0.5, 0.5), *[np.asarray(v) / W for v in
                                                ((0.8, -0.8, 0.0), (0.45, 0.45, -0.9))],
                             np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0) / n, W, H, NSAMPLES, vr_amd.OP_MAX)

    occupancy = lambda src, words: rp.mask_occupancy_device(src(False), words.data_ptr(), nw, stream=stream)
    hits = lambda src, occ, out: rp.mask_hit_render_device(cam, p, src(occ), out.data_ptr(), W * H, stream=stream)
    slices = lambda src, occ, out: rp.mask_slice_device(plane, src(occ), out.data_ptr(), W * H, stream=stream)

    # ---- what can be checked without a reference ----
    checks, infos = {}, {}
    om, ol = occupancy(src_m, occ_m), occupancy(src_l, occ_l)
    infos["occupancy"] = om
    checks["occupancy"] = dict(matching_is_the_windows_count=om["matching"] == winfo["out_set"] == ol["matching"],
                               label_words_are_the_masks=bool(torch.equal(occ_m, occ_l)),
                               cells=om["cells"] == (n // 8) ** 3 and 0 < om["cells_set"] <= om["cells"])
    for key, src in (("mask", src_m), ("label", src_l)):
        a, b = hits(src, False, rec[0]), hits(src, True, rec[1])
        infos[key + "_hit"] = a
        h = np.frombuffer(rec[0].cpu().numpy().tobytes(), DT)
        hit = h["step"] != vr_amd.MVIEW_MISS
        checks[key + "_hit"] = dict(same_bytes_with_the_words=bool(torch.equal(rec[0], rec[1])), same_info=a == b,
                                    hits=a["hits"] == int(hit.sum()) > 0,
                                    elements=bool(np.all(h["element"][hit] == (1 if key == "mask" else LABEL))),
                                    misses=bool(np.all(h["index"][~hit] == vr_amd.MVIEW_MISS)))
        a, b = slices(src, False, pix[0]), slices(src, True, pix[1])
        infos[key + "_slice"] = a
        checks[key + "_slice"] = dict(same_bytes_with_the_words=bool(torch.equal(pix[0], pix[1])), same_info=a == b,
                                      hits=a["hits"] == int((pix[0] != 0).sum()) > 0)
    hits(src_m, True, rec[0])
    h = np.frombuffer(rec[0].cpu().numpy().tobytes(), DT).reshape(H, W)
    picks = [(x, y) for x in (100, 400, 512, 700, 1000) for y in (90, 512, 800)]
    checks["pick"] = dict(equals_the_image=all(rp.mask_pick(cam, p, src_m(False), x, y).tobytes() == h[y, x].tobytes()
                                               for x, y in picks))
    bad = {k: v for k, v in checks.items() if not all(v.values())}
    assert not bad, bad

    # ---- the times ----
    def timed(call, frames):
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        rp.timing_reset()
        rp.timing_enable(True)
        for _ in range(frames):
            call()
        torch.cuda.synchronize()
        ms, cnt = rp.timing_read()
        rp.timing_enable(False)
        assert cnt == frames, (cnt, frames)  # one interval a call
        return ms / frames

    rows = {"hit_iso": dict(call=lambda: rp.hit_image_device(cam, p, vr_amd.HIT_ISO, vrec.data_ptr(), stream=stream)),
            "hit_max": dict(call=lambda: rp.hit_image_device(cam, p, vr_amd.HIT_MAX, vrec.data_ptr(), stream=stream)),
            "occupancy": dict(call=lambda: occupancy(src_m, occ_m)),
            "mask_hit": dict(call=lambda: hits(src_m, False, rec[0])),
            "mask_hit_occ": dict(call=lambda: hits(src_m, True, rec[0])),
            "label_hit": dict(call=lambda: hits(src_l, False, rec[0])),
            "label_hit_occ": dict(call=lambda: hits(src_l, True, rec[0])),
            "mpr_slab": dict(call=lambda: rp.render_mpr_device(plane, p, img.data_ptr(), vr_amd.OUT_RGBA8, stream=stream)),
            "mask_slice": dict(call=lambda: slices(src_m, False, pix[0])),
            "mask_slice_occ": dict(call=lambda: slices(src_m, True, pix[0]))}
    for r in rows.values():
        r["ms_rounds"] = []
    for _ in range(args.rounds):  # the rows alternate inside every round
        for r in rows.values():
            r["ms_rounds"].append(round(timed(r["call"], args.frames), 5))
    for r in rows.values():
        del r["call"]
        ms = r["ms_rounds"]
        r["ms_median"] = statistics.median(ms)
        r["spread"] = round((max(ms) - min(ms)) / r["ms_median"], 4)
    med = {k: r["ms_median"] for k, r in rows.items()}
    res = dict(config=name, volume=f"{n}^3 {np.dtype(dtype).name}", frame=[W, H], camera="fill_oblique",
               data_range=[lo, hi], window=[wlo, "inf"], window_info=winfo, plane_samples=NSAMPLES, infos=infos,
               checks=checks, occupancy_bytes=4 * nw, frames=args.frames, warmup=args.warmup, rounds=args.rounds,
               device=torch.cuda.get_device_name(0), code_hash=vr_amd.kernel_code_hash(),
               last_kernel=rp.mview_last_kernel_name(),
               over_hit_iso={k: round(v / med["hit_iso"], 3) for k, v in med.items() if k.endswith("hit") or k.endswith("hit_occ")},
               over_mpr_slab={k: round(v / med["mpr_slab"], 3) for k, v in med.items() if k.startswith("mask_slice")},
               rows=rows)
    path = write(res, args, name)
    print(json.dumps(dict(out=path, occupancy=om, ms=med), default=lambda o: o.item()), flush=True)
    if args.host and name == "c3":
        t0 = time.perf_counter()
        hm = mask.cpu().numpy()
        t1 = time.perf_counter()
        res["host_path"] = dict(read_mask_ms=round((t1 - t0) * 1e3, 1), set_voxels=int(np.count_nonzero(hm)),
                                agrees_with_device=int(np.count_nonzero(hm)) == om["matching"])
        assert res["host_path"]["agrees_with_device"]
        write(res, args, name)
        print(json.dumps(dict(host=res["host_path"])), flush=True)
    rp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: the next free profiles/rNN/mview")
    ap.add_argument("--config", choices=sorted(CONFIGS), action="append")
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host", action="store_true", help="also time the host path of C3 once")
    args = ap.parse_args()
    if args.out is None:
        args.out = next_free_out()
    for name in args.config or sorted(CONFIGS):
        run(name, args)


if __name__ == "__main__":
    main()
