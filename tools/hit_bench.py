"""Hit images and picks against the frames of the same view (GPU; measurement tool).

On the C3 volume (512^3 f32 from vr_generate_volume, 1920x1080) and on C4 (1024^3 u8, 2048x2048),
TF-2, the headline camera (r = 1.6) and the isovalue at 0.3 of the data range, one process times
per kind of include/vr/vr_hit.h (OPACITY at threshold 0.9)

    hit_<kind>_k{1,2}   the whole-frame hit image into device memory (vr_hit_render_device) with
                        one and with two samples of a ray in flight (VR_KNOB_HIT_INFLIGHT): both
                        sides of the choice csrc/vr_internal.h kHitDefaultInFlight makes
    pick_<kind>         a 1 x 1 vr_pick at the centre pixel (the kernel alone: the call's host
                        copy is outside the timing events)

and, for comparison, the existing frames alternated in the same process: the VR_MODE_MIP frame
with skip_empty = 0, and the VR_MODE_ISO frame with skip_empty = 0 at the same isovalue, unshaded
and shaded.  A round runs --frames launches of a row after --warmup warm-up launches and takes
the kernel time from vr_timing_read (HIP events around each launch); the rows alternate inside
every round, and a row's figure is the median over --rounds rounds.

    python tools/hit_bench.py --out profiles/r16/hit

writes <out>/c3.json and <out>/c4.json and prints one JSON line per configuration.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("volumetric-renderer_amd", "tools"):
    sys.path.insert(0, os.path.join(ROOT, sub))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import synth  # noqa: E402
import vr_amd  # noqa: E402

CONFIGS = {"c3": (512, np.float32, 1920, 1080), "c4": (1024, np.uint8, 2048, 2048)}
KINDS = {"entry": vr_amd.HIT_ENTRY, "opacity": vr_amd.HIT_OPACITY, "max": vr_amd.HIT_MAX,
         "min": vr_amd.HIT_MIN, "iso": vr_amd.HIT_ISO}
THRESHOLD, ISO_F = 0.9, 0.3


def run(name, args):
    n, dtype, W, H = CONFIGS[name]
    rp = vr_amd.OffscreenPass(W, H)
    lo, hi = rp.generate_volume((n,) * 3, dtype, seed=2024)
    rp.transfer_function_changed(synth.tf2())
    iso = float(np.float32(lo + ISO_F * (hi - lo)))
    rp.isovalue_changed(iso)
    frame = torch.empty((H + 16, W), dtype=torch.int32, device="cuda")
    records = torch.empty((H, W, 6), dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    cam = vr_amd.make_camera(radius=1.6).to_vr_camera()  # the headline's camera
    plain = vr_amd.default_params(skip_empty=0)

    def timed(launch, frames):
        for _ in range(args.warmup):
            launch()
        torch.cuda.synchronize()
        rp.timing_reset()
        rp.timing_enable(True)
        for _ in range(frames):
            launch()
        ms, cnt = rp.timing_read()
        rp.timing_enable(False)
        assert cnt == frames
        return ms / cnt

    rows = {}

    def frame_row(label, mode, params):
        def launch():
            rp.render_mode_changed(mode)
            rp.render_device(cam, params, frame.data_ptr(), vr_amd.OUT_RGBA8, 16, 0, 1, stream)
        launch()
        kernel = rp.last_kernel_name()
        st = rp.count_work(cam, params)
        rows[label] = dict(kernel=kernel, rays=st["rays"], samples=st["samples"], launch=launch)

    frame_row("mip_frame_skip0", vr_amd.MODE_MIP, plain)
    frame_row("iso_frame_skip0", vr_amd.MODE_ISO, plain)
    frame_row("iso_frame_skip0_shaded", vr_amd.MODE_ISO, vr_amd.default_params(skip_empty=0, shading=1))
    rp.render_mode_changed(vr_amd.MODE_COMPOSITE)
    for kname, kind in KINDS.items():
        st = rp.hit_count_work(cam, plain, kind, THRESHOLD)
        for k in (1, 2):
            def launch(kind=kind, k=k):
                rp.set_knob("hit_inflight", k)
                rp.hit_image_device(cam, plain, kind, records.data_ptr(), THRESHOLD, stream=stream)
                rp.set_knob("hit_inflight", -1)
            launch()
            rows[f"hit_{kname}_k{k}"] = dict(kernel=rp.last_kernel_name(), kind=kname, inflight=k,
                                             rays=st["rays"], samples=st["samples"],
                                             hits=st["shaded_samples"], launch=launch)

        def pick(kind=kind):
            rp.pick(cam, plain, W // 2, H // 2, kind, THRESHOLD)
        pick()
        rows[f"pick_{kname}"] = dict(kernel=rp.last_kernel_name(), kind=kname, pixel=[W // 2, H // 2],
                                     launch=pick)
    for r in rows.values():
        r["ms_rounds"] = []
    for _ in range(args.rounds):  # the rows alternate inside every round
        for r in rows.values():
            r["ms_rounds"].append(round(timed(r["launch"], args.frames), 5))
    for r in rows.values():
        del r["launch"]
        ms = r["ms_rounds"]
        r["ms_median"] = statistics.median(ms)
        r["spread"] = round((max(ms) - min(ms)) / r["ms_median"], 4)
        if "samples" in r:
            r["gsamples_per_s"] = round(r["samples"] / (r["ms_median"] * 1e-3) / 1e9, 2)
    rp.close()

    med = {k: r["ms_median"] for k, r in rows.items()}
    best = {kname: min((1, 2), key=lambda k: med[f"hit_{kname}_k{k}"]) for kname in KINDS}
    shipped = {kname: min(med[f"hit_{kname}_k1"], med[f"hit_{kname}_k2"]) for kname in KINDS}
    res = dict(config=name, volume=f"{n}^3 {np.dtype(dtype).name}", image=f"{W}x{H}", camera="r = 1.6",
               tf="tf2", data_range=[lo, hi], isovalue=iso, opacity_threshold=THRESHOLD, frames=args.frames,
               warmup=args.warmup, rounds=args.rounds, device=torch.cuda.get_device_name(0),
               code_hash=vr_amd.kernel_code_hash(), faster_inflight=best,
               max_over_mip_frame=round(shipped["max"] / med["mip_frame_skip0"], 3),
               iso_over_iso_frame=round(shipped["iso"] / med["iso_frame_skip0"], 3), rows=rows)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, f"{name}.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=path, faster_inflight=best, max_over_mip_frame=res["max_over_mip_frame"],
                          iso_over_iso_frame=res["iso_over_iso_frame"], ms=med)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "hit"))
    ap.add_argument("--config", choices=sorted(CONFIGS), action="append")
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    for name in args.config or sorted(CONFIGS):
        run(name, args)


if __name__ == "__main__":
    main()
