"""Minimum- and mean-intensity projection against MIP (GPU; measurement tool).

For one configuration (volume generated on the device, as bench.py's), the views `fill`
(r = 1.6) and `default` (the reference's camera, r = 3) and two slice boxes -- the whole cube
and `slab`, the central half of the cube along the axis the camera looks along (the thin-slab
case MinIP is for) -- TF-2, one process alternates

    mip_skip0              VR_MODE_MIP at the library's own samples in flight: the yardstick
    minip_skip{0,1}_k{K}   VR_MODE_MINIP, K = 1, 2, 4 (knob mip_inflight), without / with skipping
    mean_skip{0,1}_k{K}    VR_MODE_MEAN, the same

for --rounds rounds; each variant runs --frames serial frames after --warmup warm-up frames and
takes the kernel time from vr_timing_read (HIP events around each launch).  `*_k0` rows run the
library's own choice (proj_inflight).  Bar, without skipping: MinIP and the mean fetch exactly
MIP's samples, so the best K of each should run within MIP's median ms per frame plus MIP's own
round-to-round spread, (max - min) / median, in the same process.  Skipping has no bar: the
rows carry the skipped share of the in-slab samples.

    python tools/proj_bench.py --config c3 --out profiles/r11/proj

writes <out>/<config>.json.  Configurations: c3 512^3 f32 at 1920x1080, c2 256^3 u8 at
1024x1024, c4 1024^3 u8 at 2048x2048.
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

CONFIGS = {
    "c3": dict(n=512, dtype="float32", size=(1920, 1080)),
    "c2": dict(n=256, dtype="uint8", size=(1024, 1024)),
    "c4": dict(n=1024, dtype="uint8", size=(2048, 2048)),
}
VIEWS = {"fill": dict(radius=1.6, rotate=None), "default": dict(radius=3.0, rotate=None)}
KS = (1, 2, 4)
MODES = {"minip": vr_amd.MODE_MINIP, "mean": vr_amd.MODE_MEAN}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "proj"))
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    cfg = CONFIGS[args.config]
    W, H = cfg["size"]
    rp = vr_amd.OffscreenPass(W, H)
    rp.generate_volume((cfg["n"],) * 3, np.dtype(cfg["dtype"]), seed=2024)
    rp.transfer_function_changed(synth.tf2())
    out = torch.empty((H + 16, W), dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def run(cam, p):
        for _ in range(args.warmup):
            rp.render_device(cam, p, out.data_ptr(), vr_amd.OUT_RGBA8, 16, 0, 1, stream)
        torch.cuda.synchronize()
        rp.timing_reset()
        rp.timing_enable(True)
        for _ in range(args.frames):
            rp.render_device(cam, p, out.data_ptr(), vr_amd.OUT_RGBA8, 16, 0, 1, stream)
        ms, n = rp.timing_read()
        rp.timing_enable(False)
        return ms / n

    # (name, mode, skip_empty, mip_inflight knob (0: the library's own choice))
    variants = [("mip_skip0", vr_amd.MODE_MIP, 0, 0)]
    for mname, mode in MODES.items():
        for skip in (0, 1):
            variants += [(f"{mname}_skip{skip}_k{k}", mode, skip, k) for k in (0,) + KS]

    def select(mode, k):
        rp.render_mode_changed(mode)
        rp.set_knob("mip_inflight", k)
    res = dict(config=args.config, volume=f"{cfg['n']}^3 {cfg['dtype']}", frame=f"{W}x{H}", tf="tf2",
               frames=args.frames, warmup=args.warmup, rounds=args.rounds,
               code_hash=vr_amd.kernel_code_hash(), views={})
    for vname, v in VIEWS.items():
        cam = vr_amd.make_camera(**v).to_vr_camera()
        axis = int(np.argmax(np.abs(np.asarray(list(cam.position)[:3], dtype=np.float64))))
        slab = ([0.0] * 3, [1.0] * 3)
        slab[0][axis], slab[1][axis] = 0.25, 0.75
        for bname, box in (("full", ([0.0] * 3, [1.0] * 3)), ("slab", slab)):
            rp.slicing_changed(tuple(box[0]), tuple(box[1]))
            rows = {}
            for name, mode, skip, k in variants:
                select(mode, k)
                p = vr_amd.default_params(skip_empty=skip)
                rp.prepare(cam, p)
                st = rp.count_work(cam, p)
                rows[name] = dict(kernel=rp.kernel_name(p), rays=st["rays"], samples=st["samples"],
                                  skipped_samples=st["skipped_samples"],
                                  in_slab=st["samples"] + st["skipped_samples"], ms_rounds=[])
            for _ in range(args.rounds):  # alternate the variants inside every round
                for name, mode, skip, k in variants:
                    select(mode, k)
                    rows[name]["ms_rounds"].append(round(run(cam, vr_amd.default_params(skip_empty=skip)), 5))
            for r in rows.values():
                ms = r["ms_rounds"]
                r["ms_median"] = statistics.median(ms)
                r["spread"] = round((max(ms) - min(ms)) / r["ms_median"], 4)
                r["skipped_share"] = round(r["skipped_samples"] / max(r["in_slab"], 1), 4)
            mip = rows["mip_skip0"]
            bound = mip["ms_median"] * (1.0 + mip["spread"])
            summary = dict(variants=rows, slab_axis=axis, box=box, mip_ms=mip["ms_median"],
                           bound_ms=round(bound, 5))
            for mname in MODES:
                assert rows[f"{mname}_skip0_k1"]["in_slab"] == mip["in_slab"]  # MIP's samples exactly
                for skip in (0, 1):
                    best = min(KS, key=lambda k: rows[f"{mname}_skip{skip}_k{k}"]["ms_median"])
                    summary[f"{mname}_skip{skip}_best_k"] = best
                    summary[f"{mname}_skip{skip}_best_ms"] = rows[f"{mname}_skip{skip}_k{best}"]["ms_median"]
                    summary[f"{mname}_skip{skip}_auto_ms"] = rows[f"{mname}_skip{skip}_k0"]["ms_median"]
                summary[f"{mname}_within_bound"] = bool(summary[f"{mname}_skip0_best_ms"] <= bound)
                summary[f"{mname}_auto_within_bound"] = bool(summary[f"{mname}_skip0_auto_ms"] <= bound)
            res["views"][f"{vname}_{bname}"] = summary
            print(vname, bname, json.dumps({n: (r["ms_median"], r["spread"], r["skipped_share"])
                                            for n, r in rows.items()}), flush=True)
    rp.close()
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, args.config + ".json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(config=args.config, out=path,
                          **{v: {k: r[k] for k in r if k not in ("variants", "box")}
                             for v, r in res["views"].items()})))


if __name__ == "__main__":
    main()
