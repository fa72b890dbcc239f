"""First-hit isosurface against maximum-intensity projection (GPU; measurement tool).

For one configuration (volume generated on the device, as bench.py's), the views `fill`
(r = 1.6) and `default` (the reference's camera, r = 3), TF-2 and the isovalues at 0.15, 0.3
and 0.6 of the data range (a surface near the entry, in the middle, mostly empty space), one
process alternates

    iso_skip0_k{1,2,4}   VR_MODE_ISO, shaded, every search sample fetched, K samples in flight
    iso_skip1_k{1,2,4}   the same with range skipping (skip_empty = 1)
    iso_skip{0,1}_k0     the library's own K (iso_inflight; `auto_k_*` names it)
    mip_skip0            VR_MODE_MIP, every sample fetched, the library's own K: the yardstick

for --rounds rounds; each variant runs --frames serial frames after --warmup warm-up frames and
takes the kernel time from vr_timing_read (HIP events around each launch).  Yardstick: an ISO
search fetches a prefix of the samples MIP fetches on the same ray, plus at most four
refinement fetches and one gradient per ray, so iso_skip0 at the library's K should take at
most MIP's median ms per frame plus MIP's own round-to-round spread, (max - min) / median.

    python tools/iso_bench.py --config c3 --out profiles/r08/iso

writes <out>/<config>.json.  Configurations: c3 512^3 f32 at 1920x1080, c2 256^3 u8 at
1024x1024, c4 1024^3 u8 at 2048x2048.
"""
from __future__ import annotations

import argparse
import json
import os
import re
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
FRACTIONS = (0.15, 0.3, 0.6)
KS = (1, 2, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "iso"))
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    cfg = CONFIGS[args.config]
    W, H = cfg["size"]
    rp = vr_amd.OffscreenPass(W, H)
    lo, hi = rp.generate_volume((cfg["n"],) * 3, np.dtype(cfg["dtype"]), seed=2024)
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
    for skip in (0, 1):
        variants += [(f"iso_skip{skip}_k{k}", vr_amd.MODE_ISO, skip, k) for k in (0,) + KS]

    def select(mode, k):
        rp.render_mode_changed(mode)
        rp.set_knob("mip_inflight", k)

    def params(mode, skip):
        return vr_amd.default_params(skip_empty=skip, shading=1 if mode == vr_amd.MODE_ISO else 0)

    res = dict(config=args.config, volume=f"{cfg['n']}^3 {cfg['dtype']}", frame=f"{W}x{H}", tf="tf2",
               data_range=[lo, hi], frames=args.frames, warmup=args.warmup, rounds=args.rounds,
               code_hash=vr_amd.kernel_code_hash(), views={})
    for vname, v in VIEWS.items():
        cam = vr_amd.make_camera(**v).to_vr_camera()
        res["views"][vname] = {}
        for frac in FRACTIONS:
            iso = float(np.float32(lo + frac * (hi - lo)))
            rp.isovalue_changed(iso)
            rows = {}
            for name, mode, skip, k in variants:
                select(mode, k)
                p = params(mode, skip)
                rp.prepare(cam, p)
                rows[name] = dict(kernel=rp.kernel_name(p), ms_rounds=[])
                if k == 0:  # the work of the policy's rows (K does not change it)
                    st = rp.count_work(cam, p)
                    rows[name].update(rays=st["rays"], samples=st["samples"],
                                      skipped_samples=st["skipped_samples"], hits=st["shaded_samples"])
            for _ in range(args.rounds):  # alternate the variants inside every round
                for name, mode, skip, k in variants:
                    select(mode, k)
                    rows[name]["ms_rounds"].append(round(run(cam, params(mode, skip)), 5))
            for r in rows.values():
                ms = r["ms_rounds"]
                r["ms_median"] = statistics.median(ms)
                r["spread"] = round((max(ms) - min(ms)) / r["ms_median"], 4)
            mip = rows["mip_skip0"]
            bound = mip["ms_median"] * (1.0 + mip["spread"])
            auto_k = [int(re.search(r", (\d)>\(", rows[f"iso_skip{s}_k0"]["kernel"]).group(1)) for s in (0, 1)]
            res["views"][vname][f"iso_{frac}"] = dict(
                isovalue=iso, variants=rows, auto_k_skip0=auto_k[0], auto_k_skip1=auto_k[1],
                mip_skip0_ms=mip["ms_median"], bound_ms=round(bound, 5),
                iso_skip0_ms=rows["iso_skip0_k0"]["ms_median"], iso_skip1_ms=rows["iso_skip1_k0"]["ms_median"],
                iso_within_bound=bool(rows["iso_skip0_k0"]["ms_median"] <= bound),
                best_k_skip0=min(KS, key=lambda k: rows[f"iso_skip0_k{k}"]["ms_median"]),
                best_k_skip1=min(KS, key=lambda k: rows[f"iso_skip1_k{k}"]["ms_median"]))
            print(vname, frac, json.dumps({n: (r["ms_median"], r["spread"]) for n, r in rows.items()}), flush=True)
    rp.close()
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, args.config + ".json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(config=args.config, out=path,
                          **{f"{v}/{i}": dict(mip=r["mip_skip0_ms"], bound=r["bound_ms"], iso=r["iso_skip0_ms"],
                                              iso_skip=r["iso_skip1_ms"], ok=r["iso_within_bound"])
                             for v, rows in res["views"].items() for i, r in rows.items()})))


if __name__ == "__main__":
    main()
