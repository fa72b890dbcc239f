"""Maximum-intensity projection against the composite kernel (GPU; measurement tool).

For one configuration (volume generated on the device, as bench.py's) and the views `fill`
(r = 1.6) and `default` (the reference's camera, r = 3), TF-2, one process alternates

    composite        unshaded, no ERT, no skip-empty (the kernel the launch policy picks)
    mip_skip0        VR_MODE_MIP, every sample fetched
    mip_skip1        VR_MODE_MIP with range skipping (skip_empty = 1)

for --rounds rounds; each variant runs --frames serial frames after --warmup warm-up frames and
takes the kernel time from vr_timing_read (HIP events around each launch).  The MIP variants run
once per samples-in-flight count K (knob mip_inflight: 1, 2, 4) and once with the library's own
choice (`_k0`, the figure the yardstick takes; `auto_k_*` names it), so the file also holds the
K A/B.  f32 configurations add `composite_base_bricks`, the composite kept on the 8^3 bricks MIP
reads (knob alt_geometry = 0).  Yardstick (the issue's): MIP without
skipping takes the composite's positions and fetches with less arithmetic, so its median ms per
frame should be at most the composite's plus the composite's own round-to-round spread,
(max - min) / median.

    python tools/mip_bench.py --config c3 --out profiles/r07/mip

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
KS = (1, 2, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "mip"))
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

    # (name, mode, skip_empty, mip_inflight knob (0: the library's own choice), alt_geometry knob)
    variants = [("composite", vr_amd.MODE_COMPOSITE, 0, 0, -1)]
    if cfg["dtype"] == "float32":  # the composite on the 8^3 bricks MIP reads (no alternative copy)
        variants.append(("composite_base_bricks", vr_amd.MODE_COMPOSITE, 0, 0, 0))
    for skip in (0, 1):
        variants += [(f"mip_skip{skip}_k{k}", vr_amd.MODE_MIP, skip, k, -1) for k in (0,) + KS]

    def select(mode, k, alt):
        rp.render_mode_changed(mode)
        rp.set_knob("mip_inflight", k)
        rp.set_knob("alt_geometry", alt)
    res = dict(config=args.config, volume=f"{cfg['n']}^3 {cfg['dtype']}", frame=f"{W}x{H}", tf="tf2",
               frames=args.frames, warmup=args.warmup, rounds=args.rounds,
               code_hash=vr_amd.kernel_code_hash(), views={})
    for vname, v in VIEWS.items():
        cam = vr_amd.make_camera(**v).to_vr_camera()
        rows = {}
        for name, mode, skip, k, alt in variants:
            select(mode, k, alt)
            p = vr_amd.default_params(skip_empty=skip)
            rp.prepare(cam, p)
            st = rp.count_work(cam, p)
            rows[name] = dict(kernel=rp.kernel_name(p), rays=st["rays"], samples=st["samples"],
                              skipped_samples=st["skipped_samples"],
                              in_slab=st["samples"] + st["skipped_samples"], ms_rounds=[])
        for _ in range(args.rounds):  # alternate the variants inside every round
            for name, mode, skip, k, alt in variants:
                select(mode, k, alt)
                rows[name]["ms_rounds"].append(round(run(cam, vr_amd.default_params(skip_empty=skip)), 5))
        for r in rows.values():
            ms = r["ms_rounds"]
            r["ms_median"] = statistics.median(ms)
            r["spread"] = round((max(ms) - min(ms)) / r["ms_median"], 4)
            r["gsamples_in_slab_s"] = round(r["in_slab"] / (r["ms_median"] * 1e-3) / 1e9, 2)
            r["skipped_share"] = round(r["skipped_samples"] / max(r["in_slab"], 1), 4)
        comp = rows["composite"]
        bound = comp["ms_median"] * (1.0 + comp["spread"])
        mip = rows["mip_skip0_k0"]
        auto_k = [int(re.search(r", (\d)>\(", rows[f"mip_skip{s}_k0"]["kernel"]).group(1)) for s in (0, 1)]
        res["views"][vname] = dict(
            variants=rows, auto_k_skip0=auto_k[0], auto_k_skip1=auto_k[1], bound_ms=round(bound, 5),
            mip_skip0_ms=mip["ms_median"], mip_skip1_ms=rows["mip_skip1_k0"]["ms_median"],
            mip_within_bound=bool(mip["ms_median"] <= bound),
            best_k_skip0=min(KS, key=lambda k: rows[f"mip_skip0_k{k}"]["ms_median"]),
            best_k_skip1=min(KS, key=lambda k: rows[f"mip_skip1_k{k}"]["ms_median"]))
        print(vname, json.dumps({n: (r["ms_median"], r["spread"]) for n, r in rows.items()}), flush=True)
    rp.close()
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, args.config + ".json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(config=args.config, out=path,
                          **{v: dict(composite=r["variants"]["composite"]["ms_median"], bound=r["bound_ms"],
                                     mip=r["mip_skip0_ms"], mip_skip=r["mip_skip1_ms"], ok=r["mip_within_bound"])
                             for v, r in res["views"].items()})))


if __name__ == "__main__":
    main()
