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

import json

import numpy as np

import range_bench as rb
from range_bench import KS, vr_amd

MODES = {"minip": vr_amd.MODE_MINIP, "mean": vr_amd.MODE_MEAN}


def main():
    b = rb.Bench(("profiles", "r11", "proj"))
    rp = b.rp
    # (name, mode, skip_empty, mip_inflight knob (0: the library's own choice))
    variants = [("mip_skip0", vr_amd.MODE_MIP, 0, 0)]
    for mname, mode in MODES.items():
        for skip in (0, 1):
            variants += [(f"{mname}_skip{skip}_k{k}", mode, skip, k) for k in (0,) + KS]

    def select(mode, skip, k):
        rp.render_mode_changed(mode)
        rp.set_knob("mip_inflight", k)

    for vname, cam in rb.cameras():
        axis = int(np.argmax(np.abs(np.asarray(list(cam.position)[:3], dtype=np.float64))))
        slab = ([0.0] * 3, [1.0] * 3)
        slab[0][axis], slab[1][axis] = 0.25, 0.75
        for bname, box in (("full", ([0.0] * 3, [1.0] * 3)), ("slab", slab)):
            rp.slicing_changed(tuple(box[0]), tuple(box[1]))
            rows = b.measure(cam, variants, select, lambda mode, skip, k: vr_amd.default_params(skip_empty=skip),
                             lambda cam, p, *v: rb.work_counts(rp.count_work(cam, p)))
            mip = rows["mip_skip0"]
            bound = rb.bound_ms(mip)
            summary = dict(variants=rows, slab_axis=axis, box=box, mip_ms=mip["ms_median"],
                           bound_ms=round(bound, 5))
            for mname in MODES:
                assert rows[f"{mname}_skip0_k1"]["in_slab"] == mip["in_slab"]  # MIP's samples exactly
                for skip in (0, 1):
                    best = rb.best_k(rows, f"{mname}_skip{skip}")
                    summary[f"{mname}_skip{skip}_best_k"] = best
                    summary[f"{mname}_skip{skip}_best_ms"] = rows[f"{mname}_skip{skip}_k{best}"]["ms_median"]
                    summary[f"{mname}_skip{skip}_auto_ms"] = rows[f"{mname}_skip{skip}_k0"]["ms_median"]
                summary[f"{mname}_within_bound"] = bool(summary[f"{mname}_skip0_best_ms"] <= bound)
                summary[f"{mname}_auto_within_bound"] = bool(summary[f"{mname}_skip0_auto_ms"] <= bound)
            b.res["views"][f"{vname}_{bname}"] = summary
            print(vname, bname, json.dumps({n: (r["ms_median"], r["spread"], r["skipped_share"])
                                            for n, r in rows.items()}), flush=True)
    b.write(lambda views: {v: {k: r[k] for k in r if k not in ("variants", "box")} for v, r in views.items()})


if __name__ == "__main__":
    main()
