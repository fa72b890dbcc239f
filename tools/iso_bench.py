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

import json

import numpy as np

import range_bench as rb
from range_bench import KS, vr_amd

FRACTIONS = (0.15, 0.3, 0.6)


def main():
    b = rb.Bench(("profiles", "r08", "iso"), data_range=True)
    rp = b.rp
    # (name, mode, skip_empty, mip_inflight knob (0: the library's own choice))
    variants = [("mip_skip0", vr_amd.MODE_MIP, 0, 0)]
    for skip in (0, 1):
        variants += [(f"iso_skip{skip}_k{k}", vr_amd.MODE_ISO, skip, k) for k in (0,) + KS]

    def select(mode, skip, k):
        rp.render_mode_changed(mode)
        rp.set_knob("mip_inflight", k)

    def params(mode, skip, k):
        return vr_amd.default_params(skip_empty=skip, shading=1 if mode == vr_amd.MODE_ISO else 0)

    def work(cam, p, mode, skip, k):
        if k != 0:
            return {}
        st = rp.count_work(cam, p)  # the work of the policy's rows (K does not change it)
        return dict(rays=st["rays"], samples=st["samples"], skipped_samples=st["skipped_samples"],
                    hits=st["shaded_samples"])

    for vname, cam in rb.cameras():
        b.res["views"][vname] = {}
        for frac in FRACTIONS:
            iso = float(np.float32(b.lo + frac * (b.hi - b.lo)))
            rp.isovalue_changed(iso)
            rows = b.measure(cam, variants, select, params, work)
            mip = rows["mip_skip0"]
            bound = rb.bound_ms(mip)
            auto_k = rb.auto_k(rows, "iso")
            b.res["views"][vname][f"iso_{frac}"] = dict(
                isovalue=iso, variants=rows, auto_k_skip0=auto_k[0], auto_k_skip1=auto_k[1],
                mip_skip0_ms=mip["ms_median"], bound_ms=round(bound, 5),
                iso_skip0_ms=rows["iso_skip0_k0"]["ms_median"], iso_skip1_ms=rows["iso_skip1_k0"]["ms_median"],
                iso_within_bound=bool(rows["iso_skip0_k0"]["ms_median"] <= bound),
                best_k_skip0=rb.best_k(rows, "iso_skip0"), best_k_skip1=rb.best_k(rows, "iso_skip1"))
            print(vname, frac, json.dumps({n: (r["ms_median"], r["spread"]) for n, r in rows.items()}), flush=True)
    b.write(lambda views: {f"{v}/{i}": dict(mip=r["mip_skip0_ms"], bound=r["bound_ms"], iso=r["iso_skip0_ms"],
                                            iso_skip=r["iso_skip1_ms"], ok=r["iso_within_bound"])
                           for v, rows in views.items() for i, r in rows.items()})


if __name__ == "__main__":
    main()
