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

import json

import range_bench as rb
from range_bench import KS, vr_amd


def main():
    b = rb.Bench(("profiles", "r07", "mip"))
    rp = b.rp
    # (name, mode, skip_empty, mip_inflight knob (0: the library's own choice), alt_geometry knob)
    variants = [("composite", vr_amd.MODE_COMPOSITE, 0, 0, -1)]
    if b.f32:  # the composite on the 8^3 bricks MIP reads (no alternative copy)
        variants.append(("composite_base_bricks", vr_amd.MODE_COMPOSITE, 0, 0, 0))
    for skip in (0, 1):
        variants += [(f"mip_skip{skip}_k{k}", vr_amd.MODE_MIP, skip, k, -1) for k in (0,) + KS]

    def select(mode, skip, k, alt):
        rp.render_mode_changed(mode)
        rp.set_knob("mip_inflight", k)
        rp.set_knob("alt_geometry", alt)

    for vname, cam in rb.cameras():
        rows = b.measure(cam, variants, select, lambda mode, skip, k, alt: vr_amd.default_params(skip_empty=skip),
                         lambda cam, p, *v: rb.work_counts(rp.count_work(cam, p)))
        for r in rows.values():
            r["gsamples_in_slab_s"] = round(r["in_slab"] / (r["ms_median"] * 1e-3) / 1e9, 2)
        bound = rb.bound_ms(rows["composite"])
        mip = rows["mip_skip0_k0"]
        auto_k = rb.auto_k(rows, "mip")
        b.res["views"][vname] = dict(
            variants=rows, auto_k_skip0=auto_k[0], auto_k_skip1=auto_k[1], bound_ms=round(bound, 5),
            mip_skip0_ms=mip["ms_median"], mip_skip1_ms=rows["mip_skip1_k0"]["ms_median"],
            mip_within_bound=bool(mip["ms_median"] <= bound),
            best_k_skip0=rb.best_k(rows, "mip_skip0"), best_k_skip1=rb.best_k(rows, "mip_skip1"))
        print(vname, json.dumps({n: (r["ms_median"], r["spread"]) for n, r in rows.items()}), flush=True)
    b.write(lambda views: {v: dict(composite=r["variants"]["composite"]["ms_median"], bound=r["bound_ms"],
                                   mip=r["mip_skip0_ms"], mip_skip=r["mip_skip1_ms"], ok=r["mip_within_bound"])
                           for v, r in views.items()})


if __name__ == "__main__":
    main()
