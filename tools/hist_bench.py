"""The device-side volume histogram (include/vr/vr_hist.h) on the benchmark volumes (GPU;
measurement tool).

Per configuration (c3: 512^3 f32, c4: 1024^3 u8, c5: 2048^3 u8, bench.py's volumes) one process
holds two contexts -- the synthetic Gaussians (vr_generate_volume) and a constant volume of the
same size and type, the hot-bin case, uploaded from a device tensor -- and times vr_histogram over
the data's range with 256 and 4096 bins, in both kernel forms (knob hist_agg 0: every lane adds to
its bin's LDS counter; 1: the lanes that share the wave's leading bin add once), on the whole
volume of both and on a half-volume box of the Gaussians.  The rows alternate inside every round;
a round runs --reps calls of a row after --warmup warm-up calls, takes the kernel time from
vr_timing_read (HIP events around the kernel) and the wall time of the synchronous call from the
host clock; a row's figures are the medians over --rounds rounds.

Per row: kernel ms, wall ms, the bricks' bytes (vr_volume_bytes; the box rows: the bytes of the
bricks the box touches) over the kernel time in GB/s and as a share of the 8 TB/s HBM peak, and
voxels per second.  Every call's counts are checked (sum(bins) + below + above + nan == the box's
voxels).  --replaces also times what the call replaces, once: read_volume(native=True) and
numpy.histogram on the host.

    python tools/hist_bench.py --config c3 --out profiles/r15/hist --replaces

writes <out>/<config>.json and prints one JSON line.  --range-frame renders one skip_empty frame,
takes one 256-bin histogram and exits: run under a kernel trace, it gives the duration of
brick_range_kernel, the existing kernel that also reads every brick once, beside hist_kernel's.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("volumetric-renderer_amd", "tools"):
    sys.path.insert(0, os.path.join(ROOT, sub))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import synth  # noqa: E402
import vr_amd  # noqa: E402

CONFIGS = {"c3": ((512,) * 3, np.float32, 2024), "c4": ((1024,) * 3, np.uint8, 7),
           "c5": ((2048,) * 3, np.uint8, 7)}
HBM_PEAK = 8.0e12


def box_brick_bytes(rp, box, dims):
    """Bytes of the base bricks that hold the box's voxels (hist_kernel reads no others)."""
    st = rp.volume_info()[2]
    plain_byte = st in (0, 1) and int(np.prod(dims)) > (1 << 25)
    cells = (7, 8, 8) if plain_byte else (8, 8, 8)
    elem = 1 if plain_byte else (4 if st in (0, 1) else 8)
    per_brick = (cells[0] + 1) * (cells[1] + 1) * (cells[2] + 1) * elem
    n = 1
    for a in range(3):
        n *= (box[1][a] - 1 + 2) // cells[a] - (box[0][a] + 2) // cells[a] + 1
    return n * per_brick


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "hist"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replaces", action="store_true")
    ap.add_argument("--range-frame", action="store_true")
    args = ap.parse_args()
    dims, dtype, seed = CONFIGS[args.config]
    nvox = int(np.prod(dims))

    gauss = vr_amd.OffscreenPass(256, 256)
    lo, hi = gauss.generate_volume(dims, dtype, seed=seed)
    if args.range_frame:
        gauss.transfer_function_changed(synth.tf2())
        gauss.render(vr_amd.make_camera(radius=1.6).to_vr_camera(), vr_amd.default_params(skip_empty=1))
        gauss.histogram(256, lo, hi)  # (the same trace then holds both kernels)
        print(json.dumps(dict(config=args.config, range_frame=True, volume_bytes=gauss.volume_bytes())))
        gauss.close()
        return
    const = vr_amd.OffscreenPass(256, 256)
    value = 0.25 * (lo + hi) if dtype == np.float32 else int(0.25 * (lo + hi))
    t = torch.full((dims[2], dims[1], dims[0]), value,
                   dtype=torch.float32 if dtype == np.float32 else torch.uint8, device="cuda")
    torch.cuda.synchronize()
    const.set_knob("narrow", 0)  # a constant f32 volume stays f32, as the Gaussians are
    const.volume_dataset_changed_device(t.data_ptr(), dtype, dims, lo, hi)
    del t
    torch.cuda.empty_cache()
    assert const.volume_info()[2] == gauss.volume_info()[2]
    half = ((0, 0, 0), (dims[0], dims[1], dims[2] // 2))

    rows = {}
    for dist, rp, box in (("gaussians", gauss, None), ("constant", const, None), ("half_box", gauss, half)):
        for nbins in (256, 4096):
            for agg in (0, 1):
                rows[f"{dist}_b{nbins}_{'agg' if agg else 'plain'}"] = dict(
                    distribution=dist, nbins=nbins, form="aggregated" if agg else "plain", rp=rp, box=box, agg=agg,
                    voxels=nvox if box is None else nvox // 2,
                    brick_bytes=rp.volume_bytes() if box is None else box_brick_bytes(rp, box, dims),
                    kernel_ms_rounds=[], wall_ms_rounds=[])

    def timed(r, reps):
        rp = r["rp"]
        rp.set_knob("hist_agg", r["agg"])
        for _ in range(args.warmup):
            rp.histogram(r["nbins"], lo, hi, r["box"])
        rp.timing_reset()
        rp.timing_enable(True)
        t0 = time.perf_counter()
        for _ in range(reps):
            bins, info = rp.histogram(r["nbins"], lo, hi, r["box"])
        wall = (time.perf_counter() - t0) * 1e3 / reps
        ms, n = rp.timing_read()
        rp.timing_enable(False)
        rp.set_knob("hist_agg", -1)
        assert n == reps
        total = int(bins.sum()) + info["below"] + info["above"] + info["nan"]
        assert total == info["voxels"] == r["voxels"], (total, info, r["voxels"])
        r["kernel"] = rp.last_kernel_name()
        r["max_bin_share"] = round(float(bins.max()) / r["voxels"], 4)
        return ms / n, wall

    for _ in range(args.rounds):  # the rows alternate inside every round
        for r in rows.values():
            k, w = timed(r, args.reps)
            r["kernel_ms_rounds"].append(round(k, 5))
            r["wall_ms_rounds"].append(round(w, 5))
    for r in rows.values():
        for key in ("rp", "box", "agg"):
            del r[key]
        k = r["kernel_ms"] = statistics.median(r["kernel_ms_rounds"])
        r["wall_ms"] = statistics.median(r["wall_ms_rounds"])
        r["spread"] = round((max(r["kernel_ms_rounds"]) - min(r["kernel_ms_rounds"])) / k, 4)
        r["brick_gb_per_s"] = round(r["brick_bytes"] / (k * 1e-3) / 1e9, 1)
        r["share_of_hbm_peak"] = round(r["brick_bytes"] / (k * 1e-3) / HBM_PEAK, 4)
        r["gvoxels_per_s"] = round(r["voxels"] / (k * 1e-3) / 1e9, 2)

    replaces = None
    if args.replaces:
        t0 = time.perf_counter()
        vol = gauss.read_volume(native=True)
        t1 = time.perf_counter()
        ref, _ = np.histogram(vol, bins=256, range=(lo, hi))
        t2 = time.perf_counter()
        replaces = dict(read_volume_ms=round((t1 - t0) * 1e3, 1), numpy_histogram_256_ms=round((t2 - t1) * 1e3, 1),
                        voxels_counted=int(ref.sum()))
        del vol
    res = dict(config=args.config, volume=f"{dims[0]}x{dims[1]}x{dims[2]} {np.dtype(dtype).name}",
               volume_bytes=gauss.volume_bytes(), data_range=[lo, hi], constant_value=float(value),
               reps=args.reps, warmup=args.warmup, rounds=args.rounds, hbm_peak_bytes_per_s=HBM_PEAK,
               device=torch.cuda.get_device_name(0), code_hash=vr_amd.kernel_code_hash(),
               host_read_and_numpy=replaces, rows=rows)
    gauss.close()
    const.close()
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, f"{args.config}.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=path, replaces=replaces,
                          **{k: (r["kernel_ms"], r["wall_ms"], r["share_of_hbm_peak"]) for k, r in rows.items()})))


if __name__ == "__main__":
    main()
