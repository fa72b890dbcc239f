"""Multi-planar reformat images against a MIP frame (GPU; measurement tool).

On the C3 volume (512^3 f32 from vr_generate_volume, TF-2) one process times 1024x1024 MPR
images (include/vr/vr_mpr.h) at a pitch of one voxel -- the axial, coronal and sagittal planes
and the (1, 1, 1) oblique plane, all through the volume's centre -- as thin slices (nsamples 1)
and as 64-sample slabs, one voxel between samples, once per operator; and, for comparison, the
VR_MODE_MIP frame of the headline camera (r = 1.6, 1920x1080) alternated in the same process.

Every row is run under each tile order (VR_KNOB_TILE_ORDER 1: raster, 3: the frames'
XCD-interleaved super-tiles) so the file holds both sides of that choice (the library's own:
raster for thin slices, super-tiles for slabs; kMprTileOrder in csrc/vr_internal.h).  A round runs
--frames launches of a row (ten times as many of a thin slice) after --warmup warm-up launches
and takes the kernel time from
vr_timing_read (HIP events around each launch); the rows alternate inside every round, and a
row's figure is the median over --rounds rounds.

Per row: ms per image, in-slab samples (vr_mpr_count_work) and Gsamples/s, the bytes of the
bricks the plane's samples touch (its compulsory traffic: every brick holding a sample's cell,
once) and the GB/s that would be if each were read once, and the kernel name.

    python tools/mpr_bench.py --out profiles/r13/mpr

writes <out>/c3.json and prints one JSON line.
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

N, SIZE = 512, 1024
BRICK, PAD, BRICK_BYTES = 8, 2, 729 * 8  # f32 z-pair bricks: 9^3 elements of 8 B (vr_internal.h)
OPS = {"max": vr_amd.OP_MAX, "min": vr_amd.OP_MIN, "mean": vr_amd.OP_MEAN}
ORDERS = {"raster": 1, "supertile": 3}


def planes(nsamples, op):
    """name -> vr_mpr_plane: SIZE x SIZE pixels, one voxel per pixel and per slab sample."""
    v = 1.0 / N
    ex, ey, ez = np.eye(3)
    frames = {  # right, down, normal (vr_mpr_axis_plane's orientations)
        "axial": (ex, ey, ez), "coronal": (ex, -ez, ey), "sagittal": (ey, -ez, ex),
        "oblique": (np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0), np.array([1.0, 1.0, -2.0]) / np.sqrt(6.0),
                    np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)),
    }
    return {name: vr_amd.mpr_plane((0.5, 0.5, 0.5), u * v, d * v, n * v, SIZE, SIZE, nsamples, op)
            for name, (u, d, n) in frames.items()}


def touched_brick_bytes(pl, box=((0, 0, 0), (1, 1, 1))):
    """Bytes of the base bricks that hold the cell of at least one in-slab sample of the plane."""
    f = np.float32
    px = np.arange(pl.width, dtype=np.float64) + 0.5 - 0.5 * pl.width
    py = np.arange(pl.height, dtype=np.float64) + 0.5 - 0.5 * pl.height
    o, du, dv, dn = (np.array(list(getattr(pl, k)), np.float64) for k in ("origin", "du", "dv", "dn"))
    nb = (N + 3) // BRICK + 1
    seen = np.zeros(nb ** 3, bool)
    for s in range(pl.nsamples):
        t = s - 0.5 * (pl.nsamples - 1)
        q = [((o[a] + px[None, :] * du[a]) + py[:, None] * dv[a] + t * dn[a]).astype(f) for a in range(3)]
        inb = np.ones(q[0].shape, bool)
        for a in range(3):
            inb &= (q[a] > f(box[0][a])) & (q[a] < f(box[1][a])) & (q[a] >= 0) & (q[a] <= 1)
        cell = [(np.floor(q[a][inb] * f(N) - f(0.5)).astype(np.int64) + PAD) // BRICK for a in range(3)]
        seen[(cell[2] * nb + cell[1]) * nb + cell[0]] = True
    return int(seen.sum()) * BRICK_BYTES


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "mpr"))
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()

    W, H = 1920, 1080
    rp = vr_amd.OffscreenPass(W, H)
    lo, hi = rp.generate_volume((N,) * 3, np.float32, seed=2024)
    rp.transfer_function_changed(synth.tf2())
    out = torch.empty((max(H + 16, SIZE), max(W, SIZE)), dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    params = vr_amd.default_params()
    cam = vr_amd.make_camera(radius=1.6).to_vr_camera()  # the headline's camera

    def timed(launch, frames):
        for _ in range(args.warmup):
            launch()
        torch.cuda.synchronize()
        rp.timing_reset()
        rp.timing_enable(True)
        for _ in range(frames):
            launch()
        ms, n = rp.timing_read()
        rp.timing_enable(False)
        assert n == frames
        return ms / n

    rows = {}
    rp.render_mode_changed(vr_amd.MODE_MIP)
    rp.prepare(cam, params)
    mip_work = rp.count_work(cam, params)
    rows["mip_frame"] = dict(kernel=rp.kernel_name(params), samples=mip_work["samples"],
                             launch=lambda: rp.render_device(cam, params, out.data_ptr(), vr_amd.OUT_RGBA8,
                                                             16, 0, 1, stream))
    specs = [(1, "max")] + [(64, op) for op in OPS]
    touched = {}  # (plane, nsamples) -> bytes: the operators read the same samples
    for ns, opname in specs:
        for pname, pl in planes(ns, OPS[opname]).items():
            st = rp.count_work_mpr(pl)
            if (pname, ns) not in touched:
                touched[pname, ns] = touched_brick_bytes(pl)
            byts = touched[pname, ns]
            for oname, order in ORDERS.items():
                def launch(pl=pl, order=order):
                    rp.set_knob("tile_order", order)
                    rp.render_mpr_device(pl, params, out.data_ptr(), vr_amd.OUT_RGBA8, stream)
                    rp.set_knob("tile_order", 0)
                launch()
                rows[f"{pname}_n{ns}_{opname}_{oname}"] = dict(
                    kernel=rp.last_kernel_name(), plane=pname, nsamples=ns, op=opname, tile_order=oname,
                    rays=st["rays"], samples=st["samples"], touched_brick_bytes=byts, launch=launch)
    for r in rows.values():
        r["ms_rounds"] = []
    for _ in range(args.rounds):  # the rows alternate inside every round
        for r in rows.values():
            # (a thin slice is a few microseconds: ten times the launches per round)
            r["ms_rounds"].append(round(timed(r["launch"], args.frames * (10 if r.get("nsamples") == 1 else 1)), 5))
    for r in rows.values():
        del r["launch"]
        ms = r["ms_rounds"]
        r["ms_median"] = statistics.median(ms)
        r["spread"] = round((max(ms) - min(ms)) / r["ms_median"], 4)
        r["gsamples_per_s"] = round(r["samples"] / (r["ms_median"] * 1e-3) / 1e9, 2)
        if "touched_brick_bytes" in r:
            r["touched_gb_per_s"] = round(r["touched_brick_bytes"] / (r["ms_median"] * 1e-3) / 1e9, 1)
    rp.close()

    res = dict(config="c3", volume=f"{N}^3 float32", image=f"{SIZE}x{SIZE}", pitch_voxels=1.0,
               mip_frame=f"{W}x{H}, r = 1.6", tf="tf2", data_range=[lo, hi], frames=args.frames,
               warmup=args.warmup, rounds=args.rounds, device=torch.cuda.get_device_name(0),
               code_hash=vr_amd.kernel_code_hash(), rows=rows)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "c3.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=path, **{k: (r["ms_median"], r["gsamples_per_s"]) for k, r in rows.items()})))


if __name__ == "__main__":
    main()
