"""Isosurface extraction against the histogram pass over the same bricks (GPU; measurement tool).

On the C3 volume (512^3 f32 from vr_generate_volume) and on C4 (1024^3 u8), at the isovalue at 0.3
of the data range, one process times

    hist_256          vr_histogram with 256 bins over the data range: the pass that reads exactly
                      the bricks the classify pass reads, decoding one element per voxel
    mesh_count        vr_mesh_count: mesh_classify_kernel and the two scans (one timed interval)
    mesh_extract      vr_mesh_extract_device with normals: the count's interval and the interval
                      of the two emit passes (mesh_vertex_kernel<.., true>, mesh_quad_kernel)
    mesh_extract_n0   the same without normals

A round runs --frames calls of a row after --warmup warm-up calls and takes the kernel time from
vr_timing_read (HIP events around the intervals); the rows alternate inside every round, and a
row's figure is the median over --rounds rounds.  emit_ms = mesh_extract - mesh_count per round.
The counts and the bytes written are recorded beside them, and --host also times, once, the host
path the call replaces: vr_debug_read_volume and the numpy reference tests/mesh_ref.py.

    python tools/mesh_bench.py --out profiles/r17/mesh

writes <out>/c3.json and <out>/c4.json and prints one JSON line per configuration.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("volumetric-renderer_amd", "tools", "tests", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, sub))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import vr_amd  # noqa: E402

CONFIGS = {"c3": (512, np.float32), "c4": (1024, np.uint8)}
ISO_F = 0.3


def run(name, args):
    n, dtype = CONFIGS[name]
    rp = vr_amd.OffscreenPass(64, 64)
    lo, hi = rp.generate_volume((n,) * 3, dtype, seed=2024)
    iso = float(np.float32(lo + ISO_F * (hi - lo)))
    info = rp.mesh_count(iso)
    classify = rp.last_kernel_name()
    nv, nt = info["vertices"], info["triangles"]
    verts = torch.empty((max(nv, 1), 6), dtype=torch.int32, device="cuda")
    tris = torch.empty((max(nt, 1), 3), dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def timed(call, frames, per_call):
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        rp.timing_reset()
        rp.timing_enable(True)
        for _ in range(frames):
            call()
        ms, cnt = rp.timing_read()
        rp.timing_enable(False)
        assert cnt == frames * per_call, (cnt, frames, per_call)
        return ms / frames

    emit_intervals = 1 if nv else 0
    rows = {
        "hist_256": dict(call=lambda: rp.histogram(256, lo, hi), per_call=1),
        "mesh_count": dict(call=lambda: rp.mesh_count(iso), per_call=1, kernel=classify),
        "mesh_extract": dict(call=lambda: rp.mesh_device(verts.data_ptr(), nv, tris.data_ptr(), nt, iso,
                                                         True, True, stream=stream),
                             per_call=1 + emit_intervals),
        "mesh_extract_n0": dict(call=lambda: rp.mesh_device(verts.data_ptr(), nv, tris.data_ptr(), nt, iso,
                                                            True, False, stream=stream),
                                per_call=1 + emit_intervals),
    }
    rp.histogram(256, lo, hi)
    rows["hist_256"]["kernel"] = rp.last_kernel_name()
    for r in rows.values():
        r["ms_rounds"] = []
    for _ in range(args.rounds):  # the rows alternate inside every round
        for r in rows.values():
            r["ms_rounds"].append(round(timed(r["call"], args.frames, r["per_call"]), 5))
    for r in rows.values():
        del r["call"], r["per_call"]
        ms = r["ms_rounds"]
        r["ms_median"] = statistics.median(ms)
        r["spread"] = round((max(ms) - min(ms)) / r["ms_median"], 4)
    med = {k: r["ms_median"] for k, r in rows.items()}
    emit = [round(a - b, 5) for a, b in zip(rows["mesh_extract"]["ms_rounds"], rows["mesh_count"]["ms_rounds"])]
    emit_n0 = [round(a - b, 5) for a, b in zip(rows["mesh_extract_n0"]["ms_rounds"], rows["mesh_count"]["ms_rounds"])]
    res = dict(config=name, volume=f"{n}^3 {np.dtype(dtype).name}", data_range=[lo, hi], isovalue=iso,
               closed=1, counts=info, bytes_written=24 * nv + 12 * nt, frames=args.frames, warmup=args.warmup,
               rounds=args.rounds, device=torch.cuda.get_device_name(0), code_hash=vr_amd.kernel_code_hash(),
               count_over_hist=round(med["mesh_count"] / med["hist_256"], 3),
               emit_ms_median=statistics.median(emit), emit_n0_ms_median=statistics.median(emit_n0), rows=rows)
    if args.host:
        t0 = time.perf_counter()
        vol = rp.read_volume()
        t1 = time.perf_counter()
        import mesh_ref
        m = mesh_ref.extract(vol, iso, True, False)
        t2 = time.perf_counter()
        assert m.info == info, (m.info, info)
        res["host_path"] = dict(read_volume_ms=round((t1 - t0) * 1e3, 1), numpy_reference_ms=round((t2 - t1) * 1e3, 1),
                                normals=0)
    rp.close()
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, f"{name}.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=path, counts=info, count_over_hist=res["count_over_hist"],
                          emit_ms=res["emit_ms_median"], emit_n0_ms=res["emit_n0_ms_median"], ms=med,
                          host=res.get("host_path"))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17", "mesh"))
    ap.add_argument("--config", choices=sorted(CONFIGS), action="append")
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host", action="store_true", help="also time the host path once (slow)")
    args = ap.parse_args()
    for name in args.config or sorted(CONFIGS):
        run(name, args)


if __name__ == "__main__":
    main()
