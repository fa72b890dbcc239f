"""Connected components and region growing against the histogram and the mesh count over the same
bricks (GPU; measurement tool).

On the C3 volume (512^3 f32 from vr_generate_volume) and on C4 (1024^3 u8), with the window
[0.3 of the data range, +inf] under 6- and 26-connectivity, one process times

    hist_256          vr_histogram with 256 bins over the data range: one pass over the bricks
    mesh_count        vr_mesh_count at the window's lower bound: classify and the two scans
    label_count_C     vr_label_count: the labelling passes (local, seam, flatten, scan: one timed
                      interval) and the table passes (init, accumulate, largest: another)
    label_device_C    vr_label_components_device: the same two intervals into the caller's buffers
    grow_device_C     vr_region_grow_device from a seed in the largest component: the labelling
                      passes and the mask pass

A round runs --frames calls of a row after --warmup warm-up calls and takes the kernel time from
vr_timing_read (HIP events around the intervals); the rows alternate inside every round, and a
row's figure is the median over --rounds rounds.  vr_timing_read sums a call's intervals; the
passes inside them (local, seam, flatten, scan, table init, accumulate, largest, mask) are read one
by one from vr_debug_label_pass_ms, medians over --frames calls, into "pass_ms".
What can be checked without a reference at this size is checked: the roots of the label array
(label == index + 1) are as many as `components`, the records' voxels sum to in_voxels, and
in_voxels is the histogram's count of the window.  --host also times, once, the host path the
calls replace: vr_debug_read_volume and scipy.ndimage.label (tests/label_ref.py without scipy).

    python tools/label_bench.py --out profiles/r18/label

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
LO_F = 0.3
INF = float("inf")


def count_roots(labels):
    """Voxels whose label is their own index + 1, in slices (no second array of the whole size)."""
    n, roots, step = labels.numel(), 0, 1 << 26
    for a in range(0, n, step):
        b = min(n, a + step)
        idx = torch.arange(a + 1, b + 1, dtype=torch.int64, device=labels.device)
        roots += int((labels[a:b].to(torch.int64) & 0xFFFFFFFF == idx).sum())
    return roots


def run(name, args):
    n, dtype = CONFIGS[name]
    rp = vr_amd.OffscreenPass(64, 64)
    lo, hi = rp.generate_volume((n,) * 3, dtype, seed=2024)
    wlo = float(np.float32(lo + LO_F * (hi - lo)))
    nvox = n ** 3
    stream = torch.cuda.current_stream().cuda_stream
    labels = torch.empty(nvox, dtype=torch.int32, device="cuda")
    mask = torch.empty(nvox, dtype=torch.uint8, device="cuda")
    top = float(np.nextafter(np.float32(hi), np.float32(INF)))
    hist_in = int(rp.histogram(1, wlo, top)[0][0])

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

    rows = {"hist_256": dict(call=lambda: rp.histogram(256, lo, hi), per_call=1),
            "mesh_count": dict(call=lambda: rp.mesh_count(wlo), per_call=1)}
    rp.histogram(256, lo, hi)
    rows["hist_256"]["kernel"] = rp.last_kernel_name()
    rp.mesh_count(wlo)
    rows["mesh_count"]["kernel"] = rp.last_kernel_name()
    checks, counts, scratch, passes = {}, {}, {}, {}

    def pass_ms(call):
        """Median kernel ms of every pass of `call` over --frames calls (vr_debug_label_pass_ms)."""
        rp.timing_enable(True)
        rows_ = []
        for _ in range(args.warmup + args.frames):
            call()
            rows_.append(rp.label_pass_ms())
        rp.timing_reset()
        rp.timing_enable(False)
        return {k: round(statistics.median(r[k] for r in rows_[args.warmup:]), 5) for k in rows_[0]}

    for conn in (6, 26):
        info = rp.label_count(wlo, INF, conn)
        kernel = rp.last_kernel_name()
        nc = info["components"]
        comps = torch.empty((max(nc, 1), 16), dtype=torch.int32, device="cuda")
        dinfo = rp.label_device(labels.data_ptr(), nvox, comps.data_ptr(), nc, wlo, INF, conn, stream=stream)
        rec = comps[:nc].cpu().numpy().view(vr_amd.LABEL_COMPONENT_DTYPE).reshape(-1)
        roots = count_roots(labels)
        checks[str(conn)] = dict(roots=roots, roots_equal_components=roots == nc == len(rec),
                                 records_sum_to_in_voxels=int(rec["voxels"].sum()) == info["in_voxels"],
                                 in_voxels_equal_histogram=info["in_voxels"] == hist_in,
                                 device_info_equals_count=dinfo == info,
                                 records_sorted=bool(np.all(np.diff(rec["label"].astype(np.int64)) > 0)))
        assert all(v is True for k, v in checks[str(conn)].items() if k != "roots"), checks
        counts[str(conn)] = info
        # a seed in the largest component: the voxel of its label (its root)
        l = info["largest_label"] - 1
        seed = (l % n, (l // n) % n, l // (n * n))
        comp = rp.region_grow_device(seed, mask.data_ptr(), nvox, wlo, INF, conn, stream=stream)
        assert comp["voxels"] == info["largest_voxels"] == int(mask.sum(dtype=torch.int64)), (comp, info)
        passes[str(conn)] = dict(label_count=pass_ms(lambda c=conn: rp.label_count(wlo, INF, c)),
                                 grow_device=pass_ms(lambda c=conn, s=seed: rp.region_grow_device(
                                     s, mask.data_ptr(), nvox, wlo, INF, c, stream=stream)))
        scratch[str(conn)] = dict(labels_bytes=4 * nvox, root_table_bytes=12 * ((nvox + 63) // 64) + 4 * ((nvox + 8191) // 8192) + 32,
                                  component_bytes=64 * nc, mask_bytes=nvox)
        table = 1 if nc else 0
        rows[f"label_count_{conn}"] = dict(call=lambda c=conn: rp.label_count(wlo, INF, c), per_call=1 + table,
                                           kernel=kernel)
        rows[f"label_device_{conn}"] = dict(
            call=lambda c=conn, p=comps.data_ptr(), k=nc: rp.label_device(labels.data_ptr(), nvox, p, k, wlo, INF, c,
                                                                          stream=stream),
            per_call=1 + table, keep=comps)
        rows[f"grow_device_{conn}"] = dict(
            call=lambda c=conn, s=seed: rp.region_grow_device(s, mask.data_ptr(), nvox, wlo, INF, c, stream=stream),
            per_call=2)
    for r in rows.values():
        r["ms_rounds"] = []
    for _ in range(args.rounds):  # the rows alternate inside every round
        for r in rows.values():
            r["ms_rounds"].append(round(timed(r["call"], args.frames, r["per_call"]), 5))
    for r in rows.values():
        del r["call"], r["per_call"]
        r.pop("keep", None)
        ms = r["ms_rounds"]
        r["ms_median"] = statistics.median(ms)
        r["spread"] = round((max(ms) - min(ms)) / r["ms_median"], 4)
    med = {k: r["ms_median"] for k, r in rows.items()}
    res = dict(config=name, volume=f"{n}^3 {np.dtype(dtype).name}", data_range=[lo, hi], window=[wlo, "inf"],
               counts=counts, checks=checks, scratch=scratch, pass_ms=passes, frames=args.frames, warmup=args.warmup,
               rounds=args.rounds, device=torch.cuda.get_device_name(0), code_hash=vr_amd.kernel_code_hash(),
               over_hist={k: round(v / med["hist_256"], 3) for k, v in med.items() if k != "hist_256"}, rows=rows)
    if args.host and name == "c3":
        t0 = time.perf_counter()
        vol = rp.read_volume()
        t1 = time.perf_counter()
        inm = vol >= np.float32(wlo)
        try:
            import scipy.ndimage as ndi
            _, ncomp = ndi.label(inm)
            how = "scipy.ndimage.label (6-connected, labels not yet renumbered)"
        except ImportError:
            import label_ref
            ncomp = label_ref.table(label_ref.label_array(inm, 6))[1]["components"]
            how = "tests/label_ref.py"
        t2 = time.perf_counter()
        assert ncomp == counts["6"]["components"], (ncomp, counts["6"])
        res["host_path"] = dict(read_volume_ms=round((t1 - t0) * 1e3, 1), label_ms=round((t2 - t1) * 1e3, 1),
                                method=how)
    rp.close()
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, f"{name}.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=path, counts=counts, over_hist=res["over_hist"], ms=med, pass_ms=passes,
                          host=res.get("host_path"))),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "label"))
    ap.add_argument("--config", choices=sorted(CONFIGS), action="append")
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host", action="store_true", help="also time the host path of C3 once (slow)")
    args = ap.parse_args()
    for name in args.config or sorted(CONFIGS):
        run(name, args)


if __name__ == "__main__":
    main()
