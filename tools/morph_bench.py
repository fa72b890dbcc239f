"""The exact distance transform and ball morphology of a device mask against the histogram over the
same volume (GPU; measurement tool).

On the C3 volume (512^3 f32 from vr_generate_volume) and on C4 (1024^3 u8) the mask is the region
grown (vr_region_grow_device, 6-connected) from the largest component of the window [0.3 of the
data range, +inf].  One process times

    hist_256        vr_histogram with 256 bins over the data range: one pass over the bricks
    edt_set         vr_edt_squared_device to the set voxels: the passes along x, y and z
    edt_unset       the same to the unset voxels (the thickness of the region)
    <op>_<r2>       vr_mask_morph_device, op one of dilate, erode, open, close, r2 one of 1, 9, 100:
                    one transform saturated at r2 for dilate and erode, two for open and close

A round runs --frames calls of a row after --warmup warm-up calls and takes the kernel time from
vr_timing_read (HIP events around each transform); the rows alternate inside every round, and a
row's figure is the median over --rounds rounds.  What can be checked without a reference at this
size is checked on the device: the zeros of a distance are its target voxels, a dilation is the
distance's threshold, an erosion the other distance's, erode <= open <= mask <= close <= dilate as
sets, and the infos count what the arrays hold.  --host also times, once on C3, the host path the
calls replace: the mask read back and scipy.ndimage.distance_transform_edt.

    python tools/morph_bench.py            # the next free profiles/rNN/morph

writes <out>/c3.json and <out>/c4.json and prints one JSON line per configuration.
"""
from __future__ import annotations

import argparse
import json
import os
import re
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
OPS = {"dilate": vr_amd.MORPH_DILATE, "erode": vr_amd.MORPH_ERODE, "open": vr_amd.MORPH_OPEN,
       "close": vr_amd.MORPH_CLOSE}
R2 = (1, 9, 100)


def next_free_out():
    prof = os.path.join(ROOT, "profiles")
    taken = [int(m.group(1)) for m in (re.fullmatch(r"r(\d+)", d) for d in os.listdir(prof)) if m]
    return os.path.join(prof, f"r{max(taken, default=0) + 1:02d}", "morph")


def count(t):
    return int(t.sum(dtype=torch.int64))


def run(name, args):
    n, dtype = CONFIGS[name]
    rp = vr_amd.OffscreenPass(64, 64)
    lo, hi = rp.generate_volume((n,) * 3, dtype, seed=2024)
    wlo = float(np.float32(lo + LO_F * (hi - lo)))
    nvox, ext = n ** 3, (n, n, n)
    stream = torch.cuda.current_stream().cuda_stream
    mask = torch.empty(nvox, dtype=torch.uint8, device="cuda")
    out = torch.empty(nvox, dtype=torch.uint8, device="cuda")
    dist = torch.empty(nvox, dtype=torch.int32, device="cuda")
    info = rp.label_count(wlo, INF, 6)
    l = info["largest_label"] - 1
    comp = rp.region_grow_device((l % n, (l // n) % n, l // (n * n)), mask.data_ptr(), nvox, wlo, INF, 6, stream=stream)
    in_set = count(mask)
    assert comp["voxels"] == info["largest_voxels"] == in_set, (comp, info)

    edt = lambda to_set: rp.distance_transform_device(ext, mask.data_ptr(), 1, dist.data_ptr(), nvox, to_set=to_set,
                                                      stream=stream)
    morph = lambda op, r2, dst=out: rp.morph_device(ext, op, r2, mask.data_ptr(), 1, dst.data_ptr(), nvox, stream=stream)

    # ---- what can be checked without a reference ----
    checks, infos = {}, {}
    keep = torch.empty(nvox, dtype=torch.uint8, device="cuda")
    for to_set, key in ((True, "edt_set"), (False, "edt_unset")):
        i = infos[key] = edt(to_set)
        zeros = count(dist == 0)
        checks[key] = dict(zeros_equal_target=zeros == i["target_voxels"] == (in_set if to_set else nvox - in_set),
                           zeros_are_the_target=bool(torch.equal(dist == 0, (mask != 0) == to_set)),
                           max_is_the_max=i["max_dist2"] == int(dist.max()) and
                           int(dist[i["max_index"]]) == i["max_dist2"] and
                           int((dist == i["max_dist2"]).nonzero()[0]) == i["max_index"])
        for r2 in R2:  # a dilation is the threshold of the distance to the set voxels, an erosion the other's
            op = "dilate" if to_set else "erode"
            mi = infos[f"{op}_{r2}"] = morph(OPS[op], r2)
            want = (dist <= r2) if to_set else (dist > r2)
            checks[f"{op}_{r2}"] = dict(equals_threshold=bool(torch.equal(out != 0, want)),
                                        counts=mi == dict(voxels=nvox, in_set=in_set, out_set=count(want)))
    for r2 in R2:
        d_i, e_i = infos[f"dilate_{r2}"], infos[f"erode_{r2}"]
        o_i = infos[f"open_{r2}"] = morph(OPS["open"], r2, keep)
        c_i = infos[f"close_{r2}"] = morph(OPS["close"], r2)
        checks[f"order_{r2}"] = dict(
            counts_ordered=e_i["out_set"] <= o_i["out_set"] <= in_set <= c_i["out_set"] <= d_i["out_set"],
            open_inside_mask=not bool(((keep != 0) & (mask == 0)).any()),
            mask_inside_close=not bool(((mask != 0) & (out == 0)).any()),
            counts=o_i["out_set"] == count(keep) and c_i["out_set"] == count(out))
    del keep
    bad = {k: v for k, v in checks.items() if not all(v.values())}
    assert not bad, bad

    # ---- the times ----
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
            "edt_set": dict(call=lambda: edt(True), per_call=1), "edt_unset": dict(call=lambda: edt(False), per_call=1)}
    for op, code in OPS.items():
        for r2 in R2:
            rows[f"{op}_{r2}"] = dict(call=lambda c=code, r=r2: morph(c, r), per_call=2 if op in ("open", "close") else 1)
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
    res = dict(config=name, volume=f"{n}^3 {np.dtype(dtype).name}", data_range=[lo, hi], window=[wlo, "inf"],
               mask=dict(voxels=nvox, in_set=in_set, component=comp), infos=infos, checks=checks,
               scratch=dict(distance_bytes=4 * nvox, intermediate_mask_bytes=nvox, counter_bytes=64),
               frames=args.frames, warmup=args.warmup, rounds=args.rounds, device=torch.cuda.get_device_name(0),
               code_hash=vr_amd.kernel_code_hash(), last_kernel=rp.morph_last_kernel_name(),
               over_hist={k: round(v / med["hist_256"], 3) for k, v in med.items() if k != "hist_256"}, rows=rows)
    if args.host and name == "c3":
        import scipy.ndimage as ndi
        t0 = time.perf_counter()
        hm = mask.cpu().numpy().reshape(n, n, n)
        t1 = time.perf_counter()
        idx = ndi.distance_transform_edt(hm == 0, return_distances=False, return_indices=True)  # to the set voxels
        t2 = time.perf_counter()
        off = idx.astype(np.int32) - np.indices(hm.shape, dtype=np.int32)
        want = (off.astype(np.int64) ** 2).sum(axis=0).astype(np.uint32)
        edt(True)
        same = bool(np.array_equal(dist.cpu().numpy().view(np.uint32).reshape(n, n, n), want))
        assert same
        res["host_path"] = dict(read_mask_ms=round((t1 - t0) * 1e3, 1), edt_ms=round((t2 - t1) * 1e3, 1),
                                method="scipy.ndimage.distance_transform_edt (indices)", equals_device=same)
    rp.close()
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, f"{name}.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=path, in_set=in_set, over_hist=res["over_hist"], ms=med, host=res.get("host_path"))),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: the next free profiles/rNN/morph")
    ap.add_argument("--config", choices=sorted(CONFIGS), action="append")
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host", action="store_true", help="also time the host path of C3 once (slow)")
    args = ap.parse_args()
    if args.out is None:
        args.out = next_free_out()
    for name in args.config or sorted(CONFIGS):
        run(name, args)


if __name__ == "__main__":
    main()
