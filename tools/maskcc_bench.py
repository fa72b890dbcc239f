"""Labelling, filtering and filling a device mask by connected component against the window
labelling the mask came from (GPU; measurement tool).

On the C3 volume (512^3 f32 from vr_generate_volume) and on C4 (1024^3 u8) one process times

    hist_256        vr_histogram with 256 bins over the data range: one pass over the bricks
    label_window    vr_label_components_device on the window [0.3 of the data range, +inf], 6-connected:
                    the yardstick, the labelling of the parent commit
    mask_label_4    vr_mask_label_device on that call's label array as a 4-byte mask: the same set
    mask_label_1    the same set as a 1-byte mask
    mask_label_opened
                    vr_mask_label_device on the opening below: one smooth piece
    keep_largest, keep_min_50, keep_seed
                    vr_mask_select_device on the morphological opening (r2 = 9) of the region grown
                    from the window's largest component; the seed is the region's deepest voxel
    fill_holes      VR_MASK_FILL_HOLES on the region itself

A round runs --frames calls of a row after --warmup warm-up calls and takes the kernel time from
vr_timing_read (HIP events around each interval); the rows alternate inside every round, and a row's
figure is the median over --rounds rounds; pass_ms splits a call of some rows kernel by kernel
(events between the passes).  What can be checked without a reference at this size is
checked on the device: the mask's label bytes equal the window labelling's, the records are equal
and sum to in_set, out_set of KEEP_LARGEST is the info's largest_voxels, the kept seed piece holds
the seed, and the region is a subset of its filling.  --host also times, once on C3, the host path
the calls replace: the mask read back, scipy.ndimage.label and scipy.ndimage.binary_fill_holes.

    python tools/maskcc_bench.py            # the next free profiles/rNN/maskcc

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
OPEN_R2 = 9
MIN_VOXELS = 50


def next_free_out():
    prof = os.path.join(ROOT, "profiles")
    taken = [int(m.group(1)) for m in (re.fullmatch(r"r(\d+)", d) for d in os.listdir(prof)) if m]
    return os.path.join(prof, f"r{max(taken, default=0) + 1:02d}", "maskcc")


def count(t):
    return int(t.sum(dtype=torch.int64))


def write(res, args, name):
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, f"{name}.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return path


def run(name, args):
    n, dtype = CONFIGS[name]
    rp = vr_amd.OffscreenPass(64, 64)
    lo, hi = rp.generate_volume((n,) * 3, dtype, seed=2024)
    wlo = float(np.float32(lo + LO_F * (hi - lo)))
    nvox, ext = n ** 3, (n, n, n)
    stream = torch.cuda.current_stream().cuda_stream
    winfo = rp.label_count(wlo, INF, 6)
    nc = winfo["components"]
    wlab = torch.empty(nvox, dtype=torch.int32, device="cuda")
    wrec = torch.zeros(max(nc, 1) * 16, dtype=torch.int32, device="cuda")
    mlab = torch.empty(nvox, dtype=torch.int32, device="cuda")
    mrec = torch.zeros(max(nc, 1) * 16, dtype=torch.int32, device="cuda")
    out = torch.empty(nvox, dtype=torch.uint8, device="cuda")

    label_window = lambda: rp.label_device(wlab.data_ptr(), nvox, wrec.data_ptr(), nc, wlo, INF, 6, stream=stream)
    mask_label = lambda src, eb: rp.mask_label_device(ext, src.data_ptr(), eb, mlab.data_ptr(), nvox, mrec.data_ptr(),
                                                      nc, 6, stream=stream)
    select = lambda src, rule, **kw: rp.mask_select_device(ext, rule, src.data_ptr(), 1, out.data_ptr(), nvox, 6,
                                                           stream=stream, **kw)

    # ---- what can be checked without a reference ----
    checks, infos = {}, {}
    infos["label_window"] = label_window()
    assert infos["label_window"] == winfo
    byte_mask = (wlab != 0).to(torch.uint8)
    for key, src, eb in (("mask_label_4", wlab, 4), ("mask_label_1", byte_mask, 1)):
        mlab.fill_(-1)
        mrec.fill_(-1)
        i = infos[key] = mask_label(src, eb)
        voxels = mrec.view(torch.int64).view(-1, 8)[:nc, 1]  # (vr_label_component: the second 64-bit word)
        checks[key] = dict(info_equals_window=i == winfo, label_bytes_equal_window=bool(torch.equal(mlab, wlab)),
                           records_equal_window=bool(torch.equal(mrec, wrec)),
                           records_sum_to_in_set=count(voxels) == i["in_voxels"] == count(byte_mask))
    # the region under the largest component, its deepest voxel, and its opening
    region = torch.empty(nvox, dtype=torch.uint8, device="cuda")
    opened = torch.empty(nvox, dtype=torch.uint8, device="cuda")
    l = winfo["largest_label"] - 1
    comp = rp.region_grow_device((l % n, (l // n) % n, l // (n * n)), region.data_ptr(), nvox, wlo, INF, 6, stream=stream)
    deep = rp.distance_transform_device(ext, region.data_ptr(), 1, mlab.data_ptr(), nvox, to_set=False, stream=stream)
    d = deep["max_index"]
    seed = (d % n, (d // n) % n, d // (n * n))
    open_info = rp.morph_device(ext, vr_amd.MORPH_OPEN, OPEN_R2, region.data_ptr(), 1, opened.data_ptr(), nvox, stream=stream)
    assert deep["max_dist2"] > OPEN_R2 and int(opened[d]) == 1, (deep, open_info)
    # the pieces the opening left: counted first, so that the record buffer holds them
    pieces = select(opened, vr_amd.MASK_KEEP_MIN_VOXELS, min_voxels=0)["components"]
    orec = torch.zeros(max(pieces, 1) * 16, dtype=torch.int32, device="cuda")
    oinfo = rp.mask_label_device(ext, opened.data_ptr(), 1, mlab.data_ptr(), nvox, orec.data_ptr(), pieces, 6, stream=stream)
    i = infos["keep_largest"] = select(opened, vr_amd.MASK_KEEP_LARGEST)
    checks["keep_largest"] = dict(out_set_is_largest_voxels=i["out_set"] == oinfo["largest_voxels"] == count(out),
                                  counts=(i["in_set"], i["components"], i["kept"]) ==
                                  (open_info["out_set"], oinfo["components"], 1),
                                  subset=not bool(((out != 0) & (opened == 0)).any()))
    i = infos["keep_min_50"] = select(opened, vr_amd.MASK_KEEP_MIN_VOXELS, min_voxels=MIN_VOXELS)
    voxels = orec.view(torch.int64).view(-1, 8)[:pieces, 1]
    checks["keep_min_50"] = dict(out_set_counts=i["out_set"] == count(out),
                                 records_agree=(i["components"], i["kept"], i["out_set"]) ==
                                 (pieces, count(voxels >= MIN_VOXELS), count(voxels[voxels >= MIN_VOXELS])),
                                 subset=not bool(((out != 0) & (opened == 0)).any()))
    i = infos["keep_seed"] = select(opened, vr_amd.MASK_KEEP_SEED, seed=seed)
    checks["keep_seed"] = dict(holds_the_seed=int(out[d]) == 1 and i["kept"] == 1, out_set_counts=i["out_set"] == count(out),
                               subset=not bool(((out != 0) & (opened == 0)).any()))
    i = infos["fill_holes"] = select(region, vr_amd.MASK_FILL_HOLES)
    checks["fill_holes"] = dict(mask_inside_filled=not bool(((region != 0) & (out == 0)).any()),
                                counts=(i["in_set"], i["out_set"]) == (comp["voxels"], count(out)),
                                kept_at_most_components=i["kept"] <= i["components"])
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
            "label_window": dict(call=label_window, per_call=2),
            "mask_label_4": dict(call=lambda: mask_label(wlab, 4), per_call=2),
            "mask_label_1": dict(call=lambda: mask_label(byte_mask, 1), per_call=2),
            "mask_label_opened": dict(call=lambda: mask_label(opened, 1), per_call=2),
            "keep_largest": dict(call=lambda: select(opened, vr_amd.MASK_KEEP_LARGEST), per_call=3),
            "keep_min_50": dict(call=lambda: select(opened, vr_amd.MASK_KEEP_MIN_VOXELS, min_voxels=MIN_VOXELS), per_call=3),
            "keep_seed": dict(call=lambda: select(opened, vr_amd.MASK_KEEP_SEED, seed=seed), per_call=3),
            "fill_holes": dict(call=lambda: select(region, vr_amd.MASK_FILL_HOLES), per_call=3)}
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

    # pass by pass: events between the kernels of a call's intervals, medians over the calls
    def passes(call):
        call()
        rp.timing_enable(True)
        got = []
        for _ in range(max(args.frames, 3)):
            rp.timing_reset()
            call()
            got.append(rp.maskcc_pass_ms())
        rp.timing_enable(False)
        rp.timing_reset()
        return {k: round(statistics.median(g[k] for g in got), 5) for k in got[0]}

    pass_ms = {"mask_label_4": passes(lambda: mask_label(wlab, 4)),
               "mask_label_opened": passes(lambda: mask_label(opened, 1)),
               "keep_seed": passes(lambda: select(opened, vr_amd.MASK_KEEP_SEED, seed=seed)),
               "fill_holes": passes(lambda: select(region, vr_amd.MASK_FILL_HOLES))}
    label_window()
    rp.timing_enable(True)
    label_window()
    pass_ms["label_window"] = {k: round(v, 5) for k, v in rp.label_pass_ms().items()}
    rp.timing_enable(False)
    rp.timing_reset()
    res = dict(config=name, volume=f"{n}^3 {np.dtype(dtype).name}", data_range=[lo, hi], window=[wlo, "inf"],
               window_info=winfo, region=dict(component=comp, deepest=deep, seed=seed, opened=open_info, pieces=oinfo),
               infos=infos, checks=checks,
               scratch=dict(select_label_bytes=4 * nvox, root_table_bytes=3 * nvox // 16, record_bytes=65 * nc),
               frames=args.frames, warmup=args.warmup, rounds=args.rounds, device=torch.cuda.get_device_name(0),
               code_hash=vr_amd.kernel_code_hash(), last_kernel=rp.maskcc_last_kernel_name(),
               over_label_window={k: round(v / med["label_window"], 3) for k, v in med.items() if k != "label_window"},
               rows=rows, pass_ms=pass_ms)
    path = write(res, args, name)
    print(json.dumps(dict(out=path, window=winfo, over_label_window=res["over_label_window"], ms=med, pass_ms=pass_ms)),
          flush=True)
    if args.host and name == "c3":
        import scipy.ndimage as ndi
        t0 = time.perf_counter()
        hm = byte_mask.cpu().numpy().reshape(n, n, n)
        t1 = time.perf_counter()
        _, cnt = ndi.label(hm)
        t2 = time.perf_counter()
        hr = region.cpu().numpy().reshape(n, n, n)
        t3 = time.perf_counter()
        filled = ndi.binary_fill_holes(hr)
        t4 = time.perf_counter()
        select(region, vr_amd.MASK_FILL_HOLES)
        same = bool(np.array_equal(out.cpu().numpy().reshape(n, n, n), filled.astype(np.uint8)))
        assert cnt == nc and same, (cnt, nc, same)
        res["host_path"] = dict(read_mask_ms=round((t1 - t0) * 1e3, 1), label_ms=round((t2 - t1) * 1e3, 1),
                                read_region_ms=round((t3 - t2) * 1e3, 1), fill_holes_ms=round((t4 - t3) * 1e3, 1),
                                method="scipy.ndimage.label, scipy.ndimage.binary_fill_holes (6-structure)",
                                components_equal_device=cnt == nc, filled_equals_device=same)
        write(res, args, name)
        print(json.dumps(dict(host=res["host_path"])), flush=True)
    rp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: the next free profiles/rNN/maskcc")
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
