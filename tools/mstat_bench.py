"""The statistics of the volume under a device mask or label array against the histogram of the whole
volume (GPU; measurement tool).

On the C3 volume (512^3 f32 from vr_generate_volume) and on C4 (1024^3 u8) one process times

    hist_256          vr_histogram with 256 bins over the data range: one pass over the bricks, the
                      yardstick
    stats_region      vr_mask_stats_device of the region grown from the largest component of the
                      window [0.3 of the data range, +inf], 6-connected, without a histogram
    stats_region_hist the same with a 256-bin histogram
    label_stats_window
                      vr_label_stats_device on the window labelling's own labels and records
    label_stats_opened
                      vr_label_stats_device on the labels of the one-piece opening (r2 = 9) of the region
    window_mask       vr_mask_window_device of the region with the window it was grown from
    window_all        vr_mask_window_device with no mask: every voxel of the volume

A round runs --frames calls of a row after --warmup warm-up calls and takes the kernel time from
vr_timing_read (HIP events around each call's passes, its memsets and the copy of the records
included); the rows alternate inside every round, and a row's figure is the median over --rounds rounds.  What can be checked without a reference at this size
is checked: the records' voxels equal the labeller's and sum to in_voxels; a mask's region equals the
sums over its label records; the histogram's info is consistent with the region; the window of the
region is the region, and the window without a mask is the labelling's set.  --host also times, once on
C3, the host path the calls replace: both arrays read back, then numpy.

    python tools/mstat_bench.py --host      # the next free profiles/rNN/mstat

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
NBINS = 256
DT = vr_amd.MSTAT_REGION_DTYPE


def next_free_out():
    prof = os.path.join(ROOT, "profiles")
    taken = [int(m.group(1)) for m in (re.fullmatch(r"r(\d+)", d) for d in os.listdir(prof)) if m]
    return os.path.join(prof, f"r{max(taken, default=0) + 1:02d}", "mstat")


def count(t):
    return int(t.sum(dtype=torch.int64))


def write(res, args, name):
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, f"{name}.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1, default=lambda o: o.item())  # (numpy scalars of the checks and infos)
        f.write("\n")
    return path


def records(t, n):
    return np.frombuffer(t.cpu().numpy()[:n * 16].tobytes(), DT)


def run(name, args):
    n, dtype = CONFIGS[name]
    rp = vr_amd.OffscreenPass(64, 64)
    lo, hi = rp.generate_volume((n,) * 3, dtype, seed=2024)
    wlo = float(np.float32(lo + LO_F * (hi - lo)))
    nvox, ext = n ** 3, (n, n, n)
    ints = np.dtype(dtype) != np.dtype(np.float32)
    stream = torch.cuda.current_stream().cuda_stream
    winfo = rp.label_count(wlo, INF, 6)
    nc = winfo["components"]
    wlab = torch.empty(nvox, dtype=torch.int32, device="cuda")
    wrec = torch.zeros(max(nc, 1) * 16, dtype=torch.int32, device="cuda")
    wreg = torch.zeros(max(nc, 1) * 16, dtype=torch.int32, device="cuda")
    assert rp.label_device(wlab.data_ptr(), nvox, wrec.data_ptr(), nc, wlo, INF, 6, stream=stream) == winfo
    # the region under the largest component, its one-piece opening and that opening's labels
    region = torch.empty(nvox, dtype=torch.uint8, device="cuda")
    opened = torch.empty(nvox, dtype=torch.uint8, device="cuda")
    out = torch.empty(nvox, dtype=torch.uint8, device="cuda")
    l = winfo["largest_label"] - 1
    comp = rp.region_grow_device((l % n, (l // n) % n, l // (n * n)), region.data_ptr(), nvox, wlo, INF, 6, stream=stream)
    rp.morph_device(ext, vr_amd.MORPH_OPEN, OPEN_R2, region.data_ptr(), 1, opened.data_ptr(), nvox, stream=stream)
    piece = rp.mask_select_device(ext, vr_amd.MASK_KEEP_LARGEST, opened.data_ptr(), 1, out.data_ptr(), nvox, 6, stream=stream)
    opened.copy_(out)
    olab = torch.empty(nvox, dtype=torch.int32, device="cuda")
    orec = torch.zeros(16, dtype=torch.int32, device="cuda")
    oreg = torch.zeros(16, dtype=torch.int32, device="cuda")
    oinfo = rp.mask_label_device(ext, opened.data_ptr(), 1, olab.data_ptr(), nvox, orec.data_ptr(), 1, 6, stream=stream)
    assert oinfo["components"] == 1 and oinfo["in_voxels"] == piece["out_set"], (oinfo, piece)

    hist = (NBINS, lo, hi)
    stats = lambda src, h=None: rp.mask_stats_device(ext, src.data_ptr(), 1, hist=h, stream=stream)
    label_stats = lambda lab, rec, reg, k: rp.label_stats_device(ext, lab.data_ptr(), rec.data_ptr(), k, reg.data_ptr(), k,
                                                                 stream=stream)
    window = lambda src: rp.mask_window_device(ext, src.data_ptr() if src is not None else 0, 1, wlo, INF,
                                               out.data_ptr(), nvox, stream=stream)

    # ---- what can be checked without a reference ----
    checks, infos = {}, {}
    i = infos["label_stats_window"] = label_stats(wlab, wrec, wreg, nc)
    reg, comps = records(wreg, nc), np.frombuffer(wrec.cpu().numpy()[:nc * 16].tobytes(), vr_amd.LABEL_COMPONENT_DTYPE)
    checks["label_stats_window"] = dict(voxels_equal_the_labeller=bool(np.array_equal(reg["voxels"], comps["voxels"])),
                                        labels_equal=bool(np.array_equal(reg["label"], comps["label"])),
                                        sum_to_in_voxels=int(reg["voxels"].sum()) == winfo["in_voxels"] == i["set"],
                                        none_unlisted=i["unlisted"] == 0 and i["regions"] == nc,
                                        extremes_in_window=bool((reg["vmin"] >= np.float32(wlo)).all()))
    # the mask of the whole window is one region: the sums over its label records
    wmask = (wlab != 0).to(torch.uint8)
    whole = stats(wmask)["region"]
    tol = 0.0 if ints else 1e-9
    checks["mask_equals_its_records"] = dict(
        voxels=whole["voxels"] == int(reg["voxels"].sum()), nan=whole["nan"] == int(reg["nan"].sum()),
        vmin=whole["vmin"] == float(reg["vmin"].min()), vmax=whole["vmax"] == float(reg["vmax"].max()),
        min_index=whole["min_index"] == int(reg["min_index"][reg["vmin"] == reg["vmin"].min()].min()),
        max_index=whole["max_index"] == int(reg["max_index"][reg["vmax"] == reg["vmax"].max()].min()),
        sum=abs(whole["sum"] - float(np.sum(reg["sum"]))) <= tol * abs(whole["sum"]),
        sum2=abs(whole["sum2"] - float(np.sum(reg["sum2"]))) <= tol * abs(whole["sum2"]))
    r0 = infos["stats_region"] = stats(region)["region"]
    got = stats(region, hist)
    r1, hinfo = got["region"], got["hist_info"]
    infos["stats_region_hist"] = dict(region=r1, hist_info={k: float(v) for k, v in hinfo.items()})
    same = all(r0[k] == r1[k] for k in ("voxels", "nan", "vmin", "vmax", "min_index", "max_index"))
    checks["stats_region"] = dict(voxels_equal_the_grown_component=r0["voxels"] == comp["voxels"],
                                  with_and_without_histogram_agree=same and (not ints or r0 == r1),
                                  extremes_in_window=r0["vmin"] >= np.float32(wlo))
    checks["hist_info"] = dict(voxels=hinfo["voxels"] == r1["voxels"], nan=hinfo["nan"] == r1["nan"],
                               extremes=float(hinfo["vmin"]) == r1["vmin"] and float(hinfo["vmax"]) == r1["vmax"],
                               bins_sum=int(got["bins"].sum()) + hinfo["below"] + hinfo["above"] + hinfo["nan"] == r1["voxels"],
                               nothing_below_the_window=int(got["bins"][:int(LO_F * NBINS) - 1].sum()) + hinfo["below"] == 0)
    i = infos["label_stats_opened"] = label_stats(olab, orec, oreg, 1)
    oreg_h = records(oreg, 1)[0]
    checks["label_stats_opened"] = dict(voxels=int(oreg_h["voxels"]) == oinfo["in_voxels"] == i["set"],
                                        unlisted=i["unlisted"] == 0)
    i = infos["window_mask"] = window(region)
    checks["window_mask"] = dict(the_region_as_it_is=bool(torch.equal(out, region)),
                                 counts=(i["in_set"], i["out_set"]) == (comp["voxels"], comp["voxels"]))
    i = infos["window_all"] = window(None)
    checks["window_all"] = dict(equals_labels_nonzero=bool(torch.equal(out, wmask)),
                                counts=(i["in_set"], i["out_set"]) == (nvox, winfo["in_voxels"]))
    bad = {k: v for k, v in checks.items() if not all(v.values())}
    assert not bad, bad

    # ---- the times ----
    def timed(call, frames):
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        rp.timing_reset()
        rp.timing_enable(True)
        for _ in range(frames):
            call()
        ms, cnt = rp.timing_read()
        rp.timing_enable(False)
        assert cnt == frames, (cnt, frames)  # one interval a call
        return ms / frames

    rows = {"hist_256": dict(call=lambda: rp.histogram(NBINS, lo, hi)),
            "stats_region": dict(call=lambda: stats(region)),
            "stats_region_hist": dict(call=lambda: stats(region, hist)),
            "label_stats_window": dict(call=lambda: label_stats(wlab, wrec, wreg, nc)),
            "label_stats_opened": dict(call=lambda: label_stats(olab, orec, oreg, 1)),
            "window_mask": dict(call=lambda: window(region)),
            "window_all": dict(call=lambda: window(None))}
    for r in rows.values():
        r["ms_rounds"] = []
    for _ in range(args.rounds):  # the rows alternate inside every round
        for r in rows.values():
            r["ms_rounds"].append(round(timed(r["call"], args.frames), 5))
    for r in rows.values():
        del r["call"]
        ms = r["ms_rounds"]
        r["ms_median"] = statistics.median(ms)
        r["spread"] = round((max(ms) - min(ms)) / r["ms_median"], 4)
    med = {k: r["ms_median"] for k, r in rows.items()}
    res = dict(config=name, volume=f"{n}^3 {np.dtype(dtype).name}", data_range=[lo, hi], window=[wlo, "inf"],
               window_info=winfo, region=dict(component=comp, opened_piece=oinfo), infos=infos, checks=checks,
               scratch=dict(fixed_bytes=64 + 4096 * 12, record_bytes=116 * nc),
               frames=args.frames, warmup=args.warmup, rounds=args.rounds, device=torch.cuda.get_device_name(0),
               code_hash=vr_amd.kernel_code_hash(), last_kernel=rp.mstat_last_kernel_name(),
               over_hist_256={k: round(v / med["hist_256"], 3) for k, v in med.items() if k != "hist_256"}, rows=rows)
    path = write(res, args, name)
    print(json.dumps(dict(out=path, window=winfo, over_hist_256=res["over_hist_256"], ms=med), default=lambda o: o.item()),
          flush=True)
    if args.host and name == "c3":
        t0 = time.perf_counter()
        hm = region.cpu().numpy()
        t1 = time.perf_counter()
        hv = rp.read_volume().reshape(-1)
        t2 = time.perf_counter()
        sel = hv[hm != 0]
        d = sel.astype(np.float64)
        host = dict(voxels=int(sel.size), vmin=float(sel.min()), vmax=float(sel.max()), sum=float(d.sum()),
                    sum2=float((d * d).sum()))
        bins = np.histogram(sel, NBINS, (lo, hi))[0]
        t3 = time.perf_counter()
        agree = (host["voxels"], host["vmin"], host["vmax"]) == (r0["voxels"], r0["vmin"], r0["vmax"]) and \
            abs(host["sum"] - r0["sum"]) <= 1e-9 * abs(r0["sum"]) and int(bins.sum()) <= r0["voxels"]
        assert agree, (host, r0)
        res["host_path"] = dict(read_mask_ms=round((t1 - t0) * 1e3, 1), read_volume_ms=round((t2 - t1) * 1e3, 1),
                                numpy_ms=round((t3 - t2) * 1e3, 1), method="boolean index, min, max, sums, np.histogram",
                                agrees_with_device=agree)
        write(res, args, name)
        print(json.dumps(dict(host=res["host_path"]), default=lambda o: o.item()), flush=True)
    rp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: the next free profiles/rNN/mstat")
    ap.add_argument("--config", choices=sorted(CONFIGS), action="append")
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host", action="store_true", help="also time the host path of C3 once (slow)")
    args = ap.parse_args()
    if args.out is None:
        args.out = next_free_out()
    for name in args.config or sorted(CONFIGS):
        run(name, args)


if __name__ == "__main__":
    main()
