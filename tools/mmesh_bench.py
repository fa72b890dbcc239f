"""The mesh of a device mask against the isosurface mesh of the volume itself (GPU; measurement tool).

On the C3 volume (512^3 f32 from vr_generate_volume) and on C4 (1024^3 u8) one process times

    hist_256             vr_histogram with 256 bins over the data range: one pass over the bricks
    mesh_count           vr_mesh_count at iso = 0.3 of the data range, closed: the yardstick's count
    mesh_extract_n0      vr_mesh_extract_device, normals 0: the yardstick's extraction
    mask_count           vr_mask_mesh_count_device of the byte mask of the window [iso, +inf]
                         (vr_mask_window_device with no mask) over the whole volume, closed
    mask_extract_n0      vr_mask_mesh_extract_device of it, normals 0, no smoothing
    mask_extract         the same with normals
    mask_extract_s5      normals 0 and 5 smoothing sweeps at relax 0.5
    label_count          the same mask as a 4-byte array whose set elements are 7, VR_MVIEW_LABEL 7
    label_extract_n0     and its extraction, normals 0

The window's mask classifies every node as vr_mesh.h does at that iso, so the two meshes have the
same vertices and triangles: the tool ASSERTS the counts equal vr_mesh_count's, that the unsmoothed
mask mesh without normals is vr_mesh's mesh in mesh_scenes' canonical form on a 64^3 corner box, that
the label's mesh is the mask's byte for byte, and that two extractions write the same bytes.

A round runs --frames calls of a row after --warmup warm-up calls and takes the kernel time from
vr_timing_read (HIP events around each call's passes: one interval a call for this family, two for
vr_mesh_extract_device); the rows alternate inside every round, and a row's figure is the median
over --rounds rounds.  The passes of an extraction are read off as differences of rows of the same
round: emit = extract - count, a sweep = (s5 - n0) / 5.

    python tools/mmesh_bench.py      # the next free profiles/rNN/mmesh

writes <out>/c3.json and <out>/c4.json and prints one JSON line per configuration.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("volumetric-renderer_amd", "tools", "tests", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, sub))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import vr_amd  # noqa: E402

CONFIGS = {"c3": (512, np.float32), "c4": (1024, np.uint8)}
ISO_F = 0.3
INF = float("inf")
LABEL = 7
SWEEPS = 5
CORNER = 64  # the box of the record-for-record comparison with vr_mesh


def next_free_out():
    prof = os.path.join(ROOT, "profiles")
    taken = [int(m.group(1)) for m in (re.fullmatch(r"r(\d+)", d) for d in os.listdir(prof)) if m]
    return os.path.join(prof, f"r{max(taken, default=0) + 1:02d}", "mmesh")


def run(name, args):
    n, dtype = CONFIGS[name]
    rp = vr_amd.OffscreenPass(64, 64)
    lo, hi = rp.generate_volume((n,) * 3, dtype, seed=2024)
    iso = float(np.float32(lo + ISO_F * (hi - lo)))
    nvox, ext = n ** 3, (n, n, n)
    stream = torch.cuda.current_stream().cuda_stream
    vinfo = rp.mesh_count(iso)
    nv, nt = vinfo["vertices"], vinfo["triangles"]
    mask = torch.empty(nvox, dtype=torch.uint8, device="cuda")
    winfo = rp.mask_window_device(ext, 0, 1, iso, INF, mask.data_ptr(), nvox, stream=stream)
    labels = mask.to(torch.int32) * LABEL
    verts = [torch.zeros((max(nv, 1), 6), dtype=torch.int32, device="cuda") for _ in range(2)]
    tris = [torch.zeros((max(nt, 1), 3), dtype=torch.int32, device="cuda") for _ in range(2)]
    req_m = lambda **kw: vr_amd.mmesh_request(ext, mask.data_ptr(), 1, **kw)
    req_l = lambda **kw: vr_amd.mmesh_request(ext, labels.data_ptr(), 4, label=LABEL, **kw)
    extract = lambda req, k=0: rp.mask_mesh_extract_device(req, verts[k].data_ptr(), nv, tris[k].data_ptr(), nt, stream=stream)

    # ---- what can be checked without a reference at this size ----
    minfo = rp.mask_mesh_count_device(req_m(), stream=stream)
    linfo = rp.mask_mesh_count_device(req_l(), stream=stream)
    checks = dict(counts_are_vr_meshs=(minfo["vertices"], minfo["triangles"]) == (nv, nt),
                  matching_is_the_windows=minfo["matching"] == winfo["out_set"] == vinfo["inside_voxels"],
                  label_counts_are_the_masks=linfo == minfo)
    if name == "c3":
        checks["c3_counts"] = (nv, nt) == (1743989, 4151260)
    a = extract(req_m(normals=True, smooth_iters=SWEEPS), 0)
    b = extract(req_l(normals=True, smooth_iters=SWEEPS), 1)
    checks["label_mesh_is_the_masks"] = a == b == minfo and bool(torch.equal(verts[0], verts[1]) and torch.equal(tris[0], tris[1]))
    extract(req_m(normals=True, smooth_iters=SWEEPS), 1)
    checks["two_extractions_same_bytes"] = bool(torch.equal(verts[0], verts[1]) and torch.equal(tris[0], tris[1]))
    t = tris[0][:nt].cpu().numpy().astype(np.int64)
    checks["indices_in_range"] = bool(nt == 0 or (t.min() >= 0 and t.max() < nv))
    # record for record against vr_mesh on a corner box (its order is unspecified: canonical form)
    import mesh_scenes
    box = ((0, 0, 0), (CORNER,) * 3)
    bv, bt, binfo = rp.mesh(iso, True, False, box)
    sub = mask.view(n, n, n)[:CORNER, :CORNER, :CORNER].contiguous().cpu().numpy()
    mv, mt, cinfo = rp.mask_mesh_extract(sub, (0, 0, 0), None, True, False)
    checks["corner_box_is_vr_meshs_mesh"] = (cinfo["vertices"], cinfo["triangles"]) == (binfo["vertices"], binfo["triangles"])
    mesh_scenes.assert_same_mesh((mv, mt), (bv, bt), "corner box")
    bad = [k for k, v in checks.items() if not v]
    assert not bad, (bad, vinfo, minfo, winfo)

    # ---- the times ----
    def timed(call, frames, per_call):
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        rp.timing_reset()
        rp.timing_enable(True)
        for _ in range(frames):
            call()
        torch.cuda.synchronize()
        ms, cnt = rp.timing_read()
        rp.timing_enable(False)
        assert cnt == frames * per_call, (cnt, frames, per_call)
        return ms / frames

    rows = {
        "hist_256": dict(call=lambda: rp.histogram(256, lo, hi), per_call=1),
        "mesh_count": dict(call=lambda: rp.mesh_count(iso), per_call=1),
        "mesh_extract_n0": dict(call=lambda: rp.mesh_device(verts[0].data_ptr(), nv, tris[0].data_ptr(), nt, iso, True, False,
                                                            stream=stream), per_call=2 if nv else 1),
        "mask_count": dict(call=lambda: rp.mask_mesh_count_device(req_m(), stream=stream), per_call=1),
        "mask_extract_n0": dict(call=lambda: extract(req_m(normals=False)), per_call=1),
        "mask_extract": dict(call=lambda: extract(req_m(normals=True)), per_call=1),
        "mask_extract_s5": dict(call=lambda: extract(req_m(normals=False, smooth_iters=SWEEPS)), per_call=1),
        "label_count": dict(call=lambda: rp.mask_mesh_count_device(req_l(), stream=stream), per_call=1),
        "label_extract_n0": dict(call=lambda: extract(req_l(normals=False)), per_call=1),
    }
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
    diff = lambda x, y, d=1: statistics.median(round((p - q) / d, 5) for p, q in zip(rows[x]["ms_rounds"], rows[y]["ms_rounds"]))
    passes = dict(mask_emit_ms=diff("mask_extract_n0", "mask_count"), mesh_emit_ms=diff("mesh_extract_n0", "mesh_count"),
                  sweep_ms=diff("mask_extract_s5", "mask_extract_n0", SWEEPS), normals_ms=diff("mask_extract", "mask_extract_n0"))
    g = vr_amd_geometry(ext)
    res = dict(config=name, volume=f"{n}^3 {np.dtype(dtype).name}", data_range=[lo, hi], isovalue=iso, closed=1,
               vr_mesh_counts=vinfo, mask_counts=minfo, window_info=winfo, checks=checks,
               bytes_read=dict(mask=nvox, label=4 * nvox, bricks=nvox * np.dtype(dtype).itemsize),
               bytes_written=24 * nv + 12 * nt, scratch=g, frames=args.frames, warmup=args.warmup, rounds=args.rounds,
               device=torch.cuda.get_device_name(0), code_hash=vr_amd.kernel_code_hash(),
               last_kernel=rp.mmesh_last_kernel_name(),
               ratios=dict(mask_count_over_mesh_count=round(med["mask_count"] / med["mesh_count"], 3),
                           mask_extract_n0_over_mesh_extract_n0=round(med["mask_extract_n0"] / med["mesh_extract_n0"], 3),
                           label_count_over_mesh_count=round(med["label_count"] / med["mesh_count"], 3),
                           mask_count_over_hist=round(med["mask_count"] / med["hist_256"], 3),
                           mesh_count_over_hist=round(med["mesh_count"] / med["hist_256"], 3)),
               passes=passes, rows=rows)
    rp.close()
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, f"{name}.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1, default=lambda o: o.item())
        f.write("\n")
    print(json.dumps(dict(out=path, counts=minfo, ratios=res["ratios"], passes=passes, ms=med),
                     default=lambda o: o.item()), flush=True)


def vr_amd_geometry(ext):
    """The scratch of a closed call on `ext` (csrc/vr_mmesh_host.h MmeshScratch), restated."""
    import mmesh_scenes
    g = mmesh_scenes.geometry(ext, True)
    words = g["node_words"] * 8 + g["cell_words"] * 16 + (g["cell_words"] * 4 + 7) // 8 * 8
    return dict(node_words=g["node_words"], cell_words=g["cell_words"], cells=g["cells"],
                bytes=words + mmesh_scenes.K["kMmeshMaxGroups"] * 16 + 8,
                bytes_per_cell=round(words / g["cells"], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: the next free profiles/rNN/mmesh")
    ap.add_argument("--config", choices=sorted(CONFIGS), action="append")
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if args.out is None:
        args.out = next_free_out()
    for name in args.config or sorted(CONFIGS):
        run(name, args)


if __name__ == "__main__":
    main()
