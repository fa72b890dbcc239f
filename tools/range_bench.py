"""What tools/mip_bench.py, iso_bench.py and proj_bench.py share (GPU; measurement tools).

One configuration (volume generated on the device, as bench.py's: c3 512^3 f32 at 1920x1080,
c2 256^3 u8 at 1024x1024, c4 1024^3 u8 at 2048x2048), TF-2, the views `fill` (r = 1.6) and
`default` (the reference's camera, r = 3).  One process alternates a script's variants for
--rounds rounds; each variant runs --frames serial frames after --warmup warm-up frames and
takes the kernel time from vr_timing_read (HIP events around each launch).  A variant is
(name, mode, skip_empty, mip_inflight knob (0: the library's own choice), ...); the script
says how one is selected, which vr_params it renders with and which work counters its row
carries, and keeps its yardstick, its per-view summary and its final printed line.
`<out>/<config>.json` holds the header, then `views` as the script fills it.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("volumetric-renderer_amd", "tools"):
    sys.path.insert(0, os.path.join(ROOT, sub))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import synth  # noqa: E402
import vr_amd  # noqa: E402

CONFIGS = {
    "c3": dict(n=512, dtype="float32", size=(1920, 1080)),
    "c2": dict(n=256, dtype="uint8", size=(1024, 1024)),
    "c4": dict(n=1024, dtype="uint8", size=(2048, 2048)),
}
VIEWS = {"fill": dict(radius=1.6, rotate=None), "default": dict(radius=3.0, rotate=None)}
KS = (1, 2, 4)


def cameras():
    """(view name, vr_camera) of VIEWS, in order."""
    for vname, v in VIEWS.items():
        yield vname, vr_amd.make_camera(**v).to_vr_camera()


def work_counts(st):
    """The counters of a vr_count_work pass that a MIP / MinIP / mean row carries."""
    return dict(rays=st["rays"], samples=st["samples"], skipped_samples=st["skipped_samples"],
                in_slab=st["samples"] + st["skipped_samples"])


def auto_k(rows, prefix):
    """The K the library chose for `<prefix>_skip{0,1}_k0`, read off the kernel names."""
    return [int(re.search(r", (\d)>\(", rows[f"{prefix}_skip{s}_k0"]["kernel"]).group(1)) for s in (0, 1)]


def best_k(rows, prefix):
    return min(KS, key=lambda k: rows[f"{prefix}_k{k}"]["ms_median"])


def bound_ms(row):
    """The yardstick row's median plus its own round-to-round spread."""
    return row["ms_median"] * (1.0 + row["spread"])


class Bench:
    """The pass, volume and output buffer of one --config, and the result file's header."""

    def __init__(self, default_out, data_range=False):
        ap = argparse.ArgumentParser()
        ap.add_argument("--config", choices=sorted(CONFIGS), required=True)
        ap.add_argument("--out", default=os.path.join(ROOT, *default_out))
        ap.add_argument("--frames", type=int, default=200)
        ap.add_argument("--warmup", type=int, default=20)
        ap.add_argument("--rounds", type=int, default=3)
        self.args = args = ap.parse_args()
        cfg = CONFIGS[args.config]
        W, H = cfg["size"]
        self.rp = vr_amd.OffscreenPass(W, H)
        self.lo, self.hi = self.rp.generate_volume((cfg["n"],) * 3, np.dtype(cfg["dtype"]), seed=2024)
        self.rp.transfer_function_changed(synth.tf2())
        self.out = torch.empty((H + 16, W), dtype=torch.int32, device="cuda")
        self.stream = torch.cuda.current_stream().cuda_stream
        self.f32 = cfg["dtype"] == "float32"
        self.res = dict(config=args.config, volume=f"{cfg['n']}^3 {cfg['dtype']}", frame=f"{W}x{H}", tf="tf2",
                        **(dict(data_range=[self.lo, self.hi]) if data_range else {}),
                        frames=args.frames, warmup=args.warmup, rounds=args.rounds,
                        code_hash=vr_amd.kernel_code_hash(), views={})

    def run(self, cam, p):
        """ms per frame of --frames serial frames after --warmup."""
        rp, args = self.rp, self.args
        for _ in range(args.warmup):
            rp.render_device(cam, p, self.out.data_ptr(), vr_amd.OUT_RGBA8, 16, 0, 1, self.stream)
        torch.cuda.synchronize()
        rp.timing_reset()
        rp.timing_enable(True)
        for _ in range(args.frames):
            rp.render_device(cam, p, self.out.data_ptr(), vr_amd.OUT_RGBA8, 16, 0, 1, self.stream)
        ms, n = rp.timing_read()
        rp.timing_enable(False)
        return ms / n

    def measure(self, cam, variants, select, params, work):
        """name -> row.  Fills the rows (kernel name and work(cam, p, *variant)'s counters), then
        alternates the variants inside every round; median, spread and, for rows that count
        in-slab samples, the skipped share."""
        rp = self.rp
        rows = {}
        for name, *v in variants:
            select(*v)
            p = params(*v)
            rp.prepare(cam, p)
            rows[name] = dict(kernel=rp.kernel_name(p), **work(cam, p, *v), ms_rounds=[])
        for _ in range(self.args.rounds):  # alternate the variants inside every round
            for name, *v in variants:
                select(*v)
                rows[name]["ms_rounds"].append(round(self.run(cam, params(*v)), 5))
        for r in rows.values():
            ms = r["ms_rounds"]
            r["ms_median"] = statistics.median(ms)
            r["spread"] = round((max(ms) - min(ms)) / r["ms_median"], 4)
            if "in_slab" in r:
                r["skipped_share"] = round(r["skipped_samples"] / max(r["in_slab"], 1), 4)
        return rows

    def write(self, line):
        """Closes the pass, writes <out>/<config>.json and prints line(views) with its path."""
        self.rp.close()
        os.makedirs(self.args.out, exist_ok=True)
        path = os.path.join(self.args.out, self.args.config + ".json")
        with open(path, "w") as f:
            json.dump(self.res, f, indent=1)
            f.write("\n")
        print(json.dumps(dict(config=self.args.config, out=path, **line(self.res["views"]))))
