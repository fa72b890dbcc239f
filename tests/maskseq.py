"""Random chains of the mask calls on one context and their references -- test helper
(tests/test_maskseq_cpu.py, tests/test_gpu_maskseq.py).

tests/callseq.py replays the calls of libvr_amd.so.  This module does the same for the workflow the
family headers describe -- grow a region (vr_label.h), clean it (vr_morph.h, vr_maskcc.h), measure
it (vr_mstat.h), show it (vr_mview.h) -- where every call ends in an array in device memory that the
next call reads.  sequence(seed) is a list of op dicts drawn from numpy.random.default_rng alone:
nothing in it depends on what a device returned.  The volumes, cameras, planes and the composite
reference are callseq's, by import.

The model.  Beside the volume, the slice box and the framebuffer size the model keeps a REGISTER
FILE: nine fixed buffers that the GPU test allocates once per context (REGS) -- three byte registers
b0..b2, two word registers w0, w1, a component-record register c, a region-record register r, an
occupancy register o and an image/record register i, each sized for the pool's largest grid plus
slack.  The model holds EVERY BYTE of every register, the bytes past the current array that an
earlier, larger op left there included (the guard byte 0x77 before the first write), and beside the
bytes what the register means (Model.meta): kind (mask, labels, dist2, records, regions, words,
image), ext and origin of its grid, the element width, a version that every write bumps, the volume
epoch of the write, and for occupancy words the (register, version, select, label) they were built
for -- the words go to a hit or slice call only while that is still true (stale words are
"unspecified" by the header).

State ops:     volume, slice, resize.
Producers:     grow (vr_region_grow_device), label (vr_label_components_device), window0
               (vr_mask_window_device with a NULL mask), upload (a random host mask copied to an odd address).
Transformers:  morph, select, mask_label, edt, window with a mask: register to register, never in
               place.
Measurers:     stats, label_stats (its table is what a labeller left in c), occupancy, hit, pick,
               mslice (vr_mask_slice*; "slice" is the state op).
One call in four of every transformer and measurer that has one is drawn as the HOST form: it is
handed the model's array and its result is compared; it writes no register.  One op in twelve gives
a capacity one element short (VR_ENOSPC: info->voxels alone, nothing written).  Both are the base
rates: a form that a layout still owes is forced and a family short of five refusals draws four in
twelve (below), so that 177 of the 641 calls that have a host form take it and 64 of the 512 device
calls with a capacity are short.  A volume op keeps every
register: the next measurers run on a kept register, against the NEW volume where its grid still
fits and expecting VR_EINVAL where it does not.  Every device op draws one of four streams or the
NULL stream, never the stream of the op before it, and a consumer leans towards the register the op
before it wrote.  Every sequence opens with the three state ops and a producer and closes with a
shaded composite frame.

compute(op, model) is the pure reference of one op: the return code, the info, the host outputs, the
bytes it writes into which register (`writes`; everything else keeps its old bytes) and the kernel
intervals vr_timing_read must report.  Model.apply(result) advances the model.  The draws need the
model (a seed inside the mask, a label that exists, a component size), so generating IS computing:
cached(seed) returns the results sequence(seed) was drawn with.  The model is carried from seed to
seed in seed order, as the GPU test's contexts are; replay(upto) rebuilds the bytes at the start of
a seed from the cached writes.

Cost, measured with the generator and the references alone on the CPU (one core): the 24 seeds of
SEEDS, 36 ops each behind the opening four, take 9.7 s together, 0.33 s in the median and 1.9 s at
most (callseq's worst seed: 4.3 s).  The ball morphology and the labellings on the 123 k-voxel grid
and the redrawn cameras of the hit rectangles are most of it.  24 seeds of 20 ops met the counting
conditions of tests/test_maskseq_cpu.py only just, another one or two missing with every change of
a draw.  At 36 ops they hold with room -- 8 rises and falls where 5 are asked, 4 hand-overs where 3
are, 3 calls per (layout, entry point, form) where 2 are -- and held for 4 of 6 values tried of
BASE, the two others one short in one condition.  The condition on each kind's FIRST five calls is
a small sample whatever the length: it held for 2 of the 6, and BASE is the one with the most room.

The draws lean on a tally that is carried from seed to seed in seed order (_Tally), as callseq's
do: a volume op takes one of the three volumes whose layout the calls have met least, six times in
ten an (entry point, form) that has not read the current layout three times comes first, a consumer
takes the source whose grid moves its scratch group fourfold in the direction still owed, a
hand-over the consumer family that has read that producer family least, and a capacity falls short
four times in twelve while its family has not met VR_ENOSPC five times.  A camera is redrawn while the hit rectangle
holds fewer than ten hits, a plane while it misses the array and a window while it takes all of the
mask or none, as callseq redraws an isovalue.  sequence(seed) stays a function of the seed.
"""
import numpy as np

import callseq as Q
import label_ref
import maskcc_ref
import morph_ref
import mstat_ref
import mview_ref
import pyoracle
import vr_amd
from range_scenes import FULL, INSET, SLICE

F = np.float32
INF = float("inf")
SEEDS = range(24)
STEPS = 36
BASE = 84000  # (the generators are default_rng(BASE + seed))
OK, EINVAL, ENOSPC = 0, -22, vr_amd.ENOSPC
GUARD = 0x77

MAXV = max(Q.volume(n).voxels for n in Q.NAMES)
CCAP = 2048  # records the c and r registers hold
IMAGE_BYTES = 8192
OCC_WORDS = 64
# name -> bytes (each with slack behind the largest array it can hold)
REGS = {"b0": MAXV + 64, "b1": MAXV + 64, "b2": MAXV + 64, "w0": 4 * (MAXV + 16), "w1": 4 * (MAXV + 16),
        "c": 64 * CCAP + 64, "r": 64 * CCAP + 64, "o": 4 * (OCC_WORDS + 16), "i": IMAGE_BYTES + 64}
BYTE_REGS, WORD_REGS = ("b0", "b1", "b2"), ("w0", "w1")
R_OFF = 1  # the region records start at an odd address (the header: any alignment)

LAYOUT = {"g20": "f32", "g13d": "f32", "noise": "f32", "checker": "f32", "ints": "narrowed quads",
          "g33u8": "plain u8", "g48q": "u8 quads", "g64s": "i16"}
LAYOUTS = ("f32", "narrowed quads", "plain u8", "u8 quads", "i16")

STATE_OPS = ("volume", "slice", "resize")
PRODUCERS = ("grow", "label", "window0", "upload")
TRANSFORMERS = ("morph", "select", "mask_label", "edt", "window")
MEASURERS = ("stats", "label_stats", "occupancy", "hit", "pick", "mslice")
CONSUMERS = TRANSFORMERS + MEASURERS
FAMILY = {"grow": "label", "label": "label", "window0": "mstat", "upload": None, "morph": "morph", "edt": "morph",
          "select": "maskcc", "mask_label": "maskcc", "window": "mstat", "stats": "mstat", "label_stats": "mstat",
          "occupancy": "mview", "hit": "mview", "pick": "mview", "mslice": "mview"}
HAS_HOST_FORM = ("morph", "select", "mask_label", "edt", "window", "stats", "label_stats", "hit", "mslice")
HAS_CAPACITY = ("label", "morph", "select", "mask_label", "edt", "window", "window0", "label_stats", "occupancy",
                "hit", "mslice")
NEEDS_VOLUME = ("window", "stats", "label_stats", "occupancy", "hit", "pick", "mslice")  # mstat and mview
INFO_KEYS = {"morph": ("voxels", "in_set", "out_set"), "window": ("voxels", "in_set", "out_set"),
             "window0": ("voxels", "in_set", "out_set"),
             "edt": ("voxels", "target_voxels", "max_dist2", "max_index"),
             "select": ("voxels", "in_set", "out_set", "components", "kept"),
             "label": ("voxels", "in_voxels", "components", "largest_voxels", "largest_label"),
             "mask_label": ("voxels", "in_voxels", "components", "largest_voxels", "largest_label"),
             "label_stats": ("voxels", "set", "unlisted", "regions"),
             "occupancy": ("voxels", "cells", "cells_set", "matching"),
             "hit": ("voxels", "pixels", "covered", "hits", "steps", "samples"),
             "mslice": ("voxels", "pixels", "covered", "hits", "steps", "samples")}
SIZES = [(32, 24), (45, 35), (64, 48), (1, 1)]
R2 = (0, 1, 2, 3, 9)
R2_P = (0.15, 0.3, 0.25, 0.2, 0.1)  # (a ball of r2 = 9 empties or fills the small grids)
WEIGHTS = {"volume": 0.7, "slice": 0.4, "resize": 0.5,
           "grow": 1.0, "label": 0.9, "window0": 0.7, "upload": 0.6,
           "morph": 1.5, "select": 1.4, "mask_label": 1.0, "edt": 0.7, "window": 0.9,
           "stats": 1.2, "label_stats": 1.6, "occupancy": 0.7, "hit": 1.3, "pick": 0.5, "mslice": 1.0}


def voxels_of(ext):
    return int(ext[0]) * int(ext[1]) * int(ext[2])


def shape_of(ext):
    return (int(ext[2]), int(ext[1]), int(ext[0]))


def fits(ext, origin, dims):
    return all(origin[a] + ext[a] <= dims[a] for a in range(3))


def zero_info(kind, voxels=0):
    info = {k: 0 for k in INFO_KEYS[kind]}
    info["voxels"] = voxels
    return info


# ---- the model ------------------------------------------------------------------------------------
class Model:
    """The register file: every byte of every register, and what each one means."""

    def __init__(self):
        self.buf = {r: np.full(n, GUARD, np.uint8) for r, n in REGS.items()}
        self.meta = {r: dict(kind=None, ver=0) for r in REGS}

    def array(self, reg, ext, eb, off=0):
        """The (bz, by, bx) array of eb-byte elements that starts at byte `off` of the register."""
        n = voxels_of(ext) * eb
        a = self.buf[reg][off:off + n]
        return (a if eb == 1 else a.view(np.uint32)).reshape(shape_of(ext))

    def source(self, op):
        return self.array(op["src"], op["ext"], op["eb"], op["off"])

    def apply(self, res):
        for reg, off, data in res["writes"]:
            self.buf[reg][off:off + data.size] = data
        for reg, m in res["meta"].items():
            self.meta[reg] = dict(m, ver=self.meta[reg]["ver"] + 1)


def replay(upto):
    """The model at the start of seed `upto`, from the cached writes of the seeds before it."""
    m = Model()
    for seed in range(upto):
        for res in cached(seed):
            if res is not None:
                m.apply(res)
    return m


# ---- the references -------------------------------------------------------------------------------
def params(op, dims):
    return vr_amd.default_params(step=op["step"] if op["step"] else float(F(1.0) / F(max(dims))))


def scene_of(state, op):
    v = Q.volume(state["vol"])
    W, H = state["size"]
    return pyoracle.Scene.from_params(v.f32, float(F(v.lo)), float(F(v.hi)), Q.TFS["tf1"](), Q.camera(op["cam"]), W, H,
                                      params(op, v.dims), smin=state["slice"][0], smax=state["slice"][1])


def _bytes(a):
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8)


def compute(op, model, state=None):
    """The reference of one op on `model` under `state` (op["state"] where None): dict(rc, info, host,
    writes, meta, intervals, trivial).  Pure: the model is advanced by Model.apply alone."""
    st = op["state"] if state is None else state
    kind = op["op"]
    res = dict(rc=OK, info=None, host={}, writes=[], meta={}, intervals=None, trivial=False)
    if kind in STATE_OPS or kind == "frame":
        return res
    fam = FAMILY[kind]
    if fam in ("morph", "maskcc", "mstat", "mview"):
        res["intervals"] = 0
    v = Q.volume(st["vol"])
    ext, origin = op["ext"], op["origin"]
    n = voxels_of(ext)
    grid = dict(ext=tuple(ext), origin=tuple(origin), epoch=st["epoch"], vol=st["vol"])
    ints = v.storage != 4
    device = op["form"] == "device"

    def put(reg, off, data, **meta):
        if device:
            res["writes"].append((reg, off, _bytes(data)))
            res["meta"][reg] = dict(grid, off=off, **meta)
        else:
            res["host"]["out"] = np.ascontiguousarray(data)

    def refused(rc, voxels):
        res["rc"] = rc
        if kind in INFO_KEYS:
            res["info"] = zero_info(kind, voxels)
        return res

    if kind in NEEDS_VOLUME and not fits(ext, origin, v.dims):
        return refused(EINVAL, 0)
    if op.get("short"):
        return refused(ENOSPC, n)
    src = model.source(op) if op.get("src") else None
    if src is not None:
        nset = int(np.count_nonzero(src))
        res["trivial"] = nset in (0, n)
    crop = mstat_ref.crop(v.f32, origin, shape_of(ext)) if kind in NEEDS_VOLUME + ("window0",) else None

    if kind in ("grow", "label"):
        box = op["box"]
        ref = label_ref.label(v.f32, op["lo"], op["hi"], op["conn"], box)
        if kind == "grow":
            mask, comp = label_ref.region_grow(None, op["seed"], op["lo"], op["hi"], op["conn"], box, labelled=ref)
            res["host"]["comp"] = comp
            put(op["dst"], 0, mask, kind="mask", eb=1, nset=int(mask.sum()))
        else:
            labels, rec, info = ref
            res["info"] = info
            put(op["dst"], 0, labels, kind="labels", eb=4, nset=info["in_voxels"])
            if info["components"] > CCAP:
                res["rc"] = ENOSPC  # the second form: labels and info complete, the records untouched
            else:
                put("c", 0, rec, kind="records", n=len(rec))
    elif kind == "upload":
        put(op["dst"], 1, upload_mask(op), kind="mask", eb=1, nset=int(upload_mask(op).sum()))
    elif kind in ("window0", "window"):
        out, info = mstat_ref.window(crop, src, op["lo"], op["hi"])
        res["info"], res["intervals"] = info, 1
        put(op["dst"], 0, out, kind="mask", eb=1, nset=info["out_set"])
    elif kind == "morph":
        out, info = morph_ref.morph(src, op["mop"], op["r2"])
        res["info"], res["intervals"] = info, 2 if op["mop"] in (morph_ref.OPEN, morph_ref.CLOSE) else 1
        put(op["dst"], 0, out, kind="mask", eb=1, nset=info["out_set"])
    elif kind == "edt":
        d, info = morph_ref.edt(src, op["target"])
        res["info"], res["intervals"] = info, 1
        put(op["dst"], 0, d, kind="dist2", eb=4, nset=int(np.count_nonzero(d)))
    elif kind == "select":
        out, info = maskcc_ref.select(src, op["rule"], op["conn"], op["min_voxels"], op["seed"])
        res["info"], res["intervals"] = info, 2 + (info["components"] > 0)
        put(op["dst"], 0, out, kind="mask", eb=1, nset=info["out_set"])
    elif kind == "mask_label":
        labels, rec, info = maskcc_ref.label(src, op["conn"])
        res["info"], res["intervals"] = info, 1 + (info["components"] > 0)
        put(op["dst"], 0, labels, kind="labels", eb=4, nset=info["in_voxels"])
        if device and info["components"] > CCAP:
            res["rc"] = ENOSPC
        elif device:
            put("c", 0, rec, kind="records", n=len(rec))
        else:
            res["host"]["records"] = rec
    elif kind == "stats":
        rec, bins, hinfo = mstat_ref.mask_stats(crop, src, ints, op["hist"])
        res["host"].update(region=rec, bins=bins, hist_info=hinfo, values=None if ints else crop[src != 0])
        res["intervals"] = 1
    elif kind == "label_stats":
        table = model.buf["c"][:64 * op["ntable"]].view(label_ref.COMPONENT_DTYPE)
        rec, info = mstat_ref.regions(crop, src, table["label"], ints)
        res["info"], res["intervals"] = info, 1
        res["host"]["exact"] = ints
        if not ints:
            res["host"]["values"] = [crop[src == l] for l in table["label"]]
        put("r", R_OFF, rec, kind="regions", n=len(rec))
    elif kind == "occupancy":
        words, info, _ = mview_ref.occupancy(src, op["label"])
        res["info"], res["intervals"] = info, 1
        put("o", 0, words, kind="words", words_for=(op["src"], model.meta[op["src"]]["ver"], op["label"]))
    elif kind in ("hit", "pick"):
        rect = op["rect"] if kind == "hit" else (op["pick"][0], op["pick"][1], 1, 1)
        rec, info, trace = mview_ref.hit_image(scene_of(st, op), src, origin, op["label"], rect)
        res["intervals"] = 1
        if kind == "hit":
            res["info"] = info
            put("i", 0, rec, kind="image")
        else:
            res["host"]["record"] = rec.reshape(-1)[0]
    elif kind == "mslice":
        out, info = mview_ref.slice_image(v.dims, src, Q.mpr_plane(op), st["slice"], origin, op["label"])
        res["info"], res["intervals"] = info, 1
        put("i", 0, out, kind="image")
    return res


def occupancy_words(ext):
    c = [-(-int(n) // mview_ref.CELL) for n in ext]
    return -(-c[0] * c[1] * c[2] // 32)


def outputs(op):
    """[(register, byte offset, bytes)] a device-form op may write, from the request alone (the
    records of a labelling: up to the register's CCAP)."""
    k = op["op"]
    if k in STATE_OPS or k == "frame" or op.get("form") == "host" or k in ("stats", "pick"):
        return []
    n = voxels_of(op["ext"])
    if k in ("label", "mask_label"):
        return [(op["dst"], 0, 4 * n), ("c", 0, 64 * CCAP)]
    if k == "edt":
        return [(op["dst"], 0, 4 * n)]
    if k == "label_stats":
        return [("r", R_OFF, 64 * op["ntable"])]
    if k == "occupancy":
        return [("o", 0, 4 * occupancy_words(op["ext"]))]
    if k == "hit":
        return [("i", 0, 32 * op["rect"][2] * op["rect"][3])]
    if k == "mslice":
        return [("i", 0, 4 * op["w"] * op["h"])]
    return [(op["dst"], 1 if k == "upload" else 0, n)]


def inputs(op):
    """[(register, byte offset, bytes)] an op reads."""
    out = []
    if op.get("src"):
        out.append((op["src"], op["off"], voxels_of(op["ext"]) * op["eb"]))
    if op["op"] == "label_stats":
        out.append(("c", 0, 64 * op["ntable"]))
    if op.get("occ"):
        out.append(("o", 0, 4 * occupancy_words(op["ext"])))
    return out


def named(op):
    """The registers an op names, input or output, in a fixed order."""
    return sorted({r for r, _, _ in inputs(op) + outputs(op)})


def canon(x):
    """A value of a result as something == compares exactly (arrays by dtype, shape and bytes)."""
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, np.void):
        return x.tobytes()
    if isinstance(x, dict):
        return tuple((k, canon(x[k])) for k in sorted(x))
    if isinstance(x, (list, tuple)):
        return tuple(canon(v) for v in x)
    return x


def same_result(a, b):
    return canon([a[k] for k in ("rc", "info", "host", "writes")]) == canon([b[k] for k in ("rc", "info", "host", "writes")])


def scratch_group(op):
    """The grow-on-demand blocks whose sizes tests/test_maskseq_cpu.py wants to see move."""
    k = op["op"]
    if k in ("hit", "mslice"):
        return "mview staging" if op.get("form") == "host" else None
    return {"morph": "morph", "mask_label": "maskcc", "select": "maskcc", "label_stats": "mstat records",
            "grow": "label", "label": "label"}.get(k)


def upload_mask(op):
    rng = np.random.default_rng(op["mask_seed"])
    return (rng.random(shape_of(op["ext"])) < op["density"]).astype(np.uint8)


# ---- the generator --------------------------------------------------------------------------------
def _pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


def _weighted(rng, table):
    names = list(table)
    w = np.array([table[k] for k in names], np.float64)
    return names[int(rng.choice(len(names), p=w / w.sum()))]


class _Tally:
    """What the seeds before this one have covered, carried from seed to seed in seed order so that the
    draws can lean towards what is missing; a function of the seeds alone."""

    def __init__(self):
        self.model = Model()
        self.pairs = {}    # (producer family, consumer family) handed over to the very next op
        self.layout = {}   # (layout, entry point, form) calls that read the volume
        self.kept = {}     # (family, fits) measurers on a register kept across a volume op
        self.short = {}    # family -> VR_ENOSPC ops
        self.epoch = 0
        self.stream = 4
        self.size = {}     # scratch group -> the voxels of its last call
        self.moves = {}    # (scratch group, +1 or -1) -> calls of 4x / a quarter of the voxels of the one before
        self.last = None   # (register, family) the op before wrote, where it wrote a mask or labels

    def bump(self, table, key):
        table[key] = table.get(key, 0) + 1


class _Gen:
    def __init__(self, seed, tally):
        self.seed, self.t, self.m = seed, tally, tally.model
        self.rng = np.random.default_rng(BASE + seed)
        self.ops, self.refs = [], []
        self.st = dict(vol=None, slice=FULL, size=(64, 48), epoch=tally.epoch)
        self.pending = 0  # measurers still owed to the kept registers after a volume op
        self.want_view = None  # after an occupancy op: (src, label) for the hit or slice that follows

    # -- plumbing --
    def emit(self, op, **kw):
        o = dict(op=op, state=dict(self.st), **kw)
        res = reference(o, self.m)
        self.ops.append(o)
        self.refs.append(None if op in STATE_OPS + ("frame",) else res)
        t = self.t
        if op in NEEDS_VOLUME + ("window0",) and res["rc"] != EINVAL:
            t.bump(t.layout, (LAYOUT[self.st["vol"]], "window" if op == "window0" else op, o.get("form", "device")))
        if res["rc"] == ENOSPC and o.get("short"):
            t.bump(t.short, FAMILY[op])
        if op in CONSUMERS and t.last and o.get("src") == t.last[0] and "stream" in o and res["intervals"]:
            t.bump(t.pairs, (t.last[1], FAMILY[op]))
        if op in MEASURERS + ("window",) and self.m.meta[o["src"]]["vol"] != self.st["vol"]:
            t.bump(t.kept, (FAMILY[op], res["rc"] != EINVAL))
        if scratch_group(o) and res["rc"] != EINVAL and not o.get("short"):
            g, n, was = scratch_group(o), voxels_of(o["ext"]), t.size.get(scratch_group(o))
            if was and (n >= 4 * was or 4 * n <= was):
                t.bump(t.moves, (g, 1 if n > was else -1))
            t.size[g] = n
        wrote = [r for r in res["meta"] if res["meta"][r]["kind"] in ("mask", "labels")]
        fam = "mstat-window" if op in ("window", "window0") else FAMILY.get(op)
        t.last = (wrote[0], fam) if wrote and fam and "stream" in o and res["rc"] == OK else None
        return res

    def stream(self):
        s = _pick(self.rng, [i for i in range(5) if i != self.t.stream])
        self.t.stream = s
        return s

    def form(self, op):
        return dict(form="host" if op in HAS_HOST_FORM and self.rng.random() < 0.25 else "device")

    def short(self, op, form):
        fam = FAMILY[op]
        lean = 4.0 if self.t.short.get(fam, 0) < 5 else 1.0
        return op in HAS_CAPACITY and form["form"] == "device" and self.rng.random() < lean / 12.0

    # -- state ops --
    def op_volume(self, name=None):
        if name is None:  # one of the three other volumes whose layout the entry points have met least
            def met(nm):
                n = [self.t.layout.get((LAYOUT[nm], e, f), 0) for e in ("stats", "label_stats", "window", "hit", "mslice")
                     for f in ("device", "host")]
                return (min(n), sum(n))
            others = sorted((nm for nm in Q.NAMES if nm != self.st["vol"]), key=met)
            name = _pick(self.rng, others[:3])
        self.t.epoch += 1
        self.st.update(vol=name, epoch=self.t.epoch)
        self.emit("volume", name=name)
        self.pending = 1

    def op_slice(self):
        k = int(self.rng.integers(0, 4))
        if k == 3:
            a, b = self.rng.uniform(0.0, 0.3, size=3), self.rng.uniform(0.7, 1.0, size=3)
            box = (tuple(float(F(x)) for x in a), tuple(float(F(x)) for x in b))
        else:
            box = (FULL, SLICE, INSET)[k]
        self.st["slice"] = box
        self.emit("slice")

    def op_resize(self):
        self.st["size"] = _pick(self.rng, [s for s in SIZES if s != self.st["size"]])
        self.emit("resize")

    # -- grids --
    def box(self):
        """(box or None, ext, origin) inside the volume: the whole of it one time in three, else most
        of it or about 1/27 (callseq's voxel_box), so that the sizes move."""
        dims = Q.volume(self.st["vol"]).dims
        r = self.rng.random()
        if r < 1.0 / 3.0:
            return None, dims, (0, 0, 0)
        lo, hi = [], []
        for n in dims:
            if r > 0.62:
                w = max(2, n // 3)
                a = int(self.rng.integers(0, n - w + 1))
                lo.append(a)
                hi.append(a + w)
            else:
                lo.append(int(self.rng.integers(0, n // 4 + 1)))
                hi.append(int(self.rng.integers(n - n // 4, n + 1)))
        return (tuple(lo), tuple(hi)), tuple(hi[a] - lo[a] for a in range(3)), tuple(lo)

    def free(self, regs, *busy):
        """A register of `regs` that is none of `busy`; one that holds nothing yet comes first."""
        cand = [r for r in regs if r not in busy]
        empty = [r for r in cand if self.m.meta[r]["kind"] is None]
        return empty[0] if empty else _pick(self.rng, cand)

    # -- producers --
    def window_of(self, crop_of):
        """(lo, hi) whose window is neither empty nor full over the grid, redrawn up to four times."""
        v = Q.volume(self.st["vol"])
        lo, hi = None, None
        table = [(0.3, None), (0.3, 0.6), (0.15, None), (0.5, None), (0.1, 0.4)]
        for i in self.rng.permutation(len(table)):
            f = table[int(i)]
            lo, hi = v.at(f[0]), INF if f[1] is None else v.at(f[1])
            k = int(label_ref.in_window(crop_of, lo, hi).sum())
            if 0 < k < crop_of.size:
                break
        return lo, hi

    def op_grow(self, kind="grow"):
        v = Q.volume(self.st["vol"])
        box, ext, origin = self.box()
        lo, hi = self.window_of(label_ref.crop(v.f32, box)[0])
        conn = int(_pick(self.rng, [6, 26]))
        form = dict(form="device", stream=self.stream())
        if kind == "label":
            dst = self.free(WORD_REGS)
            return self.emit("label", lo=lo, hi=hi, conn=conn, box=box, ext=ext, origin=origin, dst=dst,
                             short=self.short("label", form), **form)
        labels, _, info = label_ref.label(v.f32, lo, hi, conn, box)
        flat = labels.reshape(-1)
        inside = np.flatnonzero(flat == info["largest_label"]) if info["components"] else []
        out = np.flatnonzero(flat == 0)
        l = int(inside[-1]) if len(inside) and (self.rng.random() < 0.85 or not len(out)) else int(out[len(out) // 2])
        seed = (l % ext[0] + origin[0], (l // ext[0]) % ext[1] + origin[1], l // (ext[0] * ext[1]) + origin[2])
        self.emit("grow", lo=lo, hi=hi, conn=conn, box=box, seed=seed, ext=ext, origin=origin,
                  dst=self.free(BYTE_REGS), **form)

    def op_label(self):
        self.op_grow("label")

    def op_window0(self):
        v = Q.volume(self.st["vol"])
        box, ext, origin = self.box()
        lo, hi = self.window_of(label_ref.crop(v.f32, box)[0])
        form = dict(form="device", stream=self.stream())
        self.emit("window0", lo=lo, hi=hi, ext=ext, origin=origin, eb=1, dst=self.free(BYTE_REGS),
                  short=self.short("window0", form), **form)

    def op_upload(self):
        _, ext, origin = self.box()
        self.emit("upload", ext=ext, origin=origin, density=float(_pick(self.rng, [0.03, 0.3, 0.6, 0.9])),
                  mask_seed=int(self.rng.integers(0, 1 << 30)), dst=self.free(BYTE_REGS), form="device")

    # -- consumers --
    def sources(self, labels_only=False):
        kinds = ("labels",) if labels_only else ("mask", "labels")
        return [r for r in BYTE_REGS + WORD_REGS if self.m.meta[r]["kind"] in kinds]

    def source(self, op, cand=None, form=None):
        """The fields that name the op's source register: the one the op before wrote six times in ten
        (the hand-over), else any; an empty or full array one time in ten at most."""
        if cand is None:
            cand = self.sources(op == "label_stats")
            dims = Q.volume(self.st["vol"]).dims
            ok = [r for r in cand if fits(self.m.meta[r]["ext"], self.m.meta[r]["origin"], dims)]
            if op in NEEDS_VOLUME:
                cand = ok  # (the grids that no longer fit are the kept measurers', after a volume op)
        if not cand:
            return None
        if op in ("hit", "pick", "mslice"):  # a grid of 1/27 of the volume lies beside most central rays
            big = [r for r in cand if 4 * voxels_of(self.m.meta[r]["ext"]) >= Q.volume(self.st["vol"]).voxels]
            if big and self.rng.random() < 0.7:
                cand = big
            if op == "pick":  # one pixel: the two largest grids
                cand = sorted(cand, key=lambda r: -voxels_of(self.m.meta[r]["ext"]))[:2]
        dull = lambda r: self.m.meta[r]["nset"] in (0, voxels_of(self.m.meta[r]["ext"]))
        if self.rng.random() < 0.9 and not all(dull(r) for r in cand):
            cand = [r for r in cand if not dull(r)]
        last = self.t.last
        group = scratch_group(dict(form or {}, op=op))
        prev = self.t.size.get(group)
        moved = [r for r in cand if prev and not prev / 4 < voxels_of(self.m.meta[r]["ext"]) < prev * 4]
        # the direction the group has moved in fewer than six times, while there is one
        owed = [r for r in moved if self.t.moves.get((group, 1 if voxels_of(self.m.meta[r]["ext"]) > prev else -1), 0) < 6]
        if owed and self.rng.random() < 0.85:
            reg = _pick(self.rng, owed)
        elif last and last[0] in cand and self.rng.random() < 0.6:
            reg = last[0]
        elif moved and self.rng.random() < 0.5:  # a grid of 4x or 1/4 the voxels of the group's last call
            reg = _pick(self.rng, moved)
        else:
            reg = _pick(self.rng, cand)
        m = self.m.meta[reg]
        return dict(src=reg, ext=m["ext"], origin=m["origin"], eb=m["eb"], off=m["off"])

    def label_of(self, s, p=0.5):
        """None (ANY), or a label that exists in the source."""
        if self.rng.random() < p:
            return None
        a = self.m.array(s["src"], s["ext"], s["eb"], s["off"]).reshape(-1)
        nz = np.flatnonzero(a)
        if not nz.size:
            return None
        if self.rng.random() < 0.6:  # the label with the most voxels, the smallest one of them
            vals, counts = np.unique(a[nz], return_counts=True)
            return int(vals[int(np.argmax(counts))])
        return int(a[nz[int(self.rng.integers(0, nz.size))]])

    def consumer(self, op, src=None, device=False, form=None):
        if form is None:
            form = self.form(op) if op != "pick" and not device else dict(form="device")
        s = self.source(op, form=form) if src is None else src
        if s is None and op == "label_stats":  # no label array yet: a labelling first
            self.op_label()
            s = self.source(op, form=form)
        if s is None:
            return self.op_grow()
        if op != "pick" and form["form"] == "device":
            form["stream"] = self.stream()
        dims = Q.volume(self.st["vol"]).dims
        ok = fits(s["ext"], s["origin"], dims)
        short = ok and self.short(op, form)
        a = self.m.array(s["src"], s["ext"], s["eb"], s["off"])
        kw = dict(s, short=short, **form)
        if op == "morph":
            kw.update(mop=int(self.rng.integers(0, 4)), r2=int(self.rng.choice(R2, p=R2_P)), dst=self.free(BYTE_REGS, s["src"]))
        elif op == "edt":
            kw.update(target=int(self.rng.integers(0, 2)), dst=self.free(WORD_REGS, s["src"]))
        elif op == "mask_label":
            kw.update(conn=int(_pick(self.rng, [6, 26])), dst=self.free(WORD_REGS, s["src"]))
        elif op == "select":
            rule, conn = int(self.rng.integers(0, 4)), int(_pick(self.rng, [6, 26]))
            flat = a.reshape(-1)
            sel = np.flatnonzero(flat) if self.rng.random() < 0.75 else np.flatnonzero(flat == 0)
            l = int(sel[int(self.rng.integers(0, sel.size))]) if sel.size else 0
            bx, by = s["ext"][0], s["ext"][1]
            minv = 0
            if rule == maskcc_ref.KEEP_MIN_VOXELS:  # the size of one of its components
                sizes = maskcc_ref.label(a, conn)[1]["voxels"]
                minv = int(np.sort(sizes)[int(self.rng.integers(0, sizes.size))]) if sizes.size else 1
            kw.update(rule=rule, conn=conn, min_voxels=minv, seed=(l % bx, (l // bx) % by, l // (bx * by)),
                      dst=self.free(BYTE_REGS, s["src"]))
        elif op == "window":
            v = Q.volume(self.st["vol"])
            lo, hi = (v.at(0.3), INF)
            if ok:  # redrawn while the window takes all of the mask or none of it
                crop = mstat_ref.crop(v.f32, s["origin"], shape_of(s["ext"]))
                table = [(0.1, None), (0.2, None), (0.3, None), (0.45, None), (0.6, None), (0.3, 0.6), (0.5, 0.8), (0.0, 0.4)]
                for j in self.rng.permutation(len(table)):
                    lo, hi = v.at(table[int(j)][0]), INF if table[int(j)][1] is None else v.at(table[int(j)][1])
                    k = int((label_ref.in_window(crop, lo, hi) & (a != 0)).sum())
                    if 0 < k < int(np.count_nonzero(a)):
                        break
                else:  # a small mask beside all of them: from the median of its own values up
                    if np.count_nonzero(a):
                        lo, hi = float(F(np.median(crop[a != 0]))), INF
            kw.update(lo=lo, hi=hi, dst=self.free(BYTE_REGS, s["src"]))
        elif op == "stats":
            v = Q.volume(self.st["vol"])
            hist = None
            if self.rng.random() < 0.5:
                nbins = int(_pick(self.rng, [8, 64, 256, int(self.rng.integers(8, 257))]))
                hist = (nbins,) + ((v.at(0.0), v.at(1.0)) if self.rng.random() < 0.5 else (v.at(0.2), v.at(0.7)))
            kw.update(hist=hist)
            kw.pop("short")
        elif op == "label_stats":
            nrec = self.m.meta["c"].get("n", 0) if self.m.meta["c"]["kind"] == "records" else 0
            r = self.rng.random()
            nt = nrec if r < 0.45 or nrec < 8 else (max(1, nrec // 6) if r < 0.8 else int(self.rng.integers(1, nrec)))
            prev = self.t.size.get("ntable")
            if prev and nrec and self.rng.random() < 0.9:  # 4x or 1/4 of the table before, the rarer move first
                up, down = (self.t.moves.get(("ntable", d), 0) for d in (1, -1))
                if nrec >= 4 * prev and (up <= down or prev < 4):
                    nt = nrec
                elif prev >= 4:
                    nt = max(1, min(nrec, prev // 5))
            if ok and nt and not short:
                if prev and (nt >= 4 * prev or 4 * nt <= prev):
                    self.t.bump(self.t.moves, ("ntable", 1 if nt > prev else -1))
                self.t.size["ntable"] = nt
            kw.update(ntable=int(nt))
        elif op == "occupancy":
            kw.update(label=self.label_of(s))
            self.want_view = (s["src"], kw["label"])
        elif op in ("hit", "pick", "mslice"):
            label, occ = self.label_of(s, 0.6 if op == "mslice" else 0.7), False
            w = self.m.meta["o"].get("words_for")
            if self.want_view and self.want_view[0] == s["src"]:
                label = self.want_view[1]
            if (w == (s["src"], self.m.meta[s["src"]]["ver"], label) and form["form"] == "device" and op != "pick"
                    and self.rng.random() < 0.9):
                occ = True
            self.want_view = None
            kw.update(label=label, occ=occ)
            if op == "mslice":
                # redrawn while the plane misses the array (as callseq redraws an isovalue): from the fourth
                # draw on an axis plane of the two larger sizes through the source's grid
                for t in range(8):
                    w, h = _pick(self.rng, Q.MPR_SIZES[:2] if t >= 3 else Q.MPR_SIZES)
                    if self.rng.random() < 0.6 or t >= 3:  # an axis plane, through the source's grid four times in five
                        ax, u = int(self.rng.integers(0, 3)), self.rng.uniform(0.2, 0.8)
                        if self.rng.random() < 0.8 or t >= 3:
                            u = (s["origin"][ax] + u * s["ext"][ax]) / dims[ax]
                        box = self.st["slice"]  # (a plane outside the slice box samples nothing)
                        u = min(max(u, box[0][ax] + 0.03), box[1][ax] - 0.03)
                        plane = ("axis", ax, float(F(u)))
                    else:
                        plane = ("oblique", float(_pick(self.rng, [0.05, 0.02])))
                    kw.update(plane=plane, w=w, h=h, ns=int(_pick(self.rng, [1, 5])), mpr_op=_pick(self.rng, list(Q.OPS)))
                    if not ok or mview_ref.slice_image(dims, a, Q.mpr_plane(kw), self.st["slice"], s["origin"],
                                                       label)[1]["hits"]:
                        break
            else:
                W, H = self.st["size"]
                rw, rh = (1, 1) if (W, H) == (1, 1) else _pick(self.rng, Q.HIT_RECTS)
                rect = (W // 2 - rw // 2, H // 2 - rh // 2, rw, rh)
                kw.update(step=float(_pick(self.rng, [0.005, 0.0])), rect=rect,
                          pick=(rect[0] + int(self.rng.integers(0, rw)), rect[1] + int(self.rng.integers(0, rh))))
                # the camera is redrawn while the rectangle holds fewer than ten hits, three times at most
                best = None
                for cam in self.rng.permutation(len(Q.CAMS))[:(6 if op == "pick" else 4) if ok else 1]:
                    kw.update(cam=int(cam))
                    if not ok:
                        break
                    rec = mview_ref.hit_image(scene_of(self.st, kw), a, s["origin"], label, rect)[0]
                    ys, xs = np.nonzero(rec["step"] != mview_ref.MISS)
                    if best is None or ys.size > best[1].size:
                        best = (int(cam), ys, xs)
                    if ys.size >= min(10, rw * rh):
                        break
                if best:
                    kw.update(cam=best[0])
                    ys, xs = best[1], best[2]
                if op == "pick":
                    kw.pop("short")
                    if ok and ys.size and self.rng.random() < 0.9:  # a pixel that hits, where there is one
                        j = int(self.rng.integers(0, ys.size))
                        kw.update(pick=(rect[0] + int(xs[j]), rect[1] + int(ys[j])))
        return self.emit(op, **kw)

    def kept_measurer(self):
        """After a volume op: a measurer on a register the volume before left, leaning towards the
        (family, fits or not) met least."""
        dims = Q.volume(self.st["vol"]).dims
        old = [r for r in self.sources() if self.m.meta[r]["epoch"] < self.st["epoch"]]
        if not old:
            return False
        # (once a refusal has been met eight times per family the fitting grids come first: they test more)
        want = sorted(((min(self.t.kept.get((f, ok), 0), 8), not ok, self.rng.random(), f, ok)
                       for f in ("mstat", "mview") for ok in (True, False)))
        want = [w[1:] for w in want]
        for _, _, fam, ok in want:
            cand = [r for r in old if fits(self.m.meta[r]["ext"], self.m.meta[r]["origin"], dims) == ok]
            if not cand:
                continue
            op = _pick(self.rng, ("stats", "window", "label_stats") if fam == "mstat" else ("mslice", "mslice", "hit", "occupancy"))
            labels = [r for r in cand if self.m.meta[r]["kind"] == "labels"]
            if op == "label_stats" and labels:
                cand = labels
            elif op == "label_stats":
                op = "stats"
            if op == "hit" and self.st["size"] == (1, 1) and self.rng.random() < 0.9:
                self.op_resize()
            if fam == "mview" and ok:  # the larger half of the kept grids: a small one lies beside most rays
                cand = sorted(cand, key=lambda r: -voxels_of(self.m.meta[r]["ext"]))[:(len(cand) + 1) // 2]
            self.consumer(op, self.source(op, cand))
            return True
        return False

    def handover(self):
        """The op before wrote a mask or labels: the consumer family that has read that producer
        family's output least often as the very next op."""
        reg, fam = self.t.last
        if self.m.meta[reg]["nset"] in (0, voxels_of(self.m.meta[reg]["ext"])):
            return False
        fams = sorted(("morph", "maskcc", "mstat", "mview"), key=lambda c: (self.t.pairs.get((fam, c), 0), self.rng.random()))
        ops = {"morph": ("morph", "morph", "edt"), "maskcc": ("select", "select", "mask_label"),
               "mstat": ("stats", "window", "label_stats"), "mview": ("hit", "mslice", "occupancy", "hit")}[fams[0]]
        op = _pick(self.rng, ops)
        if op == "label_stats" and self.m.meta[reg]["kind"] != "labels":
            op = "stats"
        m = self.m.meta[reg]
        src = dict(src=reg, ext=m["ext"], origin=m["origin"], eb=m["eb"], off=m["off"])
        if op in NEEDS_VOLUME and not fits(m["ext"], m["origin"], Q.volume(self.st["vol"]).dims):
            return False
        self.consumer(op, src, device=self.t.pairs.get((fam, fams[0]), 0) < 3)
        return True

    def step(self):
        last = self.t.last
        rare = last and min(self.t.pairs.get((last[1], c), 0) for c in ("morph", "maskcc", "mstat", "mview")) < 3
        if rare and self.handover():
            return
        if self.pending:
            self.pending -= 1
            if self.kept_measurer():
                return
        if self.want_view and self.rng.random() < 0.95:
            reg = self.want_view[0]
            m = self.m.meta[reg]
            if m["kind"] in ("mask", "labels"):
                op = _pick(self.rng, ["hit", "mslice"])
                if op == "hit" and self.st["size"] == (1, 1):
                    op = "mslice"
                return self.consumer(op, dict(src=reg, ext=m["ext"], origin=m["origin"], eb=m["eb"], off=m["off"]),
                                     device=True)  # (the words go to the device forms alone)
        if last and self.rng.random() < 0.6 and self.handover():
            return
        # an entry point and form that has not read this volume's layout three times comes first, six times in ten
        lay = LAYOUT[self.st["vol"]]
        needy = [(k, f) for k in ("stats", "label_stats", "window", "hit", "mslice") for f in ("device", "host")
                 if self.t.layout.get((lay, k, f), 0) < 3]
        if needy and self.rng.random() < 0.6:
            op, f = _pick(self.rng, needy)
            if op == "hit" and self.st["size"] == (1, 1):
                self.op_resize()
            return self.consumer(op, form=dict(form=f))
        op = _weighted(self.rng, WEIGHTS)
        if op in STATE_OPS or op in PRODUCERS:
            return getattr(self, "op_" + op)()
        if op in ("hit", "pick") and self.st["size"] == (1, 1) and self.rng.random() < 0.85:
            self.op_resize()
        self.consumer(op)

    def run(self):
        self.op_volume(Q.NAMES[(3 * self.seed + int(self.rng.integers(0, 2))) % len(Q.NAMES)])
        self.pending = 0
        self.op_slice()
        self.op_resize()
        getattr(self, "op_" + _pick(self.rng, ["grow", "grow", "label", "window0"]))()
        self.pending = 1  # the registers the seed before left were written under another volume
        while len(self.ops) < 4 + STEPS:
            self.step()
        self.emit("frame", cam=int(self.rng.integers(0, len(Q.CAMS))), shading=1, ert_eps=0.0, exact_gradient=0)
        return self.ops, self.refs


def generate(seeds):
    """{seed: (op list, result list)} of seeds 0 .. seeds - 1, generated afresh in seed order."""
    tally = _Tally()
    return {seed: _Gen(seed, tally).run() for seed in range(seeds)}


_seqs = {}


def _made(seed):
    if seed not in _seqs:
        _seqs.update(generate(max(int(seed) + 1, len(SEEDS))))
    return _seqs[seed]


def sequence(seed):
    """The op list of `seed` (the same list every time; treat it as read-only)."""
    return _made(seed)[0]


def cached(seed):
    """The results of sequence(seed), one per op (None for a state op and the frame), once per session."""
    return _made(seed)[1]


def reference(op, model, state=None):
    """Advance `model` through `op` and return what the op must write (compute's dict)."""
    res = compute(op, model, state)
    model.apply(res)
    return res


def frame_state(op):
    """The closing frame's state in callseq's terms (composite_ref)."""
    v = Q.volume(op["state"]["vol"])
    return dict(vol=op["state"]["vol"], window=(float(F(v.lo)), float(F(v.hi))), tf="tf1", slice=op["state"]["slice"],
                size=op["state"]["size"], mode="composite")


def describe(op):
    """One word or so per op for a failure's log."""
    k = op["op"]
    if k == "volume":
        return "volume:" + op["name"]
    if k in STATE_OPS or k == "frame":
        return k
    s = k + ("/host" if op.get("form") == "host" else "@%d" % op["stream"] if "stream" in op else "")
    if "src" in op:
        s += ":%s%s" % (op["src"], "".join(">" + d for d in ([op["dst"]] if "dst" in op else [])))
    elif "dst" in op:
        s += ":>" + op["dst"]
    return s + ("!short" if op.get("short") else "") + "[%dx%dx%d]" % tuple(op["ext"])
