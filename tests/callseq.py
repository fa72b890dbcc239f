"""Random sequences over the whole API boundary and their references -- test helper
(tests/test_callseq_cpu.py, tests/test_gpu_callseq.py).

sequence(seed) is a list of op dicts drawn from numpy.random.default_rng alone: nothing in it
depends on what a device returned, so the same list is replayed on the GPU and inspected on the
CPU.  The generator keeps the model state beside the list -- volume, value window, TF, slicing box,
framebuffer size, render mode, isovalue -- and every op carries a copy of the state AFTER it
(op["state"]): a checking op is judged against exactly that.

State ops:    volume, window, tf, slice, resize, mode, isovalue.
Checking ops: frame, mpr, hist, mesh, label (with region growing), hit (with one pick), burst
              (frames in flight plus one device-form analysis call, half of them with a histogram).

Every sequence starts with the seven state ops, so a context that other seeds have worn is set to
the whole model first; STEPS random ops follow, and the close: a mode op back to the composite
mode where it is another, and a shaded composite frame that must still equal the oracle -- so
across seeds every mode is rendered before and after the composite one only.  Three rules add a resize in front of a checking
op (an op of its own in the list, and a transition like any other):
  * a frame or burst in a ray mode (MIP, MinIP, mean, ISO) is referenced at 45x35 at most;
  * a hit rectangle must be able to hold ten hits, so hits never run on the 1x1 framebuffer;
  * hits are referenced on the small framebuffers only.
And an ISO hit whose isovalue lies outside 0.1 .. 0.35 of the volume's range -- another volume left it
behind -- gets an isovalue op first: its rectangle must hold ten hits.  For the same reason an
OPACITY hit takes threshold 1.0 under the opaque ramp only, and under a band TF with a narrowed
window (transparent to most of the volume) an ENTRY hit is asked instead.  The other way round, a
composite frame on a small framebuffer resizes to one of the two large ones (>= 256 rows) three
times in ten: the ray modes keep bringing the size down.

Knobs that shape an upload (narrow, u8_layout) are plain context fields read by the next upload
(vr_debug_set_knob), so they change on a live context: each volume op carries both, set just
before its upload.

reference(op) computes what the model state demands through the per-feature references
(pyoracle, proj_ref, iso_ref, mpr_ref, hist_ref, mesh_ref, label_ref, hit_ref); cached(seed)
keeps one list of them per seed for the session.  The composite frames go against the C oracle at
replay time (composite_ref): whether the kernel read the binary16 difference field is known to the
context alone, and the oracle costs milliseconds.

Cost, measured with the generator and the references alone on the CPU (one core): the 56 seeds
of SEEDS take 0.8 s on average, 0.4 s in the median and 4.3 s at most, 44 s together.  The
ray-mode frames (0.65 s at 32x24) and the hit rectangles are nearly all of it, so a seed whose
ray-mode frames are estimated past RAY_BUDGET goes back to the composite mode.

The draws lean on a tally that is carried from seed to seed in seed order (_Tally): a volume op
takes one of the three volumes the calls have seen least, a burst the analysis call its volume has
met least, a mode op prefers a pair of modes not yet rendered one after the other, and the op
draw leans towards rendering such a pair while it stands (a ray mode after another ray mode has to
happen inside one seed: every seed closes in the composite mode).  That is what lets 56 seeds meet
the coverage conditions of tests/test_callseq_cpu.py; sequence(seed) stays a function of the seed.
"""
import numpy as np

import hist_ref
import hit_ref
import iso_ref
import label_ref
import label_scenes
import mesh_ref
import mpr_ref
import proj_ref
import pyoracle
import synth
import vr_amd
from hit_scenes import THRESHOLDS
from range_scenes import CLEAR, FULL, INSET, SLICE

F = np.float32
INF = float("inf")
SEEDS = range(56)
STEPS = 16
RAY_BUDGET = 2.0

STATE_OPS = ("volume", "window", "tf", "slice", "resize", "mode", "isovalue")
CHECK_OPS = ("frame", "mpr", "hist", "mesh", "label", "hit", "burst")
ANALYSES = ("hit_image_device", "render_mpr_device", "mesh_device", "label_device", "region_grow_device")
# every kind the coverage conditions count: the checking ops and each burst's analysis call
KINDS = CHECK_OPS + ANALYSES

MODES = {"composite": vr_amd.MODE_COMPOSITE, "mip": vr_amd.MODE_MIP, "minip": vr_amd.MODE_MINIP,
         "mean": vr_amd.MODE_MEAN, "iso": vr_amd.MODE_ISO}
RAY_MODES = ("mip", "minip", "mean", "iso")
TFS = {"tf1": synth.tf1, "tf2": synth.tf2, "tfc": synth.tf_color, "band": lambda: synth.tf_band(0.15, 0.9),
       "band_hi": lambda: synth.tf_band(0.2, 0.95)}
CAMS = [(1.6, None), (1.6, (40.0, 25.0)), (1.6, (360.0, 0.0)), (2.0, (180.0, 140.0)),
        (3.0, None), (1.3, (-120.0, 80.0))]
SMALL = [(32, 24), (45, 35), (1, 1), (64, 48)]
LARGE = [(231, 257), (320, 288)]  # >= 256 rows (vr_render's row bands): composite frames only
RAY_SIZES = [(32, 24), (45, 35), (1, 1)]
RAY_BURST_SIZES = [(32, 24), (1, 1)]  # (two references a burst)
HIT_SIZES = [(32, 24), (45, 35), (64, 48)]
HIT_RECTS = [(8, 6), (6, 8), (12, 4), (7, 5)]  # at most 48 pixels, around the image centre
HIT_KINDS = {"entry": vr_amd.HIT_ENTRY, "opacity": vr_amd.HIT_OPACITY, "max": vr_amd.HIT_MAX,
             "min": vr_amd.HIT_MIN, "iso": vr_amd.HIT_ISO}
MPR_SIZES = [(32, 24), (45, 35), (17, 3), (1, 1)]
OPS = {"max": mpr_ref.OP_MAX, "mean": mpr_ref.OP_MEAN, "min": mpr_ref.OP_MIN}


# ---- the volume pool ------------------------------------------------------------------------------
def _ints():
    g = synth.gaussians_numpy((27, 21, 19), seed=8)
    return np.rint(g / g.max() * 255.0).astype(np.float32)


def _int16():
    g = synth.gaussians_numpy((64, 48, 40), seed=7)
    return np.rint(g / g.max() * 30000.0 - 2000.0).astype(np.int16)


# name -> (maker of the upload array (nz, ny, nx), knobs set before the upload, vr::StorageType
# the context must report, busy: thousands of mesh vertices); TAGS: the voxel type the analysis
# kernels are instantiated with, which tells plain 8-bit bricks from yz-quads
POOL = {
    "g20": (lambda: synth.gaussians_numpy((20, 18, 22), seed=11), dict(narrow=0), 4, False),
    "g13d": (lambda: (synth.gaussians_numpy((13, 7, 21), seed=3) * 7.0 - 1.0).astype(np.float64), {}, 4, False),
    "g33u8": (lambda: synth.gaussians_numpy((33, 40, 27), seed=5, dtype=np.uint8), dict(u8_layout=0), 0, False),
    "g48q": (lambda: synth.gaussians_numpy((48, 40, 36), seed=6, dtype=np.uint8), dict(u8_layout=1), 0, False),
    "g64s": (_int16, {}, 3, False),
    "ints": (_ints, dict(narrow=1), 0, False),
    "noise": (label_scenes.noise, dict(narrow=0), 4, True),
    "checker": (label_scenes.checker, dict(narrow=0), 4, True),
}
NAMES = list(POOL)
TAGS = {"g20": "float", "g13d": "float", "g33u8": "unsigned char", "g48q": "vr::Quad8<unsigned char>",
        "g64s": "short", "ints": "vr::Quad8<unsigned char>", "noise": "float", "checker": "float"}
KNOB_DEFAULTS = dict(narrow=1, u8_layout=-1)
_vols = {}


class Volume:
    def __init__(self, name):
        make, knobs, storage, busy = POOL[name]
        self.name, self.storage, self.busy, self.tag = name, storage, busy, TAGS[name]
        self.knobs = dict(KNOB_DEFAULTS, **knobs)
        self.up = np.ascontiguousarray(make())
        self.f32 = np.ascontiguousarray(self.up, dtype=np.float32)
        for a in (self.up, self.f32):
            a.setflags(write=False)
        nz, ny, nx = self.up.shape
        self.dims = (nx, ny, nz)
        self.voxels = nx * ny * nz
        self.lo, self.hi = float(self.f32.min()), float(self.f32.max())

    def at(self, f):
        """The value at fraction f of the data range, as the f32 the ABI takes."""
        return float(F(self.lo + f * (self.hi - self.lo)))


def volume(name):
    """One read-only Volume per name for the whole session."""
    if name not in _vols:
        _vols[name] = Volume(name)
    return _vols[name]


def box_voxels(box, dims):
    if box is None:
        return dims[0] * dims[1] * dims[2]
    return int(np.prod([box[1][a] - box[0][a] for a in range(3)]))


# ---- the generator --------------------------------------------------------------------------------
def _pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


def _weighted(rng, table):
    names = list(table)
    w = np.array([table[n] for n in names], np.float64)
    return names[int(rng.choice(len(names), p=w / w.sum()))]


WEIGHTS = {"volume": 2.2, "window": 2.2, "tf": 0.8, "slice": 0.8, "resize": 0.8, "mode": 1.4, "isovalue": 0.6,
           "frame": 2.0, "mpr": 1.2, "hist": 1.2, "mesh": 1.3, "label": 1.3, "hit": 1.2, "burst": 4.0}
MODE_WEIGHTS = {"composite": 0.48, "mip": 0.13, "minip": 0.13, "mean": 0.13, "iso": 0.13}


class _Tally:
    """What the seeds before this one have visited: (kind, volume) -> calls, (mode, mode) ->
    rendered one after the other.  Carried from seed to seed in seed order, so that the draws can
    lean towards what is still missing; a function of the seeds alone, like everything here."""

    def __init__(self):
        self.visits = {(k, n): 0 for k in KINDS for n in NAMES}
        self.pairs = {(a, b): 0 for a in MODES for b in MODES}
        self.rendered = None  # the mode of the last frame or burst

    def on_volume(self, name):
        """How little the calls have seen of a volume: its least-met kind, then all its calls."""
        return (min(self.visits[(k, name)] for k in KINDS), sum(self.visits[(k, name)] for k in KINDS))


class _Gen:
    def __init__(self, seed, tally):
        self.seed = seed
        self.rng = np.random.default_rng(9000 + seed)
        self.ops = []
        self.st = {}
        self.tally = tally
        self.held = []
        self.cost = 0.0  # the seed's ray-mode references so far, in estimated seconds

    def emit(self, op, **kw):
        if self.held is not None:  # the seven opening ops: each carries the whole opening state
            self.held.append((op, kw))
            return
        self.ops.append(dict(op=op, state=dict(self.st), **kw))
        t = self.tally
        if op in CHECK_OPS:
            t.visits[(op, self.st["vol"])] += 1
        if op == "burst":
            t.visits[(kw["analysis"]["kind"], self.st["vol"])] += 1
        if op in ("frame", "burst"):
            if t.rendered is not None:
                t.pairs[(t.rendered, self.st["mode"])] += 1
            t.rendered = self.st["mode"]

    # -- state ops --
    def op_volume(self, name=None):
        if name is None:  # one of the three other volumes the calls have visited least
            others = sorted((n for n in NAMES if n != self.st.get("vol")), key=self.tally.on_volume)
            name = _pick(self.rng, others[:3])
        v = volume(name)
        self.st["vol"] = name
        self.st["window"] = (float(F(v.lo)), float(F(v.hi)))  # an upload brings its own window
        self.emit("volume", name=name)

    def op_window(self):
        v = volume(self.st["vol"])
        which = _pick(self.rng, ["data", "narrow", "wide"])
        f = {"data": (0.0, 1.0), "narrow": (0.25, 0.7), "wide": (-0.3, 1.4)}[which]
        self.st["window"] = (v.at(f[0]), v.at(f[1]))
        self.emit("window", which=which)

    def op_tf(self):
        self.st["tf"] = _pick(self.rng, [n for n in TFS if n != self.st.get("tf")])
        self.emit("tf")

    def op_slice(self):
        k = int(self.rng.integers(0, 4))
        if k == 3:
            a = self.rng.uniform(0.0, 0.4, size=3)
            b = self.rng.uniform(0.6, 1.0, size=3)
            box = (tuple(float(F(x)) for x in a), tuple(float(F(x)) for x in b))
        else:
            box = (FULL, SLICE, INSET)[k]
        self.st["slice"] = box
        self.emit("slice")

    def op_resize(self, size=None):
        if size is None:
            pool = SMALL + (LARGE if self.st.get("mode") == "composite" or self.rng.random() < 0.3 else [])
            size = _pick(self.rng, [s for s in pool if s != self.st.get("size")])
        self.st["size"] = tuple(size)
        self.emit("resize")

    def op_mode(self, mode=None):
        seen = self.tally.pairs
        table = {m: w * (1.0 if seen[(self.tally.rendered or m, m)] else 40.0) for m, w in MODE_WEIGHTS.items()
                 if m != self.st.get("mode")}
        self.st["mode"] = _weighted(self.rng, table) if mode is None else mode
        self.emit("mode")

    def afford(self, frames):
        """The references of ray-mode frames are what a seed costs (about 0.65 s at 32x24): past
        RAY_BUDGET the seed goes back to the composite mode, with a mode op of its own."""
        if self.st["mode"] in RAY_MODES:
            if self.cost > RAY_BUDGET:
                self.op_mode("composite")
            else:
                self.cost += frames * 0.65 * max(self.st["size"][0] * self.st["size"][1], 768) / 768.0

    def op_isovalue(self, fractions=(0.15, 0.3, 0.45)):
        self.st["iso"] = volume(self.st["vol"]).at(_pick(self.rng, fractions))
        self.emit("isovalue")

    # -- the pieces of the checking ops --
    def voxel_box(self, small_ok=True, small=False):
        """None, or a half-open voxel box inside the volume: most of it, or (small) about 1/27."""
        nx, ny, nz = dims = volume(self.st["vol"]).dims
        r = self.rng.random()
        if not small and r < 0.4:
            return None
        lo, hi = [], []
        for n in dims:
            if small or (small_ok and r > 0.8):
                w = max(2, n // 3)
                a = int(self.rng.integers(0, n - w + 1))
                lo.append(a)
                hi.append(a + w)
            else:
                lo.append(int(self.rng.integers(0, n // 4 + 1)))
                hi.append(int(self.rng.integers(n - n // 4, n + 1)))
        return (tuple(lo), tuple(hi))

    def small_size_for(self, sizes):
        """A resize op of its own where the framebuffer is none of `sizes` (the first one mostly)."""
        if self.st["size"] not in sizes:
            p = np.array([0.6] + [0.4 / len(sizes)] * (len(sizes) - 1))
            self.op_resize(sizes[int(self.rng.choice(len(sizes), p=p / p.sum()))])

    def frame_spec(self, cam=None):
        cam = int(self.rng.integers(0, len(CAMS))) if cam is None else cam
        mode = self.st["mode"]
        spec = dict(cam=cam, shading=0, ert_eps=0.0, exact_gradient=0)
        if mode == "composite":
            spec.update(shading=int(self.rng.random() < 0.6), ert_eps=float(self.rng.choice([0.0, 1e-5])),
                        exact_gradient=int(self.rng.random() < 0.4))
        elif mode == "iso":
            spec.update(shading=int(self.rng.random() < 0.6))
        return spec

    def mpr_spec(self):
        w, h = _pick(self.rng, MPR_SIZES)
        ns = int(_pick(self.rng, [1, 5]))
        op = _pick(self.rng, list(OPS))
        if self.rng.random() < 0.5:
            plane = ("axis", int(self.rng.integers(0, 3)), float(F(self.rng.uniform(0.2, 0.8))))
        else:
            plane = ("oblique", float(_pick(self.rng, [0.05, 0.02])))
        return dict(plane=plane, w=w, h=h, ns=ns, mpr_op=op)

    def hist_spec(self):
        v = volume(self.st["vol"])
        nbins = int(_pick(self.rng, [8, 64, 256, int(self.rng.integers(8, 257))]))
        lo, hi = (v.at(0.0), v.at(1.0)) if self.rng.random() < 0.5 else (v.at(0.2), v.at(0.7))
        return dict(nbins=nbins, lo=lo, hi=hi, box=self.voxel_box())

    def mesh_spec(self):
        v = volume(self.st["vol"])
        empty = self.rng.random() < 0.06
        iso = float(F(v.hi + 1.0)) if empty else v.at(float(_pick(self.rng, [0.3, 0.6])))
        normals = bool(self.rng.random() < 0.5)
        # a busy volume's thousands of normals cost the reference seconds: a small box then
        box = self.voxel_box(small=True) if v.busy and normals else self.voxel_box(small_ok=False)
        return dict(iso=iso, closed=bool(self.rng.random() < 0.5), normals=normals, box=box, empty=bool(empty))

    def label_spec(self):
        v = volume(self.st["vol"])
        lo, hi = (v.at(0.3), INF) if self.rng.random() < 0.5 else (v.at(0.3), v.at(0.6))
        return dict(lo=lo, hi=hi, conn=int(_pick(self.rng, [6, 26])), box=self.voxel_box())

    def hit_spec(self):
        W, H = self.st["size"]
        rw, rh = _pick(self.rng, HIT_RECTS)
        rect = (W // 2 - rw // 2, H // 2 - rh // 2, rw, rh)
        kind = _pick(self.rng, list(HIT_KINDS))
        v = volume(self.st["vol"])
        if kind == "opacity" and self.st["tf"].startswith("band") and self.st["window"][0] > v.lo:
            kind = "entry"  # a band TF under a narrow window is transparent to most of the volume
        if kind == "iso" and not v.at(0.1) <= self.st["iso"] <= v.at(0.35):
            self.op_isovalue((0.15, 0.3))  # (an isovalue another volume left behind hits nothing here)
        th = float(F(_pick(self.rng, THRESHOLDS))) if kind == "opacity" else 0.5
        # threshold 1.0 needs a transmittance that rounds to 0: the opaque ramp reaches it anywhere
        if kind == "opacity" and th == 1.0 and self.st["tf"] != "tf1":
            th = float(F(THRESHOLDS[0]))
        pick = (rect[0] + int(self.rng.integers(0, rw)), rect[1] + int(self.rng.integers(0, rh)))
        return dict(cam=int(self.rng.integers(0, len(CAMS))), hit=kind, threshold=th, rect=rect, pick=pick)

    # -- checking ops --
    def op_frame(self):
        self.afford(1)
        if self.st["mode"] in RAY_MODES:
            self.small_size_for(RAY_SIZES)
        elif self.st["size"] not in LARGE and self.rng.random() < 0.3:
            self.op_resize(_pick(self.rng, LARGE))  # (the ray modes keep bringing the size down)
        self.emit("frame", **self.frame_spec())

    def op_mpr(self):
        self.emit("mpr", **self.mpr_spec())

    def op_hist(self):
        self.emit("hist", **self.hist_spec())

    def op_mesh(self):
        self.emit("mesh", **self.mesh_spec())

    def op_label(self):
        self.emit("label", **self.label_spec())

    def op_hit(self):
        self.small_size_for(HIT_SIZES)
        self.emit("hit", **self.hit_spec())

    def op_burst(self):
        self.afford(2)
        ray = self.st["mode"] in RAY_MODES
        # the analysis call this volume has met least: every volume meets every one
        met = {a: self.tally.visits[(a, self.st["vol"])] for a in ANALYSES}
        kind = _pick(self.rng, [a for a in ANALYSES if met[a] == min(met.values())])
        if kind == "hit_image_device":
            self.small_size_for([s for s in HIT_SIZES if not ray or s in RAY_BURST_SIZES])
        elif ray:
            self.small_size_for(RAY_BURST_SIZES)
        n = 2 if ray else int(self.rng.integers(2, 4))
        cams = self.rng.permutation(len(CAMS))[:n]
        frames = [self.frame_spec(int(c)) for c in cams]
        spec = {"hit_image_device": self.hit_spec, "render_mpr_device": self.mpr_spec, "mesh_device": self.mesh_spec,
                "label_device": self.label_spec, "region_grow_device": self.label_spec}[kind]()
        hist = self.hist_spec() if self.rng.random() < 0.5 else None
        self.emit("burst", frames=frames, analysis=dict(kind=kind, **spec), hist=hist)

    def run(self):
        self.op_volume(NAMES[(3 * self.seed + int(self.rng.integers(0, 2))) % len(NAMES)])
        self.op_window()
        self.op_tf()
        self.op_slice()
        self.op_resize()
        self.op_mode()
        self.op_isovalue()
        held, self.held = self.held, None
        for op, kw in held:
            self.emit(op, **kw)
        for _ in range(STEPS):
            # a checking op this volume has not met twice is drawn more often
            table = {k: w * (2.5 if k in CHECK_OPS and self.tally.visits[(k, self.st["vol"])] < 2 else 1.0)
                     for k, w in WEIGHTS.items()}
            if self.st["mode"] in RAY_MODES:  # their references cost: fewer bursts, and sooner out again
                table["burst"] *= 0.4
                table["mode"] *= 2.0
            # a pair of modes not yet rendered one after the other: render it once the mode is set,
            # and leave a ray mode that was rendered for one it has not been followed by
            t, mode = self.tally, self.st["mode"]
            if t.rendered not in (None, mode) and not t.pairs[(t.rendered, mode)]:
                table["frame"] *= 6.0
            elif t.rendered == mode and mode in RAY_MODES and not all(t.pairs[(mode, m)] for m in MODES if m != mode):
                table["mode"] *= 4.0
            getattr(self, "op_" + _weighted(self.rng, table))()
        # the close: after all of it a composite frame still equals the oracle
        if self.st["mode"] != "composite":
            self.op_mode("composite")
        self.emit("frame", **dict(self.frame_spec(), shading=1))
        return self.ops


def generate(seeds):
    """{seed: op list} of seeds 0 .. seeds - 1, generated afresh in seed order."""
    tally = _Tally()
    return {seed: _Gen(seed, tally).run() for seed in range(seeds)}


_seqs = {}


def sequence(seed):
    """The op list of `seed` (the same list every time; treat it as read-only)."""
    if seed not in _seqs:
        _seqs.update(generate(max(int(seed) + 1, len(SEEDS))))
    return _seqs[seed]


def describe(op):
    """One word or so per op for a failure's log."""
    if op["op"] == "volume":
        return "volume:" + op["name"]
    if op["op"] == "burst":
        return "burst:%s:%d%s" % (op["analysis"]["kind"], len(op["frames"]), "+hist" if op["hist"] else "")
    if op["op"] in ("window", "tf", "mode", "resize"):
        key = {"window": "which", "tf": None, "mode": None, "resize": None}[op["op"]]
        val = op[key] if key else op["state"][{"tf": "tf", "mode": "mode", "resize": "size"}[op["op"]]]
        return "%s:%s" % (op["op"], val)
    if op["op"] == "hit":
        return "hit:" + op["hit"]
    return op["op"]


def work_size(op):
    """The voxels of the request's box (hist, mesh, label; a burst's analysis call)."""
    return box_voxels(op["box"], volume(op["state"]["vol"]).dims)


def kinds_of(op):
    """The kinds of KINDS a checking op counts as, with the dict that holds each one's request."""
    if op["op"] not in CHECK_OPS:
        return []
    out = [(op["op"], op)]
    if op["op"] == "burst":
        out.append((op["analysis"]["kind"], dict(op["analysis"], state=op["state"])))
    return out


# ---- the references -------------------------------------------------------------------------------
def camera(i):
    r, rot = CAMS[i]
    return vr_amd.make_camera(radius=r, rotate=rot).to_vr_camera()


def frame_params(spec, skip, inflight=1):
    return vr_amd.default_params(shading=spec["shading"], ert_eps=spec["ert_eps"], skip_empty=skip,
                                 exact_gradient=spec["exact_gradient"], frames_in_flight=inflight)


def scene_of(state, cam, params):
    v = volume(state["vol"])
    W, H = state["size"]
    return pyoracle.Scene.from_params(v.f32, state["window"][0], state["window"][1], TFS[state["tf"]](), cam,
                                      W, H, params, smin=state["slice"][0], smax=state["slice"][1])


def composite_ref(state, spec, skip, half, inflight=1):
    """The C oracle's composite frame (restating the binary16 field where the kernel read it)."""
    v = volume(state["vol"])
    W, H = state["size"]
    sc = pyoracle.Scene.from_params(v.f32, state["window"][0], state["window"][1], TFS[state["tf"]](),
                                    camera(spec["cam"]), W, H, frame_params(spec, skip, inflight),
                                    state["slice"][0], state["slice"][1], grad_f16=half)
    return sc.render()[0].astype(np.float32)


def ray_ref(state, spec):
    """(frame, stats) of a ray-mode frame; None in the composite mode (composite_ref's)."""
    mode = state["mode"]
    if mode == "composite":
        return None
    sc = scene_of(state, camera(spec["cam"]), frame_params(spec, 0))
    if mode == "iso":
        img, st, _, _ = iso_ref.render(sc, state["iso"])
    else:
        img, st = proj_ref.render(sc, mode)
        st = dict(st, shaded_samples=0)
    return img, st


def mpr_plane(spec):
    pl = spec["plane"]
    if pl[0] == "axis":
        return mpr_ref.axis_plane(pl[1], pl[2], spec["w"], spec["h"], spec["ns"], 0.013, OPS[spec["mpr_op"]])
    return mpr_ref.oblique_plane(pl[1], spec["w"], spec["h"], spec["ns"], OPS[spec["mpr_op"]], 0.013)


def mpr_result(state, spec):
    v = volume(state["vol"])
    return mpr_ref.render(v.f32, state["window"][0], state["window"][1], TFS[state["tf"]](), mpr_plane(spec),
                          state["slice"], CLEAR)


def hist_result(state, spec):
    return hist_ref.histogram(volume(state["vol"]).f32, spec["lo"], spec["hi"], spec["nbins"], spec["box"])


def mesh_result(state, spec):
    return mesh_ref.extract(volume(state["vol"]).f32, spec["iso"], spec["closed"], spec["normals"], spec["box"])


def label_result(state, spec):
    """(labels, records, info), and the two region-grow requests: a seed in the largest component
    (its last voxel, not its root) and one outside the window, each with (mask, record) -- None
    where the labelling has no such voxel."""
    v = volume(state["vol"])
    box = spec["box"]
    ref = label_ref.label(v.f32, spec["lo"], spec["hi"], spec["conn"], box)
    labels, rec, info = ref
    origin = (0, 0, 0) if box is None else box[0]
    bz, by, bx = labels.shape
    flat = labels.reshape(-1)

    def grow(l):
        seed = (l % bx + origin[0], (l // bx) % by + origin[1], l // (bx * by) + origin[2])
        return (seed,) + label_ref.region_grow(None, seed, spec["lo"], spec["hi"], spec["conn"], box, labelled=ref)

    inside = grow(int(np.flatnonzero(flat == info["largest_label"])[-1])) if info["components"] else None
    out = np.flatnonzero(flat == 0)
    outside = grow(int(out[len(out) // 2])) if len(out) else None
    return ref, inside, outside


def hit_key(spec):
    return ("opacity", float(F(spec["threshold"]))) if spec["hit"] == "opacity" else spec["hit"]


def hit_result(state, spec):
    sc = scene_of(state, camera(spec["cam"]), vr_amd.default_params())
    return hit_ref.walk(sc, state["iso"], (spec["threshold"],), rect=spec["rect"])


ANALYSIS_RESULT = {"hit_image_device": hit_result, "render_mpr_device": mpr_result, "mesh_device": mesh_result,
                   "label_device": label_result, "region_grow_device": label_result}
RESULT = {"mpr": mpr_result, "hist": hist_result, "mesh": mesh_result, "label": label_result, "hit": hit_result}


def reference(op, state=None):
    """What the model state (op["state"], or a stand-in) demands of a checking op.
    frame: ray_ref's pair or None; burst: dict(frames=[...], analysis=..., hist=...)."""
    st = op["state"] if state is None else state
    if op["op"] == "frame":
        return ray_ref(st, op)
    if op["op"] == "burst":
        a = op["analysis"]
        return dict(frames=[ray_ref(st, f) for f in op["frames"]], analysis=ANALYSIS_RESULT[a["kind"]](st, a),
                    hist=hist_result(st, op["hist"]) if op["hist"] else None)
    return RESULT[op["op"]](st, op)


_refs = {}


def cached(seed):
    """The references of sequence(seed), one per op (None for a state op), once per session."""
    if seed not in _refs:
        _refs[seed] = [reference(op) if op["op"] in CHECK_OPS else None for op in sequence(seed)]
    return _refs[seed]
