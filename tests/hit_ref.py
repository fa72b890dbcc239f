"""Reference for the hit records (include/vr/vr_hit.h) -- test helper.

The loops of vr_hit.h in np.float32, built like tests/iso_ref.py from the oracle's own pieces:
Scene.pixel_ray for the entry point and direction, or_trilinear for every sample, or_tf_sample
for the transfer function.  One walk per scene visits every step of every covered ray once and
produces the records and the counters of all five kinds and of a list of OPACITY thresholds;
`depth` is formed in np.float64, left to right, and cast once.

tests/test_hit_cpu.py pins it independently: its ISO step and cap mask against iso_ref, OPACITY
against ENTRY and a closed form, MAX's value against proj_ref's MIP pixel.

Slow (ctypes calls per sample): frames of 32x24 to 45x35.
"""
import ctypes as C

import numpy as np

import pyoracle

F = np.float32
DTYPE = np.dtype([("pos", "<f4", 3), ("depth", "<f4"), ("value", "<f4"), ("step", "<u4")])
MISS_STEP = 0xFFFFFFFF
KINDS = ("entry", "opacity", "max", "min", "iso")  # enum vr_hit_kind, in order


def miss_records(shape):
    r = np.zeros(shape, DTYPE)
    r["depth"] = np.inf
    r["step"] = MISS_STEP
    return r


def depth_of(pos, cam):
    """vr_hit.h: (float) sqrt(dx*dx + dy*dy + dz*dz), d_a = ((double)pos[a] - 0.5) - (double)cam[a]."""
    d = [(np.float64(F(pos[a])) - np.float64(0.5)) - np.float64(F(cam[a])) for a in range(3)]
    return F(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))


class Walk:
    """What walk() returns.  records[key] is an (H, W) DTYPE array and stats[key] the vr_stats
    of vr_hit_count_work, with key one of "entry", "max", "min", "iso" or ("opacity", threshold);
    covered and cap (ISO hits at the ray's first in-slab sample after an off-slab step or none)
    are (H, W) bool."""

    def __init__(self, H, W, keys):
        self.records = {k: miss_records((H, W)) for k in keys}
        self.stats = {k: dict(rays=0, samples=0, shaded_samples=0, steps=0, skipped_samples=0)
                      for k in keys}
        self.covered = np.zeros((H, W), bool)
        self.cap = np.zeros((H, W), bool)

    def hits(self, key):
        return self.records[key]["step"] != MISS_STEP


def walk(scene, iso=0.0, thresholds=(0.5,), rect=None):
    """scene: pyoracle.Scene (its step, ray_dist, slice box, window and TF are used; shading and
    ert_eps are not).  rect = (x0, y0, w, h): walk the pixels of that rectangle only; the arrays
    keep the frame's shape, every other pixel stays a miss and uncovered, and the counters are
    those of the rectangle."""
    s = scene.s
    W, H = s.width, s.height
    vol = np.ascontiguousarray(scene.vol, dtype=np.float32)
    nz, ny, nx = vol.shape
    L = pyoracle.lib()
    vp = vol.ctypes.data
    tf = scene.tf
    iso = F(iso)
    thresholds = [F(t) for t in thresholds]
    keys = ["entry", "max", "min", "iso"] + [("opacity", float(t)) for t in thresholds]
    smin = [F(s.smin[a]) for a in range(3)]
    smax = [F(s.smax[a]) for a in range(3)]
    cam = [F(s.cam_pos[a]) for a in range(3)]
    step, vmin = F(s.step), F(s.vmin)
    rng = F(s.vmax) - F(s.vmin)
    with np.errstate(all="ignore"):
        nsteps = int(F(s.ray_dist) / step)
    one, zero, half = F(1.0), F(0.0), F(0.5)
    out = Walk(H, W, keys)
    x0, y0, rw, rh = (0, 0, W, H) if rect is None else (int(v) for v in rect)
    assert 0 <= x0 and 0 <= y0 and rw >= 1 and rh >= 1 and x0 + rw <= W and y0 + rh <= H

    def tri(p):
        return F(L.or_trilinear(vp, nx, ny, nz, C.c_float(p[0]), C.c_float(p[1]), C.c_float(p[2])))

    def put(key, py, px, pos, value, k, n_steps, n_samples, total):
        """A hit at loop index k (None: no hit) after n_samples in-slab samples; the counters run
        up to and including the step and sample that ended the walk."""
        st = out.stats[key]
        st["rays"] += 1
        if k is None:
            st["steps"] += total[0]
            st["samples"] += total[1]
            return
        st["steps"] += n_steps
        st["samples"] += n_samples
        st["shaded_samples"] += 1
        r = out.records[key]
        r["pos"][py, px] = pos
        r["depth"][py, px] = depth_of(pos, cam)
        r["value"][py, px] = value
        r["step"][py, px] = k

    with np.errstate(all="ignore"):
        for py in range(y0, y0 + rh):
            for px in range(x0, x0 + rw):
                ok, tex, _frag, d = scene.pixel_ray(px, py)
                if not ok:
                    continue
                out.covered[py, px] = True
                p0, p1, p2 = F(tex[0]), F(tex[1]), F(tex[2])
                s0, s1, s2 = F(d[0]) * step, F(d[1]) * step, F(d[2]) * step
                n_steps = 0
                samples = []  # (k, pos, d, the step before was an in-slab sample) in step order
                before = False
                for k in range(nsteps):
                    if p0 > one or p1 > one or p2 > one or p0 < zero or p1 < zero or p2 < zero:
                        break
                    n_steps += 1
                    if (p0 < smax[0] and p1 < smax[1] and p2 < smax[2] and p0 > smin[0]
                            and p1 > smin[1] and p2 > smin[2]):
                        samples.append((k, (p0, p1, p2), tri((p0, p1, p2)), before))
                        before = True
                    else:
                        before = False
                    p0, p1, p2 = p0 + s0, p1 + s1, p2 + s2
                total = (n_steps, len(samples))

                # ENTRY: the first in-slab sample
                if samples:
                    k, pos, dv, _ = samples[0]
                    put("entry", py, px, pos, dv, k, k + 1, 1, total)
                else:
                    put("entry", py, px, None, None, None, 0, 0, total)

                # MAX / MIN: the first sample equal to the extreme; NaN never updates
                for key, start, better in (("max", F(-np.inf), lambda a, b: a > b),
                                           ("min", F(np.inf), lambda a, b: a < b)):
                    m, best = start, None
                    for smp in samples:
                        if better(smp[2], m):
                            m, best = smp[2], smp
                    if best is None:
                        put(key, py, px, None, None, None, 0, 0, total)
                    else:  # the whole ray is walked
                        put(key, py, px, best[1], m, best[0], total[0], total[1], total)

                # OPACITY: the composite's transmittance, one product per in-slab sample
                found = {float(t): None for t in thresholds}
                T = one
                for n, (k, pos, dv, _) in enumerate(samples):
                    a = pyoracle.tf_sample(tf, (dv - vmin) / rng)[3]
                    T = T * (one - a)
                    A = one - T
                    for t in thresholds:
                        if found[float(t)] is None and A >= t:
                            found[float(t)] = (k, pos, dv, n + 1)
                    if all(v is not None for v in found.values()):
                        break
                for t in thresholds:
                    f = found[float(t)]
                    if f is None:
                        put(("opacity", float(t)), py, px, None, None, None, 0, 0, total)
                    else:
                        put(("opacity", float(t)), py, px, f[1], f[2], f[0], f[0] + 1, f[3], total)

                # ISO: the first sample at or above the isovalue (a NaN never hits), refined by
                # four bisection steps towards the in-slab sample before it
                hit = None
                for n, smp in enumerate(samples):
                    if smp[2] >= iso:
                        hit = (n, smp)
                        break
                if hit is None:
                    put("iso", py, px, None, None, None, 0, 0, total)
                else:
                    n, (k, hi, dv, prev) = hit
                    out.cap[py, px] = not prev
                    if prev:
                        lo = samples[n - 1][1]
                        for _ in range(4):
                            mid = ((lo[0] + hi[0]) * half, (lo[1] + hi[1]) * half, (lo[2] + hi[2]) * half)
                            if tri(mid) >= iso:
                                hi = mid
                            else:
                                lo = mid
                    put("iso", py, px, hi, tri(hi), k, k + 1, n + 1, total)
    return out


_cache = {}


def cached(key, make_scene, iso=0.0, thresholds=(0.5,)):
    """One walk per key for the whole test session (never modified by the tests)."""
    k = (key, float(iso), tuple(float(F(t)) for t in thresholds))
    if k not in _cache:
        w = walk(make_scene(), iso, thresholds)
        for a in list(w.records.values()) + [w.covered, w.cap]:
            a.setflags(write=False)
        _cache[k] = w
    return _cache[k]
