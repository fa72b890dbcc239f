"""Reference for multi-planar reformat images (include/vr/vr_mpr.h) -- test helper.

The header's loop, restated from the oracle's own pieces, in the pattern of tests/proj_ref.py:
np.float64 positions (origin + cx du + cy dv + t dn, left to right) rounded to np.float32 once,
the bounds test and the strict slab test in np.float32, pyoracle's or_trilinear for every sample,
np.fmax from -inf / np.fmin from +inf / an np.float32 running sum in s order divided by
np.float32(n), pyoracle.tf_sample for the one lookup and np.float32 arithmetic for the composite
step and the blend over the clear colour.

tests/test_mpr_cpu.py pins it independently of or_trilinear's weights with closed forms (planes
whose every position is a texel centre).

Slow (a ctypes call per sample): images of at most 48x36 with at most 9 samples, except where a
test needs the size itself.
"""
import ctypes as C

import numpy as np

import pyoracle

F = np.float32
D = np.float64
OP_MAX, OP_MIN, OP_MEAN = 0, 1, 2
CLEAR = (0.11, 0.11, 0.11, 1.0)
FULL = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def plane(origin, du, dv, dn, width, height, nsamples=1, op=OP_MAX):
    """The plane as the C struct holds it: f32 vectors."""
    return dict(origin=np.asarray(origin, F), du=np.asarray(du, F), dv=np.asarray(dv, F),
                dn=np.asarray(dn, F), width=int(width), height=int(height), nsamples=int(nsamples),
                op=int(op))


def axis_plane(axis, position, width, height, nsamples=1, spacing=0.0, op=OP_MAX):
    """vr_mpr_axis_plane restated (all f32): the whole cross-section at `position` along `axis`."""
    origin = np.full(3, 0.5, F)
    origin[axis] = F(position)
    du, dv, dn = np.zeros(3, F), np.zeros(3, F), np.zeros(3, F)
    dn[axis] = F(spacing)
    ru, rv = F(1.0) / F(width), F(1.0) / F(height)
    if axis == 2:
        du[0], dv[1] = ru, rv
    else:
        du[0 if axis == 1 else 1], dv[2] = ru, -rv
    return plane(origin, du, dv, dn, width, height, nsamples, op)


def oblique_plane(pitch, width, height, nsamples=1, op=OP_MAX, spacing=0.013, origin=(0.5, 0.5, 0.5)):
    """The (1, 1, 1) plane through `origin`: du along (1,-1,0)/sqrt 2, dv along (1,1,-2)/sqrt 6,
    both of length `pitch`; dn along (1,1,1)/sqrt 3 of length `spacing`."""
    u = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0)
    v = np.array([1.0, 1.0, -2.0]) / np.sqrt(6.0)
    n = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
    return plane(origin, u * pitch, v * pitch, n * spacing, width, height, nsamples, op)


def positions(pl, px, py):
    """The (nsamples, 3) f32 positions of pixel (px, py)."""
    cx = D(px) + D(0.5) - D(0.5) * D(pl["width"])
    cy = D(py) + D(0.5) - D(0.5) * D(pl["height"])
    o, du, dv, dn = (pl[k].astype(D) for k in ("origin", "du", "dv", "dn"))
    q = np.empty((pl["nsamples"], 3), F)
    for s in range(pl["nsamples"]):
        t = D(s) - D(0.5) * D(pl["nsamples"] - 1)
        for a in range(3):
            q[s, a] = F(((o[a] + cx * du[a]) + cy * dv[a]) + t * dn[a])
    return q


def render(vol, vmin, vmax, tf, pl, box=FULL, clear=CLEAR):
    """(frame (H, W, 4) float32, stats) of the plane over vol (nz, ny, nx) f32; stats = rays,
    steps, samples as vr_mpr_count_work counts them."""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    nz, ny, nx = vol.shape
    L = pyoracle.lib()
    vp = vol.ctypes.data
    tf = np.ascontiguousarray(np.asarray(tf, dtype=np.uint32))
    W, H, op = pl["width"], pl["height"], pl["op"]
    assert op in (OP_MAX, OP_MIN, OP_MEAN)
    clear = [F(c) for c in clear]
    smin = [F(x) for x in box[0]]
    smax = [F(x) for x in box[1]]
    vmin_, rng = F(vmin), F(vmax) - F(vmin)
    one, zero = F(1.0), F(0.0)
    out = np.empty((H, W, 4), np.float32)
    rays = steps = samples = 0
    with np.errstate(all="ignore"):
        for py in range(H):
            for px in range(W):
                m = F(-np.inf) if op == OP_MAX else F(np.inf)
                acc, n, stepped = F(0.0), 0, False
                for q in positions(pl, px, py):
                    p0, p1, p2 = q
                    if p0 > one or p1 > one or p2 > one or p0 < zero or p1 < zero or p2 < zero:
                        continue  # not a step (and not the end of the ray)
                    steps += 1
                    stepped = True
                    if not (p0 < smax[0] and p1 < smax[1] and p2 < smax[2] and p0 > smin[0]
                            and p1 > smin[1] and p2 > smin[2]):
                        continue
                    d = F(L.or_trilinear(vp, nx, ny, nz, C.c_float(p0), C.c_float(p1), C.c_float(p2)))
                    samples += 1
                    n += 1
                    if op == OP_MAX:
                        m = np.fmax(m, d)
                    elif op == OP_MIN:
                        m = np.fmin(m, d)
                    else:
                        acc = acc + d
                rays += stepped
                T, cr, cg, cb = one, zero, zero, zero
                if n:
                    v = acc / F(n) if op == OP_MEAN else m
                    sc = pyoracle.tf_sample(tf, (v - vmin_) / rng)
                    cr = (sc[0] * sc[3]) * one
                    cg = (sc[1] * sc[3]) * one
                    cb = (sc[2] * sc[3]) * one
                    T = one * (one - sc[3])
                A = one - T
                omA = one - A
                out[py, px] = (cr * A + clear[0] * omA, cg * A + clear[1] * omA,
                               cb * A + clear[2] * omA, A * A + clear[3] * omA)
    return out, dict(rays=rays, steps=steps, samples=samples)


def pixel_of(value, vmin, vmax, tf, clear=CLEAR):
    """The epilogue alone: the f32 RGBA pixel that shows density `value` (closed forms)."""
    one = F(1.0)
    with np.errstate(all="ignore"):
        sc = pyoracle.tf_sample(np.asarray(tf, np.uint32), (F(value) - F(vmin)) / (F(vmax) - F(vmin)))
        T = one * (one - sc[3])
        A = one - T
        omA = one - A
        return np.array([((sc[i] * sc[3]) * one) * A + F(clear[i]) * omA for i in range(3)]
                        + [A * A + F(clear[3]) * omA], np.float32)


_cache = {}


def cached(key, make):
    """One reference (frame, stats) per key for the whole test session (never modified)."""
    if key not in _cache:
        img, st = make()
        img.setflags(write=False)
        _cache[key] = (img, st)
    return _cache[key]
