"""Reference for the maximum-intensity projection (include/vr/vr_modes.h) -- test helper.

A float32 restatement of the ray loop of oracle/oracle.c march_pixel_impl built from the
oracle's own pieces: Scene.pixel_ray for the entry point and direction, or_trilinear for every
sample, or_tf_sample for the transfer function, np.float32 arithmetic for the position update,
the bounds break, the strict slab test and the blend.  mode="mip" keeps the largest sample
(np.fmax: a NaN sample leaves it) and looks the TF up once; mode="composite" runs the same loop
with the reference's composite, which tests/test_mip_cpu.py compares with the C oracle bit for
bit: that pins this loop, so the MIP frames it produces can serve as the reference.

Slow (a ctypes call per sample): frames of 32x24 to 48x36.
"""
import ctypes as C

import numpy as np

import pyoracle

F = np.float32


def render(scene, mode="mip"):
    """scene: pyoracle.Scene.  Returns (frame (H, W, 4) float32, stats) with stats = rays,
    steps and in-slab samples (`samples`), as the oracle counts them."""
    assert mode in ("mip", "composite")
    s = scene.s
    W, H = s.width, s.height
    vol = np.ascontiguousarray(scene.vol, dtype=np.float32)
    nz, ny, nx = vol.shape
    L = pyoracle.lib()
    vp = vol.ctypes.data
    tf = scene.tf
    clear = [F(s.clear[i]) for i in range(4)]
    smin = [F(s.smin[a]) for a in range(3)]
    smax = [F(s.smax[a]) for a in range(3)]
    step, vmin = F(s.step), F(s.vmin)
    rng = F(s.vmax) - F(s.vmin)
    with np.errstate(all="ignore"):
        nsteps = int(F(s.ray_dist) / step)
    ert = F(s.ert_eps)
    one, zero = F(1.0), F(0.0)
    out = np.empty((H, W, 4), np.float32)
    rays = steps = samples = 0
    with np.errstate(all="ignore"):
        for py in range(H):
            for px in range(W):
                ok, tex, _frag, d = scene.pixel_ray(px, py)
                if not ok:
                    out[py, px] = clear
                    continue
                rays += 1
                p0, p1, p2 = F(tex[0]), F(tex[1]), F(tex[2])
                s0, s1, s2 = F(d[0]) * step, F(d[1]) * step, F(d[2]) * step
                T, cr, cg, cb = one, zero, zero, zero
                m, hit = F(-np.inf), False
                for _ in range(nsteps):
                    if p0 > one or p1 > one or p2 > one or p0 < zero or p1 < zero or p2 < zero:
                        break
                    steps += 1
                    if (p0 < smax[0] and p1 < smax[1] and p2 < smax[2] and p0 > smin[0]
                            and p1 > smin[1] and p2 > smin[2]):
                        dv = F(L.or_trilinear(vp, nx, ny, nz, C.c_float(p0), C.c_float(p1), C.c_float(p2)))
                        samples += 1
                        if mode == "mip":
                            m = np.fmax(m, dv)
                            hit = True
                        else:
                            sc = pyoracle.tf_sample(tf, (dv - vmin) / rng)
                            cr = cr + (sc[0] * sc[3]) * T
                            cg = cg + (sc[1] * sc[3]) * T
                            cb = cb + (sc[2] * sc[3]) * T
                            T = T * (one - sc[3])
                            if T == zero or T < ert:
                                break
                    p0, p1, p2 = p0 + s0, p1 + s1, p2 + s2
                if mode == "mip" and hit:
                    sc = pyoracle.tf_sample(tf, (m - vmin) / rng)
                    cr = (sc[0] * sc[3]) * one
                    cg = (sc[1] * sc[3]) * one
                    cb = (sc[2] * sc[3]) * one
                    T = one * (one - sc[3])
                A = one - T
                omA = one - A
                out[py, px] = (cr * A + clear[0] * omA, cg * A + clear[1] * omA,
                               cb * A + clear[2] * omA, A * A + clear[3] * omA)
    return out, dict(rays=rays, steps=steps, samples=samples)


_cache = {}


def cached(key, make_scene, mode="mip"):
    """One reference frame per key for the whole test session (never modified by the tests)."""
    k = (key, mode)
    if k not in _cache:
        img, st = render(make_scene(), mode)
        img.setflags(write=False)
        _cache[k] = (img, st)
    return _cache[k]
