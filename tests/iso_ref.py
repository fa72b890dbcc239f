"""Reference for the first-hit isosurface (include/vr/vr_iso.h) -- test helper.

The loop of vr_iso.h in np.float32, built like tests/proj_ref.py from the oracle's own pieces:
Scene.pixel_ray for the entry point and direction, or_trilinear for every sample, or_tf_sample
for the transfer function.  The gradient and the Phong model are restated here from
oracle/oracle.c (texel_coord, voxel, dvox, grad_cell, powi, march_pixel_impl's shading) with a
true single-rounding fmaf from libm.  mode="composite" runs the same loop with the reference's
composite, shading included, which tests/test_iso_cpu.py compares with the C oracle bit for
bit: that pins the ray, the gradient and the Phong restatement, so the ISO frames produced
from them can serve as the reference.

Slow (ctypes calls per sample): frames of 32x24 to 45x35.
"""
import ctypes as C
import ctypes.util

import numpy as np

import pyoracle

F = np.float32

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.restype = C.c_float
_libm.fmaf.argtypes = [C.c_float, C.c_float, C.c_float]


def lerpf(a, b, w):
    """oracle.c lerpf: fmaf(w, b - a, a), the subtraction rounded to f32 first."""
    return F(_libm.fmaf(w, F(b) - F(a), a))


def texel_coord(p, n):
    u = F(p) * F(n) - F(0.5)
    f = np.floor(u)
    return int(f), F(u - f)


def voxel(vol, x, y, z):
    nz, ny, nx = vol.shape
    if x < 0 or y < 0 or z < 0 or x >= nx or y >= ny or z >= nz:
        return F(0.0)
    return vol[z, y, x]


def grad_cell(vol, i, j, k, ax, ay, az, axis):
    e = (axis == 0, axis == 1, axis == 2)

    def dv(x, y, z):
        return voxel(vol, x + e[0], y + e[1], z + e[2]) - voxel(vol, x - e[0], y - e[1], z - e[2])

    c00 = lerpf(dv(i, j, k), dv(i + 1, j, k), ax)
    c10 = lerpf(dv(i, j + 1, k), dv(i + 1, j + 1, k), ax)
    c01 = lerpf(dv(i, j, k + 1), dv(i + 1, j, k + 1), ax)
    c11 = lerpf(dv(i, j + 1, k + 1), dv(i + 1, j + 1, k + 1), ax)
    return lerpf(lerpf(c00, c10, ay), lerpf(c01, c11, ay), az)


def powi(x, p):
    r = F(1.0)
    while p:
        if p & 1:
            r = r * x
        p >>= 1
        if p:
            x = x * x
    return r


def phong(s, vol, pos, d, rgb):
    """oracle.c:626-651 at `pos`: rgb -> rgb * (ka + kd ndl) + ks ndl^p; a zero gradient leaves it."""
    nz, ny, nx = vol.shape
    i, ax = texel_coord(pos[0], nx)
    j, ay = texel_coord(pos[1], ny)
    k, az = texel_coord(pos[2], nz)
    g = [grad_cell(vol, i, j, k, ax, ay, az, a) for a in range(3)]
    wx, wy, wz = g[0] * F(nx), g[1] * F(ny), g[2] * F(nz)
    g2 = wx * wx + wy * wy + wz * wz
    if g2 > F(0.0):
        inv = F(1.0) / np.sqrt(g2)
        ndl = np.abs((wx * F(d[0]) + wy * F(d[1]) + wz * F(d[2])) * inv)
        kdiff = F(s.ka) + F(s.kd) * ndl
        spec = F(s.ks) * powi(ndl, int(s.spec_power))
        rgb = [rgb[0] * kdiff + spec, rgb[1] * kdiff + spec, rgb[2] * kdiff + spec]
    return rgb


def render(scene, iso=0.0, mode="iso"):
    """scene: pyoracle.Scene (its shading and Phong constants are used).  Returns (frame
    (H, W, 4) float32, stats, hit_step (H, W) int, -1 where the ray did not hit, cap (H, W) bool)
    with stats = rays, steps, in-slab search samples (`samples`) and shaded_samples."""
    assert mode in ("iso", "composite")
    s = scene.s
    W, H = s.width, s.height
    vol = np.ascontiguousarray(scene.vol, dtype=np.float32)
    nz, ny, nx = vol.shape
    L = pyoracle.lib()
    vp = vol.ctypes.data
    tf = scene.tf
    iso = F(iso)
    clear = [F(s.clear[i]) for i in range(4)]
    smin = [F(s.smin[a]) for a in range(3)]
    smax = [F(s.smax[a]) for a in range(3)]
    step, vmin = F(s.step), F(s.vmin)
    rng = F(s.vmax) - F(s.vmin)
    with np.errstate(all="ignore"):
        nsteps = int(F(s.ray_dist) / step)
    ert = F(s.ert_eps)
    one, zero, half = F(1.0), F(0.0), F(0.5)
    out = np.empty((H, W, 4), np.float32)
    hit_step = np.full((H, W), -1, np.int64)
    cap = np.zeros((H, W), bool)
    rays = steps = samples = shaded = 0

    def tri(p):
        return F(L.or_trilinear(vp, nx, ny, nz, C.c_float(p[0]), C.c_float(p[1]), C.c_float(p[2])))

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
                hit = prev = False
                q = None
                for k in range(nsteps):
                    if p0 > one or p1 > one or p2 > one or p0 < zero or p1 < zero or p2 < zero:
                        break
                    steps += 1
                    if (p0 < smax[0] and p1 < smax[1] and p2 < smax[2] and p0 > smin[0]
                            and p1 > smin[1] and p2 > smin[2]):
                        dv = tri((p0, p1, p2))
                        samples += 1
                        if mode == "iso":
                            if dv >= iso:  # a NaN sample never hits
                                hit = True
                                hit_step[py, px] = k
                                break
                            prev, q = True, (p0, p1, p2)
                        else:
                            sc = pyoracle.tf_sample(tf, (dv - vmin) / rng)
                            if s.shading and sc[3] > zero:
                                shaded += 1
                                sc[:3] = phong(s, vol, (p0, p1, p2), d, [sc[0], sc[1], sc[2]])
                            cr = cr + (sc[0] * sc[3]) * T
                            cg = cg + (sc[1] * sc[3]) * T
                            cb = cb + (sc[2] * sc[3]) * T
                            T = T * (one - sc[3])
                            if T == zero or T < ert:
                                break
                    else:
                        prev = False
                    p0, p1, p2 = p0 + s0, p1 + s1, p2 + s2
                if mode == "composite":
                    A = one - T
                    omA = one - A
                    out[py, px] = (cr * A + clear[0] * omA, cg * A + clear[1] * omA,
                                   cb * A + clear[2] * omA, A * A + clear[3] * omA)
                    continue
                if not hit:
                    out[py, px] = clear
                    continue
                hi = (p0, p1, p2)
                cap[py, px] = not prev
                if prev:
                    lo = q
                    for _ in range(4):
                        mid = ((lo[0] + hi[0]) * half, (lo[1] + hi[1]) * half, (lo[2] + hi[2]) * half)
                        if tri(mid) >= iso:
                            hi = mid
                        else:
                            lo = mid
                sc = pyoracle.tf_sample(tf, (iso - vmin) / rng)
                rgb = [sc[0], sc[1], sc[2]]
                if s.shading:
                    shaded += 1
                    rgb = phong(s, vol, hi, d, rgb)
                out[py, px] = (rgb[0], rgb[1], rgb[2], one)
    return out, dict(rays=rays, steps=steps, samples=samples, shaded_samples=shaded), hit_step, cap


_cache = {}


def cached(key, make_scene, iso=0.0, mode="iso"):
    """One reference per key for the whole test session (never modified by the tests)."""
    k = (key, float(iso), mode)
    if k not in _cache:
        img, st, hs, cap = render(make_scene(), iso, mode)
        for a in (img, hs, cap):
            a.setflags(write=False)
        _cache[k] = (img, st, hs, cap)
    return _cache[k]
