"""Reference for the maximum-, minimum- and mean-intensity projections
(include/vr/vr_modes.h) -- test helper.

A float32 restatement of the ray loop of oracle/oracle.c march_pixel_impl built from the
oracle's own pieces (Scene.pixel_ray for the entry point and direction, or_trilinear for every
sample, or_tf_sample for the transfer function, np.float32 arithmetic for the position update,
the bounds break, the strict slab test and the blend), keeping one quantity of the ray and
looking the TF up once when the ray took an in-slab sample:

  mode="mip"        the largest sample (np.fmax from -inf: a NaN sample leaves it);
  mode="minip"      the smallest sample (np.fmin from +inf, likewise);
  mode="mean"       an np.float32 running sum, one addition per in-slab sample in step order,
                    divided by np.float32(n) (the correctly rounded f32 quotient);
  mode="composite"  the reference's composite, which tests/test_proj_cpu.py compares with the C
                    oracle bit for bit (and tests/test_mip_cpu.py): that pins this loop, so the
                    frames of the other modes can serve as the reference.

It never skips.  order= restates the mean with its additions in another order ("reverse", or
"batch4": each batch of four summed apart first) -- not a reference, only the proof that the
parity scenes can tell a wrong order from the right one.

Beside the frame it returns a CPU model of the per-brick value ranges the library keeps for f32
volumes (csrc/vr_internal.h): padded index = logical + 2, a brick holds the elements of padded
indices 8 b .. 8 b + 8 per axis, zero outside the volume, and an f32 element is the pair
{v(z), v(z + 1)}, so the values a brick stores reach padded z = 8 b + 9.  `const_samples` is
the number of in-slab samples whose brick holds one finite value only: what the mean's range
skipping leaves out.

Slow (a ctypes call per sample): frames of 32x24 to 48x36.
"""
import ctypes as C

import numpy as np

import pyoracle

F = np.float32
PAD, BRICK = 2, 8
MODES = ("mip", "minip", "mean", "composite")


def brick_grid(n):
    """Bricks along an axis of n voxels (vr_internal.h bricks_for, 8-cell bricks)."""
    return (n + 3) // BRICK + 1


def brick_ranges(vol):
    """(lo, hi, const) over the brick grid (z, y, x) of an f32 volume (nz, ny, nx): the range of
    every value a brick stores (NaN, NaN with a NaN inside), and whether it is one finite value."""
    vol = np.asarray(vol, dtype=np.float32)
    nz, ny, nx = vol.shape
    gz, gy, gx = brick_grid(nz), brick_grid(ny), brick_grid(nx)
    padded = np.zeros((gz * BRICK + 2, gy * BRICK + 1, gx * BRICK + 1), np.float32)
    padded[PAD:PAD + nz, PAD:PAD + ny, PAD:PAD + nx] = vol
    lo = np.empty((gz, gy, gx), np.float32)
    hi = np.empty_like(lo)
    for bz in range(gz):
        for by in range(gy):
            for bx in range(gx):
                sub = padded[BRICK * bz:BRICK * bz + BRICK + 2, BRICK * by:BRICK * by + BRICK + 1,
                             BRICK * bx:BRICK * bx + BRICK + 1]
                lo[bz, by, bx], hi[bz, by, bx] = sub.min(), sub.max()  # NaN propagates
    with np.errstate(invalid="ignore"):
        const = (lo == hi) & np.isfinite(lo)
    return lo, hi, const


def _cell(p, n):
    """The low texel of the sample's cell along an axis (the oracle's texel_coord, in f32)."""
    return int(np.floor(p * F(n) - F(0.5)))


def render(scene, mode="mean", order="step"):
    """scene: pyoracle.Scene.  Returns (frame (H, W, 4) float32, stats) with stats = rays, steps,
    in-slab samples (`samples`), as the oracle counts them, and `const_samples` (module text)."""
    assert mode in MODES and order in ("step", "reverse", "batch4")
    s = scene.s
    W, H = s.width, s.height
    vol = np.ascontiguousarray(scene.vol, dtype=np.float32)
    nz, ny, nx = vol.shape
    const = brick_ranges(vol)[2]
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
    rays = steps = samples = const_samples = 0
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
                ds = []  # the ray's in-slab samples, in step order
                for _ in range(nsteps):
                    if p0 > one or p1 > one or p2 > one or p0 < zero or p1 < zero or p2 < zero:
                        break
                    steps += 1
                    if (p0 < smax[0] and p1 < smax[1] and p2 < smax[2] and p0 > smin[0]
                            and p1 > smin[1] and p2 > smin[2]):
                        dv = F(L.or_trilinear(vp, nx, ny, nz, C.c_float(p0), C.c_float(p1), C.c_float(p2)))
                        samples += 1
                        if const[(_cell(p2, nz) + PAD) // BRICK, (_cell(p1, ny) + PAD) // BRICK,
                                 (_cell(p0, nx) + PAD) // BRICK]:
                            const_samples += 1
                        if mode == "composite":
                            sc = pyoracle.tf_sample(tf, (dv - vmin) / rng)
                            cr = cr + (sc[0] * sc[3]) * T
                            cg = cg + (sc[1] * sc[3]) * T
                            cb = cb + (sc[2] * sc[3]) * T
                            T = T * (one - sc[3])
                            if T == zero or T < ert:
                                break
                        else:
                            ds.append(dv)
                    p0, p1, p2 = p0 + s0, p1 + s1, p2 + s2
                if ds:
                    if mode in ("mip", "minip"):
                        v, keep = (F(-np.inf), np.fmax) if mode == "mip" else (F(np.inf), np.fmin)
                        for dv in ds:
                            v = keep(v, dv)
                    else:
                        v = _sum(ds, order) / F(len(ds))
                    sc = pyoracle.tf_sample(tf, (v - vmin) / rng)
                    cr = (sc[0] * sc[3]) * one
                    cg = (sc[1] * sc[3]) * one
                    cb = (sc[2] * sc[3]) * one
                    T = one * (one - sc[3])
                A = one - T
                omA = one - A
                out[py, px] = (cr * A + clear[0] * omA, cg * A + clear[1] * omA,
                               cb * A + clear[2] * omA, A * A + clear[3] * omA)
    return out, dict(rays=rays, steps=steps, samples=samples, const_samples=const_samples)


def _sum(ds, order):
    acc = F(0.0)
    if order == "batch4":
        for b in range(0, len(ds), 4):
            part = F(0.0)
            for dv in ds[b:b + 4]:
                part = part + dv
            acc = acc + part
        return acc
    for dv in (reversed(ds) if order == "reverse" else ds):
        acc = acc + dv
    return acc


_cache = {}


def cached(key, make_scene, mode):
    """One reference frame per key and mode for the whole test session (never modified by the
    tests)."""
    k = (key, mode)
    if k not in _cache:
        img, st = render(make_scene(), mode)
        img.setflags(write=False)
        _cache[k] = (img, st)
    return _cache[k]
