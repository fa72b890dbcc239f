"""Reference for the view of a mask or a label array (include/vr/vr_mview.h) -- test helper.

The header's loops in np.float32, built from the oracle's own pieces: Scene.pixel_ray for the entry
point and direction of every pixel, mpr_ref.positions for the slice's positions, hit_ref.depth_of
for the depth.  The walk is vectorised over the pixels of the image (one pass of the loop per step
k, every live ray at once), so there is no ctypes call per sample; the occupancy comes from a padded
reshape and `any`.

tests/test_mview_cpu.py pins it independently: an all-set mask against hit_ref's ENTRY records, an
all-zero one against its MAX counters, closed-form normals, and the occupancy against a
voxel-by-voxel loop.
"""
import numpy as np

import hit_ref
import mpr_ref

F = np.float32
HIT_DTYPE = np.dtype([("pos", "<f4", 3), ("depth", "<f4"), ("element", "<u4"), ("step", "<u4"),
                      ("index", "<u4"), ("normal", "i1", 3), ("reserved", "u1")])
MISS = 0xFFFFFFFF
CELL = 8
OFFSETS = [(ox, oy, oz) for oz in (-1, 0, 1) for oy in (-1, 0, 1) for ox in (-1, 0, 1) if (ox, oy, oz) != (0, 0, 0)]


def miss_records(shape):
    r = np.zeros(shape, HIT_DTYPE)
    r["depth"] = np.inf
    r["step"] = MISS
    r["index"] = MISS
    return r


def match(e, label=None):
    e = np.asarray(e)
    return e != 0 if label is None else e == np.uint32(label)


def voxel_of(p, dims):
    """vr_mview.h: t = p * (float)dims, one f32 multiply; truncated; clamped to dims - 1.  p (..., 3)
    f32 in [0, 1], dims (nx, ny, nz).  Returns (v (..., 3) int64, clamped (...) bool)."""
    t = np.asarray(p, F) * np.asarray(dims, F)
    v = t.astype(np.int64)
    top = np.asarray(dims, np.int64) - 1
    return np.minimum(v, top), (v > top).any(-1)


def element_at(array, origin, v):
    """The (bz, by, bx) array's element at volume voxel v (..., 3) = (x, y, z), widened to uint32; 0
    outside the grid.  Returns (e, inside, box-linear index)."""
    bz, by, bx = array.shape
    g = np.asarray(v, np.int64) - np.asarray(origin, np.int64)
    inside = ((g >= 0) & (g < np.array([bx, by, bz]))).all(-1)
    gs = np.where(inside[..., None], g, 0)
    e = np.where(inside, array[gs[..., 2], gs[..., 1], gs[..., 0]].astype(np.uint32), np.uint32(0))
    return e, inside, (gs[..., 0] + bx * (gs[..., 1] + by * gs[..., 2])).astype(np.uint32)


def occupancy(array, label=None):
    """(words uint32, info dict, cells (cz, cy, cx) bool) of a (bz, by, bx) array."""
    m = match(array, label)
    bz, by, bx = m.shape
    c = [-(-n // CELL) for n in (bz, by, bx)]
    pad = np.zeros([n * CELL for n in c], bool)
    pad[:bz, :by, :bx] = m
    cells = pad.reshape(c[0], CELL, c[1], CELL, c[2], CELL).any(axis=(1, 3, 5))
    flat = cells.reshape(-1)  # (ck, cj, ci) in C order: m = ci + c0 * (cj + c1 * ck)
    nwords = -(-flat.size // 32)
    bits = np.zeros(nwords * 32, np.uint64)
    bits[:flat.size] = flat
    words = (bits.reshape(nwords, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
    info = dict(voxels=int(m.size), cells=int(flat.size), cells_set=int(flat.sum()), matching=int(m.sum()))
    return words, info, cells


def rays(scene, rect=None):
    """(covered (h, w), tex (h, w, 3), dir (h, w, 3)) of the rectangle (x0, y0, w, h) of the scene's frame."""
    s = scene.s
    x0, y0, w, h = (0, 0, s.width, s.height) if rect is None else (int(v) for v in rect)
    ok = np.zeros((h, w), bool)
    tex = np.zeros((h, w, 3), F)
    d = np.zeros((h, w, 3), F)
    for j in range(h):
        for i in range(w):
            ok[j, i], tex[j, i], _frag, d[j, i] = scene.pixel_ray(x0 + i, y0 + j)
    return ok, tex, d


def normals(array, origin, v, label=None):
    """normal[a] = - sum of o[a] * match(element_at(v + o)) over the 26 neighbours; v (n, 3)."""
    n = np.zeros(v.shape, np.int64)
    for o in OFFSETS:
        e, _, _ = element_at(array, origin, v + np.array(o))
        n -= np.array(o) * match(e, label)[:, None]
    return n.astype(np.int8)


def hit_image(scene, array, origin=(0, 0, 0), label=None, rect=None):
    """(records (h, w) HIT_DTYPE, info dict, trace) of the scene's frame (its camera, step, ray_dist and
    slice box are used) over a (bz, by, bx) array at `origin`.  trace: per pixel, `covered`, `clamped`
    (the hit sample's voxel was clamped) and `near` (samples before the hit in a cell whose
    occupancy bit is set but whose voxel does not match)."""
    s = scene.s
    dims = (s.nx, s.ny, s.nz)
    ok, tex, d = rays(scene, rect)
    h, w = ok.shape
    smin = np.array([s.smin[a] for a in range(3)], F)
    smax = np.array([s.smax[a] for a in range(3)], F)
    step = F(s.step)
    with np.errstate(all="ignore"):
        nsteps = int(F(s.ray_dist) / step)
    _, _, cells = occupancy(array, label)
    rec = miss_records((h, w))
    steps = np.zeros((h, w), np.int64)
    samples = np.zeros((h, w), np.int64)
    near = np.zeros((h, w), np.int64)
    clamped = np.zeros((h, w), bool)
    live = ok.copy()
    p = tex.copy()
    sd = d * step  # f32: dir * step, formed once as the kernels' operand
    zero3 = np.zeros(3, F)
    with np.errstate(all="ignore"):
        for k in range(nsteps):
            if not live.any():
                break
            live &= ~((p > F(1.0)).any(-1) | (p < F(0.0)).any(-1))
            steps += live
            slab = live & (p < smax).all(-1) & (p > smin).all(-1)
            samples += slab
            v, cl = voxel_of(np.where(slab[..., None], p, zero3), dims)
            e, inside, idx = element_at(array, origin, v)
            m = slab & inside & match(e, label)
            g = np.where((slab & inside)[..., None], v - np.asarray(origin), 0) // CELL
            near += slab & inside & ~m & cells[g[..., 2], g[..., 1], g[..., 0]]
            rec["pos"][m] = p[m]
            rec["element"][m] = e[m]
            rec["step"][m] = k
            rec["index"][m] = idx[m]
            clamped |= m & cl
            live &= ~m
            p = p + sd
    hit = rec["step"] != MISS
    if hit.any():
        pos = rec["pos"][hit]
        cam = [F(s.cam_pos[a]) for a in range(3)]
        two = np.concatenate([pos, pos[:1]])  # (depth_of takes a lone element for a scalar)
        rec["depth"][hit] = hit_ref.depth_of([two[:, 0], two[:, 1], two[:, 2]], cam)[:-1]
        rec["normal"][hit] = normals(array, origin, voxel_of(pos, dims)[0], label)
    info = dict(voxels=int(array.size), pixels=h * w, covered=int(ok.sum()), hits=int(hit.sum()),
                steps=int(steps.sum()), samples=int(samples.sum()))
    return rec, info, dict(covered=ok, clamped=clamped, near=near)


def slice_image(dims, array, pl, box=mpr_ref.FULL, origin=(0, 0, 0), label=None):
    """((H, W) uint32, info dict) of mpr_ref plane `pl` over a volume of dims (nx, ny, nz)."""
    W, H, ns = pl["width"], pl["height"], pl["nsamples"]
    q = np.empty((H, W, ns, 3), F)
    for py in range(H):
        for px in range(W):
            q[py, px] = mpr_ref.positions(pl, px, py)
    smin, smax = np.asarray(box[0], F), np.asarray(box[1], F)
    out = np.zeros((H, W), np.uint32)
    done = np.zeros((H, W), bool)
    steps = np.zeros((H, W), np.int64)
    samples = np.zeros((H, W), np.int64)
    zero3 = np.zeros(3, F)
    for s in range(ns):
        p = q[:, :, s]
        step = ~done & ~((p > F(1.0)).any(-1) | (p < F(0.0)).any(-1))
        steps += step
        slab = step & (p < smax).all(-1) & (p > smin).all(-1)
        samples += slab
        v, _ = voxel_of(np.where(slab[..., None], p, zero3), dims)
        e, inside, _ = element_at(array, origin, v)
        m = slab & inside & match(e, label)
        out[m] = e[m]
        done |= m
    info = dict(voxels=int(array.size), pixels=W * H, covered=int((steps > 0).sum()), hits=int((out != 0).sum()),
                steps=int(steps.sum()), samples=int(samples.sum()))
    return out, info


_cache = {}


def cached(key, make):
    """One reference per key for the whole test session (never modified by the tests)."""
    if key not in _cache:
        r = make()
        for a in r:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = r
    return _cache[key]
