"""Reference for include/vr/vr_morph.h: the exact squared Euclidean distance transform of a mask as
the separable min-plus transform in int64 numpy, and dilation, erosion, opening and closing with a
ball as thresholds of it.  Arrays are (bz, by, bx); a voxel is set iff its element is non-zero; only
the voxels of the grid exist."""
import numpy as np

NONE = 0xFFFFFFFF  # VR_EDT_NONE
TO_SET, TO_UNSET = 0, 1
DILATE, ERODE, OPEN, CLOSE = 0, 1, 2, 3
_BIG = 1 << 40  # above every sum of a distance and an offset's square


def _minplus(f, axis):
    """D(i) = min over k of F(k) + (i - k)^2 along `axis`, for every column at once."""
    g = np.moveaxis(f, axis, 0)
    n = g.shape[0]
    flat = np.ascontiguousarray(g.reshape(n, -1))
    cols = np.flatnonzero((flat < _BIG).any(axis=0))  # a column without a finite value keeps none
    if n == 1 or cols.size == 0:
        return f
    sub = flat[:, cols]
    res = sub.copy()
    for d in range(1, n):
        d2 = d * d
        if d2 >= int(res.max()):  # no offset from here on can improve any voxel
            break
        np.minimum(res[d:], sub[:-d] + d2, out=res[d:])
        np.minimum(res[:-d], sub[d:] + d2, out=res[:-d])
    flat[:, cols] = res
    return np.moveaxis(flat.reshape(g.shape), 0, axis)


def edt2(target):
    """uint32 (bz, by, bx): the squared distance of every voxel to the nearest True voxel of
    `target`; NONE everywhere when there is none."""
    f = np.where(np.asarray(target, bool), 0, _BIG).astype(np.int64)
    for axis in (2, 1, 0):
        f = _minplus(f, axis)
    return np.where(f >= _BIG, NONE, f).astype(np.uint32)


def edt(mask, target=TO_SET):
    """(dist2, info) as vr_edt_squared delivers them."""
    m = np.asarray(mask) != 0
    t = m if target == TO_SET else ~m
    d = edt2(t)
    flat = d.reshape(-1)
    finite = flat != NONE
    info = {"voxels": int(d.size), "target_voxels": int(t.sum()), "max_dist2": NONE, "max_index": 0}
    if finite.any():
        mx = int(flat[finite].max())
        info["max_dist2"], info["max_index"] = mx, int(np.flatnonzero(flat == mx)[0])
    return d, info


def dilate(m, r2):
    return edt2(m) <= r2  # (NONE is above every r2)


def erode(m, r2):
    return edt2(~m) > r2  # an unset voxel is at distance 0 from itself; NONE: nothing unset at all


def morph(mask, op, r2):
    """(out uint8 0/1, info) as vr_mask_morph delivers them."""
    m = np.asarray(mask) != 0
    out = {DILATE: lambda: dilate(m, r2), ERODE: lambda: erode(m, r2),
           OPEN: lambda: dilate(erode(m, r2), r2), CLOSE: lambda: erode(dilate(m, r2), r2)}[op]()
    return out.astype(np.uint8), {"voxels": int(m.size), "in_set": int(m.sum()), "out_set": int(out.sum())}


# ---- the definitions, voxel pair by voxel pair (small grids only) ----
def _pair_d2(shape):
    z, y, x = np.indices(shape).reshape(3, -1).astype(np.int64)
    return (x[:, None] - x[None]) ** 2 + (y[:, None] - y[None]) ** 2 + (z[:, None] - z[None]) ** 2


def brute_edt2(target):
    t = np.asarray(target, bool)
    d2 = _pair_d2(t.shape)
    if not t.any():
        return np.full(t.shape, NONE, np.uint32)
    return d2[:, t.reshape(-1)].min(axis=1).astype(np.uint32).reshape(t.shape)


def brute_dilate(m, r2):
    m = np.asarray(m, bool)
    return ((_pair_d2(m.shape) <= r2) & m.reshape(-1)[None]).any(axis=1).reshape(m.shape)


def brute_erode(m, r2):
    m = np.asarray(m, bool)
    return (m.reshape(-1) & ((_pair_d2(m.shape) > r2) | m.reshape(-1)[None]).all(axis=1)).reshape(m.shape)


def ball(r2):
    """The ball's footprint for scipy.ndimage: offsets d with |d|^2 <= r2."""
    r = int(np.floor(np.sqrt(r2)))
    z, y, x = np.mgrid[-r:r + 1, -r:r + 1, -r:r + 1]
    return x * x + y * y + z * z <= r2
