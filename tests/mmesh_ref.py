"""Reference for the surface of a mask or a label as a mesh (include/vr/vr_mmesh.h) -- test helper.

A numpy restatement of the header, np.float32 throughout and in the header's order of vertices and
triangles, so a device mesh is compared byte for byte: the nodes and the ring, the cell set, local
from the twelve edges (t = 0.5f on every crossing edge), the Jacobi sweeps over the six neighbours
in the header's order with the clamp to the cell, the position, the integer normal with
1.0f / sqrtf in two roundings, the quads with their winding.

tests/test_mmesh_cpu.py pins it by something independent of it: unsmoothed and without normals it
is mesh_ref.extract of the 0/1 indicator at iso 0.5, and closed meshes stay closed and positively
oriented under smoothing.
"""
import numpy as np

F = np.float32
VERTEX_DTYPE = np.dtype([("pos", "<f4", 3), ("normal", "<f4", 3)])
EDGES = [(0, (0, 1)), (0, (2, 3)), (0, (4, 5)), (0, (6, 7)),
         (1, (0, 2)), (1, (1, 3)), (1, (4, 6)), (1, (5, 7)),
         (2, (0, 4)), (2, (1, 5)), (2, (2, 6)), (2, (3, 7))]
# the six neighbours in the header's order, each with the corners of the face the two cells share
NEIGHBOURS = [((-1, 0, 0), (0, 2, 4, 6)), ((1, 0, 0), (1, 3, 5, 7)),
              ((0, -1, 0), (0, 1, 4, 5)), ((0, 1, 0), (2, 3, 6, 7)),
              ((0, 0, -1), (0, 1, 2, 3)), ((0, 0, 1), (4, 5, 6, 7))]


def match(e, label=None):
    e = np.asarray(e)
    return e != 0 if label is None else e == np.uint32(label)


class Mesh:
    """verts (VERTEX_DTYPE), tris ((T, 3) uint32), info (the header's four fields), local ((V, 3) f32
    after the last sweep), clamped (per sweep, the components the clamp changed), dims."""

    def __init__(self, verts, tris, info, local, clamped, dims):
        self.verts, self.tris, self.info = verts, tris, info
        self.local, self.clamped, self.dims = local, clamped, dims
        for a in (verts, tris, local):
            a.setflags(write=False)


def extract(array, dims, origin=(0, 0, 0), label=None, closed=True, normals=True, smooth_iters=0, relax=0.5):
    """array: (bz, by, bx) uint8 or uint32 whose voxel (0, 0, 0) is volume voxel origin = (x, y, z);
    dims: the volume's (nx, ny, nz)."""
    array = np.asarray(array)
    bz, by, bx = array.shape
    ext = (bx, by, bz)
    assert all(origin[a] + ext[a] <= dims[a] for a in range(3))
    ring = 1 if closed else 0
    nn = [ext[a] + 2 * ring for a in range(3)]
    inside = np.zeros((nn[2], nn[1], nn[0]), bool)
    inside[ring:nn[2] - ring, ring:nn[1] - ring, ring:nn[0] - ring] = match(array, label)
    matching = int(inside.sum())
    nc = [n - 1 for n in nn]

    def done(verts, tris, local, clamped):
        info = dict(voxels=bx * by * bz, vertices=len(verts), triangles=len(tris), matching=matching)
        return Mesh(verts, tris, info, local, clamped, tuple(dims))

    nothing = (np.zeros(0, VERTEX_DTYPE), np.zeros((0, 3), np.uint32), np.zeros((0, 3), F), [])
    if min(nc) <= 0:
        return done(*nothing)

    def corner(i):
        dx, dy, dz = i & 1, (i >> 1) & 1, i >> 2
        return inside[dz:dz + nc[2], dy:dy + nc[1], dx:dx + nc[0]]

    m = np.stack([corner(i) for i in range(8)])
    active = m.any(axis=0) & ~m.all(axis=0)
    cz, cy, cx = np.nonzero(active)  # z, y, x order: x fastest -- the header's vertex order
    nv = cz.size
    if nv == 0:
        return done(*nothing)
    vid = np.full(active.shape, -1, np.int64)
    vid[cz, cy, cx] = np.arange(nv)
    ins = [m[i][cz, cy, cx] for i in range(8)]
    cell = [cx, cy, cz]

    # local: vr_mesh.h's arithmetic with t = (0.5f - vA) / (vB - vA) = 0.5f on every crossing edge
    s = [np.zeros(nv, F) for _ in range(3)]
    n = np.zeros(nv, F)
    for axis, (A, B) in EDGES:
        cross = ins[A] != ins[B]
        p = [F(A & 1), F((A >> 1) & 1), F(A >> 2)]
        p[axis] = F(0.5)
        for a in range(3):
            s[a] = np.where(cross, s[a] + p[a], s[a]).astype(F)
        n = np.where(cross, n + F(1.0), n).astype(F)
    local = np.stack([s[a] / n for a in range(3)], axis=1).astype(F)

    # the sweeps
    relax = F(relax)
    clamped = []
    for _ in range(int(smooth_iters)):
        q = np.zeros((nv, 3), F)
        cnt = np.zeros(nv, np.int64)
        for o, face in NEIGHBOURS:
            nb = [cell[a] + o[a] for a in range(3)]
            in_set = np.ones(nv, bool)
            for a in range(3):
                in_set &= (nb[a] >= 0) & (nb[a] < nc[a])
            f = np.stack([ins[i] for i in face])
            counted = in_set & f.any(axis=0) & ~f.all(axis=0)
            k = np.nonzero(counted)[0]
            nvid = vid[nb[2][k], nb[1][k], nb[0][k]]
            assert (nvid >= 0).all()  # both cells are active
            for a in range(3):
                t = (local[nvid, a] + F(o[a])).astype(F)
                q[k, a] = (q[k, a] + t).astype(F)
            cnt[k] += 1
        new = local.copy()
        k = np.nonzero(cnt > 0)[0]
        changed = 0
        for a in range(3):
            mean = (q[k, a] / cnt[k].astype(F)).astype(F)
            d = (mean - local[k, a]).astype(F)
            v = (local[k, a] + (relax * d).astype(F)).astype(F)
            w = np.where(v >= F(0.0), v, F(0.0)).astype(F)
            w = np.where(w > F(1.0), F(1.0), w).astype(F)
            changed += int((w != v).sum())
            new[k, a] = w
        clamped.append(changed)
        local = new

    verts = np.zeros(nv, VERTEX_DTYPE)
    for a in range(3):
        C = (cell[a] + (int(origin[a]) - ring)).astype(np.int64)
        verts["pos"][:, a] = ((C.astype(F) + F(0.5)) + local[:, a]).astype(F) / F(dims[a])
    if normals:
        G = np.zeros((nv, 3), np.int64)
        for i in range(8):
            d = (i & 1, (i >> 1) & 1, i >> 2)
            for a in range(3):
                G[:, a] += (2 * d[a] - 1) * ins[i].astype(np.int64)
        g2 = (G * G).sum(axis=1).astype(F)
        k = g2 > F(0.0)
        r = (F(1.0) / np.sqrt(g2[k])).astype(F)
        nrm = np.zeros((nv, 3), F)
        for a in range(3):
            nrm[k, a] = ((-G[k, a]).astype(F) * r).astype(F)
        verts["normal"] = nrm

    # quads: owner cell C2 = P in cell-linear order, then the edge axis x, y, z
    keys, recs = [], []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        rng = [None, None, None]
        rng[a] = np.arange(0, nc[a])
        rng[b] = np.arange(1, nc[b])
        rng[c] = np.arange(1, nc[c])
        if any(r_.size == 0 for r_ in rng):
            continue
        px, py, pz = np.meshgrid(rng[0], rng[1], rng[2], indexing="ij")
        P = [px.ravel(), py.ravel(), pz.ravel()]
        ip = inside[P[2], P[1], P[0]]  # the cell's corner 0 is node P
        Q = [P[0] + (a == 0), P[1] + (a == 1), P[2] + (a == 2)]
        iq = inside[Q[2], Q[1], Q[0]]
        sel = ip != iq
        P = [v[sel] for v in P]
        ip = ip[sel]

        def ids(db, dc):
            w = [P[0].copy(), P[1].copy(), P[2].copy()]
            w[b] = w[b] - db
            w[c] = w[c] - dc
            r_ = vid[w[2], w[1], w[0]]
            assert (r_ >= 0).all()
            return r_

        C0, C1, C2, C3 = ids(1, 1), ids(0, 1), ids(0, 0), ids(1, 0)
        t_in = np.stack([C0, C1, C2, C0, C2, C3], axis=1)
        t_out = np.stack([C0, C2, C1, C0, C3, C2], axis=1)
        recs.append(np.where(ip[:, None], t_in, t_out))
        keys.append((P[0] + nc[0] * (P[1] + nc[1] * P[2])) * 3 + a)
    if recs:
        order = np.argsort(np.concatenate(keys), kind="stable")
        tris = np.concatenate(recs)[order].reshape(-1, 3).astype(np.uint32)
    else:
        tris = np.zeros((0, 3), np.uint32)
    return done(verts, tris, local, clamped)


_cache = {}


def cached(key, make, **kw):
    """One reference per (key, request) for the whole test session; make() -> (array, dims, origin)."""
    k = (key, tuple(sorted(kw.items())))
    if k not in _cache:
        array, dims, origin = make()
        _cache[k] = extract(array, dims, origin, **kw)
    return _cache[k]
