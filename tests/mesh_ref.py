"""Reference for the isosurface mesh (include/vr/vr_mesh.h) -- test helper.

A numpy restatement of the header's method section, np.float32 throughout: the node set and the
ring, the cell set, the vertex of an active cell (the twelve edges in the header's order, every
operation one IEEE f32 operation), the quads with their winding, inside_voxels.  Normals go through
tests/iso_ref.py's texel_coord and grad_cell, the gradient the ISO frames are checked with, then
1.0f / sqrtf in two roundings.

The order of vertices and triangles is unspecified by the header; here vertices follow their cells
in z, y, x (x fastest) order and triangles the edge axes x, y, z in turn.  Compare through
mesh_scenes.canonical.  tests/test_mesh_cpu.py pins this reference by properties no implementation
detail enters: closedness, orientation, and the derived bound between its volume and inside_voxels.
"""
import numpy as np

import iso_ref

F = np.float32
VERTEX_DTYPE = np.dtype([("pos", "<f4", 3), ("normal", "<f4", 3)])

# corner pairs (A, B) in the header's order: x, y, z edges
EDGES = [(0, (0, 1)), (0, (2, 3)), (0, (4, 5)), (0, (6, 7)),
         (1, (0, 2)), (1, (1, 3)), (1, (4, 6)), (1, (5, 7)),
         (2, (0, 4)), (2, (1, 5)), (2, (2, 6)), (2, (3, 7))]


class Mesh:
    """verts (VERTEX_DTYPE), tris ((T, 3) uint32), info (the three counts) and, for the property
    tests, active_cells and dims."""

    def __init__(self, verts, tris, info, active_cells, dims):
        self.verts, self.tris, self.info = verts, tris, info
        self.active_cells, self.dims = active_cells, dims
        for a in (verts, tris):
            a.setflags(write=False)


def extract(vol, iso, closed=True, normals=True, box=None):
    """vol: (nz, ny, nx) array of the node values as float32 (what (float)stored gives)."""
    vol = np.ascontiguousarray(vol, dtype=F)
    nz, ny, nx = vol.shape
    dims = (nx, ny, nz)
    lo = tuple(int(v) for v in box[0]) if box is not None else (0, 0, 0)
    hi = tuple(int(v) for v in box[1]) if box is not None else dims
    assert all(0 <= lo[a] < hi[a] <= dims[a] for a in range(3))
    iso = F(iso)
    ring = 1 if closed else 0
    nlo = [lo[a] - ring for a in range(3)]  # the first node per axis
    nn = [hi[a] - lo[a] + 2 * ring for a in range(3)]  # nodes per axis
    f = np.zeros((nn[2], nn[1], nn[0]), F)  # ring nodes: +0.0f
    f[ring:nn[2] - ring, ring:nn[1] - ring, ring:nn[0] - ring] = vol[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
    with np.errstate(all="ignore"):
        inside = f >= iso  # a NaN is never inside
    inside_voxels = int(inside[ring:nn[2] - ring, ring:nn[1] - ring, ring:nn[0] - ring].sum())
    nc = [n - 1 for n in nn]  # cells per axis
    empty = Mesh(np.zeros(0, VERTEX_DTYPE), np.zeros((0, 3), np.uint32),
                 dict(vertices=0, triangles=0, inside_voxels=inside_voxels), 0, dims)
    if min(nc) <= 0:
        return empty

    def corner(arr, i):
        dx, dy, dz = i & 1, (i >> 1) & 1, i >> 2
        return arr[dz:dz + nc[2], dy:dy + nc[1], dx:dx + nc[0]]

    m = np.stack([corner(inside, i) for i in range(8)])
    active = m.any(axis=0) & ~m.all(axis=0)
    cz, cy, cx = np.nonzero(active)  # z, y, x order: x fastest
    nv = cz.size
    if nv == 0:
        return empty
    vid = np.full(active.shape, -1, np.int64)
    vid[cz, cy, cx] = np.arange(nv)
    v = [corner(f, i)[cz, cy, cx] for i in range(8)]
    ins = [m[i][cz, cy, cx] for i in range(8)]
    s = [np.zeros(nv, F) for _ in range(3)]
    n = np.zeros(nv, F)
    one, zero = F(1.0), F(0.0)
    with np.errstate(all="ignore"):
        for axis, (A, B) in EDGES:
            cross = ins[A] != ins[B]
            t = (iso - v[A]) / (v[B] - v[A])
            t = np.where(t >= zero, t, zero).astype(F)  # NaN -> 0
            t = np.where(t > one, one, t).astype(F)
            p = [np.full(nv, F(A & 1)), np.full(nv, F((A >> 1) & 1)), np.full(nv, F(A >> 2))]
            p[axis] = t
            for a in range(3):
                s[a] = np.where(cross, s[a] + p[a], s[a]).astype(F)
            n = np.where(cross, n + one, n).astype(F)
        cell = [cx + nlo[0], cy + nlo[1], cz + nlo[2]]  # logical cell indices (-1: the ring cell)
        pos = np.empty((nv, 3), F)
        for a in range(3):
            local = s[a] / n
            pos[:, a] = ((cell[a].astype(F) + F(0.5)) + local) / F(dims[a])
    verts = np.zeros(nv, VERTEX_DTYPE)
    verts["pos"] = pos
    if normals:
        verts["normal"] = normals_at(vol, pos)

    tris = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        # P in cell-array coordinates (x, y, z): C2 = P is a cell, and so are P - e_b, P - e_c
        rng = [None, None, None]
        rng[a] = np.arange(0, nc[a])
        rng[b] = np.arange(1, nc[b])
        rng[c] = np.arange(1, nc[c])
        if any(r.size == 0 for r in rng):
            continue
        px, py, pz = np.meshgrid(rng[0], rng[1], rng[2], indexing="ij")
        P = [px.ravel(), py.ravel(), pz.ravel()]
        # the cell's corner 0 is node P, its corner 1 << a node Q
        ip = inside[P[2], P[1], P[0]]
        Q = [P[0] + (a == 0), P[1] + (a == 1), P[2] + (a == 2)]
        iq = inside[Q[2], Q[1], Q[0]]
        sel = ip != iq
        P = [q[sel] for q in P]
        ip = ip[sel]

        def ids(db, dc):
            q = [P[0].copy(), P[1].copy(), P[2].copy()]
            q[b] = q[b] - db
            q[c] = q[c] - dc
            r = vid[q[2], q[1], q[0]]
            assert (r >= 0).all()  # all four cells are active by construction
            return r

        C0, C1, C2, C3 = ids(1, 1), ids(0, 1), ids(0, 0), ids(1, 0)
        t_in = np.stack([C0, C1, C2, C0, C2, C3], axis=1)
        t_out = np.stack([C0, C2, C1, C0, C3, C2], axis=1)
        tris.append(np.where(ip[:, None], t_in, t_out).reshape(-1, 3))
    tris = np.concatenate(tris).astype(np.uint32) if tris else np.zeros((0, 3), np.uint32)
    info = dict(vertices=nv, triangles=int(tris.shape[0]), inside_voxels=inside_voxels)
    return Mesh(verts, tris, info, nv, dims)


def normals_at(vol, pos):
    """The header's normal at each pos: -(w * r), w = g * dims with g iso_ref's gradient."""
    nz, ny, nx = vol.shape
    out = np.zeros((pos.shape[0], 3), F)
    with np.errstate(all="ignore"):
        for q in range(pos.shape[0]):
            i, ax = iso_ref.texel_coord(pos[q, 0], nx)
            j, ay = iso_ref.texel_coord(pos[q, 1], ny)
            k, az = iso_ref.texel_coord(pos[q, 2], nz)
            g = [iso_ref.grad_cell(vol, i, j, k, ax, ay, az, a) for a in range(3)]
            wx, wy, wz = g[0] * F(nx), g[1] * F(ny), g[2] * F(nz)
            g2 = wx * wx + wy * wy + wz * wz
            if g2 > F(0.0):
                r = F(1.0) / np.sqrt(g2)
                out[q] = (-(wx * r), -(wy * r), -(wz * r))
    return out


# ---- properties of a mesh (reference or device) ---------------------------------------------------
def directed_edges(tris):
    """{(u, v): count} over the three directed edges of every triangle."""
    t = np.asarray(tris, np.int64)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    uniq, cnt = np.unique(e, axis=0, return_counts=True)
    return {(int(u), int(v)): int(c) for (u, v), c in zip(uniq, cnt)}


def edge_report(tris):
    """(every directed edge is matched by as many reversed ones, the set of undirected use counts)."""
    d = directed_edges(tris)
    balanced = all(d.get((v, u), 0) == c for (u, v), c in d.items())
    und = {}
    for (u, v), c in d.items():
        k = (min(u, v), max(u, v))
        und[k] = und.get(k, 0) + c
    return balanced, set(und.values())


def euler(nverts_used, tris):
    d = directed_edges(tris)
    e = len({(min(u, v), max(u, v)) for u, v in d})
    return nverts_used - e + len(tris)


def signed_volume(verts, tris, dims):
    """The f64 divergence sum in lattice units (voxels): sum of p0 . (p1 x p2) / 6."""
    p = verts["pos"].astype(np.float64) * np.asarray(dims, np.float64)
    a, b, c = p[tris[:, 0]], p[tris[:, 1]], p[tris[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


_cache = {}


def cached(key, make_volume, iso, closed=True, normals=True, box=None):
    """One reference per key for the whole test session (never modified by the tests)."""
    k = (key, float(iso), bool(closed), bool(normals), box)
    if k not in _cache:
        _cache[k] = extract(make_volume(), iso, closed, normals, box)
    return _cache[k]
