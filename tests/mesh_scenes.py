"""Scenes the CPU and GPU tests of the isosurface mesh share (test_mesh_cpu.py, test_gpu_mesh.py),
and the canonical form meshes are compared in -- test helper.

The order of vertices and triangles is unspecified (vr_mesh.h), so two meshes are compared as
  * the sorted list of triangles, each as its three vertex RECORDS' bytes (24 bytes a vertex),
    rotated to start at its smallest record, which keeps the winding;
  * the vertex count and the sorted multiset of all vertex records.
"""
import numpy as np

import mesh_ref

F = np.float32


def ball(dims, centre, radius, offset=0.0):
    """(nz, ny, nx) f32: radius - distance from `centre` (in voxels, x y z) + offset."""
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    d = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)
    return (radius - d).astype(F) + F(offset)


DIMS = (19, 17, 21)  # padded index = logical + 2: cells -1 .. 18 span three 8-cell bricks in x
CENTRE = (8.3, 7.6, 10.2)
BOX = ((3, 2, 5), (15, 13, 18))  # interior caps, not brick-aligned


def small_ball():
    return ball(DIMS, CENTRE, 6.0)


def big_ball():
    """Larger than the volume: every face of the cube cuts it (caps, or the open mesh's rim)."""
    return ball(DIMS, CENTRE, 12.0, 20.0)


def noise():
    """12 x 9 x 10 uniform noise: every corner configuration, non-manifold edges."""
    return np.ascontiguousarray(np.random.default_rng(1).random((12, 9, 10), dtype=F).transpose(2, 1, 0))


def integers():
    """An integer scene every storage type holds: a ball of values 0 .. 100 in 19 x 17 x 21."""
    v = np.clip(np.rint(ball(DIMS, CENTRE, 6.0) * F(12.0) + F(40.0)), 0, 100)
    return v.astype(F)


def specials():
    """f32 with NaN and +-inf voxels sprinkled over the small ball."""
    v = small_ball().copy()
    rng = np.random.default_rng(5)
    flat = v.reshape(-1)
    idx = rng.choice(flat.size, 60, replace=False)
    flat[idx[:20]] = np.nan
    flat[idx[20:40]] = np.inf
    flat[idx[40:]] = -np.inf
    return v


def long_thin():
    """24 x 24 x 3000 u8: more bricks (4 x 4 x 376 of 7 x 8 x 8 cells) than a classify launch has
    workgroups and than one workgroup of the scan covers.  A wavy tube along z."""
    nx, ny, nz = 24, 24, 3000
    z = np.arange(nz, dtype=np.float64)[:, None, None]
    y = np.arange(ny, dtype=np.float64)[None, :, None]
    x = np.arange(nx, dtype=np.float64)[None, None, :]
    cx, cy = 11.5 + 5.0 * np.sin(z / 37.0), 11.5 + 5.0 * np.cos(z / 23.0)
    r = 4.0 + 1.5 * np.sin(z / 11.0)
    d = np.sqrt((x - cx) ** 2 + (y - cy) ** 2)
    return np.clip(np.rint(128.0 + 20.0 * (r - d)), 0, 255).astype(np.uint8)


# name -> (volume maker, iso): the f32 scenes of the parity tests
SCENES = {
    "ball": (small_ball, 0.25),
    "bigball": (big_ball, 20.25),
    "noise": (noise, 0.5),
}
# (scene, closed, box) and the reference's pinned (vertices, triangles, inside_voxels)
CASES = {
    ("ball", True, None): (622, 1240, 792),
    ("ball", False, None): (622, 1240, 792),
    ("bigball", True, None): (2072, 4140, 5593),
    ("bigball", False, None): (840, 1346, 5593),
    ("bigball", True, BOX): (864, 1724, 1716),
    ("bigball", False, BOX): (0, 0, 1716),  # the box lies inside the ball: no crossing, no rim
    ("noise", True, None): (1350, 3572, 527),
    ("noise", False, None): (782, 1938, 527),
}


def reference(name, closed=True, normals=True, box=None):
    make, iso = SCENES[name]
    return mesh_ref.cached(name, make, iso, closed, normals, box)


def records(verts):
    """Vertex records as (N, 6) uint32 words."""
    v = np.ascontiguousarray(verts)
    assert v.dtype.itemsize == 24
    return v.view(np.uint32).reshape(-1, 6)


def canonical(verts, tris):
    """(sorted triangles as byte strings of 72 bytes, sorted vertex records as byte strings)."""
    w = records(verts)
    rec = [w[i].tobytes() for i in range(w.shape[0])]
    out = []
    for a, b, c in np.asarray(tris, np.int64).tolist():
        r = (rec[a], rec[b], rec[c])
        k = r.index(min(r))
        out.append(r[k] + r[(k + 1) % 3] + r[(k + 2) % 3])
    return sorted(out), sorted(rec)


def assert_same_mesh(got, want, what=""):
    """got, want: (verts, tris).  Bit for bit in the canonical form."""
    gv, gt = got
    wv, wt = want
    assert len(gv) == len(wv) and len(gt) == len(wt), (what, len(gv), len(wv), len(gt), len(wt))
    gtri, grec = canonical(gv, gt)
    wtri, wrec = canonical(wv, wt)
    assert grec == wrec, (what, "vertex records differ", sum(a != b for a, b in zip(grec, wrec)))
    assert gtri == wtri, (what, "triangles differ", sum(a != b for a, b in zip(gtri, wtri)))
