"""CPU: the conditions that make tests/edge_shapes.py a sweep -- what the GPU tests of
tests/test_gpu_edge_shapes.py rely on, shown on the references alone.

The extents stand on every axis; the references' counts are the pinned ones; components cross the
first seam of every axis long enough to have one, under both brick geometries; a reference that
leaves the seam pass out differs; the meshes are closed; few boxes are empty, and those are named;
every frame scene covers pixels and hits the isosurface."""
import numpy as np
import pytest

import edge_shapes as E
import label_ref
import label_scenes
import mesh_ref


def test_every_extent_stands_on_every_axis():
    for a in range(3):
        assert {d[a] for d in E.VOLUMES} == set(E.EXTENTS), a
    # where the brick count changes: 4 | 5 and 12 | 13 for 8 cells, 3 | 4 and 10 | 11 for 7 (x, plain 8-bit)
    assert [E.bricks_for(n, 8) for n in (4, 5, 12, 13)] == [1, 2, 2, 3]
    assert [E.bricks_for(n, 7) for n in (3, 4, 10, 11)] == [1, 2, 2, 3]
    assert {3, 4, 10, 11} <= {d[0] for d in E.VOLUMES}
    assert E.seams(19, 8) == [6, 14] and E.seams(19, 7) == [5, 12] and E.seams(6, 8) == [] and E.seams(7, 8) == [6]
    assert len(E.VOLUMES) == 19 == len(set(E.VOLUMES))
    assert all(max(d) <= 15 for d in E.VOLUMES)
    for d in E.VOLUMES:
        for name in E.FILLS:
            v = E.fill(d, name)
            assert v.shape == d[::-1] and v.dtype == np.float32
            assert np.array_equal(v, np.rint(v)) and v.min() >= 0 and v.max() <= 100
            for dtype in (np.uint8, np.uint16):  # every storage type holds it
                assert np.array_equal(v.astype(dtype).astype(np.float32), v)


def test_straddling_counts_nothing_in_an_empty_label_array():
    assert label_scenes.straddling(np.zeros((3, 4, 5), np.uint32)) == 0
    lab = np.zeros((1, 1, 9), np.uint32)
    lab[0, 0, 5:8] = 6  # voxels 5, 6, 7: padded 7, 8, 9
    assert label_scenes.straddling(lab) == 1 and label_scenes.straddling(lab, cells=(16, 8, 8)) == 0
    assert E.crossing(lab, 0, 6) == 1 and E.crossing(lab, 0, 5) == 0 and E.crossing(lab, 0, 8) == 0


@pytest.mark.parametrize("dims", E.VOLUMES)
def test_label_references_are_the_pinned_ones(dims):
    for name in E.FILLS:
        for lo, hi, conn in E.label_cases(dims, name):
            ref = E.label_reference(dims, name, lo, hi, conn)
            assert label_scenes.pinned(ref[2]) == E.LABEL_PINS[(dims, name, lo, hi, conn)], (name, lo, hi, conn)
    # the second window's upper bound is a stored value that `<` would leave out
    for name in E.FILLS:
        lo, hi = E.WINDOWS[name][1]
        v = E.fill(dims, name)
        if name == "noise" and v.size >= 500:
            assert (v == hi).any()
    # the checkerboard: every voxel its own component under 6
    for lo, hi in E.WINDOWS["checker"]:
        info = E.label_reference(dims, "checker", lo, hi, 6)[2]
        assert info["components"] == info["in_voxels"]
    # a seed that is not in exists for one of the windows of every fill
    for name in E.FILLS:
        assert any(E.grow_seeds(dims, E.label_reference(dims, name, lo, hi, 6)[0], E.CELLS["b8"])[1] is not None
                   for lo, hi in E.WINDOWS[name]), name


def test_checker_is_one_component_under_26_joined_through_diagonals_only():
    for dims in E.VOLUMES:
        if sorted(dims)[1] < 2:
            continue  # a line: no diagonal neighbour
        lo, hi = E.WINDOWS["checker"][0]
        info = E.label_reference(dims, "checker", lo, hi, 26)[2]
        assert info["components"] == 1 and info["largest_voxels"] == info["in_voxels"], dims


@pytest.mark.parametrize("dims", [d for d in E.VOLUMES if max(d) >= 7])
def test_a_component_crosses_the_first_seam_of_every_long_axis(dims):
    lo, hi = E.WINDOWS["noise"][0]
    labels = E.label_reference(dims, "noise", lo, hi, 6)[0]
    for a in range(3):
        if dims[a] < 7:
            continue
        for geom, cells in E.CELLS.items():
            seam = E.seams(dims[a], cells[a])[0]
            assert E.crossing(labels, a, seam) >= 1, (a, geom, seam)
            # label_scenes.straddling with one brick along the other axes counts the same or more
            one = [4096, 4096, 4096]
            one[a] = cells[a]
            assert label_scenes.straddling(labels, cells=tuple(one)) >= E.crossing(labels, a, seam)


@pytest.mark.parametrize("dims", [d for d in E.VOLUMES if max(d) >= 7])
def test_a_reference_without_the_seam_pass_differs(dims):
    """Each brick labelled on its own: the scenes tell a missing seam pass from the right one."""
    for name in E.FILLS:
        v = E.fill(dims, name)
        lo, hi = E.WINDOWS[name][0]
        conn = 6 if name == "noise" else 26  # (the checkerboard has no pair under 6)
        if name == "checker" and sorted(dims)[1] < 2:
            continue
        want = E.label_reference(dims, name, lo, hi, conn)[0]
        for geom, cells in E.CELLS.items():
            got = E.brickwise_labels(v, lo, hi, conn, cells)
            assert (got != 0).tobytes() == (want != 0).tobytes()
            assert got.tobytes() != want.tobytes(), (name, geom)
    # and with one brick it is the reference itself
    v = E.fill(dims, "noise")
    lo, hi = E.WINDOWS["noise"][0]
    assert np.array_equal(E.brickwise_labels(v, lo, hi, 6, (64, 64, 64)), E.label_reference(dims, "noise", lo, hi, 6)[0])


def test_thick_volumes_have_components_and_an_open_mesh():
    for dims in E.VOLUMES:
        if min(dims) < 2:
            continue
        for lo, hi in E.WINDOWS["noise"]:
            assert E.label_reference(dims, "noise", lo, hi, 6)[2]["components"] >= 2, (dims, lo, hi)
        for iso in E.ISOS:
            assert E.mesh_reference(dims, "noise", iso, False, False).info["vertices"] >= 1, (dims, iso)


@pytest.mark.parametrize("dims", E.VOLUMES)
def test_mesh_references_are_the_pinned_ones_and_closed(dims):
    for name in E.FILLS:
        for iso in E.ISOS:
            for closed in (True, False):
                m = E.mesh_reference(dims, name, iso, closed, False)
                got = (m.info["vertices"], m.info["triangles"], m.info["inside_voxels"])
                assert got == E.MESH_PINS[(dims, name, iso, closed)], (name, iso, closed)
                assert not m.verts["normal"].view(np.uint32).any()
            m = E.mesh_reference(dims, name, iso, True, False)
            assert m.info["triangles"] >= 4 or m.info["inside_voxels"] == 0
            balanced, _ = mesh_ref.edge_report(m.tris)
            assert balanced, (name, iso)
            # an axis of one voxel has no open cell
            if min(dims) == 1:
                assert E.mesh_reference(dims, name, iso, False, False).info["vertices"] == 0


def test_the_reference_without_normals_is_the_one_with_them_blanked():
    dims = (5, 11, 15)
    for closed in (True, False):
        plain = mesh_ref.extract(E.fill(dims, "noise"), 50.5, closed, False, None)
        full = E.mesh_reference(dims, "noise", 50.5, closed, True)
        bare = E.mesh_reference(dims, "noise", 50.5, closed, False)
        assert full.verts["normal"].view(np.uint32).any()
        assert bare.verts.tobytes() == plain.verts.tobytes() and bare.tris.tobytes() == plain.tris.tobytes()
        assert bare.info == plain.info == full.info


def test_boxes_are_the_listed_ones_and_few_are_empty():
    nx, ny, nz = E.BOX_DIMS
    assert E.BOX_DIMS == (19, 17, 21) and len(set(E.BOXES)) == len(E.BOXES)
    for b in E.BOXES:
        assert all(0 <= b[0][a] < b[1][a] <= E.BOX_DIMS[a] for a in range(3)), b
    for want in (((6, 0, 0), (7, 17, 21)), ((5, 0, 0), (6, 17, 21)), ((4, 0, 0), (5, 17, 21)), ((12, 0, 0), (13, 17, 21)),
                 ((0, 14, 0), (19, 15, 21)), ((0, 0, 20), (19, 17, 21)), ((0, 0, 0), (1, 1, 1)), ((18, 16, 20), (19, 17, 21)),
                 ((6, 6, 6), (7, 7, 7)), ((6, 6, 6), (14, 14, 14)), ((5, 5, 5), (7, 7, 7)), ((0, 0, 0), (6, 6, 6)),
                 ((14, 14, 14), (19, 17, 21)), ((0, 0, 0), (19, 17, 21))):
        assert want in E.BOXES, want
    assert sum(1 for b in E.BOXES if all(b[1][a] - b[0][a] == 1 for a in range(3))) == 9
    for layout in E.BOX_LAYOUTS:
        empty = tuple(b for b in E.BOXES if E.box_label_reference(layout, b, 6)[2]["in_voxels"] == 0)
        assert empty == E.EMPTY_BOXES[layout], layout
        assert 10 * len(empty) <= len(E.BOXES)
        for b in E.BOXES:
            for conn in (6, 26):
                ref = E.box_label_reference(layout, b, conn)
                assert label_scenes.pinned(ref[2]) == E.BOX_LABEL_PINS[(layout, b, conn)], (layout, b, conn)
                seed = E.box_seed(b, ref[0])
                assert all(b[0][a] <= seed[a] < b[1][a] for a in range(3))
            for closed in (True, False):
                m = E.box_mesh_reference(layout, b, closed, normals=False)
                got = (m.info["vertices"], m.info["triangles"], m.info["inside_voxels"])
                assert got == E.BOX_MESH_PINS[(layout, b, closed)], (layout, b, closed)
                if closed:
                    assert mesh_ref.edge_report(m.tris)[0], (layout, b)
        # the whole volume as a box is the call without a box
        vol = E.box_volume(layout)
        s = E.box_scale(layout)
        whole = E.box_label_reference(layout, E.WHOLE, 26)
        free = label_ref.label(vol, E.BOX_WINDOW[0] * s, E.BOX_WINDOW[1] * s, 26, None)
        assert whole[0].tobytes() == free[0].tobytes() and whole[1].tobytes() == free[1].tobytes() and whole[2] == free[2]
    # the 8-bit copy is the f32 volume's rint(. x 100): every storage type holds it
    v8 = E.box_volume("plain8")
    assert np.array_equal(v8.astype(np.uint8).astype(np.float32), v8) and not np.array_equal(v8, E.box_volume("f32") * 100)


def test_every_frame_scene_covers_pixels_and_hits_the_isosurface():
    scenes = E.ray_scenes()
    vols = {d for d, _, _ in scenes}
    assert set(E.LINES) | set(E.SHEETS) <= vols and 9 <= len(vols) <= 12
    assert sum(1 for d in vols if {5, 6} & set(d)) >= 2 and sum(1 for d in vols if {13, 14} & set(d)) >= 2
    assert set(E.MPR_VOLUMES) <= vols
    for d in E.SHEETS:  # the view along the sheet's normal, and an edge-on one
        assert len(E.cameras(d)) == 3
    for a in range(3):  # the axis cameras look along their axis
        pos = E.camera("axis%d" % a).get_position()
        assert int(np.argmax(np.abs(pos))) == a and np.abs(np.delete(pos, a)).max() < 1e-5
    for layout in E.RAY_LAYOUTS:
        for d, camname, boxname in scenes:
            box = E.ray_box(d, boxname, layout)
            if boxname == "centres":  # faces on texel centres, an axis of one voxel left whole
                for a in range(3):
                    lo, hi = box[0][a] * d[a] - 0.5, box[1][a] * d[a] - 0.5
                    assert (d[a] == 1 and (box[0][a], box[1][a]) == (0.0, 1.0)) or \
                        (abs(lo - round(lo)) < 1e-5 and abs(hi - (d[a] - 1)) < 1e-5 and lo < hi), (d, box)
            _, st, hit_step, _ = E.iso_reference(d, camname, box, 0)
            assert st["rays"] >= 30 and int((hit_step >= 0).sum()) >= 20, (d, camname, boxname, st)
    for d in E.MPR_VOLUMES:
        names = [n for n, _ in E.mpr_planes(d, E.CELLS["b8"])]
        assert "oblique" in names and "1x1" in names and len(set(names)) == len(names)
