"""The reference of include/vr/vr_maskcc.h in numpy -- test helper.

Labels and records are tests/label_ref.py's, on `mask != 0`: label_array gives 0 or 1 + the smallest
box-linear index of the voxel's component, table the records in grid indices and the info.  The
selection rules and hole filling follow the header's definitions word for word: a hole is a
component of unset voxels that holds no voxel with an index 0 or ext[a] - 1 along some axis.

Masks are (bz, by, bx) arrays of uint8 or uint32, seeds (i, j, k): the binding's conventions.
"""
import numpy as np

import label_ref

KEEP_LARGEST, KEEP_MIN_VOXELS, KEEP_SEED, FILL_HOLES = 0, 1, 2, 3


def label(mask, connectivity=6):
    """(labels (bz, by, bx) uint32, records, info) as OffscreenPass.mask_label returns them."""
    labels = label_ref.label_array(np.asarray(mask) != 0, connectivity)
    rec, info = label_ref.table(labels)
    return labels, rec, info


def border(shape):
    """The voxels with an index 0 or ext - 1 along some axis."""
    b = np.zeros(shape, bool)
    for a in range(3):
        sl = [slice(None)] * 3
        for at in (0, shape[a] - 1):
            sl[a] = at
            b[tuple(sl)] = True
    return b


def select(mask, rule, connectivity=6, min_voxels=0, seed=(0, 0, 0), labelled=None):
    """(out (bz, by, bx) uint8 of 0/1, info dict) of vr_mask_select.  labelled: label() of the mask
    (of its complement for FILL_HOLES) under `connectivity`, where the caller has it already."""
    m = np.asarray(mask) != 0
    if rule == FILL_HOLES:
        labels, rec, linfo = labelled if labelled is not None else label(~m, connectivity)
        outside = np.unique(labels[border(m.shape) & ~m])  # the labels that reach the border
        holes = np.setdiff1d(rec["label"], outside)
        out = m | np.isin(labels, holes)
        kept = int(holes.size)
    else:
        labels, rec, linfo = labelled if labelled is not None else label(m, connectivity)
        if rule == KEEP_LARGEST:
            keep = np.array([linfo["largest_label"]] if linfo["components"] else [], np.uint32)
        elif rule == KEEP_MIN_VOXELS:
            keep = rec["label"][rec["voxels"] >= min_voxels]
        elif rule == KEEP_SEED:
            lab = int(labels[seed[2], seed[1], seed[0]])
            keep = np.array([lab] if lab else [], np.uint32)
        else:
            raise ValueError(rule)
        out = np.isin(labels, keep) & m
        kept = int(keep.size)
    out = out.astype(np.uint8)
    return out, {"voxels": int(m.size), "in_set": int(m.sum()), "out_set": int(out.sum()),
                 "components": int(linfo["components"]), "kept": kept}


def holes_from_records(rec, shape):
    """The same holes from the records alone: a bounding box that touches no face of the grid."""
    ext = np.array(shape[::-1], np.int64)  # (bx, by, bz)
    inner = np.all(rec["bbox_min"].astype(np.int64) > 0, axis=1) & np.all(rec["bbox_max"].astype(np.int64) < ext, axis=1)
    return rec["label"][inner]
