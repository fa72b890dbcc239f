"""CPU: the random call sequences of tests/callseq.py cover what tests/test_gpu_callseq.py is for.

A random test that happens never to shrink a scratch block tests nothing, so the coverage
conditions are asserted here over the union of the seeds the GPU test runs, in the order it runs
them (its contexts live for the module: "the previous call on that context" crosses seeds), with
the generator and the references alone.  Also: hit_ref.walk's rect parameter, and the proof that a
model which forgot one volume op has another reference for every kind of checking op -- what makes
a stale device state visible."""
import numpy as np
import pytest

import callseq as Q
import hit_scenes
import mesh_scenes
from hit_scenes import KEYS, PARITY, words

ALL = [(seed, i, op) for seed in Q.SEEDS for i, op in enumerate(Q.sequence(seed))]
# hist, mesh, label and region grow: the kinds that make such a call, and every kind that runs on the
# same grow-only scratch blocks (a label and a region-grow call both use label_dev and label_aux_dev;
# a burst's null-stream histogram uses hist_dev like the hist op)
FAMILIES = {"hist": (("hist",), ("hist", "burst_hist")),
            "mesh": (("mesh", "mesh_device"), ("mesh", "mesh_device")),
            "label": (("label", "label_device"), ("label", "label_device", "region_grow_device")),
            "grow": (("label", "region_grow_device"), ("label", "label_device", "region_grow_device"))}


def calls():
    """(seed, step, kind of Q.KINDS, request dict with its state) of every checking call, in run
    order: the checking ops and each burst's analysis call (Q.kinds_of) -- the one meaning of
    "kind" in every condition here."""
    for seed, i, op in ALL:
        for kind, req in Q.kinds_of(op):
            yield seed, i, kind, req


def scratch_calls():
    """calls() and, as "burst_hist", the null-stream histogram of half the bursts: no kind of its
    own, but a call on the histogram's scratch block."""
    for seed, i, op in ALL:
        for kind, req in Q.kinds_of(op):
            yield seed, i, kind, req
        if op["op"] == "burst" and op["hist"]:
            yield seed, i, "burst_hist", dict(op["hist"], state=op["state"])


def test_the_generator_is_a_function_of_the_seed():
    a, b = Q.generate(8), Q.generate(8)
    assert repr(a) == repr(b) and a[7] is not b[7]
    assert repr(a[7]) == repr(Q.sequence(7))
    for seed in Q.SEEDS:
        ops = Q.sequence(seed)
        assert [op["op"] for op in ops[:7]] == list(Q.STATE_OPS)  # the whole model first
        assert len(ops) >= 7 + Q.STEPS + 1
        close = ops[-1]  # after all of it a composite frame
        assert close["op"] == "frame" and close["state"]["mode"] == "composite" and close["shading"] == 1
        for op in ops[7:]:
            assert set(op["state"]) == {"vol", "window", "tf", "slice", "size", "mode", "iso"}


def test_the_size_rules_hold():
    for seed, i, op in ALL:
        st = op["state"]
        ray = st.get("mode") in Q.RAY_MODES
        if op["op"] in ("frame", "burst") and ray:
            assert st["size"] in Q.RAY_SIZES, (seed, i)
        if op["op"] == "hit" or (op["op"] == "burst" and op["analysis"]["kind"] == "hit_image_device"):
            spec = op if op["op"] == "hit" else op["analysis"]
            x0, y0, w, h = spec["rect"]
            W, H = st["size"]
            assert st["size"] in Q.HIT_SIZES and w * h <= 48 and 0 <= x0 and x0 + w <= W and 0 <= y0 and y0 + h <= H
            assert x0 <= spec["pick"][0] < x0 + w and y0 <= spec["pick"][1] < y0 + h
    sizes = {op["state"]["size"] for _, _, op in ALL if op["op"] in ("frame", "burst")}
    assert set(Q.LARGE) <= sizes and set(Q.SMALL) <= sizes


def test_the_pool_is_what_the_sequences_need():
    vox = sorted(Q.volume(n).voxels for n in Q.NAMES)
    assert vox[0] < 2100 and vox[-1] > 120000
    chunks = {(Q.volume(n).voxels + 8191) // 8192 for n in Q.NAMES}  # kLabelChunk
    assert min(chunks) == 1 and max(chunks) == 15
    for n in Q.NAMES:
        v = Q.volume(n)
        assert np.isfinite(v.f32).all() and not v.up.flags.writeable
        assert sum((d + 3) // 8 + 1 >= 3 for d in v.dims) >= 2  # three or more bricks on two axes
    assert {Q.volume(n).up.dtype for n in Q.NAMES} >= {np.dtype(t) for t in (np.float32, np.float64, np.uint8, np.int16)}
    assert Q.volume("g64s").lo < 0


# ---- the coverage conditions ----------------------------------------------------------------------------
def test_every_kind_comes_first_after_a_new_volume_and_after_a_new_window():
    pending = {"volume": set(), "window": set()}
    count = {(k, w): 0 for k in Q.KINDS for w in pending}
    dims = None
    for seed, i, op in ALL:
        if op["op"] == "volume":
            d = Q.volume(op["name"]).dims
            if d != dims:
                pending["volume"] = set(Q.KINDS)
            dims = d
        elif op["op"] == "window":
            pending["window"] = set(Q.KINDS)
        for kind, _ in Q.kinds_of(op):
            for w in pending:
                if kind in pending[w]:
                    pending[w].discard(kind)
                    count[(kind, w)] += 1
    print(count)
    assert all(n >= 5 for n in count.values()), {k: n for k, n in count.items() if n < 5}


def test_work_sizes_rise_and_fall_fourfold_between_neighbouring_calls():
    """Per family: how often a call of its kinds follows a call ON THE SAME SCRATCH BLOCKS, whatever
    its kind, of at least 4x, and of at most 1/4, the voxels."""
    for fam, (kinds, scratch) in FAMILIES.items():
        prev, larger, smaller = None, 0, 0
        for seed, i, kind, req in scratch_calls():
            if kind not in scratch:
                continue
            size = Q.work_size(req)
            if prev is not None and kind in kinds:
                larger += prev >= 4 * size
                smaller += size >= 4 * prev
            prev = size
        print(fam, larger, smaller)
        assert larger >= 5 and smaller >= 5, (fam, larger, smaller)


def test_every_volume_meets_every_kind_twice():
    seen = {(k, n): 0 for k in Q.KINDS for n in Q.NAMES}
    for seed, i, kind, req in calls():
        seen[(kind, req["state"]["vol"])] += 1
    short = {k: n for k, n in seen.items() if n < 2}
    assert not short, short


def test_every_mode_is_rendered_after_every_other():
    pairs, last = set(), None
    for seed, i, op in ALL:
        if op["op"] in ("frame", "burst"):
            m = op["state"]["mode"]
            if last is not None and last != m:
                pairs.add((last, m))
            last = m
    want = {(a, b) for a in Q.MODES for b in Q.MODES if a != b}
    assert pairs == want, want - pairs


# ---- the references alone are not trivial (one case per seed: its references, computed once) -------------
def checked(seed):
    """(where, kind, request, reference) of every call of sequence(seed) that has a reference of its
    own: the checking ops but the bursts, each burst's analysis call, and "burst_frame" for a
    burst's frames."""
    for i, (op, ref) in enumerate(zip(Q.sequence(seed), Q.cached(seed))):
        where = (seed, i, Q.describe(op))
        if op["op"] == "burst":
            yield where, op["analysis"]["kind"], dict(op["analysis"], state=op["state"]), ref["analysis"]
            for spec, r in zip(op["frames"], ref["frames"]):
                yield where, "burst_frame", dict(spec, state=op["state"]), r
        elif op["op"] in Q.CHECK_OPS:
            yield where, op["op"], op, ref


@pytest.mark.parametrize("seed", Q.SEEDS)
def test_the_references_of_a_seed_are_not_trivial(seed):
    for where, kind, spec, r in checked(seed):
        st = spec["state"]
        if kind in ("frame", "burst_frame") and st["mode"] in Q.RAY_MODES:
            assert r[1]["rays"] >= (1 if st["size"] == (1, 1) else 30), where
        if kind in ("mesh", "mesh_device"):
            assert (r.info["vertices"] == 0) if spec["empty"] else (r.info["vertices"] >= 50), (where, r.info)
        if kind in ("hit", "hit_image_device"):
            hits = int(r.hits(Q.hit_key(spec)).sum())
            assert hits >= 10, (where, spec["hit"], spec["threshold"], hits)


def test_over_all_seeds_iso_and_opacity_miss_and_labels_have_components():
    """(The references are cached: after the per-seed cases this costs nothing, alone what they cost.)"""
    misses = {"iso": 0, "opacity": 0}
    comps = []  # (kind, components) of every call on the label scratch, in run order
    for seed in Q.SEEDS:
        for where, kind, spec, r in checked(seed):
            if kind in ("hit", "hit_image_device") and spec["hit"] in misses:
                misses[spec["hit"]] += int(r.covered.sum()) - int(r.hits(Q.hit_key(spec)).sum())
            if kind in ("label", "label_device", "region_grow_device"):
                comps.append((kind, r[0][2]["components"]))
    assert misses["iso"] >= 1 and misses["opacity"] >= 1, misses
    n = [c for _, c in comps]
    assert sum(c >= 2 for c in n) * 2 >= len(n), n
    # the component table grows and shrinks fourfold between a labelling and the call before it on
    # the same scratch
    larger = sum(a >= 4 * max(b, 1) for (_, a), (k, b) in zip(comps, comps[1:]) if k != "region_grow_device")
    smaller = sum(b >= 4 * max(a, 1) for (_, a), (k, b) in zip(comps, comps[1:]) if k != "region_grow_device")
    assert larger >= 5 and smaller >= 5, (larger, smaller, comps)


# ---- hit_ref.walk(rect=) -------------------------------------------------------------------------------------
def test_a_rect_walk_is_that_window_of_the_full_walk():
    volname, camname, box, tfname, w, h = PARITY[0]
    full = hit_scenes.reference(volname, camname, box, tfname, w, h)
    rect = (12, 9, 8, 6)
    x0, y0, rw, rh = rect
    part = Q.hit_ref.walk(hit_scenes.make_scene(volname, camname, box, tfname, w, h),
                          hit_scenes.isovalue(hit_scenes.volume(volname)), hit_scenes.THRESHOLDS, rect=rect)
    win = (slice(y0, y0 + rh), slice(x0, x0 + rw))
    inside = np.zeros((h, w), bool)
    inside[win] = True
    assert np.array_equal(part.covered[win], full.covered[win]) and full.covered[win].sum() >= 40
    assert not part.covered[~inside].any() and not part.cap[~inside].any()
    assert np.array_equal(part.cap[win], full.cap[win])
    for key in KEYS:
        assert np.array_equal(words(part.records[key][win]), words(full.records[key][win])), key
        assert not part.hits(key)[~inside].any()
        assert part.stats[key]["rays"] == int(full.covered[win].sum())
        assert part.stats[key]["shaded_samples"] == int(full.hits(key)[win].sum())


# ---- a model that forgot one volume op ---------------------------------------------------------------------------
def _clip(box, dims):
    if box is None:
        return None
    lo = tuple(min(box[0][a], dims[a] - 1) for a in range(3))
    return lo, tuple(max(min(box[1][a], dims[a]), lo[a] + 1) for a in range(3))


def _same(kind, a, b):
    """Would the GPU test's comparison of this kind pass with b in a's place?"""
    if kind == "frame":
        return a[0].shape == b[0].shape and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    if kind in ("mpr", "render_mpr_device"):
        return np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    if kind == "hist":
        return np.array_equal(a[0], b[0]) and Q.hist_ref.same_info(a[1], b[1])
    if kind in ("mesh", "mesh_device"):
        if a.info != b.info:
            return False
        return mesh_scenes.canonical(a.verts, a.tris) == mesh_scenes.canonical(b.verts, b.tris)
    if kind in ("label", "label_device", "region_grow_device"):
        return a[0][2] == b[0][2] and a[0][0].tobytes() == b[0][0].tobytes()
    if kind in ("hit", "hit_image_device"):
        return all(np.array_equal(words(a.records[k]), words(b.records[k])) for k in a.records)
    raise AssertionError(kind)


STALE_TRIES = 5


def test_a_model_that_forgot_a_volume_op_has_another_reference_for_every_kind():
    """For each kind, its first STALE_TRIES calls whose latest volume op changed the volume, each
    judged against the state that op should have replaced (the old volume and its window): the
    reference differs in most of them, at least 4 of the 5.  Not in all by necessity: a request
    whose window or isovalue comes from the new volume's range can lie outside the old volume's
    values and the new one's alike -- an empty mesh on purpose, a band that holds no voxel of a
    box -- and nothing equals nothing.  One in five is allowed for that: the empty mesh is drawn 6
    times in 100, and no other request is built to be empty.  (Every call of every seed would cost
    the references of all seeds a second time.)"""
    differ = {k: [] for k in Q.KINDS if k != "burst"}  # (a burst is its frames and its analysis call)
    prev_vol = cur_vol = None
    for seed, i, op in ALL:
        if op["op"] == "volume":
            prev_vol, cur_vol = cur_vol, op["name"]
            continue
        if prev_vol is None or prev_vol == cur_vol:
            continue
        old = Q.volume(prev_vol)
        stale = dict(op["state"], vol=prev_vol, window=(float(np.float32(old.lo)), float(np.float32(old.hi))))
        for kind, req in Q.kinds_of(op):
            if kind == "burst" or len(differ[kind]) >= STALE_TRIES:
                continue
            if kind == "frame" and stale["mode"] == "composite":
                a, b = (Q.composite_ref(s, req, 0, False) for s in (op["state"], stale))
                same = a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
            else:
                spec = {k: v for k, v in req.items() if k != "state"}
                if "box" in spec:
                    spec["box"] = _clip(spec["box"], old.dims)
                if kind == "frame":
                    a, b = Q.ray_ref(op["state"], spec), Q.ray_ref(stale, spec)
                else:
                    f = Q.ANALYSIS_RESULT.get(kind) or Q.RESULT[kind]
                    a, b = f(op["state"], req), f(stale, spec)
                same = _same(kind, a, b)
            differ[kind].append(not same)
        if all(len(v) >= STALE_TRIES for v in differ.values()):
            break
    print(differ)
    assert all(len(v) == STALE_TRIES and sum(v) >= STALE_TRIES - 1 for v in differ.values()), differ
