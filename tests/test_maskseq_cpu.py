"""CPU: the random chains of tests/maskseq.py cover what tests/test_gpu_maskseq.py is for.

A replay that never runs a small grid behind a large one on the same scratch block, never hands an
array from one stream to another, or never measures a kept mask under a new volume tests nothing,
so the coverage conditions are asserted here over the union of the seeds the GPU test runs, in the
order it runs them (its contexts live for the module), with the generator and the references alone.
Also: the model's bytes change only inside an op's declared outputs, and a model that forgot the
last write to an op's source register -- or the last volume op -- has another reference: what makes a
stale device state visible."""
import copy

import numpy as np

import callseq as Q
import maskseq as M

RUN = [(seed, i, op, res) for seed in M.SEEDS for i, (op, res) in enumerate(zip(M.sequence(seed), M.cached(seed)))]
CALLS = [(seed, i, op, res) for seed, i, op, res in RUN if res is not None]
MASK_FAMILIES = ("morph", "maskcc", "mstat", "mview")
# the mstat and mview kinds whose result is a function of the volume (vr_mask_occupancy_device reads the
# array alone: of the volume it takes the dims, to refuse a grid beyond them)
VOLUME_KINDS = tuple(k for k in M.NEEDS_VOLUME if k != "occupancy")


def ran(res):
    """The call launched kernels: VR_OK, or the labellers' VR_ENOSPC for the records alone."""
    return res["intervals"] != 0 and (res["rc"] == M.OK or bool(res["writes"]))


def walk():
    """RUN with the model BEFORE each op, what the model knew before the last write of every
    register (bytes and meaning), and the volume before the last change of volume."""
    m = M.Model()
    undo = {r: (m.buf[r].copy(), dict(m.meta[r])) for r in M.REGS}
    vol, prev_vol = None, None
    for seed, i, op, res in RUN:
        if op["op"] == "volume" and op["name"] != vol:
            vol, prev_vol = op["name"], vol
        yield seed, i, op, res, m, undo, prev_vol
        if res is not None:
            for reg in {w[0] for w in res["writes"]}:
                undo[reg] = (m.buf[reg].copy(), dict(m.meta[reg]))
            m.apply(res)


def test_the_generator_is_a_function_of_the_seed():
    a, b = M.generate(5), M.generate(5)
    assert repr(a[4][0]) == repr(b[4][0]) and a[4][0] is not b[4][0]
    assert repr(a[4][0]) == repr(M.sequence(4))
    for seed in M.SEEDS:
        ops = M.sequence(seed)
        assert [op["op"] for op in ops[:3]] == list(M.STATE_OPS) and ops[3]["op"] in M.PRODUCERS
        assert len(ops) == 4 + M.STEPS + 1 or len(ops) == 4 + M.STEPS + 2  # (a resize in front of a hit)
        assert ops[-1]["op"] == "frame" and ops[-1]["shading"] == 1
        prev = None
        for op in ops:
            assert set(op["state"]) == {"vol", "slice", "size", "epoch"}
            if "stream" in op:  # one of four streams or the NULL stream, never the one before
                assert 0 <= op["stream"] <= 4 and op["stream"] != prev
                prev = op["stream"]


def test_every_ops_registers_exist_and_do_not_overlap():
    for seed, i, op, res in CALLS:
        ins, outs = M.inputs(op), M.outputs(op)
        for reg, off, n in ins + outs:
            assert reg in M.REGS and 0 <= off and off + n <= M.REGS[reg], (seed, i, M.describe(op))
        assert not {r for r, _, _ in ins} & {r for r, _, _ in outs}, (seed, i, M.describe(op))
        for reg, off, n in ins + outs:
            if reg in M.WORD_REGS + ("o", "i"):
                assert off % 4 == 0
        if op["op"] == "upload":
            assert outs[0][1] % 2 == 1  # the odd address
        if op.get("occ"):
            assert op["form"] == "device"


def test_the_models_bytes_change_only_inside_the_declared_outputs():
    changed = 0
    for seed, i, op, res, m, undo, _ in walk():
        if res is None:
            continue
        before = {r: m.buf[r].copy() for r in {w[0] for w in res["writes"]}}
        allowed = {r: np.zeros(M.REGS[r], bool) for r in before}
        for reg, off, n in M.outputs(op):
            if reg in allowed:
                allowed[reg][off:off + n] = True
        assert set(before) <= {r for r, _, _ in M.outputs(op)}, (seed, i, M.describe(op))
        probe = copy.copy(m)
        probe.buf = {r: (b.copy() if r in before else b) for r, b in m.buf.items()}
        probe.meta = dict(m.meta)
        probe.apply(res)
        for r in before:
            diff = probe.buf[r] != before[r]
            changed += int(diff.sum())
            assert not (diff & ~allowed[r]).any(), (seed, i, M.describe(op), r)
        if res["rc"] in (M.EINVAL,) or op.get("short"):
            assert not res["writes"] and not res["meta"], (seed, i, M.describe(op))
    assert changed > 1000000


def rise_and_fall(sizes):
    up = sum(1 for a, b in zip(sizes, sizes[1:]) if b >= 4 * a and a > 0)
    down = sum(1 for a, b in zip(sizes, sizes[1:]) if 4 * b <= a and b > 0)
    return up, down


def test_work_sizes_rise_and_fall_fourfold_on_every_scratch_group():
    """Per group of calls on the same grow-on-demand blocks: how often a call follows one of at least 4x,
    and of at most 1/4, the voxels; and the same for the component count on maskcc_tab_dev and for
    ntable on mstat_aux_dev."""
    # (vr_edt_squared* transforms in the caller's buffer: morph_dist_dev is vr_mask_morph*'s alone, and
    # morph_tmp_dev an opening's or closing's)
    groups = {"morph": lambda op: op["op"] == "morph",
              "morph open and close": lambda op: op["op"] == "morph" and op["mop"] in (2, 3),
              "maskcc label": lambda op: op["op"] in ("mask_label", "select"),
              "maskcc select": lambda op: op["op"] == "select",
              "mstat records": lambda op: op["op"] == "label_stats",
              "mview staging": lambda op: op["op"] in ("hit", "mslice") and op["form"] == "host",
              "label": lambda op: op["op"] in ("grow", "label")}
    report = {}
    for name, member in groups.items():
        sizes = [M.voxels_of(op["ext"]) for _, _, op, res in CALLS if member(op) and ran(res)]
        report[name] = rise_and_fall(sizes) + (len(sizes),)
    comps = [res["info"]["components"] for _, _, op, res in CALLS
             if op["op"] in ("mask_label", "select") and ran(res) and res["info"]["components"]]
    report["maskcc_tab_dev components"] = rise_and_fall(comps) + (len(comps),)
    ntab = [op["ntable"] for _, _, op, res in CALLS if op["op"] == "label_stats" and ran(res) and op["ntable"]]
    report["mstat_aux_dev ntable"] = rise_and_fall(ntab) + (len(ntab),)
    print("scratch (rises, falls, calls):", report)
    assert all(up >= 5 and down >= 5 for up, down, _ in report.values()), report


def test_every_producer_family_hands_over_to_every_consumer_family_across_streams():
    count = {(p, c): 0 for p in ("label", "morph", "maskcc", "mstat-window") for c in MASK_FAMILIES}
    for (s0, i0, a, ra), (s1, i1, b, rb) in zip(RUN, RUN[1:]):
        if s0 != s1 or ra is None or rb is None or "stream" not in a or "stream" not in b:
            continue
        fam = "mstat-window" if a["op"] in ("window", "window0") else M.FAMILY[a["op"]]
        wrote = [w[0] for w in ra["writes"]]
        if fam in ("label", "morph", "maskcc", "mstat-window") and b.get("src") in wrote and ran(rb):
            assert a["stream"] != b["stream"]
            count[(fam, M.FAMILY[b["op"]])] += 1
    print("hand-overs:", count)
    assert all(n >= 3 for n in count.values()), {k: n for k, n in count.items() if n < 3}


def test_every_layout_meets_every_call_that_reads_the_volume():
    """Per entry point: the device and the host form of the three mstat calls (a NULL-mask window is
    vr_mask_window_device), vr_mask_hit_render_device and vr_mask_slice_device, each on every layout
    at least twice.  (The host forms of the hit image and the slice are printed, not asserted.)"""
    count = {(l, e, f): 0 for l in M.LAYOUTS for e in ("stats", "label_stats", "window", "hit", "mslice")
             for f in ("device", "host")}
    widths, host = {}, {}
    for _, _, op, res in CALLS:
        if not ran(res):
            continue
        e = "window" if op["op"] == "window0" else op["op"]
        if (M.LAYOUT[op["state"]["vol"]], e, op["form"]) in count:
            count[(M.LAYOUT[op["state"]["vol"]], e, op["form"])] += 1
        if op["op"] in M.CONSUMERS:
            widths.setdefault(op["op"], set()).add(op["eb"])
        if op.get("form") == "host":
            host[op["op"]] = host.get(op["op"], 0) + 1
    print("layouts:", count, "host forms:", host)
    asked = {k: n for k, n in count.items() if k[2] == "device" or k[1] in ("stats", "label_stats", "window")}
    print("least per (layout, entry point, form):", min(asked.values()))
    assert all(n >= 2 for n in asked.values()), {k: n for k, n in asked.items() if n < 2}
    assert set(M.LAYOUT[n] for n in Q.NAMES) == set(M.LAYOUTS)
    # (a label array is uint32_t: vr_label_stats* has one width)
    assert all(widths[e] == ({4} if e == "label_stats" else {1, 4}) for e in M.CONSUMERS), widths
    assert all(host.get(e, 0) >= 3 for e in M.HAS_HOST_FORM), host


def test_kept_registers_are_measured_after_a_volume_change_and_capacities_fall_short():
    kept = {(f, ok): 0 for f in ("mstat", "mview") for ok in (True, False)}
    short = {f: 0 for f in MASK_FAMILIES + ("label",)}
    for seed, i, op, res, m, _, _ in walk():
        if res is None:
            continue
        fam = M.FAMILY[op["op"]]
        if op.get("short"):
            assert res["rc"] == M.ENOSPC and res["info"] == M.zero_info(op["op"], M.voxels_of(op["ext"]))
            short[fam] += 1
        if op["op"] in M.NEEDS_VOLUME:
            v = Q.volume(op["state"]["vol"])
            ok = M.fits(op["ext"], op["origin"], v.dims)
            assert (res["rc"] == M.EINVAL) == (not ok), (seed, i, M.describe(op))
            was = m.meta[op["src"]]["vol"]
            # another volume of other dims or another layout (noise and checker share both)
            if Q.volume(was).dims != v.dims or M.LAYOUT[was] != M.LAYOUT[op["state"]["vol"]]:
                kept[(fam, ok)] += 1
    print("kept registers (family, fits):", kept, "VR_ENOSPC:", short)
    assert all(n >= 5 for n in kept.values()) and all(n >= 5 for n in short.values())


def test_the_arrays_are_not_trivial():
    cons = [res for _, _, op, res in CALLS if op["op"] in M.CONSUMERS and ran(res)]
    dull = sum(res["trivial"] for res in cons)
    hits = [res["info"] for _, _, op, res in CALLS if op["op"] == "hit" and ran(res)]
    ten = sum(h["hits"] >= 10 for h in hits)
    misses = sum(h["covered"] - h["hits"] for h in hits)
    print("consumers:", len(cons), "on an empty or full array:", dull, "; hit images:", len(hits),
          "with ten hits or more:", ten, "; misses among covered pixels:", misses)
    assert 5 * dull <= len(cons) and 2 * ten >= len(hits) and misses >= 1
    # the device forms of the hit image and the slice run with the occupancy words and without
    words = {(k, occ): sum(1 for _, _, op, res in CALLS if op["op"] == k and ran(res) and op["form"] == "device" and
                           op["occ"] == occ) for k in ("hit", "mslice") for occ in (True, False)}
    print("with and without occupancy words:", words)
    assert all(n >= 5 for n in words.values()), words


def test_a_model_that_forgot_a_write_or_a_volume_op_has_another_reference():
    """For every consumer kind, its first 5 calls: the reference from a model that forgot the last
    write to the source register differs in at least 4; and for the mstat and mview kinds, so does the
    reference from a model that forgot the last change of volume."""
    seen, differs = {}, {}
    vseen, vdiffers = {}, {}
    for seed, i, op, res, m, undo, prev_vol in walk():
        k = op["op"]
        if k not in M.CONSUMERS or not ran(res):
            continue
        assert M.same_result(M.compute(op, m), res), (seed, i, M.describe(op))  # (compute is pure)
        if seen.get(k, 0) < 5:
            seen[k] = seen.get(k, 0) + 1
            stale = copy.copy(m)
            stale.buf = dict(m.buf, **{op["src"]: undo[op["src"]][0]})
            differs[k] = differs.get(k, 0) + (not M.same_result(M.compute(op, stale), res))
        if k in VOLUME_KINDS and prev_vol is not None and vseen.get(k, 0) < 5:
            vseen[k] = vseen.get(k, 0) + 1
            old = M.compute(op, m, dict(op["state"], vol=prev_vol))
            vdiffers[k] = vdiffers.get(k, 0) + (not M.same_result(old, res))
    print("a forgotten write differs:", differs, "a forgotten volume op differs:", vdiffers)
    assert set(seen) == set(M.CONSUMERS) and all(seen[k] == 5 and differs[k] >= 4 for k in seen), (seen, differs)
    assert set(vseen) == set(VOLUME_KINDS) and all(vseen[k] == 5 and vdiffers[k] >= 4 for k in vseen), (vseen, vdiffers)
