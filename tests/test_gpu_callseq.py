"""GPU: random sequences of every call of the boundary on one context (state that a call carries
into the next; tests/test_gpu_sequences.py does this for composite frames alone).

tests/callseq.py draws the sequences and computes the references; tests/test_callseq_cpu.py proves
on the CPU that they shrink and grow every scratch block, visit every storage layout with every
call and follow every volume and window change with every call.  Here each seed is replayed on
two contexts that live for the module -- so what one seed leaves behind the next one meets --: a
one-device context, and a vr_create_mask context over device 0.  The device forms
(vr_hit_render_device, vr_mpr_render_device, vr_mesh_extract_device, vr_label_components_device,
vr_region_grow_device) are used on both: their headers let a multi-device context compute on its
lowest device, which is the device the tensors live on.

Every output is compared bit for bit with the reference of the model state, through the
comparisons of the per-feature tests (the mesh in mesh_scenes' canonical form).  Host outputs go
into arrays, device outputs into tensors, filled with a guard word and sized by the REFERENCE's
counts plus slack: a call that needs more than the reference fails with VR_ENOSPC, and one that
writes past its own counts breaks the guard.  Around every analysis call the memory report's
evictions and downgrades stand still, so whatever the report shows the frames alone caused; every
sequence closes with a composite frame that must still equal the oracle.  After each upload the
context reports the volume's dimensions and storage type, and after every mesh, label and hit op
the last kernel is the instantiation of the layout the upload's knobs asked for (plain 8-bit
bricks for u8_layout 0, yz-quads for 1 and for the narrowed floats).

A failure names the seed, the step, the ops so far, the last kernel and the differing words."""
import ctypes as C

import numpy as np
import pytest

import callseq as Q
import hist_ref
import mesh_scenes
import synth
import vr_amd
from gpu_kit import GUARD32, c_plane
from hit_scenes import words

pytestmark = pytest.mark.gpu

SLACK = 64
P = vr_amd.default_params


@pytest.fixture(scope="module", params=[None, 0x1], ids=["device", "mask"])
def rp(request, gpu):
    r = vr_amd.OffscreenPass(64, 48, device_mask=request.param)
    yield r
    r.close()


@pytest.fixture(scope="module")
def streams(gpu):
    import torch
    return [torch.cuda.Stream() for _ in range(4)]


def host_guarded(nwords):
    return np.full(int(nwords) + SLACK, GUARD32, np.uint32)


def dev_guarded(nwords):
    import torch
    return torch.full((int(nwords) + SLACK,), GUARD32, dtype=torch.int32, device="cuda")


def host(t):
    return t.cpu().numpy().view(np.uint32)


def box_req(req, box):
    if box is not None:
        req.use_box = 1
        for a in range(3):
            req.box_min[a], req.box_max[a] = int(box[0][a]), int(box[1][a])
    return req


class Replay:
    def __init__(self, rp, seed, streams):
        self.rp, self.seed, self.streams = rp, seed, streams
        self.L = vr_amd.lib()
        self.log = []
        self.step = -1

    # -- reporting --
    def where(self):
        return (f"seed {self.seed} step {self.step} ({' '.join(self.log)}), "
                f"last kernel {self.rp.last_kernel_name()}")

    def ok(self, cond, what):
        assert cond, f"{self.where()}: {what}"

    def same(self, what, got, want):
        """got, want: arrays of the same bytes; the message counts the differing 32-bit words."""
        g = np.ascontiguousarray(got).reshape(-1).view(np.uint8)
        w = np.ascontiguousarray(want).reshape(-1).view(np.uint8)
        self.ok(g.size == w.size, f"{what}: {g.size} bytes, the reference has {w.size}")
        if g.size % 4 == 0:
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = int((g != w).sum())
        self.ok(bad == 0, f"{what}: {bad} of {g.size} words differ from the reference")

    def guard(self, what, tail):
        bad = int((np.asarray(tail) != GUARD32).sum())
        self.ok(bad == 0, f"{what}: {bad} guard words past the output were written")

    def rc(self, rc, what):
        self.ok(rc == 0, f"{what} failed ({rc}): {self.L.vr_last_error(self.rp._ctx).decode()}")

    # -- state ops --
    def apply(self, op):
        rp, st = self.rp, op["state"]
        if op["op"] == "volume":
            v = Q.volume(op["name"])
            for k, val in v.knobs.items():
                rp.set_knob(k, val)
            rp.volume_dataset_changed(synth.dataset(v.up))
            dims, window, storage = rp.volume_info()
            self.ok((dims, storage) == (v.dims, v.storage), f"volume_info {dims} {storage}")
        elif op["op"] == "window":
            rp.value_range_changed(*st["window"])
        elif op["op"] == "tf":
            rp.transfer_function_changed(Q.TFS[st["tf"]]())
        elif op["op"] == "slice":
            rp.slicing_changed(*st["slice"])
        elif op["op"] == "resize":
            rp.framebuffer_size_changed(*st["size"])
        elif op["op"] == "mode":
            rp.render_mode_changed(Q.MODES[st["mode"]])
        elif op["op"] == "isovalue":
            rp.isovalue_changed(st["iso"])

    # -- frames --
    def frame_want(self, st, spec, ref, p, skip, inflight=1):
        if st["mode"] == "composite":
            return Q.composite_ref(st, spec, skip, "F32H" in self.rp.kernel_name(p), inflight)
        return ref[0]

    def serial_frame(self, st, spec, ref, skip, inflight=1, counts=True):
        rp = self.rp
        cam, p = Q.camera(spec["cam"]), Q.frame_params(spec, skip, inflight)
        img = rp.render(cam, p, vr_amd.OUT_RGBA32F)
        self.same(f"{st['mode']} frame {st['size']}, skip_empty {skip}", img,
                  self.frame_want(st, spec, ref, p, skip, inflight))
        if counts and st["mode"] != "composite":  # range_scenes.check_against's counters
            w, want = rp.count_work(cam, p), ref[1]
            self.ok((w["rays"], w["steps"], w["shaded_samples"]) == (want["rays"], want["steps"], want["shaded_samples"])
                    and w["samples"] + w["skipped_samples"] == want["samples"] and (skip or not w["skipped_samples"]),
                    f"count_work {w}, the reference {want}")
        return img

    def frame(self, op, ref):
        for skip in (0, 1):
            self.serial_frame(op["state"], op, ref, skip)

    # -- the analysis calls, host forms --
    def mpr(self, op, ref):
        cp = c_plane(Q.mpr_plane(op))
        img = self.rp.render_mpr(cp, None, vr_amd.OUT_RGBA32F)
        self.same("mpr image", img, ref[0])
        w, st = self.rp.count_work_mpr(cp), ref[1]
        self.ok(w == dict(rays=st["rays"], steps=st["steps"], samples=st["samples"], shaded_samples=0,
                          skipped_samples=0), f"count_work_mpr {w}, the reference {st}")

    def hist(self, spec, ref):
        want_bins, want = ref
        req = vr_amd.vr_hist_request()
        req.lo, req.hi, req.nbins = spec["lo"], spec["hi"], spec["nbins"]
        box_req(req, spec["box"])
        bins = host_guarded(2 * spec["nbins"])
        info = vr_amd.vr_hist_info()
        self.rc(self.L.vr_histogram(self.rp._ctx, C.byref(req), bins.ctypes.data_as(C.POINTER(C.c_uint64)),
                                    C.byref(info)), "vr_histogram")
        self.same("histogram bins", bins[:2 * spec["nbins"]], want_bins)
        self.guard("histogram", bins[2 * spec["nbins"]:])
        got = {"voxels": info.voxels, "below": info.below, "above": info.above, "nan": info.nan,
               "vmin": np.float32(info.vmin), "vmax": np.float32(info.vmax)}
        self.ok(hist_ref.same_info(got, want), f"histogram info {got}, the reference {want}")

    def same_mesh(self, what, vw, tw, ref):
        nv, nt = ref.info["vertices"], ref.info["triangles"]
        verts = vw[:nv * 6].view(vr_amd.MESH_VERTEX_DTYPE)
        tris = tw[:nt * 3].reshape(-1, 3)
        self.ok(nt == 0 or int(tris.max()) < nv, f"{what}: a triangle names vertex {int(tris.max()) if nt else 0} of {nv}")
        gt, gv = mesh_scenes.canonical(verts, tris)
        wt, wv = mesh_scenes.canonical(ref.verts, ref.tris)
        bad = sum(a != b for a, b in zip(gv, wv)) + sum(a != b for a, b in zip(gt, wt))
        self.ok(bad == 0, f"{what}: {bad} vertex records and triangles differ from the reference (canonical form)")
        self.guard(what + " vertices", vw[nv * 6:])
        self.guard(what + " triangles", tw[nt * 3:])

    def mesh(self, op, ref):
        rp = self.rp
        args = (op["iso"], op["closed"], op["normals"], op["box"])
        got = rp.mesh_count(*args)
        self.ok(got == ref.info, f"mesh_count {got}, the reference {ref.info}")
        nv, nt = ref.info["vertices"], ref.info["triangles"]
        hv, ht = host_guarded(nv * 6), host_guarded(nt * 3)
        info = vr_amd.vr_mesh_info()
        req = vr_amd.mesh_request(*args)
        self.rc(self.L.vr_mesh_extract(rp._ctx, C.byref(req), hv.ctypes.data, nv, ht.ctypes.data, nt, C.byref(info)),
                "vr_mesh_extract")
        self.ok(rp._mesh_info(info) == ref.info, f"mesh info {rp._mesh_info(info)}, the reference {ref.info}")
        self.same_mesh("mesh", hv, ht, ref)

    def same_labels(self, what, lw, cw, info, ref):
        labels, rec, want = ref
        n, nc = want["voxels"], want["components"]
        self.ok(info == want, f"{what} info {info}, the reference {want}")
        self.same(what + " labels", lw[:n], labels)
        self.same(what + " records", cw[:nc * 16], rec)
        self.guard(what + " labels", lw[n:])
        self.guard(what + " records", cw[nc * 16:])

    def same_grow(self, what, mask_words, comp, grown):
        seed, want_mask, want_comp = grown
        n = want_mask.size
        self.ok(comp == want_comp, f"{what} from {seed}: record {comp}, the reference {want_comp}")
        self.same(f"{what} mask from {seed}", mask_words.view(np.uint8)[:n], want_mask)
        self.guard(what + " mask", mask_words.view(np.uint8)[(n + 3) // 4 * 4:].view(np.uint32))
        tail = mask_words.view(np.uint8)[n:(n + 3) // 4 * 4]
        self.ok(bool((tail == 0x77).all()), f"{what}: bytes past the mask were written")

    def label(self, op, ref):
        rp = self.rp
        labelled, inside, outside = ref
        want = labelled[2]
        args = (op["lo"], op["hi"], op["conn"], op["box"])
        got = rp.label_count(*args)
        self.ok(got == want, f"label_count {got}, the reference {want}")
        n, nc = want["voxels"], want["components"]
        hl, hc = host_guarded(n), host_guarded(nc * 16)
        info = vr_amd.vr_label_info()
        req = vr_amd.label_request(*args)
        self.rc(self.L.vr_label_components(rp._ctx, C.byref(req), hl.ctypes.data, n, hc.ctypes.data, nc,
                                           C.byref(info)), "vr_label_components")
        self.same_labels("label", hl, hc, rp._label_info(info), labelled)
        for grown in (inside, outside):
            if grown is None:
                continue
            hm = host_guarded((n + 3) // 4)
            comp = vr_amd.vr_label_component()
            sd = (C.c_uint32 * 3)(*grown[0])
            self.rc(self.L.vr_region_grow(rp._ctx, C.byref(req), sd, hm.ctypes.data, n, C.byref(comp)),
                    "vr_region_grow")
            self.same_grow("region_grow", hm, vr_amd.label_component_dict(comp), grown)

    def same_hits(self, what, got_words, spec, walk):
        x0, y0, rw, rh = spec["rect"]
        want = walk.records[Q.hit_key(spec)][y0:y0 + rh, x0:x0 + rw]
        self.same(what, got_words[:rw * rh * 6], words(want))
        self.guard(what, got_words[rw * rh * 6:])

    def hit(self, op, walk):
        rp = self.rp
        cam, p = Q.camera(op["cam"]), P()
        kind, th, rect = Q.HIT_KINDS[op["hit"]], op["threshold"], op["rect"]
        out = host_guarded(rect[2] * rect[3] * 6)
        req = vr_amd.hit_request(kind, th, rect)
        self.rc(self.L.vr_hit_render(rp._ctx, C.byref(cam), C.byref(p), C.byref(req), out.ctypes.data), "vr_hit_render")
        # (words() makes every NaN value one NaN, as the per-feature test compares them)
        rec = out[:rect[2] * rect[3] * 6].view(vr_amd.HIT_DTYPE).reshape(rect[3], rect[2])
        self.same_hits(f"hit records {op['hit']} {rect}", np.concatenate([words(rec).reshape(-1), out[rec.size * 6:]]),
                       op, walk)
        key = Q.hit_key(op)
        px, py = op["pick"]
        got = rp.pick(cam, p, px, py, kind, th)
        self.same(f"pick {op['hit']} at {op['pick']}", words(np.asarray(got).reshape(1)),
                  words(walk.records[key][py, px].reshape(1)))
        st = rp.hit_count_work(cam, p, kind, th, rect=rect)
        self.ok((st["rays"], st["shaded_samples"], st["skipped_samples"]) ==
                (walk.stats[key]["rays"], walk.stats[key]["shaded_samples"], 0),
                f"hit_count_work {st}, the reference {walk.stats[key]}")

    # -- frames in flight, one device-form analysis call beside them, one synchronize --
    def burst(self, op, ref):
        import torch
        rp, st, a, aref = self.rp, op["state"], op["analysis"], ref["analysis"]
        W, H = st["size"]
        n = len(op["frames"])
        kind = a["kind"]
        if kind == "mesh_device":  # the capacities come from a count made before the burst
            cnt = rp.mesh_count(a["iso"], a["closed"], a["normals"], a["box"])
            self.ok(cnt == aref.info, f"mesh_count {cnt}, the reference {aref.info}")
            tv, tt = dev_guarded(cnt["vertices"] * 6), dev_guarded(cnt["triangles"] * 3)
        elif kind in ("label_device", "region_grow_device"):
            want = aref[0][2]
            nvox, nc = want["voxels"], want["components"]
            tl, tc, tm = dev_guarded(nvox), dev_guarded(nc * 16), dev_guarded((nvox + 3) // 4)
        elif kind == "hit_image_device":
            th = dev_guarded(a["rect"][2] * a["rect"][3] * 6)
        else:
            tp = dev_guarded(a["w"] * a["h"] * 4)
        outs = [dev_guarded(W * H * 4) for _ in range(n)]
        torch.cuda.synchronize()
        frames = []
        for i, spec in enumerate(op["frames"]):
            skip = (i + self.step) & 1
            p = Q.frame_params(spec, skip, n)
            rp.render_device(Q.camera(spec["cam"]), p, outs[i].data_ptr(), vr_amd.OUT_RGBA32F, 16, 0, 1,
                             self.streams[i].cuda_stream)
            frames.append((spec, skip))
        s3 = self.streams[3].cuda_stream
        done = None
        if kind == "hit_image_device":
            rp.hit_image_device(Q.camera(a["cam"]), P(), Q.HIT_KINDS[a["hit"]], th.data_ptr(), a["threshold"],
                                rect=a["rect"], stream=s3)
        elif kind == "render_mpr_device":
            rp.render_mpr_device(c_plane(Q.mpr_plane(a)), None, tp.data_ptr(), vr_amd.OUT_RGBA32F, stream=s3)
        elif kind == "mesh_device":
            done = rp.mesh_device(tv.data_ptr(), cnt["vertices"], tt.data_ptr(), cnt["triangles"], a["iso"],
                                  a["closed"], a["normals"], a["box"], stream=s3)
        elif kind == "label_device":
            done = rp.label_device(tl.data_ptr(), nvox, tc.data_ptr(), nc, a["lo"], a["hi"], a["conn"], a["box"],
                                   stream=s3)
        else:
            grown = aref[1] if aref[1] is not None else aref[2]
            done = rp.region_grow_device(grown[0], tm.data_ptr(), nvox, a["lo"], a["hi"], a["conn"], a["box"],
                                         stream=s3)
        if op["hist"]:  # on the null stream, synchronous, between enqueueing and synchronizing
            self.hist(op["hist"], ref["hist"])
        torch.cuda.synchronize()
        what = f"{kind} beside {n} frames in flight"
        if kind == "hit_image_device":
            hw = host(th)
            rw, rh = a["rect"][2], a["rect"][3]
            rec = hw[:rw * rh * 6].view(vr_amd.HIT_DTYPE).reshape(rh, rw)
            self.same_hits(what, np.concatenate([words(rec).reshape(-1), hw[rw * rh * 6:]]), a, aref)
        elif kind == "render_mpr_device":
            hw = host(tp)
            self.same(what, hw[:a["w"] * a["h"] * 4], aref[0])
            self.guard(what, hw[a["w"] * a["h"] * 4:])
        elif kind == "mesh_device":
            self.ok(done == aref.info, f"{what}: info {done}, the reference {aref.info}")
            self.same_mesh(what, host(tv), host(tt), aref)
        elif kind == "label_device":
            self.same_labels(what, host(tl), host(tc), done, aref[0])
        else:
            self.same_grow(what, host(tm), done, grown)
        for i, (spec, skip) in enumerate(frames):
            hw = host(outs[i])
            self.guard(f"frame {i} of {n} in flight", hw[W * H * 4:])
            serial = self.serial_frame(st, spec, ref["frames"][i], skip, n, counts=False)
            got = hw[:W * H * 4].view(np.float32).reshape(H, W, 4)
            bad = int((got.view(np.uint32) != serial.view(np.uint32)).sum())
            self.ok(bad == 0, f"frame {i} of {n} in flight beside {kind}: {bad} words differ from the serial frame")

    # -- the sequence --
    def run(self):
        rp = self.rp
        ops, refs = Q.sequence(self.seed), Q.cached(self.seed)
        for self.step, (op, ref) in enumerate(zip(ops, refs)):
            self.log.append(Q.describe(op))
            if op["op"] in Q.STATE_OPS:
                self.apply(op)
                continue
            before = rp.memory_report()
            if op["op"] in ("hist",):
                self.hist(op, ref)
            else:
                getattr(self, op["op"])(op, ref)
            if op["op"] in ("mesh", "label", "hit"):
                # the layout the upload's knobs asked for: plain 8-bit bricks, yz-quads, 16-bit, f32
                name, tag = rp.last_kernel_name(), Q.volume(op["state"]["vol"]).tag
                self.ok(f"_kernel<{tag}," in name or f"_kernel<{tag}>" in name,
                        f"{op['state']['vol']} is not stored as {tag}")
            if op["op"] not in ("frame", "burst"):  # the analysis calls evict and downgrade nothing
                after = rp.memory_report()
                keys = ("evictions", "downgrades", "last_downgrade")
                self.ok(all(before[k] == after[k] for k in keys),
                        f"{op['op']} changed the memory report: {before} -> {after}")


@pytest.mark.parametrize("seed", Q.SEEDS)
def test_random_sequence_of_every_call(rp, streams, seed):
    Replay(rp, seed, streams).run()
