"""GPU: random chains of the mask calls on one worn context (state that a call of vr_label.h,
vr_morph.h, vr_maskcc.h, vr_mstat.h or vr_mview.h carries into the next; tests/test_gpu_callseq.py
does this for the calls of libvr_amd.so).

tests/maskseq.py draws the chains and computes the references; tests/test_maskseq_cpu.py proves on
the CPU that they shrink and grow every scratch group, hand every producer family's array to every
consumer family across streams, meet every storage layout and measure kept masks under a new
volume.  Here each seed is replayed on two contexts that live for the module -- so what one seed
leaves behind the next one meets --: a one-device context and a vr_create_mask context over device
0.  The registers of maskseq.REGS are torch tensors allocated once per context and filled with the
guard byte; there are four streams beside the NULL stream.  The test issues no host wait of its own
between ops: the only waits are the ones the calls make ("return when their outputs are complete"),
so a consumer on one stream reads what a producer on another stream has just written.  (An upload
is the host's own copy and waits for itself.)

After every op: the return code is the expected one; the info and the host outputs equal the
reference byte for byte (the two f32 sums of a region record as tests/test_gpu_mstat.py judges
them: mstat_ref.same_records on integer storage, same_but_sums and sum_bounds on f32); EVERY
register the op names, input or output, is read back whole and equals the model's whole buffer --
the output is right, nothing past it or in an input was written, a refused call touched nothing;
vr_memory_report's builds, evictions and downgrades stand still; each family's *_last_kernel_name
changes only when that family ran (a refused call leaves its own family's name too); and on the seeds with an even number timing is enabled and
vr_timing_read reports the intervals the family's header states (0 for a refused call).  At the end
of every seed all registers are read back (a write into a register no op named) and the closing
composite frame equals callseq.composite_ref.

A seed that does not follow the seed before it on its context (a selection with -k) first copies
the model's registers at its start into the tensors (maskseq.replay).

A failure names the seed, the step, the ops so far, every family's last kernel and the count of
differing words.  Wall time on an MI355X: 4.3 s for the first seed of the first context, which draws
every seed's sequence and references (9.7 s on one slower CPU core), 0.01 s for every seed after it;
11 s for the module's 48 cases."""
import numpy as np
import pytest

import callseq as Q
import hist_ref
import maskseq as M
import mstat_ref
import synth
import vr_amd
from gpu_kit import c_plane

pytestmark = pytest.mark.gpu

FAMILIES = ("morph", "maskcc", "mstat", "mview")
REPORT_KEYS = ("builds", "evictions", "downgrades", "last_downgrade")


class Pass(vr_amd.OffscreenPass):
    """The binding with the return code kept instead of raised while `lenient` (the refusals are
    part of the sequences); everything else of the binding is used as it is."""
    lenient = False
    rc = 0

    def _check(self, rc, what):
        if not self.lenient:
            return super()._check(rc, what)
        self.rc = rc


class Context:
    def __init__(self, device_mask):
        import torch
        self.rp = Pass(64, 48, device_mask=device_mask)
        self.rp.transfer_function_changed(Q.TFS["tf1"]())
        self.rp.render_mode_changed(vr_amd.MODE_COMPOSITE)
        self.regs = {r: torch.full((n,), M.GUARD, dtype=torch.uint8, device="cuda") for r, n in M.REGS.items()}
        self.model = M.Model()
        self.next = 0
        torch.cuda.synchronize()

    def at(self, seed):
        """The registers as the model has them at the start of `seed`."""
        import torch
        if self.next != seed:
            self.model = M.replay(seed)
            for r, t in self.regs.items():
                t.copy_(torch.from_numpy(self.model.buf[r]))
            torch.cuda.synchronize()
        self.next = None  # (until the seed has passed: a failed seed leaves the registers anywhere)


@pytest.fixture(scope="module", params=[None, 0x1], ids=["device", "mask"])
def ctx(request, gpu):
    c = Context(request.param)
    yield c
    c.rp.close()


@pytest.fixture(scope="module")
def streams(gpu):
    import torch
    return [torch.cuda.Stream() for _ in range(4)]


class Replay:
    def __init__(self, ctx, seed, streams):
        self.ctx, self.rp, self.seed, self.streams = ctx, ctx.rp, seed, streams
        self.m = ctx.model
        self.log = []
        self.step = -1

    # -- reporting --
    def kernels(self):
        rp = self.rp
        return {"morph": rp.morph_last_kernel_name(), "maskcc": rp.maskcc_last_kernel_name(),
                "mstat": rp.mstat_last_kernel_name(), "mview": rp.mview_last_kernel_name()}

    def where(self):
        return f"seed {self.seed} step {self.step} ({' '.join(self.log)}), last kernels {self.kernels()}"

    def ok(self, cond, what):
        assert cond, f"{self.where()}: {what}"

    def same(self, what, got, want):
        g = np.ascontiguousarray(got).reshape(-1).view(np.uint8)
        w = np.ascontiguousarray(want).reshape(-1).view(np.uint8)
        self.ok(g.size == w.size, f"{what}: {g.size} bytes, the reference has {w.size}")
        if g.size % 4 == 0:
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = int((g != w).sum())
        self.ok(bad == 0, f"{what}: {bad} of {g.size} words differ from the reference")

    # -- plumbing --
    def ptr(self, reg, off=0):
        return self.ctx.regs[reg].data_ptr() + off

    def stream(self, op):
        return self.streams[op["stream"]].cuda_stream if op["stream"] < 4 else 0

    def read(self, reg):
        return self.ctx.regs[reg].cpu().numpy()

    def source(self, op, occ=False):
        return vr_amd.mview_source(op["ext"], self.ptr(op["src"], op["off"]), op["eb"], op["origin"], op["label"],
                                   self.ptr("o") if occ else 0)

    def regions(self, what, got, res):
        """Region records against the reference's: bytes on integer storage, the f32 sums within the
        header's bound."""
        want = np.frombuffer(res["writes"][0][2].tobytes() if res["writes"] else res["host"]["out"].tobytes(),
                             mstat_ref.REGION_DTYPE)
        got = np.frombuffer(np.ascontiguousarray(got).tobytes(), mstat_ref.REGION_DTYPE)
        self.ok(got.size == want.size, f"{what}: {got.size} records, the reference has {want.size}")
        if res["host"]["exact"]:
            return self.ok(mstat_ref.same_records(got, want), f"{what}: the records differ from the reference")
        self.ok(mstat_ref.same_but_sums(got, want), f"{what}: the records differ from the reference beside the sums")
        for i, values in enumerate(res["host"]["values"]):
            b1, b2 = mstat_ref.sum_bounds(values)
            e1, e2 = abs(float(got["sum"][i]) - float(want["sum"][i])), abs(float(got["sum2"][i]) - float(want["sum2"][i]))
            self.ok(e1 <= b1 and e2 <= b2, f"{what}: region {i} sum error {e1} (bound {b1}), sum2 error {e2} (bound {b2})")

    # -- state ops --
    def apply(self, op):
        rp, st = self.rp, op["state"]
        if op["op"] == "volume":
            v = Q.volume(op["name"])
            for k, val in v.knobs.items():
                rp.set_knob(k, val)
            rp.volume_dataset_changed(synth.dataset(v.up))
            dims, _, storage = rp.volume_info()
            self.ok((dims, storage) == (v.dims, v.storage), f"volume_info {dims} {storage}")
        elif op["op"] == "slice":
            rp.slicing_changed(*st["slice"])
        else:
            rp.framebuffer_size_changed(*st["size"])

    def frame(self, op):
        st = M.frame_state(op)
        cam = Q.camera(op["cam"])
        for skip in (0, 1):
            p = Q.frame_params(op, skip)
            img = self.rp.render(cam, p, vr_amd.OUT_RGBA32F)
            self.same(f"closing composite frame {st['size']}, skip_empty {skip}", img,
                      Q.composite_ref(st, op, skip, "F32H" in self.rp.kernel_name(p)))

    # -- the calls: each returns (info or None, host outputs) --
    def call(self, op, res):
        import torch
        rp, k = self.rp, op["op"]
        ext, origin = op["ext"], op["origin"]
        n = M.voxels_of(ext)
        cap = n - 1 if op.get("short") else n
        dev = op["form"] == "device"
        if k == "upload":
            mask = M.upload_mask(op).reshape(-1)
            self.ctx.regs[op["dst"]][1:1 + n] = torch.from_numpy(mask)
            torch.cuda.current_stream().synchronize()  # (the host's own copy, not a call of the library)
            return None, {}
        if k == "grow":
            comp = rp.region_grow_device(op["seed"], self.ptr(op["dst"]), cap, op["lo"], op["hi"], op["conn"], op["box"],
                                         stream=self.stream(op))
            return None, {"comp": comp}
        if k == "label":
            return rp.label_device(self.ptr(op["dst"]), cap, self.ptr("c"), M.CCAP, op["lo"], op["hi"], op["conn"],
                                   op["box"], stream=self.stream(op)), {}
        if k == "window0":
            return rp.mask_window_device(ext, 0, 1, op["lo"], op["hi"], self.ptr(op["dst"]), cap, origin,
                                         stream=self.stream(op)), {}
        src = self.m.source(op).copy() if not dev else None  # the host forms are handed the model's array
        sp = self.ptr(op["src"], op["off"])
        eb = op["eb"]
        if k == "morph":
            if dev:
                return rp.morph_device(ext, op["mop"], op["r2"], sp, eb, self.ptr(op["dst"]), cap, stream=self.stream(op)), {}
            r = rp.morph(src, op["mop"], op["r2"])
            return r["info"], {"out": r["mask"]}
        if k == "edt":
            if dev:
                return rp.distance_transform_device(ext, sp, eb, self.ptr(op["dst"]), cap, op["target"] == 0,
                                                    stream=self.stream(op)), {}
            r = rp.distance_transform(src, op["target"] == 0)
            return r["info"], {"out": r["dist2"]}
        if k == "select":
            if dev:
                return rp.mask_select_device(ext, op["rule"], sp, eb, self.ptr(op["dst"]), cap, op["conn"], op["min_voxels"],
                                             op["seed"], stream=self.stream(op)), {}
            r = rp.mask_select(src, op["rule"], op["conn"], op["min_voxels"], op["seed"])
            return r["info"], {"out": r["mask"]}
        if k == "mask_label":
            if dev:
                return rp.mask_label_device(ext, sp, eb, self.ptr(op["dst"]), cap, self.ptr("c"), M.CCAP, op["conn"],
                                            stream=self.stream(op)), {}
            labels, comps, info = rp.mask_label(src, op["conn"])
            return info, {"out": labels, "records": comps}
        if k == "window":
            if dev:
                return rp.mask_window_device(ext, sp, eb, op["lo"], op["hi"], self.ptr(op["dst"]), cap, origin,
                                             stream=self.stream(op)), {}
            r = rp.mask_window(src, op["lo"], op["hi"], origin)
            return r["info"], {"out": r["mask"]}
        if k == "stats":
            if dev:
                return None, rp.mask_stats_device(ext, sp, eb, origin, op["hist"], stream=self.stream(op))
            return None, rp.mask_stats(src, origin, op["hist"])
        if k == "label_stats":
            nt = op["ntable"]
            if dev:
                return rp.label_stats_device(ext, sp, self.ptr("c"), nt, self.ptr("r", M.R_OFF), nt - 1 if op["short"] else nt,
                                             origin, stream=self.stream(op)), {}
            table = self.m.buf["c"][:64 * nt].copy().view(vr_amd.LABEL_COMPONENT_DTYPE)
            rec, info = rp.label_stats(src, table, origin)
            return info, {"out": rec}
        if k == "occupancy":
            words = M.occupancy_words(ext)
            return rp.mask_occupancy_device(self.source(op), self.ptr("o"), words - 1 if op["short"] else words,
                                            stream=self.stream(op)), {}
        if k in ("hit", "pick"):
            cam, p = Q.camera(op["cam"]), M.params(op, Q.volume(op["state"]["vol"]).dims)
            if k == "pick":
                return None, {"record": rp.mask_pick(cam, p, self.source(op), *op["pick"])}
            npix = op["rect"][2] * op["rect"][3]
            if dev:
                return rp.mask_hit_render_device(cam, p, self.source(op, op["occ"]), self.ptr("i"),
                                                 npix - 1 if op["short"] else npix, op["rect"], stream=self.stream(op)), {}
            rec, info = rp.mask_hit_render(cam, p, src, origin, op["label"], op["rect"])
            return info, {"out": rec}
        if k == "mslice":
            pl = c_plane(Q.mpr_plane(op))
            npix = op["w"] * op["h"]
            if dev:
                return rp.mask_slice_device(pl, self.source(op, op["occ"]), self.ptr("i"), npix - 1 if op["short"] else npix,
                                            stream=self.stream(op)), {}
            out, info = rp.mask_slice(pl, src, origin, op["label"])
            return info, {"out": out}
        raise AssertionError(k)

    def host_outputs(self, op, res, got):
        k, want = op["op"], res["host"]
        what = M.describe(op)
        if k == "stats":
            if res["rc"] != M.OK:
                return self.ok(all(v == 0 for v in got["region"].values()) and
                               ("bins" not in got or not got["bins"].any()), f"{what}: a refused call wrote {got}")
            rec = np.zeros(1, mstat_ref.REGION_DTYPE)
            for name, v in got["region"].items():
                rec[name] = v
            if want["values"] is None:
                self.ok(mstat_ref.same_records(rec, want["region"]), f"{what}: {rec}, the reference {want['region']}")
            else:
                self.ok(mstat_ref.same_but_sums(rec, want["region"]), f"{what}: {rec}, the reference {want['region']}")
                b1, b2 = mstat_ref.sum_bounds(want["values"])
                e1 = abs(float(rec["sum"][0]) - float(want["region"]["sum"]))
                e2 = abs(float(rec["sum2"][0]) - float(want["region"]["sum2"]))
                self.ok(e1 <= b1 and e2 <= b2, f"{what}: sum error {e1} (bound {b1}), sum2 error {e2} (bound {b2})")
            self.ok(("bins" in got) == (want["bins"] is not None), f"{what}: bins without a histogram request")
            if want["bins"] is not None:
                self.same(what + " bins", got["bins"], want["bins"])
                self.ok(hist_ref.same_info(got["hist_info"], want["hist_info"]),
                        f"{what}: hist info {got['hist_info']}, the reference {want['hist_info']}")
            return
        if res["rc"] != M.OK and k != "grow":  # refused: the binding's zeroed host arrays are untouched
            for name, a in got.items():
                self.ok(not np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).any(), f"{what}: a refused call wrote {name}")
            return
        if k == "grow":
            return self.ok(got["comp"] == want["comp"], f"{what}: record {got['comp']}, the reference {want['comp']}")
        if k == "pick":
            return self.same(what + " record", np.asarray(got["record"]).reshape(1), np.asarray(want["record"]).reshape(1))
        if op["form"] == "host":
            if k == "label_stats":
                self.regions(what, got["out"], res)
            else:
                self.same(what + " result", got["out"], want["out"])
            if k == "mask_label":
                self.same(what + " records", got["records"], want["records"])

    # -- the sequence --
    def run(self):
        rp = self.rp
        self.ctx.at(self.seed)
        self.m = self.ctx.model
        timed = self.seed % 2 == 0
        rp.timing_enable(timed)
        ops, refs = M.sequence(self.seed), M.cached(self.seed)
        for self.step, (op, res) in enumerate(zip(ops, refs)):
            self.log.append(M.describe(op))
            if op["op"] in M.STATE_OPS:
                self.apply(op)
                continue
            if op["op"] == "frame":
                self.frame(op)
                continue
            before, names = rp.memory_report(), self.kernels()
            if timed:
                rp.timing_reset()
            rp.lenient, rp.rc = True, M.OK
            try:
                info, got = self.call(op, res)
                rc = rp.rc
            finally:
                rp.lenient = False
            what = M.describe(op)
            self.ok(rc == res["rc"], f"{what} returned {rc} ({vr_amd.lib().vr_last_error(rp._ctx).decode()}), "
                                     f"the reference {res['rc']}")
            if res["info"] is not None:
                self.ok(info == res["info"], f"{what}: info {info}, the reference {res['info']}")
            self.host_outputs(op, res, got)
            # every register the op names, read back whole, against the model's whole buffer
            self.m.apply(res)
            for reg in M.named(op):
                dev = self.read(reg)
                if reg == "r" and op["op"] == "label_stats" and res["rc"] == M.OK:
                    nb = 64 * op["ntable"]
                    self.regions(what, dev[M.R_OFF:M.R_OFF + nb], res)
                    self.m.buf["r"][M.R_OFF:M.R_OFF + nb] = dev[M.R_OFF:M.R_OFF + nb]  # (the sums the device added)
                self.same(f"{what}: register {reg}, whole", dev, self.m.buf[reg])
            fam = M.FAMILY[op["op"]]
            after = self.kernels()
            # (a refused call of the four families launches nothing: its own family's name stands too)
            still = [f for f in FAMILIES if f != fam or res["intervals"] == 0]
            self.ok(all(after[f] == names[f] for f in still),
                    f"{what} changed the last kernel of a family that did not run: {names} -> {after}")
            report = rp.memory_report()
            self.ok(all(before[key] == report[key] for key in REPORT_KEYS),
                    f"{what} changed the memory report: {before} -> {report}")
            if timed and res["intervals"] is not None:
                n = rp.timing_read()[1]
                self.ok(n == res["intervals"], f"{what}: vr_timing_read reports {n} intervals, the header {res['intervals']}")
        for reg in M.REGS:  # a write into a register no op named
            self.same(f"register {reg} at the end of the seed", self.read(reg), self.m.buf[reg])
        self.ctx.next = self.seed + 1


@pytest.mark.parametrize("seed", M.SEEDS)
def test_random_chain_of_the_mask_calls(ctx, streams, seed):
    Replay(ctx, seed, streams).run()
