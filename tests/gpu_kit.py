"""What the GPU tests of the analysis families share: the stream fixture, arrays and guarded output
buffers in device memory, and the bracket that holds a context to "as it was".  A plain module,
imported like edge_shapes.py or hit_scenes.py; a family's Source class, its *_pass and *_device
wrappers stay in its own file, built on these."""
import numpy as np
import pytest

import synth
import vr_amd

GUARD = 0x77            # the byte an output buffer is filled with before a call
GUARD32 = 0x77777777    # the same as a 32-bit word, for buffers of words
PAD = 0x55              # the byte around an input array


@pytest.fixture(scope="module")
def stream(gpu):
    """(import it by name into a test module: `from gpu_kit import stream  # noqa: F401`)"""
    import torch
    return torch.cuda.Stream()


def err(rp):
    return vr_amd.lib().vr_last_error(rp._ctx).decode()


def ext_of(a):
    return (a.shape[2], a.shape[1], a.shape[0])


def c_plane(pl):
    """The vr_mpr_plane of one of mpr_ref's planes."""
    return vr_amd.mpr_plane(pl["origin"], pl["du"], pl["dv"], pl["dn"], pl["width"], pl["height"],
                            pl["nsamples"], pl["op"])


def device_bytes(a, odd=False):
    """The array's bytes in device memory (a tensor to keep, the pointer), 16 bytes of 0x55 around
    them; odd: at an odd address (byte masks)."""
    import torch
    b = np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8)
    t = torch.full((b.size + 16,), PAD, dtype=torch.uint8, device="cuda")
    off = 1 if odd else 0
    if b.size:
        t[off:off + b.size] = torch.from_numpy(b.copy()).cuda()
    torch.cuda.synchronize()
    return t, t.data_ptr() + off


def unchanged(keep, a, odd=False):
    """device_bytes' tensor still holds the array, and the padding around it."""
    h = keep.cpu().numpy()
    off = 1 if odd else 0
    return h[off:off + a.nbytes].tobytes() == a.tobytes() and np.all(h[:off] == PAD) and np.all(h[off + a.nbytes:] == PAD)


def guarded(nbytes):
    """A device buffer of nbytes at a 4-byte (not 8-byte) aligned address with guard bytes around it:
    (the tensor, the pointer, its offset in the tensor)."""
    import torch
    t = torch.full((nbytes + 24,), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    off = 4 if t.data_ptr() % 8 == 0 else 8 - t.data_ptr() % 8 + 4
    return t, t.data_ptr() + off, off


def read_guarded(t, off, nbytes):
    h = t.cpu().numpy()
    assert np.all(h[:off] == GUARD) and np.all(h[off + nbytes:] == GUARD)
    return h[off:off + nbytes].tobytes()


def first_difference(got, want, rec):
    """For a failure's message: (records that differ, the first one's index, its words, the wanted
    words) of two byte strings of rec-byte records, None where they are equal."""
    g = np.frombuffer(got, np.uint32).reshape(-1, rec // 4)
    w = np.frombuffer(want, np.uint32).reshape(-1, rec // 4)
    if g.shape != w.shape:
        return g.shape, w.shape
    bad = np.nonzero((g != w).any(1))[0]
    return (int(bad.size), int(bad[0]), g[bad[0]].tolist(), w[bad[0]].tolist()) if bad.size else None


class context_untouched:
    """`with context_untouched(rp):` -- the calls inside leave the context as it was.  On entry: one
    OUT_RGBA32F frame, then the memory report and the last kernel name of libvr_amd.so; on exit the
    report and the name are equal and the frame renders again bit for bit.  rebase() re-reads the
    name, for a test that makes a call of libvr_amd.so's own inside the bracket (the report stays
    the entry's)."""

    def __init__(self, rp, cam=None, params=None):
        self.rp = rp
        self.cam = synth.camera("rotA").to_vr_camera() if cam is None else cam
        self.params = vr_amd.default_params(shading=1, skip_empty=1) if params is None else params

    def rebase(self):
        self.last = self.rp.last_kernel_name()

    def __enter__(self):
        self.before = self.rp.render(self.cam, self.params, vr_amd.OUT_RGBA32F)
        self.rep = self.rp.memory_report()
        self.rebase()
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            rp = self.rp
            assert rp.memory_report() == self.rep and rp.last_kernel_name() == self.last
            assert np.array_equal(rp.render(self.cam, self.params, vr_amd.OUT_RGBA32F).view(np.uint32),
                                  self.before.view(np.uint32))
        return False
