"""What the tests of the four loop-step descriptor calls (obca_pool_loop_advance, obca_fleet_step, obca_fleet_tracks,
obca_pool_tracks) share: the buffers of one descriptor in host memory between guard bands (``DescriptorCase``), the call on the
device on those buffers uploaded between sentinels (``device_descriptor_call``) and the check of a ctypes mirror against the
header (``check_struct_mirror``).  A plain helper module, imported by name."""
import ctypes

import numpy as np

from tests import test_scene_core as tsc

TOL = 1e-9                        # device against host core: tests/test_gpu_scene.py's TOL
PAD = 32                          # sentinel words on either side of every buffer
FILL_X, FILL_I = tsc.FILL_X, tsc.FILL_I


def _np(t):
    return t.cpu().numpy()


def same_words(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class DescriptorCase:
    """the buffers of one descriptor in host memory, every one between guard bands: ``whole`` with the bands, ``a`` without.
    A subclass sets ``dims`` (the int members), ``ego`` and the attributes SCALARS names before it calls this constructor."""
    SCALARS = ()

    def __init__(self, Mirror, shapes, INT):
        self.Mirror, self.INT = Mirror, INT
        self.whole, self.a = {}, {}
        for name, shape in shapes.items():
            dt, fill = (np.int32, FILL_I) if name in INT else (np.float64, FILL_X)
            self.whole[name], self.a[name] = tsc.banded(shape, dt, fill)

    def __getitem__(self, name):
        return self.a[name]

    def absent(self, name):
        """is the pointer member NULL although the case holds a buffer of that name"""
        return False

    def descriptor(self, null=(), **over):
        d = self.Mirror().set(ego=self.ego, **self.dims, **{n: getattr(self, n) for n in self.SCALARS})
        d.set(**{name: None if name in null or self.absent(name) else arr for name, arr in self.a.items()})
        return d.set(**over)

    def snapshot(self):
        return {k: v.copy() for k, v in self.whole.items()}

    def bands_clean(self):
        return all(tsc.band_clean(w, FILL_I if k in self.INT else FILL_X) for k, w in self.whole.items())


def device_descriptor_call(case, fn, ints, read_names, int_names, rc=0, null=(), device=None, stream=None, **over):
    """the library's ``fn(descriptor, *ints, device, stream)`` itself on the buffers of ``case`` uploaded between sentinels:
    returns name -> numpy of every buffer after the call.  The sentinels are checked here; a refused call must leave every
    word as uploaded, and an accepted one every buffer of ``read_names``."""
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import _lib
    bufs, d = {}, case.descriptor(null=null, **over)
    for name, arr in case.a.items():
        is_int = name in int_names
        buf = torch.full((arr.size + 2 * PAD,), FILL_I if is_int else FILL_X, dtype=torch.int32 if is_int else torch.float64,
                         device="cuda")
        buf[PAD:PAD + arr.size] = torch.as_tensor(np.ascontiguousarray(arr).reshape(-1), device="cuda")
        bufs[name] = buf
        if getattr(d, name) is not None:
            setattr(d, name, buf.data_ptr() + PAD * buf.element_size())
    before = {k: v.clone() for k, v in bufs.items()}
    torch.cuda.synchronize()
    got = fn(ctypes.byref(d), *ints, torch.cuda.current_device() if device is None else device,
             _lib.stream_ptr(torch.device("cuda")) if stream is None else ctypes.c_void_p(stream.cuda_stream))
    assert got == rc
    torch.cuda.synchronize()
    out = {}
    for name, buf in bufs.items():
        fill = FILL_I if name in int_names else FILL_X
        assert (buf[:PAD] == fill).all() and (buf[-PAD:] == fill).all(), name
        if rc != 0 or name in read_names:
            assert torch.equal(buf.view(torch.int32), before[name].view(torch.int32)), name
        out[name] = _np(buf[PAD:PAD + case.a[name].size]).reshape(case.a[name].shape)
    return out


def check_struct_mirror(layout_fn, init_fn, Mirror):
    """the ctypes mirror against the header as the host build sees it: sizeof and the offset of every member in declaration
    order (``layout_fn``; None where only the library's init is at hand), and the bytes of a new instance against what
    ``init_fn`` leaves in memory full of 0xff"""
    if layout_fn is not None:
        out = (ctypes.c_longlong * 64)()
        n = layout_fn(out, 64)
        fields = [f[0] for f in Mirror._fields_]
        assert n == 1 + len(fields)
        assert out[0] == ctypes.sizeof(Mirror)
        assert [out[1 + i] for i in range(len(fields))] == [getattr(Mirror, f).offset for f in fields]
    raw = Mirror()
    ctypes.memset(ctypes.byref(raw), 0xff, ctypes.sizeof(raw))
    init_fn(ctypes.byref(raw))
    assert bytes(raw) == bytes(Mirror())
