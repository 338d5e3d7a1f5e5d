"""The frame store (csrc: context and pyramid units): Context, the raw-image upload path and the raw-batch switches."""
import ctypes as C
import numpy as np

from ._abi import HipLibraryError, _Handle, _chk, _f, _i, c_f, load_library


class Context(_Handle):
    """dmvio_hip_ctx: device, stream and the resident image pyramids (frame slots)."""
    _destroy = "dmvio_hip_destroy"

    def __init__(self, w, h, n_slots=16, device=0):
        L = load_library()
        if L.dmvio_hip_device_count() <= 0:
            raise HipLibraryError("no HIP device visible: the dm-vio_amd hot path has no CPU fallback")
        self._create(L, "dmvio_hip_create", device, w, h, n_slots)
        self.w, self.h, self.n_slots = w, h, n_slots
        self.levels = self.L.dmvio_hip_pyr_levels(self.p)

    def set_stream(self, stream_ptr):
        _chk(self.L, self.L.dmvio_hip_set_stream(self.p, C.c_void_p(stream_ptr)), "set_stream")

    def synchronize(self):
        _chk(self.L, self.L.dmvio_hip_synchronize(self.p), "synchronize")

    def frame_upload(self, slot, img):
        img = np.ascontiguousarray(img, dtype=np.float32)
        assert img.size == self.w * self.h
        _chk(self.L, self.L.dmvio_hip_frame_upload(self.p, slot, _f(img)), "frame_upload")

    def frame_from_device(self, slot, dev_ptr):
        _chk(self.L, self.L.dmvio_hip_frame_from_device(self.p, slot, C.c_void_p(dev_ptr)), "frame_from_device")

    def frames_from_device_batch(self, slots, dev_ptr, stride_bytes):
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        _chk(self.L, self.L.dmvio_hip_frames_from_device_batch(self.p, len(slots), _i(slots), C.c_void_p(dev_ptr), stride_bytes), "frames_from_device_batch")

    def frames_attach_device_batch(self, slots, dev_ptr, stride_bytes):
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        _chk(self.L, self.L.dmvio_hip_frames_attach_device_batch(self.p, len(slots), _i(slots), C.c_void_p(dev_ptr), stride_bytes), "frames_attach_device_batch")

    def selftest_divide(self, a, b):
        a = np.ascontiguousarray(a, dtype=np.float32); b = np.ascontiguousarray(b, dtype=np.float32)
        qs = np.zeros_like(a); qi = np.zeros_like(a)
        _chk(self.L, self.L.dmvio_hip_selftest_divide(self.p, a.size, a.ctypes.data, b.ctypes.data, qs.ctypes.data, qi.ctypes.data), "selftest_divide")
        return qs, qi

    def set_deferred_attach(self, on):
        """dmvio_hip_set_deferred_attach: 1 (default) = frames_attach_device_batch leaves the coarser levels to the tracking kernel that first reads a slot (or to the first
        other reader), 0 = the attach builds them itself."""
        _chk(self.L, self.L.dmvio_hip_set_deferred_attach(self.p, 1 if on else 0), "set_deferred_attach")

    def set_build_stream(self, stream_ptr):
        """dmvio_hip_set_build_stream: the batched pyramid builds on a stream of their own (0 / None: the context's stream); the caller orders the streams with events."""
        _chk(self.L, self.L.dmvio_hip_set_build_stream(self.p, C.c_void_p(stream_ptr or 0)), "set_build_stream")

    def frame_is_clean(self, slot):
        return bool(_chk(self.L, self.L.dmvio_hip_frame_is_clean(self.p, int(slot)), "frame_is_clean"))

    def frame_mark_unclean(self, slot):
        _chk(self.L, self.L.dmvio_hip_frame_mark_unclean(self.p, slot), "frame_mark_unclean")

    def frame_download(self, slot, lvl):
        out = np.zeros(((self.h >> lvl), (self.w >> lvl), 3), dtype=np.float32)
        _chk(self.L, self.L.dmvio_hip_frame_download(self.p, slot, lvl, _f(out)), "frame_download")
        return out

    def abs_squared_grad(self, slot, n_levels=3, B=None):
        """FrameHessian::absSquaredGrad[0..n_levels-1] of a resident frame (the pixel selector's input); B = CalibHessian::B (256 floats) or None."""
        outs = [np.zeros(((self.h >> l), (self.w >> l)), dtype=np.float32) for l in range(n_levels)]
        ptrs = (c_f * n_levels)(*[_f(o) for o in outs])
        Bp = None
        if B is not None:
            Bf = np.ascontiguousarray(B, dtype=np.float32)
            if Bf.size != 256:
                raise ValueError("B must hold 256 floats")
            Bp = _f(Bf)
        _chk(self.L, self.L.dmvio_hip_frame_abs_squared_grad(self.p, slot, n_levels, Bp, ptrs), "frame_abs_squared_grad")
        return outs


def set_raw_batch_layout(ctx, tiled):
    """What UndistorterHip.from_raw_device_batch writes as level 0: 8x4 tiles (True) or row-major (False, the default) (dmvio_hip_set_raw_batch_layout)."""
    _chk(ctx.L, ctx.L.dmvio_hip_set_raw_batch_layout(ctx.p, 1 if tiled else 0), "set_raw_batch_layout")


def set_raw_batch_kernel(ctx, variant):
    """Kernel behind UndistorterHip.from_raw_device_batch: 1 = a 4 x 8 pixel block per thread, levels in registers (default where the geometry allows), 0 = the LDS-tile build
    (dmvio_hip_set_raw_batch_kernel)."""
    _chk(ctx.L, ctx.L.dmvio_hip_set_raw_batch_kernel(ctx.p, int(variant)), "set_raw_batch_kernel")


def frame_level0_is_tiled(ctx, slot):
    return bool(_chk(ctx.L, ctx.L.dmvio_hip_frame_level0_is_tiled(ctx.p, int(slot)), "frame_level0_is_tiled"))


class UndistorterHip(_Handle):
    """Raw camera image -> PhotometricUndistorter::processFrame + Undistort::undistort on the device (upload path)."""
    _destroy = "dmvio_hip_undistorter_destroy"

    def __init__(self, ctx, wOrg, hOrg, bits=8, G=None, vignetteMapInv=None, remapX=None, remapY=None):
        self.ctx = ctx
        self._keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (G, vignetteMapInv, remapX, remapY)]
        self._create(ctx.L, "dmvio_hip_undistorter_create", ctx.p, wOrg, hOrg, bits, *[None if a is None else _f(a) for a in self._keep])
        self.dtype = np.uint8 if bits == 8 else np.uint16

    def upload(self, slot, raw, factor=1.0, want_image=True):
        raw = np.ascontiguousarray(raw, dtype=self.dtype)
        out = np.zeros((self.ctx.h, self.ctx.w), np.float32) if want_image else None
        _chk(self.L, self.L.dmvio_hip_frame_upload_raw(self.ctx.p, self.p, slot, raw.ctypes.data, factor, None if out is None else _f(out)), "frame_upload_raw")
        return out

    def from_raw_device_batch(self, slots, raw_dev_ptr, stride_bytes, factor=1.0):
        """B raw images resident in device memory -> undistorted level 0 + pyramids of `slots` in one launch (asynchronous on the ctx stream)."""
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        _chk(self.L, self.L.dmvio_hip_frames_from_raw_device_batch(self.ctx.p, self.p, len(slots), _i(slots), C.c_void_p(raw_dev_ptr), stride_bytes, factor),
             "frames_from_raw_device_batch")
