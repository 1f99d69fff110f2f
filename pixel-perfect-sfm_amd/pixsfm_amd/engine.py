"""Thin Python host layer over the C-ABI: context, device arrays, patch arena, BA problem.

Everything numerical happens in libpixsfm_hip.so on the GPU.  numpy is used only to stage
host arrays in and out.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import F16, F32, F64, KPAD, OBS_REC, BaView, InterpCfg, Loss, check

_NP2DT = {np.dtype(np.float16): F16, np.dtype(np.float32): F32, np.dtype(np.float64): F64}


class Context:
    """One HIP device + stream.  `stream` may be a raw hipStream_t handle (int), e.g.
    torch.cuda.current_stream().cuda_stream, so torch events see the kernels."""

    def __init__(self, device=0, stream=None):
        self.lib = _lib.load()
        h = C.c_void_p()
        check(self.lib.pxr_ctx_create(int(device), C.c_void_p(stream or 0), C.byref(h)), "pxr_ctx_create")
        self.handle = h
        self.device = device

    def sync(self):
        check(self.lib.pxr_ctx_sync(self.handle), "pxr_ctx_sync")

    def timer_start(self):
        check(self.lib.pxr_timer_start(self.handle), "pxr_timer_start")

    def timer_stop(self):
        ms = C.c_double()
        check(self.lib.pxr_timer_stop(self.handle, C.byref(ms)), "pxr_timer_stop")
        return ms.value

    def close(self):
        if getattr(self, "handle", None):
            self.lib.pxr_ctx_destroy(self.handle)
            self.handle = None

    # -- multi-GPU ----------------------------------------------------------
    @staticmethod
    def comm_unique_id():
        """128 opaque bytes from rank 0 (ncclGetUniqueId) that every rank passes to comm_init."""
        buf = C.create_string_buffer(_lib.COMM_ID_BYTES)
        check(_lib.load().pxr_comm_unique_id(buf), "pxr_comm_unique_id")
        return bytes(buf.raw)

    def comm_init(self, unique_id, rank, nranks):
        """Collective: creates this context's RCCL communicator (ncclCommInitRank on its device)."""
        assert len(unique_id) == _lib.COMM_ID_BYTES
        check(self.lib.pxr_comm_init(self.handle, C.c_char_p(bytes(unique_id)), int(rank), int(nranks)), "pxr_comm_init")

    def comm_set_rank(self, rank, nranks):
        """Rank / size when the collective is a caller-supplied callback (gloo tests, MPI)."""
        check(self.lib.pxr_comm_set_rank(self.handle, int(rank), int(nranks)), "pxr_comm_set_rank")

    def comm_rank(self):
        r, n = C.c_int(), C.c_int()
        check(self.lib.pxr_comm_rank(self.handle, C.byref(r), C.byref(n)), "pxr_comm_rank")
        return r.value, n.value

    @property
    def deterministic(self):
        """Order-independent accumulation in pxr_ba_solve / pxr_ka_solve: bit-identical results from run to run (direct BA solver
        and KA: for every number of ranks too).  ON by default since round 5 (pxr_set_deterministic; PXR_DETERMINISTIC=0 switches it
        off for every new context)."""
        return bool(self.lib.pxr_get_deterministic(self.handle))

    @deterministic.setter
    def deterministic(self, on):
        check(self.lib.pxr_set_deterministic(self.handle, int(bool(on))), "pxr_set_deterministic")

    @property
    def gram_cache(self):
        """pxr_ba_solve evaluates the residual blocks' records from cached Gram matrices of the 4 x 4 stencils instead of from
        the texels: ~3x less HBM traffic per LM iteration, records differ from pxr_ba_eval's by the rounding of the reference's
        fp32 horizontal pass.  ON by default since round 5 (pxr_set_gram_cache; PXR_GRAM_CACHE=0 switches it off for every new
        context)."""
        return bool(self.lib.pxr_get_gram_cache(self.handle))

    @gram_cache.setter
    def gram_cache(self, on):
        check(self.lib.pxr_set_gram_cache(self.handle, int(bool(on))), "pxr_set_gram_cache")

    def set_iteration_callbacks(self, callbacks):
        """ceres::IterationCallback objects for the BA solves of this context (pxr_set_iteration_callback): each callable gets
        the iteration summary (attributes iteration, step_is_valid, step_is_successful, cost, cost_change, relative_decrease,
        trust_region_radius, step_norm) and returns None / 0 to continue, 1 to abort, 2 to terminate successfully; the largest
        answer wins.  An empty list removes the hook -- and re-raises an exception a callback raised during the solve (which
        was aborted at that iteration)."""
        callbacks = list(callbacks or [])
        if not callbacks:
            check(self.lib.pxr_set_iteration_callback(self.handle, None, None), "pxr_set_iteration_callback")
            self._iter_cb = None
            pending, self._iter_exc = getattr(self, "_iter_exc", None), None
            if pending is not None:          # an exception raised inside a callback aborted the solve: it surfaces here
                raise pending
            return
        self._iter_exc = None

        def hook(summary, _user):
            rc = 0
            try:
                # a copy: the solver's summary lives on its stack, a callback may keep what it is given
                snap = type(summary.contents).from_buffer_copy(summary.contents)
                for cb in callbacks:
                    ans = cb(snap)
                    rc = max(rc, int(getattr(ans, "value", ans) or 0))
            except BaseException as e:       # noqa: BLE001 -- ctypes would print and swallow it; abort the solve instead
                self._iter_exc = e
                return 1
            return rc
        self._iter_cb = _lib.ITERATION_CALLBACK(hook)            # kept alive as long as it is installed
        check(self.lib.pxr_set_iteration_callback(self.handle, C.cast(self._iter_cb, C.c_void_p), None), "pxr_set_iteration_callback")

    def comm_force(self, on=True):
        """Diagnostics: with a ONE-rank communicator the solvers still take their multi-rank branch (pack, ncclAllReduce on the
        context's stream, unpack); results must equal the plain solve bit for bit (pxr_comm_force)."""
        check(self.lib.pxr_comm_force(self.handle, int(bool(on))), "pxr_comm_force")

    def comm_stats(self, reset=False):
        """(ncclAllReduce calls, payload bytes) issued through this context so far."""
        calls, nbytes = C.c_int64(), C.c_int64()
        check(self.lib.pxr_comm_stats(self.handle, C.byref(calls), C.byref(nbytes), int(bool(reset))), "pxr_comm_stats")
        return calls.value, nbytes.value

    def comm_destroy(self):
        check(self.lib.pxr_comm_destroy(self.handle), "pxr_comm_destroy")

    def allreduce_sum(self, array):
        """In-place sum over the ranks of a float64 DeviceArray through the context's communicator."""
        assert array.dtype == np.float64
        check(self.lib.pxr_comm_allreduce_sum(self.handle, array.ptr, array.nbytes // 8), "pxr_comm_allreduce_sum")

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- device arrays ------------------------------------------------------------------
    def empty(self, shape, dtype):
        return DeviceArray(self, shape, dtype)

    def zeros(self, shape, dtype):
        a = DeviceArray(self, shape, dtype)
        check(self.lib.pxr_memset(self.handle, a.ptr, 0, a.nbytes), "pxr_memset")
        return a

    def to_device(self, host, dtype=None):
        host = np.ascontiguousarray(host, dtype=dtype)
        a = DeviceArray(self, host.shape, host.dtype)
        a.upload(host)
        return a


class DeviceArray:
    """A typed HBM buffer owned through pxr_malloc/pxr_free."""

    def __init__(self, ctx, shape, dtype):
        self.ctx = ctx
        self.shape = tuple(int(s) for s in (shape if hasattr(shape, "__len__") else (shape,)))
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        p = C.c_void_p()
        check(ctx.lib.pxr_malloc(ctx.handle, self.nbytes, C.byref(p)), "pxr_malloc")
        self.ptr = p

    def upload(self, host):
        host = np.ascontiguousarray(host, dtype=self.dtype)
        assert host.nbytes == self.nbytes, (host.shape, self.shape)
        check(self.ctx.lib.pxr_memcpy_h2d(self.ctx.handle, self.ptr, host.ctypes.data, self.nbytes), "pxr_memcpy_h2d")

    def download(self):
        out = np.empty(self.shape, dtype=self.dtype)
        check(self.ctx.lib.pxr_memcpy_d2h(self.ctx.handle, out.ctypes.data, self.ptr, self.nbytes), "pxr_memcpy_d2h")
        return out

    def __array__(self, dtype=None, copy=None):
        """np.asarray(device array): a download."""
        a = self.download()
        return a if dtype is None else a.astype(dtype, copy=False)

    def free(self):
        if getattr(self, "ptr", None) and self.ctx.handle:
            self.ctx.lib.pxr_free(self.ctx.handle, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PatchArena:
    """HBM-resident patches (n, H, W, C) channel-fastest + per-patch corner / scale.

    Replaces the FeaturePatch / FeatureMap / FeatureSet / FeatureView containers
    (pixsfm/features/src/featurepatch.h:40-156, featureview.cc:44-55) on the device.
    """

    def __init__(self, ctx, n, H, W, channels, dtype=np.float16, device_ptr=None):
        self.ctx = ctx
        self.n, self.H, self.W, self.C = int(n), int(H), int(W), int(channels)
        self.dtype = np.dtype(dtype)
        h = C.c_void_p()
        check(ctx.lib.pxr_arena_create(ctx.handle, _NP2DT[self.dtype], self.C, self.H, self.W, self.n,
                                       C.c_void_p(device_ptr or 0), C.byref(h)), "pxr_arena_create")
        self.handle = h

    @classmethod
    def from_numpy(cls, ctx, patches, corners, scales=None):
        patches = np.ascontiguousarray(patches)
        n, H, W, ch = patches.shape
        a = cls(ctx, n, H, W, ch, patches.dtype)
        a.upload(0, patches, corners, scales)
        return a

    def upload(self, first, patches=None, corners=None, scales=None):
        count = len(patches) if patches is not None else len(corners)
        if patches is not None:
            patches = np.ascontiguousarray(patches, dtype=self.dtype)
            assert patches.shape[1:] == (self.H, self.W, self.C)
        if corners is not None:
            corners = np.ascontiguousarray(corners, dtype=np.int32).reshape(count, 2)
        if scales is None and corners is not None:
            scales = np.ones((count, 2))
        if scales is not None:
            scales = np.ascontiguousarray(scales, dtype=np.float64).reshape(count, 2)
        check(self.ctx.lib.pxr_arena_upload(
            self.handle, int(first), int(count),
            None if patches is None else patches.ctypes.data,
            None if corners is None else corners.ctypes.data,
            None if scales is None else scales.ctypes.data), "pxr_arena_upload")

    @classmethod
    def from_patch_pointers(cls, ctx, pointers, shape, dtype, corners, scales):
        """An arena filled from SEPARATE host patches (pointers[i]: address of patch i, `shape` = (H, W, C) elements of
        `dtype`): pxr_arena_upload_gather -- all host cores gather into pinned staging buffers, the upload is
        double-buffered; no stacked host copy of the whole set.  The caller keeps the patches alive during the call."""
        pointers = np.ascontiguousarray(pointers, dtype=np.uint64)
        n = len(pointers)
        a = cls(ctx, n, shape[0], shape[1], shape[2], dtype)
        corners = np.ascontiguousarray(corners, dtype=np.int32).reshape(n, 2)
        scales = np.ascontiguousarray(scales, dtype=np.float64).reshape(n, 2)
        check(ctx.lib.pxr_arena_upload_gather(a.handle, 0, n, pointers.ctypes.data, corners.ctypes.data, scales.ctypes.data),
              "pxr_arena_upload_gather")
        return a

    def extract(self, first, fmap, keypoints, image_size, l2_normalize=True):
        """Fill patches [first, first + len(keypoints)) from ONE image's dense feature map that is
        already on the device (FeatureExtractor.tensor_to_fmap sparse branch, extractor.py:152-199,
        without the GPU -> CPU -> GPU round trip).

        fmap: a CUDA/ROCm tensor-like exposing __cuda_array_interface__ (e.g. a contiguous
        torch.cuda tensor) of shape (C, h, w) or (1, C, h, w), float16 or float32.
        keypoints: (n, 2) COLMAP image coordinates (host array or DeviceArray).
        image_size: (width, height) of the image the keypoints live in."""
        cai = fmap.__cuda_array_interface__
        shape = tuple(cai["shape"])
        if len(shape) == 4 and shape[0] == 1:
            shape = shape[1:]
        if len(shape) != 3 or shape[0] != self.C:
            raise ValueError("feature map must be (C=%d, h, w); got %r" % (self.C, tuple(cai["shape"])))
        if cai.get("strides") is not None:
            item = int(cai["typestr"][2:])
            full = tuple(cai["shape"])
            expect = tuple(int(np.prod(full[i + 1:])) * item for i in range(len(full)))
            if tuple(cai["strides"]) != expect:
                raise ValueError("feature map must be contiguous (call .contiguous())")
        src = {"<f2": _lib.F16, "<f4": _lib.F32}.get(cai["typestr"])
        if src is None:
            raise ValueError("feature map dtype %s not supported (float16 / float32)" % cai["typestr"])
        if isinstance(keypoints, DeviceArray):
            d_kp, n = keypoints, keypoints.shape[0]
        else:
            kp = np.ascontiguousarray(keypoints, dtype=np.float64).reshape(-1, 2)
            d_kp, n = self.ctx.to_device(kp, np.float64), len(kp)
        check(self.ctx.lib.pxr_arena_extract(self.ctx.handle, self.handle, int(first), int(n), C.c_void_p(cai["data"][0]),
                                             src, int(shape[1]), int(shape[2]), d_kp.ptr, float(image_size[0]),
                                             float(image_size[1]), int(bool(l2_normalize))), "pxr_arena_extract")
        self.ctx.sync()          # the temporary keypoint upload may be released after this
        return n

    def extract_dsift(self, first, grey, keypoints, image_size, spatial_bin_size=4, rootsift=True, clipval=0.2,
                      l2_normalize=True):
        """Fill patches [first, first + len(keypoints)) with dense SIFT descriptors of ONE grey image (the reference's `dsift`
        model, pixsfm/features/models/dsift.py, followed by FeatureExtractor.tensor_to_fmap's sparse branch,
        extractor.py:152-199) computed only on the patch windows (pxr_dsift_extract): the dense map is never formed.
        grey: (h, w) uint8 (value / 255) or float32 image, a torch.cuda tensor / __cuda_array_interface__ object or a host
        array (uploaded).  keypoints: (n, 2) COLMAP coordinates in the ORIGINAL image; image_size: its (width, height).
        The arena needs C = 128.  Bit-identical to dsift_dense() followed by extract()."""
        img = _grey_on_device(self.ctx, grey)
        if isinstance(keypoints, DeviceArray):
            d_kp, n = keypoints, keypoints.shape[0]
        else:
            kp = np.ascontiguousarray(keypoints, dtype=np.float64).reshape(-1, 2)
            d_kp, n = self.ctx.to_device(kp, np.float64), len(kp)
        check(self.ctx.lib.pxr_dsift_extract(self.ctx.handle, self.handle, int(first), int(n), img.ptr, img.dtype, img.h, img.w,
                                             int(spatial_bin_size), int(bool(rootsift)), float(clipval), d_kp.ptr,
                                             float(image_size[0]), float(image_size[1]), int(bool(l2_normalize))),
              "pxr_dsift_extract")
        self.ctx.sync()          # the temporary uploads may be released after this
        return n

    def download(self, first=0, count=None):
        """(patches, corners, scales) of a range of the arena as numpy arrays (tests / debugging)."""
        count = self.n - first if count is None else count
        patches = np.empty((count, self.H, self.W, self.C), dtype=self.dtype)
        corners = np.empty((count, 2), dtype=np.int32)
        scales = np.empty((count, 2), dtype=np.float64)
        lib, h = self.ctx.lib, self.ctx.handle
        pb = patches[0].nbytes if count else 0
        check(lib.pxr_memcpy_d2h(h, patches.ctypes.data, C.c_void_p(self.data_ptr + pb * first), patches.nbytes), "d2h")
        check(lib.pxr_memcpy_d2h(h, corners.ctypes.data, C.c_void_p(lib.pxr_arena_corners(self.handle) + 8 * first),
                                 corners.nbytes), "d2h")
        check(lib.pxr_memcpy_d2h(h, scales.ctypes.data, C.c_void_p(lib.pxr_arena_scales(self.handle) + 16 * first),
                                 scales.nbytes), "d2h")
        return patches, corners, scales

    @property
    def data_ptr(self):
        return self.ctx.lib.pxr_arena_data(self.handle)

    @property
    def upsampling_factor(self):
        """FeaturePatch::UpsamplingFactor of every patch of the arena (cost maps; 1 for feature patches)."""
        return float(self.ctx.lib.pxr_arena_upsampling(self.handle))

    @upsampling_factor.setter
    def upsampling_factor(self, value):
        check(self.ctx.lib.pxr_arena_set_upsampling(self.handle, float(value)), "pxr_arena_set_upsampling")

    def close(self):
        if getattr(self, "handle", None) and self.ctx.handle:
            self.ctx.lib.pxr_arena_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Grey:
    """A grey image on the device: pointer, pxr dtype, size (+ whatever keeps the memory alive)."""

    def __init__(self, ptr, dtype, h, w, keep):
        self.ptr, self.dtype, self.h, self.w, self.keep = C.c_void_p(ptr), dtype, int(h), int(w), keep


def _grey_on_device(ctx, grey):
    """(h, w) or (1, 1, h, w) uint8 / float32 grey image -> _Grey; host arrays are uploaded, device tensors used in place."""
    cai = getattr(grey, "__cuda_array_interface__", None)
    if cai is None:
        a = np.asarray(grey)
        if a.dtype not in (np.uint8, np.float32):
            raise ValueError("grey image dtype %s not supported (uint8 / float32)" % a.dtype)
        a = np.ascontiguousarray(a)
        shape = a.shape
        while len(shape) > 2 and shape[0] == 1:
            shape = shape[1:]
        if len(shape) != 2 or a.size == 0:
            raise ValueError("grey image must be (h, w); got %r" % (a.shape,))
        d = ctx.to_device(a)
        return _Grey(d.ptr.value, _lib.U8 if a.dtype == np.uint8 else F32, shape[0], shape[1], d)
    shape = tuple(cai["shape"])
    while len(shape) > 2 and shape[0] == 1:
        shape = shape[1:]
    if len(shape) != 2 or 0 in shape:
        raise ValueError("grey image must be (h, w); got %r" % (tuple(cai["shape"]),))
    dt = {"|u1": _lib.U8, "<f4": F32}.get(cai["typestr"])
    if dt is None:
        raise ValueError("grey image dtype %s not supported (uint8 / float32)" % cai["typestr"])
    if cai.get("strides") is not None:
        item = 1 if dt == _lib.U8 else 4
        full = tuple(cai["shape"])
        if tuple(cai["strides"]) != tuple(int(np.prod(full[i + 1:])) * item for i in range(len(full))):
            raise ValueError("grey image must be contiguous (call .contiguous())")
    _sync_torch()
    return _Grey(cai["data"][0], dt, shape[0], shape[1], grey)


def _sync_torch():
    """Work torch queued on its own stream (the upload of a tensor, say) completes before a kernel on the context's stream."""
    import sys
    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_initialized():
        torch.cuda.current_stream().synchronize()


def dsift_dense(ctx, grey, spatial_bin_size=4, rootsift=True, clipval=0.2):
    """The reference's `dsift` model (pixsfm/features/models/dsift.py: kornia DenseSIFTDescriptor(8, 4, spatial_bin_size,
    rootsift, clipval, stride=1, padding=1)) on ONE grey image, on the GPU (pxr_dsift_dense): a torch.cuda float32 tensor
    (1, 128, h, w) on the context's device.  grey: (h, w) uint8 (value / 255, as to_tensor) or float32, device or host."""
    import torch
    img = _grey_on_device(ctx, grey)
    out = torch.empty((1, 128, img.h, img.w), dtype=torch.float32, device="cuda:%d" % ctx.device)
    _sync_torch()
    check(ctx.lib.pxr_dsift_dense(ctx.handle, img.ptr, img.dtype, img.h, img.w, int(spatial_bin_size), int(bool(rootsift)),
                                  float(clipval), C.c_void_p(out.data_ptr())), "pxr_dsift_dense")
    ctx.sync()
    return out


def interpolate(ctx, arena, cfg, keypoints, patch_idx, jacobian=False):
    """PatchInterpolator::Evaluate, batched (pxr_interpolate): descriptors (n, C) of arena patches patch_idx at
    the keypoints (COLMAP image coordinates) and, with jacobian=True, their (n, C, 2) derivatives d/d(x, y)."""
    kp = ctx.to_device(np.ascontiguousarray(keypoints, dtype=np.float64).reshape(-1, 2), np.float64)
    n = kp.shape[0]
    pidx = ctx.to_device(np.ascontiguousarray(patch_idx, dtype=np.int64), np.int64)
    desc = ctx.empty((n, arena.C), np.float64)
    J = ctx.empty((n, arena.C, 2), np.float64) if jacobian else None
    check(ctx.lib.pxr_interpolate(ctx.handle, arena.handle, C.byref(cfg), n, kp.ptr, pidx.ptr, desc.ptr,
                                  J.ptr if J else None), "pxr_interpolate")
    return desc.download(), (J.download() if J else None)


def nearest_references(ctx, arena, cfg, keypoints, patch_idx, cand_ptr, cand_desc, cand_index=None, want_desc=False):
    """FindNearestReferences (localization/src/nearest_references.h:20-52) on the device.
    keypoints (n, 2), patch_idx (n,) arena patches of the query keypoints; candidates of correspondence i:
    rows cand_index[cand_ptr[i]:cand_ptr[i+1]] of cand_desc (a DeviceArray or host array (m, C); cand_index None:
    the rows themselves).  Returns (best row per correspondence, squared distances, winners (n, C) | None)."""
    kp = ctx.to_device(np.ascontiguousarray(keypoints, dtype=np.float64).reshape(-1, 2), np.float64)
    n = kp.shape[0]
    pidx = ctx.to_device(np.ascontiguousarray(patch_idx, dtype=np.int64), np.int64)
    cptr = ctx.to_device(np.ascontiguousarray(cand_ptr, dtype=np.int64), np.int64)
    cidx = None if cand_index is None else ctx.to_device(np.ascontiguousarray(cand_index, dtype=np.int64), np.int64)
    cdesc = cand_desc if isinstance(cand_desc, DeviceArray) else ctx.to_device(np.ascontiguousarray(cand_desc, dtype=np.float64), np.float64)
    best = ctx.empty((n,), np.int64)
    dist = ctx.empty((n,), np.float64)
    out = ctx.empty((n, arena.C), np.float64) if want_desc else None
    check(ctx.lib.pxr_nearest_references(ctx.handle, arena.handle, C.byref(cfg), n, kp.ptr, pidx.ptr, cptr.ptr,
                                         cidx.ptr if cidx else None, cdesc.ptr, best.ptr, dist.ptr,
                                         out.ptr if out else None), "pxr_nearest_references")
    return best.download(), dist.download(), (out.download() if out else None)


def dense_spd_inverse(ctx, a):
    """The inverse of a symmetric positive definite matrix (pxr_dense_spd_inverse): `a` is a DeviceArray (n, n), inverted in
    place, or a host array, of which only the upper triangle is read.  Returns (info, inverse): info is 0, or the 1-based
    index of the first non-positive pivot -- the inverse then holds nothing meaningful.  The result is symmetric bit for bit
    and the same on every run."""
    d = a if isinstance(a, DeviceArray) else ctx.to_device(np.ascontiguousarray(a, dtype=np.float64), np.float64)
    if len(d.shape) != 2 or d.shape[0] != d.shape[1] or d.shape[0] < 1:
        raise ValueError("dense_spd_inverse takes a square matrix")
    info = C.c_int(0)
    check(ctx.lib.pxr_dense_spd_inverse(ctx.handle, d.ptr, int(d.shape[0]), C.byref(info)), "pxr_dense_spd_inverse")
    return info.value, (d if d is a else d.download())


def interp_cfg(l2_normalize=True, use_float_simd=False, check_bounds=False, mode="BICUBIC", nodes=None,
               ncc_normalize=False, **_):
    """InterpolationConfig (pixsfm/base/main.py:1-7).  Only the hot-path configuration is accepted."""
    if str(mode).upper() != "BICUBIC":
        raise ValueError("InterpolatorType %r is outside the accelerated path (BICUBIC only)" % (mode,))
    if nodes is not None and [list(map(float, n)) for n in nodes] != [[0.0, 0.0]]:
        raise ValueError("only a single interpolation node [[0, 0]] is supported (N_NODES = 1)")
    if ncc_normalize:
        raise ValueError("ncc_normalize needs N_NODES > 1, which is outside the accelerated path")
    return InterpCfg(int(l2_normalize), int(use_float_simd), int(check_bounds))


def make_loss(name="cauchy", params=(0.25,)):
    name = str(name).lower()
    if name not in _lib.LOSS_IDS:
        raise ValueError("unsupported loss %r (have %s)" % (name, sorted(_lib.LOSS_IDS)))
    a = float(params[0]) if (params is not None and len(params)) else 1.0
    return Loss(_lib.LOSS_IDS[name], a)


def lm_options(max_iterations=100, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0,
               initial_radius=1e4, max_radius=1e16, min_radius=1e-32, min_relative_decrease=1e-3,
               min_lm_diagonal=1e-6, max_lm_diagonal=1e32, max_consecutive_invalid_steps=10, jacobi_scaling=1,
               use_inner_iterations=False, inner_iteration_tolerance=1e-3, linear_solver="auto",
               max_linear_solver_iterations=200, eta=0.1, linear_r_tolerance=-1.0, **ignored):
    """Subset of ceres::Solver::Options the engine honours (pixsfm/base/main.py:9-22 +
    bundle_adjustment_options.h:48-64); unknown keys are ignored like pyceres ignores nothing --
    callers should pass only what they need."""
    return _lib.LMOptions(int(max_iterations), float(function_tolerance), float(gradient_tolerance),
                          float(parameter_tolerance), float(initial_radius), float(max_radius), float(min_radius),
                          float(min_relative_decrease), float(min_lm_diagonal), float(max_lm_diagonal),
                          int(max_consecutive_invalid_steps), int(jacobi_scaling), int(bool(use_inner_iterations)),
                          float(inner_iteration_tolerance), _linear_solver_id(linear_solver),
                          int(max_linear_solver_iterations), float(eta), float(linear_r_tolerance))


def _linear_solver_id(name):
    """"auto": by image count like bundle_optimizer.h:180-191 (<= 1000 images: Schur complement + Cholesky;
    more: ITERATIVE_SCHUR).  Ceres' names are accepted: DENSE_SCHUR / SPARSE_SCHUR -> direct, ITERATIVE_SCHUR."""
    if isinstance(name, int):
        return int(name)
    key = str(name).lower()
    table = {"auto": _lib.LINEAR_AUTO, "direct": _lib.LINEAR_DIRECT, "dense_schur": _lib.LINEAR_DIRECT,
             "sparse_schur": _lib.LINEAR_DIRECT, "iterative": _lib.LINEAR_ITERATIVE,
             "iterative_schur": _lib.LINEAR_ITERATIVE}
    if key not in table:
        raise ValueError("unknown linear solver %r (auto, direct, iterative)" % (name,))
    return table[key]


def _padded_cam_params(cam_params, n_cameras):
    """cam_params as (n_cameras, KPAD), zero-padded.  A 2-D array of n_cameras rows (or of one row, for every camera) is taken
    as it is, anything else -- a flat list, one camera's parameters -- is reshaped to n_cameras rows."""
    out = np.zeros((n_cameras, KPAD))
    cp = np.asarray(cam_params, dtype=np.float64)
    if cp.ndim != 2 or cp.shape[0] not in (1, n_cameras):
        cp = cp.reshape(n_cameras, -1)
    out[:, :cp.shape[1]] = cp
    return out


def _csr_offsets(offsets, name, rows):
    """The offsets of a CSR list as a flat int64 array: `name` must hold `rows` + 1 entries, at least one."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    if len(offsets) < 1:
        raise ValueError("%s must hold %s + 1 entries" % (name, rows))
    return offsets


def _start(values, rows, width):
    """The host array an output starts from: the caller's (rows, width), or NaN -- what a row without a result keeps."""
    return np.full((rows, width), np.nan) if values is None else np.asarray(values, dtype=np.float64).reshape(rows, width)


def _launch(ctx, name, args, stages, timed):
    """Call the entry point `name`, or with `timed` its twin `name`_timed, which also fills one HIP-event time per stage.
    Returns {stage: milliseconds}, or None for an untimed call."""
    if not timed:
        check(getattr(ctx.lib, name)(*args), name)
        return None
    ms = (C.c_double * len(stages))()
    check(getattr(ctx.lib, name + "_timed")(*args, ms), name + "_timed")
    return dict(zip(stages, (float(x) for x in ms)))


_ROBUST_STAGES = ("records", "compact", "hypotheses", "refine")     # the kernels of abspose and of the three pair estimators


def column_layout(pose_const, tvec_const_mask, cam_const_mask, cam_model):
    """The columns of the reduced camera system (block_layout, csrc/pxr_ba_structure.h): per image 3 rotation columns and the
    variable tvec components, then per camera the variable intrinsics.  Returns pose_off / pose_dim (per image), intr_off /
    intr_dim (per camera), pose_slots / intr_slots (per block: the component 0..5 of (rotation, t) / the parameter index of every
    column) and n_c."""
    off = 0
    pose_off, pose_dim, pose_slots = [], [], []
    for const, tm in zip(pose_const, tvec_const_mask):
        slots = [] if const else [0, 1, 2] + [3 + k for k in range(3) if not (int(tm) >> k) & 1]
        pose_off.append(off); pose_dim.append(len(slots)); pose_slots.append(slots)
        off += len(slots)
    intr_off, intr_dim, intr_slots = [], [], []
    for mask, model in zip(cam_const_mask, cam_model):
        slots = [k for k in range(_lib.CAMERA_NUM_PARAMS[int(model)]) if not (int(mask) >> k) & 1]
        intr_off.append(off); intr_dim.append(len(slots)); intr_slots.append(slots)
        off += len(slots)
    return {"pose_off": pose_off, "pose_dim": pose_dim, "pose_slots": pose_slots, "intr_off": intr_off, "intr_dim": intr_dim,
            "intr_slots": intr_slots, "n_c": off}


class _BABase:
    """What the featuremetric and the geometric bundle-adjustment problems share: the device arrays of poses, cameras and
    points behind one pxr_ba_view, the records of the last evaluation, and the host side of a solve."""

    def _upload(self, ctx, g, **more):
        """Counts, the shared device arrays of problem dict `g` plus `more`, the record buffer and the view."""
        self.ctx = ctx
        self.n_obs = len(g["obs_image"])
        self.n_images = len(g["image_camera"])
        self.n_cameras = len(g["cam_model"])
        self.n_points = len(g["xyz"])
        self.d = {
            "obs_image": ctx.to_device(g["obs_image"], np.int32),
            "obs_point": ctx.to_device(g["obs_point"], np.int32),
            "image_camera": ctx.to_device(g["image_camera"], np.int32),
            "qvec": ctx.to_device(g["qvec"], np.float64),
            "tvec": ctx.to_device(g["tvec"], np.float64),
            "cam_model": ctx.to_device(g["cam_model"], np.int32),
            "cam_params": ctx.to_device(_padded_cam_params(g["cam_params"], self.n_cameras), np.float64),
            "xyz": ctx.to_device(g["xyz"], np.float64),
            **more,
        }
        self.rec = ctx.empty((self.n_obs, OBS_REC), np.float64)
        self.view = self._view()

    def _view(self):
        d = self.d
        patch, refs = d.get("obs_patch"), d.get("refs")
        return BaView(self.n_obs, d["obs_image"].ptr, d["obs_point"].ptr, patch.ptr if patch is not None else None,
                      self.n_images, d["image_camera"].ptr, d["qvec"].ptr, d["tvec"].ptr,
                      self.n_cameras, d["cam_model"].ptr, d["cam_params"].ptr,
                      self.n_points, d["xyz"].ptr, refs.ptr if refs is not None else None)

    def _masks(self, pose_const, tvec_const_mask, cam_const_mask, point_const):
        """The constant masks as the arrays the C entry points take, checked against the problem's dimensions."""
        pc = np.ascontiguousarray(pose_const, dtype=np.uint8)
        tm = np.ascontiguousarray(tvec_const_mask, dtype=np.uint8)
        cm = np.ascontiguousarray(cam_const_mask, dtype=np.uint16)
        ptc = np.ascontiguousarray(point_const, dtype=np.uint8)
        if len(pc) != self.n_images or len(tm) != self.n_images or len(cm) != self.n_cameras \
                or len(ptc) != self.n_points:
            raise ValueError("parameterisation arrays do not match the problem dimensions")
        return pc, tm, cm, ptc

    def _solve(self, name, head, loss, pose_const, tvec_const_mask, cam_const_mask, point_const, options, allreduce):
        """The entry point `name` over its leading arguments `head` and what every BA solve takes after them: the loss, the
        constant masks (checked against the problem's dimensions), the options, the all-reduce callback and the summary."""
        pc, tm, cm, ptc = self._masks(pose_const, tvec_const_mask, cam_const_mask, point_const)
        opts = options or lm_options()
        summ = _lib.LMSummary()
        cb = None
        if allreduce is not None:
            def _cb(user, ptr, count):
                try:
                    allreduce(ptr, count)
                    return 0
                except Exception as e:  # noqa: BLE001 -- must not unwind through C
                    import sys
                    print("all-reduce callback failed: %r" % (e,), file=sys.stderr)
                    return 1
            cb = _lib.ALLREDUCE_FN(_cb)
        check(getattr(self.ctx.lib, name)(*head, C.byref(loss), pc.ctypes.data, tm.ctypes.data, cm.ctypes.data, ptc.ctypes.data,
                                          C.byref(opts), C.cast(cb, C.c_void_p) if cb else None, None, C.byref(summ)), name)
        return summ.as_dict()

    def covariance(self, loss, pose_const, tvec_const_mask, cam_const_mask, point_const, rec=None, cameras=False):
        """Covariance of the parameters at the current point (pxr_ba_covariance): blocks of the inverse of the Gauss-Newton
        matrix the solver linearises, from the records `rec` (default: those of the last eval() -- evaluate first, with
        Jacobians).  Returns a dict of numpy arrays: "pose" (n_images, 6, 6) in the order (rotation tangent, tx, ty, tz) with
        the rotation in the solver's HALF-angle units, "intrinsics" (n_cameras, KPAD, KPAD), "points" (n_points, 3, 3; NaN for
        a singular point), with `cameras` also "cameras" (n_c, n_c) and "columns" (column_layout), and "summary".  Rows and columns
        of constant parameters are zero.  summary["info"] > 0: the reduced camera matrix is rank deficient at that column (a gauge
        is not fixed) and the arrays hold nothing meaningful."""
        pc, tm, cm, ptc = self._masks(pose_const, tvec_const_mask, cam_const_mask, point_const)
        ctx = self.ctx
        cols = column_layout(pc, tm, cm, self.d["cam_model"].download())
        n_c = cols["n_c"]
        pose = ctx.empty((self.n_images, 6, 6), np.float64)
        intr = ctx.empty((self.n_cameras, KPAD, KPAD), np.float64)
        pts = ctx.empty((self.n_points, 3, 3), np.float64)
        dense = ctx.empty((max(n_c, 1), max(n_c, 1)), np.float64) if cameras else None
        summ = _lib.CovSummary()
        check(ctx.lib.pxr_ba_covariance(ctx.handle, C.byref(self.view), (self.rec if rec is None else rec).ptr, C.byref(loss),
                                        pc.ctypes.data, tm.ctypes.data, cm.ctypes.data, ptc.ctypes.data,
                                        dense.ptr if dense else None, pose.ptr, intr.ptr, pts.ptr, C.byref(summ)), "pxr_ba_covariance")
        out = {"pose": pose.download(), "intrinsics": intr.download(), "points": pts.download(), "summary": summ.as_dict()}
        if summ.num_camera_unknowns != n_c:
            raise RuntimeError("column layout mismatch: %d columns here, %d in the library" % (n_c, summ.num_camera_unknowns))
        if cameras:
            out["cameras"] = dense.download()[:n_c, :n_c]
            out["columns"] = cols
        return out

    def projection_jacobian(self, out=None):
        """The 2 x (10+K) projection Jacobian P of every observation (k_jac) -- for the geometric problem the Jacobian of the
        residual block itself; `out` re-uses a device array."""
        P = out if out is not None else self.ctx.empty((self.n_obs, 2, 10 + KPAD), np.float64)
        check(self.ctx.lib.pxr_ba_projection_jacobian(self.ctx.handle, C.byref(self.view), P.ptr),
              "pxr_ba_projection_jacobian")
        return P

    def params(self):
        """Download (qvec, tvec, cam_params, xyz)."""
        d = self.d
        return d["qvec"].download(), d["tvec"].download(), d["cam_params"].download(), d["xyz"].download()

    def cost(self, loss):
        """Sum of 0.5 rho(|r|^2) over the records of the last eval()."""
        out = C.c_double()
        check(self.ctx.lib.pxr_ba_cost(self.ctx.handle, self.rec.ptr, self.n_obs, C.byref(loss), C.byref(out)),
              "pxr_ba_cost")
        return out.value


class BAProblem(_BABase):
    """Device-resident flat arrays of a bundle-adjustment problem (pxr_ba_view).

    problem: dict with obs_image, obs_point, obs_patch, image_camera, qvec, tvec,
    cam_model, cam_params (n_cams x KPAD), xyz, refs (n_points x C; None: no reference is
    subtracted -- the cost-map BA, costmap_bundle_optimizer.h:104-119).
    """

    def __init__(self, ctx, arena, problem):
        self.arena = arena
        g = problem
        self._upload(ctx, g, obs_patch=ctx.to_device(g["obs_patch"], np.int64),
                     refs=ctx.to_device(g["refs"], np.float64) if g.get("refs") is not None else None)

    def extract_costmaps(self, loss, as_gradientfield=True, apply_sqrt=False, dtype=None, out=None, first_out=0,
                         upsampling_factor=1.0, compute_cross_derivative=False, cfg=None):
        """CostMapExtractor (bundle_adjustment/src/costmap_extractor.h:177-358) on the GPU: one cost map per
        observation -- the featuremetric error of every texel of its feature patch against the reference of
        its 3D point (this problem's `refs`, e.g. after compute_references()).  Returns a PatchArena of
        n_obs maps, 3 channels [cost, dcost/dr, dcost/dc] (as_gradientfield) or 1, dtype = the features' unless
        given; map i belongs to observation i.  out: an existing arena to write into, maps first_out .. first_out + n_obs - 1
        (several problems -- chunks of a scene too large for the device -- can share one cost-map arena)."""
        ctx, a = self.ctx, self.arena
        if self.d["refs"] is None:
            raise ValueError("cost maps need reference descriptors")
        up = float(upsampling_factor)
        co = (4 if compute_cross_derivative else 3) if as_gradientfield else 1          # GetEffectiveChannels
        if out is None:
            out = PatchArena(ctx, self.n_obs, int(a.H * (up + 1.0e-6)), int(a.W * (up + 1.0e-6)), co,
                             a.dtype if dtype is None else dtype)
        if up == 1.0 and not compute_cross_derivative:
            check(ctx.lib.pxr_costmap_extract(ctx.handle, a.handle, out.handle, int(first_out), self.n_obs, self.d["obs_patch"].ptr,
                                              self.d["obs_point"].ptr, self.d["refs"].ptr, C.byref(loss),
                                              int(bool(as_gradientfield)), int(bool(apply_sqrt))), "pxr_costmap_extract")
        else:       # CostMapConfig.upsampling_factor / compute_cross_derivative: the interpolating branch, under `cfg`
            cfg = cfg if cfg is not None else interp_cfg()
            check(ctx.lib.pxr_costmap_extract_ex(ctx.handle, a.handle, out.handle, int(first_out), self.n_obs,
                                                 self.d["obs_patch"].ptr, self.d["obs_point"].ptr, self.d["refs"].ptr,
                                                 C.byref(loss), int(bool(as_gradientfield)), int(bool(apply_sqrt)),
                                                 C.byref(cfg), up, int(bool(compute_cross_derivative))), "pxr_costmap_extract_ex")
        return out

    def costmap_problem(self, costmaps):
        """The cost-map BA problem over this problem's parameters (CostMapBundleOptimizer::AddResiduals,
        costmap_bundle_optimizer.h:76-132): the SAME device qvec / tvec / cam_params / xyz arrays (refined in
        place by either problem), observation i reads cost map i, no reference descriptor."""
        p = object.__new__(BAProblem)
        p.ctx, p.arena = self.ctx, costmaps
        p.n_obs, p.n_images, p.n_cameras, p.n_points = self.n_obs, self.n_images, self.n_cameras, self.n_points
        p.d = dict(self.d)
        p.d["obs_patch"] = self.ctx.to_device(np.arange(self.n_obs, dtype=np.int64), np.int64)
        p.d["refs"] = None
        p.rec = self.ctx.empty((self.n_obs, OBS_REC), np.float64)
        p.view = p._view()
        return p

    def eval(self, cfg, with_jacobian=True, materialize=False):
        """Launch the fused residual kernel.  Returns device arrays (rec, r, gx, gy)."""
        ctx = self.ctx
        r = gx = gy = None
        if materialize:
            r = ctx.empty((self.n_obs, self.arena.C), np.float64)
            if with_jacobian:
                gx = ctx.empty((self.n_obs, self.arena.C), np.float64)
                gy = ctx.empty((self.n_obs, self.arena.C), np.float64)
        check(ctx.lib.pxr_ba_eval(ctx.handle, self.arena.handle, C.byref(self.view), C.byref(cfg),
                                  int(with_jacobian), self.rec.ptr,
                                  r.ptr if r else None, gx.ptr if gx else None, gy.ptr if gy else None),
              "pxr_ba_eval")
        return self.rec, r, gx, gy

    def eval_gram(self, cfg, reset=True, sync=True):
        """The records of eval(with_jacobian=True) through the Gram-matrix cache of the context (pxr_ba_eval_gram).  Returns
        (rec, number of observations whose matrices this call built -- None without `sync`)."""
        built = C.c_int32(0)
        check(self.ctx.lib.pxr_ba_eval_gram(self.ctx.handle, self.arena.handle, C.byref(self.view), C.byref(cfg), int(bool(reset)),
                                            self.rec.ptr, C.byref(built) if sync else None), "pxr_ba_eval_gram")
        return self.rec, (built.value if sync else None)

    def solve(self, cfg, loss, pose_const, tvec_const_mask, cam_const_mask, point_const, options=None,
              allreduce=None):
        """Run the GPU LM (pxr_ba_solve); parameters are refined in place on the device.

        allreduce: optional callable(device_ptr:int, count:int) summing `count` doubles in place
        over the ranks (see parallel.make_allreduce); None for one GPU.
        Returns the summary dict; use params() to fetch the refined parameters.
        """
        head = (self.ctx.handle, self.arena.handle, C.byref(self.view), C.byref(cfg))
        return self._solve("pxr_ba_solve", head, loss, pose_const, tvec_const_mask, cam_const_mask, point_const, options, allreduce)

    def compute_references(self, cfg, loss, iters=100, keep_mean=False, keep_observations=False):
        """ReferenceExtractor.run on the GPU: fills this problem's `refs` in place (device) and
        returns (ref_obs indices, robust means | None) as numpy arrays.  keep_observations
        (reference_extractor.h:60): the per-observation descriptors stay on the device in
        self.obs_desc (n_obs x C), e.g. as candidates for nearest_references()."""
        ctx = self.ctx
        ref_obs = ctx.empty((self.n_points,), np.int64)
        mean = ctx.empty((self.n_points, self.arena.C), np.float64) if keep_mean else None
        self.obs_desc = ctx.empty((self.n_obs, self.arena.C), np.float64) if keep_observations else None
        check(ctx.lib.pxr_ba_compute_references(ctx.handle, self.arena.handle, C.byref(self.view), C.byref(cfg),
                                                C.byref(loss), int(iters), self.d["refs"].ptr, ref_obs.ptr,
                                                mean.ptr if mean else None,
                                                self.obs_desc.ptr if self.obs_desc else None), "pxr_ba_compute_references")
        return ref_obs.download(), (mean.download() if mean else None)


class GeometricBAProblem(_BABase):
    """Device-resident flat arrays of a geometric (reprojection-error) bundle-adjustment problem: the pxr_ba_view without a
    patch arena plus the observed keypoints (GeometricBundleOptimizer::AddResiduals, geometric_bundle_optimizer.h:39-88).

    problem: dict as for BAProblem without obs_patch / refs, plus obs_xy (n_obs x 2, image pixels, COLMAP convention).
    """

    def __init__(self, ctx, problem):
        g = problem
        obs_xy = np.ascontiguousarray(g["obs_xy"], dtype=np.float64).reshape(-1, 2)
        if len(obs_xy) != len(g["obs_image"]):
            raise ValueError("obs_xy must hold one keypoint per observation")
        self._upload(ctx, g, obs_xy=ctx.to_device(obs_xy, np.float64))
        self.res = ctx.empty((self.n_obs, 2), np.float64)

    def eval(self, residuals=True):
        """Launch the reprojection-residual kernel (pxr_ba_geom_eval).  Returns device arrays (rec, res): the 8-double
        records and the residuals (n_obs x 2; None with residuals=False: the records alone, what the solver asks for)."""
        res = self.res if residuals else None
        check(self.ctx.lib.pxr_ba_geom_eval(self.ctx.handle, C.byref(self.view), self.d["obs_xy"].ptr, self.rec.ptr,
                                            res.ptr if res else None), "pxr_ba_geom_eval")
        return self.rec, res

    def reprojection_errors(self):
        """Per-observation reprojection error in pixels at the current parameters (numpy, n_obs)."""
        _, res = self.eval()
        r = res.download()
        return np.hypot(r[:, 0], r[:, 1])

    def solve(self, loss, pose_const, tvec_const_mask, cam_const_mask, point_const, options=None, allreduce=None):
        """Run the GPU LM (pxr_ba_solve_geometric); parameters are refined in place on the device.  Arguments as
        BAProblem.solve without the interpolation configuration.  Returns the summary dict."""
        head = (self.ctx.handle, C.byref(self.view), self.d["obs_xy"].ptr)
        return self._solve("pxr_ba_solve_geometric", head, loss, pose_const, tvec_const_mask, cam_const_mask, point_const, options,
                           allreduce)


def tri_options(min_tri_angle=1.5, max_angle_error=2.0, max_reproj_error=4.0, min_track_len=2, max_hypotheses=256):
    """pxr_tri_options: the triangulator values the reference inherits from COLMAP through hloc (angles in degrees, the
    reprojection error in pixels) and the bound on the two-view hypotheses per track."""
    return _lib.TriOptions(float(min_tri_angle), float(max_angle_error), float(max_reproj_error), int(min_track_len),
                           int(max_hypotheses))


def image_to_world(ctx, cam_model, cam_params, xy, cam_index=None):
    """Camera::ImageToWorld, batched on the GPU (pxr_image_to_world): pixels xy (n, 2) -> normalised image points (n, 2) under
    camera cam_index[i] (None: camera 0) of cam_model (n_cameras,) / cam_params (n_cameras, <= KPAD).  Returns (uv, ok) as
    numpy arrays; uv is NaN where ok is False (no convergence, singular Jacobian, non-finite input)."""
    cam_model = np.atleast_1d(np.asarray(cam_model, dtype=np.int32))
    n_cameras = len(cam_model)
    xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
    n = len(xy)
    if cam_index is not None and len(cam_index) != n:
        raise ValueError("cam_index must hold one camera per pixel")
    if n == 0:
        return np.empty((0, 2)), np.empty((0,), dtype=bool)
    d_model = ctx.to_device(cam_model, np.int32)
    d_params = ctx.to_device(_padded_cam_params(cam_params, n_cameras), np.float64)
    d_xy = ctx.to_device(xy, np.float64)
    d_idx = None if cam_index is None else ctx.to_device(cam_index, np.int32)
    d_uv, d_ok = ctx.empty((n, 2), np.float64), ctx.empty((n,), np.uint8)
    check(ctx.lib.pxr_image_to_world(ctx.handle, n, d_idx.ptr if d_idx else None, n_cameras, d_model.ptr, d_params.ptr, d_xy.ptr,
                                     d_uv.ptr, d_ok.ptr), "pxr_image_to_world")
    return d_uv.download(), d_ok.download().astype(bool)


class TriangulationProblem:
    """Device-resident flat arrays of a track-triangulation problem (pxr_tri_view): known poses and cameras, the keypoints
    of every observation, tracks in CSR form over the observations.

    problem: dict with track_offsets (n_tracks + 1), obs_image, obs_xy (n_obs x 2, image pixels, COLMAP convention),
    image_camera, qvec, tvec, cam_model, cam_params (n_cams x <= KPAD).
    """

    def __init__(self, ctx, problem):
        self.ctx = ctx
        g = problem
        offsets = _csr_offsets(g["track_offsets"], "track_offsets", "n_tracks")
        self.n_tracks = len(offsets) - 1
        self.n_obs = len(g["obs_image"])
        self.n_images = len(g["image_camera"])
        self.n_cameras = len(g["cam_model"])
        obs_xy = np.ascontiguousarray(g["obs_xy"], dtype=np.float64).reshape(-1, 2)
        if len(obs_xy) != self.n_obs:
            raise ValueError("obs_xy must hold one keypoint per observation")
        self.d = {
            "track_offsets": ctx.to_device(offsets, np.int64),
            "obs_image": ctx.to_device(np.asarray(g["obs_image"]).reshape(-1), np.int32),
            "obs_xy": ctx.to_device(obs_xy, np.float64),
            "image_camera": ctx.to_device(g["image_camera"], np.int32),
            "qvec": ctx.to_device(np.asarray(g["qvec"], dtype=np.float64).reshape(-1, 4), np.float64),
            "tvec": ctx.to_device(np.asarray(g["tvec"], dtype=np.float64).reshape(-1, 3), np.float64),
            "cam_model": ctx.to_device(g["cam_model"], np.int32),
            "cam_params": ctx.to_device(_padded_cam_params(g["cam_params"], self.n_cameras), np.float64),
        }
        d = self.d
        self.view = _lib.TriView(self.n_tracks, d["track_offsets"].ptr, self.n_obs, d["obs_image"].ptr, d["obs_xy"].ptr,
                                 self.n_images, d["image_camera"].ptr, d["qvec"].ptr, d["tvec"].ptr, self.n_cameras,
                                 d["cam_model"].ptr, d["cam_params"].ptr)
        self.kernel_ms = None

    def triangulate(self, xyz=None, timed=False, **options):
        """Run the kernels (pxr_triangulate_tracks) with tri_options(**options).  Returns the device arrays
        (xyz (n_tracks, 3), status (n_tracks,) int32, n_inliers (n_tracks,) int32, obs_inlier (n_obs,) uint8,
        obs_err (n_obs,) float64).  xyz: a (n_tracks, 3) host array the output starts from -- rows of tracks without a point
        keep it (default: NaN).  timed: also keep the kernels' HIP-event times in self.kernel_ms
        {"check", "rays", "compact", "tracks"} (milliseconds)."""
        ctx = self.ctx
        opts = tri_options(**options)
        d_xyz = ctx.to_device(_start(xyz, self.n_tracks, 3), np.float64)
        d_status, d_ninl = ctx.empty((self.n_tracks,), np.int32), ctx.empty((self.n_tracks,), np.int32)
        d_inl, d_err = ctx.empty((self.n_obs,), np.uint8), ctx.empty((self.n_obs,), np.float64)
        args = (ctx.handle, C.byref(self.view), C.byref(opts), d_xyz.ptr, d_status.ptr, d_ninl.ptr, d_inl.ptr, d_err.ptr)
        self.kernel_ms = _launch(ctx, "pxr_triangulate_tracks", args, ("check", "rays", "compact", "tracks"), timed) or self.kernel_ms
        return d_xyz, d_status, d_ninl, d_inl, d_err


def rotavg_options(l1_iterations=20, max_iterations=40, min_angle=1e-3, sigma=5.0, tolerance=1e-10):
    """pxr_rotavg_options: iterations of the L1 phase and in all, the floor of the angle in the L1 weights (radians), the Cauchy
    scale after it (degrees), the step below which the iteration stops (radians)."""
    return _lib.RotavgOptions(int(l1_iterations), int(max_iterations), float(min_angle), float(sigma), float(tolerance))


class RotationAveragingProblem:
    """Device-resident view graph of pxr_rotation_averaging: pair_image (n_pairs x 2) indices into the n_images images, pair_qvec
    (n_pairs x 4) the rotation of the second image relative to the first, pair_weight (n_pairs) >= 0."""

    def __init__(self, ctx, n_images, pair_image, pair_qvec, pair_weight):
        self.ctx = ctx
        self.n_images = int(n_images)
        pair_image = np.ascontiguousarray(pair_image, dtype=np.int32).reshape(-1, 2)
        self.n_pairs = len(pair_image)
        pair_qvec = np.ascontiguousarray(pair_qvec, dtype=np.float64).reshape(-1, 4)
        pair_weight = np.ascontiguousarray(pair_weight, dtype=np.float64).reshape(-1)
        if len(pair_qvec) != self.n_pairs or len(pair_weight) != self.n_pairs:
            raise ValueError("pair_qvec and pair_weight must hold one row per pair")
        rows = max(self.n_pairs, 1)        # (an empty graph still gets buffers)
        self.d = {"pair_image": ctx.zeros((rows, 2), np.int32), "pair_qvec": ctx.zeros((rows, 4), np.float64),
                  "pair_weight": ctx.zeros((rows,), np.float64)}
        if self.n_pairs:
            self.d["pair_image"].upload(pair_image)
            self.d["pair_qvec"].upload(pair_qvec)
            self.d["pair_weight"].upload(pair_weight)
        self.kernel_ms = None

    def solve(self, timed=False, **options):
        """Run pxr_rotation_averaging with rotavg_options(**options).  Returns (qvec device array (n_images, 4), root, iterations,
        pair_angle device array (n_pairs,) in radians).  timed: self.kernel_ms {"residuals", "assembly", "solve"} summed over
        the iterations."""
        ctx, d = self.ctx, self.d
        opts = rotavg_options(**options)
        d_q = ctx.to_device(np.full((self.n_images, 4), np.nan), np.float64)
        d_angle = ctx.to_device(np.full((max(self.n_pairs, 1),), np.nan), np.float64)
        root, iterations = C.c_int32(-1), C.c_int32(-1)
        args = (ctx.handle, self.n_images, self.n_pairs, d["pair_image"].ptr, d["pair_qvec"].ptr, d["pair_weight"].ptr, C.byref(opts),
                d_q.ptr, C.byref(root), C.byref(iterations), d_angle.ptr)
        self.kernel_ms = _launch(ctx, "pxr_rotation_averaging", args, ("residuals", "assembly", "solve"), timed) or self.kernel_ms
        return d_q, int(root.value), int(iterations.value), d_angle


def globalpos_options(iterations=8, cheirality_from=2, sigma_obs=1.0, sigma_pair=3.0, min_det=1e-12):
    """pxr_globalpos_options: rounds, the first round (from 0) that rejects what lies behind its camera, the Cauchy scales of the
    observations and the pairs (degrees), the determinant a track's 3 x 3 matrix must exceed."""
    return _lib.GlobalposOptions(int(iterations), int(cheirality_from), float(sigma_obs), float(sigma_pair), float(min_det))


class GlobalPositioningProblem:
    """Device-resident arrays of pxr_global_positioning.

    problem: dict as for TriangulationProblem (track_offsets, obs_image, obs_xy, image_camera, qvec = the averaged rotations,
    cam_model, cam_params; a tvec is ignored); pair_image (n_pairs x 2), pair_dir (n_pairs x 3) the unit baseline directions in
    the world, pair_weight (n_pairs) >= 0; root: the image at the origin."""

    def __init__(self, ctx, problem, pair_image, pair_dir, pair_weight, root):
        self.ctx = ctx
        g = problem
        offsets = _csr_offsets(g["track_offsets"], "track_offsets", "n_tracks")
        self.n_tracks = len(offsets) - 1
        self.n_obs = len(g["obs_image"])
        self.n_images = len(g["image_camera"])
        self.n_cameras = len(g["cam_model"])
        self.root = int(root)
        obs_xy = np.ascontiguousarray(g["obs_xy"], dtype=np.float64).reshape(-1, 2)
        if len(obs_xy) != self.n_obs:
            raise ValueError("obs_xy must hold one keypoint per observation")
        pair_image = np.ascontiguousarray(pair_image, dtype=np.int32).reshape(-1, 2)
        self.n_pairs = len(pair_image)
        pair_dir = np.ascontiguousarray(pair_dir, dtype=np.float64).reshape(-1, 3)
        pair_weight = np.ascontiguousarray(pair_weight, dtype=np.float64).reshape(-1)
        if len(pair_dir) != self.n_pairs or len(pair_weight) != self.n_pairs:
            raise ValueError("pair_dir and pair_weight must hold one row per pair")
        rows, obs = max(self.n_pairs, 1), max(self.n_obs, 1)
        self.d = {
            "track_offsets": ctx.to_device(offsets, np.int64),
            "obs_image": ctx.zeros((obs,), np.int32), "obs_xy": ctx.zeros((obs, 2), np.float64),
            "image_camera": ctx.to_device(g["image_camera"], np.int32),
            "qvec": ctx.to_device(np.asarray(g["qvec"], dtype=np.float64).reshape(-1, 4), np.float64),
            "cam_model": ctx.to_device(g["cam_model"], np.int32),
            "cam_params": ctx.to_device(_padded_cam_params(g["cam_params"], self.n_cameras), np.float64),
            "pair_image": ctx.zeros((rows, 2), np.int32), "pair_dir": ctx.zeros((rows, 3), np.float64),
            "pair_weight": ctx.zeros((rows,), np.float64),
        }
        d = self.d
        if self.n_obs:
            d["obs_image"].upload(np.asarray(g["obs_image"]).reshape(-1))
            d["obs_xy"].upload(obs_xy)
        if self.n_pairs:
            d["pair_image"].upload(pair_image)
            d["pair_dir"].upload(pair_dir)
            d["pair_weight"].upload(pair_weight)
        self.view = _lib.TriView(self.n_tracks, d["track_offsets"].ptr, self.n_obs, d["obs_image"].ptr, d["obs_xy"].ptr,
                                 self.n_images, d["image_camera"].ptr, d["qvec"].ptr, None, self.n_cameras,
                                 d["cam_model"].ptr, d["cam_params"].ptr)
        self.kernel_ms = None

    def solve(self, timed=False, **options):
        """Run pxr_global_positioning with globalpos_options(**options).  Returns a dict of device arrays centre (n_images, 3), xyz
        (n_tracks, 3; NaN where track_status is 1), track_status (n_tracks,) int32, obs_weight (n_obs,), pair_weight (n_pairs,),
        and the host values status (0 = ok, 1 = degenerate) and rounds.  timed: self.kernel_ms {"tracks", "contraction", "gauge_pack",
        "cholesky", "update"} summed over the rounds."""
        ctx, d = self.ctx, self.d
        opts = globalpos_options(**options)
        out = dict(centre=ctx.to_device(np.full((self.n_images, 3), np.nan), np.float64),
                   xyz=ctx.to_device(np.full((max(self.n_tracks, 1), 3), np.nan), np.float64),
                   track_status=ctx.to_device(np.full((max(self.n_tracks, 1),), -1), np.int32),
                   obs_weight=ctx.zeros((max(self.n_obs, 1),), np.float64), pair_weight=ctx.zeros((max(self.n_pairs, 1),), np.float64))
        status, rounds = C.c_int32(-1), C.c_int32(-1)
        args = (ctx.handle, C.byref(self.view), self.n_pairs, d["pair_image"].ptr, d["pair_dir"].ptr, d["pair_weight"].ptr, self.root,
                C.byref(opts), out["centre"].ptr, out["xyz"].ptr, out["track_status"].ptr, out["obs_weight"].ptr, out["pair_weight"].ptr,
                C.byref(status), C.byref(rounds))
        stages = ("tracks", "contraction", "gauge_pack", "cholesky", "update")
        self.kernel_ms = _launch(ctx, "pxr_global_positioning", args, stages, timed) or self.kernel_ms
        out.update(status=int(status.value), rounds=int(rounds.value))
        return out


def abspose_options(max_error=12.0, min_inlier_ratio=0.01, min_num_inliers=4, confidence=0.99999, min_num_trials=64,
                    max_num_trials=4096, round_size=64, seed=0, refine_max_iterations=100, refine_loss_scale=1.0, lo_rounds=4):
    """pxr_abspose_options: pycolmap 0.x / COLMAP 3.8's AbsolutePoseEstimationOptions and AbsolutePoseRefinementOptions values
    with the reference's max_error of 12 px, and the estimator's own round_size, seed and lo_rounds."""
    return _lib.AbsposeOptions(float(max_error), float(min_inlier_ratio), float(confidence), float(refine_loss_scale), int(seed),
                               int(min_num_inliers), int(min_num_trials), int(max_num_trials), int(round_size),
                               int(refine_max_iterations), int(lo_rounds))


class AbsolutePoseProblem:
    """Device-resident flat arrays of a batch of absolute-pose queries (pxr_absolute_pose): the 2D-3D correspondences of
    every query in CSR form, one camera per query.

    problem: dict with query_offsets (n_queries + 1), xy (n_corr x 2, image pixels, COLMAP convention), xyz (n_corr x 3),
    query_camera (n_queries), cam_model, cam_params (n_cams x <= KPAD).
    """

    def __init__(self, ctx, problem):
        self.ctx = ctx
        g = problem
        offsets = _csr_offsets(g["query_offsets"], "query_offsets", "n_queries")
        self.n_queries = len(offsets) - 1
        xy = np.ascontiguousarray(g["xy"], dtype=np.float64).reshape(-1, 2)
        xyz = np.ascontiguousarray(g["xyz"], dtype=np.float64).reshape(-1, 3)
        if len(xy) != len(xyz):
            raise ValueError("xy and xyz must hold one row per correspondence")
        self.n_corr = len(xy)
        self.n_cameras = len(g["cam_model"])
        if len(np.asarray(g["query_camera"]).reshape(-1)) != self.n_queries:
            raise ValueError("query_camera must hold one camera per query")
        self.d = {
            "query_offsets": ctx.to_device(offsets, np.int64),
            "xy": ctx.to_device(xy, np.float64),
            "xyz": ctx.to_device(xyz, np.float64),
            "query_camera": ctx.to_device(np.asarray(g["query_camera"]).reshape(-1), np.int32),
            "cam_model": ctx.to_device(g["cam_model"], np.int32),
            "cam_params": ctx.to_device(_padded_cam_params(g["cam_params"], self.n_cameras), np.float64),
        }
        self.kernel_ms = None

    @classmethod
    def from_device(cls, ctx, query_offsets, n_corr, xy, xyz, query_camera, cam_model, cam_params):
        """The same problem over arrays that already live on the device (DeviceArray each; nothing is copied): query_offsets
        (n_queries + 1) int64, xy / xyz with at least n_corr rows, query_camera (n_queries) int32, cam_model (n_cameras) int32,
        cam_params (n_cameras, KPAD).  What MapperScene.visibility returns goes in as it is."""
        self = cls.__new__(cls)
        self.ctx = ctx
        self.n_queries = int(query_offsets.shape[0]) - 1
        self.n_corr = int(n_corr)
        self.n_cameras = int(cam_model.shape[0])
        if self.n_queries < 0 or int(query_camera.shape[0]) != self.n_queries:
            raise ValueError("query_camera must hold one camera per query")
        if int(xy.shape[0]) < self.n_corr or int(xyz.shape[0]) < self.n_corr:
            raise ValueError("xy and xyz must hold one row per correspondence")
        self.d = {"query_offsets": query_offsets, "xy": xy, "xyz": xyz, "query_camera": query_camera, "cam_model": cam_model,
                  "cam_params": cam_params}
        self.kernel_ms = None
        return self

    def estimate(self, qvec=None, tvec=None, timed=False, **options):
        """Run the kernels (pxr_absolute_pose) with abspose_options(**options).  Returns the device arrays (qvec (n_queries, 4),
        tvec (n_queries, 3), status, n_inliers, n_trials (n_queries,) int32, inlier (n_corr,) uint8, err (n_corr,) float64).
        qvec / tvec: host arrays the outputs start from -- rows of queries without a pose keep them (default: NaN).  timed: also
        keep the kernels' HIP-event times in self.kernel_ms {"records", "compact", "hypotheses", "refine"} (milliseconds)."""
        ctx, d, T, N = self.ctx, self.d, self.n_queries, self.n_corr
        opts = abspose_options(**options)
        d_q, d_t = ctx.to_device(_start(qvec, T, 4), np.float64), ctx.to_device(_start(tvec, T, 3), np.float64)
        d_status, d_ninl, d_ntr = ctx.empty((T,), np.int32), ctx.empty((T,), np.int32), ctx.empty((T,), np.int32)
        d_inl, d_err = ctx.empty((N,), np.uint8), ctx.empty((N,), np.float64)
        args = (ctx.handle, T, d["query_offsets"].ptr, N, d["xy"].ptr, d["xyz"].ptr, d["query_camera"].ptr, self.n_cameras,
                d["cam_model"].ptr, d["cam_params"].ptr, C.byref(opts), d_q.ptr, d_t.ptr, d_status.ptr, d_ninl.ptr, d_ntr.ptr,
                d_inl.ptr, d_err.ptr)
        self.kernel_ms = _launch(ctx, "pxr_absolute_pose", args, _ROBUST_STAGES, timed) or self.kernel_ms
        return d_q, d_t, d_status, d_ninl, d_ntr, d_inl, d_err


def query_ba_supported(arena):
    """Whether pxr_query_ba_solve has a kernel for the arena's patches (fp16 / fp32 / fp64 with 128 or 64 channels)."""
    return np.dtype(arena.dtype) in _NP2DT and int(arena.C) in (128, 64)


class QueryBAProblem:
    """Device-resident flat arrays of a batch of query bundle adjustments (pxr_query_ba_solve): the residual blocks of every
    query in CSR form, one camera and one pose per query, every point constant.

    problem: dict with query_offsets (n_queries + 1), obs_patch (n_obs, arena indices), xyz (n_obs x 3), refs (n_obs x C),
    qvec (n_queries x 4), tvec (n_queries x 3), query_camera (n_queries), cam_model, cam_params (n_cams x <= KPAD).
    """

    def __init__(self, ctx, arena, problem):
        self.ctx, self.arena = ctx, arena
        g = problem
        offsets = _csr_offsets(g["query_offsets"], "query_offsets", "n_queries")
        self.n_queries = len(offsets) - 1
        obs_patch = np.ascontiguousarray(g["obs_patch"], dtype=np.int64).reshape(-1)
        self.n_obs = len(obs_patch)
        xyz = np.ascontiguousarray(g["xyz"], dtype=np.float64).reshape(-1, 3)
        refs = np.ascontiguousarray(g["refs"], dtype=np.float64)
        if len(xyz) != self.n_obs or refs.size % max(self.n_obs, 1) or (self.n_obs == 0 and refs.size):
            raise ValueError("obs_patch, xyz and refs must hold one row per residual block")
        refs = refs.reshape(self.n_obs, refs.size // max(self.n_obs, 1))
        if self.n_obs and refs.shape[1] != int(arena.C):
            raise ValueError("refs must hold %d channels per residual block" % int(arena.C))
        self.n_cameras = len(g["cam_model"])
        qvec = np.ascontiguousarray(g["qvec"], dtype=np.float64).reshape(-1, 4)
        tvec = np.ascontiguousarray(g["tvec"], dtype=np.float64).reshape(-1, 3)
        if not len(qvec) == len(tvec) == len(np.asarray(g["query_camera"]).reshape(-1)) == self.n_queries:
            raise ValueError("qvec, tvec and query_camera must hold one row per query")
        self.d = {
            "query_offsets": ctx.to_device(offsets, np.int64),
            "obs_patch": ctx.to_device(obs_patch, np.int64),
            "xyz": ctx.to_device(xyz, np.float64),
            "refs": ctx.to_device(refs, np.float64),
            "qvec": ctx.to_device(qvec, np.float64),
            "tvec": ctx.to_device(tvec, np.float64),
            "query_camera": ctx.to_device(np.asarray(g["query_camera"]).reshape(-1), np.int32),
            "cam_model": ctx.to_device(g["cam_model"], np.int32),
            "cam_params": ctx.to_device(_padded_cam_params(g["cam_params"], self.n_cameras), np.float64),
        }
        self.kernel_ms = None

    def solve(self, cfg, loss, options=None, timed=False):
        """Refine every pose in place on the device (pxr_query_ba_solve); returns the per-query summaries as dicts.  timed: also
        keep the solve kernel's HIP-event time in self.kernel_ms {"solve"} (milliseconds)."""
        ctx, d = self.ctx, self.d
        opts = options or lm_options()
        summaries = (_lib.LMSummary * max(self.n_queries, 1))()
        args = (ctx.handle, self.arena.handle, self.n_queries, d["query_offsets"].ptr, self.n_obs, d["obs_patch"].ptr, d["xyz"].ptr,
                d["refs"].ptr, d["query_camera"].ptr, self.n_cameras, d["cam_model"].ptr, d["cam_params"].ptr, d["qvec"].ptr,
                d["tvec"].ptr, C.byref(cfg), C.byref(loss), C.byref(opts), summaries)
        self.kernel_ms = _launch(ctx, "pxr_query_ba_solve", args, ("solve",), timed) or self.kernel_ms
        return [summaries[i].as_dict() for i in range(self.n_queries)]

    def poses(self):
        """(qvec (n_queries, 4), tvec (n_queries, 3)) as they stand on the device."""
        return self.d["qvec"].download(), self.d["tvec"].download()


def two_view_options(max_error=4.0, min_inlier_ratio=0.25, min_num_inliers=15, confidence=0.999, min_num_trials=64,
                     max_num_trials=10000, round_size=64, seed=0, refine_max_iterations=100, lo_rounds=4):
    """pxr_pair_options, the one struct the header also names pxr_two_view_options, pxr_homography_options and
    pxr_fundamental_options: COLMAP 3.8's two-view geometry values as remembered (parity unpinned), and the estimators' own
    min_num_trials, round_size, seed, refine_max_iterations and lo_rounds.  homography_options and fundamental_options are this
    function: the same fields and defaults, for the homography and the fundamental-matrix estimator."""
    return _lib.PairOptions(float(max_error), float(min_inlier_ratio), float(confidence), int(seed), int(min_num_inliers),
                            int(min_num_trials), int(max_num_trials), int(round_size), int(refine_max_iterations), int(lo_rounds))


homography_options = fundamental_options = two_view_options


class _PairProblem:
    """Device-resident flat arrays of a batch of image pairs: the matches of every pair in CSR form, two cameras per pair.

    batch: dict with pair_offsets (n_pairs + 1), xy1 / xy2 (n_matches x 2, image pixels, COLMAP convention), pair_camera
    (n_pairs x 2), cam_model, cam_params (n_cams x <= KPAD).  Any pair problem in place of the dict shares its device arrays:
    several estimators on one upload.
    """

    def __init__(self, ctx, batch):
        self.ctx, self.kernel_ms = ctx, None
        if isinstance(batch, _PairProblem):
            self.n_pairs, self.n_matches, self.n_cameras, self.d = batch.n_pairs, batch.n_matches, batch.n_cameras, batch.d
            return
        g = batch
        offsets = _csr_offsets(g["pair_offsets"], "pair_offsets", "n_pairs")
        self.n_pairs = len(offsets) - 1
        xy1 = np.ascontiguousarray(g["xy1"], dtype=np.float64).reshape(-1, 2)
        xy2 = np.ascontiguousarray(g["xy2"], dtype=np.float64).reshape(-1, 2)
        if len(xy1) != len(xy2):
            raise ValueError("xy1 and xy2 must hold one row per match")
        self.n_matches = len(xy1)
        self.n_cameras = len(g["cam_model"])
        pair_camera = np.ascontiguousarray(g["pair_camera"], dtype=np.int32).reshape(-1, 2)
        if len(pair_camera) != self.n_pairs:
            raise ValueError("pair_camera must hold two cameras per pair")
        self.d = {
            "pair_offsets": ctx.to_device(offsets, np.int64),
            "xy1": ctx.to_device(xy1, np.float64),
            "xy2": ctx.to_device(xy2, np.float64),
            "pair_camera": ctx.to_device(pair_camera, np.int32),
            "cam_model": ctx.to_device(g["cam_model"], np.int32),
            "cam_params": ctx.to_device(_padded_cam_params(g["cam_params"], self.n_cameras), np.float64),
        }

    def _estimate(self, name, options, starts, n_counts, timed, prior=()):
        """Run the entry point `name` with two_view_options(**options).  starts: (host array or None, width) per model output,
        each starting from _start; n_counts: its per-pair int32 outputs; prior: what goes between the batch and the options.
        Returns the device arrays (model outputs, counts, inlier (n_matches,) uint8, err (n_matches,) float64)."""
        ctx, d, T, N = self.ctx, self.d, self.n_pairs, self.n_matches
        opts = two_view_options(**options)
        models = [ctx.to_device(_start(a, T, w), np.float64) for a, w in starts]
        counts = [ctx.empty((T,), np.int32) for _ in range(n_counts)]
        d_inl, d_err = ctx.empty((N,), np.uint8), ctx.empty((N,), np.float64)
        args = (ctx.handle, T, d["pair_offsets"].ptr, N, d["xy1"].ptr, d["xy2"].ptr, d["pair_camera"].ptr, self.n_cameras,
                d["cam_model"].ptr, d["cam_params"].ptr, *prior, C.byref(opts), *(a.ptr for a in models), *(a.ptr for a in counts),
                d_inl.ptr, d_err.ptr)
        self.kernel_ms = _launch(ctx, name, args, _ROBUST_STAGES, timed) or self.kernel_ms
        return (*models, *counts, d_inl, d_err)


class TwoViewProblem(_PairProblem):
    """The pair batch of pxr_two_view_geometry: the batch dict of every pair problem, and optionally prior_qvec (n_pairs x 4) +
    prior_tvec (n_pairs x 3): the pose of camera 2 relative to camera 1, which switches the estimator to known-pose
    verification.
    """

    def __init__(self, ctx, batch):
        prior = None
        if not isinstance(batch, _PairProblem):
            prior = (batch.get("prior_qvec"), batch.get("prior_tvec"))
            if (prior[0] is None) != (prior[1] is None):
                raise ValueError("prior_qvec and prior_tvec go together")
        super().__init__(ctx, batch)
        if prior is not None and prior[0] is not None:
            self.d["prior_qvec"] = ctx.to_device(np.asarray(prior[0], dtype=np.float64).reshape(self.n_pairs, 4), np.float64)
            self.d["prior_tvec"] = ctx.to_device(np.asarray(prior[1], dtype=np.float64).reshape(self.n_pairs, 3), np.float64)
        self.has_prior = "prior_qvec" in self.d

    def estimate(self, qvec=None, tvec=None, E=None, timed=False, **options):
        """Run the kernels (pxr_two_view_geometry) with two_view_options(**options).  Returns the device arrays (qvec (n_pairs, 4),
        tvec (n_pairs, 3), E (n_pairs, 9), status, n_inliers, n_trials (n_pairs,) int32, inlier (n_matches,) uint8, err
        (n_matches,) float64).  qvec / tvec / E: host arrays the outputs start from -- rows of pairs without a pose keep them
        (default: NaN).  timed: also keep the kernels' HIP-event times in self.kernel_ms {"records", "compact", "hypotheses",
        "refine"} (milliseconds)."""
        prior = (self.d["prior_qvec"].ptr, self.d["prior_tvec"].ptr) if self.has_prior else (None, None)
        return self._estimate("pxr_two_view_geometry", options, ((qvec, 4), (tvec, 3), (E, 9)), 3, timed, prior)


class HomographyProblem(_PairProblem):
    """The pair batch of pxr_homography: the batch dict of every pair problem; a pose prior is not used."""

    def estimate(self, H=None, rot_qvec=None, timed=False, **options):
        """Run the kernels (pxr_homography) with homography_options(**options).  Returns the device arrays (H (n_pairs, 9),
        rot_qvec (n_pairs, 4), status, n_inliers, n_rot_inliers, n_trials (n_pairs,) int32, inlier (n_matches,) uint8, err
        (n_matches,) float64).  H / rot_qvec: host arrays the outputs start from -- rows of pairs without a homography keep them
        (default: NaN).  timed: also keep the kernels' HIP-event times in self.kernel_ms {"records", "compact", "hypotheses",
        "refine"} (milliseconds)."""
        return self._estimate("pxr_homography", options, ((H, 9), (rot_qvec, 4)), 4, timed)


class FundamentalProblem(_PairProblem):
    """The pair batch of pxr_fundamental: the batch dict of every pair problem.  The cameras are the ones the records are
    normalised with -- for an uncalibrated pair, conditioning transforms."""

    def estimate(self, F=None, timed=False, **options):
        """Run the kernels (pxr_fundamental) with fundamental_options(**options).  Returns the device arrays (F (n_pairs, 9),
        status, n_inliers, n_trials (n_pairs,) int32, inlier (n_matches,) uint8, err (n_matches,) float64).  F: a host array the
        output starts from -- rows of pairs without a fundamental matrix keep it (default: NaN).  timed: also keep the kernels'
        HIP-event times in self.kernel_ms {"records", "compact", "hypotheses", "refine"} (milliseconds)."""
        return self._estimate("pxr_fundamental", options, ((F, 9),), 3, timed)


MATCH_CONFS = {            # hloc's match_features confs for its NearestNeighbor matcher
    "NN-mutual": dict(ratio_threshold=0.0, distance_threshold=0.0, do_mutual_check=True),
    "NN-ratio": dict(ratio_threshold=0.8, distance_threshold=0.0, do_mutual_check=True),
    "NN-superpoint": dict(ratio_threshold=0.0, distance_threshold=0.7, do_mutual_check=True),
}


def match_options(ratio_threshold=0.0, distance_threshold=0.0, do_mutual_check=True):
    """pxr_match_options: a threshold <= 0 (or None) switches its test off; the defaults are hloc's "NN-mutual"."""
    return _lib.MatchOptions(float(ratio_threshold or 0.0), float(distance_threshold or 0.0), int(bool(do_mutual_check)), 0)


class DescriptorSet:
    """Device-resident descriptors of a set of images, as pxr_match_descriptors and pxr_vlad_aggregate take them: d_desc (n_total, D)
    float32, image_offsets (n_images + 1) on the host and d_offsets on the device.

    descriptors: a list of (n, D) float32 host arrays or DeviceArrays (one per image; n may be 0), or one (n_total, D) array
    with image_offsets (n_images + 1), which is used in place when it is a DeviceArray (a DeviceArray inside a list is staged
    through the host).  Every image is uploaded once."""

    def __init__(self, ctx, descriptors, image_offsets=None):
        self.ctx = ctx
        if image_offsets is not None:
            desc = descriptors if isinstance(descriptors, DeviceArray) else np.ascontiguousarray(descriptors, dtype=np.float32)
            if len(desc.shape) != 2:
                raise ValueError("descriptors must be (n_total, D)")
            offsets = _csr_offsets(image_offsets, "image_offsets", "n_images")
            self.dim = int(desc.shape[1])
            self.d_desc = desc if isinstance(desc, DeviceArray) else ctx.to_device(desc, np.float32)
        else:
            shapes = [tuple(d.shape) for d in descriptors]
            if any(len(s) != 2 for s in shapes) or len({s[1] for s in shapes}) > 1:
                raise ValueError("descriptors must be (n, D) arrays of one D")
            self.dim = int(shapes[0][1]) if shapes else 1
            offsets = np.concatenate([[0], np.cumsum([s[0] for s in shapes])]).astype(np.int64)
            self.d_desc = ctx.empty((int(offsets[-1]), self.dim), np.float32)
            row = self.dim * 4
            for d, first in zip(descriptors, offsets[:-1]):
                if d.shape[0] == 0:
                    continue
                dst = C.c_void_p(self.d_desc.ptr.value + int(first) * row)
                h = np.ascontiguousarray(d.download() if isinstance(d, DeviceArray) else d, dtype=np.float32)
                check(ctx.lib.pxr_memcpy_h2d(ctx.handle, dst, h.ctypes.data, h.nbytes), "pxr_memcpy_h2d")
        self.image_offsets = offsets
        self.n_images = len(offsets) - 1
        self.n_total = int(self.d_desc.shape[0])
        self.d_offsets = ctx.to_device(offsets, np.int64)


class MatchProblem:
    """Device-resident descriptors of a set of images and a list of image pairs (pxr_match_descriptors).

    descriptors: a list of (n, D) float32 host arrays or DeviceArrays (one per image; n may be 0), or one (n_total, D) array
    with image_offsets (n_images + 1), which is used in place when it is a DeviceArray (a DeviceArray inside a list is staged
    through the host).  pairs: (n_pairs, 2) image indices.  Every image is uploaded once, however many pairs name it.
    keypoints (run_guided only): per image an (n, 2) float64 array in the frame of the pairs' models, or one (n_total, 2) array
    (a DeviceArray is used in place), row-aligned with the descriptors.
    """

    def __init__(self, ctx, descriptors, pairs, image_offsets=None, keypoints=None):
        self.ctx = ctx
        d = descriptors if isinstance(descriptors, DescriptorSet) else DescriptorSet(ctx, descriptors, image_offsets)
        self.dim, self.d_desc, self.image_offsets, self.n_images, self.n_total, self.d_offsets = (d.dim, d.d_desc, d.image_offsets, d.n_images,
                                                                                                   d.n_total, d.d_offsets)
        offsets = self.image_offsets
        self.pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        self.n_pairs = len(self.pairs)
        counts = np.diff(offsets)
        first = self.pairs[:, 0]
        in_range = (first >= 0) & (first < self.n_images)          # an index out of range is the library's to report
        rows = np.zeros(self.n_pairs, dtype=np.int64)
        rows[in_range] = counts[first[in_range]]
        self.pair_offsets = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
        self.d_pairs = ctx.to_device(self.pairs, np.int32)
        self.d_pair_offsets = ctx.to_device(self.pair_offsets, np.int64)
        self.kernel_ms = None
        self.d_xy = None
        if isinstance(keypoints, DeviceArray):
            self.d_xy = keypoints
        elif keypoints is not None:
            if not isinstance(keypoints, np.ndarray):
                keypoints = [np.asarray(k, dtype=np.float64).reshape(-1, 2) for k in keypoints]
                keypoints = np.concatenate(keypoints) if keypoints else np.empty((0, 2))
            self.d_xy = ctx.to_device(np.asarray(keypoints, dtype=np.float64).reshape(-1, 2), np.float64)
        if self.d_xy is not None and tuple(self.d_xy.shape) != (self.n_total, 2):
            raise ValueError("keypoints must hold one (x, y) per descriptor: (%d, 2), not %s" % (self.n_total, tuple(self.d_xy.shape)))

    def _outputs(self, out):
        ctx, n_rows = self.ctx, int(self.pair_offsets[-1])
        return out if out is not None else (ctx.empty((n_rows,), np.int32), ctx.empty((n_rows,), np.float32),
                                            ctx.empty((self.n_pairs,), np.int32))

    def run_guided(self, kinds, models, thresholds, timed=False, out=None, **options):
        """Run the guided kernels (pxr_match_guided): per pair a kind (_lib.GUIDE_EPIPOLAR / GUIDE_HOMOGRAPHY), a 3 x 3 model and a
        threshold in the keypoints' units; only candidates the model admits compete.  Needs `keypoints`.  Returns what run returns;
        timed keeps self.kernel_ms {"records", "tiles", "columns", "mutual"}."""
        ctx = self.ctx
        if self.d_xy is None:
            raise ValueError("run_guided needs the keypoints of the images (MatchProblem(..., keypoints=...))")
        kinds = np.ascontiguousarray(kinds, dtype=np.int32).reshape(-1)
        models = np.ascontiguousarray(models, dtype=np.float64).reshape(-1, 9)
        thresholds = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
        if not (len(kinds) == len(models) == len(thresholds) == self.n_pairs):
            raise ValueError("kinds, models and thresholds must hold one entry per pair (%d)" % self.n_pairs)
        opts = match_options(**options)
        d_m, d_s, d_n = self._outputs(out)
        d_kind, d_model, d_thr = ctx.to_device(kinds, np.int32), ctx.to_device(models, np.float64), ctx.to_device(thresholds, np.float64)
        args = (ctx.handle, self.n_images, self.d_offsets.ptr, self.n_total, self.dim, self.d_desc.ptr, self.d_xy.ptr, self.n_pairs,
                self.d_pairs.ptr, self.d_pair_offsets.ptr, d_kind.ptr, d_model.ptr, d_thr.ptr, C.byref(opts), d_m.ptr, d_s.ptr, d_n.ptr)
        self.kernel_ms = _launch(ctx, "pxr_match_guided", args, ("records", "tiles", "columns", "mutual"), timed) or self.kernel_ms
        return d_m, d_s, d_n

    def run(self, timed=False, out=None, **options):
        """Run the kernels (pxr_match_descriptors) with match_options(**options).  Returns the device arrays (matches0
        (n_rows,) int32, scores0 (n_rows,) float32, n_matches (n_pairs,) int32); pair p owns rows [pair_offsets[p],
        pair_offsets[p + 1]).  out: the three device arrays to write into.  timed: also keep the kernels' HIP-event times in
        self.kernel_ms {"tiles", "columns", "mutual"} (milliseconds)."""
        ctx = self.ctx
        opts = match_options(**options)
        d_m, d_s, d_n = self._outputs(out)
        args = (ctx.handle, self.n_images, self.d_offsets.ptr, self.n_total, self.dim, self.d_desc.ptr, self.n_pairs, self.d_pairs.ptr,
                self.d_pair_offsets.ptr, C.byref(opts), d_m.ptr, d_s.ptr, d_n.ptr)
        self.kernel_ms = _launch(ctx, "pxr_match_descriptors", args, ("tiles", "columns", "mutual"), timed) or self.kernel_ms
        return d_m, d_s, d_n


def image_major_transpose(obs_image, n_images):
    """The image-major transpose of a track-major observation list: (image_obs_offsets (n_images + 1,) int64, image_obs (n_obs,)
    int64) -- image i owns the observation indices image_obs[offsets[i]:offsets[i + 1]], ascending."""
    obs_image = np.asarray(obs_image, dtype=np.int64).reshape(-1)
    if len(obs_image) and (obs_image.min() < 0 or obs_image.max() >= n_images):
        raise ValueError("an observation names an image outside [0, %d)" % n_images)
    offsets = np.zeros(n_images + 1, dtype=np.int64)
    np.cumsum(np.bincount(obs_image, minlength=n_images), out=offsets[1:])
    return offsets, np.argsort(obs_image, kind="stable").astype(np.int64)


def restrict_tracks(track_offsets, obs_image, registered):
    """The track CSR that keeps only the observations in registered images (registered: (n_images,) bool).  The track count is
    unchanged -- a track may become empty -- so track indices stay what they are.  Returns (track_offsets (n_tracks + 1,) int64,
    obs_index: the kept observations as indices into the full list, ascending)."""
    keep = np.asarray(registered, dtype=bool)[np.asarray(obs_image, dtype=np.int64)]
    before = np.zeros(len(keep) + 1, dtype=np.int64)
    np.cumsum(keep, out=before[1:])
    return before[np.asarray(track_offsets, dtype=np.int64)], np.flatnonzero(keep).astype(np.int64)


class MapperScene:
    """The flat arrays of a scene that an incremental mapper keeps on the device for all of its rounds (pxr_mapper_visibility):
    every observation of every track with its image and keypoint, the image-major transpose, images, cameras and their sizes.

    problem: the dict of TriangulationProblem (track_offsets, obs_image, obs_xy, image_camera, cam_model, cam_params; qvec / tvec
    are not needed) plus cam_size (n_cameras x 2: width, height).  ctx None: host arrays only (restricted_tracks works,
    visibility does not).
    """

    def __init__(self, ctx, problem):
        self.ctx = ctx
        g = problem
        self.track_offsets = _csr_offsets(g["track_offsets"], "track_offsets", "n_tracks")
        self.n_tracks = len(self.track_offsets) - 1
        self.obs_image = np.ascontiguousarray(np.asarray(g["obs_image"]).reshape(-1), dtype=np.int32)
        self.n_obs = len(self.obs_image)
        self.obs_xy = np.ascontiguousarray(g["obs_xy"], dtype=np.float64).reshape(-1, 2)
        if len(self.obs_xy) != self.n_obs:
            raise ValueError("obs_xy must hold one keypoint per observation")
        self.image_camera = np.ascontiguousarray(g["image_camera"], dtype=np.int32).reshape(-1)
        self.n_images = len(self.image_camera)
        self.cam_model = np.ascontiguousarray(g["cam_model"], dtype=np.int32).reshape(-1)
        self.n_cameras = len(self.cam_model)
        self.cam_size = np.ascontiguousarray(g["cam_size"], dtype=np.int32).reshape(-1, 2)
        if len(self.cam_size) != self.n_cameras:
            raise ValueError("cam_size must hold one (width, height) per camera")
        self.obs_track = np.repeat(np.arange(self.n_tracks, dtype=np.int64), np.diff(self.track_offsets))
        if len(self.obs_track) != self.n_obs:
            raise ValueError("track_offsets must end at the number of observations")
        self.image_obs_offsets, self.image_obs = image_major_transpose(self.obs_image, self.n_images)
        self.kernel_ms = None
        if ctx is None:
            return
        self.d = {
            "track_offsets": ctx.to_device(self.track_offsets, np.int64),
            "obs_image": ctx.to_device(self.obs_image, np.int32),
            "obs_xy": ctx.to_device(self.obs_xy, np.float64),
            "obs_track": ctx.to_device(self.obs_track, np.int64),
            "image_obs_offsets": ctx.to_device(self.image_obs_offsets, np.int64),
            "image_obs": ctx.to_device(self.image_obs, np.int64),
            "image_camera": ctx.to_device(self.image_camera, np.int32),
            "cam_model": ctx.to_device(self.cam_model, np.int32),
            "cam_params": ctx.to_device(_padded_cam_params(g["cam_params"], self.n_cameras), np.float64),
            "cam_size": ctx.to_device(self.cam_size, np.int32),
        }
        d = self.d
        self.view = _lib.TriView(self.n_tracks, d["track_offsets"].ptr, self.n_obs, d["obs_image"].ptr, d["obs_xy"].ptr,
                                 self.n_images, d["image_camera"].ptr, None, None, self.n_cameras, d["cam_model"].ptr,
                                 d["cam_params"].ptr)

    def restricted_tracks(self, registered):
        """restrict_tracks on this scene, as the problem dict entries of TriangulationProblem: track_offsets, obs_image, obs_xy,
        and obs_index (the kept observations as indices into the scene's list)."""
        offsets, obs_index = restrict_tracks(self.track_offsets, self.obs_image, registered)
        return dict(track_offsets=offsets, obs_index=obs_index, obs_image=self.obs_image[obs_index], obs_xy=self.obs_xy[obs_index])

    def visibility(self, xyz, status, image_mask, levels=6, timed=False, out=None):
        """Run the kernels (pxr_mapper_visibility).  xyz (n_tracks, 3) float64 and status (n_tracks,) int32: device arrays as
        TriangulationProblem.triangulate returns them; image_mask (n_images,) host array, non-zero = candidate.  Returns a dict
        of device arrays: n_visible (n_images,) int32, score (n_images,) int64, corr_offsets (n_images + 1,) int64, corr_obs
        (n_obs,) int64, corr_xy (n_obs, 2), corr_xyz (n_obs, 3) -- the first n_corr rows are written -- and n_corr (int).
        out: a dict of these six device arrays to write into.
        timed: also keep the kernels' HIP-event times in self.kernel_ms {"check", "count", "scan", "write"} (milliseconds)."""
        ctx, d = self.ctx, self.d
        mask = np.ascontiguousarray(image_mask, dtype=np.uint8).reshape(-1)
        if len(mask) != self.n_images:
            raise ValueError("image_mask must hold one entry per image")
        if tuple(xyz.shape) != (self.n_tracks, 3) or tuple(status.shape) != (self.n_tracks,):
            raise ValueError("xyz and status must hold one row per track")
        d_mask = ctx.to_device(mask, np.uint8)
        out = dict(out) if out is not None else dict(
            n_visible=ctx.empty((self.n_images,), np.int32), score=ctx.empty((self.n_images,), np.int64),
            corr_offsets=ctx.empty((self.n_images + 1,), np.int64), corr_obs=ctx.empty((max(self.n_obs, 1),), np.int64),
            corr_xy=ctx.empty((max(self.n_obs, 1), 2), np.float64), corr_xyz=ctx.empty((max(self.n_obs, 1), 3), np.float64))
        n_corr = C.c_int64()
        args = (ctx.handle, C.byref(self.view), d["obs_track"].ptr, d["image_obs_offsets"].ptr, d["image_obs"].ptr, xyz.ptr, status.ptr,
                d_mask.ptr, d["cam_size"].ptr, int(levels), out["n_visible"].ptr, out["score"].ptr, out["corr_offsets"].ptr,
                out["corr_obs"].ptr, out["corr_xy"].ptr, out["corr_xyz"].ptr, C.byref(n_corr))
        self.kernel_ms = _launch(ctx, "pxr_mapper_visibility", args, ("check", "count", "scan", "write"), timed) or self.kernel_ms
        out["n_corr"] = int(n_corr.value)
        return out


# ---- batched map localization ----------------------------------------------------------------------------------------------------
def _on_device(ctx, array, dtype, shape):
    """`array` as a DeviceArray of `dtype` and `shape` (-1: any): a DeviceArray is used in place, a host array is uploaded."""
    if not isinstance(array, DeviceArray):
        array = ctx.to_device(np.ascontiguousarray(array, dtype=dtype).reshape(shape), dtype)
    if array.dtype != np.dtype(dtype) or len(array.shape) != len(shape) or any(s >= 0 and s != t for s, t in zip(shape, array.shape)):
        raise ValueError("expected a %s array of shape %s, not %s %s" % (np.dtype(dtype), shape, array.dtype, array.shape))
    return array


class CovisibilityGraph:
    """The covisibility counts of a map on the device (pxr_covisibility): count[i][j] = over the tracks, the ordered pairs of
    observations in images i != j -- hloc's count, symmetric, diagonal 0.

    track_offsets (n_tracks + 1), obs_image (n_obs): the tracks as TriangulationProblem takes them; track_mask (n_tracks) or None:
    the tracks that count.  At most _lib.MAX_COVIS_IMAGES images (the matrix is dense).
    timed keeps the kernels' HIP-event times in self.kernel_ms {"check", "count", "topk"} (milliseconds)."""

    def __init__(self, ctx, track_offsets, obs_image, n_images, track_mask=None, timed=False):
        self.ctx = ctx
        offsets = _csr_offsets(track_offsets, "track_offsets", "n_tracks")
        self.n_tracks, self.n_images = len(offsets) - 1, int(n_images)
        obs_image = np.ascontiguousarray(np.asarray(obs_image).reshape(-1), dtype=np.int32)
        self.n_obs = len(obs_image)
        self.d_track_offsets, self.d_obs_image = ctx.to_device(offsets, np.int64), ctx.to_device(obs_image, np.int32)
        self.d_track_mask = None
        if track_mask is not None:
            mask = np.ascontiguousarray(track_mask, dtype=np.uint8).reshape(-1)
            if len(mask) != self.n_tracks:
                raise ValueError("track_mask must hold one entry per track")
            self.d_track_mask = ctx.to_device(mask, np.uint8)
        if self.n_images > _lib.MAX_COVIS_IMAGES:
            raise ValueError("%d map images, more than %d: the covisibility matrix is dense" % (self.n_images, _lib.MAX_COVIS_IMAGES))
        self.d_count = ctx.empty((self.n_images, self.n_images), np.int32)
        self.kernel_ms = None
        self._run(1, None, None, None, timed)

    def _run(self, num_matched, d_index, d_count, d_n, timed):
        ctx = self.ctx
        ptr = lambda a: None if a is None else a.ptr                                           # noqa: E731
        args = (ctx.handle, self.n_images, self.n_tracks, self.d_track_offsets.ptr, self.n_obs, self.d_obs_image.ptr, ptr(self.d_track_mask),
                int(num_matched), self.d_count.ptr, ptr(d_index), ptr(d_count), ptr(d_n))
        self.kernel_ms = _launch(ctx, "pxr_covisibility", args, ("check", "count", "topk"), timed) or self.kernel_ms

    def counts(self):
        """The (n_images, n_images) int32 matrix, downloaded."""
        return self.d_count.download()

    def topk(self, num_matched, timed=False):
        """Per image its min(num_matched, partners with a positive count) best partners by (count descending, index ascending).
        Returns the device arrays (index (n_images, num_matched) int32, -1 where a row ends; count, the same shape, 0 there;
        n (n_images,) int32).  The counts are computed again by the same call: they come out the same."""
        ctx, K = self.ctx, int(num_matched)
        if not 1 <= K <= _lib.MAX_COVIS_MATCHED:
            raise ValueError("num_matched = %d outside [1, %d]" % (K, _lib.MAX_COVIS_MATCHED))
        out = ctx.empty((self.n_images, K), np.int32), ctx.empty((self.n_images, K), np.int32), ctx.empty((self.n_images,), np.int32)
        self._run(K, *out, timed)
        return out

    def clusters(self, ret_offsets, ret, timed=False):
        """The covisibility clusters of every query's retrieved images (pxr_covisibility_clusters): query q owns
        ret[ret_offsets[q]:ret_offsets[q + 1]], map image indices in retrieval rank order, at most _lib.MAX_LOC_ENTRIES of them.
        Returns the device arrays (cluster (n_ret,) int32: the number of every entry's cluster, clusters numbered by (size
        descending, first member ascending); n_clusters (n_queries,) int32).  timed keeps self.kernel_ms {"check", "clusters"}."""
        ctx = self.ctx
        offsets = _csr_offsets(ret_offsets, "ret_offsets", "n_queries")
        ret = np.ascontiguousarray(np.asarray(ret).reshape(-1), dtype=np.int32)
        n_q = len(offsets) - 1
        d_off, d_ret = ctx.to_device(offsets, np.int64), ctx.to_device(ret, np.int32)
        d_cluster, d_n = ctx.empty((len(ret),), np.int32), ctx.empty((n_q,), np.int32)
        args = (ctx.handle, self.n_images, self.d_count.ptr, n_q, d_off.ptr, len(ret), d_ret.ptr, d_cluster.ptr, d_n.ptr)
        self.kernel_ms = _launch(ctx, "pxr_covisibility_clusters", args, ("check", "clusters"), timed) or self.kernel_ms
        return d_cluster, d_n


class LocalizationPairs:
    """The gather between matching and absolute pose for a batch of localization problems (pxr_localization_pairs).

    match: the MatchProblem whose pairs are (query, database image) -- its pair list, pair offsets and image offsets are used
    where they live on the device.  kp_xy (n_total, 2) float64: the keypoint of every descriptor row; kp_point (n_total,) int64:
    the row of xyz that keypoint observes, negative = none; xyz (n_points, 3).  Each a host array or a DeviceArray (used in place).
    """

    def __init__(self, ctx, match, kp_xy, kp_point, xyz):
        self.ctx, self.match = ctx, match
        self.d_kp_xy = _on_device(ctx, kp_xy, np.float64, (match.n_total, 2))
        self.d_kp_point = _on_device(ctx, kp_point, np.int64, (match.n_total,))
        self.d_xyz = _on_device(ctx, xyz, np.float64, (-1, 3))
        self.n_points = int(self.d_xyz.shape[0])
        self.kernel_ms = None

    def gather(self, matches0, problem_offsets, problem_pair, timed=False, out=None):
        """matches0: the device array MatchProblem.run returned.  Problem p owns the entries problem_pair[problem_offsets[p]:
        problem_offsets[p + 1]], indices into the match's pair list in visiting order, all of one query, at most
        _lib.MAX_LOC_ENTRIES.  Returns a dict of device arrays: corr_offsets (n_problems + 1,) int64, corr_kp (capacity,) int32,
        corr_point (capacity,) int64, corr_xy (capacity, 2), corr_xyz (capacity, 3) -- the first n_corr rows are written, per
        problem by ascending query keypoint and, within a keypoint, by first appearance -- and n_corr (int).  corr_offsets, n_corr,
        corr_xy and corr_xyz go into AbsolutePoseProblem.from_device as they are.  out: a dict of the five arrays to write into.
        timed keeps the kernels' HIP-event times in self.kernel_ms {"count", "scan", "write"} (milliseconds)."""
        ctx, m = self.ctx, self.match
        offsets = _csr_offsets(problem_offsets, "problem_offsets", "n_problems")
        entries = np.ascontiguousarray(np.asarray(problem_pair).reshape(-1), dtype=np.int32)
        n_p = len(offsets) - 1
        rows = np.diff(m.pair_offsets)
        ok = (entries >= 0) & (entries < m.n_pairs)              # an index out of range is the library's to report
        cap = max(int(rows[entries[ok]].sum()), 1)
        out = dict(out) if out is not None else dict(
            corr_offsets=ctx.empty((n_p + 1,), np.int64), corr_kp=ctx.empty((cap,), np.int32), corr_point=ctx.empty((cap,), np.int64),
            corr_xy=ctx.empty((cap, 2), np.float64), corr_xyz=ctx.empty((cap, 3), np.float64))
        d_off, d_ent = ctx.to_device(offsets, np.int64), ctx.to_device(entries, np.int32)
        n_corr = C.c_int64()
        args = (ctx.handle, n_p, d_off.ptr, len(entries), d_ent.ptr, m.n_pairs, m.d_pairs.ptr, m.d_pair_offsets.ptr,
                int(m.pair_offsets[-1]), matches0.ptr, m.n_images, m.d_offsets.ptr, m.n_total, self.d_kp_xy.ptr, self.d_kp_point.ptr,
                self.n_points, self.d_xyz.ptr, out["corr_offsets"].ptr, out["corr_kp"].ptr, out["corr_point"].ptr, out["corr_xy"].ptr,
                out["corr_xyz"].ptr, C.byref(n_corr))
        self.kernel_ms = _launch(ctx, "pxr_localization_pairs", args, ("count", "scan", "write"), timed) or self.kernel_ms
        out["n_corr"] = int(n_corr.value)
        return out


# ---- SIFT ------------------------------------------------------------------------------------------------------------------------
def sift_options(**options):
    """pxr_sift_options: the library's defaults (pxr_sift_default_options) with `options` over them.  peak_threshold < 0 (the
    default) stands for 0.02 / octave_resolution.  An unknown name is a ValueError."""
    o = _lib.SiftOptions()
    _lib.load().pxr_sift_default_options(C.byref(o))
    names = {k: t for k, t in _lib.SiftOptions._fields_ if k != "reserved"}
    for k, v in options.items():
        if k not in names:
            raise ValueError("unknown SIFT option %r (known: %s)" % (k, ", ".join(sorted(names))))
        setattr(o, k, float(v) if names[k] is C.c_double else int(v))
    return o


def _rows(array, n):
    """The first n rows of a device array, as the same buffer under a smaller shape."""
    array.shape = (int(n),) + tuple(array.shape[1:])
    array.nbytes = int(np.prod(array.shape, dtype=np.int64)) * array.dtype.itemsize
    return array


class SiftPyramid:
    """The Gaussian scale space of one grey image on the device (pxr_sift_pyramid), and the stages that read it.

    grey: (h, w) uint8 (value / 255) or float32, host array or device tensor.  options: sift_options(**options).
    kernel_ms collects the HIP-event times of the timed calls {"pyramid", "count", "scan", "write", "orient", "emit", "describe"}."""

    def __init__(self, ctx, grey, timed=False, **options):
        self.ctx = ctx
        self.options = sift_options(**options)
        img = _grey_on_device(ctx, grey)
        self.h, self.w = img.h, img.w
        n_oct, sizes, offsets = C.c_int32(), np.zeros((_lib.SIFT_MAX_OCTAVES, 2), np.int32), np.zeros(_lib.SIFT_MAX_OCTAVES, np.int64)
        check(ctx.lib.pxr_sift_pyramid_layout(self.h, self.w, C.byref(self.options), C.byref(n_oct), sizes.ctypes.data,
                                              offsets.ctypes.data), "pxr_sift_pyramid_layout")
        nbytes = C.c_int64()
        check(ctx.lib.pxr_sift_pyramid_bytes(self.h, self.w, C.byref(self.options), C.byref(nbytes)), "pxr_sift_pyramid_bytes")
        self.n_octaves, self.sizes, self.offsets = int(n_oct.value), sizes[:n_oct.value], offsets[:n_oct.value]
        self.levels = self.options.octave_resolution + 3
        self.d_pyramid = ctx.empty((max(nbytes.value // 4, 1),), np.float32)
        self.kernel_ms = {}
        args = (ctx.handle, img.ptr, img.dtype, self.h, self.w, C.byref(self.options), self.d_pyramid.ptr)
        self.kernel_ms.update(_launch(ctx, "pxr_sift_pyramid", args, ("pyramid",), timed) or {})
        ctx.sync()                                      # (the image may be a temporary upload)

    def level(self, k, s):
        """Plane (octave index k, level s) as a host (h_k, w_k) float32 array."""
        h, w = (int(v) for v in self.sizes[k])
        flat = self.d_pyramid.download()
        first = int(self.offsets[k]) + s * h * w
        return flat[first:first + h * w].reshape(h, w)

    def octaves(self):
        """[octave: (S + 3, h_k, w_k) float32] on the host."""
        flat = self.d_pyramid.download()
        return [flat[int(o):int(o) + self.levels * int(h) * int(w)].reshape(self.levels, int(h), int(w))
                for o, (h, w) in zip(self.offsets, self.sizes)]

    def detect(self, capacity=None, timed=False, out=None):
        """pxr_sift_detect.  Returns (keypoints (n, 4) float64 x, y, sigma, theta in pixel indices, record (n, 4) int32 o, s, xi,
        yi, response (n,) float32) as device arrays of the rows written, and the number found.  capacity=None: a first guess, and
        a second run when more were found; out: the three device arrays (capacity rows) to write into."""
        ctx = self.ctx
        guess = capacity is None
        cap = max(4096, self.h * self.w // 32) if guess else int(capacity)
        while True:
            kp, rec, resp = out if out is not None else (ctx.empty((max(cap, 0), 4), np.float64), ctx.empty((max(cap, 0), 4), np.int32),
                                                         ctx.empty((max(cap, 0),), np.float32))
            found = C.c_int64(-1)
            args = (ctx.handle, self.d_pyramid.ptr, self.h, self.w, C.byref(self.options), cap, kp.ptr, rec.ptr, resp.ptr, C.byref(found))
            self.kernel_ms.update(_launch(ctx, "pxr_sift_detect", args, ("count", "scan", "write", "orient", "emit"), timed) or {})
            if not guess or found.value <= cap or out is not None:
                break
            cap = int(found.value)
        n = min(int(found.value), cap)
        if out is None:
            kp, rec, resp = _rows(kp, n), _rows(rec, n), _rows(resp, n)
        return kp, rec, resp, int(found.value)

    def gather(self, keypoints, response=None, index=None, offset=0.0):
        """pxr_sift_gather: rows `index` (host int64 array; None: all) of detect()'s arrays as device arrays (keypoints (n, 4),
        xy (n, 2) + offset, scales (n,), orientations (n,), scores (n,) or None)."""
        ctx = self.ctx
        n_in = int(keypoints.shape[0])
        d_index = None if index is None else ctx.to_device(np.ascontiguousarray(index, dtype=np.int64).reshape(-1), np.int64)
        n = n_in if index is None else int(d_index.shape[0])
        kp, xy, sc, th = ctx.empty((n, 4), np.float64), ctx.empty((n, 2), np.float64), ctx.empty((n,), np.float64), ctx.empty((n,), np.float64)
        scores = ctx.empty((n,), np.float32) if response is not None else None
        check(ctx.lib.pxr_sift_gather(ctx.handle, n, n_in, d_index.ptr if d_index is not None else None, keypoints.ptr,
                                      response.ptr if response is not None else None, float(offset), kp.ptr, xy.ptr, sc.ptr, th.ptr,
                                      scores.ptr if scores is not None else None), "pxr_sift_gather")
        ctx.sync()                                      # (d_index may go out of scope)
        return kp, xy, sc, th, scores

    def describe(self, keypoints, timed=False, out=None):
        """pxr_sift_describe of (n, 4) x, y, sigma, theta (pixel indices; a device array is used in place).  Returns the device
        arrays (descriptors (n, 128) float32, valid (n,) uint8)."""
        ctx = self.ctx
        kp = keypoints if isinstance(keypoints, DeviceArray) else ctx.to_device(np.asarray(keypoints, dtype=np.float64).reshape(-1, 4), np.float64)
        n = int(kp.shape[0])
        desc, valid = out if out is not None else (ctx.empty((n, 128), np.float32), ctx.empty((n,), np.uint8))
        args = (ctx.handle, self.d_pyramid.ptr, self.h, self.w, C.byref(self.options), n, kp.ptr, desc.ptr, valid.ptr)
        self.kernel_ms.update(_launch(ctx, "pxr_sift_describe", args, ("describe",), timed) or {})
        ctx.sync()
        return desc, valid


def _device_descriptors(ctx, descriptors, image_offsets=None):
    """A DescriptorSet of a list of (n, D) arrays, one per image, or of one (n_total, D) array with image_offsets (None: one image)."""
    flat = isinstance(descriptors, (DeviceArray, np.ndarray))
    if flat and image_offsets is None:
        image_offsets = [0, int(descriptors.shape[0])]
    return DescriptorSet(ctx, descriptors, image_offsets)


class VladVocabulary:
    """The centroids of a VLAD vocabulary on the device (pxr_vocab_train, pxr_vlad_aggregate).

    centroids: (K, D) float32, a host array or a DeviceArray (used in place).  After train(): counts (K,) int32, the rows of the
    training set per centroid in the last iteration, and n_empty, the zeros among them."""

    def __init__(self, ctx, centroids):
        self.ctx = ctx
        self.d_centroids = centroids if isinstance(centroids, DeviceArray) else ctx.to_device(np.asarray(centroids), np.float32)
        if len(self.d_centroids.shape) != 2 or self.d_centroids.dtype != np.float32:
            raise ValueError("centroids must be (K, D) float32")
        self.n_clusters, self.dim = (int(s) for s in self.d_centroids.shape)
        self.counts = self.n_empty = self.kernel_ms = None

    @classmethod
    def train(cls, ctx, descriptors, n_clusters=64, n_iterations=10, max_train=262144, timed=False):
        """Spherical k-means over the descriptors (a list of (n, D) arrays or one (n_total, D) array): a function of the input
        alone, no random state.  timed: kernel_ms {"gather", "assign", "accumulate", "update"}, summed over the iterations."""
        d = _device_descriptors(ctx, descriptors)
        K = int(n_clusters)
        d_c, d_cnt = ctx.empty((max(K, 0), d.dim), np.float32), ctx.empty((max(K, 0),), np.int32)
        n_empty = C.c_int32(-1)
        args = (ctx.handle, d.n_total, d.dim, d.d_desc.ptr, K, int(n_iterations), int(max_train), d_c.ptr, d_cnt.ptr, C.byref(n_empty))
        ms = _launch(ctx, "pxr_vocab_train", args, ("gather", "assign", "accumulate", "update"), timed)
        voc = cls(ctx, d_c)
        voc.counts, voc.n_empty, voc.kernel_ms = d_cnt.download(), int(n_empty.value), ms
        return voc

    @property
    def centroids(self):
        return self.d_centroids.download()

    def aggregate(self, descriptors_by_image, image_offsets=None, timed=False, details=False):
        """The VLAD global descriptors of a list of (n, D) arrays (or of one (n_total, D) array with image_offsets): a device
        array (n_images, K * D) float32.  details: also the device arrays assign (n_total,) int32 and counts (n_images, K) int32.
        timed: kernel_ms {"assign", "accumulate", "finalise"}."""
        ctx = self.ctx
        d = _device_descriptors(ctx, descriptors_by_image, image_offsets)
        if d.n_total and d.dim != self.dim:
            raise ValueError("descriptors of dimension %d for a vocabulary of dimension %d" % (d.dim, self.dim))
        g = ctx.empty((d.n_images, self.n_clusters * self.dim), np.float32)
        d_a = ctx.empty((d.n_total,), np.int32) if details else None
        d_n = ctx.empty((d.n_images, self.n_clusters), np.int32) if details else None
        args = (ctx.handle, d.n_images, d.d_offsets.ptr, d.n_total, self.dim, d.d_desc.ptr, self.n_clusters, self.d_centroids.ptr, g.ptr,
                d_a.ptr if details else None, d_n.ptr if details else None)
        self.kernel_ms = _launch(ctx, "pxr_vlad_aggregate", args, ("assign", "accumulate", "finalise"), timed) or self.kernel_ms
        ctx.sync()                                      # (the uploaded descriptors may go out of scope)
        return (g, d_a, d_n) if details else g


def retrieval_topk(ctx, query, db, num_matched, query_self=None, mask=None, min_score=None, timed=False):
    """pxr_retrieval_topk: per row of query (n_query, Dg) its num_matched most similar rows of db (n_db, Dg), by (similarity
    descending, index ascending).  query / db: float32 host arrays or DeviceArrays (one object for both: uploaded once).
    query_self (n_query,) int32: the db row that is the query itself (-1: none), never returned; mask (n_query, n_db): 0 = excluded;
    min_score: the smallest similarity kept.  Returns the device arrays (top_index (n_query, num_matched) int32 padded with -1,
    top_sim float32 padded with 0, n_found (n_query,) int32), and with timed also {"similarity", "select"} in milliseconds."""
    d_q = query if isinstance(query, DeviceArray) else ctx.to_device(np.asarray(query), np.float32)
    d_db = d_q if db is query else (db if isinstance(db, DeviceArray) else ctx.to_device(np.asarray(db), np.float32))
    if len(d_q.shape) != 2 or len(d_db.shape) != 2 or d_q.shape[1] != d_db.shape[1]:
        raise ValueError("query and db must be (n, Dg) arrays of one Dg")
    nq, ndb, k = int(d_q.shape[0]), int(d_db.shape[0]), int(num_matched)
    d_self = None if query_self is None else ctx.to_device(np.asarray(query_self).reshape(-1), np.int32)
    d_mask = None if mask is None else ctx.to_device(np.asarray(mask).astype(bool).reshape(-1), np.uint8)
    if (d_self is not None and d_self.shape[0] != nq) or (d_mask is not None and d_mask.shape[0] != nq * ndb):
        raise ValueError("query_self must be (n_query,) and mask (n_query, n_db)")
    top, sim, found = ctx.empty((nq, max(k, 0)), np.int32), ctx.empty((nq, max(k, 0)), np.float32), ctx.empty((nq,), np.int32)
    args = (ctx.handle, nq, ndb, int(d_q.shape[1]), d_q.ptr, d_db.ptr, d_self.ptr if d_self is not None else None,
            d_mask.ptr if d_mask is not None else None, k, float("inf") if min_score is None else float(min_score), top.ptr, sim.ptr, found.ptr)
    ms = _launch(ctx, "pxr_retrieval_topk", args, ("similarity", "select"), timed)
    ctx.sync()                                          # (the uploaded arrays may go out of scope)
    return (top, sim, found, ms) if timed else (top, sim, found)


def _device_cloud(ctx, xyz, name):
    """A cloud as pxr_cloud_nearest takes it: (n, 3) float64 on the device.  A DeviceArray is used in place."""
    d = xyz if isinstance(xyz, DeviceArray) else ctx.to_device(np.asarray(xyz, dtype=np.float64).reshape(-1, 3), np.float64)
    if len(d.shape) != 2 or d.shape[1] != 3 or d.dtype != np.float64:
        raise ValueError("%s must be (n, 3) float64" % name)
    return d


def cloud_nearest(ctx, ref, query, max_dist, timed=False):
    """pxr_cloud_nearest: per row of query (n_query, 3) the nearest row of ref (n_ref, 3) within max_dist, ties to the lowest
    index -- the brute-force search bit for bit.  ref / query: float64 host arrays or DeviceArrays (one object for both:
    uploaded once).  Returns the device arrays (index (n_query,) int32, -1 without a candidate; dist2 (n_query,) float64, +inf
    without one), and with timed also {"grid", "query"} in milliseconds."""
    d_r = _device_cloud(ctx, ref, "ref")
    d_q = d_r if query is ref else _device_cloud(ctx, query, "query")
    nq = int(d_q.shape[0])
    index, dist2 = ctx.empty((nq,), np.int32), ctx.empty((nq,), np.float64)
    args = (ctx.handle, int(d_r.shape[0]), d_r.ptr, nq, d_q.ptr, float(max_dist), index.ptr, dist2.ptr)
    ms = _launch(ctx, "pxr_cloud_nearest", args, ("grid", "query"), timed)
    ctx.sync()                                          # (the uploaded arrays may go out of scope)
    return (index, dist2, ms) if timed else (index, dist2)


def cloud_voxel_fractions(ctx, xyz, dist2, voxel_size, tolerances, timed=False):
    """pxr_cloud_voxel_fractions: the fraction of the points of xyz (n, 3) whose dist2 (n,) is within each tolerance, averaged
    over the occupied voxels of side voxel_size (0: over the points).  xyz / dist2: float64 host arrays or DeviceArrays.
    Returns (fractions (n_tol,) float64, n_voxels), and with timed also {"insert", "reduce"} in milliseconds."""
    d_x = _device_cloud(ctx, xyz, "xyz")
    d_d = dist2 if isinstance(dist2, DeviceArray) else ctx.to_device(np.asarray(dist2, dtype=np.float64).reshape(-1), np.float64)
    if d_d.dtype != np.float64 or int(np.prod(d_d.shape)) != d_x.shape[0]:
        raise ValueError("dist2 must be (n,) float64, one entry per point")
    tol = np.ascontiguousarray(tolerances, dtype=np.float64).reshape(-1)
    frac = np.full(len(tol), np.nan)
    n_voxels = C.c_int64(0)
    args = (ctx.handle, int(d_x.shape[0]), d_x.ptr, d_d.ptr, float(voxel_size), len(tol), tol.ctypes.data_as(C.POINTER(C.c_double)),
            frac.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n_voxels))
    ms = _launch(ctx, "pxr_cloud_voxel_fractions", args, ("insert", "reduce"), timed)
    return (frac, int(n_voxels.value), ms) if timed else (frac, int(n_voxels.value))
