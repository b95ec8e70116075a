"""Python mirror of the reference's `sift::Sift` / `sift::InterestPoint` API
(/root/reference/sift.hpp:17-78, interestpoint.hpp:13-63) on top of the C ABI (include/sift_hip.h).

Same constructor arguments, same meaning, same error behaviour: Vigra precondition failures the
reference would throw surface as `PreconditionViolation`, its assert()s as `AssertionError`.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib

K_SQRT2 = float(np.float32(np.sqrt(2.0)))

KINDS = {"gaussian": 0, "dog": 1, "magnitude": 2, "orientation": 3}
STAGES = {"candidates": 0, "after_sort1": 1, "after_orient": 2, "after_sort2": 3, "final": 4}


class PreconditionViolation(RuntimeError):
    """vigra::PreconditionViolation analogue; str() carries Vigra's message text."""


class HipError(RuntimeError):
    pass


@dataclass
class InterestPoint:  # interestpoint.hpp:13-63
    scale: float
    octave: int
    index: int
    filtered: bool
    loc: tuple
    orientation: float
    descriptors: list = field(default_factory=list)


def _raise(rc, err):
    msg = err.value.decode(errors="replace")
    if rc == _lib.EPRECONDITION:
        raise PreconditionViolation(msg)
    if rc == _lib.EASSERT:
        raise AssertionError(msg)
    if rc == _lib.EINVAL:
        raise ValueError(msg or "sift_hip: invalid argument")
    raise HipError(msg or f"sift_hip error {rc}")


def pinned_array(shape, dtype=np.float32) -> np.ndarray:
    """numpy array in page-locked host memory (sift_hip_host_alloc): the copy engines move it at the PCIe rate in one
    asynchronous copy, where ordinary memory goes through the library's staging buffers (include/sift_hip.h).  The memory
    is released when the array (and every view of it) is gone."""
    import weakref
    L = _lib.load()
    dtype = np.dtype(dtype)
    n = int(np.prod(shape)) * dtype.itemsize
    p = L.sift_hip_host_alloc(max(n, 1))
    if not p:
        raise MemoryError(f"sift_hip_host_alloc({n}) failed")
    buf = (C.c_char * max(n, 1)).from_address(p)
    weakref.finalize(buf, L.sift_hip_host_free, p)
    return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)


class Gate:
    """sift_hip_gate: orders the phases of batches that run on different contexts of one GPU (include/sift_hip.h)."""

    def __init__(self, device: int = 0):
        self._L = _lib.load()
        self._h = C.c_void_p()
        if self._L.sift_hip_gate_create(device, C.byref(self._h)):
            self._h = C.c_void_p()
            raise HipError(f"sift_hip_gate_create({device}) failed")

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.sift_hip_gate_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One sift_hip_ctx (one GPU, one stream)."""

    def __init__(self, device: int = 0):
        self._L = _lib.load()
        self._h = C.c_void_p()
        err = C.create_string_buffer(512)
        rc = self._L.sift_hip_create(device, C.byref(self._h), err, 512)
        if rc:
            self._h = C.c_void_p()
            _raise(rc, err)
        self.device = device

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.sift_hip_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_gate(self, gate: "Gate | None"):
        self._gate = gate    # keeps the Gate object alive as long as this context points at it
        if self._L.sift_hip_set_gate(self._h, gate._h if gate is not None else None):
            raise ValueError("gate and context are on different devices, or the gate already joins its maximum of four contexts")

    def set_option(self, name: str, value: int):
        if self._L.sift_hip_set_option(self._h, name.encode(), int(value)):
            raise ValueError(f"unknown option {name}")

    # ---- Sift::calculate ---------------------------------------------------------------------
    def calculate_batch(self, imgs, params, raise_on_error=True):
        """Frames from host memory.  A uint8 array takes the 8-bit entry point (a quarter of the bytes cross the link, the GPU
        widens them to the floats vigra::importImage would have produced); anything else is handed over as float32."""
        imgs = np.asarray(imgs)
        u8 = imgs.dtype == np.uint8
        imgs = np.ascontiguousarray(imgs, dtype=np.uint8 if u8 else np.float32)
        if imgs.ndim == 2:
            imgs = imgs[None]
        n, h, w = imgs.shape
        err = C.create_string_buffer(512)
        if u8:
            rc = self._L.sift_hip_calculate_batch_u8(self._h, imgs.ctypes.data, n, w, h, C.byref(params), err, 512)
        else:
            rc = self._L.sift_hip_calculate_batch(self._h, imgs.reshape(-1), n, w, h, C.byref(params), err, 512)
        if rc and raise_on_error:
            _raise(rc, err)
        return rc, err.value.decode(errors="replace")

    def calculate_batch_device(self, dev_ptr: int, n: int, w: int, h: int, params, raise_on_error=True):
        err = C.create_string_buffer(512)
        rc = self._L.sift_hip_calculate_batch_device(self._h, C.c_void_p(dev_ptr), n, w, h, C.byref(params), err, 512)
        if rc and raise_on_error:
            _raise(rc, err)
        return rc, err.value.decode(errors="replace")

    def n_images(self) -> int:
        """Images of the batch whose results the context holds (the library's count, not the caller's)."""
        n = int(self._L.sift_hip_result_images(self._h))
        if n < 0:
            raise HipError("no result")
        return n

    def counts(self):
        out = np.zeros(self.n_images(), np.int32)
        if self._L.sift_hip_result_counts(self._h, out, out.size):
            raise HipError("no result")
        return out

    def status(self):
        out = np.zeros(self.n_images(), np.int32)
        if self._L.sift_hip_result_status(self._h, out, out.size):
            raise HipError("no result")
        return out

    def total(self) -> int:
        return int(self._L.sift_hip_result_total(self._h))

    def results(self, kp_out=None, desc_out=None):
        """(keypoints, descriptors [total, 128]).  `kp_out` / `desc_out`: caller arrays to fill (e.g. `pinned_array`s with
        room for at least total() entries); views of their first total() entries are returned."""
        t = max(self.total(), 0)
        kp = np.zeros(t, _lib.KEYPOINT_DTYPE) if kp_out is None else kp_out.reshape(-1)[:t]
        desc = np.zeros((t, 128), np.float32) if desc_out is None else desc_out.reshape(-1, 128)[:t]
        if kp.size < t or desc.shape[0] < t:
            raise ValueError("result arrays too small")
        if t > 0 and self._L.sift_hip_result_copy(self._h, kp.ctypes.data, desc.ctypes.data):
            raise HipError("sift_hip_result_copy failed")
        return kp, desc

    def results_u8(self, kp_out=None, desc_out=None):
        """(keypoints, descriptors [total, 128] uint8): results() with the descriptors quantised to 8 bits on the GPU
        (sift_hip_result_copy_u8; include/sift_hip.h, "8-bit descriptors and integer matching") - 128 instead of 512 bytes per
        keypoint cross the link.  `kp_out` / `desc_out` as for results()."""
        t = max(self.total(), 0)
        kp = np.zeros(t, _lib.KEYPOINT_DTYPE) if kp_out is None else kp_out.reshape(-1)[:t]
        desc = np.zeros((t, 128), np.uint8) if desc_out is None else desc_out.reshape(-1, 128)[:t]
        if kp.size < t or desc.shape[0] < t or desc.dtype != np.uint8:
            raise ValueError("result arrays too small, or descriptors not uint8")
        if t > 0 and (self._L.sift_hip_result_copy(self._h, kp.ctypes.data, None) or self._L.sift_hip_result_copy_u8(self._h, desc.ctypes.data)):
            raise HipError("sift_hip_result_copy_u8 failed")
        return kp, desc

    def results_sparse(self, rec_out=None, val_out=None):
        """The results in the sparse wire format, in host memory: (records uint8 [total, 34] = 20-byte keypoint record + 112
        presence bits, values float32 [n] = the descriptor floats that are not +0.0f) - what crosses the link is ~200 instead of
        532 bytes per keypoint.  `unpack_sparse_host` turns them back into (keypoints, descriptors).  Falls back to None when the
        results hold a value the format would lose (see sift_hip_result_sparse_size)."""
        t = max(self.total(), 0)
        nnz, lossless = C.c_int64(), C.c_int()
        if self._L.sift_hip_result_sparse_size(self._h, C.byref(nnz), C.byref(lossless)):
            raise HipError("sift_hip_result_sparse_size failed")
        if not lossless.value:
            return None
        rec = np.zeros((t, 34), np.uint8) if rec_out is None else rec_out.reshape(-1)[:t * 34].reshape(t, 34)
        val = np.zeros(nnz.value, np.float32) if val_out is None else val_out.reshape(-1)[:nnz.value]
        if val.size < nnz.value or rec.shape[0] < t:
            raise ValueError("result arrays too small")
        if t > 0 and self._L.sift_hip_result_copy_sparse(self._h, rec.ctypes.data, val.ctypes.data):
            raise HipError("sift_hip_result_copy_sparse failed")
        return rec, val

    def result_device_ptrs(self):
        a, b = C.c_void_p(), C.c_void_p()
        if self._L.sift_hip_result_device(self._h, C.byref(a), C.byref(b)):
            raise HipError("no result")
        return a.value or 0, b.value or 0

    def sparse_size(self, require_lossless: bool = True) -> int:
        """Number of descriptor floats the sparse wire format carries for the current results (include/sift_hip.h).
        Raises ValueError when the format cannot carry them (some bin 7 is not +0.0f): use the "full" wire then."""
        n, ok = C.c_int64(), C.c_int()
        if self._L.sift_hip_result_sparse_size(self._h, C.byref(n), C.byref(ok)):
            raise HipError("sift_hip_result_sparse_size failed")
        if require_lossless and not ok.value:
            raise ValueError("the sparse wire format would lose a bin 7 that is not +0.0f: send the full descriptors")
        return int(n.value)

    def sparse_pack(self, dev_records: int, dev_values: int, wait: bool = True):
        """Write total*34 record bytes and sparse_size() floats to the device addresses given.  wait=False: the pack is only
        queued (side stream) and this context's next batch may be started at once; `pack_wait()` - from any thread - returns
        when the lists are complete."""
        f = self._L.sift_hip_result_sparse_pack if wait else self._L.sift_hip_result_sparse_pack_async
        if f(self._h, C.c_void_p(dev_records), C.c_void_p(dev_values)):
            raise HipError("sift_hip_result_sparse_pack failed")

    def pack_wait(self):
        if self._L.sift_hip_result_pack_wait(self._h):
            raise HipError("sift_hip_result_pack_wait failed")

    def sparse_unpack(self, dev_records: int, dev_values: int, n_keypoints: int, dev_keypoints: int, dev_descriptors: int):
        """34-byte records + set floats (device addresses, from any context's sparse_pack) -> n_keypoints 20-byte keypoint
        records and n_keypoints * 128 floats at the device addresses given, on this context's GPU."""
        if self._L.sift_hip_sparse_unpack(self._h, C.c_void_p(dev_records), C.c_void_p(dev_values), int(n_keypoints),
                                          C.c_void_p(dev_keypoints), C.c_void_p(dev_descriptors)):
            raise HipError("sift_hip_sparse_unpack failed")

    def image(self, image: int = 0):
        w, h = C.c_int(), C.c_int()
        self._L.sift_hip_image_dims(self._h, C.byref(w), C.byref(h))
        out = np.empty((h.value, w.value), np.float32)
        if self._L.sift_hip_image_copy(self._h, image, out):
            return None
        return out

    # ---- inspection ------------------------------------------------------------------------------
    def level(self, kind: str, octave: int, level: int, image: int = 0):
        w, h = C.c_int(), C.c_int()
        if self._L.sift_hip_level_dims(self._h, KINDS[kind], octave, level, C.byref(w), C.byref(h)) or w.value == 0:
            return None
        out = np.empty((h.value, w.value), np.float32)
        if self._L.sift_hip_level_copy(self._h, image, KINDS[kind], octave, level, out):
            raise HipError("sift_hip_level_copy failed")
        return out

    def dog_stack(self, octave: int, dogs: int, image: int = 0):
        """The `dogs` DoG levels of one octave of one image as one array [dogs, h, w]: the stack localize() reads."""
        return np.stack([self.level("dog", octave, j, image) for j in range(dogs)])

    def level_scale(self, kind: str, octave: int, level: int) -> float:
        return float(self._L.sift_hip_level_scale(self._h, KINDS[kind], octave, level))

    def stage(self, name: str, image: int = 0):
        s = STAGES[name]
        n = self._L.sift_hip_stage_count(self._h, image, s)
        if n < 0:
            raise HipError("no such stage")
        out = np.zeros(n, _lib.KEYPOINT_DTYPE)
        if n and self._L.sift_hip_stage_copy(self._h, image, s, out.ctypes.data):
            raise HipError("sift_hip_stage_copy failed")
        return out

    # ---- sift::alg operators -------------------------------------------------------------------
    def _op(self, fn, img, sigma, shape):
        img = np.ascontiguousarray(img, np.float32)
        h, w = img.shape
        out = np.empty(shape, np.float32)
        err = C.create_string_buffer(512)
        rc = fn(self._h, img, w, h, sigma, out, err, 512)
        if rc:
            _raise(rc, err)
        return out

    def convolve_with_gauss(self, img, sigma):
        return self._op(self._L.sift_hip_convolve_with_gauss, img, sigma, np.shape(img))

    def reduce_to_next_level(self, img, sigma):
        h, w = np.shape(img)
        return self._op(self._L.sift_hip_reduce_to_next_level, img, sigma, ((h + 1) // 2, (w + 1) // 2))

    def increase_to_next_level(self, img, sigma):
        h, w = np.shape(img)
        return self._op(self._L.sift_hip_increase_to_next_level, img, sigma, (2 * h, 2 * w))

    def dog(self, lower, higher):
        lower = np.ascontiguousarray(lower, np.float32)
        higher = np.ascontiguousarray(higher, np.float32)
        out = np.empty_like(lower)
        if self._L.sift_hip_dog(self._h, lower, higher, lower.shape[1], lower.shape[0], out):
            raise HipError("sift_hip_dog failed")
        return out

    def gradient(self, img):
        img = np.ascontiguousarray(img, np.float32)
        mag, ori = np.empty_like(img), np.empty_like(img)
        if self._L.sift_hip_gradient(self._h, img, img.shape[1], img.shape[0], mag, ori):
            raise HipError("sift_hip_gradient failed")
        return mag, ori

    def edge_responses(self, d0, d1, d2, xs, ys):
        d0, d1, d2 = (np.ascontiguousarray(a, np.float32) for a in (d0, d1, d2))
        xs = np.ascontiguousarray(xs, np.uint16)
        ys = np.ascontiguousarray(ys, np.uint16)
        flags = np.zeros(xs.size, np.uint8)
        if self._L.sift_hip_edge_responses(self._h, d0, d1, d2, d0.shape[1], d0.shape[0], xs, ys, xs.size, flags):
            raise HipError("sift_hip_edge_responses failed")
        return flags

    # ---- sub-pixel localisation (include/sift_hip.h, "sub-pixel localisation") -------------------------
    def localize(self, max_moves=5, use=False, out=None):
        """sift_hip_result_localize: every keypoint of the last batch moved to the vertex of the 3D quadratic through its 27 DoG
        samples, in one launch -> LOCALIZED_DTYPE records in keypoint order (x, y: image coordinates; status 0: moved).  `use`:
        until the next calculate, verify_images, refine_fundamental_images and match_images_guided gather these x, y instead of
        (float)(x << octave).  `out`: a numpy array, a tensor or an address (host or device memory) that receives the records and
        is returned as given."""
        total = max(self.total(), 0) if self._L.sift_hip_result_images(self._h) >= 0 else 0   # no results: the call says so
        recs = np.zeros(total, _lib.LOCALIZED_DTYPE) if out is None else out
        err = C.create_string_buffer(512)
        rc = self._L.sift_hip_result_localize(self._h, int(max_moves), int(use), self._addr(recs), err, 512)
        if rc:
            _raise(rc, err)
        return recs

    def localize_points(self, dogs, xs, ys, indices, max_moves=5):
        """sift_hip_localize_points: the same device function over one stack `dogs` [L, h, w] and the points (xs, ys, indices)
        -> LOCALIZED_DTYPE records (octave 0, coordinates unscaled)."""
        dogs = np.ascontiguousarray(dogs, np.float32)
        xs, ys, indices = (np.ascontiguousarray(a, np.uint16).reshape(-1) for a in (xs, ys, indices))
        if dogs.ndim != 3 or not (xs.size == ys.size == indices.size):
            raise ValueError("localize_points: dogs is [L, h, w]; one x, y and index per point")
        out = np.zeros(xs.size, _lib.LOCALIZED_DTYPE)
        err = C.create_string_buffer(512)
        rc = self._L.sift_hip_localize_points(self._h, dogs, dogs.shape[0], dogs.shape[2], dogs.shape[1], xs, ys, indices, xs.size, int(max_moves),
                                              C.c_void_p(out.ctypes.data), err, 512)
        if rc:
            _raise(rc, err)
        return out

    def vertex_parabola(self, lnx, lny, px, py, rnx, rny):
        a = [np.ascontiguousarray(v, np.uint16) for v in (lnx, px, rnx)]
        b = [np.ascontiguousarray(v, np.float32) for v in (lny, py, rny)]
        out = np.zeros(a[0].size, np.float32)
        if self._L.sift_hip_vertex_parabola(self._h, a[0], b[0], a[1], b[1], a[2], b[2], a[0].size, out):
            raise HipError("sift_hip_vertex_parabola failed")
        return out

    def sort_by_filter(self, flags):
        flags = np.ascontiguousarray(flags, np.uint8)
        perm = np.zeros(flags.size, np.int32)
        if self._L.sift_hip_sort_by_filter(self._h, flags, flags.size, perm):
            raise HipError("sift_hip_sort_by_filter failed")
        return perm

    def profile(self, which: int):
        ms, n, by = C.c_double(), C.c_int64(), C.c_double()
        self._L.sift_hip_profile_get(self._h, which, C.byref(ms), C.byref(n), C.byref(by))
        return ms.value, n.value, by.value

    def profile_busy_ms(self, which: int) -> float:
        """time during which at least one launch of the class ran (overlapping launches counted once)"""
        ms = C.c_double()
        self._L.sift_hip_profile_get_busy(self._h, which, C.byref(ms))
        return ms.value

    def profile_batches(self) -> int:
        """Batches whose launches carried timing events since the last profile_reset()."""
        n = C.c_int64()
        self._L.sift_hip_profile_batches(self._h, C.byref(n))
        return int(n.value)

    def profile_reset(self):
        self._L.sift_hip_profile_reset(self._h)

    # ---- descriptor matching (include/sift_hip.h, "descriptor matching") --------------------------------
    @staticmethod
    def _addr(a):
        """Address of a numpy array, of a tensor (data_ptr) or a plain integer address: host or device memory."""
        if a is None:
            return None
        if isinstance(a, np.ndarray):
            return C.c_void_p(a.ctypes.data)
        if hasattr(a, "data_ptr"):
            return C.c_void_p(a.data_ptr())
        return C.c_void_p(int(a))

    @staticmethod
    def _pairs(pairs):
        p = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
        return np.ascontiguousarray(p[:, 0]), np.ascontiguousarray(p[:, 1])

    def knn2_sets(self, desc, offsets, pairs, kp=None, idx_out=None, dist_out=None):
        """sift_hip_knn2: top-2 of every query row of every pair -> (idx [rows, 2] int32, dist2 [rows, 2] float32), rows = the
        pairs' query rows in pair order.  `desc` / `kp`: numpy arrays, tensors or addresses (host or device memory); `idx_out` /
        `dist_out`: where the result goes instead of new numpy arrays (returned as given)."""
        return self._knn2_sets(self._L.sift_hip_knn2, np.float32, desc, offsets, pairs, kp, idx_out, dist_out)

    def _knn2_sets(self, call, dtype, desc, offsets, pairs, kp, idx_out, dist_out):
        offsets = np.ascontiguousarray(offsets, np.int64)
        pq, pt = self._pairs(pairs)
        rows = int(sum(offsets[q + 1] - offsets[q] for q in pq if 0 <= q < offsets.size - 1))
        idx = np.full((rows, 2), -1, np.int32) if idx_out is None else idx_out
        dist = np.full((rows, 2), np.inf, np.float32) if dist_out is None else dist_out
        if isinstance(desc, np.ndarray):
            desc = self._rows(desc, dtype)
        err = C.create_string_buffer(512)
        rc = call(self._h, self._addr(desc), self._addr(kp), offsets.size - 1, offsets, pq.size, pq, pt,
                                   self._addr(idx), self._addr(dist), err, 512)
        if rc:
            _raise(rc, err)
        return idx, dist

    def knn2(self, q, t, q_kp=None, t_kp=None):
        """Top-2 train rows of every row of `q` [nq, 128] among `t` [nt, 128] (numpy, host memory).  `q_kp` / `t_kp`: keypoint
        records whose has_descriptor decides which rows are valid (None: all)."""
        q = np.ascontiguousarray(q, np.float32).reshape(-1, 128)
        t = np.ascontiguousarray(t, np.float32).reshape(-1, 128)
        desc, offsets, kp = self._two_sets(q, t, q_kp, t_kp)
        return self.knn2_sets(desc, offsets, [(0, 1)], kp)

    @staticmethod
    def _rows(desc, dtype):
        """A numpy array as contiguous rows of `dtype`; byte rows must arrive as uint8 (no silent conversion of floats)."""
        if dtype == np.uint8 and desc.dtype != np.uint8:
            raise ValueError("8-bit matching: the rows must be uint8 (Context.quantize makes them)")
        return np.ascontiguousarray(desc, dtype)

    @staticmethod
    def _two_sets(q, t, q_kp, t_kp):
        desc = np.concatenate([q, t])
        offsets = np.array([0, q.shape[0], q.shape[0] + t.shape[0]], np.int64)
        kp = None
        if q_kp is not None or t_kp is not None:
            kp = np.zeros(desc.shape[0], _lib.KEYPOINT_DTYPE)
            kp["has_descriptor"] = 1
            if q_kp is not None:
                kp[:q.shape[0]] = q_kp
            if t_kp is not None:
                kp[q.shape[0]:] = t_kp
        return desc, offsets, kp

    def match_sets(self, desc, offsets, pairs, ratio=0.8, cross_check=False, kp=None, recs_out=None, quantized=False):
        """sift_hip_match: the filtered matches of every pair -> (records, counts): records (query, train, dist2, second2) in
        pair order, then query order; counts[p] of them belong to pair p.  `recs_out`: a tensor / address with room for one
        record per query row (then the first element returned is the total instead of an array).  `quantized`: the float rows
        are quantised to 8 bits on the device and matched by the integer distance (match_sets_u8 of quantize(desc))."""
        return self._match_sets(self._L.sift_hip_match, np.float32, desc, offsets, pairs, ratio, cross_check, kp, recs_out, quantized)

    def _match_sets(self, call, dtype, desc, offsets, pairs, ratio, cross_check, kp, recs_out, quantized):
        offsets = np.ascontiguousarray(offsets, np.int64)
        pq, pt = self._pairs(pairs)
        rows = int(sum(offsets[q + 1] - offsets[q] for q in pq if 0 <= q < offsets.size - 1))
        recs = np.zeros(rows, _lib.MATCH_DTYPE) if recs_out is None else recs_out
        counts = np.zeros(pq.size, np.int32)
        total = C.c_int64()
        if isinstance(desc, np.ndarray):
            desc = self._rows(desc, dtype)
        prm = _lib.MatchParams(float(ratio), 1 if cross_check else 0, self._quantized(quantized))
        err = C.create_string_buffer(512)
        rc = call(self._h, self._addr(desc), self._addr(kp), offsets.size - 1, offsets, pq.size, pq, pt, C.byref(prm),
                                    self._addr(recs), counts, C.byref(total), err, 512)
        if rc:
            _raise(rc, err)
        return (recs[:total.value] if recs_out is None else int(total.value)), counts

    def match(self, q, t, ratio=0.8, cross_check=False, q_kp=None, t_kp=None, quantized=False):
        """Matches of the rows of `q` among `t` (numpy, host memory): records (query, train, dist2, second2) in query order.
        `quantized` as for match_sets."""
        q = np.ascontiguousarray(q, np.float32).reshape(-1, 128)
        t = np.ascontiguousarray(t, np.float32).reshape(-1, 128)
        desc, offsets, kp = self._two_sets(q, t, q_kp, t_kp)
        return self.match_sets(desc, offsets, [(0, 1)], ratio, cross_check, kp, quantized=quantized)[0]

    # ---- 8-bit rows (include/sift_hip.h, "8-bit descriptors and integer matching") -----------------------------
    @staticmethod
    def _quantized(quantized):
        """The byte of sift_hip_match_params: False / True, or a number the call itself judges (above 1: ValueError)."""
        q = int(quantized)
        if not 0 <= q <= 255:
            raise ValueError("quantized must be False or True")
        return q

    def quantize(self, desc, out=None):
        """sift_hip_quantize: float rows [n, 128] -> uint8 rows [n, 128], q(v) = trunc(fmaf(v, 255, 0.5)) clamped to 0 .. 255.
        `desc`: a numpy array, a tensor or an address; `out`: where the bytes go instead of a new numpy array (a tensor or an
        address needs `rows`-sized room; returned as given)."""
        if isinstance(desc, np.ndarray):
            desc = np.ascontiguousarray(desc, np.float32).reshape(-1, 128)
            rows = desc.shape[0]
        elif hasattr(desc, "numel"):
            rows = int(desc.numel()) // 128
        else:
            raise ValueError("quantize: a numpy array or a tensor (use the C call for a plain address)")
        res = np.zeros((rows, 128), np.uint8) if out is None else out
        err = C.create_string_buffer(512)
        rc = self._L.sift_hip_quantize(self._h, self._addr(desc), rows, self._addr(res), err, 512)
        if rc:
            _raise(rc, err)
        return res

    def knn2_sets_u8(self, desc, offsets, pairs, kp=None, idx_out=None, dist_out=None):
        """sift_hip_knn2_u8: knn2_sets over uint8 rows; the distances are the exact integers sum (a - b)^2 as float32."""
        return self._knn2_sets(self._L.sift_hip_knn2_u8, np.uint8, desc, offsets, pairs, kp, idx_out, dist_out)

    def knn2_u8(self, q, t, q_kp=None, t_kp=None):
        """knn2 over uint8 rows `q` [nq, 128] and `t` [nt, 128] (numpy, host memory)."""
        q = self._rows(np.asarray(q), np.uint8).reshape(-1, 128)
        t = self._rows(np.asarray(t), np.uint8).reshape(-1, 128)
        desc, offsets, kp = self._two_sets(q, t, q_kp, t_kp)
        return self.knn2_sets_u8(desc, offsets, [(0, 1)], kp)

    def match_sets_u8(self, desc, offsets, pairs, ratio=0.8, cross_check=False, kp=None, recs_out=None):
        """sift_hip_match_u8: match_sets over uint8 rows."""
        return self._match_sets(self._L.sift_hip_match_u8, np.uint8, desc, offsets, pairs, ratio, cross_check, kp, recs_out, False)

    def match_u8(self, q, t, ratio=0.8, cross_check=False, q_kp=None, t_kp=None):
        """match over uint8 rows (numpy, host memory): records in query order."""
        q = self._rows(np.asarray(q), np.uint8).reshape(-1, 128)
        t = self._rows(np.asarray(t), np.uint8).reshape(-1, 128)
        desc, offsets, kp = self._two_sets(q, t, q_kp, t_kp)
        return self.match_sets_u8(desc, offsets, [(0, 1)], ratio, cross_check, kp)[0]

    def match_images(self, pairs, ratio=0.8, cross_check=False, quantized=False):
        """sift_hip_result_match: matches between images of the last batch, on the device-resident results -> (records, counts).
        `quantized`: over the results' descriptors quantised to 8 bits (match_sets_u8 of results_u8())."""
        pq, pt = self._pairs(pairs)
        cnt = self.counts() if self._L.sift_hip_result_images(self._h) >= 0 else np.zeros(0, np.int32)   # none: the call says so
        rows = int(sum(cnt[q] for q in pq if 0 <= q < cnt.size))
        recs = np.zeros(rows, _lib.MATCH_DTYPE)
        counts = np.zeros(pq.size, np.int32)
        total = C.c_int64()
        prm = _lib.MatchParams(float(ratio), 1 if cross_check else 0, self._quantized(quantized))
        err = C.create_string_buffer(512)
        rc = self._L.sift_hip_result_match(self._h, pq.size, pq, pt, C.byref(prm), C.c_void_p(recs.ctypes.data), counts, C.byref(total), err, 512)
        if rc:
            _raise(rc, err)
        return recs[:total.value], counts

    # ---- guided matching (include/sift_hip.h, "guided matching") --------------------------------------------
    @staticmethod
    def _guide(model, threshold):
        if model not in _lib.GUIDE_MODELS:
            raise ValueError('guided matching: model must be "homography" or "fundamental"')
        return _lib.GuideParams(_lib.GUIDE_MODELS[model], float(threshold))

    @staticmethod
    def _models9(models, n_pairs):
        """[n, 9] float32 of a HOMOGRAPHY_DTYPE / FUNDAMENTAL_DTYPE array (as verify_images returns it) or of n x 9 numbers; a
        tensor or an address (device memory) passes through."""
        if isinstance(models, np.ndarray) and models.dtype.names:
            models = models["h" if "h" in models.dtype.names else "f"]
        if isinstance(models, (np.ndarray, list, tuple)):
            models = np.ascontiguousarray(models, np.float32).reshape(-1, 9)
            if models.shape[0] != n_pairs:
                raise ValueError("guided matching: one model per pair")
        return models

    def knn2_guided_sets(self, desc, xy, offsets, pairs, models, model="homography", threshold=3.0, kp=None, idx_out=None, dist_out=None):
        """sift_hip_knn2_guided: knn2_sets among the train rows that are admissible under the pair's model -> (idx, dist2).  `xy`:
        two floats per row of `desc`; `models`: one per pair, a HOMOGRAPHY_DTYPE / FUNDAMENTAL_DTYPE array or [n_pairs, 9] floats;
        xy and models may be numpy arrays, tensors or addresses (host or device memory)."""
        return self._knn2_guided_sets(self._L.sift_hip_knn2_guided, np.float32, desc, xy, offsets, pairs, models, model, threshold, kp, idx_out,
                                      dist_out)

    def _knn2_guided_sets(self, call, dtype, desc, xy, offsets, pairs, models, model, threshold, kp, idx_out, dist_out):
        offsets = np.ascontiguousarray(offsets, np.int64)
        pq, pt = self._pairs(pairs)
        rows = int(sum(offsets[q + 1] - offsets[q] for q in pq if 0 <= q < offsets.size - 1))
        idx = np.full((rows, 2), -1, np.int32) if idx_out is None else idx_out
        dist = np.full((rows, 2), np.inf, np.float32) if dist_out is None else dist_out
        if isinstance(desc, np.ndarray):
            desc = self._rows(desc, dtype)
        if isinstance(xy, np.ndarray):
            xy = np.ascontiguousarray(xy, np.float32)
        prm = self._guide(model, threshold)
        models = self._models9(models, pq.size)
        err = C.create_string_buffer(512)
        rc = call(self._h, self._addr(desc), self._addr(kp), self._addr(xy), offsets.size - 1, offsets, pq.size, pq, pt,
                                          C.byref(prm), self._addr(models), self._addr(idx), self._addr(dist), err, 512)
        if rc:
            _raise(rc, err)
        return idx, dist

    def knn2_guided(self, q, t, q_xy, t_xy, model_matrix, model="homography", threshold=3.0, q_kp=None, t_kp=None):
        """Guided top-2 of the rows of `q` among `t` (numpy, host memory): `q_xy` / `t_xy` [n, 2] the rows' points, `model_matrix`
        nine floats (query to train)."""
        q = np.ascontiguousarray(q, np.float32).reshape(-1, 128)
        t = np.ascontiguousarray(t, np.float32).reshape(-1, 128)
        desc, offsets, kp = self._two_sets(q, t, q_kp, t_kp)
        xy = np.concatenate([np.asarray(q_xy, np.float32).reshape(-1, 2), np.asarray(t_xy, np.float32).reshape(-1, 2)])
        return self.knn2_guided_sets(desc, xy, offsets, [(0, 1)], np.asarray(model_matrix, np.float32).reshape(1, 9), model, threshold, kp)

    def match_guided_sets(self, desc, xy, offsets, pairs, models, model="homography", threshold=3.0, ratio=0.8, cross_check=False, kp=None,
                          recs_out=None, quantized=False):
        """sift_hip_match_guided: match_sets under the pairs' models -> (records, counts).  Arguments as for knn2_guided_sets and
        match_sets.  This call takes float rows only: `quantized=True` is a ValueError (the call says so; match_guided_sets_u8)."""
        return self._match_guided_sets(self._L.sift_hip_match_guided, np.float32, desc, xy, offsets, pairs, models, model, threshold, ratio,
                                       cross_check, kp, recs_out, quantized)

    def _match_guided_sets(self, call, dtype, desc, xy, offsets, pairs, models, model, threshold, ratio, cross_check, kp, recs_out, quantized):
        offsets = np.ascontiguousarray(offsets, np.int64)
        pq, pt = self._pairs(pairs)
        rows = int(sum(offsets[q + 1] - offsets[q] for q in pq if 0 <= q < offsets.size - 1))
        recs = np.zeros(rows, _lib.MATCH_DTYPE) if recs_out is None else recs_out
        counts = np.zeros(pq.size, np.int32)
        total = C.c_int64()
        if isinstance(desc, np.ndarray):
            desc = self._rows(desc, dtype)
        if isinstance(xy, np.ndarray):
            xy = np.ascontiguousarray(xy, np.float32)
        mprm = _lib.MatchParams(float(ratio), 1 if cross_check else 0, self._quantized(quantized))
        gprm = self._guide(model, threshold)
        models = self._models9(models, pq.size)
        err = C.create_string_buffer(512)
        rc = call(self._h, self._addr(desc), self._addr(kp), self._addr(xy), offsets.size - 1, offsets, pq.size, pq, pt,
                                           C.byref(mprm), C.byref(gprm), self._addr(models), self._addr(recs), counts, C.byref(total), err, 512)
        if rc:
            _raise(rc, err)
        return (recs[:total.value] if recs_out is None else int(total.value)), counts

    def match_guided(self, q, t, q_xy, t_xy, model_matrix, model="homography", threshold=3.0, ratio=0.8, cross_check=False, q_kp=None,
                     t_kp=None):
        """Guided matches of the rows of `q` among `t` (numpy, host memory): records in query order."""
        q = np.ascontiguousarray(q, np.float32).reshape(-1, 128)
        t = np.ascontiguousarray(t, np.float32).reshape(-1, 128)
        desc, offsets, kp = self._two_sets(q, t, q_kp, t_kp)
        xy = np.concatenate([np.asarray(q_xy, np.float32).reshape(-1, 2), np.asarray(t_xy, np.float32).reshape(-1, 2)])
        return self.match_guided_sets(desc, xy, offsets, [(0, 1)], np.asarray(model_matrix, np.float32).reshape(1, 9), model, threshold, ratio,
                                      cross_check, kp)[0]

    def match_images_guided(self, pairs, models, model="homography", threshold=3.0, ratio=0.8, cross_check=False, quantized=False,
                            localized=False):
        """sift_hip_result_match_guided: match_images under the pairs' models, e.g. those verify_images returned, on the
        device-resident results (the keypoints' image coordinates are built on the GPU) -> (records, counts).  `quantized=True`
        is a ValueError, as for match_guided_sets.  `localized`: localize(use=True) first - the points are the sub-pixel ones."""
        return self._match_images_guided(self._L.sift_hip_result_match_guided, pairs, models, model, threshold, ratio, cross_check, quantized,
                                         localized)

    def _match_images_guided(self, call, pairs, models, model, threshold, ratio, cross_check, quantized, localized):
        if localized:
            self.localize(use=True)
        pq, pt = self._pairs(pairs)
        cnt = self.counts() if self._L.sift_hip_result_images(self._h) >= 0 else np.zeros(0, np.int32)   # none: the call says so
        rows = int(sum(cnt[q] for q in pq if 0 <= q < cnt.size))
        recs = np.zeros(rows, _lib.MATCH_DTYPE)
        counts = np.zeros(pq.size, np.int32)
        total = C.c_int64()
        mprm = _lib.MatchParams(float(ratio), 1 if cross_check else 0, self._quantized(quantized))
        gprm = self._guide(model, threshold)
        models = self._models9(models, pq.size)
        err = C.create_string_buffer(512)
        rc = call(self._h, pq.size, pq, pt, C.byref(mprm), C.byref(gprm), self._addr(models), C.c_void_p(recs.ctypes.data), counts,
                  C.byref(total), err, 512)
        if rc:
            _raise(rc, err)
        return recs[:total.value], counts

    # ---- guided matching on 8-bit descriptors (include/sift_hip.h) ------------------------------------------
    def knn2_guided_sets_u8(self, desc, xy, offsets, pairs, models, model="homography", threshold=3.0, kp=None, idx_out=None, dist_out=None):
        """sift_hip_knn2_guided_u8: knn2_guided_sets over uint8 rows; the distances are the exact integers of knn2_sets_u8."""
        return self._knn2_guided_sets(self._L.sift_hip_knn2_guided_u8, np.uint8, desc, xy, offsets, pairs, models, model, threshold, kp, idx_out,
                                      dist_out)

    def knn2_guided_u8(self, q, t, q_xy, t_xy, model_matrix, model="homography", threshold=3.0, q_kp=None, t_kp=None):
        """knn2_guided over uint8 rows `q` [nq, 128] and `t` [nt, 128] (numpy, host memory)."""
        q = self._rows(np.asarray(q), np.uint8).reshape(-1, 128)
        t = self._rows(np.asarray(t), np.uint8).reshape(-1, 128)
        desc, offsets, kp = self._two_sets(q, t, q_kp, t_kp)
        xy = np.concatenate([np.asarray(q_xy, np.float32).reshape(-1, 2), np.asarray(t_xy, np.float32).reshape(-1, 2)])
        return self.knn2_guided_sets_u8(desc, xy, offsets, [(0, 1)], np.asarray(model_matrix, np.float32).reshape(1, 9), model, threshold, kp)

    def match_guided_sets_u8(self, desc, xy, offsets, pairs, models, model="homography", threshold=3.0, ratio=0.8, cross_check=False, kp=None,
                             recs_out=None, quantized=True):
        """sift_hip_match_guided_u8: match_guided_sets over uint8 rows -> (records, counts).  `quantized` is the byte of the
        parameters: False and True both mean bytes here, a number above 1 is a ValueError (the call says so)."""
        return self._match_guided_sets(self._L.sift_hip_match_guided_u8, np.uint8, desc, xy, offsets, pairs, models, model, threshold, ratio,
                                       cross_check, kp, recs_out, quantized)

    def match_guided_u8(self, q, t, q_xy, t_xy, model_matrix, model="homography", threshold=3.0, ratio=0.8, cross_check=False, q_kp=None,
                        t_kp=None):
        """match_guided over uint8 rows (numpy, host memory): records in query order."""
        q = self._rows(np.asarray(q), np.uint8).reshape(-1, 128)
        t = self._rows(np.asarray(t), np.uint8).reshape(-1, 128)
        desc, offsets, kp = self._two_sets(q, t, q_kp, t_kp)
        xy = np.concatenate([np.asarray(q_xy, np.float32).reshape(-1, 2), np.asarray(t_xy, np.float32).reshape(-1, 2)])
        return self.match_guided_sets_u8(desc, xy, offsets, [(0, 1)], np.asarray(model_matrix, np.float32).reshape(1, 9), model, threshold,
                                         ratio, cross_check, kp)[0]

    def match_images_guided_u8(self, pairs, models, model="homography", threshold=3.0, ratio=0.8, cross_check=False, localized=False):
        """sift_hip_result_match_guided_u8: match_images_guided over the results' descriptors quantised to 8 bits on the device
        (match_guided_sets_u8 of results_u8() and the same coordinates) -> (records, counts)."""
        return self._match_images_guided(self._L.sift_hip_result_match_guided_u8, pairs, models, model, threshold, ratio, cross_check, True,
                                         localized)

    # ---- geometric verification (include/sift_hip.h, "geometric verification") ----------------------------
    def ransac_homography(self, pts, offsets=None, iterations=2048, threshold=3.0, seed=0, want_scores=False, models_out=None,
                          inlier_out=None, scores_out=None, refine=0):
        """sift_hip_ransac_homography: the best four-point homography of every set of correspondences (qx, qy, tx, ty) ->
        (models, inlier[, scores]): models[s] = (h [9] row-major, inliers, iteration; -1: none, refined), inlier one byte per row,
        scores [n_sets, iterations] with `want_scores`.  `refine`: rounds of least-squares re-estimation over the winner's inliers,
        0 .. 8 (0: the minimal-sample model); models[s]["refined"] of them were accepted.  `pts`: a numpy array [rows, 4], a tensor or an address (host or device memory);
        `offsets`: n_sets + 1 row offsets (None: one set, numpy input only); `*_out`: where a result goes instead of a new numpy
        array (returned as given)."""
        if isinstance(pts, np.ndarray):
            pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
        if offsets is None:
            offsets = [0, pts.shape[0]]
        offsets = np.ascontiguousarray(offsets, np.int64)
        n_sets = max(offsets.size - 1, 0)
        rows = int(offsets[-1]) if offsets.size and offsets[-1] > 0 else 0
        models = np.zeros(n_sets, _lib.HOMOGRAPHY_DTYPE) if models_out is None else models_out
        inlier = np.zeros(rows, np.uint8) if inlier_out is None else inlier_out
        scores = scores_out
        if scores is None and want_scores:
            scores = np.zeros((n_sets, int(iterations) if 0 < iterations <= 65536 else 0), np.int32)   # out of range: the call says so
        prm = _lib.RansacParams(int(iterations) & 0xffffffff, int(seed) & 0xffffffff, float(threshold), int(refine) & 0xffffffff)
        err = C.create_string_buffer(512)
        rc = self._L.sift_hip_ransac_homography(self._h, self._addr(pts), n_sets, offsets, C.byref(prm), self._addr(models), self._addr(inlier),
                                                self._addr(scores), err, 512)
        if rc:
            _raise(rc, err)
        return (models, inlier, scores) if scores is not None else (models, inlier)

    def ransac_fundamental(self, pts, offsets=None, iterations=2048, threshold=3.0, seed=0, want_scores=False, models_out=None,
                           inlier_out=None, scores_out=None, refine=0):
        """sift_hip_ransac_fundamental: the best seven-point fundamental matrix of every set of correspondences (qx, qy, tx, ty),
        (tx, ty, 1) F (qx, qy, 1)^T = 0 -> (models, inlier[, scores]): models[s] = (f [9] row-major, inliers, iteration; -1: none,
        root), inlier one byte per row, scores [n_sets, 3 * iterations] with `want_scores` (slot 3 * sample + root).  Arguments as
        for ransac_homography; `refine` must be 0 (there is no least-squares refit of F)."""
        if isinstance(pts, np.ndarray):
            pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
        if offsets is None:
            offsets = [0, pts.shape[0]]
        offsets = np.ascontiguousarray(offsets, np.int64)
        n_sets = max(offsets.size - 1, 0)
        rows = int(offsets[-1]) if offsets.size and offsets[-1] > 0 else 0
        models = np.zeros(n_sets, _lib.FUNDAMENTAL_DTYPE) if models_out is None else models_out
        inlier = np.zeros(rows, np.uint8) if inlier_out is None else inlier_out
        scores = scores_out
        if scores is None and want_scores:
            scores = np.zeros((n_sets, 3 * int(iterations) if 0 < iterations <= 65536 else 0), np.int32)   # out of range: the call says so
        prm = _lib.RansacParams(int(iterations) & 0xffffffff, int(seed) & 0xffffffff, float(threshold), int(refine) & 0xffffffff)
        err = C.create_string_buffer(512)
        rc = self._L.sift_hip_ransac_fundamental(self._h, self._addr(pts), n_sets, offsets, C.byref(prm), self._addr(models), self._addr(inlier),
                                                 self._addr(scores), err, 512)
        if rc:
            _raise(rc, err)
        return (models, inlier, scores) if scores is not None else (models, inlier)

    def refine_homography(self, pts, models, offsets=None, threshold=3.0, rounds=2, inlier_out=None):
        """sift_hip_refine_homography: at most `rounds` (0 .. 8) rounds of least-squares re-estimation of given models over their
        own inliers, no sampling -> (models, inlier).  `models`: a HOMOGRAPHY_DTYPE array (copied; h and iteration are read, a
        model with iteration -1 is left alone), or a tensor / address that is refined in place and returned as given."""
        if isinstance(pts, np.ndarray):
            pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
        if offsets is None:
            offsets = [0, pts.shape[0]]
        offsets = np.ascontiguousarray(offsets, np.int64)
        n_sets = max(offsets.size - 1, 0)
        rows = int(offsets[-1]) if offsets.size and offsets[-1] > 0 else 0
        if isinstance(models, np.ndarray):
            models = np.array(models, _lib.HOMOGRAPHY_DTYPE).reshape(-1)
            if models.size != n_sets:
                raise ValueError("refine_homography: one model per set")
        inlier = np.zeros(rows, np.uint8) if inlier_out is None else inlier_out
        err = C.create_string_buffer(512)
        rc = self._L.sift_hip_refine_homography(self._h, self._addr(pts), n_sets, offsets, float(threshold), int(rounds), self._addr(models),
                                                self._addr(inlier), err, 512)
        if rc:
            _raise(rc, err)
        return models, inlier

    def refine_fundamental(self, pts, offsets, models, threshold=3.0, rounds=2, refined_out=None, inlier_out=None):
        """sift_hip_refine_fundamental: at most `rounds` (0 .. 8) rounds of the least-squares refit of given fundamental matrices
        over their own inliers, no sampling -> (models, refined, inlier); refined[s] = the rounds accepted for set s.  `models`:
        a FUNDAMENTAL_DTYPE array (copied; f and iteration are read, a model with iteration -1 is left alone), or a tensor /
        address that is refined in place and returned as given.  `offsets` None: one set (numpy rows only)."""
        if isinstance(pts, np.ndarray):
            pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
        if offsets is None:
            offsets = [0, pts.shape[0]]
        offsets = np.ascontiguousarray(offsets, np.int64)
        n_sets = max(offsets.size - 1, 0)
        rows = int(offsets[-1]) if offsets.size and offsets[-1] > 0 else 0
        if isinstance(models, np.ndarray):
            models = np.array(models, _lib.FUNDAMENTAL_DTYPE).reshape(-1)
            if models.size != n_sets:
                raise ValueError("refine_fundamental: one model per set")
        refined = np.zeros(n_sets, np.int32) if refined_out is None else refined_out
        inlier = np.zeros(rows, np.uint8) if inlier_out is None else inlier_out
        err = C.create_string_buffer(512)
        rc = self._L.sift_hip_refine_fundamental(self._h, self._addr(pts), n_sets, offsets, float(threshold), int(rounds), self._addr(models),
                                                 self._addr(refined), self._addr(inlier), err, 512)
        if rc:
            _raise(rc, err)
        return models, refined, inlier

    def refine_fundamental_images(self, pairs, recs, counts, models, threshold=3.0, rounds=2, localized=False):
        """sift_hip_result_refine_fundamental: refine_fundamental over the last batch, from the records, counts and models that
        verify_images(model="fundamental") returned for `pairs`; the coordinates are built on the GPU -> (models, refined,
        inlier), inlier[i] belonging to recs[i].  `localized`: localize(use=True) first - sub-pixel coordinates."""
        if localized:
            self.localize(use=True)
        pq, pt = self._pairs(pairs)
        recs = np.ascontiguousarray(recs, _lib.MATCH_DTYPE).reshape(-1)
        counts = np.ascontiguousarray(counts, np.int32).reshape(-1)
        models = np.array(models, _lib.FUNDAMENTAL_DTYPE).reshape(-1)
        if counts.size != pq.size or models.size != pq.size or (counts >= 0).all() and int(counts.sum()) != recs.size:
            raise ValueError("refine_fundamental_images: one count and one model per pair, and the counts' records")
        refined = np.zeros(pq.size, np.int32)
        inlier = np.zeros(recs.size, np.uint8)
        err = C.create_string_buffer(512)
        rc = self._L.sift_hip_result_refine_fundamental(self._h, pq.size, pq, pt, C.c_void_p(recs.ctypes.data), counts, float(threshold), int(rounds),
                                                        C.c_void_p(models.ctypes.data), C.c_void_p(refined.ctypes.data),
                                                        C.c_void_p(inlier.ctypes.data), err, 512)
        if rc:
            _raise(rc, err)
        return models, refined, inlier

    def verify_images(self, pairs, ratio=0.8, cross_check=False, iterations=2048, threshold=3.0, seed=0, refine=0, model="homography",
                      quantized=False, localized=False):
        """sift_hip_result_verify: match_images followed by ransac_homography on the matches' image coordinates, all on the
        device-resident results -> (records, counts, models, inlier): models[p] belongs to pair p, inlier[i] to records[i].
        `refine` as for ransac_homography.  model="fundamental": sift_hip_result_verify_fundamental, ransac_fundamental in
        place of ransac_homography (models of FUNDAMENTAL_DTYPE; `refine` must be 0).  `quantized` as for match_images.
        `localized`: localize(use=True) first - the coordinates are the sub-pixel ones of the localisation records."""
        if model not in ("homography", "fundamental"):
            raise ValueError('verify_images: model must be "homography" or "fundamental"')
        fund = model == "fundamental"
        if localized:
            self.localize(use=True)
        pq, pt = self._pairs(pairs)
        cnt = self.counts() if self._L.sift_hip_result_images(self._h) >= 0 else np.zeros(0, np.int32)   # none: the call says so
        rows = int(sum(cnt[q] for q in pq if 0 <= q < cnt.size))
        recs = np.zeros(rows, _lib.MATCH_DTYPE)
        inlier = np.zeros(rows, np.uint8)
        models = np.zeros(pq.size, _lib.FUNDAMENTAL_DTYPE if fund else _lib.HOMOGRAPHY_DTYPE)
        counts = np.zeros(pq.size, np.int32)
        total = C.c_int64()
        mprm = _lib.MatchParams(float(ratio), 1 if cross_check else 0, self._quantized(quantized))
        rprm = _lib.RansacParams(int(iterations) & 0xffffffff, int(seed) & 0xffffffff, float(threshold), int(refine) & 0xffffffff)
        err = C.create_string_buffer(512)
        call = self._L.sift_hip_result_verify_fundamental if fund else self._L.sift_hip_result_verify
        rc = call(self._h, pq.size, pq, pt, C.byref(mprm), C.byref(rprm), C.c_void_p(recs.ctypes.data), counts, C.byref(total),
                  C.c_void_p(models.ctypes.data), C.c_void_p(inlier.ctypes.data), err, 512)
        if rc:
            _raise(rc, err)
        return recs[:total.value], counts, models, inlier[:total.value]

    # ---- homography warp (include/sift_hip.h, "homography warp") ---------------------------------------------
    def warp_homography(self, imgs, models, src=None, out_shape=None, origin=(0, 0), fill=0.0, interp="bilinear", path=0, out=None, mask=False,
                        want_tiles=False, shape=None):
        """sift_hip_warp_homography: job j resamples image src[j] (None: image j) under models[j] -> (out[, mask][, tiles]):
        out [n_jobs, out_h, out_w] float32, pixel (x, y) being the source at H (x + origin[0], y + origin[1], 1); mask one byte
        per pixel (1: covered, else `fill`); tiles = (staged, direct) with `want_tiles`.  The model maps query to train, so the
        H of a verified pair brings the pair's TRAIN image into its QUERY frame.  `imgs`: a numpy array [n, h, w], or a tensor
        / an address (device memory) with `shape` = (n, h, w); `models`: [n_jobs, 9] numbers, the records verify_images returns,
        a tensor or an address; `out_shape` (h, w): the images' by default; `interp`: "nearest" or "bilinear"; `path` 1: every
        tile reads global memory (the same bits); `out`, and `mask` when it is not a bool: where a result goes (returned as given)."""
        if isinstance(imgs, np.ndarray):
            imgs = np.ascontiguousarray(imgs, np.float32)
            imgs = imgs[None] if imgs.ndim == 2 else imgs
            shape = imgs.shape
        elif shape is None:
            shape = tuple(imgs.shape)   # a tensor
        if len(shape) != 3:
            raise ValueError("warp_homography: imgs is [n, h, w]")
        if interp not in _lib.WARP_INTERP:
            raise ValueError('warp_homography: interp must be "nearest" or "bilinear"')
        if isinstance(models, np.ndarray) and models.dtype.names:
            models = models["h"]
        if isinstance(models, (np.ndarray, list, tuple)):
            models = np.ascontiguousarray(models, np.float32).reshape(-1, 9)
            n_jobs = models.shape[0]
        else:
            n_jobs = len(src) if src is not None else int(shape[0])
        if src is not None:
            src = np.ascontiguousarray(src, np.int32).reshape(-1)
            if src.size != n_jobs:
                raise ValueError("warp_homography: one src index per model")
        oh, ow = (int(shape[1]), int(shape[2])) if out_shape is None else (int(out_shape[0]), int(out_shape[1]))
        prm = _lib.WarpParams(ow, oh, int(origin[0]), int(origin[1]), float(fill), _lib.WARP_INTERP[interp], int(path) & 0xff)
        size = (n_jobs, max(oh, 0), max(ow, 0))   # a bad size: the call says so
        res = np.zeros(size, np.float32) if out is None else out
        msk = (np.zeros(size, np.uint8) if mask else None) if isinstance(mask, bool) else mask
        tiles = np.zeros(2, np.int64) if want_tiles else None
        err = C.create_string_buffer(512)
        rc = self._L.sift_hip_warp_homography(self._h, self._addr(imgs), int(shape[0]), int(shape[2]), int(shape[1]), n_jobs, self._addr(src),
                                              self._addr(models), C.byref(prm), self._addr(res), self._addr(msk), self._addr(tiles), err, 512)
        if rc:
            _raise(rc, err)
        got = (res,) + ((msk,) if msk is not None else ()) + (((int(tiles[0]), int(tiles[1])),) if want_tiles else ())
        return got[0] if len(got) == 1 else got

    # ---- direct alignment (include/sift_hip.h, "direct alignment") ----------------------------------------------
    def align_homography(self, imgs, pairs, models, rounds=4, border=2, min_pixels=256, damping=0.0, path=0, out=None, want_sums=False, shape=None):
        """sift_hip_align_homography: refines models[p] (query to train) of pair p = (query, train) on the pixels of the two
        frames, by at most `rounds` (0 .. 8) Gauss-Newton steps on sum (Q - gain T(H .) - bias)^2 -> (models, out[, sums]):
        the records with h rewritten, and one ALIGNMENT_DTYPE record per pair (h, gain, bias, rms0, rms, pixels, rounds,
        status).  `imgs`: a numpy array [n, h, w], or a tensor / an address (device memory) with `shape` = (n, h, w);
        `models`: HOMOGRAPHY_DTYPE records (copied; [n_pairs, 9] numbers become records with iteration 0), or a tensor / an
        address of such records (host or device memory), rewritten in place; `out`: where the result records go (returned as given);
        `border`: pixels of the query frame's rim left out; a pass with fewer than `min_pixels` pixels stops its pair;
        `damping`: the diagonal of the normal matrix times 1 + damping; `path` 1: the masked kernel (the same bits);
        `want_sums`: [n_pairs, 80] float64, the sums of each pair's last pass."""
        if isinstance(imgs, np.ndarray):
            imgs = np.ascontiguousarray(imgs, np.float32)
            imgs = imgs[None] if imgs.ndim == 2 else imgs
            shape = imgs.shape
        elif shape is None:
            shape = tuple(imgs.shape)   # a tensor
        if len(shape) != 3:
            raise ValueError("align_homography: imgs is [n, h, w]")
        if not 0 <= int(path) <= 255:
            raise ValueError("align_homography: path must be 0 or 1")
        pq, pt = self._pairs(pairs)
        if isinstance(models, (np.ndarray, list, tuple)):
            if isinstance(models, np.ndarray) and models.dtype.names:
                models = np.array(models, _lib.HOMOGRAPHY_DTYPE).reshape(-1)
            else:
                h9 = np.ascontiguousarray(models, np.float32).reshape(-1, 9)
                models = np.zeros(h9.shape[0], _lib.HOMOGRAPHY_DTYPE)
                models["h"] = h9
            if models.size != pq.size:
                raise ValueError("align_homography: one model per pair")
        res = np.zeros(pq.size, _lib.ALIGNMENT_DTYPE) if out is None else out
        sums = np.zeros((pq.size, _lib.ALIGN_SUMS), np.float64) if want_sums else None
        prm = _lib.AlignParams(int(rounds), int(border), int(min_pixels), float(damping), int(path))
        err = C.create_string_buffer(512)
        rc = self._L.sift_hip_align_homography(self._h, self._addr(imgs), int(shape[0]), int(shape[2]), int(shape[1]), pq.size, pq, pt, C.byref(prm),
                                               self._addr(models), self._addr(res), self._addr(sums), err, 512)
        if rc:
            _raise(rc, err)
        return (models, res, sums) if want_sums else (models, res)

    # ---- compositor (include/sift_hip.h, "compositor") ---------------------------------------------------------
    @staticmethod
    def _composite_inputs(name, imgs, models, offsets, src, out_shape, interp, shape, gains):
        """What composite_homography and composite_twoband share -> (imgs, shape, models, n_jobs, offsets, src, (oh, ow), gains)."""
        if isinstance(imgs, np.ndarray):
            imgs = np.ascontiguousarray(imgs, np.float32)
            imgs = imgs[None] if imgs.ndim == 2 else imgs
            shape = imgs.shape
        elif shape is None:
            shape = tuple(imgs.shape)   # a tensor
        if len(shape) != 3:
            raise ValueError(name + ": imgs is [n, h, w]")
        if interp not in _lib.WARP_INTERP:
            raise ValueError(name + ': interp must be "nearest" or "bilinear"')
        if isinstance(models, np.ndarray) and models.dtype.names:
            models = models["h"]
        if isinstance(models, (np.ndarray, list, tuple)):
            models = np.ascontiguousarray(models, np.float32).reshape(-1, 9)
            n_jobs = models.shape[0]
        else:
            n_jobs = len(src) if src is not None else int(shape[0])
        if src is not None:
            src = np.ascontiguousarray(src, np.int32).reshape(-1)
            if src.size != n_jobs:
                raise ValueError(name + ": one src index per model")
        offsets = np.array([0, n_jobs], np.int64) if offsets is None else np.ascontiguousarray(offsets, np.int64).reshape(-1)
        if offsets.size < 1 or offsets[-1] != n_jobs:
            raise ValueError(name + ": offsets has one entry per canvas and one more, the last being the number of models")
        oh, ow = (int(shape[1]), int(shape[2])) if out_shape is None else (int(out_shape[0]), int(out_shape[1]))
        if isinstance(gains, (np.ndarray, list, tuple)):
            gains = np.ascontiguousarray(gains, np.float32).reshape(-1)
            if gains.size != n_jobs:
                raise ValueError(name + ": one gain per model")
        return imgs, shape, models, n_jobs, offsets, src, (oh, ow), gains

    def composite_homography(self, imgs, models, offsets=None, src=None, out_shape=None, origin=(0, 0), fill=0.0, interp="bilinear", blend="feather",
                             path=0, out=None, count=False, want_tiles=False, shape=None, gains=None):
        """sift_hip_composite_homography: canvas c accumulates jobs offsets[c] .. offsets[c + 1] - 1 in order, job j being image
        src[j] (None: image j) under models[j] as in warp_homography -> (out[, count][, tiles]): out [n_canvases, out_h, out_w]
        float32, one picture per canvas; count uint16, the jobs that cover each pixel (0: `fill`); tiles = (staged, direct,
        skipped) (tile, job) visits with `want_tiles`.  `offsets` None: one canvas of all jobs.  `blend`: "first" (the first
        covering job's value), "mean" or "feather" (weights: distance to the source frame's border plus one).  `imgs`, `models`,
        `out_shape`, `origin`, `interp`, `path`, `shape` as in warp_homography; `out`, and `count` when it is not a bool: where
        a result goes (returned as given).  `gains` (sift_hip_composite_homography_gains): one float per job, numbers, a tensor
        or an address - a covering job's value is multiplied by its gain (overlap_stats solves them); None: no gains."""
        if blend not in _lib.COMPOSITE_BLEND:
            raise ValueError('composite_homography: blend must be "first", "mean" or "feather"')
        imgs, shape, models, n_jobs, offsets, src, (oh, ow), gains = self._composite_inputs("composite_homography", imgs, models, offsets, src, out_shape, interp,
                                                                                            shape, gains)
        prm = _lib.CompositeParams(ow, oh, int(origin[0]), int(origin[1]), float(fill), _lib.WARP_INTERP[interp], _lib.COMPOSITE_BLEND[blend], int(path) & 0xff)
        size = (offsets.size - 1, max(oh, 0), max(ow, 0))   # a bad size: the call says so
        res = np.zeros(size, np.float32) if out is None else out
        cnt = (np.zeros(size, np.uint16) if count else None) if isinstance(count, bool) else count
        tiles = np.zeros(3, np.int64) if want_tiles else None
        err = C.create_string_buffer(512)
        head = (self._h, self._addr(imgs), int(shape[0]), int(shape[2]), int(shape[1]), offsets.size - 1, self._addr(offsets), self._addr(src),
                self._addr(models), C.byref(prm))
        if gains is None:
            rc = self._L.sift_hip_composite_homography(*head, self._addr(res), self._addr(cnt), self._addr(tiles), err, 512)
        else:
            rc = self._L.sift_hip_composite_homography_gains(*head, self._addr(gains), self._addr(res), self._addr(cnt), self._addr(tiles), err, 512)
        if rc:
            _raise(rc, err)
        got = (res,) + ((cnt,) if cnt is not None else ()) + ((tuple(int(t) for t in tiles),) if want_tiles else ())
        return got[0] if len(got) == 1 else got

    # ---- two-band compositor (include/sift_hip.h, "two-band compositor") ---------------------------------------
    @staticmethod
    def band_taps(sigma: float):
        """The taps composite_twoband forms from `sigma`: the centre-to-edge half of gauss_taps(sigma) -> float32 [radius + 1]."""
        r, taps = gauss_taps(float(sigma))
        if r > _lib.TWOBAND_MAX_RADIUS:
            raise ValueError(f"composite_twoband: sigma {sigma} gives a radius of {r}, above {_lib.TWOBAND_MAX_RADIUS}")
        return np.ascontiguousarray(taps[r:], np.float32)

    def composite_twoband(self, imgs, models, offsets=None, src=None, out_shape=None, origin=(0, 0), fill=0.0, interp="bilinear", sigma=5.0, taps=None,
                          path=0, out=None, count=False, want_tiles=False, shape=None, gains=None):
        """sift_hip_composite_twoband: composite_homography's canvases and jobs blended in two frequency bands (Burt and Adelson)
        -> (out[, count][, tiles]).  A job's low band - its warped values under the separable blur `taps`, normalised by the blur
        of its coverage - is feathered; its high band, value minus low band, comes from the one covering job with the largest
        feather weight, so fine detail is not doubled where frames overlap.  `taps`: radius + 1 numbers, the weight at offsets
        +d and -d, radius at most 16; None: band_taps(`sigma`), whose radius is three sigma (sigma <= 16 / 3).  tiles =
        (general, constant-norm, skipped) (tile, job) visits with `want_tiles`; `path` 1: every visit takes the general path
        (the same bits).  Everything else as in composite_homography."""
        imgs, shape, models, n_jobs, offsets, src, (oh, ow), gains = self._composite_inputs("composite_twoband", imgs, models, offsets, src, out_shape, interp,
                                                                                            shape, gains)
        taps = self.band_taps(sigma) if taps is None else np.ascontiguousarray(taps, np.float32).reshape(-1)
        if not 1 <= taps.size <= _lib.TWOBAND_MAX_RADIUS + 1:
            raise ValueError(f"composite_twoband: taps are radius + 1 numbers, radius 0 .. {_lib.TWOBAND_MAX_RADIUS}")
        prm = _lib.TwobandParams(ow, oh, int(origin[0]), int(origin[1]), float(fill), _lib.WARP_INTERP[interp], int(path) & 0xff, taps.size - 1)
        size = (offsets.size - 1, max(oh, 0), max(ow, 0))   # a bad size: the call says so
        res = np.zeros(size, np.float32) if out is None else out
        cnt = (np.zeros(size, np.uint16) if count else None) if isinstance(count, bool) else count
        tiles = np.zeros(3, np.int64) if want_tiles else None
        err = C.create_string_buffer(512)
        rc = self._L.sift_hip_composite_twoband(self._h, self._addr(imgs), int(shape[0]), int(shape[2]), int(shape[1]), offsets.size - 1, self._addr(offsets),
                                                self._addr(src), self._addr(models), C.byref(prm), self._addr(taps), self._addr(gains), self._addr(res),
                                                self._addr(cnt), self._addr(tiles), err, 512)
        if rc:
            _raise(rc, err)
        got = (res,) + ((cnt,) if cnt is not None else ()) + ((tuple(int(t) for t in tiles),) if want_tiles else ())
        return got[0] if len(got) == 1 else got

    # ---- overlap statistics and gains (include/sift_hip.h, "overlap statistics") -------------------------------
    def overlap_stats(self, imgs, models, offsets=None, src=None, out_shape=None, origin=(0, 0), scale=1.0, interp="bilinear", gains=False,
                      sigma_n=10.0, sigma_g=0.1, path=0, shape=None, stats=None):
        """sift_hip_overlap_stats: for canvas c and its jobs offsets[c] .. offsets[c + 1] - 1 (at most 32; job j is image src[j]
        under models[j], as in composite_homography) the sums, over the canvas pixels that jobs i and j both cover, of 1, q_i,
        q_i^2 and q_i q_j with q the 8-bit intensity round(value * scale) -> stats int64 [n_canvases, 4, 32, 32] (planes N, S,
        SS, X; rows and columns past a canvas's jobs are zero); with `gains` (stats, gains, status): one float32 gain per job,
        Brown and Lowe's gain compensation with `sigma_n`, `sigma_g` on the 0 .. 255 grid, and one byte per canvas, 1 where
        the solve failed and the canvas's gains are all 1.  `scale`: 1 for frames of 0 .. 255, 255 for frames in [0, 1].
        `path` 1: every chunk of pixels is flushed by itself (the same bits).  `stats`, and `gains` when it is not a bool:
        where a result goes (returned as given).  The other arguments as in composite_homography."""
        if isinstance(imgs, np.ndarray):
            imgs = np.ascontiguousarray(imgs, np.float32)
            imgs = imgs[None] if imgs.ndim == 2 else imgs
            shape = imgs.shape
        elif shape is None:
            shape = tuple(imgs.shape)   # a tensor
        if len(shape) != 3:
            raise ValueError("overlap_stats: imgs is [n, h, w]")
        if interp not in _lib.WARP_INTERP:
            raise ValueError('overlap_stats: interp must be "nearest" or "bilinear"')
        if isinstance(models, np.ndarray) and models.dtype.names:
            models = models["h"]
        if isinstance(models, (np.ndarray, list, tuple)):
            models = np.ascontiguousarray(models, np.float32).reshape(-1, 9)
            n_jobs = models.shape[0]
        else:
            n_jobs = len(src) if src is not None else int(shape[0])
        if src is not None:
            src = np.ascontiguousarray(src, np.int32).reshape(-1)
            if src.size != n_jobs:
                raise ValueError("overlap_stats: one src index per model")
        offsets = np.array([0, n_jobs], np.int64) if offsets is None else np.ascontiguousarray(offsets, np.int64).reshape(-1)
        if offsets.size < 1 or offsets[-1] != n_jobs:
            raise ValueError("overlap_stats: offsets has one entry per canvas and one more, the last being the number of models")
        oh, ow = (int(shape[1]), int(shape[2])) if out_shape is None else (int(out_shape[0]), int(out_shape[1]))
        prm = _lib.OverlapParams(ow, oh, int(origin[0]), int(origin[1]), float(scale), float(sigma_n), float(sigma_g), _lib.WARP_INTERP[interp], int(path) & 0xff)
        res = np.zeros((offsets.size - 1, 4, _lib.OVERLAP_MAX_JOBS, _lib.OVERLAP_MAX_JOBS), np.int64) if stats is None else stats
        g = (np.ones(n_jobs, np.float32) if gains else None) if isinstance(gains, bool) else gains
        status = np.zeros(offsets.size - 1, np.uint8) if g is not None else None
        err = C.create_string_buffer(512)
        rc = self._L.sift_hip_overlap_stats(self._h, self._addr(imgs), int(shape[0]), int(shape[2]), int(shape[1]), offsets.size - 1, self._addr(offsets),
                                            self._addr(src), self._addr(models), C.byref(prm), self._addr(res), self._addr(g), self._addr(status), err, 512)
        if rc:
            _raise(rc, err)
        return res if g is None else (res, g, status)

    @staticmethod
    def overlap_zncc(stats, n):
        """The zero-mean normalised cross-correlation of every pair of the first `n` jobs of ONE canvas's `stats` [4, 32, 32]
        over the pair's overlap, host numpy in float64: (N X - S_ij S_ji) / sqrt((N SS_ij - S_ij^2) (N SS_ji - S_ji^2)), NaN
        where a factor is <= 0 (no overlap, or a constant frame there)."""
        N, S, SS, X = (np.asarray(stats)[k, :n, :n].astype(np.float64) for k in range(4))
        vi, vj = N * SS - S * S, N * SS.T - S.T * S.T
        with np.errstate(all="ignore"):
            return np.where((vi > 0) & (vj > 0), (N * X - S * S.T) / np.sqrt(vi * vj), np.nan)


class Group:
    """sift_hip_group: one batch block-sharded over several GPUs of this node from one process (one context and host thread
    per entry of `devices`; a device may be listed more than once), keypoint lists gathered device-to-device on devices[0] in
    global image order (include/sift_hip.h)."""

    def __init__(self, devices):
        self._L = _lib.load()
        self._h = C.c_void_p()
        devs = (C.c_int * len(devices))(*devices)
        err = C.create_string_buffer(512)
        rc = self._L.sift_hip_group_create(devs, len(devices), C.byref(self._h), err, 512)
        if rc:
            self._h = C.c_void_p()
            _raise(rc, err)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.sift_hip_group_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, name: str, value: int):
        if self._L.sift_hip_group_set_option(self._h, name.encode(), int(value)):
            raise ValueError(f"unknown option {name}")

    def calculate_batch(self, imgs, params, raise_on_error=True):
        imgs = np.ascontiguousarray(imgs, dtype=np.float32)
        n, h, w = imgs.shape
        err = C.create_string_buffer(512)
        rc = self._L.sift_hip_group_calculate(self._h, imgs.reshape(-1), n, w, h, C.byref(params), err, 512)
        if rc and raise_on_error:
            _raise(rc, err)
        return rc, err.value.decode(errors="replace")

    def submit(self, imgs, params):
        """Start a batch and return at once (at most two in flight); `collect()` waits for the oldest one.  The gather of a batch
        runs under the kernels of the next."""
        imgs = np.ascontiguousarray(imgs, dtype=np.float32)
        n, h, w = imgs.shape
        err = C.create_string_buffer(512)
        rc = self._L.sift_hip_group_submit(self._h, imgs.reshape(-1), n, w, h, C.byref(params), err, 512)
        if rc:
            _raise(rc, err)
        self._inflight = getattr(self, "_inflight", []) + [imgs]    # the frames stay alive until their batch is collected

    def collect(self, raise_on_error=True):
        err = C.create_string_buffer(512)
        rc = self._L.sift_hip_group_collect(self._h, err, 512)
        if getattr(self, "_inflight", None):
            self._inflight.pop(0)
        if rc and raise_on_error:
            _raise(rc, err)
        return rc, err.value.decode(errors="replace")

    def transport(self):
        """(1 if the gather runs over RCCL else 0, why)"""
        text = C.create_string_buffer(256)
        return int(self._L.sift_hip_group_transport(self._h, text, 256)), text.value.decode(errors="replace")

    def gather_exposed_ms(self):
        v = C.c_double()
        if self._L.sift_hip_group_gather_exposed(self._h, C.byref(v)):
            raise HipError("no batch collected")
        return v.value

    def counts(self):
        out = np.zeros(max(self._L.sift_hip_group_result_images(self._h), 0), np.int32)
        if self._L.sift_hip_group_result_counts(self._h, out, out.size):
            raise HipError("no result")
        return out

    def status(self):
        out = np.zeros(max(self._L.sift_hip_group_result_images(self._h), 0), np.int32)
        if self._L.sift_hip_group_result_status(self._h, out, out.size):
            raise HipError("no result")
        return out

    def total(self) -> int:
        return int(self._L.sift_hip_group_result_total(self._h))

    def results(self):
        t = max(self.total(), 0)
        kp = np.zeros(t, _lib.KEYPOINT_DTYPE)
        desc = np.zeros((t, 128), np.float32)
        if t and self._L.sift_hip_group_result_copy(self._h, kp.ctypes.data, desc.ctypes.data):
            raise HipError("sift_hip_group_result_copy failed")
        return kp, desc

    def timing(self):
        """(ms in the shards' calculate calls, ms in the gather, bytes that crossed devices) of the last batch"""
        a, b, n = C.c_double(), C.c_double(), C.c_int64()
        if self._L.sift_hip_group_timing(self._h, C.byref(a), C.byref(b), C.byref(n)):
            raise HipError("no result")
        return a.value, b.value, n.value


def lock_wait_ms() -> float:
    """Time this process's host threads have spent waiting for the library's per-device launch locks (sift_hip_lock_wait_ms)."""
    v = C.c_double()
    if _lib.load().sift_hip_lock_wait_ms(C.byref(v)):
        raise HipError("sift_hip_lock_wait_ms failed")
    return v.value


def unpack_sparse_host(rec, val, kp_out=None, desc_out=None, threads: int = 8):
    """Sparse wire format in host memory -> (keypoints, descriptors [n, 128]), bit for bit what Context.results returns
    (sift_hip_sparse_unpack_host: plain host code, `threads` threads)."""
    L = _lib.load()
    rec = np.ascontiguousarray(rec, np.uint8).reshape(-1, 34)
    val = np.ascontiguousarray(val, np.float32)
    n = rec.shape[0]
    kp = np.zeros(n, _lib.KEYPOINT_DTYPE) if kp_out is None else kp_out.reshape(-1)[:n]
    desc = np.empty((n, 128), np.float32) if desc_out is None else desc_out.reshape(-1, 128)[:n]
    if L.sift_hip_sparse_unpack_host(rec.ctypes.data, val.ctypes.data, n, kp.ctypes.data, desc.ctypes.data, int(threads)):
        raise HipError("sift_hip_sparse_unpack_host failed")
    return kp, desc


def gauss_taps(sigma: float):
    L = _lib.load()
    buf = np.zeros(8192, np.float32)
    r = L.sift_hip_gauss_taps(sigma, buf, buf.size)
    if r < 0:
        raise PreconditionViolation("Kernel1D::initGaussian(): Standard deviation must be >= 0.")
    return r, buf[:2 * r + 1].copy()


class Sift:
    """sift::Sift (sift.hpp:17-78): Sift(dogsPerEpoch=3, octaves=3, sigma=1.6, k=sqrt(2), subpixel=False)."""

    def __init__(self, dogsPerEpoch: int = 3, octaves: int = 3, sigma: float = 1.6, k: float = K_SQRT2,
                 subpixel: bool = False, device: int = 0, context: Context | None = None):
        self.subpixel = bool(subpixel)
        self._params = _lib.Params(dogsPerEpoch, octaves, sigma, k, 1 if subpixel else 0)
        self.ctx = context or Context(device)

    @property
    def params(self):
        return self._params

    def calculate(self, img: np.ndarray):
        """Returns (points, img): the InterestPoint list and the image the reference leaves in the
        caller's array (the 2x upsampled one when subpixel, sift.cpp:20-21)."""
        img = np.asarray(img)
        img = np.ascontiguousarray(img, np.uint8 if img.dtype == np.uint8 else np.float32)   # uint8: widened on the GPU
        try:
            self.ctx.calculate_batch(img[None], self._params)
        finally:
            self.image = self.ctx.image(0) if self.subpixel else img
        sparse = self.ctx.results_sparse() if self.ctx.total() > 0 else None    # ~200 instead of 532 bytes per keypoint over the link
        kp, desc = unpack_sparse_host(*sparse, threads=1) if sparse is not None else self.ctx.results()
        pts = [InterestPoint(float(k["scale"]), int(k["octave"]), int(k["index"]), bool(k["filtered"]),
                             (int(k["x"]), int(k["y"])), float(k["orientation"]),
                             desc[i].tolist() if k["has_descriptor"] else [])
               for i, k in enumerate(kp)]
        return pts

    def calculate_batch(self, imgs: np.ndarray):
        """Batch of independent frames -> (counts, keypoints structured array, descriptors [N,128])."""
        self.ctx.calculate_batch(imgs, self._params)
        kp, desc = self.ctx.results()
        return self.ctx.counts(), kp, desc

    def _coords(self, points, which, localized, side):
        """Image coordinates [len(which), 2] of points[which]: loc * 2^octave (halved with subpixel), or the x, y of the side's
        records when `localized` is a pair of LOCALIZED_DTYPE arrays (Context.localize() after the calculate() of each list)."""
        which = np.asarray(which, np.int64)
        if localized is not None:
            if len(localized) != 2 or len(localized[side]) != len(points):
                raise ValueError("localized is a pair of record arrays, one record per point")
            return np.stack([localized[side]["x"][which], localized[side]["y"][which]], axis=1).astype(np.float32).reshape(-1, 2)
        xy = np.array([[points[i].loc[0] << points[i].octave, points[i].loc[1] << points[i].octave] for i in which], np.float32)
        return xy.reshape(-1, 2) * np.float32(0.5 if self.subpixel else 1.0)

    def match(self, points_a, points_b, ratio: float = 0.8, cross_check: bool = False, quantized: bool = False):
        """Matches between two InterestPoint lists (an extension: the reference has no matcher) -> records (query, train,
        dist2, second2), indices into the lists.  A point without a 128-float descriptor is an invalid row.  `quantized`: the
        descriptors are quantised to 8 bits on the GPU and matched by the integer distance (dist2 / second2 are integers)."""
        def rows(points):
            d = np.zeros((len(points), 128), np.float32)
            kp = np.zeros(len(points), _lib.KEYPOINT_DTYPE)
            for i, p in enumerate(points):
                if len(p.descriptors) == 128:
                    d[i] = p.descriptors
                    kp["has_descriptor"][i] = 1
            return d, kp
        qa, ka = rows(points_a)
        qb, kb = rows(points_b)
        return self.ctx.match(qa, qb, ratio, cross_check, ka, kb, quantized)

    def verify(self, points_a, points_b, ratio: float = 0.8, cross_check: bool = False, iterations: int = 2048, threshold: float = 3.0,
               seed: int = 0, refine: int = 0, model: str = "homography", quantized: bool = False, localized=None):
        """match() followed by the geometric check of its list (an extension) -> (records, model, inlier): the best four-point
        homography from image a to image b over the matches' image coordinates (loc * 2^octave, halved with subpixel), as one
        record (h [9] row-major, inliers, iteration; -1: none, refined), and one flag per record.  `refine`: rounds of
        least-squares re-estimation over the inliers, 0 .. 8 (0: the minimal-sample model).  model="fundamental": the best
        seven-point fundamental matrix instead, (tb, 1) F (ta, 1)^T = 0, as one record (f [9], inliers, iteration, root); the
        right model for two views of a general scene, where a homography explains one plane only.  `refine` must then be 0.
        `localized`: a pair of LOCALIZED_DTYPE arrays, the records ctx.localize() returned after the calculate() of each list;
        the coordinates are then the records' sub-pixel x, y."""
        if model not in ("homography", "fundamental"):
            raise ValueError('verify: model must be "homography" or "fundamental"')
        recs = self.match(points_a, points_b, ratio, cross_check, quantized)
        pts = np.concatenate([self._coords(points_a, recs["query"], localized, 0), self._coords(points_b, recs["train"], localized, 1)], axis=1)
        run = self.ctx.ransac_fundamental if model == "fundamental" else self.ctx.ransac_homography
        models, inlier = run(pts, None, iterations, threshold, seed, refine=refine)
        return recs, models[0], inlier

    def register(self, imgs, pairs, ratio: float = 0.8, cross_check: bool = False, iterations: int = 2048, threshold: float = 3.0, seed: int = 0,
                 refine: int = 0, quantized: bool = False, fill: float = 0.0, interp: str = "bilinear", align: int = 0):
        """Registration (an extension): calculate() on every frame of `imgs` [n, h, w], verify() on every pair (query, train) and
        Context.warp_homography of each pair's train frame into its query frame -> (models, registered, mask): one homography
        record per pair, registered[p] the train frame resampled on the query frame's pixels, mask[p] 1 where it is covered
        (elsewhere `fill`; a pair without a model is all `fill`).  Bit for bit the composition of those calls.  `align` > 0:
        Context.align_homography(rounds=align) refines every pair's model on the pixels before the warp."""
        imgs = np.asarray(imgs)
        if imgs.ndim != 3:
            raise ValueError("register: imgs is [n, h, w]")
        pairs = [(int(q), int(t)) for q, t in pairs]
        points = [self.calculate(img) for img in imgs]
        models = np.zeros(len(pairs), _lib.HOMOGRAPHY_DTYPE)
        for p, (q, t) in enumerate(pairs):
            models[p] = self.verify(points[q], points[t], ratio, cross_check, iterations, threshold, seed, refine, "homography", quantized)[1]
        if align:
            models = self.ctx.align_homography(imgs.astype(np.float32), pairs, models, rounds=align)[0]
        registered, mask = self.ctx.warp_homography(imgs.astype(np.float32), models, [t for _, t in pairs], fill=fill, interp=interp, mask=True)
        return models, registered, mask

    @staticmethod
    def mosaic_canvas(models, w: int, h: int):
        """The canvas mosaic() chooses -> (origin (x, y), shape (out_h, out_w)): in float64, the box of the w x h reference frame
        and of every model's frame corners through the inverse model, each side clipped to 4 x the frame's larger side around
        the reference frame (a frame with a corner at or behind the horizon reaches as far as allowed)."""
        reach = 4 * max(w, h)
        lo, hi = np.array([-reach, -reach], np.float64), np.array([w - 1 + reach, h - 1 + reach], np.float64)
        box_lo, box_hi = np.zeros(2), np.array([w - 1, h - 1], np.float64)
        corners = np.array([[0, 0, 1], [w - 1, 0, 1], [0, h - 1, 1], [w - 1, h - 1, 1]], np.float64).T
        for m in np.asarray(models, np.float64).reshape(-1, 3, 3):
            with np.errstate(all="ignore"):
                c = np.linalg.inv(m) @ corners if abs(np.linalg.det(m)) > 0 else np.full((3, 4), np.nan)
                xy = c[:2] / c[2]
            if not (np.isfinite(xy).all() and (c[2] * c[2, 0] > 0).all()):
                box_lo, box_hi = lo.copy(), hi.copy()
                continue
            box_lo, box_hi = np.minimum(box_lo, np.floor(xy.min(axis=1))), np.maximum(box_hi, np.ceil(xy.max(axis=1)))
        box_lo, box_hi = np.clip(box_lo, lo, hi), np.clip(box_hi, lo, hi)
        return (int(box_lo[0]), int(box_lo[1])), (int(box_hi[1] - box_lo[1]) + 1, int(box_hi[0] - box_lo[0]) + 1)

    def mosaic(self, imgs, ref: int = 0, pairs=None, blend: str = "feather", ratio: float = 0.8, cross_check: bool = False, iterations: int = 2048,
               threshold: float = 3.0, seed: int = 0, refine: int = 0, quantized: bool = False, fill: float = 0.0, interp: str = "bilinear",
               chain: bool = False, canvas=None, gain: bool = False, scale: float = 1.0, band_sigma: float = 5.0, align: int = 0):
        """A mosaic or a stack (an extension): calculate() on every frame of `imgs` [n, h, w], verify() on every pair (query,
        train) and Context.composite_homography of the placed frames on one canvas in frame `ref`'s coordinates -> (models,
        canvas, count, origin): one homography record per pair, the picture [out_h, out_w], the number of frames that cover each
        pixel (0: `fill`), and origin (x, y), the lattice point of `ref` at canvas pixel (0, 0).  `pairs`: (ref, k) for every
        other frame k by default, and every query must be `ref`; with `chain` the pairs are taken in order, each query being
        `ref` or an earlier pair's train frame, and a frame's model to `ref` is the float64 product along its chain, rounded
        once to float.  Job 0 is frame `ref` under the identity, then the train frames in the pairs' order; a frame without a
        model (or behind one in its chain) is left out, and a frame is placed once, by its first pair.  `canvas` None: the box, computed in float64, of every placed frame's
        corners through its inverse model, each side clipped to 4 x the frame's larger side around frame `ref`; else (origin,
        shape) = ((x, y), (out_h, out_w)).  Bit for bit the composition of those calls.  `gain`: Context.overlap_stats(gains=True, scale=`scale`)
        on the same canvas first, the gains given to the compositor -> (models, canvas, count, origin, gains, zncc): one gain
        per placed frame in job order and Context.overlap_zncc of the placed frames (at most 32).  `blend` "twoband":
        Context.composite_twoband(sigma=`band_sigma`) in the compositor's place, also together with `gain`.  `align` > 0:
        Context.align_homography(rounds=align) refines every pair's model on the pixels of its two frames before the chain
        product and the choice of the canvas."""
        imgs = np.asarray(imgs)
        if imgs.ndim != 3:
            raise ValueError("mosaic: imgs is [n, h, w]")
        n, h, w = imgs.shape
        ref = int(ref)
        pairs = [(ref, k) for k in range(n) if k != ref] if pairs is None else [(int(q), int(t)) for q, t in pairs]
        to_ref = {ref: np.eye(3)}   # frame -> the float64 model from ref's lattice to the frame, as far as it is exact
        for q, t in pairs:
            if not chain and q != ref:
                raise ValueError("mosaic: without chain every pair's query is the reference frame")
        points = [self.calculate(img) for img in imgs]
        models = np.zeros(len(pairs), _lib.HOMOGRAPHY_DTYPE)
        job_models, src = [np.eye(3, dtype=np.float32).reshape(9)], [ref]
        for p, (q, t) in enumerate(pairs):
            models[p] = self.verify(points[q], points[t], ratio, cross_check, iterations, threshold, seed, refine, "homography", quantized)[1]
        if align:
            models = self.ctx.align_homography(imgs.astype(np.float32), pairs, models, rounds=align)[0]
        for p, (q, t) in enumerate(pairs):
            if models[p]["iteration"] < 0 or q not in to_ref or t in to_ref:
                continue
            to_ref[t] = models[p]["h"].astype(np.float64).reshape(3, 3) @ to_ref[q]
            job_models.append(models[p]["h"] if q == ref else to_ref[t].astype(np.float32).reshape(9))
            src.append(t)
        job_models = np.array(job_models, np.float32)
        if canvas is None:
            origin, shape = self.mosaic_canvas(job_models[1:], w, h)
        else:
            origin, shape = (int(canvas[0][0]), int(canvas[0][1])), (int(canvas[1][0]), int(canvas[1][1]))
        def compose(gains):
            if blend == "twoband":
                return self.ctx.composite_twoband(imgs.astype(np.float32), job_models, None, src, shape, origin, fill, interp, band_sigma, count=True, gains=gains)
            return self.ctx.composite_homography(imgs.astype(np.float32), job_models, None, src, shape, origin, fill, interp, blend, count=True, gains=gains)

        if gain:
            stats, gains, _ = self.ctx.overlap_stats(imgs.astype(np.float32), job_models, None, src, shape, origin, scale, interp, gains=True)
            out, count = compose(gains)
            return models, out[0], count[0], origin, gains, self.ctx.overlap_zncc(stats[0], len(src))
        out, count = compose(None)
        return models, out[0], count[0], origin

    def refine_fundamental(self, points_a, points_b, recs, model, threshold: float = 3.0, rounds: int = 2, localized=None):
        """The least-squares refit of the record verify(model="fundamental") returned, over its own inliers among `recs` (an
        extension; Context.refine_fundamental) -> (model, refined, inlier): at most `rounds` (0 .. 8) rounds of which `refined`
        were accepted; the inlier count never decreases.  Coordinates, and `localized`, as for verify()."""
        if "f" not in (getattr(getattr(model, "dtype", None), "names", None) or ()):
            raise ValueError("refine_fundamental: model must be a record as verify(model=\"fundamental\") returns it")
        pts = np.concatenate([self._coords(points_a, recs["query"], localized, 0), self._coords(points_b, recs["train"], localized, 1)], axis=1)
        models, refined, inlier = self.ctx.refine_fundamental(pts, None, np.asarray(model).reshape(1), threshold, rounds)
        return models[0], int(refined[0]), inlier

    def match_guided(self, points_a, points_b, model, threshold: float = 3.0, ratio: float = 0.8, cross_check: bool = False, localized=None,
                     quantized: bool = False):
        """match() again under the model verify() returned (an extension): a point of b competes for a point of a only when it
        lies within `threshold` pixels of the model - of the transferred point (a homography record) or of the epipolar line (a
        fundamental record).  Coordinates, and `localized`, as for verify().  A model that is none (all zeros) gives no records.
        `quantized`: the descriptors are quantised to 8 bits on the GPU and matched by the integer distance, as for match()."""
        names = getattr(getattr(model, "dtype", None), "names", None) or ()
        if "h" not in names and "f" not in names:
            raise ValueError("match_guided: model must be a record as verify() returns it")
        kind = "homography" if "h" in names else "fundamental"

        def rows(points, side):
            d = np.zeros((len(points), 128), np.float32)
            kp = np.zeros(len(points), _lib.KEYPOINT_DTYPE)
            for i, p in enumerate(points):
                if len(p.descriptors) == 128:
                    d[i] = p.descriptors
                    kp["has_descriptor"][i] = 1
            return d, kp, self._coords(points, range(len(points)), localized, side)
        qa, ka, xa = rows(points_a, 0)
        qb, kb, xb = rows(points_b, 1)
        m9 = np.asarray(model["h" if kind == "homography" else "f"], np.float32)
        if quantized:
            return self.ctx.match_guided_u8(self.ctx.quantize(qa), self.ctx.quantize(qb), xa, xb, m9, kind, threshold, ratio, cross_check, ka, kb)
        return self.ctx.match_guided(qa, qb, xa, xb, m9, kind, threshold, ratio, cross_check, ka, kb)
