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
        offsets = np.ascontiguousarray(offsets, np.int64)
        pq, pt = self._pairs(pairs)
        rows = int(sum(offsets[q + 1] - offsets[q] for q in pq if 0 <= q < offsets.size - 1))
        idx = np.full((rows, 2), -1, np.int32) if idx_out is None else idx_out
        dist = np.full((rows, 2), np.inf, np.float32) if dist_out is None else dist_out
        if isinstance(desc, np.ndarray):
            desc = np.ascontiguousarray(desc, np.float32)
        if isinstance(xy, np.ndarray):
            xy = np.ascontiguousarray(xy, np.float32)
        prm = self._guide(model, threshold)
        models = self._models9(models, pq.size)
        err = C.create_string_buffer(512)
        rc = self._L.sift_hip_knn2_guided(self._h, self._addr(desc), self._addr(kp), self._addr(xy), offsets.size - 1, offsets, pq.size, pq, pt,
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
        match_sets.  Guided matching takes float rows only: `quantized=True` is a ValueError (the call says so)."""
        offsets = np.ascontiguousarray(offsets, np.int64)
        pq, pt = self._pairs(pairs)
        rows = int(sum(offsets[q + 1] - offsets[q] for q in pq if 0 <= q < offsets.size - 1))
        recs = np.zeros(rows, _lib.MATCH_DTYPE) if recs_out is None else recs_out
        counts = np.zeros(pq.size, np.int32)
        total = C.c_int64()
        if isinstance(desc, np.ndarray):
            desc = np.ascontiguousarray(desc, np.float32)
        if isinstance(xy, np.ndarray):
            xy = np.ascontiguousarray(xy, np.float32)
        mprm = _lib.MatchParams(float(ratio), 1 if cross_check else 0, self._quantized(quantized))
        gprm = self._guide(model, threshold)
        models = self._models9(models, pq.size)
        err = C.create_string_buffer(512)
        rc = self._L.sift_hip_match_guided(self._h, self._addr(desc), self._addr(kp), self._addr(xy), offsets.size - 1, offsets, pq.size, pq, pt,
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

    def match_images_guided(self, pairs, models, model="homography", threshold=3.0, ratio=0.8, cross_check=False, quantized=False):
        """sift_hip_result_match_guided: match_images under the pairs' models, e.g. those verify_images returned, on the
        device-resident results (the keypoints' image coordinates are built on the GPU) -> (records, counts).  `quantized=True`
        is a ValueError, as for match_guided_sets."""
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
        rc = self._L.sift_hip_result_match_guided(self._h, pq.size, pq, pt, C.byref(mprm), C.byref(gprm), self._addr(models),
                                                  C.c_void_p(recs.ctypes.data), counts, C.byref(total), err, 512)
        if rc:
            _raise(rc, err)
        return recs[:total.value], counts

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

    def verify_images(self, pairs, ratio=0.8, cross_check=False, iterations=2048, threshold=3.0, seed=0, refine=0, model="homography",
                      quantized=False):
        """sift_hip_result_verify: match_images followed by ransac_homography on the matches' image coordinates, all on the
        device-resident results -> (records, counts, models, inlier): models[p] belongs to pair p, inlier[i] to records[i].
        `refine` as for ransac_homography.  model="fundamental": sift_hip_result_verify_fundamental, ransac_fundamental in
        place of ransac_homography (models of FUNDAMENTAL_DTYPE; `refine` must be 0).  `quantized` as for match_images."""
        if model not in ("homography", "fundamental"):
            raise ValueError('verify_images: model must be "homography" or "fundamental"')
        fund = model == "fundamental"
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
               seed: int = 0, refine: int = 0, model: str = "homography", quantized: bool = False):
        """match() followed by the geometric check of its list (an extension) -> (records, model, inlier): the best four-point
        homography from image a to image b over the matches' image coordinates (loc * 2^octave, halved with subpixel), as one
        record (h [9] row-major, inliers, iteration; -1: none, refined), and one flag per record.  `refine`: rounds of
        least-squares re-estimation over the inliers, 0 .. 8 (0: the minimal-sample model).  model="fundamental": the best
        seven-point fundamental matrix instead, (tb, 1) F (ta, 1)^T = 0, as one record (f [9], inliers, iteration, root); the
        right model for two views of a general scene, where a homography explains one plane only.  `refine` must then be 0."""
        if model not in ("homography", "fundamental"):
            raise ValueError('verify: model must be "homography" or "fundamental"')
        recs = self.match(points_a, points_b, ratio, cross_check, quantized)
        scale = np.float32(0.5 if self.subpixel else 1.0)

        def coords(points, which):
            xy = np.array([[points[i].loc[0] << points[i].octave, points[i].loc[1] << points[i].octave] for i in which], np.float32)
            return xy.reshape(-1, 2) * scale
        pts = np.concatenate([coords(points_a, recs["query"]), coords(points_b, recs["train"])], axis=1)
        run = self.ctx.ransac_fundamental if model == "fundamental" else self.ctx.ransac_homography
        models, inlier = run(pts, None, iterations, threshold, seed, refine=refine)
        return recs, models[0], inlier

    def match_guided(self, points_a, points_b, model, threshold: float = 3.0, ratio: float = 0.8, cross_check: bool = False):
        """match() again under the model verify() returned (an extension): a point of b competes for a point of a only when it
        lies within `threshold` pixels of the model - of the transferred point (a homography record) or of the epipolar line (a
        fundamental record).  Coordinates as verify() forms them.  A model that is none (all zeros) gives no records."""
        names = getattr(getattr(model, "dtype", None), "names", None) or ()
        if "h" not in names and "f" not in names:
            raise ValueError("match_guided: model must be a record as verify() returns it")
        kind = "homography" if "h" in names else "fundamental"
        scale = np.float32(0.5 if self.subpixel else 1.0)

        def rows(points):
            d = np.zeros((len(points), 128), np.float32)
            kp = np.zeros(len(points), _lib.KEYPOINT_DTYPE)
            xy = np.zeros((len(points), 2), np.float32)
            for i, p in enumerate(points):
                xy[i] = (p.loc[0] << p.octave, p.loc[1] << p.octave)
                if len(p.descriptors) == 128:
                    d[i] = p.descriptors
                    kp["has_descriptor"][i] = 1
            return d, kp, xy * scale
        qa, ka, xa = rows(points_a)
        qb, kb, xb = rows(points_b)
        return self.ctx.match_guided(qa, qb, xa, xb, np.asarray(model["h" if kind == "homography" else "f"], np.float32), kind, threshold,
                                     ratio, cross_check, ka, kb)
