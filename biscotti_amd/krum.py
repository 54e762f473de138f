"""Host-side mirror of Biscotti's Multi-Krum verifier interface, on libbk.

Reference surface kept (same names, argument meaning and error behaviour):

  krum(deltas, clip)              ML/code/logistic_validator.py:36-49
                                  (== ML/Pytorch/client_obj.py:114-127)
  get_krum_scores(X, groupsize)   ML/code/logistic_validator.py:54-65
  KRUMValidator                   DistSys/krum.go:22-29
    .initialize()                 krum.go:31-44   (binds the engine instead of pyKRUMFunc)
    .check_if_accepted(peer_id)   krum.go:47-73
    .compute_scores()             krum.go:77-98
    .get_top_krum_index(deltas)   krum.go:100-166 (the go-python call this engine replaces)
    .flush_collected_updates()    krum.go:169-176
    .add_update(u)                krum.go:291     (the append; collect=True streams it)
  Update                          DistSys/update.go:13-22

Differences a caller can observe, all documented in DESIGN.md:
  * the selected indices come back ascending (a set; numpy returns
    argpartition order, and the only consumer tests membership);
  * ties at the selection boundary resolve to the lower index;
  * clip = 0 raises ValueError, as np.argpartition does in the reference.

Everything runs through libbk.so on the GPU; there is no CPU path.
"""
from dataclasses import dataclass, field
from typing import List, Optional

import ctypes
import numpy as np

from . import _lib
from ._lib import check, lib

__all__ = ["Engine", "krum", "krum_batch", "get_krum_scores", "krum_mean", "KRUMValidator",
           "Update", "default_engine"]


def _p(x):
    return ctypes.c_void_p(x) if x is not None else None


def _as_rows(X):
    X = np.asarray(X)
    if X.dtype not in (np.float64, np.float32):
        X = X.astype(np.float64)
    if X.ndim != 2:
        raise ValueError("deltas must be 2-D (n updates x d)")
    if X.strides[1] != X.itemsize or X.strides[0] % X.itemsize:
        X = np.ascontiguousarray(X)
    return X


def _dtype_code(dt):
    return _lib.BK_F32 if dt == np.float32 else _lib.BK_F64


def _ptr(a):
    """a's address, or None for an output that was not asked for."""
    return a.ctypes.data if a is not None else None


def _ptr_array(arrays):
    return (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def _row(r, dt, d, what="every row"):
    a = np.asarray(r)
    if a.dtype != dt or a.ndim != 1 or a.shape[0] != d:
        raise ValueError("%s must be a 1-D %s array of length %d" % (what, dt, d))
    return a if a.flags.c_contiguous else np.ascontiguousarray(a)


def _outs(n, d, f, want_scores, want_mean, batch=None):
    """bk_check_args, then a call's outputs (sel, scores, mean), the last two
    None when not wanted; batch: of B problems of this shape."""
    check(lib().bk_check_args(n, d, f))
    lead = () if batch is None else (batch,)
    sel = np.empty(lead + (n - f,), dtype=np.int64)
    sc = np.empty(lead + (n,), dtype=np.float64) if want_scores else None
    mean = np.empty(lead + (d,), dtype=np.float64) if want_mean else None
    return sel, sc, mean


def _noise_arg(delta, noise, dt, d):
    """One noised update as the collection takes it: delta (d,), the noise as a
    (k, d) array (None: k = 0) and its k row pointers (None when k = 0)."""
    if dt != np.float64:
        raise ValueError("noise is float64 only: the collection is %s" % dt)
    D = np.ascontiguousarray(delta, dtype=np.float64)
    if D.ndim != 1 or D.shape[0] != d:
        raise ValueError("delta must be a 1-D float64 array of length %d" % d)
    if noise is None:
        N = np.empty((0, d), dtype=np.float64)
    else:
        N = np.ascontiguousarray(noise, dtype=np.float64)
        if N.ndim == 1:
            N = N.reshape(1, -1)
        if N.ndim != 2 or (N.shape[0] > 0 and N.shape[1] != d):
            raise ValueError("noise must be None, a vector of length %d or a (k, %d) array"
                             % (d, d))
    return D, N, _ptr_array(list(N)) if len(N) else None


def _fs_arg(fs, B):
    """fs as B int64s (an int: the same f for all) and nothing else."""
    if np.ndim(fs) == 0:
        fs = [int(fs)] * B
    fs = np.ascontiguousarray(fs, dtype=np.int64)
    if fs.ndim != 1 or fs.shape[0] != B:
        raise ValueError("fs must be an int or one f per problem (%d problems)" % B)
    return fs


def _offsets(ns):
    offsets = np.zeros(len(ns) + 1, dtype=np.int64)
    np.cumsum(ns, out=offsets[1:])
    return offsets


def _ragged_outs(ns, fs, d, want_scores, want_mean):
    """A ragged call's outputs (sel, the m per problem, scores, mean), with room
    for every problem even where a check in the library would refuse the call."""
    B = len(ns)
    sel = np.empty(max(int(np.maximum(ns - fs, 0).sum()), 1), dtype=np.int64)
    mo = np.zeros(B, dtype=np.int64)
    sc = np.empty(max(int(ns.sum()), 1), dtype=np.float64) if want_scores else None
    mean = np.empty((B, max(d, 1)), dtype=np.float64) if want_mean else None
    return sel, mo, sc, mean


def _ragged_unpack(sel, mo, sc, offsets):
    """The packed sel and scores as one copy per problem (scores None stays None)."""
    so = _offsets(mo)
    B = len(mo)
    sels = [sel[so[b]:so[b + 1]].copy() for b in range(B)]
    scs = [sc[offsets[b]:offsets[b + 1]].copy() for b in range(B)] if sc is not None else None
    return sels, scs


class GroupEngine:
    """One process driving G GPUs (bk_group_*): the Go verifier's multi-GPU
    form.  Each device copies its column shard of the host batch over its own
    PCIe link; the partial Grams are summed (RCCL all-reduce, RCCL all-gather
    + fixed-order sum, or a fixed-order sum through pinned host memory); every
    device selects identically and writes the mean of its columns."""

    def __init__(self, devices, mode=_lib.BK_GROUP_ALLREDUCE):
        devices = [int(x) for x in devices]
        arr = (ctypes.c_int * len(devices))(*devices)
        self._g = ctypes.c_void_p()
        check(lib().bk_group_create(ctypes.byref(self._g), len(devices), arr, int(mode)))
        self.devices = devices

    def close(self):
        if self._g:
            lib().bk_group_destroy(self._g)
            self._g = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def size(self):
        return lib().bk_group_size(self._g)

    def ctx(self, r):
        return lib().bk_group_ctx(self._g, int(r))

    def multikrum(self, X, f, want_scores=True, want_mean=True, pinned=False):
        """bk_group_multikrum on a host batch: (sel ascending, scores, mean)."""
        X = _as_rows(X)
        n, d = X.shape
        f = int(f)
        sel, sc, mean = _outs(n, d, f, want_scores, want_mean)
        mo = ctypes.c_int64(0)
        check(lib().bk_group_multikrum(self._g, X.ctypes.data,
                                       _lib.BK_HOST_PINNED if pinned else _lib.BK_HOST,
                                       _dtype_code(X.dtype), n, d, X.strides[0] // X.itemsize, f,
                                       sel.ctypes.data, ctypes.addressof(mo), _ptr(sc), _ptr(mean)))
        assert mo.value == n - f
        return sel, sc, mean


class Engine:
    """One libbk context (bk_ctx) bound to one GPU."""

    def __init__(self, device=0):
        self._ctx = ctypes.c_void_p()
        check(lib().bk_create(ctypes.byref(self._ctx), int(device)))
        self.device = int(device)

    def close(self):
        if self._ctx:
            lib().bk_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def ctx(self):
        return self._ctx

    # ---- host entry (bk_multikrum): numpy in, numpy out -----------------
    def multikrum(self, X, f, want_scores=True, want_mean=True):
        X = _as_rows(X)
        n, d = X.shape
        f = int(f)
        sel, sc, mean = _outs(n, d, f, want_scores, want_mean)
        mo = ctypes.c_int64(0)
        check(lib().bk_multikrum(self._ctx, X.ctypes.data, _lib.BK_HOST, _dtype_code(X.dtype), n,
                                 d, X.strides[0] // X.itemsize, f, sel.ctypes.data,
                                 ctypes.addressof(mo), _ptr(sc), _ptr(mean)))
        assert mo.value == n - f
        return sel, sc, mean

    # ---- row-fed host entry (bk_multikrum_rows): n separate host rows, ---
    #      as the Go verifier holds them (deltas [][]float64, krum.go:100-166)
    def multikrum_rows(self, rows, f, want_scores=True, want_mean=True):
        """rows: a sequence of n 1-D arrays (all float64 or all float32, each d
        long, each contiguous); they are packed on libbk's host threads, not
        here.  Returns (sel, scores, mean) as multikrum."""
        rows = list(rows)
        n = len(rows)
        if n == 0:
            raise ValueError("no rows")
        dt = np.asarray(rows[0]).dtype
        if dt not in (np.float64, np.float32):
            raise ValueError("rows must be float64 or float32")
        keep = []
        for r in rows:
            a = np.asarray(r)
            if a.dtype != dt or a.ndim != 1:
                raise ValueError("every row must be a 1-D array of the first row's dtype")
            keep.append(a if a.flags.c_contiguous else np.ascontiguousarray(a))
        d = keep[0].shape[0]
        if any(a.shape[0] != d for a in keep):
            raise ValueError("ragged rows")
        f = int(f)
        sel, sc, mean = _outs(n, d, f, want_scores, want_mean)
        mo = ctypes.c_int64(0)
        check(lib().bk_multikrum_rows(self._ctx, _ptr_array(keep), _dtype_code(dt), n, d, f,
                                      sel.ctypes.data, ctypes.addressof(mo), _ptr(sc), _ptr(mean)))
        assert mo.value == n - f
        return sel, sc, mean

    def multikrum_rows_ptr(self, row_ptrs, dtype, n, d, f, sel_ptr, scores_ptr=None,
                           mean_ptr=None):
        """Raw host row pointers (a ctypes c_void_p array); host outputs."""
        mo = ctypes.c_int64(0)
        check(lib().bk_multikrum_rows(self._ctx, row_ptrs, dtype, n, d, f, _p(sel_ptr),
                                      ctypes.addressof(mo), _p(scores_ptr), _p(mean_ptr)))
        return mo.value

    def set_host_threads(self, threads):
        check(lib().bk_set_host_threads(self._ctx, int(threads)))

    # ---- incremental Multi-Krum (bk_collect_*): each update is uploaded and
    #      folded into the Gram when it arrives (VerifyUpdateKRUM's append,
    #      krum.go:291); the finish is scores, selection and mean only -------
    def collect_begin(self, n_cap, d, dtype=np.float64):
        """Start (or restart) the context's collection of up to n_cap rows of d."""
        dt = np.dtype(dtype)
        if dt not in (np.float64, np.float32):
            raise ValueError("dtype must be float64 or float32")
        check(lib().bk_collect_begin(self._ctx, _dtype_code(dt), int(n_cap), int(d)))
        self._collect = (dt, int(d))

    def _collection(self, who):
        st = getattr(self, "_collect", None)
        if st is None:
            raise ValueError("%s without collect_begin" % who)
        return st

    def _order_arg(self, order, n, f, extra=0):
        """A finish's order, n and f as the library takes them: order int64 slots
        or None (every collected row, and the `extra` the call itself adds); n
        defaults to the order's length."""
        if f is None:
            raise ValueError("f is required")
        if order is not None:
            order = np.ascontiguousarray(order, dtype=np.int64)
            if n is None:
                n = len(order)
            if order.ndim != 1 or len(order) < n:
                raise ValueError("order must list n arrival slots")
        elif n is None:
            n = self.collect_count() + extra
        return order, int(n), int(f)

    def collect_add(self, rows):
        """One 1-D array, or a sequence of them (one add: the resident rows are
        read once for the group): host rows of the collection's dtype and d.
        Returns the first arrival slot."""
        dt, d = self._collection("collect_add")
        if isinstance(rows, np.ndarray) and rows.ndim == 1:
            rows = [rows]
        keep = [_row(r, dt, d) for r in rows]
        if not keep:
            raise ValueError("no rows")
        return self.collect_add_ptr(_ptr_array(keep), len(keep), _lib.BK_HOST)

    def collect_add_ptr(self, row_ptrs, count, where):
        """Raw row pointers (a ctypes c_void_p array): pageable, pinned or device."""
        first = ctypes.c_int64(-1)
        check(lib().bk_collect_add(self._ctx, row_ptrs, int(count), int(where),
                                   ctypes.byref(first)))
        return first.value

    def collect_add_noised(self, delta, noise=None):
        """One noised update arrives as Delta and Noise (bk_collect_add_noised):
        delta a 1-D float64 array of the collection's d; noise None (k = 0: the
        row is delta), a vector of length d (k = 1) or a (k, d) array.  The
        stored row is delta + (0 + v_0 + ... + v_{k-1}) / k, added on the
        device.  Returns the arrival slot."""
        dt, d = self._collection("collect_add_noised")
        D, N, nz = _noise_arg(delta, noise, dt, d)
        return self.collect_add_noised_ptr(_ptr_array([D]), nz, len(N), 1, _lib.BK_HOST)

    def collect_add_noised_ptr(self, delta_ptrs, noise_ptrs, k, count, where):
        """Raw pointers (ctypes c_void_p arrays): count deltas and count * k noise
        vectors (vector j of update i at noise_ptrs[i * k + j]; None when k = 0),
        all pageable, pinned or device rows."""
        first = ctypes.c_int64(-1)
        check(lib().bk_collect_add_noised(self._ctx, delta_ptrs, noise_ptrs, int(k), int(count),
                                          int(where), ctypes.byref(first)))
        return first.value

    def collect_read_rows(self, slots):
        """The stored rows of the named arrival slots (bk_collect_read_rows), a
        (len(slots), d) float64 array: after a noised add, NoisedDelta."""
        _, d = self._collection("collect_read_rows")
        slots = np.ascontiguousarray(np.atleast_1d(slots), dtype=np.int64)
        if slots.ndim != 1 or len(slots) < 1:
            raise ValueError("slots must list at least one arrival slot")
        out = np.empty((len(slots), d), dtype=np.float64)
        check(lib().bk_collect_read_rows(self._ctx, slots.ctypes.data, len(slots),
                                         _ptr_array(list(out))))
        return out

    def collect_count(self):
        cnt = ctypes.c_int64(0)
        check(lib().bk_collect_count(self._ctx, ctypes.byref(cnt)))
        return cnt.value

    def collect_finish(self, order=None, n=None, f=None, want_scores=True, want_mean=True):
        """Multi-Krum over the collected rows: order[i] = arrival slot of the
        caller's row i (None: every row, in arrival order).  Returns (sel,
        scores, mean) as multikrum, indices into the caller's rows."""
        _, d = self._collection("collect_finish")
        order, n, f = self._order_arg(order, n, f)
        sel, sc, mean = _outs(n, d, f, want_scores, want_mean)
        mo = ctypes.c_int64(0)
        check(lib().bk_collect_finish(self._ctx, _ptr(order), n, f, sel.ctypes.data,
                                      ctypes.addressof(mo), _ptr(sc), _ptr(mean)))
        assert mo.value == n - f
        return sel, sc, mean

    def collect_add_finish(self, row, order=None, n=None, f=None, want_scores=True,
                           want_mean=True, where=_lib.BK_HOST):
        """The last arrival and the verdict in one call (bk_collect_add_finish):
        collect_add(row) followed by collect_finish(order, n, f), bitwise, in
        one launch at the deployed shapes.  order may name the new slot (the
        count before the call); None: every row, the new one included.  where:
        BK_HOST_PINNED when row is a view of pinned memory (a pageable row of
        more than 32 KiB takes the two calls inside the entry: no faster fused).
        Returns (slot, sel, scores, mean)."""
        dt, d = self._collection("collect_add_finish")
        a = _row(row, dt, d, "the row")
        order, n, f = self._order_arg(order, n, f, extra=1)
        sel, sc, mean = _outs(n, d, f, want_scores, want_mean)
        slot, mo = self.collect_add_finish_ptr(a.ctypes.data, where, _ptr(order), n, f,
                                               sel.ctypes.data, _ptr(sc), _ptr(mean))
        assert mo == n - f
        return slot, sel, sc, mean

    def collect_add_finish_ptr(self, row_ptr, where, order_ptr, n, f, sel_ptr, scores_ptr=None,
                               mean_ptr=None):
        """Raw pointers: the row pageable, pinned or device; order (nullable) and
        the outputs host.  Returns (slot, m)."""
        first, mo = ctypes.c_int64(-1), ctypes.c_int64(0)
        check(lib().bk_collect_add_finish(self._ctx, _p(row_ptr), int(where), _p(order_ptr),
                                          int(n), int(f), ctypes.byref(first), _p(sel_ptr),
                                          ctypes.addressof(mo), _p(scores_ptr), _p(mean_ptr)))
        return first.value, mo.value

    def collect_add_noised_finish(self, delta, noise=None, order=None, n=None, f=None,
                                  want_scores=True, want_mean=True, where=_lib.BK_HOST):
        """The last arrival as Delta and Noise and the verdict in one call
        (bk_collect_add_noised_finish): collect_add_noised(delta, noise)
        followed by collect_finish(order, n, f), bitwise, in one launch at the
        deployed shapes.  delta and noise as collect_add_noised takes them
        (noise None: k = 0, collect_add_finish on delta); order as
        collect_add_finish's; where: BK_HOST_PINNED when delta and noise are
        views of pinned memory.  Returns (slot, sel, scores, mean)."""
        dt, d = self._collection("collect_add_noised_finish")
        D, N, nz = _noise_arg(delta, noise, dt, d)
        order, n, f = self._order_arg(order, n, f, extra=1)
        sel, sc, mean = _outs(n, d, f, want_scores, want_mean)
        slot, mo = self.collect_add_noised_finish_ptr(D.ctypes.data, nz, len(N), where,
                                                      _ptr(order), n, f, sel.ctypes.data,
                                                      _ptr(sc), _ptr(mean))
        assert mo == n - f
        return slot, sel, sc, mean

    def collect_add_noised_finish_ptr(self, delta_ptr, noise_ptrs, k, where, order_ptr, n, f,
                                      sel_ptr, scores_ptr=None, mean_ptr=None):
        """Raw pointers: the delta and the k noise vectors (a ctypes c_void_p
        array; None when k = 0) pageable, pinned or device; order (nullable) and
        the outputs host.  Returns (slot, m)."""
        first, mo = ctypes.c_int64(-1), ctypes.c_int64(0)
        check(lib().bk_collect_add_noised_finish(self._ctx, _p(delta_ptr), noise_ptrs, int(k),
                                                 int(where), _p(order_ptr), int(n), int(f),
                                                 ctypes.byref(first), _p(sel_ptr),
                                                 ctypes.addressof(mo), _p(scores_ptr),
                                                 _p(mean_ptr)))
        return first.value, mo.value

    def collect_stats(self):
        """The collection's launches since collect_begin (bk_collect_stats): which
        path the adds and finishes took."""
        out = (ctypes.c_int64 * 4)()
        check(lib().bk_collect_stats(self._ctx, out))
        return {"border": out[0], "border_reduce": out[1], "one_launch_finishes": out[2],
                "fused_arrivals": out[3]}

    def set_collect_tiny(self, on=True):
        """Opt in: a collection of at most 16 rows with d <= 128 runs every add,
        finish and fused arrival as one launch of one workgroup with no copy call
        (bk_set_collect_tiny); the outputs are bitwise the other paths'."""
        check(lib().bk_set_collect_tiny(self._ctx, 1 if on else 0))

    def collect_tiny_stats(self):
        """The tiny path's launches since collect_begin (bk_collect_tiny_stats):
        adds without a finish, finishes without an add, adds with a finish."""
        out = (ctypes.c_int64 * 3)()
        check(lib().bk_collect_tiny_stats(self._ctx, out))
        return {"adds": out[0], "finishes": out[1], "arrivals": out[2]}

    def collect_finish_batch(self, orders, f, want_scores=True, want_mean=True):
        """B finishes over the one collection in one call (bk_collect_finish_batch):
        orders is a (B, n) integer array, row b the arrival slots of problem
        b's rows (a subset and any permutation), all with the same n and f.
        Returns sel (B, n - f) int64, scores (B, n) or None, mean (B, d) or
        None, shaped as multikrum_batch's; problem b's are bitwise
        collect_finish(order=orders[b], f=f)'s."""
        orders = np.asarray(orders)
        if orders.ndim != 2:
            raise ValueError("orders must be 2-D (B problems x n arrival slots)")
        if orders.dtype.kind not in "iu":
            raise ValueError("orders must be an integer array")
        _, d = self._collection("collect_finish_batch")
        orders = np.ascontiguousarray(orders, dtype=np.int64)
        B, n = orders.shape
        if B < 1:
            raise ValueError("need at least one problem (B=%d)" % B)
        f = int(f)
        sel, sc, mean = _outs(n, d, f, want_scores, want_mean, batch=B)
        mo = ctypes.c_int64(0)
        check(lib().bk_collect_finish_batch(self._ctx, orders.ctypes.data, B, n, f, sel.ctypes.data,
                                            ctypes.addressof(mo), _ptr(sc), _ptr(mean)))
        assert mo.value == n - f
        return sel, sc, mean

    def collect_finish_ragged(self, orders, fs, want_scores=True, want_mean=True):
        """B finishes over the one collection in one call, each with its own n
        and f (bk_collect_finish_ragged): orders is a sequence of 1-D integer
        arrays, element b the arrival slots of problem b's rows; fs an int (the
        same f for all) or a sequence of B of them.  Returns (sels, scores,
        mean): sels a list of int64 arrays, scores a list of float64 arrays or
        None, mean (B, d) or None; problem b's are bitwise
        collect_finish(order=orders[b], f=fs[b])'s."""
        if isinstance(orders, np.ndarray) and orders.ndim < 2:
            raise ValueError("orders must be a sequence of 1-D integer arrays, one per problem")
        orders = [np.asarray(o) for o in orders]
        if not orders:
            raise ValueError("need at least one problem")
        for b, o in enumerate(orders):
            if o.ndim != 1:
                raise ValueError("orders[%d] must be 1-D (its arrival slots)" % b)
            if o.dtype.kind not in "iu":
                raise ValueError("orders[%d] must be an integer array" % b)
        B = len(orders)
        fs = _fs_arg(fs, B)
        _, d = self._collection("collect_finish_ragged")
        ns = np.array([len(o) for o in orders], dtype=np.int64)
        offsets = _offsets(ns)
        packed = np.ascontiguousarray(np.concatenate(orders), dtype=np.int64)
        sel, mo, sc, mean = _ragged_outs(ns, fs, d, want_scores, want_mean)
        check(lib().bk_collect_finish_ragged(self._ctx, packed.ctypes.data, offsets.ctypes.data,
                                             fs.ctypes.data, B, sel.ctypes.data, mo.ctypes.data,
                                             _ptr(sc), _ptr(mean)))
        assert np.array_equal(mo, ns - fs)
        return _ragged_unpack(sel, mo, sc, offsets) + (mean,)

    # ---- host entry with the noise applied in the H2D staging -----------
    #      (bk_multikrum_noised) -------------------
    def multikrum_noised(self, delta, noise, f, want_scores=True, want_mean=True,
                         want_noised=False):
        """Multi-Krum of NoisedDelta = delta + mean of the k noise vectors
        (main.go:1524-1537, 1606-1653) with the noise added on the device as
        the rows land.  delta (n, d) fp64; noise (n, k, d) fp64, k >= 0 (k = 0:
        no noisers, NoisedDelta = Delta).  Returns (sel, scores, mean, noised)."""
        D = np.asarray(delta, dtype=np.float64)
        if D.ndim != 2:
            raise ValueError("delta must be 2-D (n updates x d)")
        if D.strides[1] != 8 or D.strides[0] % 8:
            D = np.ascontiguousarray(D)
        n, d = D.shape
        N = np.ascontiguousarray(noise, dtype=np.float64)
        if N.ndim != 3 or N.shape[0] != n or (N.shape[1] > 0 and N.shape[2] != d):
            raise ValueError("noise must be (n, k, d) matching delta (n, d)")
        k = N.shape[1]
        f = int(f)
        sel, sc, mean = _outs(n, d, f, want_scores, want_mean)
        mo = ctypes.c_int64(0)
        out = np.empty((n, d), dtype=np.float64) if want_noised else None
        check(lib().bk_multikrum_noised(self._ctx, D.ctypes.data, D.strides[0] // 8,
                                        N.ctypes.data if k else None, k, d, _lib.BK_HOST, n, d,
                                        f, sel.ctypes.data, ctypes.addressof(mo), _ptr(sc),
                                        _ptr(mean), _ptr(out), d))
        assert mo.value == n - f
        return sel, sc, mean, out

    def multikrum_noised_ptr(self, delta_ptr, ld, noise_ptr, k, noise_ld, where, n, d, f,
                             sel_ptr, scores_ptr=None, mean_ptr=None, noised_ptr=None,
                             out_ld=0):
        """Raw host pointers (e.g. pinned torch tensors); outputs are host pointers."""
        mo = ctypes.c_int64(0)
        check(lib().bk_multikrum_noised(self._ctx, _p(delta_ptr), ld, _p(noise_ptr), k, noise_ld,
                                        where, n, d, f, _p(sel_ptr), ctypes.addressof(mo),
                                        _p(scores_ptr), _p(mean_ptr), _p(noised_ptr),
                                        out_ld or d))
        return mo.value

    # ---- device entry (bk_multikrum_device): raw device pointers --------
    def multikrum_device_ptr(self, x_ptr, dtype, n, d, ld, f, sel_ptr, scores_ptr=None,
                             mean_ptr=None):
        check(lib().bk_multikrum_device(self._ctx, _p(x_ptr), dtype, n, d, ld, f, _p(sel_ptr),
                                        _p(scores_ptr), _p(mean_ptr)))

    # ---- batched entries (bk_multikrum_batch*): B problems of one shape ----
    def multikrum_batch(self, X, f, want_scores=True, want_mean=True, pinned=False):
        """X: (B, n, d) float64 / float32, C-contiguous or with uniform strides
        (unit element stride; row and problem strides whole elements, the
        problems not overlapping) -- B independent Multi-Krum problems.  Returns
        sel (B, n - f) int64, scores (B, n) or None, mean (B, d) or None; problem
        b's are bitwise multikrum's on X[b].  pinned: X lies in pinned host
        memory (BK_HOST_PINNED)."""
        X = np.asarray(X)
        if X.dtype not in (np.float64, np.float32):
            X = X.astype(np.float64)
        if X.ndim != 3:
            raise ValueError("X must be 3-D (B problems x n updates x d)")
        B, n, d = X.shape
        it = X.itemsize
        if B < 1:
            raise ValueError("need at least one problem (B=%d)" % B)
        if (X.strides[2] != it or X.strides[1] % it or X.strides[0] % it or
                X.strides[1] < d * it or X.strides[0] < (n - 1) * X.strides[1] + d * it):
            X = np.ascontiguousarray(X)
        ld = X.strides[1] // it
        stride = X.strides[0] // it
        f = int(f)
        sel, sc, mean = _outs(n, d, f, want_scores, want_mean, batch=B)
        mo = ctypes.c_int64(0)
        check(lib().bk_multikrum_batch(self._ctx, X.ctypes.data,
                                       _lib.BK_HOST_PINNED if pinned else _lib.BK_HOST,
                                       _dtype_code(X.dtype), B, n, d, ld, stride, f,
                                       sel.ctypes.data, ctypes.addressof(mo), _ptr(sc), _ptr(mean)))
        assert mo.value == n - f
        return sel, sc, mean

    def multikrum_batch_device_ptr(self, x_ptr, dtype, batch, n, d, ld, stride, f, sel_ptr,
                                   scores_ptr=None, mean_ptr=None):
        check(lib().bk_multikrum_batch_device(self._ctx, _p(x_ptr), dtype, batch, n, d, ld,
                                              stride, f, _p(sel_ptr), _p(scores_ptr),
                                              _p(mean_ptr)))

    # ---- ragged entries (bk_multikrum_ragged*): every problem its own n and f ----
    def multikrum_ragged(self, problems, fs, want_scores=True, want_mean=True, pinned=False):
        """problems: a sequence of 2-D arrays (n_b, d) that share d and dtype
        (float64 / float32) -- B independent Multi-Krum problems; fs an int (the
        same f for all) or a sequence of B of them.  Returns a list of (sel,
        scores, mean) per problem (scores / mean None when not wanted); problem
        b's are bitwise multikrum's on problems[b].  The problems go to the
        library packed in one matrix: views of consecutive rows of one
        C-contiguous array are passed as they lie (pinned: that array is in
        pinned host memory, BK_HOST_PINNED), anything else is packed into a
        pageable copy first."""
        if isinstance(problems, np.ndarray) and problems.ndim < 3:
            raise ValueError("problems must be a sequence of 2-D arrays, one per problem")
        problems = [np.asarray(x) for x in problems]
        if not problems:
            raise ValueError("need at least one problem")
        for b, x in enumerate(problems):
            if x.ndim != 2:
                raise ValueError("problems[%d] must be 2-D (n updates x d)" % b)
        if any(x.dtype not in (np.float64, np.float32) for x in problems):
            problems = [x.astype(np.float64) for x in problems]
        dtype, d = problems[0].dtype, problems[0].shape[1]
        for b, x in enumerate(problems):
            if x.shape[1] != d:
                raise ValueError("problems[%d] has d=%d, problems[0] has d=%d: the problems share d"
                                 % (b, x.shape[1], d))
            if x.dtype != dtype:
                raise ValueError("problems[%d] is %s, problems[0] is %s: the problems share a dtype"
                                 % (b, x.dtype, dtype))
        B = len(problems)
        fs = _fs_arg(fs, B)
        ns = np.array([x.shape[0] for x in problems], dtype=np.int64)
        offsets = _offsets(ns)
        it = dtype.itemsize
        packed = all(x.flags.c_contiguous for x in problems) and all(
            problems[b + 1].ctypes.data == problems[b].ctypes.data + int(ns[b]) * d * it
            for b in range(B - 1))
        if packed:
            x_ptr = problems[0].ctypes.data
        else:
            X = np.concatenate(problems, axis=0) if offsets[B] else np.empty((0, d), dtype=dtype)
            X = np.ascontiguousarray(X)
            x_ptr, pinned = X.ctypes.data, False
        sel, mo, sc, mean = _ragged_outs(ns, fs, d, want_scores, want_mean)
        check(lib().bk_multikrum_ragged(self._ctx, x_ptr,
                                        _lib.BK_HOST_PINNED if pinned else _lib.BK_HOST,
                                        _dtype_code(dtype), B, offsets.ctypes.data, fs.ctypes.data,
                                        d, d, sel.ctypes.data, mo.ctypes.data, _ptr(sc), _ptr(mean)))
        assert np.array_equal(mo, ns - fs)
        sels, scs = _ragged_unpack(sel, mo, sc, offsets)
        return [(sels[b], scs[b] if want_scores else None, mean[b].copy() if want_mean else None)
                for b in range(B)]

    def multikrum_ragged_device_ptr(self, x_ptr, dtype, offsets, fs, d, ld, sel_ptr,
                                    scores_ptr=None, mean_ptr=None):
        """Raw device pointers; offsets (B + 1) and fs (B) are host integer
        sequences, consumed before the call returns."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        fs = np.ascontiguousarray(fs, dtype=np.int64)
        if offsets.ndim != 1 or fs.ndim != 1 or offsets.shape[0] != fs.shape[0] + 1:
            raise ValueError("offsets must hold one entry more than fs (one f per problem)")
        check(lib().bk_multikrum_ragged_device(self._ctx, _p(x_ptr), dtype, fs.shape[0],
                                               offsets.ctypes.data, fs.ctypes.data, d, ld,
                                               _p(sel_ptr), _p(scores_ptr), _p(mean_ptr)))

    def selection_margin_batch(self, batch):
        """The records of the last batched call, one dict per problem (the keys
        of selection_margin); batch: that call's problem count."""
        rec = (ctypes.c_double * (8 * batch))()
        check(lib().bk_selection_margin_batch(self._ctx, rec, batch))
        keys = ("gap", "err_bound", "near_tie", "M", "s_lo", "s_hi", "d", "k")
        out = []
        for b in range(batch):
            r = dict(zip(keys, (float(x) for x in rec[8 * b:8 * b + 8])))
            r["near_tie"] = bool(r["near_tie"])
            r["d"] = int(r["d"])
            r["k"] = int(r["k"])
            out.append(r)
        return out

    def multikrum_sharded_ptr(self, x_ptr, dtype, n, d_local, ld, f, sel_ptr, scores_ptr=None,
                              mean_ptr=None):
        check(lib().bk_multikrum_sharded_device(self._ctx, _p(x_ptr), dtype, n, d_local, ld, f,
                                                _p(sel_ptr), _p(scores_ptr), _p(mean_ptr)))

    # ---- SURVEY §8(f) rows 2-3 (bk_aggregate*, bk_quantized_sum_device,
    #      bk_noise_apply_device) --------------------------------------------
    def aggregate(self, X, idx, global_w):
        """global_w += X[idx[0]] + X[idx[1]] + ... in place (host arrays; bk_aggregate)."""
        X = np.asarray(X)
        if X.dtype not in (np.float64, np.float32):
            X = X.astype(np.float64)
        if X.strides[1] != X.itemsize or X.strides[0] % X.itemsize:
            X = np.ascontiguousarray(X)
        n, d = X.shape
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        if global_w.dtype != np.float64 or not global_w.flags.c_contiguous or global_w.shape != (d,):
            raise ValueError("global_w must be a C-contiguous float64 vector of length d")
        check(lib().bk_aggregate(self._ctx, X.ctypes.data, _lib.BK_HOST, _dtype_code(X.dtype), n, d,
                                 X.strides[0] // X.itemsize, idx.ctypes.data, len(idx),
                                 global_w.ctypes.data))
        return global_w

    def aggregate_device_ptr(self, x_ptr, dtype, n, d, ld, idx_ptr, m, global_ptr):
        check(lib().bk_aggregate_device(self._ctx, _p(x_ptr), dtype, n, d, ld, _p(idx_ptr), m,
                                        _p(global_ptr)))

    def quantized_sum_ptr(self, x_ptr, dtype, n, d, ld, idx_ptr, m, precision, sum_ptr,
                          sumf_ptr=None):
        check(lib().bk_quantized_sum_device(self._ctx, _p(x_ptr), dtype, n, d, ld, _p(idx_ptr), m,
                                            int(precision), _p(sum_ptr), _p(sumf_ptr)))

    # ---- the miner's block, added to as the updates arrive (bk_block_*) -----
    def block_begin(self, global_w, precision=None, dtype=np.float64):
        """Start (or restart) the context's block from the gradient global_w (a
        float64 vector); rows will be `dtype`.  precision None: no quantised sum."""
        dt = np.dtype(dtype)
        if dt not in (np.float64, np.float32):
            raise ValueError("dtype must be float64 or float32")
        g = np.ascontiguousarray(global_w, dtype=np.float64)
        if g.ndim != 1 or g.shape[0] < 1:
            raise ValueError("global_w must be a float64 vector")
        self.block_begin_ptr(g.ctypes.data, _lib.BK_HOST, g.shape[0], dt, precision)

    def block_begin_ptr(self, global_ptr, where, d, dtype=np.float64, precision=None):
        """global_w by raw pointer: pageable, pinned or device memory (d doubles)."""
        dt = np.dtype(dtype)
        p = -1 if precision is None else int(precision)
        check(lib().bk_block_begin(self._ctx, _dtype_code(dt), int(d), _p(global_ptr), int(where),
                                   p))
        self._block = (dt, int(d), p)

    def _block_state(self, who):
        st = getattr(self, "_block", None)
        if st is None:
            raise ValueError("%s without block_begin" % who)
        return st

    def block_add(self, rows, accepted=None):
        """One 1-D array, or a sequence of them: host rows of the block's dtype
        and d, in arrival order; accepted None (all) or one flag per row (a
        rejected row may be None: it is never read).  Returns the first slot."""
        dt, d, _ = self._block_state("block_add")
        if isinstance(rows, np.ndarray) and rows.ndim == 1:
            rows = [rows]
        rows = list(rows)
        if not rows:
            raise ValueError("no rows")
        if accepted is not None:
            acc = np.ascontiguousarray(np.atleast_1d(accepted)).astype(np.uint8)
            if acc.shape != (len(rows),):
                raise ValueError("accepted must have one flag per row")
        dummy = np.zeros(1, dtype=dt)
        keep = [dummy if (r is None and accepted is not None and not acc[i])
                else _row(r, dt, d) for i, r in enumerate(rows)]
        return self.block_add_ptr(_ptr_array(keep), len(keep), _lib.BK_HOST,
                                  acc.ctypes.data if accepted is not None else None)

    def block_add_ptr(self, row_ptrs, count, where, accepted_ptr=None):
        """Raw row pointers (a ctypes c_void_p array): pageable, pinned or device
        rows; accepted_ptr: count bytes, or None for all."""
        first = ctypes.c_int64(-1)
        check(lib().bk_block_add(self._ctx, row_ptrs, _p(accepted_ptr), int(count), int(where),
                                 ctypes.byref(first)))
        return first.value

    def block_count(self):
        """(rows added, rows accepted) since block_begin."""
        a, b = ctypes.c_int64(0), ctypes.c_int64(0)
        check(lib().bk_block_count(self._ctx, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def _block_outs(self, want_qsum, p, d):
        if want_qsum and p < 0:
            raise ValueError("the block was begun without a precision: it keeps no quantised sum")
        g = np.empty(d, dtype=np.float64)
        q = np.empty(d, dtype=np.int64) if want_qsum else None
        qf = np.empty(d, dtype=np.float64) if want_qsum else None
        return g, q, qf

    def block_finish(self, want_qsum=False):
        """The block so far (it is not consumed): the gradient, or with want_qsum
        (gradient, int64 sum, float sum)."""
        _, d, p = self._block_state("block_finish")
        g, q, qf = self._block_outs(want_qsum, p, d)
        self.block_finish_ptr(g.ctypes.data, _ptr(q), _ptr(qf))
        return (g, q, qf) if want_qsum else g

    def block_finish_ptr(self, global_ptr, qsum_ptr=None, qsum_float_ptr=None):
        """Host outputs by raw pointer (d entries each)."""
        check(lib().bk_block_finish(self._ctx, _p(global_ptr), _p(qsum_ptr), _p(qsum_float_ptr)))

    def block_add_finish(self, row, accepted=True, want_qsum=False):
        """The last arrival and the block in one call (bk_block_add_finish):
        block_add(row, accepted) followed by block_finish, bitwise.  Returns
        (slot, gradient) or (slot, gradient, int64 sum, float sum)."""
        dt, d, p = self._block_state("block_add_finish")
        a = _row(row, dt, d)
        g, q, qf = self._block_outs(want_qsum, p, d)
        slot = self.block_add_finish_ptr(a.ctypes.data, accepted, _lib.BK_HOST, g.ctypes.data,
                                         _ptr(q), _ptr(qf))
        return (slot, g, q, qf) if want_qsum else (slot, g)

    def block_add_finish_ptr(self, row_ptr, accepted, where, global_ptr, qsum_ptr=None,
                             qsum_float_ptr=None):
        first = ctypes.c_int64(-1)
        check(lib().bk_block_add_finish(self._ctx, _p(row_ptr), 1 if accepted else 0, int(where),
                                        ctypes.byref(first), _p(global_ptr), _p(qsum_ptr),
                                        _p(qsum_float_ptr)))
        return first.value

    def block_stats(self):
        """The block's launches since block_begin (bk_block_stats): [add launches,
        fused add-finish launches, launches reading mapped host rows, finishes
        without a D2H copy call]."""
        out = (ctypes.c_int64 * 4)()
        check(lib().bk_block_stats(self._ctx, out))
        return list(out)

    # ---- the convergence check: resident evaluation sets (bk_eval*) ---------
    def eval_set_logistic(self, set_index, X, y):
        """Make (X, y) the context's evaluation set `set_index` (0 .. 3): X nv x d
        float64 (a row stride is kept), y the nv labels (stored as float64)."""
        X = np.asarray(X)
        if X.ndim != 2 or X.dtype != np.float64 or X.shape[0] < 1 or X.shape[1] < 1:
            raise ValueError("X must be a float64 matrix, nv x d")
        if X.strides[1] != 8 or X.strides[0] % 8 or X.strides[0] < 8 * X.shape[1]:
            X = np.ascontiguousarray(X)
        y = np.ascontiguousarray(y, dtype=np.float64)
        if y.shape != (X.shape[0],):
            raise ValueError("y must have one label per row of X")
        check(lib().bk_eval_set_logistic(self._ctx, int(set_index), X.ctypes.data, X.shape[0],
                                         X.shape[1], X.strides[0] // 8, y.ctypes.data))

    def eval_set_softmax(self, set_index, X, y, n_classes):
        """X nv x d_in float32, y integer labels in [0, n_classes); the model
        scored on it has n_classes * (d_in + 1) entries (W row-major, then b)."""
        X = np.asarray(X)
        if X.ndim != 2 or X.dtype != np.float32 or X.shape[0] < 1 or X.shape[1] < 1:
            raise ValueError("X must be a float32 matrix, nv x d_in")
        if X.strides[1] != 4 or X.strides[0] % 4 or X.strides[0] < 4 * X.shape[1]:
            X = np.ascontiguousarray(X)
        ya = np.asarray(y)
        if ya.shape != (X.shape[0],) or not np.issubdtype(ya.dtype, np.integer):
            raise ValueError("y must have one integer label per row of X")
        y32 = np.ascontiguousarray(ya, dtype=np.int32)
        if not np.array_equal(y32, ya):
            raise ValueError("labels do not fit int32")
        check(lib().bk_eval_set_softmax(self._ctx, int(set_index), X.ctypes.data, X.shape[0],
                                        X.shape[1], X.strides[0] // 4, y32.ctypes.data,
                                        int(n_classes)))

    def eval_clear(self, set_index):
        check(lib().bk_eval_clear(self._ctx, int(set_index)))

    @staticmethod
    def _eval_outs(sets):
        s = np.ascontiguousarray(np.atleast_1d(sets), dtype=np.intc)
        if s.ndim != 1 or not 1 <= s.shape[0] <= _lib.BK_EVAL_MAX_SETS:
            raise ValueError("sets must name 1 .. %d evaluation sets" % _lib.BK_EVAL_MAX_SETS)
        n = s.shape[0]
        return s, np.empty(n), np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int32)

    def eval(self, ww, sets):
        """Score the model ww (float64 vector) on the resident sets named:
        (err float64, wrong int64, near_ties int32), one entry per set."""
        w = np.ascontiguousarray(ww, dtype=np.float64)
        if w.ndim != 1 or w.shape[0] < 1:
            raise ValueError("ww must be a float64 vector")
        s, err, wrong, near = self._eval_outs(sets)
        self.eval_ptr(w.ctypes.data, w.shape[0], _lib.BK_HOST, s, err, wrong, near)
        return err, wrong, near

    def eval_ptr(self, ww_ptr, d, where, sets, err, wrong, near_ties=None):
        """The model by raw pointer (pageable, pinned or device memory); sets an
        intc array, err / wrong / near_ties numpy outputs of its length."""
        check(lib().bk_eval(self._ctx, _p(ww_ptr), int(d), int(where), sets.ctypes.data,
                            int(sets.shape[0]), err.ctypes.data, wrong.ctypes.data,
                            _ptr(near_ties)))

    def eval_stats(self):
        """[launches, calls] of bk_eval / bk_block_finish_eval since the engine
        was made."""
        out = (ctypes.c_int64 * 2)()
        check(lib().bk_eval_stats(self._ctx, out))
        return list(out)

    def block_finish_eval(self, sets, want_qsum=False):
        """block_finish and eval of the returned gradient in one call
        (bk_block_finish_eval): (gradient[, int64 sum, float sum], err, wrong,
        near_ties)."""
        _, d, p = self._block_state("block_finish_eval")
        g, q, qf = self._block_outs(want_qsum, p, d)
        s, err, wrong, near = self._eval_outs(sets)
        check(lib().bk_block_finish_eval(self._ctx, g.ctypes.data, _ptr(q), _ptr(qf),
                                         s.ctypes.data, int(s.shape[0]), err.ctypes.data,
                                         wrong.ctypes.data, near.ctypes.data))
        return ((g, q, qf) if want_qsum else (g,)) + (err, wrong, near)

    # ---- secure aggregation: shares, their sum and recovery (bk_shares_*) ----
    @staticmethod
    def _shares_shape(d, poly_size, precision=0):
        d, poly_size, precision = int(d), int(poly_size), int(precision)
        if d < 1:
            raise ValueError("d=%d < 1" % d)
        if not 1 <= poly_size <= _lib.BK_SHARES_MAX_POLY:
            raise ValueError("poly_size=%d outside [1, %d]" % (poly_size, _lib.BK_SHARES_MAX_POLY))
        if not 0 <= precision <= 18:
            raise ValueError("precision=%d outside [0, 18]" % precision)
        return d, poly_size, precision, -(-d // poly_size)

    @staticmethod
    def _shares_part(a, chunks, held, what="part"):
        a = np.asarray(a)
        if a.dtype != np.int64 or a.shape != (chunks, held):
            raise ValueError("%s must be an int64 array of shape (%d, %d)" % (what, chunks, held))
        return a if a.flags.c_contiguous else np.ascontiguousarray(a)

    def shares_generate(self, delta, precision=4, poly_size=10, total_shares=20):
        """A client's shares of the float64 vector delta: int64 [chunk][share],
        createShareAndWitness's values bit for bit (bk_shares_generate)."""
        a = np.asarray(delta)
        if a.dtype != np.float64 or a.ndim != 1:
            raise ValueError("delta must be a 1-D float64 array")
        a = a if a.flags.c_contiguous else np.ascontiguousarray(a)
        d, P, p, chunks = self._shares_shape(a.shape[0] if a.shape[0] else 0, poly_size, precision)
        T = int(total_shares)
        if not P <= T <= _lib.BK_SHARES_MAX_POINTS:
            raise ValueError("total_shares=%d outside [poly_size=%d, %d]"
                             % (T, P, _lib.BK_SHARES_MAX_POINTS))
        y = np.empty((chunks, T), dtype=np.int64)
        self.shares_generate_ptr(a.ctypes.data, _lib.BK_HOST, d, p, P, T, y.ctypes.data)
        return y

    def shares_generate_ptr(self, delta_ptr, where, d, precision, poly_size, total_shares, y_ptr):
        """delta and y by raw pointer, both pageable, pinned or device memory."""
        check(lib().bk_shares_generate(self._ctx, _p(delta_ptr), int(where), int(d), int(precision),
                                       int(poly_size), int(total_shares), _p(y_ptr)))

    def shares_begin(self, d, poly_size, held, n_cap):
        """The miner's store: up to n_cap parts of ceil(d / poly_size) x held int64."""
        d, P, _, chunks = self._shares_shape(d, poly_size)
        held, n_cap = int(held), int(n_cap)
        if not 1 <= held <= _lib.BK_SHARES_MAX_POINTS:
            raise ValueError("held=%d outside [1, %d]" % (held, _lib.BK_SHARES_MAX_POINTS))
        if not 1 <= n_cap <= _lib.BK_MAX_N:
            raise ValueError("n_cap=%d outside [1, %d]" % (n_cap, _lib.BK_MAX_N))
        check(lib().bk_shares_begin(self._ctx, d, P, held, n_cap))
        self._shares = (d, P, held, chunks)

    def _shares_state(self, who):
        st = getattr(self, "_shares", None)
        if st is None:
            raise ValueError("%s without shares_begin" % who)
        return st

    def shares_add(self, part):
        """One client's part (int64, chunks x held, host); returns its slot."""
        _, _, held, chunks = self._shares_state("shares_add")
        a = self._shares_part(part, chunks, held)
        return self.shares_add_ptr(a.ctypes.data, _lib.BK_HOST)

    def shares_add_ptr(self, part_ptr, where):
        self._shares_state("shares_add")
        slot = ctypes.c_int64(-1)
        check(lib().bk_shares_add(self._ctx, _p(part_ptr), int(where), ctypes.byref(slot)))
        return slot.value

    def shares_count(self):
        n = ctypes.c_int64(0)
        check(lib().bk_shares_count(self._ctx, ctypes.byref(n)))
        return n.value

    def shares_sum(self, slots, want=True):
        """The wrapping sum of the listed slots' parts: kept on the device as the
        context's own aggregate, and returned (chunks x held int64) if wanted."""
        _, _, held, chunks = self._shares_state("shares_sum")
        s = np.asarray(slots)
        if s.ndim != 1 or s.shape[0] < 1 or not np.issubdtype(s.dtype, np.integer):
            raise ValueError("slots must be a non-empty 1-D integer array")
        s = np.ascontiguousarray(s, dtype=np.int64)
        out = np.empty((chunks, held), dtype=np.int64) if want else None
        check(lib().bk_shares_sum(self._ctx, s.ctypes.data, s.shape[0], _p(_ptr(out))))
        return out

    def shares_recover(self, global_w, parts, xs, precision=4, poly_size=10, want_coef=True,
                       want_delta=True):
        """The leader's recovery (bk_shares_recover): parts a sequence of int64
        (chunks x held_i) host arrays, at most one of them None for the
        context's own aggregate; xs the nodes in part order.  Returns
        (global_w + delta, coef or None, delta or None, bad chunks)."""
        w = np.asarray(global_w)
        if w.dtype != np.float64 or w.ndim != 1:
            raise ValueError("global_w must be a 1-D float64 array")
        w = w if w.flags.c_contiguous else np.ascontiguousarray(w)
        d, P, p, chunks = self._shares_shape(w.shape[0], poly_size, precision)
        parts = list(parts)
        if not 1 <= len(parts) <= _lib.BK_SHARES_MAX_POINTS:
            raise ValueError("%d parts outside [1, %d]" % (len(parts), _lib.BK_SHARES_MAX_POINTS))
        if sum(q is None for q in parts) > 1:
            raise ValueError("at most one part may be None (the own aggregate)")
        keep, held = [], []
        for i, q in enumerate(parts):
            if q is None:
                held.append(self._shares_state("a None part")[2])
                keep.append(None)
                continue
            a = np.asarray(q)
            if a.ndim != 2 or a.shape[1] < 1:
                raise ValueError("parts[%d] must be an int64 array of shape (%d, held)" % (i, chunks))
            keep.append(self._shares_part(a, chunks, a.shape[1], "parts[%d]" % i))
            held.append(a.shape[1])
        x = np.asarray(xs)
        if x.ndim != 1 or not np.issubdtype(x.dtype, np.integer) or x.shape[0] != sum(held):
            raise ValueError("xs must hold one integer node per share: %d" % sum(held))
        x = np.ascontiguousarray(x, dtype=np.int64)
        if not P <= x.shape[0] <= _lib.BK_SHARES_MAX_POINTS:
            raise ValueError("%d points outside [poly_size=%d, %d]"
                             % (x.shape[0], P, _lib.BK_SHARES_MAX_POINTS))
        if len(set(x.tolist())) != x.shape[0]:
            raise ValueError("the nodes xs must differ")
        ptrs = (ctypes.c_void_p * len(keep))(*[a.ctypes.data if a is not None else None
                                               for a in keep])
        h = np.ascontiguousarray(held, dtype=np.intc)
        g = np.empty(d, dtype=np.float64)
        coef = np.empty(d, dtype=np.int64) if want_coef else None
        delta = np.empty(d, dtype=np.float64) if want_delta else None
        bad = self.shares_recover_ptr(ptrs, h, x, _lib.BK_HOST, d, P, p, w.ctypes.data, _ptr(coef),
                                      _ptr(delta), g.ctypes.data)
        return g, coef, delta, bad

    def shares_recover_ptr(self, part_ptrs, held, xs, where, d, poly_size, precision, global_ptr,
                           coef_ptr, delta_ptr, out_ptr):
        """Raw pointers: part_ptrs a ctypes c_void_p array (an entry None: the
        own aggregate), held an intc array, xs an int64 array (both host); the
        parts, global_w and the outputs at `where`.  Returns the bad chunks."""
        bad = ctypes.c_int64(-1)
        check(lib().bk_shares_recover(self._ctx, part_ptrs, held.ctypes.data, xs.ctypes.data,
                                      int(held.shape[0]), int(where), int(d), int(poly_size),
                                      int(precision), _p(global_ptr), _p(coef_ptr), _p(delta_ptr),
                                      _p(out_ptr), ctypes.byref(bad)))
        return bad.value

    def shares_stats(self):
        """[kernel launches, copy calls, calls, bad chunks] of bk_shares_* since
        the engine was made."""
        out = (ctypes.c_int64 * 4)()
        check(lib().bk_shares_stats(self._ctx, out))
        return list(out)

    # ---- polynomial commitments in bn256 G1 (bk_commit_*) ---------------------
    def commit_set_key(self, points):
        """Make PKG1 the context's resident key: count x 64 marshalled bytes
        (bytes, or a uint8 array of shape (count, 64))."""
        a = np.frombuffer(points, dtype=np.uint8) if isinstance(points, (bytes, bytearray)) \
            else np.asarray(points)
        if a.dtype != np.uint8 or a.size < 64 or a.size % 64 or a.ndim > 2 or \
                (a.ndim == 2 and a.shape[1] != 64):
            raise ValueError("the key must be count x 64 bytes")
        a = np.ascontiguousarray(a)
        check(lib().bk_commit_set_key(self._ctx, a.ctypes.data, a.size // 64))
        self._commit_key = a.size // 64

    def commit_key_count(self):
        n = ctypes.c_int64(-1)
        check(lib().bk_commit_key_count(self._ctx, ctypes.byref(n)))
        return n.value

    def _commit_scalars(self, scalars, first):
        s = np.asarray(scalars)
        if s.ndim != 1 or s.shape[0] < 1 or s.dtype != np.int64:
            raise ValueError("the scalars must be a non-empty 1-D int64 array")
        first = int(first)
        count = getattr(self, "_commit_key", None)
        if count is None:
            raise ValueError("no commitment key: commit_set_key first")
        if first < 0 or first + s.shape[0] > count:
            raise ValueError("key points [%d, %d) outside the key's %d"
                             % (first, first + s.shape[0], count))
        return np.ascontiguousarray(s), first

    def commit_msm(self, scalars, first=0):
        """createCommitment(scalars, PKG1[first:first + n]): 64 bytes."""
        s, first = self._commit_scalars(scalars, first)
        out = np.empty(64, dtype=np.uint8)
        self.commit_msm_ptr(s.ctypes.data, _lib.BK_HOST, s.shape[0], first, out.ctypes.data)
        return out.tobytes()

    def commit_msm_ptr(self, scalars_ptr, where, n, first, out_ptr):
        """scalars and the 64 output bytes by raw pointer, both at `where`."""
        check(lib().bk_commit_msm(self._ctx, _p(scalars_ptr), int(where), int(n), int(first),
                                  _p(out_ptr)))

    def commit_verify(self, scalars, committed, first=0):
        """verifyCommitment: whether the commitment's bytes equal `committed`."""
        s, first = self._commit_scalars(scalars, first)
        c = np.frombuffer(bytes(committed), dtype=np.uint8)
        if c.shape[0] != 64:
            raise ValueError("a committed point is 64 bytes")
        ok = ctypes.c_int(-1)
        check(lib().bk_commit_verify(self._ctx, s.ctypes.data, _lib.BK_HOST, s.shape[0], first,
                                     c.ctypes.data, ctypes.byref(ok)))
        return bool(ok.value)

    def commit_generate(self, update, precision=4, poly_size=10, total_shares=20, want_commit=True,
                        want_chunks=True, want_witnesses=True):
        """generateMinerSecretShares' commitments of a 1-D update: float64 (a
        delta, quantised with `precision`) or int64 (taken as it is).  Returns
        (commitment: 64 uint8, chunk commitments: chunks x 64, witnesses:
        chunks x total_shares x 64), None for what was not wanted."""
        a = np.asarray(update)
        if a.ndim != 1 or a.dtype not in (np.float64, np.int64):
            raise ValueError("the update must be a 1-D float64 or int64 array")
        a = a if a.flags.c_contiguous else np.ascontiguousarray(a)
        d, P, p, chunks = self._shares_shape(a.shape[0] if a.shape[0] else 0, poly_size, precision)
        T = int(total_shares)
        if not P <= T <= _lib.BK_SHARES_MAX_POINTS:
            raise ValueError("total_shares=%d outside [poly_size=%d, %d]"
                             % (T, P, _lib.BK_SHARES_MAX_POINTS))
        if not (want_commit or want_chunks or want_witnesses):
            raise ValueError("no output requested")
        count = getattr(self, "_commit_key", None)
        if count is None:
            raise ValueError("no commitment key: commit_set_key first")
        if d > count:
            raise ValueError("d=%d exceeds the key's %d points" % (d, count))
        com = np.empty(64, dtype=np.uint8) if want_commit else None
        chk = np.empty((chunks, 64), dtype=np.uint8) if want_chunks else None
        wit = np.empty((chunks, T, 64), dtype=np.uint8) if want_witnesses else None
        is_q = a.dtype == np.int64
        self.commit_generate_ptr(None if is_q else a.ctypes.data, a.ctypes.data if is_q else None,
                                 _lib.BK_HOST, d, p, P, T, _ptr(com), _ptr(chk), _ptr(wit))
        return com, chk, wit

    def commit_generate_ptr(self, delta_ptr, q_ptr, where, d, precision, poly_size, total_shares,
                            commit_ptr, chunk_ptr, witness_ptr):
        """Raw pointers, all at `where`; exactly one of delta_ptr / q_ptr."""
        check(lib().bk_commit_generate(self._ctx, _p(delta_ptr), _p(q_ptr), int(where), int(d),
                                       int(precision), int(poly_size), int(total_shares),
                                       _p(commit_ptr), _p(chunk_ptr), _p(witness_ptr)))

    def commit_stats(self):
        """[kernel launches, copy calls, calls, key points] of bk_commit_*."""
        out = (ctypes.c_int64 * 4)()
        check(lib().bk_commit_stats(self._ctx, out))
        return list(out)

    # ---- the gradient step on the resident training shard (bk_grad_*) --------
    def grad_set_logistic(self, X, y):
        """Make (X, y) the context's training set: X nn x d float64 (a row stride
        is kept), y the nn labels (stored as float64)."""
        X = np.asarray(X)
        if X.ndim != 2 or X.dtype != np.float64 or X.shape[0] < 1 or X.shape[1] < 1:
            raise ValueError("X must be a float64 matrix, nn x d")
        if X.shape[1] > _lib.BK_GRAD_MAX_D:
            raise ValueError("d=%d exceeds %d" % (X.shape[1], _lib.BK_GRAD_MAX_D))
        if X.strides[1] != 8 or X.strides[0] % 8 or X.strides[0] < 8 * X.shape[1]:
            X = np.ascontiguousarray(X)
        y = np.ascontiguousarray(y, dtype=np.float64)
        if y.shape != (X.shape[0],):
            raise ValueError("y must have one label per row of X")
        check(lib().bk_grad_set_logistic(self._ctx, X.ctypes.data, X.shape[0], X.shape[1],
                                         X.strides[0] // 8, y.ctypes.data))
        self._grad = ("logistic", X.shape[0], X.shape[1])

    def grad_set_softmax(self, X, y, n_classes):
        """X nn x d_in float32, y integer labels in [0, n_classes), 2 <= n_classes
        <= 16; the model has n_classes * (d_in + 1) entries (W row-major, then b)."""
        X = np.asarray(X)
        if X.ndim != 2 or X.dtype != np.float32 or X.shape[0] < 1 or X.shape[1] < 1:
            raise ValueError("X must be a float32 matrix, nn x d_in")
        C = int(n_classes)
        if not 2 <= C <= 16:
            raise ValueError("n_classes=%d outside [2, 16]" % C)
        if X.shape[1] > _lib.BK_GRAD_MAX_D:
            raise ValueError("d_in=%d exceeds %d" % (X.shape[1], _lib.BK_GRAD_MAX_D))
        if X.strides[1] != 4 or X.strides[0] % 4 or X.strides[0] < 4 * X.shape[1]:
            X = np.ascontiguousarray(X)
        ya = np.asarray(y)
        if ya.shape != (X.shape[0],) or not np.issubdtype(ya.dtype, np.integer):
            raise ValueError("y must have one integer label per row of X")
        if ya.min() < 0 or ya.max() >= C:
            raise ValueError("labels outside [0, %d)" % C)
        y32 = np.ascontiguousarray(ya, dtype=np.int32)
        check(lib().bk_grad_set_softmax(self._ctx, X.ctypes.data, X.shape[0], X.shape[1],
                                        X.strides[0] // 4, y32.ctypes.data, C))
        self._grad = ("softmax", X.shape[0], C * (X.shape[1] + 1))

    def grad_clear(self):
        check(lib().bk_grad_clear(self._ctx))
        self._grad = None

    def _grad_args(self, kind, ww, idx, noise, precision):
        """The host arrays of a gradient call, validated: (w, idx or None, noise
        or None, precision or -1, delta, q or None)."""
        st = getattr(self, "_grad", None)
        if not st or st[0] != kind:
            raise ValueError("no resident %s training set: call grad_set_%s" % (kind, kind))
        _, nn, d = st
        w = np.ascontiguousarray(ww, dtype=np.float64)
        if w.shape != (d,):
            raise ValueError("ww must be a float64 vector of %d entries" % d)
        ix = None
        if idx is not None:
            ia = np.asarray(idx)
            if ia.ndim != 1 or ia.shape[0] < 1 or not np.issubdtype(ia.dtype, np.integer):
                raise ValueError("idx must be a non-empty 1-D integer array")
            if ia.min() < 0 or ia.max() >= nn:
                raise ValueError("idx outside [0, %d)" % nn)
            ix = np.ascontiguousarray(ia, dtype=np.int64)
        if (nn if ix is None else ix.shape[0]) > _lib.BK_GRAD_MAX_BATCH:
            raise ValueError("a batch of more than %d rows" % _lib.BK_GRAD_MAX_BATCH)
        nz = None
        if noise is not None:
            nz = np.ascontiguousarray(noise, dtype=np.float64)
            if nz.shape != (d,):
                raise ValueError("noise must be a float64 vector of %d entries" % d)
        p = -1 if precision is None else int(precision)
        if not -1 <= p <= 18:
            raise ValueError("precision=%d outside [0, 18]" % p)
        return w, ix, nz, p, np.empty(d), (np.empty(d, dtype=np.int64) if p >= 0 else None)

    def grad_logistic(self, ww, idx=None, batch_size=10, alpha=1e-2, lammy=0.01, noise=None,
                      precision=None):
        """privateFun of the logistic model on the rows idx of the resident set
        (None: all of them): (delta, q or None, loss)."""
        if int(batch_size) < 1:
            raise ValueError("batch_size=%d < 1" % int(batch_size))
        w, ix, nz, p, delta, q = self._grad_args("logistic", ww, idx, noise, precision)
        loss = ctypes.c_double()
        self.grad_logistic_ptr(w.ctypes.data, _lib.BK_HOST, ix, batch_size, alpha, lammy, _ptr(nz),
                               p, delta.ctypes.data, _ptr(q), loss)
        return delta, q, loss.value

    def grad_logistic_ptr(self, ww_ptr, where, idx, batch_size, alpha, lammy, noise_ptr, precision,
                          delta_ptr, q_ptr, loss=None):
        """The model, noise and outputs by raw pointer (pageable, pinned or
        device memory); idx an int64 numpy array or None; loss a ctypes.c_double."""
        check(lib().bk_grad_logistic(self._ctx, _p(ww_ptr), int(where), _p(_ptr(idx)),
                                     0 if idx is None else int(idx.shape[0]), int(batch_size),
                                     float(alpha), float(lammy), _p(noise_ptr), int(precision),
                                     _p(delta_ptr), _p(q_ptr),
                                     ctypes.byref(loss) if loss is not None else None))

    def grad_softmax(self, ww, idx=None, max_norm=100.0, noise=None, precision=None):
        """privateFun of the torch softmax model: (delta, q or None, loss, norm
        before clipping)."""
        mn = float(max_norm)
        if not (np.isfinite(mn) and mn > 0.0):
            raise ValueError("max_norm must be a positive finite number")
        w, ix, nz, p, delta, q = self._grad_args("softmax", ww, idx, noise, precision)
        loss, norm = ctypes.c_double(), ctypes.c_double()
        self.grad_softmax_ptr(w.ctypes.data, _lib.BK_HOST, ix, mn, _ptr(nz), p, delta.ctypes.data,
                              _ptr(q), loss, norm)
        return delta, q, loss.value, norm.value

    def grad_softmax_ptr(self, ww_ptr, where, idx, max_norm, noise_ptr, precision, delta_ptr, q_ptr,
                         loss=None, norm=None):
        check(lib().bk_grad_softmax(self._ctx, _p(ww_ptr), int(where), _p(_ptr(idx)),
                                    0 if idx is None else int(idx.shape[0]), float(max_norm),
                                    _p(noise_ptr), int(precision), _p(delta_ptr), _p(q_ptr),
                                    ctypes.byref(loss) if loss is not None else None,
                                    ctypes.byref(norm) if norm is not None else None))

    def grad_stats(self):
        """[kernel launches, gradient calls] of bk_grad_* since the engine was made."""
        out = (ctypes.c_int64 * 2)()
        check(lib().bk_grad_stats(self._ctx, out))
        return list(out)

    def noise_apply_ptr(self, delta_ptr, n, d, ld, noise_ptr, k, noise_ld, out_ptr, out_ld):
        check(lib().bk_noise_apply_device(self._ctx, _p(delta_ptr), n, d, ld, _p(noise_ptr), k,
                                          noise_ld, _p(out_ptr), out_ld))

    def gram_upper_ptr(self, x_ptr, dtype, n, d, ld, upper_ptr):
        check(lib().bk_gram_upper_device(self._ctx, _p(x_ptr), dtype, n, d, ld, _p(upper_ptr)))

    def finish_ptr(self, upper_ptr, x_ptr, dtype, n, d, ld, f, sel_ptr, scores_ptr=None,
                   mean_ptr=None):
        check(lib().bk_finish_device(self._ctx, _p(upper_ptr), _p(x_ptr), dtype, n, d, ld, f,
                                     _p(sel_ptr), _p(scores_ptr), _p(mean_ptr)))

    def synth_fill_ptr(self, x_ptr, dtype, n, d_local, ld, c0, d_total, seed, nbyz,
                       mu_scale=0.01, byz_scale=0.05, sigma=1e-3, flags=0):
        check(lib().bk_synth_fill_device(self._ctx, _p(x_ptr), dtype, n, d_local, ld, c0, d_total,
                                         seed, nbyz, mu_scale, byz_scale, sigma, flags))

    # ---- plumbing ------------------------------------------------------
    def set_stream(self, stream_handle):
        check(lib().bk_set_stream(self._ctx, _p(stream_handle)))

    def stream(self):
        return lib().bk_get_stream(self._ctx)

    def synchronize(self):
        check(lib().bk_synchronize(self._ctx))

    def comm_init(self, nranks, rank, uid_bytes):
        buf = ctypes.create_string_buffer(bytes(uid_bytes), _lib.BK_UNIQUE_ID_BYTES)
        check(lib().bk_comm_init(self._ctx, int(nranks), int(rank), buf))

    def comm_set_mode(self, mode):
        """0 (or False): all-reduce; 1 (or True): deterministic all-gather +
        rank-order sum; 2: all-reduce overlapped with the Gram (bk.h)."""
        check(lib().bk_comm_set_mode(self._ctx, int(mode)))

    def timing_enable(self, on=True):
        check(lib().bk_timing_enable(self._ctx, 1 if on else 0))

    # ---- selection margin (bk_selection_margin): where the selection may
    #      legitimately differ from numpy's (logistic_validator.py:45,59-63) --
    def selection_margin(self):
        """{gap, err_bound, near_tie, M, s_lo, s_hi, d, k} of the last call on
        this context; near_tie False proves the reference selects the same set."""
        rec = (ctypes.c_double * 8)()
        check(lib().bk_selection_margin_record(self._ctx, rec))
        keys = ("gap", "err_bound", "near_tie", "M", "s_lo", "s_hi", "d", "k")
        out = dict(zip(keys, (float(x) for x in rec)))
        out["near_tie"] = bool(out["near_tie"])
        out["d"] = int(out["d"])
        out["k"] = int(out["k"])
        return out

    def set_small_path(self, on=True):
        """n <= 128: the one-launch k_small path (default) or the general chain."""
        check(lib().bk_set_small_path(self._ctx, 1 if on else 0))

    def set_collect_wide(self, on=True):
        """opt-in (default off): collection finishes of n <= 128 rows with 32,768 <
        d <= 1,048,576 in one launch as well (bk_set_collect_wide); the outputs
        are bitwise the chain's."""
        check(lib().bk_set_collect_wide(self._ctx, 1 if on else 0))

    def set_collect_wide_arrive(self, on=True, everywhere=False):
        """opt-in (default off; needs set_collect_wide): collect_add_finish of a
        pinned or a device row whose finish is in the wide one-launch range is
        the row's copy and one launch, k_collect_arrive_wide
        (bk_set_collect_wide_arrive); the outputs are bitwise the two calls'.
        on alone takes the launch only where it was measured ahead (a pinned
        row of at most 320,000 bytes with the mean); everywhere=True in the
        whole range."""
        check(lib().bk_set_collect_wide_arrive(self._ctx, (2 if everywhere else 1) if on else 0))

    def certified_reruns(self):
        return int(lib().bk_certified_reruns(self._ctx))

    def comm_size(self):
        nr, rk = ctypes.c_int(0), ctypes.c_int(0)
        check(lib().bk_comm_size(self._ctx, ctypes.byref(nr), ctypes.byref(rk)))
        return nr.value, rk.value

    def comm_stats(self):
        ex, by = ctypes.c_int64(0), ctypes.c_double(0)
        check(lib().bk_comm_stats(self._ctx, ctypes.byref(ex), ctypes.byref(by)))
        return ex.value, by.value

    def set_f32_mode(self, mode):
        """_lib.BK_F32_EXACT (fp32 rows widened onto the fp64 MFMA, default),
        _lib.BK_F32_MFMA (the fp32 MFMA, fp32 accumulation per K1 segment),
        _lib.BK_F32_CERTIFIED (the fp32 MFMA, re-run exactly on a near tie),
        _lib.BK_F32_I8 / _lib.BK_F32_I8_CERTIFIED (the Gram from exact int8
        digit slices, K1i8: three digits, six products), _lib.BK_F32_I8X2 /
        _lib.BK_F32_I8X2_CERTIFIED (two digits, three products)."""
        check(lib().bk_set_f32_mode(self._ctx, int(mode)))

    def set_f64_mode(self, mode):
        """fp64 rows: BK_F64_EXACT (the fp64 MFMA), BK_F64_I8 (the Gram from exact
        int8 digit slices, error bound in the margin) or BK_F64_I8_CERTIFIED
        (exact re-run on a near tie); BK_F64_I8X2 / BK_F64_I8X2_CERTIFIED the
        two-digit slicing."""
        check(lib().bk_set_f64_mode(self._ctx, int(mode)))

    def graph_enable(self, on=True):
        """Replay multikrum_device_ptr calls as hipGraphs (bk_graph_enable)."""
        check(lib().bk_graph_enable(self._ctx, 1 if on else 0))

    def timing_select(self, kernels):
        """Time only these kernels (names from _lib.ALL_KERNELS)."""
        mask = 0
        for k in kernels:
            mask |= 1 << _lib.K[k]
        check(lib().bk_timing_select(self._ctx, mask))

    def timing_stride(self, every):
        """Record a timed kernel's events on every `every`-th launch (bk_timing_stride)."""
        check(lib().bk_timing_stride(self._ctx, int(every)))

    def timing_read(self):
        out = {}
        for i, name in enumerate(_lib.ALL_KERNELS):
            ms = ctypes.c_double(0)
            cnt = ctypes.c_int64(0)
            check(lib().bk_timing_read(self._ctx, i, ctypes.byref(ms), ctypes.byref(cnt)))
            if cnt.value:
                out[name] = {"total_ms": ms.value, "count": cnt.value,
                             "avg_ms": ms.value / cnt.value}
        return out

    def plan(self, n, d):
        v = [ctypes.c_int64(0) for _ in range(4)]
        check(lib().bk_plan(self._ctx, n, d, *[ctypes.byref(x) for x in v]))
        return dict(zip(("S", "kc", "ntile", "nwg"), (x.value for x in v)))


def comm_unique_id():
    buf = ctypes.create_string_buffer(_lib.BK_UNIQUE_ID_BYTES)
    check(lib().bk_comm_unique_id(buf))
    return buf.raw


_default = {}


def default_engine(device=0):
    if device not in _default:
        _default[device] = Engine(device)
    return _default[device]


def _as_matrix(deltas):
    # logistic_validator.py:41 -- deltas = np.array(deltas)
    X = np.asarray(deltas)
    if X.dtype not in (np.float64, np.float32):
        X = np.array(deltas, dtype=np.float64)
    return X


def krum(deltas, clip, engine: Optional[Engine] = None):
    """Indices of the n - clip updates with the lowest Krum scores.

    Mirrors ``krum(deltas, clip)`` (logistic_validator.py:36-49); the result is
    the same index set, returned ascending.
    """
    X = _as_matrix(deltas)
    n = len(X)
    if clip < 1 or clip >= n:
        # np.argpartition(scores, n - clip) raises for kth == n (clip == 0)
        raise ValueError("kth(=%d) out of bounds (%d)" % (n - clip, n))
    sel, _, _ = (engine or default_engine()).multikrum(X, clip, want_scores=False,
                                                       want_mean=False)
    return sel


def krum_batch(deltas, clip, engine: Optional[Engine] = None):
    """krum(deltas[b], clip) for every batch b of a sequence of equally shaped
    batches (B x n x d), in one call: a (B, n - clip) array of ascending
    indices.  Raises krum's ValueError for clip outside [1, n)."""
    X = _as_matrix(deltas)
    if X.ndim != 3:
        raise ValueError("deltas must be B batches of n updates of d values")
    n = X.shape[1]
    if clip < 1 or clip >= n:
        raise ValueError("kth(=%d) out of bounds (%d)" % (n - clip, n))
    sel, _, _ = (engine or default_engine()).multikrum_batch(X, clip, want_scores=False,
                                                             want_mean=False)
    return sel


def krum_ragged(list_of_deltas, clips, engine: Optional[Engine] = None):
    """[krum(deltas, clip) for deltas, clip in zip(list_of_deltas, clips)] in
    one call: the batches may differ in their number of updates (they share d);
    clips an int or one clip per batch.  A list of ascending index arrays.
    Raises krum's ValueError for a clip outside [1, n) of its batch."""
    Xs = [_as_matrix(deltas) for deltas in list_of_deltas]
    if not Xs:
        raise ValueError("need at least one batch of updates")
    if np.ndim(clips) == 0:
        clips = [clips] * len(Xs)
    if len(clips) != len(Xs):
        raise ValueError("clips must be an int or one clip per batch (%d batches)" % len(Xs))
    for X, clip in zip(Xs, clips):
        if X.ndim != 2:
            raise ValueError("every batch must be n updates of d values")
        if clip < 1 or clip >= len(X):
            raise ValueError("kth(=%d) out of bounds (%d)" % (len(X) - clip, len(X)))
    if len({X.dtype for X in Xs}) > 1:
        Xs = [X.astype(np.float64) for X in Xs]
    out = (engine or default_engine()).multikrum_ragged(Xs, [int(c) for c in clips],
                                                        want_scores=False, want_mean=False)
    return [sel for sel, _, _ in out]


def krum_mean(deltas, clip, engine: Optional[Engine] = None):
    """(selected indices, mean of the selected deltas): the aggregate the
    reference leaves commented out at logistic_validator.py:51."""
    X = _as_matrix(deltas)
    n = len(X)
    if clip < 1 or clip >= n:
        raise ValueError("kth(=%d) out of bounds (%d)" % (n - clip, n))
    sel, _, mean = (engine or default_engine()).multikrum(X, clip, want_scores=False,
                                                          want_mean=True)
    return sel, mean


def get_krum_scores(X, groupsize, engine: Optional[Engine] = None):
    """Krum score of every row: sum of its groupsize-2 smallest distances to
    the others (logistic_validator.py:54-65).  groupsize = n - clip."""
    X = _as_matrix(X)
    n = len(X)
    f = n - int(groupsize)
    if f < 1 or f >= n:
        raise ValueError("groupsize must satisfy 1 <= n - groupsize < n")
    _, sc, _ = (engine or default_engine()).multikrum(X, f, want_scores=True, want_mean=False)
    return sc


@dataclass
class Update:
    """DistSys/update.go:13-22 (the fields the verifier path reads)."""
    SourceID: int
    Iteration: int = 0
    Delta: Optional[np.ndarray] = None
    Commitment: bytes = b""
    Noise: Optional[np.ndarray] = None
    NoisedDelta: Optional[np.ndarray] = None
    Accepted: bool = False
    SignatureList: List[bytes] = field(default_factory=list)


class KRUMValidator:
    """DistSys/krum.go:22-29, with getTopKRUMIndex running on libbk."""

    def __init__(self, num_adversaries=0.5, engine: Optional[Engine] = None, device=0,
                 collect=False, n_cap=128, wide=False, noised=False, tiny=False,
                 wide_arrive=False):
        """collect=True (opt-in): add_update streams each update's NoisedDelta
        to the engine's collection as it arrives (bk_collect_add), and
        compute_scores only finishes (bk_collect_finish) in SourceID order;
        n_cap bounds the updates of one round (KRUM_UPDATETHRESH).  wide=True
        (with collect) turns the engine's wide one-launch finish on when the
        round begins (Engine.set_collect_wide: the CNN models' d).  noised=True
        (with collect): add_update sends update.Delta and update.Noise through
        the noised add (bk_collect_add_noised; k = 1 when Noise is present, k =
        0 when it is absent, as the shim does), so NoisedDelta is never built on
        the host; noised_delta(i) reads it back from the row store when asked.
        tiny=True (with collect, with or without noised) turns the engine's
        one-workgroup tiny collection on when the round begins
        (Engine.set_collect_tiny: creditcard's d, at most 16 updates).
        wide_arrive=True (with collect and wide) turns the fused wide last
        arrival on as well (Engine.set_collect_wide_arrive): add_update(u,
        last=True) hands a row of more than 32 KiB over through pinned staging
        (bk_stage_alloc, as the cgo shim packs Go's rows), so that the copy and
        k_collect_arrive_wide are the whole call."""
        self.UpdateList: List[Update] = []
        self.AcceptedList: List[int] = []
        self.NumAdversaries = num_adversaries  # fixed at 0.5 (main.go:783)
        self._engine = engine
        self._device = device
        self._collect = bool(collect)
        self._n_cap = int(n_cap)
        self._wide = bool(wide)
        self._noised = bool(noised)
        self._tiny = bool(tiny)
        self._wide_arrive = bool(wide_arrive)
        if self._noised and not self._collect:
            raise ValueError("noised=True needs collect=True")
        if self._tiny and not self._collect:
            raise ValueError("tiny=True needs collect=True")
        if self._wide_arrive and not (self._collect and self._wide):
            raise ValueError("wide_arrive=True needs collect=True and wide=True")
        self._slots: List[int] = []  # collect mode: arrival slot of UpdateList[i]

    def initialize(self):
        # krum.go:31-44 bound pyKRUMFunc; here: create the engine context
        if self._engine is None:
            self._engine = default_engine(self._device)
        return self

    def check_if_accepted(self, peer_id):
        # krum.go:47-73 (the isPoisoning bypass at :51-58 is dead code: the
        # global is never set, main.go:843 declares a local)
        return any(self.UpdateList[i].SourceID == peer_id for i in self.AcceptedList)

    def add_update(self, update, last=False):
        """VerifyUpdateKRUM's append (krum.go:291).  In collect mode the update's
        NoisedDelta is uploaded and folded into the Gram now.  last=True is the
        threshold-th arrival (krum.go:291-314): the append, the sort by SourceID
        and Krum in one engine call (bk_collect_add_finish; noised mode:
        bk_collect_add_noised_finish on Delta and Noise), AcceptedList set on
        return; outside collect mode it is add_update, then compute_scores."""
        if last and self._collect and self._slots:
            row = np.ascontiguousarray(update.Delta if self._noised else update.NoisedDelta,
                                       dtype=np.float64)
            ups = self.UpdateList + [update]
            slots = self._slots + [len(self._slots)]  # the new slot: the rows collected so far
            by_id = sorted(range(len(ups)), key=lambda i: ups[i].SourceID)
            order = [slots[i] for i in by_id]
            n = len(ups)
            clip = int(self.NumAdversaries * float(n))
            if self._noised:
                slot, sel, _, _ = self._engine.collect_add_noised_finish(
                    row, update.Noise, order=order, n=n, f=clip, want_scores=False,
                    want_mean=False)
            elif self._wide_arrive and row.nbytes > 32768:
                slot, sel = self._last_pinned(row, order, n, clip)
            else:
                slot, sel, _, _ = self._engine.collect_add_finish(
                    row, order=order, n=n, f=clip, want_scores=False, want_mean=False)
            assert slot == slots[-1]
            self.UpdateList = [ups[i] for i in by_id]
            self._slots = order
            self.AcceptedList = [int(i) for i in sel]
            return
        if last:
            self.add_update(update)
            self.compute_scores()
            return
        if self._collect:
            if self._engine is None:
                self.initialize()
            row = np.ascontiguousarray(update.Delta if self._noised else update.NoisedDelta,
                                       dtype=np.float64)
            if not self._slots:
                if self._wide:
                    self._engine.set_collect_wide(True)
                if self._tiny:
                    self._engine.set_collect_tiny(True)
                if self._wide_arrive:
                    self._engine.set_collect_wide_arrive(True)
                self._engine.collect_begin(self._n_cap, row.shape[0], np.float64)
            if self._noised:
                self._slots.append(self._engine.collect_add_noised(row, update.Noise))
            else:
                self._slots.append(self._engine.collect_add(row))
        self.UpdateList.append(update)

    def _last_pinned(self, row, order, n, clip):
        """the last arrival from pinned staging: (slot, sel)"""
        pin = ctypes.c_void_p()
        check(lib().bk_stage_alloc(self._engine.ctx, row.nbytes, ctypes.byref(pin)))
        try:
            ctypes.memmove(pin, row.ctypes.data, row.nbytes)
            order = np.ascontiguousarray(order, dtype=np.int64)
            sel = np.empty(n - clip, dtype=np.int64)
            slot, m = self._engine.collect_add_finish_ptr(pin.value, _lib.BK_HOST_PINNED,
                                                          order.ctypes.data, n, clip,
                                                          sel.ctypes.data)
            assert m == n - clip
        finally:
            lib().bk_stage_free(self._engine.ctx, pin)
        return slot, sel

    def noised_delta(self, i):
        """noised mode: UpdateList[i].NoisedDelta, read back from the row store
        on first use (bk_collect_read_rows) and kept on the update."""
        if not self._noised:
            raise ValueError("noised_delta needs KRUMValidator(collect=True, noised=True)")
        u = self.UpdateList[i]
        if u.NoisedDelta is None:
            u.NoisedDelta = self._engine.collect_read_rows([self._slots[i]])[0]
        return u.NoisedDelta

    def compute_scores(self):
        # krum.go:77-98
        if self._collect:
            # krum.go:202-210 / 306-314: the updates sorted by SourceID, then Krum;
            # the finish takes the matching arrival slots as its order
            by_id = sorted(range(len(self.UpdateList)), key=lambda i: self.UpdateList[i].SourceID)
            self.UpdateList = [self.UpdateList[i] for i in by_id]
            self._slots = [self._slots[i] for i in by_id]
            n = len(self.UpdateList)
            clip = int(self.NumAdversaries * float(n))
            sel, _, _ = self._engine.collect_finish(order=self._slots, n=n, f=clip,
                                                    want_scores=False, want_mean=False)
            self.AcceptedList = [int(i) for i in sel]
            return
        running = [u.NoisedDelta for u in self.UpdateList]
        self.AcceptedList = self.get_top_krum_index(running)

    def get_top_krum_index(self, deltas) -> List[int]:
        # krum.go:100-166: adversaryCount := int(NumAdversaries * float64(n))
        n = len(deltas)
        clip = int(self.NumAdversaries * float(n))
        if self._engine is None:
            self.initialize()
        # the rows go to libbk as they are (bk_multikrum_rows: packed on its
        # host threads into pinned memory, as the cgo shim hands Go's slices)
        rows = [np.asarray(r, dtype=np.float64) for r in deltas]
        sel, _, _ = self._engine.multikrum_rows(rows, clip, want_scores=False, want_mean=False)
        return [int(i) for i in sel]

    def flush_collected_updates(self, collecting_updates=False):
        # krum.go:169-176
        if not collecting_updates:
            self.UpdateList = []
            self.AcceptedList = []
            self._slots = []  # collect mode: the next add_update begins again
