"""Host-side mirror of the reference's `flash_join` module (PYBIND11_MODULE, hash_join.cpp:598-640).

Same thirteen names, same keyword arguments (`build_keys, build_values, probe_keys`), same
return value `(total_results: int, core_duration_sec: float)` for every join, `initialize()`
returning None.  The join itself runs in libflashjoin_hip.so (HIP kernels for gfx950) through the
C ABI of include/flashjoin.h; there is no CPU implementation behind these functions.

Differences from the reference, all deliberate:
  * non-contiguous inputs are made contiguous instead of being silently misread;
  * `build_values` shorter than `build_keys` raises ValueError instead of reading out of bounds;
  * `core_duration_sec` is the device-resident time (HIP events); PCIe copies of NumPy inputs
    are reported separately in `last_timings()`;
  * opt-in `return_arrays=True` returns the materialised pairs the reference computes and drops
    (hash_join.cpp:365-380): `(count, seconds, keys, values)`;
  * torch tensors that already live on a ROCm device are joined in place (no PCIe); so is any device array that
    speaks DLPack (`__dlpack__` / `__dlpack_device__`); pandas / Arrow / list inputs go through `np.asarray`;
  * the "scalar" functions (`hash_join*`: ONE table for the whole build side) run the partitioned plan by default:
    a table that does not fit LDS costs a cache-missing 64-B access per probe in HBM, more traffic than two
    streaming partition passes, so on MI355X it is the slower way to the same result at every size.
    `set_option("scalar_hbm_table", 1)` restores the literal algorithm (HBM table with linear probing over 8-slot
    groups, bloom word per group for the `_bloom` variants); it is also the fallback when a partition overflows LDS.
"""
from __future__ import annotations

import ctypes
import threading
from typing import Any, Dict, Optional, Tuple

import numpy as np

from . import _lib
from ._lib import FjTimings, check

ALGO_ADAPTIVE, ALGO_SCALAR, ALGO_RADIX = 0, 1, 2
ALGO_MANY_TO_MANY = 0x10          # FJ_ALGO_MANY_TO_MANY: OR'ed into algo (extension, include/flashjoin.h)
ALGO_LEFT_OUTER = 0x20            # FJ_ALGO_LEFT_OUTER: left outer join, np rows (extension)
ALGO_ANTI = 0x40                  # FJ_ALGO_ANTI: the probe rows without a partner (extension)
ALGO_ROW_IDS = 0x80               # FJ_ALGO_ROW_IDS: output rows hold row positions (gather maps) instead of keys and values (extension)
ALGO_FULL_OUTER = 0x100           # FJ_ALGO_FULL_OUTER: full outer join, np + r rows; the count is the pair (m, r) (extension)
ALGO_ALL_COPIES = 0x200           # FJ_ALGO_ALL_COPIES: modifier of LEFT_OUTER / FULL_OUTER - every copy of a duplicated build key; the count is (P, r, u) (extension)
ALGO_PROBE_ORDER = 0x800          # FJ_ALGO_PROBE_ORDER: one row per probe row at the probe row's position - np values and / or an np-byte mask (extension)
ALGO_BUILD_ORDER = 0x1000         # FJ_ALGO_BUILD_ORDER: one word per build row at the build row's position - nb counts and / or nb sums of a probe-side column (extension)
ALGO_AGG_MIN = 0x4000             # FJ_ALGO_AGG_MIN: modifier of ALGO_BUILD_ORDER - the values output holds the minimum instead of the sum (extension)
ALGO_AGG_MAX = 0x8000             # FJ_ALGO_AGG_MAX: ... the maximum
ALGO_AGG_SIGNED = 0x10000         # FJ_ALGO_AGG_SIGNED: modifier of AGG_MIN / AGG_MAX - the words compare as two's-complement int64 instead of uint64
ALGO_GROUP_BY = 0x40000           # FJ_ALGO_GROUP_BY: group-by on ONE relation (the build side) - its g distinct keys and one aggregate per key; AGG_* and ROW_IDS modify it (extension)
ALGO_INVERSE = 0x100000           # FJ_ALGO_INVERSE: modifier of ALGO_GROUP_BY - the values output holds the group id of EVERY row, at the row's position (extension)
ALGO_RETAIN_BUILD = 0x400000      # FJ_ALGO_RETAIN_BUILD: modifier of ALGO_PROBE_ORDER - the call also leaves its build side prepared on the context (extension)
ALGO_REUSE_BUILD = 0x800000       # FJ_ALGO_REUSE_BUILD: modifier of ALGO_PROBE_ORDER - no build side in the call: the context's prepared one is probed (extension)
ALGO_ACCUMULATE = 0x1000000       # FJ_ALGO_ACCUMULATE: modifier of ALGO_BUILD_ORDER | ALGO_REUSE_BUILD - the outputs are combined into as they are instead of filled first (extension)
ALGO_AGG_FLOAT = 0x2000000        # FJ_ALGO_AGG_FLOAT: modifier of ALGO_BUILD_ORDER / ALGO_GROUP_BY - the value column and the values output hold IEEE-754 float64 words: float sum, or float min / max with AGG_MIN / AGG_MAX (extension)
ALGO_AGG_ALL = 0x4000000          # FJ_ALGO_AGG_ALL: modifier of ALGO_GROUP_BY - the values output holds FOUR planes: row count, sum, minimum and maximum of the value column (extension)
ALGO_AGG_MERGE = 0x10000000       # FJ_ALGO_AGG_MERGE: modifier of ALGO_GROUP_BY | ALGO_AGG_ALL - the input rows are PARTIAL aggregates (a key and four planes: count, sum, min, max) and the rows of one key are combined (extension)
ALGO_KEY_PAIR = 0x20000000        # FJ_ALGO_KEY_PAIR: modifier of ALGO_GROUP_BY | ALGO_INVERSE - the key is the PAIR (keys, values): the values output holds every row's group id, the keys output the row index of each group's first occurrence (extension)
ALGO_GROUP_ROWS = 0x40000000       # FJ_ALGO_GROUP_ROWS: modifier of ALGO_GROUP_BY alone - the values output holds TWO planes: the row indices in group-contiguous order and the first of them that belongs to each group, a CSR of row indices (extension)
ALGO_AGG_ARG = 0x8000000          # FJ_ALGO_AGG_ARG: modifier of ALGO_GROUP_BY with AGG_MIN or AGG_MAX - the values output holds TWO planes: the row index of each group's extreme (smallest index on ties) and the extreme (extension)
_OUTER = ALGO_LEFT_OUTER | ALGO_ANTI

_ctxs: Dict[int, int] = {}
_ctx_locks: Dict[int, Any] = {}
_last: Optional[FjTimings] = None


def _is_torch_tensor(x: Any) -> bool:
    return type(x).__module__.startswith("torch") and hasattr(x, "data_ptr")


def _as_u64_host(a: Any, name: str) -> np.ndarray:
    """array_t<uint64_t> forcecast semantics: uint64 zero-copy, int64 reinterpreted bit-for-bit,
    anything else value-cast; N-D inputs are flattened (hash_join.cpp:317)."""
    arr = np.asarray(a)
    if arr.dtype == np.int64:
        arr = arr.view(np.uint64) if arr.flags.c_contiguous else np.ascontiguousarray(arr).view(np.uint64)
    elif arr.dtype != np.uint64:
        if arr.dtype.kind not in "iufb":
            raise TypeError(f"{name}: cannot convert dtype {arr.dtype} to uint64")
        arr = arr.astype(np.uint64, casting="unsafe")
    arr = np.ascontiguousarray(arr).reshape(-1)
    if arr.ctypes.data % 16:
        arr = np.require(arr.copy(), requirements=["ALIGNED", "C"])
    return arr


_FLOAT64_HINT = "; a floating-point column is aggregated as numbers with float64=True"


def _float_words(name: str, what: str, values: Any, signed: Any = None):
    """float64=True: a floating-point value column as the 8-byte words the native library reads (FJ_ALGO_AGG_FLOAT), in the container
    it came in.  NumPy float64 and torch.float64 are reinterpreted in place (a view, no copy); narrower floats are widened first, which
    is exact.  Anything that is not floating point is refused: its words would be read as doubles."""
    if signed is not None:
        raise TypeError(f"{name}: signed must be None with float64=True (a float64 carries its own sign), got {signed!r}")
    values = _from_dlpack_if_device(values)
    if _is_torch_tensor(values):
        import torch
        if not values.dtype.is_floating_point:
            raise TypeError(f"{name}: float64=True needs floating-point {what}, got {values.dtype}")
        if values.dtype != torch.float64:
            values = values.double()
        return values.view(torch.int64)
    values = np.asarray(values)
    if values.dtype.kind != "f" or values.dtype.itemsize > 8:
        raise TypeError(f"{name}: float64=True needs floating-point {what} (float64, float32 or float16), got dtype {values.dtype}")
    if values.dtype != np.float64:
        values = values.astype(np.float64)
    return values.view(np.uint64)


def _as_float64_words(buf: Any):
    """the int64 words of a float64 buffer (a view), where it lives"""
    if _is_torch_tensor(buf):
        import torch
        return buf.view(torch.int64)
    return buf.view(np.int64)


def _as_float64(words: Any):
    """the float64 numbers an aggregate's int64 / uint64 words hold (a view), where they live"""
    if words is None:
        return None
    if _is_torch_tensor(words):
        import torch
        return words.view(torch.float64)
    return words.view(np.float64)


def context(device: int) -> int:
    """One native context (workspace, events) per device, created on first use."""
    if device not in _ctxs:
        L = _lib.load()
        h = L.fj_ctx_create(int(device))
        if not h:
            raise RuntimeError(_lib.last_error())
        _ctxs[device] = h
    return _ctxs[device]


def workspace_bytes(device: Optional[int] = None) -> int:
    """Device memory the native contexts keep cached between joins (grow-only until trim_workspace)."""
    L = _lib.load()
    return sum(int(L.fj_ctx_workspace_bytes(h)) for d, h in _ctxs.items() if device is None or d == device)


def trim_workspace(device: Optional[int] = None) -> None:
    """Give the cached workspace back to the device (tens of GB after a 1B-row join); contexts stay usable."""
    L = _lib.load()
    for d, h in list(_ctxs.items()):
        if device is None or d == device:
            with _ctx_locks.setdefault(d, threading.RLock()):     # not between another thread's count and emit calls
                check(L.fj_ctx_trim(h))
    check(L.fj_ctx_trim(None))                  # the context behind the NumPy entry


def set_option(name: str, value: int) -> None:
    """Process-wide dispatch option of the native library: "radix_threshold", "scalar_hbm_table", "mm_heavy_keys",
    "mm_heavy_outer", ... (the list: include/flashjoin.h).  "mm_heavy_keys" = 1 lets the many-to-many INNER join take a build key with
    thousands of copies; "mm_heavy_outer" = 1 does the same for left_join / full_join / join_indices with duplicates="all".  The two
    are independent, both default to 0 and accept only 0 and 1."""
    check(_lib.load().fj_set_option(name.encode(), int(value)))


def get_option(name: str) -> int:
    v = int(_lib.load().fj_get_option(name.encode()))
    if v < 0:
        raise KeyError(_lib.last_error())
    return v


def last_timings() -> Optional[dict]:
    """Phase timings (ms) of the most recent join on this thread."""
    return _last.as_dict() if _last is not None else None


def _take_host(ptr, rows: int, dtype=np.uint64) -> np.ndarray:
    """`rows` elements of a library-owned host result, as a copy the caller keeps (fj_free_host takes the original); no rows: an
    empty array of that dtype, whatever the pointer holds"""
    if not rows:
        return np.empty(0, dtype)
    return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape=(rows,)).copy()


def _host_call(algo: int, bloom: int, materialize: int, a, b, rows_a: int, c, rows_c: int, want0: bool, want1: bool, read):
    """ONE fj_join_host call on NumPy word columns (None: a null pointer): (count, seconds, what `read` returned).  count is the
    three words the library may fill - a full outer join fills two (matched probe rows, unmatched build rows), ALL_COPIES three,
    every other form the first.  The call's timings become last_timings().  want0 / want1: which of the two library-owned results
    are asked for; `read(count, out0, out1)` copies what it needs of them with _take_host, and both are freed whatever it does.
    read=None: no result is asked for, so there is nothing to free.  A failing call raises before anything is read or freed: the
    library hands out no result then."""
    global _last
    L = _lib.load()
    ptr = lambda x: x.ctypes.data if x is not None else None
    cnt, sec = (ctypes.c_uint64 * 3)(0, 0, 0), ctypes.c_double(0.0)
    out0, out1 = ctypes.c_void_p(), ctypes.c_void_p()
    check(L.fj_join_host(algo, bloom, materialize, ptr(a), ptr(b), rows_a, ptr(c), rows_c, cnt, ctypes.byref(sec),
                         ctypes.byref(out0) if want0 else None, ctypes.byref(out1) if want1 else None))
    t = FjTimings()
    L.fj_last_timings(ctypes.byref(t))
    _last = t
    count = (int(cnt[0]), int(cnt[1]), int(cnt[2]))
    if read is None:
        return count, float(sec.value), None
    try:
        res = read(count, out0, out1)
    finally:
        L.fj_free_host(out0)
        L.fj_free_host(out1)
    return count, float(sec.value), res


def _join_host(algo: int, bloom: int, materialize: int, bk, bv, pk, return_arrays: bool):
    bk, pk = _as_u64_host(bk, "build_keys"), _as_u64_host(pk, "probe_keys")
    bv = _as_u64_host(bv, "build_values") if bv is not None else None      # (None: an anti join, which reads no value)
    if bv is not None and bv.size < bk.size:
        raise ValueError(f"build_values has {bv.size} elements, build_keys has {bk.size}")
    want = bool(materialize and return_arrays)

    def read(c, ok, ov):
        if algo & ALGO_ALL_COPIES:          # P + u + r rows; the count is the triple (P, r, u)
            rows = sum(c)
        elif algo & ALGO_FULL_OUTER:        # np + r rows; the count is the pair (m, r)
            rows = pk.size + c[1]
        elif algo & ALGO_LEFT_OUTER:        # left outer: np rows
            rows = pk.size
        else:                               # inner: n pairs; anti: n keys and no values
            rows = c[0]
        keys_only = bool(algo & ALGO_ANTI) and not algo & (ALGO_ALL_COPIES | ALGO_FULL_OUTER | ALGO_LEFT_OUTER)
        return _take_host(ok, rows), (None if keys_only else _take_host(ov, rows))
    c, sec, arrays = _host_call(algo, bloom, materialize, bk, bv, bk.size, pk, pk.size, want, want, read if want else None)
    n = c if algo & ALGO_ALL_COPIES else c[:2] if algo & ALGO_FULL_OUTER else c[0]
    return (n, sec, *arrays) if want else (n, sec)


def _device_index(t) -> int:
    """the index of the ROCm device a tensor lives on (a device without an index: the current one)"""
    if t.device.index is not None:
        return t.device.index
    import torch
    return torch.cuda.current_device()


def _trim(buf, g: int):
    """The first g rows of a device buffer that was allocated with room for ANY result (the 3/4 rule).  A view of them would keep the
    whole buffer alive for as long as the caller keeps the result - 16 bytes per PROBE row for the pairs of a join, 16 GB at config
    3 for 8 GB of pairs.  So unless the rows fill most of it, hand back an exact-size copy (one device-to-device copy of g rows)
    and let the big buffer go.  A (P, cap) buffer of planes is cut along cap: (P, g)."""
    if buf is None:
        return None
    return buf[..., :g].clone() if g * 4 < buf.shape[-1] * 3 else buf[..., :g]


def _dev_tensor(t, name: str):
    import torch
    if t.dtype not in (torch.int64, torch.uint64):
        raise TypeError(f"{name}: device tensors must be int64/uint64, got {t.dtype}")
    t = t.reshape(-1)
    if not t.is_contiguous():
        t = t.contiguous()
    if t.data_ptr() % 16:
        t = t.clone()
    return t


def _room_for(np_rows: int, dev: int) -> bool:
    """Output buffers for ANY result of a materialising join (16 bytes per probe row) are worth allocating when they take at
    most a third of the device memory that is free right now."""
    import torch
    try:
        free, _ = torch.cuda.mem_get_info(dev)
    except Exception:                                          # noqa: BLE001
        return False
    return 16 * np_rows <= free // 3


def join_device(algo: int, bloom: int, materialize: int, bk, bv, pk, return_arrays: bool = False,
                hash_top_bits: int = 64, want_values: bool = True, want_mask: bool = False, want_counts: bool = True):
    """Device-resident join on torch ROCm tensors (int64 storage, bit-identical to uint64).
    want_values / want_mask: which outputs a probe-order join (ALGO_PROBE_ORDER) writes; not read otherwise.
    ALGO_BUILD_ORDER: bv is the PROBE side's value column (len(pk) words, or None); want_counts / want_values: the counts and the sums
    (ALGO_AGG_MIN / ALGO_AGG_MAX in algo: the minima / maxima)."""
    global _last
    import torch
    L = _lib.load()
    bk, pk = _dev_tensor(bk, "build_keys"), _dev_tensor(pk, "probe_keys")
    bv = _dev_tensor(bv, "probe_values" if algo & ALGO_BUILD_ORDER else "build_values") if bv is not None else None      # (None: an anti join, which reads no value)
    if bv is not None and not algo & ALGO_BUILD_ORDER and bv.numel() < bk.numel():
        raise ValueError(f"build_values has {bv.numel()} elements, build_keys has {bk.numel()}")
    dev = _device_index(bk)
    ctx = context(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    cnt = ctypes.c_uint64(0)
    t = FjTimings()
    bv_ptr = bv.data_ptr() if bv is not None else None
    if algo & ALGO_BUILD_ORDER:
        # build-order aggregate join: exactly nb int64 counts and / or nb int64 sums, one call, never a pending result, no emit.
        # Returns (P, seconds, counts or None, sums or None)
        want_sums = want_values and bv is not None
        if not (want_counts or want_sums):
            raise ValueError("build-order join: want_counts, probe values with want_values, or both")
        if bv is not None and bv.numel() != pk.numel():
            raise ValueError(f"probe_values has {bv.numel()} elements, probe_keys has {pk.numel()}")
        n_b = bk.numel()
        oc = torch.empty(n_b, dtype=torch.int64, device=bk.device) if want_counts else None
        osum = torch.empty(n_b, dtype=torch.int64, device=bk.device) if want_sums else None
        with _ctx_locks.setdefault(dev, threading.RLock()):
            check(L.fj_join_device(ctx, algo, bloom, materialize, bk.data_ptr(), bv_ptr if want_sums else None, n_b, pk.data_ptr(), pk.numel(), stream,
                                   hash_top_bits, ctypes.byref(cnt), oc.data_ptr() if want_counts else None,
                                   osum.data_ptr() if want_sums else None, n_b, ctypes.byref(t)))
        _last = t
        return int(cnt.value), t.total_ms * 1e-3, oc, osum
    if algo & ALGO_PROBE_ORDER:
        # probe-order join: exactly np int64 and / or np uint8, one call, never a pending result, no emit.  Returns
        # (m, seconds, values or None, mask or None) whatever return_arrays says: the arrays ARE the result
        if not (want_values or want_mask):
            raise ValueError("probe-order join: want_values, want_mask or both")
        n_p = pk.numel()
        ov = torch.empty(n_p, dtype=torch.int64, device=bk.device) if want_values else None
        om = torch.empty(n_p, dtype=torch.uint8, device=bk.device) if want_mask else None
        with _ctx_locks.setdefault(dev, threading.RLock()):
            check(L.fj_join_device(ctx, algo, bloom, materialize, bk.data_ptr(), bv_ptr, bk.numel(), pk.data_ptr(), n_p, stream,
                                   hash_top_bits, ctypes.byref(cnt), om.data_ptr() if want_mask else None,
                                   ov.data_ptr() if want_values else None, n_p, ctypes.byref(t)))
        _last = t
        return int(cnt.value), t.total_ms * 1e-3, ov, om
    if algo & ALGO_ALL_COPIES:
        # every copy of a duplicated build key: the size is not known up front - count, allocate exactly P + u + r rows, emit;
        # the two calls share the context's one pending result, so other threads stay out in between.  The count is (P, r, u)
        cnt3 = (ctypes.c_uint64 * 3)(0, 0, 0)
        with _ctx_locks.setdefault(dev, threading.RLock()):
            check(L.fj_join_device(ctx, algo, bloom, materialize, bk.data_ptr(), bv_ptr, bk.numel(), pk.data_ptr(), pk.numel(), stream,
                                   hash_top_bits, cnt3, None, None, 0, ctypes.byref(t)))
            c3 = (int(cnt3[0]), int(cnt3[1]), int(cnt3[2]))
            rows = sum(c3)
            ok = torch.empty(rows, dtype=torch.int64, device=bk.device)
            ov = torch.empty(rows, dtype=torch.int64, device=bk.device)
            if rows:
                check(L.fj_emit_pairs(ctx, ok.data_ptr(), ov.data_ptr(), rows, stream, ctypes.byref(t)))
        _last = t
        if not return_arrays:
            return c3, t.total_ms * 1e-3
        return c3, t.total_ms * 1e-3, ok, ov
    if algo & ALGO_FULL_OUTER:
        # full outer join: room for every row of both sides, one call, never a pending result; the count is the pair (m, r)
        n_p, n_b = pk.numel(), bk.numel()
        ok = torch.empty(n_p + n_b, dtype=torch.int64, device=bk.device)
        ov = torch.empty(n_p + n_b, dtype=torch.int64, device=bk.device)
        cnt2 = (ctypes.c_uint64 * 2)(0, 0)
        with _ctx_locks.setdefault(dev, threading.RLock()):
            check(L.fj_join_device(ctx, algo, bloom, materialize, bk.data_ptr(), bv_ptr, n_b, pk.data_ptr(), n_p, stream,
                                   hash_top_bits, cnt2, ok.data_ptr(), ov.data_ptr(), n_p + n_b, ctypes.byref(t)))
        m, r = int(cnt2[0]), int(cnt2[1])
        _last = t
        if not return_arrays:
            return (m, r), t.total_ms * 1e-3
        return (m, r), t.total_ms * 1e-3, _trim(ok, n_p + r), _trim(ov, n_p + r)
    if (algo & _OUTER) and materialize:
        # left outer / anti join: np-row buffers always (a left join HAS np rows), one call, never a pending result to emit
        left = bool(algo & ALGO_LEFT_OUTER)
        n_p = pk.numel()
        ok = torch.empty(n_p, dtype=torch.int64, device=bk.device)
        ov = torch.empty(n_p, dtype=torch.int64, device=bk.device) if left else None
        with _ctx_locks.setdefault(dev, threading.RLock()):
            check(L.fj_join_device(ctx, algo, bloom, materialize, bk.data_ptr(), bv_ptr, bk.numel(), pk.data_ptr(), n_p, stream,
                                   hash_top_bits, ctypes.byref(cnt), ok.data_ptr(), ov.data_ptr() if left else None, n_p, ctypes.byref(t)))
        n = int(cnt.value)
        _last = t
        if not return_arrays:
            return n, t.total_ms * 1e-3
        if left:
            return n, t.total_ms * 1e-3, ok, ov
        return n, t.total_ms * 1e-3, _trim(ok, n), None      # anti: the first n rows
    with _ctx_locks.setdefault(dev, threading.RLock()):      # count + emit are two calls on one context: keep other threads out
        out = None
        if (materialize and not (algo & (ALGO_MANY_TO_MANY | _OUTER)) and pk.numel() > 0 and bk.numel() > 0 and get_option("mat_single_pass")
                and _room_for(pk.numel(), dev)):      # (a many-to-many join can return more pairs than probe rows)
            # room for ANY result (the reference allocates the same, hash_join.cpp:330-334): the join may run in one pass over
            # the probe side; the pairs are the first n rows
            ok = torch.empty(pk.numel(), dtype=torch.int64, device=bk.device)
            ov = torch.empty(pk.numel(), dtype=torch.int64, device=bk.device)
            check(L.fj_join_device(ctx, algo, bloom, materialize, bk.data_ptr(), bv_ptr, bk.numel(), pk.data_ptr(),
                                   pk.numel(), stream, hash_top_bits, ctypes.byref(cnt), ok.data_ptr(), ov.data_ptr(), pk.numel(), ctypes.byref(t)))
            n = int(cnt.value)
            _last = t
            if return_arrays:
                return n, t.total_ms * 1e-3, _trim(ok, n), _trim(ov, n)
            return n, t.total_ms * 1e-3
        check(L.fj_join_device(ctx, algo, bloom, materialize, bk.data_ptr(), bv_ptr, bk.numel(), pk.data_ptr(),
                               pk.numel(), stream, hash_top_bits, ctypes.byref(cnt), None, None, 0, ctypes.byref(t)))
        n = int(cnt.value)
        if materialize and n > 0:
            ok = torch.empty(n, dtype=torch.int64, device=bk.device)
            ov = torch.empty(n, dtype=torch.int64, device=bk.device)
            check(L.fj_emit_pairs(ctx, ok.data_ptr(), ov.data_ptr(), n, stream, ctypes.byref(t)))
            out = (ok, ov)
        elif materialize:
            out = (torch.empty(0, dtype=torch.int64, device=bk.device), torch.empty(0, dtype=torch.int64, device=bk.device))
    _last = t
    if materialize and return_arrays:
        return n, t.total_ms * 1e-3, out[0], out[1]
    return n, t.total_ms * 1e-3


_DL_DEVICE_GPU = (2, 10)         # DLPack device types kDLCUDA (what torch-ROCm reports) and kDLROCM


def _from_dlpack_if_device(x: Any):
    """Device arrays of other libraries (CuPy-ROCm, JAX, Arrow-on-GPU, ...) enter through DLPack, zero-copy."""
    if _is_torch_tensor(x) or isinstance(x, np.ndarray) or not hasattr(x, "__dlpack_device__"):
        return x
    try:
        dev_type = int(x.__dlpack_device__()[0])
    except Exception:
        return x
    if dev_type not in _DL_DEVICE_GPU:
        return x
    import torch
    return torch.from_dlpack(x)


def _join(algo: int, bloom: int, materialize: int, build_keys, build_values, probe_keys, return_arrays: bool):
    build_keys, build_values, probe_keys = (_from_dlpack_if_device(x) if x is not None else None for x in (build_keys, build_values, probe_keys))
    if _is_torch_tensor(build_keys) and build_keys.is_cuda:
        return join_device(algo, bloom, materialize, build_keys, build_values, probe_keys, return_arrays)
    if _is_torch_tensor(build_keys):
        build_keys, build_values, probe_keys = (x.numpy() if x is not None else None for x in (build_keys, build_values, probe_keys))
    return _join_host(algo, bloom, materialize, build_keys, build_values, probe_keys, return_arrays)


# ---- the reference's exported names (hash_join.cpp:603-639) -------------------------------------
def adaptive_join(build_keys, build_values, probe_keys, return_arrays: bool = False):
    """Adaptively chooses between scalar and radix join for materialization. (hash_join.cpp:603)"""
    return _join(ALGO_ADAPTIVE, 0, 1, build_keys, build_values, probe_keys, return_arrays)


def adaptive_join_bloom(build_keys, build_values, probe_keys, return_arrays: bool = False):
    """Adaptive join with bloom filter for materialization. (hash_join.cpp:607)"""
    return _join(ALGO_ADAPTIVE, 1, 1, build_keys, build_values, probe_keys, return_arrays)


def adaptive_join_count(build_keys, build_values, probe_keys):
    """Adaptively chooses between scalar and radix join for counting. (hash_join.cpp:611)"""
    return _join(ALGO_ADAPTIVE, 0, 0, build_keys, build_values, probe_keys, False)


def adaptive_join_count_bloom(build_keys, build_values, probe_keys):
    """Adaptive join with bloom filter for counting. (hash_join.cpp:615)"""
    return _join(ALGO_ADAPTIVE, 1, 0, build_keys, build_values, probe_keys, False)


def hash_join_radix(build_keys, build_values, probe_keys, return_arrays: bool = False):
    """Forces the use of radix join for materialization. (hash_join.cpp:621)"""
    return _join(ALGO_RADIX, 0, 1, build_keys, build_values, probe_keys, return_arrays)


def hash_join(build_keys, build_values, probe_keys, return_arrays: bool = False):
    """Forces the use of scalar (non-partitioned) join for materialization. (hash_join.cpp:624)"""
    return _join(ALGO_SCALAR, 0, 1, build_keys, build_values, probe_keys, return_arrays)


def hash_join_radix_bloom(build_keys, build_values, probe_keys, return_arrays: bool = False):
    """Radix join with bloom tables, materialization. (hash_join.cpp:627)"""
    return _join(ALGO_RADIX, 1, 1, build_keys, build_values, probe_keys, return_arrays)


def hash_join_bloom(build_keys, build_values, probe_keys, return_arrays: bool = False):
    """Scalar join with bloom precheck, materialization. (hash_join.cpp:628)"""
    return _join(ALGO_SCALAR, 1, 1, build_keys, build_values, probe_keys, return_arrays)


def hash_join_count_radix(build_keys, build_values, probe_keys):
    """Forces the use of radix join for counting. (hash_join.cpp:630)"""
    return _join(ALGO_RADIX, 0, 0, build_keys, build_values, probe_keys, False)


def hash_join_count(build_keys, build_values, probe_keys):
    """Forces the use of scalar (non-partitioned) join for counting. (hash_join.cpp:633)"""
    return _join(ALGO_SCALAR, 0, 0, build_keys, build_values, probe_keys, False)


def hash_join_count_radix_bloom(build_keys, build_values, probe_keys):
    """Radix join with bloom tables, counting. (hash_join.cpp:636)"""
    return _join(ALGO_RADIX, 1, 0, build_keys, build_values, probe_keys, False)


def hash_join_count_bloom(build_keys, build_values, probe_keys):
    """Scalar join with bloom precheck, counting. (hash_join.cpp:637)"""
    return _join(ALGO_SCALAR, 1, 0, build_keys, build_values, probe_keys, False)


# ---- extension: many-to-many inner join (the reference deduplicates build keys, hash_join.cpp:125) -------------------
def inner_join_count(build_keys, build_values, probe_keys):
    """Number of (probe row, build row) pairs with equal keys - every duplicate build row counts (SQL inner join).
    Not part of the reference's API; same argument and return conventions as the other joins.
    A final partition of more than 4096 build rows (a key with thousands of copies) is refused unless
    set_option("mm_heavy_keys", 1): then it is joined in tiles of at most 4096 build rows."""
    return _join(ALGO_RADIX | ALGO_MANY_TO_MANY, 0, 0, build_keys, build_values, probe_keys, False)


def inner_join(build_keys, build_values, probe_keys, return_arrays: bool = False):
    """Materialises every (probe_key, build_value) pair of the many-to-many inner join; `return_arrays=True` returns them.
    Build keys with thousands of copies need set_option("mm_heavy_keys", 1) (inner_join_count)."""
    return _join(ALGO_RADIX | ALGO_MANY_TO_MANY, 0, 1, build_keys, build_values, probe_keys, return_arrays)


# ---- extension: left outer and anti joins (N:1 semantics: a duplicated build key matches with its FIRST occurrence's value) ---------
def _fill(vals, m: int, fill_value, end: Optional[int] = None):
    end = vals.shape[0] if end is None else end
    if fill_value == 0 or end <= m:
        return vals
    if _is_torch_tensor(vals):
        vals[m:end] = int(np.array(fill_value, dtype=np.uint64).view(np.int64))     # int64 storage of the uint64 word
    else:
        vals[m:end] = np.uint64(fill_value)
    return vals


def _all_copies(duplicates: str, who: str) -> bool:
    if duplicates not in ("first", "all"):
        raise ValueError(f"{who}: duplicates must be 'first' or 'all', got {duplicates!r}")
    return duplicates == "all"


def left_join(build_keys, build_values, probe_keys, return_arrays: bool = False, fill_value: int = 0, duplicates: str = "first"):
    """Left outer join: every probe row once.  Returns (m, seconds) or (m, seconds, keys, values), m = matched probe rows (what
    the counting joins return).  keys / values hold len(probe_keys) rows: rows [0, m) the matched (probe_key, build_value) pairs,
    rows [m, n) the unmatched probe keys with value `fill_value`; order within either range unspecified.

    duplicates="all" (SQL semantics; "first" is the N:1 rule above): a probe row yields one row per build row with its key.  Returns
    (P, u, seconds) or (P, u, seconds, keys, values): P pairs (what inner_join_count returns), u probe rows without a partner (what
    anti_join_count returns); P + u rows, `fill_value` in rows [P, P + u).  A build key with thousands of copies (a final partition
    of more than 4096 build rows) is refused unless set_option("mm_heavy_outer", 1): then that partition is joined in tiles."""
    if _all_copies(duplicates, "left_join"):
        res = _join(ALGO_ADAPTIVE | ALGO_LEFT_OUTER | ALGO_ALL_COPIES, 0, 1, build_keys, build_values, probe_keys, return_arrays)
        (P, _, u), sec = res[0], res[1]
        if not return_arrays:
            return P, u, sec
        return P, u, sec, res[2], _fill(res[3], P, fill_value, P + u)
    r = _join(ALGO_ADAPTIVE | ALGO_LEFT_OUTER, 0, 1, build_keys, build_values, probe_keys, return_arrays)
    if not return_arrays:
        return r
    m, sec, keys, vals = r
    return m, sec, keys, _fill(vals, m, fill_value)


def anti_join(build_keys, probe_keys, return_arrays: bool = False):
    """Anti join (NOT EXISTS / NOT IN): the probe rows whose key is not among the build keys.  Returns (u, seconds) or
    (u, seconds, keys) with the u unmatched probe keys, in unspecified order."""
    r = _join(ALGO_ADAPTIVE | ALGO_ANTI, 0, 1, build_keys, None, probe_keys, return_arrays)
    return r if not return_arrays else r[:3]


def anti_join_count(build_keys, probe_keys):
    """Number of probe rows whose key is not among the build keys: (u, seconds)."""
    return _join(ALGO_ADAPTIVE | ALGO_ANTI, 0, 0, build_keys, None, probe_keys, False)


# ---- extension: full outer join, fused into one call and one set of partition passes (csrc/fj_outer.hip) ---------------------------
def full_join(build_keys, build_values, probe_keys, return_arrays: bool = False, fill_value: int = 0, duplicates: str = "first"):
    """Full outer join (N:1).  Returns (m, r, seconds) or (m, r, seconds, keys, values) with len(probe_keys) + r rows:
    rows [0, m) the matched (probe_key, build_value) pairs (a duplicated build key: its FIRST occurrence's value), rows
    [m, len(probe_keys)) the unmatched probe keys with value `fill_value` - together what left_join returns - and behind them the r
    build rows (build_key, build_value) whose key is not among the probe keys, every copy of a duplicated key included.  Order
    within each range unspecified.

    duplicates="all" (SQL semantics): every copy of a duplicated build key pairs with the probe rows of its key.  Returns
    (P, u, r, seconds) or (P, u, r, seconds, keys, values) with P + u + r rows: rows [0, P) the pairs, rows [P, P + u) the unmatched
    probe keys with `fill_value`, rows [P + u, P + u + r) the build rows whose key is not among the probe keys.  A build key with
    thousands of copies is refused unless set_option("mm_heavy_outer", 1) (left_join)."""
    if _all_copies(duplicates, "full_join"):
        res = _join(ALGO_ADAPTIVE | ALGO_FULL_OUTER | ALGO_ALL_COPIES, 0, 1, build_keys, build_values, probe_keys, return_arrays)
        (P, r, u), sec = res[0], res[1]
        if not return_arrays:
            return P, u, r, sec
        return P, u, r, sec, res[2], _fill(res[3], P, fill_value, P + u)
    res = _join(ALGO_ADAPTIVE | ALGO_FULL_OUTER, 0, 1, build_keys, build_values, probe_keys, return_arrays)
    (m, r), sec = res[0], res[1]
    if not return_arrays:
        return m, r, sec
    keys, vals = res[2], res[3]
    n_p = keys.shape[0] - r
    if fill_value != 0 and n_p > m:
        vals[m:n_p] = (int(np.array(fill_value, dtype=np.uint64).view(np.int64)) if _is_torch_tensor(vals) else np.uint64(fill_value))
    return m, r, sec, keys, vals


# ---- extension: semi join (the N:1 inner join minus its value column; no new kernel) -------------------------------------------------
def semi_join(build_keys, probe_keys, return_arrays: bool = False):
    """Semi join (EXISTS / IN): the probe rows whose key is among the build keys, each once.  Returns (s, seconds) or
    (s, seconds, keys) with the s matched probe keys, in unspecified order.  No value column is asked of the caller: the build
    keys stand in for it and the join's value output is dropped."""
    if not return_arrays:
        return semi_join_count(build_keys, probe_keys)
    return _join(ALGO_ADAPTIVE, 0, 1, build_keys, build_keys, probe_keys, True)[:3]


def semi_join_count(build_keys, probe_keys):
    """Number of probe rows whose key is among the build keys: (s, seconds) - the N:1 count (a counting join reads no value)."""
    return _join(ALGO_ADAPTIVE, 0, 0, build_keys, build_keys, probe_keys, False)


# ---- extension: probe-order joins (one row per probe row, at the probe row's position; csrc/fj_aligned.hip) -------------------------
def _probe_order_host(algo: int, bk, bv, pk, want_values: bool, want_mask: bool):
    bk, pk = _as_u64_host(bk, "build_keys"), _as_u64_host(pk, "probe_keys")
    bv = _as_u64_host(bv, "build_values") if bv is not None else None
    if bv is not None and bv.size < bk.size:
        raise ValueError(f"build_values has {bv.size} elements, build_keys has {bk.size}")
    n = pk.size                             # the mask comes back where a join's keys do: one byte per probe row
    read = lambda c, om, ov: (_take_host(ov, n) if want_values else None, _take_host(om, n, np.uint8) if want_mask else None)
    c, sec, (vals, mask) = _host_call(algo, 0, 1, bk, bv, bk.size, pk, n, want_mask, want_values, read)
    return c[0], sec, vals, mask


def _probe_order(algo: int, build_keys, build_values, probe_keys, want_values: bool, want_mask: bool):
    """(m, seconds, values or None, mask or None): int64 values and a uint8 mask of len(probe_keys), where the inputs live"""
    build_keys, build_values, probe_keys = (_from_dlpack_if_device(x) if x is not None else None for x in (build_keys, build_values, probe_keys))
    if _is_torch_tensor(build_keys) and build_keys.is_cuda:
        return join_device(algo | ALGO_PROBE_ORDER, 0, 1, build_keys, build_values, probe_keys, want_values=want_values, want_mask=want_mask)
    if _is_torch_tensor(build_keys):
        build_keys, build_values, probe_keys = (x.numpy() if x is not None else None for x in (build_keys, build_values, probe_keys))
    m, sec, vals, mask = _probe_order_host(algo | ALGO_PROBE_ORDER, build_keys, build_values, probe_keys, want_values, want_mask)
    return m, sec, (vals.view(np.int64) if vals is not None else None), mask


def _fill_word(fill_value) -> int:
    if isinstance(fill_value, bool) or not isinstance(fill_value, (int, np.integer)):
        raise TypeError(f"lookup: fill_value must be an integer, got {type(fill_value).__name__}")
    fill_value = int(fill_value)
    if not -(1 << 63) <= fill_value < (1 << 64):
        raise ValueError("lookup: fill_value does not fit 64 bits")
    return fill_value


def _apply_fill(vals, mask, m: int, fill_value: int) -> None:
    if fill_value != 0 and m < vals.shape[0]:                # applied through the mask, as _fill does for left_join's ranges
        word = int(np.array(fill_value % (1 << 64), dtype=np.uint64).view(np.int64))     # int64 storage of the uint64 word
        if _is_torch_tensor(vals):
            vals.masked_fill_(mask == 0, word)
        else:
            vals[mask == 0] = word


def lookup(build_keys, build_values, probe_keys, fill_value: int = 0, return_mask: bool = False):
    """Dictionary / foreign-key lookup in probe order: values[i] is the build value of probe_keys[i] (a duplicated build key: its
    FIRST occurrence's), `fill_value` where the key is not among the build keys.  Returns (m, seconds, values) or, return_mask=True,
    (m, seconds, values, mask): m = probe rows with a partner (what the counting joins return), values int64 of len(probe_keys) (the
    storage of the uint64 words), mask uint8 1 / 0 per probe row.  One pass over the probe side: no counting pass, no compaction.
    NumPy arrays in, NumPy arrays out; torch ROCm tensors / DLPack are joined in place and the outputs live on their device."""
    fill_value = _fill_word(fill_value)
    if build_values is None:
        raise ValueError("lookup: build_values is required (isin / lookup_indices take none)")
    need_mask = return_mask or fill_value != 0
    m, sec, vals, mask = _probe_order(ALGO_ADAPTIVE, build_keys, build_values, probe_keys, True, need_mask)
    _apply_fill(vals, mask, m, fill_value)
    return (m, sec, vals, mask) if return_mask else (m, sec, vals)


def isin(probe_keys, build_keys):
    """Membership mask in probe order (torch.isin / the mark join of IN and EXISTS): (m, seconds, mask), mask[i] = 1 if probe_keys[i]
    is among the build keys, uint8 of len(probe_keys); m = mask.sum().  The mask-only form: no build value is read or asked for."""
    m, sec, _, mask = _probe_order(ALGO_ADAPTIVE, build_keys, None, probe_keys, False, True)
    return m, sec, mask


def lookup_indices(build_keys, probe_keys):
    """Gather map in probe order: (m, seconds, build_idx), build_idx[i] = 0-based row of the FIRST occurrence of probe_keys[i] among
    the build keys, -1 where there is none; int64 of len(probe_keys).  join_indices(how="left") without the compaction."""
    m, sec, idx, _ = _probe_order(ALGO_ADAPTIVE | ALGO_ROW_IDS, build_keys, None, probe_keys, True, False)
    return m, sec, idx


# ---- extension: a prepared build side - build once, probe many times (csrc/fj_prepared.hip) ------------------------------------------
def _device_scope(dev: int):
    """hipMalloc and hipMemcpy of the NumPy staging act on the calling thread's current device"""
    import contextlib
    try:
        import torch
    except ImportError:
        if dev != 0:
            raise RuntimeError("build_index: staging NumPy arrays on a device other than 0 needs torch (it selects the device)")
        return contextlib.nullcontext()
    return torch.cuda.device(dev)


class _Staged:
    """device buffers of a NumPy call (fj_device_malloc), freed on exit"""
    def __init__(self):
        self.L, self.ptrs = _lib.load(), []

    def alloc(self, nbytes: int) -> int:
        p = ctypes.c_void_p()
        check(self.L.fj_device_malloc(ctypes.byref(p), nbytes))
        self.ptrs.append(p)
        return p.value

    def upload(self, arr: np.ndarray) -> int:
        d = self.alloc(arr.nbytes)
        check(self.L.fj_memcpy_h2d(d, arr.ctypes.data, arr.nbytes))
        return d

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.L.fj_device_free(p)
        self.ptrs = []
        return False


class Index:
    """A build side prepared once (build_index) and probed any number of times: `lookup`, `isin` and `lookup_indices` return what the
    module functions of the same name return for (build_keys, build_values, probe_keys), without the build side's partition passes
    and first-occurrence logic in every call.  The index owns a native context of its own - the prepared side lives in device memory
    of that context, beside the workspace of the probe side's passes - and a lock: calls on one index are serialised, two indexes
    are independent.  A context manager; `close()` frees the device memory, after which every call raises.

    num_keys: distinct build keys (g); num_rows: build rows (nb); has_values: built with build_values; device: the ROCm device index."""

    def __init__(self, ctx: int, device: int, num_rows: int, num_keys: int, has_values: bool):
        self._ctx, self._lock = ctx, threading.RLock()
        self.device, self.num_rows, self.num_keys, self.has_values = device, num_rows, num_keys, has_values

    def close(self) -> None:
        with self._lock:
            ctx, self._ctx = self._ctx, None
            if ctx:
                _lib.load().fj_ctx_destroy(ctx)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:                                          # noqa: BLE001  (interpreter shutdown)
            pass

    def _probe(self, probe_keys, flags: int, want_values: bool, want_mask: bool):
        """(m, seconds, values or None, mask or None) as _probe_order returns them, against the prepared side"""
        global _last
        L = _lib.load()
        algo = ALGO_PROBE_ORDER | ALGO_REUSE_BUILD | flags
        cnt, t = ctypes.c_uint64(0), FjTimings()
        pk = _from_dlpack_if_device(probe_keys)
        if _is_torch_tensor(pk) and pk.is_cuda:
            import torch
            pk = _dev_tensor(pk, "probe_keys")
            dev = _device_index(pk)
            if dev != self.device:
                raise ValueError(f"probe_keys live on device {dev}, the index on device {self.device}")
            n_p = pk.numel()
            ov = torch.empty(n_p, dtype=torch.int64, device=pk.device) if want_values else None
            om = torch.empty(n_p, dtype=torch.uint8, device=pk.device) if want_mask else None
            stream = torch.cuda.current_stream(dev).cuda_stream
            with self._lock:
                if not self._ctx:
                    raise RuntimeError("this Index is closed")
                check(L.fj_join_device(self._ctx, algo, 0, 1, None, None, 0, pk.data_ptr(), n_p, stream, 64, ctypes.byref(cnt),
                                       om.data_ptr() if want_mask else None, ov.data_ptr() if want_values else None, n_p, ctypes.byref(t)))
            _last = t
            return int(cnt.value), t.total_ms * 1e-3, ov, om
        if _is_torch_tensor(pk):
            pk = pk.numpy()
        pk = _as_u64_host(pk, "probe_keys")
        n_p = pk.size
        vals = np.empty(n_p, np.int64) if want_values else None
        mask = np.empty(n_p, np.uint8) if want_mask else None
        with self._lock:
            if not self._ctx:
                raise RuntimeError("this Index is closed")
            with _device_scope(self.device), _Staged() as st:
                d_pk = st.upload(pk)
                d_ov = st.alloc(n_p * 8) if want_values else None
                d_om = st.alloc(n_p) if want_mask else None
                check(L.fj_join_device(self._ctx, algo, 0, 1, None, None, 0, d_pk, n_p, None, 64, ctypes.byref(cnt), d_om, d_ov, n_p, ctypes.byref(t)))
                if want_values:
                    check(L.fj_memcpy_d2h(vals.ctypes.data, d_ov, n_p * 8))
                if want_mask:
                    check(L.fj_memcpy_d2h(mask.ctypes.data, d_om, n_p))
        _last = t
        return int(cnt.value), t.total_ms * 1e-3, vals, mask

    def lookup(self, probe_keys, fill_value: int = 0, return_mask: bool = False):
        """lookup(build_keys, build_values, probe_keys, fill_value, return_mask) of this module against the prepared side"""
        fill_value = _fill_word(fill_value)
        if not self.has_values:
            raise ValueError("Index.lookup: this index was built without build_values (isin and lookup_indices need none)")
        need_mask = return_mask or fill_value != 0
        m, sec, vals, mask = self._probe(probe_keys, 0, True, need_mask)
        _apply_fill(vals, mask, m, fill_value)
        return (m, sec, vals, mask) if return_mask else (m, sec, vals)

    def isin(self, probe_keys):
        """isin(probe_keys, build_keys) of this module against the prepared side"""
        m, sec, _, mask = self._probe(probe_keys, 0, False, True)
        return m, sec, mask

    def lookup_indices(self, probe_keys):
        """lookup_indices(build_keys, probe_keys) of this module against the prepared side"""
        m, sec, idx, _ = self._probe(probe_keys, ALGO_ROW_IDS, True, False)
        return m, sec, idx

    # ---- build-order aggregates onto the prepared side (FJ_ALGO_BUILD_ORDER | FJ_ALGO_REUSE_BUILD [| FJ_ALGO_ACCUMULATE]) ----
    def _check_out(self, name: str, what: str, buf, on_device: bool, float64: bool = False):
        """a caller's accumulator: of the kind of probe_keys, int64 storage, num_rows elements, contiguous (before any native call).
        float64: a float aggregate's accumulator instead - float64, and everything about its kind is a TypeError that says so"""
        if float64:
            if on_device:
                import torch
                if not _is_torch_tensor(buf) or buf.dtype != torch.float64:
                    raise TypeError(f"{name}: with float64=True {what} must be a float64 torch tensor on the index's device, like probe_keys "
                                    f"(got {buf.dtype if _is_torch_tensor(buf) else type(buf).__name__})")
            elif not isinstance(buf, np.ndarray) or buf.dtype != np.float64 or not buf.flags.c_contiguous or not buf.flags.writeable:
                raise TypeError(f"{name}: with float64=True {what} must be a writable C-contiguous float64 NumPy array, like probe_keys "
                                f"(got {buf.dtype if isinstance(buf, np.ndarray) else type(buf).__name__})")
            buf = _as_float64_words(buf)                         # (the rest: the checks of the integer forms)
        if on_device:
            if not _is_torch_tensor(buf):
                raise TypeError(f"{name}: {what} must be a torch tensor on the index's device, like probe_keys (got {type(buf).__name__})")
            import torch
            if buf.dtype != torch.int64:
                raise TypeError(f"{name}: {what} must be int64, got {buf.dtype}")
            if not buf.is_cuda or _device_index(buf) != self.device:
                raise ValueError(f"{name}: {what} lives on {buf.device}, the index on device {self.device}")
            if buf.dim() != 1 or buf.numel() != self.num_rows:
                raise ValueError(f"{name}: {what} has shape {tuple(buf.shape)}, the index has {self.num_rows} rows")
            if not buf.is_contiguous():
                raise ValueError(f"{name}: {what} must be contiguous (it is combined into in place)")
        else:
            if not isinstance(buf, np.ndarray):
                raise TypeError(f"{name}: {what} must be a NumPy array, like probe_keys (got {type(buf).__name__})")
            if buf.dtype not in (np.int64, np.uint64):
                raise TypeError(f"{name}: {what} must be int64 or uint64, got {buf.dtype}")
            if buf.ndim != 1 or buf.size != self.num_rows:
                raise ValueError(f"{name}: {what} has shape {buf.shape}, the index has {self.num_rows} rows")
            if not buf.flags.c_contiguous or not buf.flags.writeable:
                raise ValueError(f"{name}: {what} must be a writable C-contiguous array (it is combined into in place)")

    def _group(self, name: str, probe_keys, probe_values, agg: int, out, counts_out, want_counts: bool, float64: bool = False):
        """(m, seconds, values or None, counts or None): num_rows int64 words each, where probe_keys live.  probe_values None: the
        count form (`out` is then the counts).  out / counts_out given: ALGO_ACCUMULATE, combined into in place and returned.
        float64 (agg carries ALGO_AGG_FLOAT, probe_values are the words of _float_words): the values, and `out`, are float64"""
        global _last
        L = _lib.load()
        want_vals = probe_values is not None
        if not want_vals:
            counts_out, out, want_counts = out, None, True
        want_counts = bool(want_counts) or counts_out is not None
        pk, pv = (_from_dlpack_if_device(x) if x is not None else None for x in (probe_keys, probe_values))
        on_device = _is_torch_tensor(pk) and pk.is_cuda
        if want_vals and want_counts and (out is None) != (counts_out is None):
            raise ValueError(f"{name}: out and counts_out are given together or not at all (one call either fills its outputs or combines into them)")
        accumulate = out is not None or counts_out is not None
        for what, buf in (("out" if want_vals else "out (the counts)", out if want_vals else counts_out), ("counts_out", counts_out if want_vals else None)):
            if buf is not None:
                self._check_out(name, what, buf, on_device, float64 and want_vals and what == "out")
        out_given = out
        if float64 and out is not None:                          # the words of the caller's float64 accumulator: a view, combined into in place
            out = _as_float64_words(out)
        algo = ALGO_BUILD_ORDER | ALGO_REUSE_BUILD | agg | (ALGO_ACCUMULATE if accumulate else 0)
        n_b = self.num_rows
        cnt, t = ctypes.c_uint64(0), FjTimings()
        if on_device:
            import torch
            pk = _dev_tensor(pk, "probe_keys")
            dev = _device_index(pk)
            if dev != self.device:
                raise ValueError(f"probe_keys live on device {dev}, the index on device {self.device}")
            n_p = pk.numel()
            if want_vals:
                if not (_is_torch_tensor(pv) and pv.is_cuda and pv.device == pk.device):
                    raise ValueError(f"{name}: probe_values must live on the device of probe_keys")
                pv = _dev_tensor(pv, "probe_values")
                if pv.numel() < n_p:
                    raise ValueError(f"{name}: probe_values has {pv.numel()} elements, probe_keys has {n_p}")
            ov = (out if out is not None else torch.empty(n_b, dtype=torch.int64, device=pk.device)) if want_vals else None
            oc = (counts_out if counts_out is not None else torch.empty(n_b, dtype=torch.int64, device=pk.device)) if want_counts else None
            dummy = torch.empty(2, dtype=torch.int64, device=pk.device) if n_b == 0 else None      # (an empty tensor has no address; nothing is written)
            ptr = lambda x: None if x is None else (x.data_ptr() if n_b else dummy.data_ptr())
            stream = torch.cuda.current_stream(dev).cuda_stream
            with self._lock:
                if not self._ctx:
                    raise RuntimeError("this Index is closed")
                check(L.fj_join_device(self._ctx, algo, 0, 1, None, pv.data_ptr() if want_vals and n_p else None, 0, pk.data_ptr() if n_p else None, n_p,
                                       stream, 64, ctypes.byref(cnt), ptr(oc), ptr(ov), n_b, ctypes.byref(t)))
            _last = t
            if float64:
                ov = out_given if out_given is not None else _as_float64(ov)
            return int(cnt.value), t.total_ms * 1e-3, ov, oc
        if _is_torch_tensor(pk):
            pk = pk.numpy()
        if _is_torch_tensor(pv):
            pv = pv.cpu().numpy()
        pk = _as_u64_host(pk, "probe_keys")
        n_p = pk.size
        if want_vals:
            pv = _as_u64_host(pv, "probe_values")
            if pv.size < n_p:
                raise ValueError(f"{name}: probe_values has {pv.size} elements, probe_keys has {n_p}")
        vals = (out if out is not None else np.empty(n_b, np.int64)) if want_vals else None
        counts = (counts_out if counts_out is not None else np.empty(n_b, np.int64)) if want_counts else None
        with self._lock:
            if not self._ctx:
                raise RuntimeError("this Index is closed")
            with _device_scope(self.device), _Staged() as st:
                d_pk = st.upload(pk)
                d_pv = st.upload(pv[:n_p]) if want_vals else None
                d_ov = st.alloc(max(n_b, 2) * 8) if want_vals else None
                d_oc = st.alloc(max(n_b, 2) * 8) if want_counts else None
                if accumulate and n_b:                               # the running aggregate goes up, is combined into and comes back
                    for d, h in ((d_ov, vals), (d_oc, counts)):
                        if h is not None:
                            check(L.fj_memcpy_h2d(d, h.ctypes.data, n_b * 8))
                check(L.fj_join_device(self._ctx, algo, 0, 1, None, d_pv if n_p else None, 0, d_pk if n_p else None, n_p, None, 64, ctypes.byref(cnt), d_oc, d_ov, n_b, ctypes.byref(t)))
                for d, h in ((d_ov, vals), (d_oc, counts)):
                    if h is not None and n_b:
                        check(L.fj_memcpy_d2h(h.ctypes.data, d, n_b * 8))
        _last = t
        if float64:
            vals = out_given if out_given is not None else _as_float64(vals)
        return int(cnt.value), t.total_ms * 1e-3, vals, counts

    def group_count(self, probe_keys, out=None):
        """Orders per customer over a batch: (m, seconds, counts), counts[i] = the rows of probe_keys whose key equals the index's build
        key i, int64 of num_rows, aligned with the build rows; m = probe rows with a partner = counts.sum() of this batch.
        FIRST-OCCURRENCE RULE (the Index rule: lookup_indices names the first row): a duplicated build key's count lands at the key's
        FIRST build row and every further copy holds 0 - group_join_count gives every copy the count; on distinct build keys the two
        agree bit for bit.  out=: a buffer of num_rows int64 (a contiguous device tensor on the index's device, used on the current
        stream, for device probe_keys; a writable C-contiguous int64 / uint64 NumPy array, staged up and back, for NumPy probe_keys) that
        the call ADDS into in place and returns (ALGO_ACCUMULATE): `m, s, acc = idx.group_count(pk0)`, then `idx.group_count(pk1, out=acc)`
        is a running aggregate over morsels.  Without out= a fresh, filled array is returned each time.  No build value is read: a
        keys-only index serves every group_* form."""
        m, sec, _, counts = self._group("Index.group_count", probe_keys, None, 0, out, None, True)
        return m, sec, counts

    def group_sum(self, probe_keys, probe_values, out=None, return_counts: bool = False, counts_out=None, float64: bool = False):
        """Revenue per product over a batch: (m, seconds, sums) or, with return_counts / counts_out, (m, seconds, sums, counts).  sums[i] =
        the sum modulo 2^64 of probe_values[j] over the rows j of probe_keys whose key equals build key i (int64 storage of the uint64
        words), at the key's FIRST build row; 0 in every other row (group_count: the first-occurrence rule).  probe_values has at least
        len(probe_keys) words; the first len(probe_keys) are read.  out= / counts_out=: accumulators the call combines into in place and
        returns (group_count); when counts are asked for, both are given or neither - one flag covers the call - and counts_out implies
        return_counts.
        float64=True: probe_values is a floating-point column (NumPy float64 and torch.float64 / DLPack are read in place, float32 /
        float16 are widened exactly; integers raise TypeError) and sums is float64 - a NumPy array, or a torch.float64 tensor on the
        device - 0.0 in every row without a partner; counts stay int64.  out= must then be float64 (a torch.float64 tensor on the
        index's device, or a writable C-contiguous NumPy float64 array; anything else is a TypeError), counts_out stays int64.  The sum
        is accumulated with atomic adds in an UNSPECIFIED ORDER: it can differ in its last bits from run to run and from a sequential
        sum.  A NaN makes the sum of its own key NaN and touches no other key."""
        if probe_values is None:
            raise ValueError("Index.group_sum: probe_values is required (group_count takes none)")
        if float64:
            pv = _float_words("Index.group_sum", "probe_values", probe_values)
            m, sec, vals, counts = self._group("Index.group_sum", probe_keys, pv, ALGO_AGG_FLOAT, out, counts_out, return_counts, float64=True)
            return (m, sec, vals, counts) if counts is not None else (m, sec, vals)
        m, sec, vals, counts = self._group("Index.group_sum", probe_keys, probe_values, 0, out, counts_out, return_counts)
        return (m, sec, vals, counts) if counts is not None else (m, sec, vals)

    def _group_minmax(self, name: str, flag: int, probe_keys, probe_values, out, return_counts, counts_out, signed, float64: bool = False):
        if probe_values is None:
            raise ValueError(f"{name}: probe_values is required (group_count takes none)")
        pv, signed, _ = _word_column(name, "probe_values", probe_values, signed, float64, integers_only=False)      # the sign of the container, as in group_join_min
        m, sec, vals, counts = self._group(name, probe_keys, pv, flag | _agg_flags(signed, float64), out, counts_out, return_counts, float64=float64)
        return (m, sec, vals, counts) if counts is not None else (m, sec, vals)

    def group_min(self, probe_keys, probe_values, out=None, return_counts: bool = False, counts_out=None, signed=None, float64: bool = False):
        """Cheapest offer per product over a batch: values[i] = the minimum of probe_values[j] over the rows j whose key equals build
        key i, at the key's FIRST build row (group_count: the first-occurrence rule).  signed=None follows the rule of group_join_min: a
        NumPy uint64 (torch.uint64) value column compares unsigned, everything else signed; True / False force it.  A row without a
        partner - every further copy of a duplicated key among them - holds the aggregate's identity, 2^64 - 1 (unsigned) or 2^63 - 1
        (signed); a true minimum equal to it is told apart by the counts.  The outputs are int64 storage of the words.  out= /
        counts_out= as for group_sum: the call takes the minimum of what `out` holds and the batch's - start a running minimum from a
        call without out=, or from a buffer filled with the identity - and rows without a partner keep their contents.
        float64=True: probe_values is a floating-point column (as for group_sum), `signed` must stay None (TypeError otherwise) and the
        minima are float64, compared as numbers; the identity is +inf, out= must be float64 (group_sum), counts_out stays int64.  Which
        zero comes back for a key that holds both -0.0 and +0.0 is unspecified; a NaN makes the minimum of its own key unspecified and
        touches no other key."""
        return self._group_minmax("Index.group_min", ALGO_AGG_MIN, probe_keys, probe_values, out, return_counts, counts_out, signed, float64)

    def group_max(self, probe_keys, probe_values, out=None, return_counts: bool = False, counts_out=None, signed=None, float64: bool = False):
        """Latest event per user over a batch: the max form of group_min.  Identity: 0 (unsigned) or -2^63 (signed); float64=True: -inf."""
        return self._group_minmax("Index.group_max", ALGO_AGG_MAX, probe_keys, probe_values, out, return_counts, counts_out, signed, float64)



def build_index(build_keys, build_values=None, device: Optional[int] = None) -> Index:
    """Prepare a build side once for many probes: returns an Index whose lookup / isin / lookup_indices answer as the module functions
    do for these build_keys (and build_values; None: a keys-only index, lookup then raises).  The keys, the values and every key's
    first-occurrence position are copied into device memory the index owns (16 bytes per build row, 24 with values): the caller's
    arrays may be overwritten or freed as soon as this returns.  Torch ROCm tensors / DLPack are read in place, on their device and the
    current stream, and the outputs of later probes with device tensors live on the device.  NumPy arrays are staged through
    fj_device_malloc / fj_memcpy_*, here and in every probe with NumPy keys: synchronous and unpipelined copies - a host-side caller
    who wants the copy hidden under the join uses the one-shot functions - and their outputs are NumPy.  `device`: where a NumPy-built
    index lives (default 0); for device tensors it must be their device.  An index built from NumPy arrays may be probed with device
    tensors of its device and the reverse.  The plan is chosen now, from the build side's size and the options in force."""
    global _last
    L = _lib.load()
    bk, bv = (_from_dlpack_if_device(x) if x is not None else None for x in (build_keys, build_values))
    cnt, t = ctypes.c_uint64(0), FjTimings()
    algo = ALGO_ADAPTIVE | ALGO_PROBE_ORDER | ALGO_RETAIN_BUILD
    on_device = _is_torch_tensor(bk) and bk.is_cuda
    if on_device:
        import torch
        bk = _dev_tensor(bk, "build_keys")
        bv = _dev_tensor(bv, "build_values") if bv is not None else None
        n_b, n_v = bk.numel(), (bv.numel() if bv is not None else 0)
        dev = _device_index(bk)
        if bv is not None and (not bv.is_cuda or bv.device != bk.device):
            raise ValueError("build_values must live on the device of build_keys")
    else:
        if _is_torch_tensor(bk):
            bk = bk.numpy()
        if _is_torch_tensor(bv):
            bv = bv.cpu().numpy()
        bk = _as_u64_host(bk, "build_keys")
        bv = _as_u64_host(bv, "build_values") if bv is not None else None
        n_b, n_v = bk.size, (bv.size if bv is not None else 0)
        dev = 0 if device is None else int(device)
    if bv is not None and n_v < n_b:
        raise ValueError(f"build_values has {n_v} elements, build_keys has {n_b}")
    if device is not None and int(device) != dev:
        raise ValueError(f"device={device}, but build_keys live on device {dev}")
    ctx = L.fj_ctx_create(dev)
    if not ctx:
        raise RuntimeError(_lib.last_error())
    try:
        if on_device:
            stream = torch.cuda.current_stream(dev).cuda_stream
            check(L.fj_join_device(ctx, algo, 0, 1, bk.data_ptr(), bv.data_ptr() if bv is not None else None, n_b, None, 0, stream, 64,
                                   ctypes.byref(cnt), None, None, 0, ctypes.byref(t)))
        else:
            with _device_scope(dev), _Staged() as st:
                d_bk = st.upload(bk)
                d_bv = st.upload(bv[:n_b]) if bv is not None else None
                check(L.fj_join_device(ctx, algo, 0, 1, d_bk, d_bv, n_b, None, 0, None, 64, ctypes.byref(cnt), None, None, 0, ctypes.byref(t)))
        check(L.fj_ctx_trim(ctx))       # the build side's passes are over: their workspace goes back, the prepared side is no workspace
    except BaseException:
        L.fj_ctx_destroy(ctx)
        raise
    _last = t
    return Index(ctx, dev, n_b, int(cnt.value), bv is not None)


# ---- extension: build-order aggregate joins (one word per build row, at the build row's position; csrc/fj_group.hip) -----------------
def _group_host(algo: int, bk, pk, pv, want_counts: bool):
    bk, pk = _as_u64_host(bk, "build_keys"), _as_u64_host(pk, "probe_keys")
    pv = _as_u64_host(pv, "probe_values") if pv is not None else None
    if pv is not None and pv.size != pk.size:
        raise ValueError(f"probe_values has {pv.size} elements, probe_keys has {pk.size}")
    n, want_sums = bk.size, pv is not None  # the probe side's value column goes where a join takes its build values
    read = lambda c, oc, osum: (_take_host(oc, n).view(np.int64) if want_counts else None, _take_host(osum, n).view(np.int64) if want_sums else None)
    c, sec, (counts, sums) = _host_call(algo, 0, 1, bk, pv, n, pk, pk.size, want_counts, want_sums, read)
    return c[0], sec, counts, sums


def _group(build_keys, probe_keys, probe_values, want_counts: bool, agg: int = 0):
    """(P, seconds, counts or None, sums or None): int64 of len(build_keys), where the inputs live.  agg: ALGO_AGG_* flags - the
    second array then holds the minima / maxima"""
    build_keys, probe_keys, probe_values = (_from_dlpack_if_device(x) if x is not None else None for x in (build_keys, probe_keys, probe_values))
    algo = ALGO_ADAPTIVE | ALGO_BUILD_ORDER | agg
    if _is_torch_tensor(build_keys) and build_keys.is_cuda:
        return join_device(algo, 0, 1, build_keys, probe_values, probe_keys, want_counts=want_counts)
    if _is_torch_tensor(build_keys):
        build_keys, probe_keys, probe_values = (x.numpy() if x is not None else None for x in (build_keys, probe_keys, probe_values))
    return _group_host(algo, build_keys, probe_keys, probe_values, want_counts)


def group_join_count(build_keys, probe_keys):
    """The join that feeds a GROUP BY on the build side, count form: (P, seconds, counts), counts[i] = the probe rows whose key equals
    build_keys[i], int64 of len(build_keys), aligned with the build rows; every copy of a duplicated build key carries the key's count.
    P = counts.sum(), the pairs of the many-to-many inner join.  No pairs are made and the probe side moves its keys only.
    NumPy arrays in, NumPy arrays out; torch ROCm tensors / DLPack are joined in place and the outputs live on their device."""
    P, sec, counts, _ = _group(build_keys, probe_keys, None, True)
    return P, sec, counts


def group_join_sum(build_keys, probe_keys, probe_values, return_counts: bool = False, float64: bool = False):
    """Sum form: (P, seconds, sums) or, return_counts=True, (P, seconds, sums, counts).  sums[i] = the sum modulo 2^64 of
    probe_values[j] over the probe rows j whose key equals build_keys[i] (int64 storage of the uint64 words), 0 where there are none;
    probe_values has one word per probe row.  The mean is sums / counts.
    float64=True: probe_values is a floating-point column - NumPy float64 and torch.float64 / DLPack are read in place, float32 /
    float16 are widened exactly, integers raise TypeError - and sums is float64 (a NumPy array, or a torch.float64 tensor on the
    inputs' device), 0.0 where there is no partner; counts stay int64.  The sum is accumulated with atomic adds in an
    UNSPECIFIED ORDER: it can differ in its last bits from run to run and from a sequential sum.  A NaN makes the sum of its own
    key NaN and touches no other key.  Without the keyword a NumPy float column is value-cast to uint64 words, as ever."""
    if probe_values is None:
        raise ValueError("group_join_sum: probe_values is required (group_join_count takes none)")
    if float64:
        pv = _float_words("group_join_sum", "probe_values", probe_values)
        P, sec, counts, sums = _group(build_keys, probe_keys, pv, bool(return_counts), ALGO_AGG_FLOAT)
        return (P, sec, _as_float64(sums), counts) if return_counts else (P, sec, _as_float64(sums))
    P, sec, counts, sums = _group(build_keys, probe_keys, probe_values, bool(return_counts))
    return (P, sec, sums, counts) if return_counts else (P, sec, sums)


def _group_minmax(name: str, flag: int, build_keys, probe_keys, probe_values, return_counts: bool, signed, float64: bool = False):
    if probe_values is None:
        raise ValueError(f"{name}: probe_values is required (group_join_count takes none)")
    pv, signed, unsigned_in = _word_column(name, "probe_values", probe_values, signed, float64, integers_only=False)
    P, sec, counts, vals = _group(build_keys, probe_keys, pv, bool(return_counts), flag | _agg_flags(signed, float64))
    vals = _agg_values(vals, signed, unsigned_in, float64)
    return (P, sec, vals, counts) if return_counts else (P, sec, vals)


def group_join_min(build_keys, probe_keys, probe_values, return_counts: bool = False, signed=None, float64: bool = False):
    """Min form: (P, seconds, values) or, return_counts=True, (P, seconds, values, counts).  values[i] = the minimum of probe_values[j]
    over the probe rows j whose key equals build_keys[i] ("cheapest offer per product"); every copy of a duplicated build key carries
    the key's minimum; P = the sum of all counts.  signed=None takes the sign from the container: a NumPy uint64 value column
    compares unsigned, everything else (NumPy int64, torch int64, DLPack) signed; True / False force it.
    A build row WITHOUT a partner holds the aggregate's identity: 2^64 - 1 (unsigned) or 2^63 - 1 (signed).  A key whose true minimum
    equals the identity looks the same: return_counts=True is how to tell them apart (counts[i] == 0: no partner).
    NumPy in, NumPy out: values has the dtype of probe_values when that is uint64 / int64 and `signed` agrees with it, otherwise it is
    the int64 storage of the words; counts is int64.  Torch ROCm tensors / DLPack are joined in place, the outputs are torch.int64 on
    their device.  The probe side moves keys and values once; no pairs are made (csrc/fj_group.hip).
    float64=True: probe_values is a floating-point column (as for group_join_sum), `signed` must stay None (TypeError otherwise) and
    values is float64, compared as numbers; a build row without a partner holds +inf (group_join_max: -inf) and count 0.  Which zero
    comes back for a key that holds both -0.0 and +0.0 is unspecified; a NaN makes the minimum / maximum of its own key unspecified
    and touches no other key."""
    return _group_minmax("group_join_min", ALGO_AGG_MIN, build_keys, probe_keys, probe_values, return_counts, signed, float64)


def group_join_max(build_keys, probe_keys, probe_values, return_counts: bool = False, signed=None, float64: bool = False):
    """Max form of group_join_min ("latest order date per customer"): values[i] = the maximum of probe_values[j] over the probe rows j
    whose key equals build_keys[i].  A build row WITHOUT a partner holds the aggregate's identity: 0 (unsigned) or -2^63 (signed); a
    key whose true maximum equals it looks the same, so ask for return_counts=True to tell them apart (counts[i] == 0: no partner).
    Arguments, `signed`, `float64` (identity -inf), containers and dtypes as for group_join_min."""
    return _group_minmax("group_join_max", ALGO_AGG_MAX, build_keys, probe_keys, probe_values, return_counts, signed, float64)


# ---- extension: group-by on one relation (the distinct keys and one aggregate per key; csrc/fj_groupby.hip) ----------------------------
def _group_columns(keys, values=None):
    """(k, v, n): the key column and the value column (None: none) of a group-by on one relation as word columns of n rows where the
    keys live - torch.int64 on the keys' device, or NumPy uint64"""
    keys, values = (_from_dlpack_if_device(x) if x is not None else None for x in (keys, values))
    if _is_torch_tensor(keys) and keys.is_cuda:
        k = _dev_tensor(keys, "keys")
        v = _dev_tensor(values, "values") if values is not None else None
    else:
        keys, values = (x.numpy() if _is_torch_tensor(x) else x for x in (keys, values))
        k = _as_u64_host(keys, "keys")
        v = _as_u64_host(values, "values") if values is not None else None
    if v is not None and v.shape[0] != k.shape[0]:
        raise ValueError(f"values has {v.shape[0]} elements, keys has {k.shape[0]}")
    return k, v, k.shape[0]


def _group_by_call(algo: int, a, b, c, n: int, vals, want_keys: bool = True, max_groups: Optional[int] = None, overflow: Optional[str] = None):
    """ONE FJ_ALGO_GROUP_BY call where the inputs live: (g, seconds, group_keys or None, values or None).  a, b, c: up to three word
    columns of n rows (None: none), all contiguous torch.int64 on one device - read in place on that device's current stream, under
    its context and the context's lock - or all NumPy uint64; c travels as the probe side.  The outputs are torch.int64 tensors on
    that device, or NumPy uint64 keys and int64 words.  vals is the layout of the values output:
      None      none is wanted
      "groups"  one word per group: g words
      "rows"    one word per input row (ALGO_INVERSE): n words, never trimmed to g
      "csr"     ALGO_GROUP_ROWS: the n row indices and then the g starts, n + g words (the device buffer holds two planes of n)
      an int P  P planes: (P, g)
    want_keys=False: nothing is materialised.  The device buffers hold n rows; those of the plane forms max(1, min(n, max_groups)) rows
    (max_groups None: n).  overflow: the text, around {g}, of the ValueError for a result beyond max_groups."""
    global _last
    planes = vals if isinstance(vals, int) else 0
    if not _is_torch_tensor(a):
        def read(count, ok, ov):
            g = count[0]
            gk = _take_host(ok, g) if want_keys else None
            if vals is None:
                return gk, None
            words = _take_host(ov, planes * g if planes else n if vals == "rows" else n + g if vals == "csr" else g).view(np.int64)
            return gk, (words.reshape(planes, g) if planes else words)
        count, sec, (gk, gv) = _host_call(algo, 0, int(want_keys), a, b, n, c, n if c is not None else 0, want_keys, vals is not None, read)
        if overflow and max_groups is not None and count[0] > max_groups:      # (host arrays are sized by the library: the bound is checked all the same)
            raise ValueError(overflow.format(g=count[0]))
        return count[0], sec, gk, gv
    import torch
    L = _lib.load()
    dev = _device_index(a)
    ctx = context(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    cap = max(1, n if max_groups is None else min(n, max_groups)) if planes else (n if want_keys else 0)
    empty = lambda *shape: torch.empty(shape, dtype=torch.int64, device=a.device)
    ok = empty(cap) if want_keys else None
    ov = None if vals is None else empty(planes, cap) if planes else empty(2 * n if vals == "csr" else cap)
    src = lambda x: x.data_ptr() if x is not None and n else None             # (no rows: null input pointers)
    dst = lambda x: x.data_ptr() if x is not None else None
    cnt, t = ctypes.c_uint64(0), FjTimings()
    with _ctx_locks.setdefault(dev, threading.RLock()):
        rc = L.fj_join_device(ctx, algo, 0, int(want_keys), src(a), src(b), n, src(c), n if c is not None else 0, stream, 64,
                              ctypes.byref(cnt), dst(ok), dst(ov), cap, ctypes.byref(t))
        g = int(cnt.value)
        if rc and overflow and g > cap:                      # (the device work is done and the context usable: the buffers were too small)
            raise ValueError(overflow.format(g=g))
        check(rc)
    _last = t
    return g, t.total_ms * 1e-3, _trim(ok, g), (ov if vals in ("rows", "csr") else _trim(ov, g))


def _group_by(keys, values, flags: int, materialize: bool = True, want_vals: bool = True):
    """(g, seconds, group_keys or None, aggregates or None), where the inputs live: NumPy uint64 keys and int64 words (the storage of
    the uint64 aggregates), or torch.int64 tensors on the inputs' device.  values=None: the count form (or ALGO_ROW_IDS in flags).
    ALGO_INVERSE in flags: the fourth item is the group id of every row instead - len(keys) int64 in [0, g), never trimmed to g."""
    inverse = bool(flags & ALGO_INVERSE)
    if inverse and not (materialize and want_vals):
        raise ValueError("ALGO_INVERSE: the group ids are the values output (materialize and want_vals)")
    k, v, n = _group_columns(keys, values)
    vals = ("rows" if inverse else "groups") if materialize and want_vals else None
    return _group_by_call(ALGO_ADAPTIVE | ALGO_GROUP_BY | flags, k, v, None, n, vals, want_keys=materialize)


def _align_by_key(keys_a, keys_b, vals_b):
    """vals_b, given in the order of keys_b, in the order of keys_a (the same set of distinct keys)"""
    if _is_torch_tensor(keys_a):
        import torch
        out = torch.empty_like(vals_b)
        out[torch.argsort(keys_a)] = vals_b[torch.argsort(keys_b)]
        return out
    out = np.empty_like(vals_b)
    out[np.argsort(keys_a, kind="stable")] = vals_b[np.argsort(keys_b, kind="stable")]
    return out


def _bincount(ids, g: int):
    """rows per id in [0, g), int64, where the ids live"""
    if _is_torch_tensor(ids):
        import torch
        return torch.bincount(ids, minlength=g)
    return np.bincount(ids, minlength=g).astype(np.int64, copy=False)


def _ids_by_key(keys_a, keys_b, ids_b):
    """ids_b, indices into keys_b, as indices into keys_a (the same set of distinct keys in another order)"""
    if _is_torch_tensor(keys_a):
        import torch
        perm = torch.empty_like(keys_a)
        perm[torch.argsort(keys_b)] = torch.argsort(keys_a)
        return perm[ids_b]
    perm = np.empty(keys_a.shape[0], np.int64)
    perm[np.argsort(keys_b, kind="stable")] = np.argsort(keys_a, kind="stable")
    return perm[ids_b]


def factorize(keys):
    """The dense group id of every row (pandas.factorize; the dictionary encoding of a key column): (g, seconds, codes, uniques) -
    uniques the g distinct keys in unspecified order (neither sorted nor by first occurrence), codes one int64 in [0, g) per row of
    keys with uniques[codes] == keys.  One library call: the relation is grouped once, and every further aggregate is an
    index_add_ / scatter_reduce_ / np.bincount of the caller's over codes.  NumPy in: uniques is uint64, codes int64; torch ROCm
    tensors / DLPack are grouped in place, both outputs are torch.int64 on their device."""
    g, sec, uniques, codes = _group_by(keys, None, ALGO_INVERSE)
    return g, sec, codes, uniques


def _group_rows(keys):
    """(g, seconds, group_keys, offsets, row_index) of ALGO_GROUP_BY | ALGO_GROUP_ROWS, where the keys live: the two planes of the
    values output come back as row_index (the first len(keys) words of plane 0) and offsets (the g starts of plane 1 and len(keys))"""
    k, _, n = _group_columns(keys)
    g, sec, gk, words = _group_by_call(ALGO_ADAPTIVE | ALGO_GROUP_BY | ALGO_GROUP_ROWS, k, None, None, n, "csr")
    on_device = _is_torch_tensor(words)
    offsets = words.new_empty(g + 1) if on_device else np.empty(g + 1, np.int64)
    offsets[:g] = words[n:n + g]
    offsets[g] = n
    return g, sec, gk, offsets, (words[:n] if on_device else words[:n].copy())       # (NumPy: a copy, not a view of the n + g words)


def group_rows(keys):
    """The ROWS of every group (pandas groupby().indices, cuDF groupby.groups, SQL array_agg over the row number, the CSR of an edge
    list by source): (g, seconds, group_keys, offsets, row_index).  group_keys holds the g distinct keys in unspecified order; offsets
    is int64 of g + 1 with offsets[0] == 0 and offsets[g] == len(keys); row_index is int64 of len(keys), a permutation of the row
    numbers, and keys[row_index[offsets[i]:offsets[i + 1]]] are all group_keys[i].  offsets is what torch.segment_reduce(...,
    offsets=) and np.add.reduceat(values[row_index], offsets[:-1]) take as it is: a median, a quantile, a top-k, a list per group -
    every aggregate the library has no kernel for - is one gather and one segmented pass of the caller's.  The order of the rows
    INSIDE a group is unspecified and may differ from run to run.  One library call and no sort (C ABI: algo | FJ_ALGO_GROUP_BY |
    FJ_ALGO_GROUP_ROWS).  Keys are converted as `factorize` converts them: NumPy in, group_keys is uint64 and the rest int64 NumPy;
    torch ROCm tensors / DLPack are grouped in place on the current stream, every output is torch.int64 on their device."""
    return _group_rows(keys)


def group_by_collect(keys, values):
    """The values of every group, gathered (SQL array_agg, pandas groupby().agg(list) as one flat array with offsets):
    (g, seconds, group_keys, offsets, values[row_index]) with group_keys, offsets and row_index as `group_rows(keys)` returns them.
    values has one row per key along its first dimension and keeps its dtype and any trailing dimensions; the rows of group i are
    collected[offsets[i]:offsets[i + 1]], in unspecified order.  The gather is ONE indexing operation where the inputs live: NumPy
    (or CPU torch) values with NumPy keys, a torch tensor on the keys' device with device keys."""
    keys, values = _from_dlpack_if_device(keys), _from_dlpack_if_device(values)
    dev_keys = _is_torch_tensor(keys) and keys.is_cuda
    if dev_keys:
        if not (_is_torch_tensor(values) and values.device == keys.device):
            raise TypeError("group_by_collect: keys is a device tensor, values must be a torch tensor on the same device")
        n = keys.numel()
    else:
        if _is_torch_tensor(values) and values.is_cuda:
            raise TypeError("group_by_collect: values is a device tensor, keys must be a torch tensor on the same device")
        if not _is_torch_tensor(values):
            values = np.asarray(values)
        n = keys.numel() if _is_torch_tensor(keys) else np.asarray(keys).size
    if values.ndim < 1 or values.shape[0] != n:
        raise ValueError(f"group_by_collect: values has {values.shape[0] if values.ndim else 'no'} rows along its first dimension, keys has {n}")
    g, sec, gk, offsets, rows = _group_rows(keys)
    if _is_torch_tensor(values) and not _is_torch_tensor(rows):
        import torch
        rows = torch.from_numpy(rows)
    return g, sec, gk, offsets, values[rows]


def _key_columns(name: str, what: str, columns: Any):
    """(columns, torch_in): a key of one or more columns as a list of word columns - a single array is one column, a list / tuple of
    arrays (or of nested sequences) is one column each.  Every column is converted as `factorize` converts its keys; all are of one
    kind - NumPy-like (torch_in False), or torch tensors on one device - and of one length."""
    if isinstance(columns, (list, tuple)) and len(columns) and all(_is_array(c) or isinstance(c, (list, tuple)) for c in columns):
        cols = [_from_dlpack_if_device(c) for c in columns]
    elif isinstance(columns, (list, tuple)) and not len(columns):
        cols = []
    else:
        cols = [_from_dlpack_if_device(columns)]
    if not cols:
        return cols, False
    torch_in = [_is_torch_tensor(c) for c in cols]
    if any(torch_in) and not all(torch_in):
        raise TypeError(f"{name}: {what} must be of one kind, got NumPy and torch columns side by side")
    if all(torch_in):
        _same_container(name, cols)
        if cols[0].is_cuda:
            cols = [_dev_tensor(c, f"{what}[{i}]") for i, c in enumerate(cols)]
        else:
            cols = [_as_u64_host(c.numpy(), f"{what}[{i}]") for i, c in enumerate(cols)]
    else:
        cols = [_as_u64_host(c, f"{what}[{i}]") for i, c in enumerate(cols)]
    for i, c in enumerate(cols[1:], 1):
        if c.shape[0] != cols[0].shape[0]:
            raise ValueError(f"{name}: {what}[{i}] has {c.shape[0]} rows, {what}[0] has {cols[0].shape[0]}")
    return cols, all(torch_in)


def _first_rows(idx):
    """the row indices the pair form returns where the keys go, as int64 in their container"""
    return idx if _is_torch_tensor(idx) else idx.view(np.int64)


def factorize_columns(columns):
    """The dense group id of every row under a MULTI-COLUMN key - (customer, day), (src, dst), (tenant, user):
    (g, seconds, codes, first_index).  columns is a sequence of two or more key columns of equal length and one kind, each converted
    as `factorize` converts its keys.  codes holds one int64 in [0, g) per row, and two rows share a code iff they agree in EVERY
    column; first_index holds, per group, the int64 row index of its first occurrence, so the distinct tuples are
    tuple(c[first_index] for c in columns) and c[first_index][codes] == c for every column.  The order of the groups is unspecified.
    Two columns are ONE library call (C ABI: algo | FJ_ALGO_GROUP_BY | FJ_ALGO_INVERSE | FJ_ALGO_KEY_PAIR), exact for every input; a
    third and fourth column fold on left to right - (codes so far, next column) through the same call - and `seconds` is the sum.  The
    codes are ordinary dense keys: group_by_agg(codes, v), inner_join(build_codes, bv, probe_codes) and build_index(codes) take them
    unchanged.  NumPy in, NumPy out; torch ROCm tensors / DLPack are grouped in place on the current stream, both outputs torch.int64
    on their device.  A single column is `factorize`'s: here it is a ValueError."""
    if _is_array(columns):
        raise ValueError("factorize_columns: got a single array; columns is a sequence of two or more key columns (one column: factorize)")
    cols, _ = _key_columns("factorize_columns", "columns", columns)
    if len(cols) < 2:
        raise ValueError(f"factorize_columns: got {len(cols)} column{'s' if len(cols) != 1 else ''}; columns is a sequence of two or more key columns (one column: factorize)")
    g, sec, first, codes = _group_by(cols[0], cols[1], ALGO_INVERSE | ALGO_KEY_PAIR)
    for c in cols[2:]:
        g, sec2, first, codes = _group_by(codes, c, ALGO_INVERSE | ALGO_KEY_PAIR)    # (the first rows of (codes, c) are rows of the relation already)
        sec += sec2
    return g, sec, codes, _first_rows(first)


def encode_keys(build_columns, probe_columns):
    """ONE shared dictionary over the keys of two relations: (g, seconds, build_codes, probe_codes).  Each argument is a sequence of
    key columns as for `factorize_columns` - or a single array, a one-column key - and both name the same number of columns.  The
    columns are concatenated, build rows first, factorized in one `factorize_columns` call (`factorize` for one column) and the
    codes split again: equal tuples get equal int64 codes in [0, g) across the two relations, so every join, `build_index` and every
    `group_join_*` takes the codes as its keys.  NumPy in, NumPy out; torch ROCm tensors stay on their device and stream."""
    b, b_torch = _key_columns("encode_keys", "build_columns", build_columns)
    p, p_torch = _key_columns("encode_keys", "probe_columns", probe_columns)
    if len(b) != len(p) or not b:
        raise ValueError(f"encode_keys: build_columns names {len(b)} key columns, probe_columns {len(p)}; both sides need the same number, at least one")
    if b_torch != p_torch:
        raise TypeError("encode_keys: build_columns and probe_columns must be of one kind, got NumPy and torch columns side by side")
    if _is_torch_tensor(b[0]):
        import torch
        _same_container("encode_keys", b + p)
        cat = [torch.cat((x.view(torch.int64), y.view(torch.int64))) for x, y in zip(b, p)]
    else:
        cat = [np.concatenate((x, y)) for x, y in zip(b, p)]
    nb = b[0].shape[0]
    if len(cat) == 1:
        g, sec, codes, _ = factorize(cat[0])
    else:
        g, sec, codes, _ = factorize_columns(cat)
    return g, sec, codes[:nb], codes[nb:]


def unique(keys, return_index: bool = False, return_counts: bool = False, return_inverse: bool = False):
    """The distinct keys of one relation (DISTINCT; torch.unique / np.unique without the sort): (g, seconds, unique_keys) followed by
    first_index if return_index (the 0-based position of every key's FIRST occurrence, int64), by inverse if return_inverse (int64,
    one per row of keys: unique_keys[inverse] == keys) and by counts if return_counts (int64) - NumPy's order.
    The order of the keys is unspecified; the extras are aligned with unique_keys.  Any one extra is one call; so is return_inverse
    with return_counts (the counts are the bincount of the inverse, where the data lives).  return_index with either of the others
    makes two calls (one per-call output) and aligns the second by key with two argsorts of g keys - `seconds` is the sum of both.
    NumPy in: unique_keys is uint64; torch ROCm tensors / DLPack are grouped in place, every output is torch.int64 on their device."""
    if return_inverse:
        if not return_index:
            g, sec, gk, inv = _group_by(keys, None, ALGO_INVERSE)
            return (g, sec, gk, inv, _bincount(inv, g)) if return_counts else (g, sec, gk, inv)
        g, sec, gk, idx = _group_by(keys, None, ALGO_ROW_IDS)
        g2, sec2, gk2, inv2 = _group_by(keys, None, ALGO_INVERSE)
        inv = _ids_by_key(gk, gk2, inv2)
        return (g, sec + sec2, gk, idx, inv, _bincount(inv, g)) if return_counts else (g, sec + sec2, gk, idx, inv)
    if return_index:
        g, sec, gk, idx = _group_by(keys, None, ALGO_ROW_IDS)
        if not return_counts:
            return g, sec, gk, idx
        g2, sec2, gk2, counts = _group_by(keys, None, 0)
        return g, sec + sec2, gk, idx, _align_by_key(gk, gk2, counts)
    if return_counts:
        return _group_by(keys, None, 0)
    return _group_by(keys, None, 0, want_vals=False)[:3]


def distinct_count(keys):
    """COUNT(DISTINCT keys): (g, seconds).  A keys-only pass; nothing is written."""
    return _group_by(keys, None, 0, materialize=False)[:2]


def group_by_count(keys):
    """GROUP BY keys, COUNT(*): (g, seconds, group_keys, counts) - the g distinct keys in unspecified order and the number of rows of
    each, int64, aligned with group_keys.  The list of groups the group_join_* functions ask for, made inside the library."""
    return _group_by(keys, None, 0)


def group_by_sum(keys, values, float64: bool = False):
    """GROUP BY keys, SUM(values): (g, seconds, group_keys, sums), sums[i] = the sum modulo 2^64 of values[j] over the rows j whose
    key is group_keys[i] (int64 storage of the uint64 words).  values has one word per row.
    float64=True: values is a floating-point column - NumPy float64 and torch.float64 / DLPack are read in place, float32 / float16
    are widened exactly, integers raise TypeError - and sums is float64 (a NumPy array, or a torch.float64 tensor on the inputs'
    device).  The sum is accumulated with atomic adds in an UNSPECIFIED ORDER: it can differ in its last bits from run to run and
    from a sequential sum.  A NaN makes the sum of its own group NaN and touches no other group.  Without the keyword a NumPy float
    column is value-cast to uint64 words, as ever, and a torch float tensor is refused."""
    if values is None:
        raise ValueError("group_by_sum: values is required (group_by_count takes none)")
    if float64:
        g, sec, gk, sums = _group_by(keys, _float_words("group_by_sum", "values", values), ALGO_AGG_FLOAT)
        return g, sec, gk, _as_float64(sums)
    return _group_by(keys, values, 0)


def _group_by_minmax(name: str, flag: int, keys, values, signed, float64: bool = False):
    if values is None:
        raise ValueError(f"{name}: values is required")
    values, signed, unsigned_in = _word_column(name, "values", values, signed, float64)
    g, sec, gk, vals = _group_by(keys, values, flag | _agg_flags(signed, float64))
    return g, sec, gk, _agg_values(vals, signed, unsigned_in, float64)


def group_by_min(keys, values, signed=None, float64: bool = False):
    """GROUP BY keys, MIN(values): (g, seconds, group_keys, values).  signed=None takes the sign from the container, as group_join_min
    does: a NumPy uint64 column compares unsigned, everything else signed; True / False force it.  Every group has a row, so no
    identity appears.  NumPy in: the minima have the dtype of `values` when that is uint64 / int64 and `signed` agrees, else int64.
    float64=True: values is a floating-point column (as for group_by_sum), `signed` must stay None (TypeError otherwise) and the
    minima are float64, compared as numbers.  Which zero comes back for a group that holds both -0.0 and +0.0 is unspecified; a NaN
    makes the minimum of its own group unspecified and touches no other group."""
    return _group_by_minmax("group_by_min", ALGO_AGG_MIN, keys, values, signed, float64)


def group_by_max(keys, values, signed=None, float64: bool = False):
    """GROUP BY keys, MAX(values): the max form of group_by_min (`float64` included)."""
    return _group_by_minmax("group_by_max", ALGO_AGG_MAX, keys, values, signed, float64)


# ---- extension: group-by with count, sum, min and max of a column in one call (csrc/fj_groupby_multi.hip) -------------------------------
def _group_by_all(keys, values, flags: int, max_groups: Optional[int] = None):
    """(g, seconds, group_keys, planes): ONE library call, FJ_ALGO_GROUP_BY | FJ_ALGO_AGG_ALL | flags.  planes is a (4, g) array of
    int64 words where the inputs live - row counts, sums, minima, maxima - each row aligned with group_keys.  flags: a base value
    (ALGO_SCALAR, ALGO_RADIX), ALGO_AGG_SIGNED or ALGO_AGG_FLOAT.  max_groups: the rows the device buffers hold (None: len(keys));
    a result beyond it is a ValueError that names g."""
    k, v, n = _group_columns(keys, values)
    return _group_by_call(ALGO_ADAPTIVE | ALGO_GROUP_BY | ALGO_AGG_ALL | flags, k, v, None, n, 4, max_groups=max_groups,
                          overflow=f"group_by_agg: the relation has g = {{g}} distinct keys, max_groups = {max_groups}")


_AGG_NAMES = ("count", "sum", "min", "max", "mean")


def _check_aggs(name: str, aggs, float64: bool) -> tuple:
    """the `aggs` argument of group_by_agg and GroupByAccumulator.result as a tuple of names, or the ValueError that says what is wrong"""
    if isinstance(aggs, str) or not hasattr(aggs, "__iter__"):
        raise ValueError(f"{name}: aggs must be a sequence of names from {_AGG_NAMES}, got {aggs!r}")
    aggs = tuple(aggs)
    if not aggs:
        raise ValueError(f"{name}: aggs is empty (name at least one of {_AGG_NAMES})")
    for a in aggs:
        if a not in _AGG_NAMES:
            raise ValueError(f"{name}: unknown aggregate {a!r} (aggs takes {_AGG_NAMES})")
    if len(set(aggs)) != len(aggs):
        raise ValueError(f"{name}: aggs repeats a name: {aggs!r}")
    if "mean" in aggs and not float64:
        raise ValueError(f"{name}: 'mean' needs float64=True (the integer sum wraps modulo 2^64: an integer mean would be silently wrong)")
    return aggs


def _check_max_groups(name: str, max_groups) -> Optional[int]:
    if max_groups is None:
        return None
    if isinstance(max_groups, (bool, np.bool_)) or not isinstance(max_groups, (int, np.integer)) or max_groups < 1:
        raise ValueError(f"{name}: max_groups must be None or an integer >= 1, got {max_groups!r}")
    return int(max_groups)


def _agg_columns(planes, aggs: tuple, float64: bool, unsigned_out: bool) -> list:
    """the columns `aggs` names, from the (4, g) planes of words - counts, sums, minima, maxima - with group_by_agg's dtypes"""
    cols = []
    for a in aggs:
        if a == "count":
            col = planes[0]
        elif a == "mean":
            cnt = planes[0].double() if _is_torch_tensor(planes) else planes[0].astype(np.float64)
            col = _as_float64(planes[1]) / cnt
        else:
            col = planes[_AGG_NAMES.index(a)]
            if float64:
                col = _as_float64(col)
            elif a != "sum" and unsigned_out and isinstance(col, np.ndarray):
                col = col.view(np.uint64)                    # the column's own dtype; otherwise int64 storage of the words
        cols.append(col)
    return cols


def group_by_agg(keys, values, aggs=("count", "sum", "min", "max"), signed=None, float64: bool = False, max_groups: Optional[int] = None):
    """GROUP BY keys with several aggregates of ONE value column - SELECT k, COUNT(*), SUM(v), MIN(v), MAX(v), AVG(v) ... GROUP BY k:
    (g, seconds, group_keys, *columns), one column per entry of `aggs`, in that order, every one aligned with group_keys (whose order
    is unspecified).  ONE library call whatever `aggs` names: the relation goes through the partition passes once, where
    group_by_count + group_by_sum + group_by_min + group_by_max take four trips and three alignments by key.
    aggs: a non-empty sequence without repeats of "count", "sum", "min", "max", "mean".  "mean" is sum / count as float64, computed
    where the data lives, and needs float64=True: the integer sum wraps modulo 2^64, so an integer mean would be silently wrong.
    signed and float64 follow group_by_min and group_by_sum exactly: signed=None takes the sign from the container (a NumPy uint64
    column compares unsigned, everything else signed), True / False force it; float64=True reads a floating-point column as numbers
    (`signed` must stay None, integers raise TypeError).  Dtypes are those of the single forms: counts int64; the sum int64 storage of
    the words, or float64; min and max the column's own dtype for a NumPy uint64 column compared unsigned, else int64, or float64.
    max_groups: a caller who knows a bound on the number of groups gets device buffers of min(len(keys), max_groups) rows instead of
    len(keys) - five arrays of len(keys) words are 40 bytes per input row; a result beyond the bound raises ValueError naming g, and
    the context stays usable.  NumPy in, NumPy out; torch ROCm tensors / DLPack are read in place on the current stream and every
    output is a tensor on their device."""
    aggs = _check_aggs("group_by_agg", aggs, float64)
    max_groups = _check_max_groups("group_by_agg", max_groups)
    if values is None:
        raise ValueError("group_by_agg: values is required (group_by_count takes none)")
    values, signed, unsigned_in = _word_column("group_by_agg", "values", values, signed, float64)
    g, sec, gk, planes = _group_by_all(keys, values, _agg_flags(signed, float64), max_groups)
    return (g, sec, gk, *_agg_columns(planes, aggs, float64, unsigned_in and not signed))


# ---- extension: GROUP BY a, b with four aggregates in one call (csrc/fj_groupby_pair_agg.hip) ---------------------------------------------
def _group_by_pair_all(a, b, values, flags: int, max_groups: Optional[int] = None):
    """(g, seconds, group_a, planes): ONE library call, FJ_ALGO_GROUP_BY | FJ_ALGO_KEY_PAIR | FJ_ALGO_AGG_ALL | flags, over word columns
    as `_key_columns` returns them.  planes is a (5, g) array of int64 words where the inputs live - column B of every group, then row
    counts, sums, minima, maxima - each row aligned with group_a.  flags and max_groups as for `_group_by_all`."""
    n = a.shape[0]
    if _is_torch_tensor(a):
        v = _dev_tensor(_from_dlpack_if_device(values), "values")
    else:
        v = _as_u64_host(values.numpy() if _is_torch_tensor(values) else values, "values")
    if v.shape[0] != n:
        raise ValueError(f"values has {v.shape[0]} elements, the key columns have {n}")
    if _is_torch_tensor(a) and v.device != a.device:
        raise ValueError(f"group_by_agg_columns: values lives on {v.device}, the key columns on {a.device}")
    # (the value column and its rows go where a join takes its probe side)
    return _group_by_call(ALGO_ADAPTIVE | ALGO_GROUP_BY | ALGO_KEY_PAIR | ALGO_AGG_ALL | flags, a, b, v, n, 5, max_groups=max_groups,
                          overflow=f"group_by_agg_columns: the relation has g = {{g}} distinct key tuples, max_groups = {max_groups}")


def group_by_agg_columns(columns, values, aggs=("count", "sum", "min", "max"), signed=None, float64: bool = False, max_groups: Optional[int] = None):
    """GROUP BY a MULTI-COLUMN key with several aggregates of one value column - SELECT a, b, COUNT(*), SUM(v), MIN(v), MAX(v), AVG(v)
    ... GROUP BY a, b: (g, seconds, group_columns, *aggregate_columns).  group_columns is a tuple with one array per key column, the
    distinct tuples, every aggregate column aligned with them; the order of the groups is unspecified.  columns is a sequence of key
    columns of equal length and one kind, each converted as `factorize_columns` converts them (a single array is one column).
    aggs, "mean", signed, float64, max_groups, the output dtypes and the containers are exactly `group_by_agg`'s.
    Two columns are ONE library call (C ABI: algo | FJ_ALGO_GROUP_BY | FJ_ALGO_KEY_PAIR | FJ_ALGO_AGG_ALL): the relation goes through
    the partition passes once and no group ids are written, where factorize_columns + group_by_agg(codes, v) + two gathers take two
    trips.  One column delegates to `group_by_agg`.  Three or more fold the leading columns with `factorize_columns`, make the one
    fused call on (codes, last column, values) and recover the leading columns as c[first_index[codes of the groups]]; `seconds` is the
    sum.  values=None is allowed with aggs == ("count",) alone."""
    name = "group_by_agg_columns"
    aggs = _check_aggs(name, aggs, float64)
    max_groups = _check_max_groups(name, max_groups)
    cols, _ = _key_columns(name, "columns", columns)
    if not cols:
        raise ValueError(f"{name}: columns is empty (name at least one key column)")
    if values is None:
        if aggs != ("count",):
            raise ValueError(f"{name}: values is required unless aggs == ('count',) (got aggs = {aggs!r})")
        if float64 or signed is not None:
            raise ValueError(f"{name}: values=None counts rows: float64 and signed describe a value column")
        values = cols[-1]                                    # (any column stands in: the counts read none)
        signed = False
    if len(cols) == 1:
        g, sec, gk, *out = group_by_agg(cols[0], values, aggs, signed, float64, max_groups)
        return (g, sec, (gk,), *out)
    values, signed, unsigned_in = _word_column(name, "values", values, signed, float64)
    flags, unsigned_out = _agg_flags(signed, float64), unsigned_in and not signed
    if _is_torch_tensor(values) and not values.is_cuda:
        values = values.numpy()                              # (as _key_columns takes host tensors)
    if _is_torch_tensor(cols[0]) != _is_torch_tensor(values):
        raise TypeError(f"{name}: columns and values must be of one kind, got NumPy and torch side by side")
    nv = values.numel() if _is_torch_tensor(values) else values.size
    if nv != cols[0].shape[0]:
        raise ValueError(f"{name}: values has {nv} elements, the key columns have {cols[0].shape[0]} rows")
    sec0, lead_first = 0.0, None
    a = cols[0]
    if len(cols) > 2:                                        # the leading columns as one column of dense codes
        _, sec0, codes, lead_first = factorize_columns(cols[:-1])
        a = _dev_tensor(codes, "codes") if _is_torch_tensor(codes) else _as_u64_host(codes, "codes")
    g, sec, ga, planes = _group_by_pair_all(a, cols[-1], values, flags, max_groups)
    gb = planes[0] if _is_torch_tensor(planes) else planes[0].view(np.uint64)
    if lead_first is None:
        group_columns = (ga, gb)
    else:                                                    # (ga holds the groups' codes: any row of a code carries its leading tuple)
        rows = lead_first[ga if _is_torch_tensor(ga) else ga.view(np.int64)]
        group_columns = tuple(c[rows] for c in cols[:-1]) + (gb,)
    return (g, sec0 + sec, group_columns, *_agg_columns(planes[1:], aggs, float64, unsigned_out))


# ---- extension: the row that holds each group's minimum / maximum (csrc/fj_groupby_arg.hip) ------------------------------------------------
def _group_by_arg(keys, values, flags: int):
    """(g, seconds, group_keys, planes): ONE library call, FJ_ALGO_GROUP_BY | FJ_ALGO_AGG_ARG | flags.  planes is a (2, g) array of int64
    words where the inputs live - the row indices and the extremes - each row aligned with group_keys.  flags: ALGO_AGG_MIN or
    ALGO_AGG_MAX, a base value (ALGO_SCALAR, ALGO_RADIX), ALGO_AGG_SIGNED or ALGO_AGG_FLOAT."""
    k, v, n = _group_columns(keys, values)
    return _group_by_call(ALGO_ADAPTIVE | ALGO_GROUP_BY | ALGO_AGG_ARG | flags, k, v, None, n, 2)


def _group_by_argext(name: str, flag: int, keys, values, signed, float64: bool, return_values: bool):
    if values is None:
        raise ValueError(f"{name}: values is required")
    values, signed, unsigned_in = _word_column(name, "values", values, signed, float64)
    g, sec, gk, planes = _group_by_arg(keys, values, flag | _agg_flags(signed, float64))
    if not return_values:
        return g, sec, gk, planes[0]
    return g, sec, gk, planes[0], _agg_values(planes[1], signed, unsigned_in, float64)


def group_by_argmin(keys, values, signed=None, float64: bool = False, return_values: bool = False):
    """GROUP BY keys and, per key, the ROW that holds MIN(values) - pandas idxmin, SQL arg_min: (g, seconds, group_keys, row_index),
    row_index int64, one per group, aligned with group_keys (whose order is unspecified): keys[row_index] == group_keys, and
    values[row_index] are the minima - gather any other column of the relation with it ("the cheapest offer per product": which
    offer).  Ties: the SMALLEST row index wins (first occurrence), so the result is deterministic.  ONE library call: the relation
    goes through the partition passes once, where group_by_min + lookup + a second group_by_min over the surviving positions take
    three trips.  return_values=True appends the minima, with the dtype group_by_min returns.
    signed and float64 follow group_by_min exactly: signed=None takes the sign from the container (a NumPy uint64 column compares
    unsigned, everything else signed), True / False force it; float64=True reads a floating-point column as numbers (`signed` must
    stay None, integers raise TypeError): -0.0 and +0.0 tie, and a group that holds a NaN has an unspecified value and an index in
    [-1, len(keys)) while every other group is unaffected.  Every group has a row, so every other index is a valid row - also where
    the minimum equals the aggregate's identity.  NumPy in, NumPy out; torch ROCm tensors / DLPack are read in place on the current
    stream and every output is a tensor on their device."""
    return _group_by_argext("group_by_argmin", ALGO_AGG_MIN, keys, values, signed, float64, return_values)


def group_by_argmax(keys, values, signed=None, float64: bool = False, return_values: bool = False):
    """GROUP BY keys and, per key, the row that holds MAX(values): the max form of group_by_argmin.  Ties: the smallest row index,
    as there ("the latest event per user": the first row with the latest timestamp)."""
    return _group_by_argext("group_by_argmax", ALGO_AGG_MAX, keys, values, signed, float64, return_values)


# ---- extension: merging partial group-by results (csrc/fj_groupby_merge.hip) ---------------------------------------------------------------
def _group_by_merge(k, planes, flags: int, max_groups: Optional[int] = None):
    """(g, seconds, group_keys, planes): ONE library call, FJ_ALGO_GROUP_BY | FJ_ALGO_AGG_ALL | FJ_ALGO_AGG_MERGE | flags.  k: the n keys
    of the partial rows, planes: their (4, n) words - counts, sums, minima, maxima - both NumPy (uint64) or both contiguous torch.int64
    on one device.  Returns what _group_by_all returns.  flags: a base value, ALGO_AGG_SIGNED or ALGO_AGG_FLOAT."""
    if _is_torch_tensor(k):
        n = k.numel()
        if tuple(planes.shape) != (4, n) or not planes.is_contiguous() or planes.device != k.device:
            raise ValueError(f"_group_by_merge: planes must be a contiguous (4, {n}) tensor on the keys' device")
    else:
        n = k.size
        if planes.shape != (4, n):
            raise ValueError(f"_group_by_merge: planes must be a (4, {n}) array")
        k, planes = _as_u64_host(k, "keys"), _as_u64_host(planes, "planes")
    return _group_by_call(ALGO_ADAPTIVE | ALGO_GROUP_BY | ALGO_AGG_ALL | ALGO_AGG_MERGE | flags, k, planes, None, n, 4, max_groups=max_groups,
                          overflow=f"group_by_merge: the partial rows hold g = {{g}} distinct keys, max_groups = {max_groups}")


def _is_array(x: Any) -> bool:
    return isinstance(x, np.ndarray) or _is_torch_tensor(x) or hasattr(x, "__dlpack_device__")


def _parts(x: Any) -> list:
    """one array, or a sequence of arrays (the partials of several batches), as a list of arrays"""
    if isinstance(x, (list, tuple)) and (not x or all(_is_array(p) for p in x)):
        return [_from_dlpack_if_device(p) for p in x]
    return [_from_dlpack_if_device(x)]


def _container(x: Any):
    """where an array lives: "numpy", or ("device", index).  A torch tensor in host memory counts as NumPy, as everywhere"""
    if _is_torch_tensor(x) and x.is_cuda:
        return ("device", _device_index(x))
    return "numpy"


def _same_container(name: str, arrays, want=None):
    """the one container of all `arrays` (and `want`, where given), or the TypeError"""
    for a in arrays:
        c = _container(a)
        if want is None:
            want = c
        if c != want:
            raise TypeError(f"{name}: every argument must be of one kind and on one device, got {want} and {c}")
    return want or "numpy"


def _check_signed(name: str, signed: Any) -> None:
    if signed is not None and not isinstance(signed, (bool, np.bool_)):
        raise TypeError(f"{name}: signed must be None, True or False, got {type(signed).__name__}")


def _word_column(name: str, what: str, col: Any, signed: Any, float64: bool, integers_only: bool = True):
    """(words, signed, unsigned_in): a sum / min / max column as 8-byte words in its container, under the rules of group_by_min -
    signed=None takes the sign from the container: a NumPy uint64 column (a torch.uint64 tensor) compares unsigned, everything else
    signed - and of float64=True.  A device array of another library is a torch tensor from here on.  integers_only=False (the
    group_join_* and Index.group_* forms): a column that is not of integers is not refused here - a NumPy float column is value-cast
    to words, as ever, and a torch float tensor is refused where the device tensors are checked"""
    if float64:
        return _float_words(name, what, col, signed), False, False
    _check_signed(name, signed)
    col = _from_dlpack_if_device(col)
    if _is_torch_tensor(col):
        if integers_only and col.dtype.is_floating_point:
            raise TypeError(f"{name}: {what} must be 64-bit integers, got {col.dtype} (the words are compared as integers{_FLOAT64_HINT})")
        unsigned_in = str(col.dtype) == "torch.uint64"
    else:
        col = np.asarray(col)
        if integers_only and col.dtype.kind not in "iub":
            raise TypeError(f"{name}: {what} must be integers, got dtype {col.dtype} (the words are compared as integers{_FLOAT64_HINT})")
        unsigned_in = col.dtype == np.uint64
    return col, ((not unsigned_in) if signed is None else bool(signed)), unsigned_in


def _agg_flags(signed: bool, float64: bool) -> int:
    """how the words of a value column compare and add: as float64, as two's-complement int64, or as uint64"""
    return ALGO_AGG_FLOAT if float64 else (ALGO_AGG_SIGNED if signed else 0)


def _agg_values(words, signed: bool, unsigned_in: bool, float64: bool):
    """a column of minima / maxima with the dtype the single forms return: float64; the column's own dtype for a NumPy uint64 column
    compared unsigned; otherwise the int64 storage of the words"""
    if float64:
        return _as_float64(words)
    if unsigned_in and not signed and isinstance(words, np.ndarray):
        return words.view(np.uint64)
    return words


def _count_column(name: str, col: Any):
    if not _is_torch_tensor(col):
        col = np.asarray(col)
    if str(col.dtype).replace("torch.", "") not in ("int64", "uint64"):
        raise TypeError(f"{name}: counts must be int64 or uint64, got {col.dtype}")
    return col


def _pack_partials(name: str, parts, container):
    """parts: [(keys, counts, sums, mins, maxs)] of words in one container -> (key buffer of n, (4, n) buffer): ONE copy of every
    word into the layout the C ABI reads"""
    n = sum(int(p[0].shape[0]) for p in parts)
    if container == "numpy":
        k, planes = np.empty(n, np.uint64), np.empty((4, n), np.uint64)
        at = 0
        for p in parts:
            m = p[0].shape[0]
            k[at:at + m] = _as_u64_host(p[0], "keys")
            for q in range(4):
                planes[q, at:at + m] = _as_u64_host(p[1 + q], name)
            at += m
        return k, planes
    import torch
    words = lambda t: t.reshape(-1).view(torch.int64) if t.dtype == torch.uint64 else t.reshape(-1)
    dev = torch.device("cuda", container[1])
    k, planes = torch.empty(n, dtype=torch.int64, device=dev), torch.empty((4, n), dtype=torch.int64, device=dev)
    if parts:                                                # one torch.cat per column, whatever the number of batches
        torch.cat([words(_dev_tensor(p[0], "keys")) for p in parts], out=k)
        for q in range(4):
            torch.cat([words(_dev_tensor(p[1 + q], name)) for p in parts], out=planes[q])
    return k, planes


def _partial_words(name: str, keys, counts, sums, mins, maxs, signed, float64: bool):
    """the five arguments of group_by_merge, checked: ([(keys, counts, sums, mins, maxs)] as words, container, signed, unsigned_out)"""
    cols = [_parts(x) for x in (keys, counts, sums, mins, maxs)]
    names = ("keys", "counts", "sums", "mins", "maxs")
    for nm, c in zip(names[1:], cols[1:]):
        if len(c) != len(cols[0]):
            raise ValueError(f"{name}: {nm} has {len(c)} arrays, keys has {len(cols[0])} (one of each per batch)")
    if float64 and signed is not None:
        raise TypeError(f"{name}: signed must be None with float64=True (a float64 carries its own sign), got {signed!r}")
    container = _same_container(name, [a for c in cols for a in c if _is_array(a)])
    parts, resolved, unsigned_out = [], None, False
    for i in range(len(cols[0])):
        k, c = cols[0][i], _count_column(name, cols[1][i])
        if not _is_array(k):
            k = _as_u64_host(k, "keys")
        row = [k, c]
        for nm, col in zip(names[2:], (cols[2][i], cols[3][i], cols[4][i])):
            w, sg, unsigned_in = _word_column(name, nm, col, signed, float64)
            if nm == "mins" and resolved is None:
                resolved, unsigned_out = sg, unsigned_in and not sg
            row.append(w)
        lens = [int(np.prod(a.shape)) for a in row]
        for nm, ln in zip(names[1:], lens[1:]):
            if ln != lens[0]:
                raise ValueError(f"{name}: {nm} has {ln} elements, keys has {lens[0]}")
        parts.append(tuple(a.reshape(-1) for a in row))
    return parts, container, bool(resolved), unsigned_out


def group_by_merge(keys, counts, sums, mins, maxs, signed=None, float64: bool = False, max_groups: Optional[int] = None):
    """Merge PARTIAL group-by results - what group_by_agg returned for every batch of a column that arrives in morsels, for every shard
    of a relation, or Index.group_* with its counts: (g, seconds, group_keys, counts, sums, mins, maxs), one row per distinct key of
    `keys`, the rows that share a key combined - the counts and the sums add (modulo 2^64; float64 sums in an unspecified order), the
    minima and maxima take the extreme.  The order of group_keys is unspecified; the four columns are aligned with it.
    Every argument is one array, or a sequence of arrays - one per batch: they are copied ONCE into one key buffer and one (4, n)
    buffer, and the merge is ONE library call, where factorize of the concatenated keys plus four scatters over the codes takes a trip
    through the partition passes and four scattered passes.  Containers, dtypes and errors follow group_by_agg: NumPy arrays or torch
    ROCm tensors / DLPack, all of one kind and on one device (TypeError otherwise); counts int64 or uint64; sums, mins and maxs integer
    words, or floating point with float64=True (an integer column is a TypeError then); signed=None takes the sign from the container
    of `mins` as group_by_min does (a NumPy uint64 column compares unsigned, everything else signed), True / False force it.
    Columns of unequal length are a ValueError.  A row with count 0 whose sum, min and max hold the aggregates' identities (what
    Index.group_* leaves for a key without a partner) is legal: its key is a group of the result, with count 0 unless another row of
    that key says otherwise.  max_groups bounds the device buffers as in group_by_agg: a result beyond it raises ValueError naming g
    and the context stays usable.  No rows: g = 0 and empty arrays."""
    max_groups = _check_max_groups("group_by_merge", max_groups)
    parts, container, signed, unsigned_out = _partial_words("group_by_merge", keys, counts, sums, mins, maxs, signed, float64)
    k, planes = _pack_partials("group_by_merge", parts, container)
    if k.shape[0] == 0:
        g, sec, gk, out = 0, 0.0, k, (planes.view(np.int64) if container == "numpy" else planes)
    else:
        g, sec, gk, out = _group_by_merge(k, planes, _agg_flags(signed, float64), max_groups)
    return (g, sec, gk, *_agg_columns(out, ("count", "sum", "min", "max"), float64, unsigned_out))


class GroupByAccumulator:
    """A running GROUP BY keys with COUNT, SUM, MIN and MAX of one value column over batches whose key set is not known beforehand:

        acc = GroupByAccumulator()
        for keys, values in batches: acc.update(keys, values)
        g, seconds, group_keys, counts, sums, mins, maxs = acc.result()

    update() groups the batch with group_by_agg (all four aggregates) and keeps the partial result; once the pending partial rows reach
    max(rows of the merged state, compact_at) the state and all pending partials become a new state with ONE group_by_merge.  A merge
    therefore handles at most twice the rows that arrived since the last one, and the total merge work stays within a constant factor
    of the partial rows seen, however many batches there are.  compact_at is a policy constant, not a measured optimum: it keeps
    small batches from merging one by one (tests set it small).
    signed, float64 and max_groups are group_by_agg's and hold for every batch.  The accumulator keeps the container kind and the
    device of its first batch, and the signedness that batch resolved to: a later batch of another kind, device or signedness is a
    TypeError and leaves the accumulator as it was.  merge() takes another accumulator or a (keys, counts, sums, mins, maxs) tuple - a
    shard's result, or an Index.group_* result with its counts (rows of count 0 included).  result() compacts and returns
    (g, seconds, group_keys, *columns) exactly as group_by_agg does; with no batch g = 0.  close() drops the buffers; a context manager."""

    def __init__(self, signed=None, float64: bool = False, max_groups: Optional[int] = None, compact_at: int = 65536):
        if float64 and signed is not None:
            raise TypeError(f"GroupByAccumulator: signed must be None with float64=True (a float64 carries its own sign), got {signed!r}")
        _check_signed("GroupByAccumulator", signed)
        if isinstance(compact_at, (bool, np.bool_)) or not isinstance(compact_at, (int, np.integer)) or compact_at < 1:
            raise ValueError(f"GroupByAccumulator: compact_at must be an integer >= 1, got {compact_at!r}")
        self._signed_arg, self._float64 = signed, bool(float64)
        self._max_groups = _check_max_groups("GroupByAccumulator", max_groups)
        self._compact_at = int(compact_at)
        self._container = None                               # of the first batch; with it the resolved signedness
        self._signed = self._unsigned_out = False
        self._state = None                                   # (keys, (4, g) planes) of distinct keys, as words
        self._pending: list = []                             # (keys, counts, sums, mins, maxs) partials not merged yet, as words
        self._pending_rows = self._rows_seen = self._merges = 0
        self._closed = False

    # -- bookkeeping ---------------------------------------------------------------------------------------------------------------
    @property
    def num_groups(self) -> int:
        """the groups of the merged state (after the last compaction; the pending partials are not counted)"""
        return 0 if self._state is None else int(self._state[0].shape[0])

    @property
    def pending_rows(self) -> int:
        return self._pending_rows

    @property
    def rows_seen(self) -> int:
        """the input rows behind everything taken so far: the rows of every batch, the counts of every merged partial"""
        return self._rows_seen

    @property
    def merges(self) -> int:
        """the library merge calls so far"""
        return self._merges

    def close(self) -> None:
        self._state, self._pending, self._pending_rows, self._closed = None, [], 0, True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _open(self, who: str) -> None:
        if self._closed:
            raise ValueError(f"{who}: the accumulator is closed")

    def _agree(self, who: str, container, signed: bool) -> None:
        """a later input must have the container and the signedness the first one fixed (checked before anything is kept)"""
        if self._container is None:
            return
        if container != self._container:
            raise TypeError(f"{who}: this accumulator holds {self._container} data, got {container} (one container kind and one device)")
        elif signed != self._signed:
            raise TypeError(f"{who}: this accumulator compares {'signed' if self._signed else 'unsigned'}, the input resolves to "
                            f"{'signed' if signed else 'unsigned'} (pass signed= to the constructor)")

    def _take(self, parts, rows: int, container, signed: bool, unsigned_out: bool) -> float:
        if self._container is None:
            self._container, self._signed, self._unsigned_out = container, signed, unsigned_out
        self._pending.extend(parts)
        self._pending_rows += sum(int(p[0].shape[0]) for p in parts)
        self._rows_seen += rows
        return self._compact() if self._pending_rows >= max(self.num_groups, self._compact_at) else 0.0

    def _compact(self) -> float:
        """state + pending -> state with one group_by_merge; seconds of that call (nothing pending: no call)"""
        if not self._pending:
            return 0.0
        k, planes = _pack_partials("GroupByAccumulator", self._partials(), self._container)
        sec = 0.0
        if k.shape[0]:
            g, sec, k, planes = _group_by_merge(k, planes, _agg_flags(self._signed, self._float64), self._max_groups)
            self._merges += 1
        self._state = (k, planes)
        self._pending, self._pending_rows = [], 0
        return sec

    def _partials(self) -> list:
        """the merged state and the pending partials as (keys, counts, sums, mins, maxs) rows"""
        return ([(self._state[0], *self._state[1])] if self._state is not None else []) + self._pending

    # -- input ---------------------------------------------------------------------------------------------------------------------
    def update(self, keys, values):
        """One batch: (g_batch, seconds) - the batch's distinct keys, and the device time of its group_by_agg plus that of the merge
        it set off, if any."""
        self._open("GroupByAccumulator.update")
        keys, values = _from_dlpack_if_device(keys), _from_dlpack_if_device(values)
        if values is None:
            raise ValueError("GroupByAccumulator.update: values is required")
        container = _same_container("GroupByAccumulator.update", [a for a in (keys, values) if _is_array(a)])
        _, signed, unsigned_in = _word_column("GroupByAccumulator.update", "values", values, self._signed_arg, self._float64)
        self._agree("GroupByAccumulator.update", container, signed)
        g, sec, gk, c, s, mn, mx = group_by_agg(keys, values, signed=self._signed_arg, float64=self._float64, max_groups=self._max_groups)
        words = _as_float64_words if self._float64 else (lambda a: a)
        rows = int(np.prod(keys.shape)) if _is_array(keys) else len(keys)
        return g, sec + self._take([(gk, c, words(s), words(mn), words(mx))], rows, container, signed, unsigned_in and not signed)

    def merge(self, other):
        """Another accumulator's groups (it stays as it is), or a (keys, counts, sums, mins, maxs) tuple of partial rows - every item
        one array or a sequence of arrays, as for group_by_merge: seconds of the merge this set off, 0.0 if none."""
        self._open("GroupByAccumulator.merge")
        if isinstance(other, GroupByAccumulator):
            other._open("GroupByAccumulator.merge")
            if other._float64 != self._float64:
                raise TypeError("GroupByAccumulator.merge: one accumulator is float64, the other is not")
            if other._container is None:
                return 0.0
            self._agree("GroupByAccumulator.merge", other._container, other._signed)
            return self._take(other._partials(), other._rows_seen, other._container, other._signed, other._unsigned_out)
        if not isinstance(other, (tuple, list)) or len(other) != 5:
            raise TypeError("GroupByAccumulator.merge: another GroupByAccumulator, or a (keys, counts, sums, mins, maxs) tuple")
        parts, container, signed, unsigned_out = _partial_words("GroupByAccumulator.merge", *other, self._signed_arg, self._float64)
        self._agree("GroupByAccumulator.merge", container, signed)
        return self._take(parts, sum(int(p[1].sum()) for p in parts), container, signed, unsigned_out)

    # -- output --------------------------------------------------------------------------------------------------------------------
    def result(self, aggs=("count", "sum", "min", "max")):
        """(g, seconds, group_keys, *columns) as group_by_agg returns them, one column per name in aggs ("mean" only with float64=True);
        seconds: the merge this call made, 0.0 when everything was merged already.  The accumulator goes on taking batches."""
        self._open("GroupByAccumulator.result")
        aggs = _check_aggs("GroupByAccumulator.result", aggs, self._float64)
        sec = self._compact()
        k, planes = self._state if self._state is not None else (np.empty(0, np.uint64), np.empty((4, 0), np.int64))
        if isinstance(planes, np.ndarray):
            planes = planes.view(np.int64)
        return (int(k.shape[0]), sec, k, *_agg_columns(planes, aggs, self._float64, self._unsigned_out))


def group_by_accumulator(signed=None, float64: bool = False, max_groups: Optional[int] = None, compact_at: int = 65536) -> GroupByAccumulator:
    """GroupByAccumulator(...), under the naming of build_index"""
    return GroupByAccumulator(signed=signed, float64=float64, max_groups=max_groups, compact_at=compact_at)


# ---- extension: gather maps (row positions instead of keys and values) ------------------------------------------------------
_HOW ={"inner": 0, "left": ALGO_LEFT_OUTER, "anti": ALGO_ANTI, "full": ALGO_FULL_OUTER, "semi": 0}


def join_indices(build_keys, probe_keys, how: str = "inner", many_to_many: bool = False, duplicates: str = "first"):
    """Row-index gather maps of a join: which probe row matched which build row, so that the caller can gather the other
    columns of both tables.  Positions are 0-based row numbers of the flattened inputs; order within each range unspecified.

    how="inner"  (n, seconds, probe_idx, build_idx): one row per matched probe row, build_idx the key's FIRST occurrence
                 (smallest build row); many_to_many=True: one row per (probe row, build row) pair with equal keys.
    how="left"   (m, seconds, probe_idx, build_idx): every probe row once, rows [0, m) matched, rows [m, len(probe_keys))
                 unmatched with build_idx == -1; m = matched rows, as left_join returns.
    how="anti"   (u, seconds, probe_idx, None): the u probe rows whose key is not among the build keys.
    how="semi"   (s, seconds, probe_idx, None): the s probe rows whose key IS among the build keys, each once.
    how="full"   (m, r, seconds, probe_idx, build_idx): len(probe_keys) + r rows - the rows of how="left", then the r build rows
                 whose key is not among the probe keys with probe_idx == -1 (every copy of a duplicated key).
    duplicates="all" (every copy of a duplicated build key; "first" is the rule above):
    how="left"   (P, u, seconds, probe_idx, build_idx): P + u rows - one per (probe row, build row) pair with equal keys, then the
                 u probe rows without a partner with build_idx == -1.
    how="full"   (P, u, r, seconds, probe_idx, build_idx): P + u + r rows - those, then the r build rows whose key is not among
                 the probe keys with probe_idx == -1.
    how="inner"  the same as many_to_many=True; how="semi" / "anti": as without it (multiplicity does not matter to them).
    A final partition of more than 4096 build rows is refused by the many-to-many forms; set_option("mm_heavy_keys", 1) lifts that
    for how="inner" (many_to_many=True or duplicates="all"), set_option("mm_heavy_outer", 1) for duplicates="all" with
    how="left" / "full"; the two options are independent.
    The index arrays are int64: NumPy for host inputs, torch.int64 on the inputs' device for device tensors / DLPack."""
    if how not in _HOW:
        raise ValueError(f"join_indices: how must be one of {sorted(_HOW)}, got {how!r}")
    if many_to_many and how != "inner":
        raise ValueError(f"join_indices: many_to_many=True needs how='inner' (got how={how!r})")
    all_copies = _all_copies(duplicates, "join_indices")
    as_i64 = lambda a: a if a is None or _is_torch_tensor(a) else np.asarray(a).view(np.int64)
    if all_copies and how in ("left", "full"):
        (P, r, u), sec, pi, bi = _join(ALGO_ADAPTIVE | _HOW[how] | ALGO_ALL_COPIES | ALGO_ROW_IDS, 0, 1, build_keys, None, probe_keys, True)
        return (P, u, sec, as_i64(pi), as_i64(bi)) if how == "left" else (P, u, r, sec, as_i64(pi), as_i64(bi))
    many_to_many = many_to_many or (all_copies and how == "inner")
    algo = (ALGO_RADIX | ALGO_MANY_TO_MANY if many_to_many else ALGO_ADAPTIVE | _HOW[how]) | ALGO_ROW_IDS
    n, sec, pi, bi = _join(algo, 0, 1, build_keys, None, probe_keys, True)
    if how == "full":
        return n[0], n[1], sec, as_i64(pi), as_i64(bi)
    if how == "semi":
        return n, sec, as_i64(pi), None
    return n, sec, as_i64(pi), as_i64(bi)


def sort_pairs(keys, values):
    """The pairs a `return_arrays=True` join handed back, in (key, value) order as unsigned 64-bit integers - the join's own
    output order is unspecified, so comparisons go through this.  NumPy arrays or device tensors."""
    if _is_torch_tensor(keys):
        import torch
        if keys.numel() == 0:
            return keys, values
        flip = torch.tensor(-(1 << 63), dtype=torch.int64, device=keys.device)     # int64 storage: order as uint64
        k, v = keys.reshape(-1) ^ flip, values.reshape(-1) ^ flip
        i = torch.argsort(v, stable=True)
        j = torch.argsort(k[i], stable=True)
        o = i[j]
        return keys.reshape(-1)[o], values.reshape(-1)[o]
    k, v = np.asarray(keys).reshape(-1).view(np.uint64), np.asarray(values).reshape(-1).view(np.uint64)
    o = np.lexsort((v, k))
    return k[o], v[o]


def initialize() -> None:
    """Replaces initialize_memory_system (hash_join.cpp:596, :639): checks that a HIP device is
    usable and warms up the native context. Returns None like the reference."""
    L = _lib.load()
    check(L.fj_initialize())
    context(0)
    return None


# benchmark.py's labels (benchmark.py:240-247) and BASELINE.json's wording, as aliases
flash_join = hash_join
flash_join_radix = hash_join_radix
flash_join_bloom = hash_join_bloom
flash_join_radix_bloom = hash_join_radix_bloom
adaptive_bloom = adaptive_join_bloom

REFERENCE_EXPORTS = [
    "adaptive_join", "adaptive_join_bloom", "adaptive_join_count", "adaptive_join_count_bloom",
    "hash_join_radix", "hash_join", "hash_join_radix_bloom", "hash_join_bloom",
    "hash_join_count_radix", "hash_join_count", "hash_join_count_radix_bloom", "hash_join_count_bloom",
    "initialize",
]
ALIASES = ["flash_join", "flash_join_radix", "flash_join_bloom", "flash_join_radix_bloom", "adaptive_bloom"]
EXTENSIONS = ["inner_join", "inner_join_count", "left_join", "anti_join", "anti_join_count", "join_indices",
              "full_join", "semi_join", "semi_join_count", "lookup", "isin", "lookup_indices", "group_join_count", "group_join_sum",
              "group_join_min", "group_join_max", "unique", "distinct_count", "group_by_count", "group_by_sum", "group_by_min", "group_by_max",
              "group_by_agg", "group_by_argmin", "group_by_argmax", "group_by_merge", "GroupByAccumulator", "group_by_accumulator", "factorize",
              "build_index"]
# multi-column keys: compositions over the entries above (`_group_by`, `factorize`), whose caller-context rows
# (tests/test_caller_context_cpu.py walks EXTENSIONS) cover the path they take; their own suite is tests/test_factorize_columns.py.
# group_by_agg_columns is NOT such a composition: it has a library entry of its own (`_group_by_pair_all`: ALGO_KEY_PAIR | ALGO_AGG_ALL,
# through `_group_by_call`'s context lookup, per-device lock and stream), as group_rows below has.  Like ROW_EXTENSIONS it is exempt from the
# caller-context walk, which reads EXTENSIONS only; what covers its caller context is its own suite, tests/test_group_by_agg_columns.py
# (device tensors in place, a side stream, a strided view, the inputs' device)
KEY_EXTENSIONS = ["factorize_columns", "encode_keys", "group_by_agg_columns"]
# the rows of every group: one entry of their own (ALGO_GROUP_ROWS) and a gather over it; their suite is tests/test_group_rows.py
ROW_EXTENSIONS = ["group_rows", "group_by_collect"]
__all__ = REFERENCE_EXPORTS + ALIASES + EXTENSIONS + KEY_EXTENSIONS + ROW_EXTENSIONS + ["last_timings", "join_device", "context", "set_option", "get_option", "sort_pairs", "workspace_bytes", "trim_workspace", "Index"]
