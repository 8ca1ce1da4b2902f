"""Group-by on one relation (FJ_ALGO_GROUP_BY, csrc/fj_groupby.hip; api.unique / distinct_count / group_by_count / group_by_sum /
group_by_min / group_by_max): the distinct keys of a relation and one aggregate per key.  The C-ABI contract and the argument checks
need no GPU; on an MI355X every form is compared with a NumPy reference on every plan.

Reference: np.unique(return_index, return_inverse, return_counts) and np.add.at / np.minimum.at / np.maximum.at over uint64 and int64
words; both sides sorted by key, exact integer equality, no hashing anywhere, never the library.

The three-pass plan: "plan_target_keys" has a lower bound of 16 and a plan takes three passes beyond 18 radix bits, so the 200 003-row
input reaches two passes at most (14 bits); the three-pass case therefore uses the smallest input that reaches 19 bits, 16 * 2^18 + 1
rows."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import hbm_timings
import keymix
from conftest import ROOT

MANY, LEFT, ANTI, ROW_IDS, FULL, ALL, PO, BO = 0x10, 0x20, 0x40, 0x80, 0x100, 0x200, 0x800, 0x1000
MIN, MAX, SIGNED, GB = 0x4000, 0x8000, 0x10000, 0x40000
U64_MAX = np.uint64(2**64 - 1)
I64_MIN, I64_MAX = np.uint64(2**63), np.uint64(2**63 - 1)               # the words of INT64_MIN / INT64_MAX


def ref_group_by(keys, vals):
    """dict of arrays aligned with the sorted distinct keys 'keys': first, count, sum (wrapping uint64), min_u, max_u, min_s, max_s"""
    keys, vals = np.asarray(keys, dtype=np.uint64), np.asarray(vals, dtype=np.uint64)
    uk, first, inv, cnt = np.unique(keys, return_index=True, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    g = uk.size
    r = {"keys": uk, "first": first.astype(np.int64), "count": cnt.astype(np.int64)}
    r["sum"] = np.zeros(g, np.uint64); np.add.at(r["sum"], inv, vals)                       # wraps modulo 2^64
    r["min_u"] = np.full(g, U64_MAX, np.uint64); np.minimum.at(r["min_u"], inv, vals)
    r["max_u"] = np.zeros(g, np.uint64); np.maximum.at(r["max_u"], inv, vals)
    sv = vals.view(np.int64)
    r["min_s"] = np.full(g, np.iinfo(np.int64).max, np.int64); np.minimum.at(r["min_s"], inv, sv)
    r["max_s"] = np.full(g, np.iinfo(np.int64).min, np.int64); np.maximum.at(r["max_s"], inv, sv)
    return r


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_header_flag_and_python_mirror():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    assert int(re.search(r"#define FJ_ALGO_GROUP_BY\s+(0x[0-9a-fA-F]+)", hdr).group(1), 16) == 0x40000
    from flash_hash_join_amd import api
    assert api.ALGO_GROUP_BY == 0x40000


def test_abi_version_and_function_count_are_unchanged():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    assert int(re.search(r"#define FJ_ABI_VERSION (\d+)", hdr).group(1)) == 8
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert len(set(re.findall(r"\b(fj_[a-z0-9_]+)\s*\(", code))) == 40
    assert "FJ_ALGO_GROUP_BY" in hdr                                  # (what makes this test one of the new feature's)
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_abi_version() == 8 and len(_lib.SYMBOLS) == 40


def test_flash_join_exposes_the_functions():
    import flash_join
    from flash_hash_join_amd import api
    for name in ("unique", "distinct_count", "group_by_count", "group_by_sum", "group_by_min", "group_by_max"):
        assert callable(getattr(flash_join, name)) and name in api.EXTENSIONS and name in api.__all__


def _device_call(algo, materialize=1, vals=0x20000, pk=None, n_p=0, ok=0x40000, ov=0x50000, cap=100, nb=100):
    from flash_hash_join_amd import _lib
    cnt = ctypes.c_uint64(0)
    rc = _lib.load().fj_join_device(None, algo, 0, materialize, 0x10000, vals, nb, pk, n_p, None, 64, ctypes.byref(cnt), ok, ov, cap, None)
    return rc, _lib.last_error()


DEVICE_REFUSALS = [   # id, keyword arguments of _device_call, needles
    ("many", dict(algo=GB | MANY), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_MANY_TO_MANY",)),
    ("left", dict(algo=GB | LEFT), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_LEFT_OUTER",)),
    ("anti", dict(algo=GB | ANTI | 2), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_ANTI",)),
    ("full", dict(algo=GB | FULL), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_FULL_OUTER",)),
    ("all_copies", dict(algo=GB | ALL), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_ALL_COPIES",)),
    ("probe_order", dict(algo=GB | PO | 1), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_PROBE_ORDER",)),
    ("build_order", dict(algo=GB | BO), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_BUILD_ORDER",)),
    ("build_order_min", dict(algo=GB | BO | MIN), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_BUILD_ORDER",)),
    ("probe_keys", dict(algo=GB, pk=0x30000), ("FJ_ALGO_GROUP_BY", "no probe side")),
    ("probe_rows", dict(algo=GB | 2, n_p=7), ("FJ_ALGO_GROUP_BY", "no probe side")),
    ("probe_keys_and_rows", dict(algo=GB, pk=0x30000, n_p=7, materialize=0), ("FJ_ALGO_GROUP_BY", "no probe side")),
    ("min_and_max", dict(algo=GB | MIN | MAX), ("FJ_ALGO_AGG_MIN cannot be combined with FJ_ALGO_AGG_MAX",)),
    ("signed_alone", dict(algo=GB | SIGNED), ("FJ_ALGO_AGG_SIGNED modifies FJ_ALGO_AGG_MIN or FJ_ALGO_AGG_MAX",)),
    ("min_without_values", dict(algo=GB | MIN, vals=None), ("FJ_ALGO_AGG_MIN", "d_build_vals")),
    ("max_without_values", dict(algo=GB | MAX | SIGNED | 1, vals=None), ("FJ_ALGO_AGG_MAX", "d_build_vals")),
    ("row_ids_min", dict(algo=GB | ROW_IDS | MIN), ("FJ_ALGO_ROW_IDS cannot be combined with FJ_ALGO_AGG_MIN",)),
    ("row_ids_max", dict(algo=GB | ROW_IDS | MAX | SIGNED), ("FJ_ALGO_ROW_IDS cannot be combined with FJ_ALGO_AGG_MAX",)),
    ("row_ids_count_only", dict(algo=GB | ROW_IDS, materialize=0), ("FJ_ALGO_ROW_IDS", "materialize = 1")),
    ("no_keys_output", dict(algo=GB, ok=None), ("FJ_ALGO_GROUP_BY", "d_out_keys")),
    ("capacity", dict(algo=GB, cap=99), ("output capacity 99 < 100",)),
    ("capacity_keys_only", dict(algo=GB | 1, ov=None, vals=None, cap=0), ("output capacity",)),
    ("misaligned_keys", dict(algo=GB, ok=0x40004), ("8-byte aligned",)),
    ("misaligned_vals", dict(algo=GB | 2, ov=0x50004), ("8-byte aligned",)),
]


@pytest.mark.parametrize("cid,kw,needles", DEVICE_REFUSALS, ids=[r[0] for r in DEVICE_REFUSALS])
def test_invalid_combinations_are_refused_before_any_device_work(cid, kw, needles):
    """A NULL context: the checks come before the context is touched (no GPU needed; the pointers are never dereferenced)."""
    rc, err = _device_call(**kw)
    assert rc != 0 and "null context" not in err, err
    for needle in needles:
        assert needle in err, err


FORM_FLAGS = [   # id, flags, keyword arguments of _device_call
    ("count", 0, dict(vals=None)),
    ("distinct", 0, dict(vals=None, ov=None)),
    ("sum", 0, dict()),
    ("min_u", MIN, dict()),
    ("min_s", MIN | SIGNED, dict()),
    ("max_u", MAX, dict()),
    ("max_s", MAX | SIGNED, dict()),
    ("row_ids", ROW_IDS, dict(vals=None)),
    ("row_ids_values_ignored", ROW_IDS, dict()),
    ("count_only", 0, dict(materialize=0, vals=None, ok=None, ov=None, cap=0)),
    ("count_only_with_values", 0, dict(materialize=0, ok=None, ov=None, cap=0)),
    ("more_capacity_than_rows", 0, dict(cap=5000)),
]
VALID = [(f"{('adaptive', 'scalar', 'radix')[base]}-{fid}", dict(algo=GB | base | flags, **kw)) for base in (0, 1, 2) for fid, flags, kw in FORM_FLAGS]


@pytest.mark.parametrize("cid,kw", VALID, ids=[v[0] for v in VALID])
def test_valid_combinations_reach_the_context(cid, kw):
    rc, err = _device_call(**kw)
    assert rc != 0 and "null context" in err, err


def test_other_bits_and_bases_are_still_unknown():
    for algo, needle in ((0x400, "unknown algo 1024"), (0x2000, "unknown algo 8192"), (0x20000, "unknown algo 131072"), (MIN, "unknown algo 16384"),
                         (MAX | SIGNED, "unknown algo"), (GB | 0x400, "unknown algo"), (GB | 0x2000, "unknown algo"), (GB | 0x20000, "unknown algo"),
                         (GB | 0x80000, "unknown algo"), (GB | 3, "unknown algo"), (GB | 9, "unknown algo")):
        rc, err = _device_call(algo=algo)
        assert rc != 0 and needle in err and "null context" not in err, (hex(algo), err)


HOST_REFUSALS = [   # id, algo, materialize, values, probe keys, np, needles
    ("many", GB | MANY, 1, True, False, 0, ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_MANY_TO_MANY",)),
    ("left", GB | LEFT, 1, True, False, 0, ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_LEFT_OUTER",)),
    ("anti", GB | ANTI, 1, True, False, 0, ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_ANTI",)),
    ("full", GB | FULL | 2, 1, True, False, 0, ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_FULL_OUTER",)),
    ("all_copies", GB | ALL, 1, True, False, 0, ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_ALL_COPIES",)),
    ("probe_order", GB | PO, 1, True, False, 0, ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_PROBE_ORDER",)),
    ("build_order", GB | BO, 1, True, False, 0, ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_BUILD_ORDER",)),
    ("probe_keys", GB, 1, True, True, 0, ("no probe side",)),
    ("probe_rows", GB, 0, True, True, 8, ("no probe side",)),
    ("min_and_max", GB | MIN | MAX, 1, True, False, 0, ("FJ_ALGO_AGG_MIN cannot be combined with FJ_ALGO_AGG_MAX",)),
    ("signed_alone", GB | SIGNED, 1, True, False, 0, ("FJ_ALGO_AGG_SIGNED modifies",)),
    ("min_without_values", GB | MIN, 1, False, False, 0, ("FJ_ALGO_AGG_MIN", "build_vals")),
    ("row_ids_max", GB | ROW_IDS | MAX, 1, True, False, 0, ("FJ_ALGO_ROW_IDS cannot be combined with FJ_ALGO_AGG_MAX",)),
    ("row_ids_count_only", GB | ROW_IDS, 0, False, False, 0, ("FJ_ALGO_ROW_IDS", "materialize = 1")),
    ("next_bit", GB | 0x80000, 1, True, False, 0, ("unknown algo",)),
    ("base_9", GB | 9, 1, True, False, 0, ("unknown algo",)),
    ("bare_min", MIN, 1, True, False, 0, ("unknown algo",)),
]


@pytest.mark.parametrize("cid,algo,materialize,vals,pk,n_p,needles", HOST_REFUSALS, ids=[r[0] for r in HOST_REFUSALS])
def test_host_entry_refusals(cid, algo, materialize, vals, pk, n_p, needles):
    """fj_join_host makes the same checks before its context is created (no GPU needed)."""
    from flash_hash_join_amd import _lib
    L = _lib.load()
    k = np.arange(8, dtype=np.uint64)
    cnt, sec = ctypes.c_uint64(0), ctypes.c_double(0)
    ok, ov = ctypes.c_void_p(), ctypes.c_void_p()
    rc = L.fj_join_host(algo, 0, materialize, k.ctypes.data, k.ctypes.data if vals else None, 8, k.ctypes.data if pk else None, n_p,
                        ctypes.byref(cnt), ctypes.byref(sec), ctypes.byref(ok), ctypes.byref(ov))
    err = _lib.last_error()
    assert rc != 0 and "null context" not in err and "HIP device" not in err, err
    for needle in needles:
        assert needle in err, err
    assert not ok.value and not ov.value


def test_python_argument_errors():
    from flash_hash_join_amd import api
    k = np.arange(4, dtype=np.uint64)
    with pytest.raises(ValueError, match="values has 3 elements, keys has 4"):
        api.group_by_sum(k, k[:3])
    with pytest.raises(ValueError, match="values has 5 elements, keys has 4"):
        api.group_by_min(k, np.arange(5, dtype=np.int64))
    with pytest.raises(ValueError, match="values has 5 elements"):
        api.group_by_max(k, np.arange(5, dtype=np.uint64), signed=True)
    with pytest.raises(ValueError, match="values is required"):
        api.group_by_sum(k, None)
    with pytest.raises(ValueError, match="values is required"):
        api.group_by_min(k, None)
    with pytest.raises(TypeError):
        api.group_by_sum(k)                                            # values is not optional
    with pytest.raises(TypeError, match="values"):
        api.group_by_sum(k, np.array(["a", "b", "c", "d"]))
    with pytest.raises(TypeError, match="keys"):
        api.group_by_count(np.array(["a", "b", "c", "d"]))
    with pytest.raises(TypeError, match="keys"):
        api.unique(np.array(["a", "b"]), return_index=True)
    with pytest.raises(TypeError, match="signed must be None, True or False"):
        api.group_by_min(k, k, signed=1.0)
    with pytest.raises(TypeError, match="signed must be None, True or False"):
        api.group_by_max(k, k, signed="yes")
    for fn in (api.group_by_min, api.group_by_max):                    # a float column has no integer order to compare by
        for signed in (None, True, False):
            with pytest.raises(TypeError, match="values must be integers"):
                fn(k, k.astype(np.float64), signed=signed)


def test_numpy_reference_on_a_hand_written_case():
    keys = np.array([7, 5, 7, 2**64 - 1, 0, 7, 2**64 - 1, 9], dtype=np.uint64)
    vals = np.array([1, 4, 2**63, 2**63, 32, 2**63 + 3, 2**64 - 1, 0], dtype=np.uint64)
    r = ref_group_by(keys, vals)
    assert r["keys"].tolist() == [0, 5, 7, 9, 2**64 - 1]
    assert r["first"].tolist() == [4, 1, 0, 7, 3] and r["count"].tolist() == [1, 1, 3, 1, 2]
    assert r["sum"].dtype == np.uint64 and r["sum"].tolist() == [32, 4, 4, 0, 2**63 - 1]          # 1 + 2^63 + 2^63 + 3 wraps to 4
    assert r["min_u"].tolist() == [32, 4, 1, 0, 2**63] and r["max_u"].tolist() == [32, 4, 2**63 + 3, 0, 2**64 - 1]
    assert r["min_s"].tolist() == [32, 4, -2**63, 0, -2**63] and r["max_s"].tolist() == [32, 4, 1, 0, -1]
    r = ref_group_by(np.empty(0, np.uint64), np.empty(0, np.uint64))
    assert all(a.size == 0 for a in r.values())


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fj():
    import flash_join
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_device_count() >= 1, "no HIP device: the product path must not silently fall back"
    assert flash_join.initialize() is None
    return flash_join


EXTREMES = np.array([2**63, 2**63 - 1, 0, 2**64 - 1], dtype=np.uint64)      # INT64_MIN, INT64_MAX, 0, UINT64_MAX (= -1)


def _values_for(rng, keys):
    """random full-width words (the sums wrap), never 0 - except the planted extremes: INT64_MIN, INT64_MAX, 0 and 2^64 - 1 on rows of
    the most frequent key and, one each, on other rows"""
    n = keys.size
    v = rng.integers(0, 2**64, size=n, dtype=np.uint64)
    v[v == 0] = np.uint64(1)
    if n >= 8:
        uk, cnt = np.unique(keys, return_counts=True)
        rows = np.flatnonzero(keys == uk[np.argmax(cnt)])[:4]
        v[rows] = EXTREMES[:rows.size]
        v[rng.choice(n, 4, replace=False)] = EXTREMES
    return v


class Ref:
    """a relation and its reference, computed once"""
    def __init__(self, keys, rng):
        self.keys = np.ascontiguousarray(keys, dtype=np.uint64)
        self.vals = _values_for(rng, self.keys)
        self.r = ref_group_by(self.keys, self.vals)
        self.g = self.r["keys"].size
        self._dev = None

    def args(self, device):
        if not device:
            return self.keys, self.vals
        if self._dev is None:
            import torch
            self._dev = tuple(torch.from_numpy(a.view(np.int64)).cuda() for a in (self.keys, self.vals))
        return self._dev


def _host(a, device):
    if device:
        assert a.is_cuda and str(a.dtype) == "torch.int64", a.dtype
        return a.cpu().numpy()
    assert isinstance(a, np.ndarray), type(a)
    return a


# form, ALGO flags, takes the value column, key of the reference
FORMS = [("count", 0, False, "count"), ("sum", 0, True, "sum"), ("min_u", MIN, True, "min_u"), ("min_s", MIN | SIGNED, True, "min_s"),
         ("max_u", MAX, True, "max_u"), ("max_s", MAX | SIGNED, True, "max_s"), ("first_index", ROW_IDS, False, "first")]


def _check(ref, what, g, gk, gv, want, device):
    """one result against the reference: sorted by key, exact"""
    r = ref.r
    assert isinstance(g, int) and g == ref.g, (what, g, ref.g)
    gk = _host(gk, device).view(np.uint64)
    assert gk.shape == (g,), (what, gk.shape)
    order = np.argsort(gk, kind="stable")
    assert np.array_equal(gk[order], r["keys"]), f"{what}: the distinct keys"
    if want is None:
        assert gv is None
        return
    gv = _host(gv, device)
    assert gv.shape == (g,) and gv.dtype.itemsize == 8, (what, gv.shape, gv.dtype)
    assert np.array_equal(gv[order].view(r[want].dtype), r[want]), f"{what}: {want}"


def check_all_forms(fj, ref, device, base=0, after=None):
    """count, sum, the four min / max forms, first occurrences, distinct_count and unique with each extra.  base = 0: through the
    public functions; another base value (ALGO_SCALAR, ALGO_RADIX): through api._group_by, which they all call; after(name, timings)"""
    from flash_hash_join_amd import api
    keys, vals = ref.args(device)
    note = (lambda fn: after(fn, fj.last_timings())) if after else (lambda fn: None)
    for name, flags, takes_vals, want in FORMS:
        if base:
            g, sec, gk, gv = api._group_by(keys, vals if takes_vals else None, base | flags)
        elif name == "count":
            g, sec, gk, gv = fj.group_by_count(keys)
        elif name == "sum":
            g, sec, gk, gv = fj.group_by_sum(keys, vals)
        elif name == "first_index":
            g, sec, gk, gv = fj.unique(keys, return_index=True)
        else:
            g, sec, gk, gv = (fj.group_by_min if flags & MIN else fj.group_by_max)(keys, vals, signed=bool(flags & SIGNED))
        note(name)
        assert isinstance(sec, float)
        _check(ref, name, g, gk, gv, want, device)
    if base:
        g, sec, gk, gv = api._group_by(keys, None, base, materialize=False)
        assert gk is None and gv is None
    else:
        g, sec = fj.distinct_count(keys)
    note("distinct_count")
    assert g == ref.g and isinstance(g, int) and isinstance(sec, float)
    if base:
        g, sec, gk, gv = api._group_by(keys, None, base, want_vals=False)
        note("unique")
        _check(ref, "keys alone", g, gk, gv, None, device)
        return
    g, sec, gk = fj.unique(keys)
    note("unique")
    _check(ref, "unique", g, gk, None, None, device)
    g, sec, gk, cnt = fj.unique(keys, return_counts=True)
    note("unique(return_counts)")
    _check(ref, "unique(return_counts)", g, gk, cnt, "count", device)
    g, sec, gk, idx, cnt = fj.unique(keys, return_index=True, return_counts=True)
    note("unique(return_index, return_counts)")
    _check(ref, "unique(both): first_index", g, gk, idx, "first", device)
    _check(ref, "unique(both): counts aligned by key", g, gk, cnt, "count", device)


def _dup_keys(rng, n, distinct):
    pool = np.unique(rng.integers(0, 2**64, size=distinct + 64, dtype=np.uint64))[:distinct]
    rng.shuffle(pool)
    keys = np.concatenate([pool, rng.choice(pool, n - distinct)]) if n > distinct else pool[:n].copy()
    rng.shuffle(keys)
    return keys


def _hot_keys(rng):
    single = np.unique(rng.integers(0, 2**64, size=100_100, dtype=np.uint64))[:100_001]
    keys = np.concatenate([np.full(100_000, single[-1]), single[:100_000]])
    rng.shuffle(keys)                                                  # the hot key's rows are spread through the input
    return keys


def _special_keys(rng, background, bits):
    """the hash domain's special keys (tests/keymix.py: the marker, the wide kernel's filler and their neighbours, raw 0 and raw
    2^64 - 1), three copies each, among `background` random rows"""
    _, raw = keymix.special_raw_keys(bits)
    keys = np.concatenate([np.repeat(raw, 3), rng.integers(0, 2**64, size=background, dtype=np.uint64)])
    rng.shuffle(keys)
    return keys


PASSES_0, PASSES_1, PASSES_2, PASSES_3 = (lambda p: p == 0), (lambda p: p == 1), (lambda p: p == 2), (lambda p: p == 3)
CASES = {   # id: (keys builder, plan_target_keys, passes, containers)
    "zero_pass": (lambda rng: _dup_keys(rng, 1000, 37), 4096, PASSES_0, (False, True)),
    "single_row": (lambda rng: np.array([0x1234567890ABCDEF], dtype=np.uint64), 4096, PASSES_0, (False, True)),
    "n4097": (lambda rng: _dup_keys(rng, 4097, 1500), 4096, PASSES_1, (False, True)),
    "one_pass": (lambda rng: _dup_keys(rng, 200_003, 50_000), 4096, PASSES_1, (False, True)),
    "all_distinct_zero_pass": (lambda rng: _dup_keys(rng, 3000, 3000), 4096, PASSES_0, (False, True)),
    "all_distinct": (lambda rng: _dup_keys(rng, 20_011, 20_011), 4096, PASSES_1, (False, True)),
    "all_equal": (lambda rng: np.full(100_003, 0xDEADBEEF12345678, dtype=np.uint64), 4096, PASSES_1, (False, True)),
    "all_equal_zero_pass": (lambda rng: np.full(777, 42, dtype=np.uint64), 4096, PASSES_0, (True,)),
    "two_pass_10_bits": (lambda rng: _dup_keys(rng, 200_003, 50_000), 256, PASSES_2, (True,)),
    "two_pass_14_bits": (lambda rng: _dup_keys(rng, 200_003, 50_000), 16, PASSES_2, (False, True)),
    "three_pass": (lambda rng: _dup_keys(rng, 16 * 2**18 + 1, 1_000_000), 16, PASSES_3, (True,)),
    "hot_key": (_hot_keys, 4096, PASSES_1, (False, True)),
    "special_keys_zero_pass": (lambda rng: _special_keys(rng, 500, 0), 4096, PASSES_0, (False, True)),
    "special_keys_one_pass": (lambda rng: _special_keys(rng, 20_000, 5), 4096, PASSES_1, (False, True)),
}
PARITY = [(cid, device) for cid, c in CASES.items() for device in c[3]]


@functools.lru_cache(maxsize=None)
def _ref_case(cid):
    rng = np.random.default_rng(sorted(CASES).index(cid) + 100)
    return Ref(CASES[cid][0](rng), rng)


@pytest.mark.gpu
@pytest.mark.parametrize("cid,device", PARITY, ids=[f"{c}-{'device' if d else 'numpy'}" for c, d in PARITY])
def test_parity_with_the_numpy_reference(fj, cid, device):
    _, target, passes, _ = CASES[cid]
    ref = _ref_case(cid)
    if cid.startswith("special_keys"):
        for k in (keymix.EMPTY_RAW, keymix.FILLER_RAW, 0, 2**64 - 1):
            i = int(np.searchsorted(ref.r["keys"], np.uint64(k)))
            # (three copies each; raw 0 six: it is also the raw key of the mixed word 0)
            assert ref.r["keys"][i] == np.uint64(k) and ref.r["count"][i] in (3, 6) and ref.r["sum"][i] != 0
    if cid == "hot_key":
        assert ref.g == 100_001 and ref.r["count"].max() == 100_000
    if cid.startswith("all_distinct"):
        assert ref.g == ref.keys.size

    def after(fn, lt):
        assert lt["path"] == 0 and lt["fell_back"] == 0 and passes(lt["passes"]) and lt["emit_ms"] == 0.0, (fn, lt)
        assert lt["join_ms"] == lt["probe_phase_ms"], (fn, lt)
    fj.set_option("plan_target_keys", target)
    try:
        check_all_forms(fj, ref, device, after=after)
    finally:
        fj.set_option("plan_target_keys", 4096)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_empty_input(fj, device):
    ref = Ref(np.empty(0, np.uint64), np.random.default_rng(0))
    check_all_forms(fj, ref, device)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["one_pass", "special_keys_one_pass", "all_equal", "single_row"])
@pytest.mark.parametrize("option,base", [("scalar_hbm_table", 1), ("radix_threshold", 0)])
def test_hbm_table_form(fj, option, base, cid):
    """FJ_ALGO_SCALAR under scalar_hbm_table = 1 and FJ_ALGO_ADAPTIVE below radix_threshold: the global table from the start.  There
    the out-of-band key is raw 2^64 - 1; the special-key case holds it three times beside the LDS tables' marker"""
    ref = _ref_case(cid)

    def after(fn, lt):
        assert lt["path"] == 1 and lt["fell_back"] == 0 and lt["passes"] == 0 and lt["emit_ms"] == 0.0, (fn, lt)
        hbm_timings.check_hbm_form(lt, fn)
    fj.set_option(option, 1 if base else ref.keys.size + 1)
    try:
        for device in (False, True):
            check_all_forms(fj, ref, device, base=base, after=after)
    finally:
        fj.set_option(option, 0)


@functools.lru_cache(maxsize=1)
def _oversized_case():
    """9000 distinct keys whose mixed words carry the radix digits of ONE final partition of the 5-bit plan that 29 000 rows take
    (partition 19: the top five bits of hash word 1), each once, among 20 000 background rows"""
    rng = np.random.default_rng(77)
    low = np.unique(rng.integers(0, 2**59, size=9100, dtype=np.uint64))[:9000]
    one = keymix.unmix((np.uint64(19) << np.uint64(59)) | low)
    assert np.unique(one).size == 9000 and np.all(keymix.hash_w1(one) >> np.uint32(27) == 19)
    keys = np.concatenate([one, rng.integers(0, 2**64, size=20_000, dtype=np.uint64)])
    rng.shuffle(keys)
    return Ref(keys, rng)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_a_partition_beyond_the_lds_table_falls_back_to_the_hbm_table(fj, device):
    """more distinct keys in one partition than the 8192-slot table takes: the whole call runs again on the HBM table from cursor 0
    (fell_back == 1), over whatever the other partitions wrote before"""
    from flash_hash_join_amd import _lib
    L = _lib.load()
    ref = _oversized_case()
    for k in ref.keys[:50]:
        assert L.fj_key_unmix64(L.fj_key_mix64(int(k))) == int(k) and int(keymix.mix(np.array([k]))[0]) == L.fj_key_mix64(int(k))

    def after(fn, lt):
        assert lt["fell_back"] == 1 and lt["path"] == 1 and lt["emit_ms"] == 0.0, (fn, lt)
        hbm_timings.check_hbm_form(lt, fn)
    check_all_forms(fj, ref, device, after=after)


@pytest.mark.gpu
@pytest.mark.parametrize("base", [2, 1], ids=["partitioned", "hbm_table"])
@pytest.mark.parametrize("cid", ["all_distinct", "one_pass"])
def test_guard_words_behind_the_capacity_stay_intact(fj, base, cid):
    """fj_join_device on buffers of nb + 16 words with a sentinel in the last 16 and out_capacity = nb: rows [0, g) are the result
    (all nb rows when every key is distinct), nothing at or beyond word nb is touched"""
    import threading
    import torch
    from flash_hash_join_amd import _lib, api
    L = _lib.load()
    ref = _ref_case(cid)
    keys, vals = ref.args(True)
    nb = ref.keys.size
    ctx = api.context(0)
    stream = torch.cuda.current_stream(0).cuda_stream
    A5 = int(np.array(0xA5A5A5A5A5A5A5A5, dtype=np.uint64).view(np.int64))
    if base == 1:
        fj.set_option("scalar_hbm_table", 1)
    try:
        for flags, want in ((0, "sum"), (MAX | SIGNED, "max_s"), (ROW_IDS, "first")):
            ok = torch.full((nb + 16,), A5, dtype=torch.int64, device="cuda")
            ov = torch.full((nb + 16,), A5, dtype=torch.int64, device="cuda")
            cnt = ctypes.c_uint64(0)
            t = _lib.FjTimings()
            with api._ctx_locks.setdefault(0, threading.RLock()):
                _lib.check(L.fj_join_device(ctx, base | GB | flags, 0, 1, keys.data_ptr(), vals.data_ptr(), nb, None, 0, stream, 64,
                                            ctypes.byref(cnt), ok.data_ptr(), ov.data_ptr(), nb, ctypes.byref(t)))
            assert t.path == (0 if base == 2 else 1) and t.emit_ms == 0.0 and t.fell_back == 0
            g = int(cnt.value)
            hk, hv = ok.cpu().numpy(), ov.cpu().numpy()
            assert np.all(hk[nb:] == A5) and np.all(hv[nb:] == A5), "a word at or beyond out_capacity was written"
            _check(ref, want, g, hk[:g], hv[:g], want, False)
    finally:
        fj.set_option("scalar_hbm_table", 0)


@pytest.mark.gpu
def test_the_same_context_reused(fj):
    """group_by_sum twice: the same result; a counting join afterwards: the oracle's count; a pending result is dropped by group-by"""
    import threading
    import torch
    from flash_hash_join_amd import _lib, api
    from oracle import oracle as O
    L = _lib.load()
    ref = _ref_case("one_pass")
    keys, vals = ref.args(True)
    for _ in range(2):
        g, _, gk, gs = fj.group_by_sum(keys, vals)
        _check(ref, "group_by_sum", g, gk, gs, "sum", True)
    rng = np.random.default_rng(3)
    bk = ref.r["keys"][:30_000].copy()
    bv = rng.integers(0, 2**64, size=bk.size, dtype=np.uint64)
    pk = np.concatenate([rng.choice(bk, 40_000), rng.integers(0, 2**64, size=40_000, dtype=np.uint64)])
    n, _ = fj.hash_join_count(*(torch.from_numpy(a.view(np.int64)).cuda() for a in (bk, bv, pk)))
    assert n == O.np_join(bk, bv, pk)
    dbk, dpk = (torch.from_numpy(a.view(np.int64)).cuda() for a in (bk, pk))
    ctx = api.context(0)
    stream = torch.cuda.current_stream(0).cuda_stream
    cnt = ctypes.c_uint64(0)
    out = torch.empty(pk.size, dtype=torch.int64, device="cuda")
    with api._ctx_locks.setdefault(0, threading.RLock()):
        # a materialising call without buffers counts and leaves its result pending; the group-by drops it
        _lib.check(L.fj_join_device(ctx, 2, 0, 1, dbk.data_ptr(), dbk.data_ptr(), bk.size, dpk.data_ptr(), pk.size, stream, 64, ctypes.byref(cnt), None, None, 0, None))
        assert int(cnt.value) == n
        g, _, gk, gs = fj.group_by_sum(keys, vals)
        assert L.fj_emit_pairs(ctx, out.data_ptr(), out.data_ptr(), pk.size, stream, None) != 0, "a result was left pending"
        assert "no counted materialising join is pending" in _lib.last_error()
    _check(ref, "group_by_sum after a pending result", g, gk, gs, "sum", True)


@pytest.mark.gpu
def test_host_entry_returns_exactly_g_rows_and_drops_a_null_output(fj):
    """fj_join_host on NumPy arrays: *out_keys / *out_vals are arrays of exactly g rows; NULL for either pointer drops that output"""
    from flash_hash_join_amd import _lib
    L = _lib.load()
    ref = _ref_case("one_pass")
    k, v = ref.keys, ref.vals
    take = lambda p, g: np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint64)), shape=(g,)).copy()
    for want_keys, want_vals in ((True, True), (True, False), (False, True), (False, False)):
        cnt, sec = ctypes.c_uint64(0), ctypes.c_double(0)
        ok, ov = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(L.fj_join_host(GB | 2, 0, 1, k.ctypes.data, v.ctypes.data, k.size, None, 0, ctypes.byref(cnt), ctypes.byref(sec),
                                  ctypes.byref(ok) if want_keys else None, ctypes.byref(ov) if want_vals else None))
        try:
            g = int(cnt.value)
            assert g == ref.g and bool(ok.value) == want_keys and bool(ov.value) == want_vals
            if want_keys and want_vals:
                _check(ref, "host sum", g, take(ok, g), take(ov, g), "sum", False)
            elif want_keys:
                _check(ref, "host keys alone", g, take(ok, g), None, None, False)
            elif want_vals:
                assert np.array_equal(np.sort(take(ov, g)), np.sort(ref.r["sum"]))      # (no keys to align by)
        finally:
            L.fj_free_host(ok)
            L.fj_free_host(ov)
    cnt = ctypes.c_uint64(0)
    _lib.check(L.fj_join_host(GB, 0, 0, k.ctypes.data, None, k.size, None, 0, ctypes.byref(cnt), None, None, None))
    assert int(cnt.value) == ref.g
