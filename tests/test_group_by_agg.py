"""Group-by with count, sum, min and max of a column in ONE call (FJ_ALGO_GROUP_BY | FJ_ALGO_AGG_ALL, csrc/fj_groupby_multi.hip;
api.group_by_agg) on an MI355X: every column of one call against a NumPy reference, aligned with that call's keys.

References (tests/test_group_by_agg_cpu.py, checked there on a hand-written case): integers - np.unique plus np.add.at /
np.minimum.at / np.maximum.at over the uint64 and int64 words, both sides sorted by key, exact equality; floats - the two value domains
and the acceptance rule of tests/test_float_aggregates.py: "exact" values (multiples of 2^-10 below 2^10: every partial sum is
representable, so any order of addition gives the same double) must equal the reference, "inexact" sums lie within
n_g * 2^-52 * sum(|v|) of math.fsum, minima and maxima are exact.  Nothing is compared with the library itself.

Plans: this form aims at 2048 rows per partition (half of its 4096-slot table), so 2048 rows are the largest flat plan, 2049 the first
one-pass plan (5 bits), 200 003 rows take 7 bits in one pass and, under plan_target_keys = 16, 14 bits in two."""
import ctypes
import functools
import math
import threading

import numpy as np
import pytest

import hbm_timings
import keymix
from test_float_aggregates import exact_values, extreme_values, inexact_values
from test_group_by import _dup_keys, _hot_keys, _special_keys, _values_for
from test_group_by_agg_cpu import ref_group_by_agg, ref_group_by_agg_float

SIGNED, GB, FLOAT, ALL = 0x10000, 0x40000, 0x2000000, 0x4000000
KINDS = ("unsigned", "signed", "float")
TS, LIMIT = 4096, 3840                                                   # the table of fj_group_by_all_kernel


@pytest.fixture(scope="module")
def fj():
    import flash_join
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_device_count() >= 1, "no HIP device: the product path must not silently fall back"
    assert flash_join.initialize() is None
    for name, value in (("plan_target_keys", 4096), ("scalar_hbm_table", 0), ("radix_threshold", 0)):
        assert flash_join.get_option(name) == value, f"option {name} is not at its default"
    return flash_join


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64 else np.ascontiguousarray(a)).cuda()


class Ref:
    """a relation, an integer and an "exact" float value column, and their references - each computed once and never changed"""
    def __init__(self, keys, rng, fvals=None):
        self.keys = np.ascontiguousarray(keys, dtype=np.uint64)
        self.vals = _values_for(rng, self.keys)
        self.fvals = exact_values(int(rng.integers(1 << 30)), self.keys.size) if fvals is None else fvals
        self.r = ref_group_by_agg(self.keys, self.vals)
        self.g = self.r["keys"].size
        self._f = None
        self._dev = {}

    @property
    def f(self):
        if self._f is None:
            self._f = ref_group_by_agg_float(self.keys, self.fvals)
        return self._f

    def dev(self, name):
        if name not in self._dev:
            self._dev[name] = _dev(getattr(self, name))
        return self._dev[name]


def call(fj, ref, kind, device, base=0, **kw):
    """group_by_agg (base 0) or api._group_by_all (ALGO_SCALAR / ALGO_RADIX) on the relation in its container; the signedness comes
    from the container where it can: a NumPy uint64 / int64 column unsigned / signed, a device tensor (int64) signed unless told"""
    from flash_hash_join_amd import api
    keys = ref.dev("keys") if device else ref.keys
    if kind == "float":
        vals, args = (ref.dev("fvals") if device else ref.fvals), dict(float64=True)
    elif device:
        vals, args = ref.dev("vals"), dict(signed=(kind == "signed"))
    else:
        vals, args = (ref.vals if kind == "unsigned" else ref.vals.view(np.int64)), dict()
    if base:
        if kind == "float":
            vals = api._float_words("test", "values", vals)
        g, sec, gk, planes = api._group_by_all(keys, vals, base | {"unsigned": 0, "signed": SIGNED, "float": FLOAT}[kind])
        cols = [planes[0], planes[1], planes[2], planes[3]]
        if kind == "float":
            cols[1:] = [api._as_float64(c) for c in cols[1:]]
        return (g, sec, gk, *cols)
    return fj.group_by_agg(keys, vals, **args, **kw)


def _host(a, device, dtype):
    if device:
        assert a.is_cuda and str(a.dtype) == "torch." + dtype, (a.dtype, dtype)
        return a.cpu().numpy()
    assert isinstance(a, np.ndarray) and str(a.dtype) == dtype, (a.dtype, dtype)
    return a


def sorted_columns(out, device, dtypes, g_ref):
    """the columns of ONE call in the order of that call's sorted keys"""
    g, sec, gk = out[:3]
    assert isinstance(g, int) and isinstance(sec, float) and g == g_ref, (g, g_ref)
    gk = _host(gk, device, "int64" if device else "uint64").view(np.uint64)
    assert gk.shape == (g,) and len(out) == 3 + len(dtypes)
    order = np.argsort(gk, kind="stable")
    cols = []
    for col, dt in zip(out[3:], dtypes):
        col = _host(col, device, dt)
        assert col.shape == (g,), col.shape
        cols.append(col[order])
    return gk[order], cols


def check(ref, kind, out, device, public=True, sums_exact=True):
    """all four columns of one call, aligned with its keys, against the reference"""
    if kind == "float":
        r = ref.f
        gk, (cnt, sm, mn, mx) = sorted_columns(out, device, ("int64", "float64", "float64", "float64"), ref.g)
        assert np.array_equal(gk, r["keys"]), "the distinct keys"
        assert np.array_equal(cnt, r["count"]), "count"
        assert bool(np.all(mn == r["min"])) and bool(np.all(mx == r["max"])), "float min / max"
        if sums_exact:
            assert bool(np.all(sm == r["sum"])), "float sum (exact domain)"
        else:
            err, bound = np.abs(sm - r["sum"]), r["count"] * 2.0**-52 * r["abs"]
            print(f"largest |got - fsum| / bound = {np.max(err / np.maximum(bound, 5e-324)):.3g}")
            assert np.all(err <= bound), "float sum (inexact domain)"
        return
    r = ref.r
    own = "uint64" if (kind == "unsigned" and not device and public) else "int64"       # a NumPy uint64 column compared unsigned keeps its dtype
    gk, (cnt, sm, mn, mx) = sorted_columns(out, device, ("int64", "int64", own, own), ref.g)
    sfx = "_u" if kind == "unsigned" else "_s"
    assert np.array_equal(gk, r["keys"]), "the distinct keys"
    assert np.array_equal(cnt, r["count"]), "count"
    assert np.array_equal(sm.view(np.uint64), r["sum"]), "sum"
    assert np.array_equal(mn.view(r["min" + sfx].dtype), r["min" + sfx]), "min" + sfx
    assert np.array_equal(mx.view(r["max" + sfx].dtype), r["max" + sfx]), "max" + sfx


def planned(fj, passes, fell_back=0, path=0):
    lt = fj.last_timings()
    assert lt["path"] == path and lt["fell_back"] == fell_back and lt["emit_ms"] == 0.0, lt
    if path == 1:
        hbm_timings.check_hbm_form(lt)
    if passes is not None:
        assert lt["passes"] == passes, lt
    assert lt["join_ms"] == lt["probe_phase_ms"], lt


CASES = {   # id: (keys builder, plan_target_keys, passes, containers)
    "zero_pass": (lambda rng: _dup_keys(rng, 1000, 37), 4096, 0, (False, True)),
    "single_row": (lambda rng: np.array([0x1234567890ABCDEF], dtype=np.uint64), 4096, 0, (False, True)),
    "n2048_all_distinct": (lambda rng: _dup_keys(rng, 2048, 2048), 4096, 0, (False, True)),
    "n2049": (lambda rng: _dup_keys(rng, 2049, 700), 4096, 1, (False, True)),
    "n4097": (lambda rng: _dup_keys(rng, 4097, 1500), 4096, 1, (False, True)),
    "one_pass": (lambda rng: _dup_keys(rng, 200_003, 50_000), 4096, 1, (False, True)),
    "all_distinct": (lambda rng: _dup_keys(rng, 20_011, 20_011), 4096, 1, (False, True)),
    "all_equal": (lambda rng: np.full(100_003, 0xDEADBEEF12345678, dtype=np.uint64), 4096, 1, (True,)),
    "two_pass": (lambda rng: _dup_keys(rng, 200_003, 50_000), 16, 2, (True,)),
    "hot_key": (_hot_keys, 4096, 1, (True,)),
    "special_keys_zero_pass": (lambda rng: _special_keys(rng, 500, 0), 4096, 0, (False, True)),
    "special_keys_one_pass": (lambda rng: _special_keys(rng, 20_000, 5), 4096, 1, (False, True)),
}
PARITY = [(cid, device) for cid, c in CASES.items() for device in c[3]]


@functools.lru_cache(maxsize=None)
def _ref_case(cid):
    rng = np.random.default_rng(sorted(CASES).index(cid) + 900)
    return Ref(CASES[cid][0](rng), rng)


@pytest.mark.gpu
@pytest.mark.parametrize("cid,device", PARITY, ids=[f"{c}-{'device' if d else 'numpy'}" for c, d in PARITY])
def test_four_aggregates_of_one_call_match_the_numpy_reference(fj, cid, device):
    _, target, passes, _ = CASES[cid]
    ref = _ref_case(cid)
    if cid.startswith("special_keys"):
        for k in (keymix.EMPTY_RAW, keymix.FILLER_RAW, 0, 2**64 - 1):
            i = int(np.searchsorted(ref.r["keys"], np.uint64(k)))
            assert ref.r["keys"][i] == np.uint64(k) and ref.r["count"][i] in (3, 6) and ref.r["sum"][i] != 0
    if cid == "hot_key":
        assert ref.g == 100_001 and ref.r["count"].max() == 100_000
    if cid in ("all_distinct", "n2048_all_distinct"):
        assert ref.g == ref.keys.size
    fj.set_option("plan_target_keys", target)
    try:
        for kind in KINDS:
            out = call(fj, ref, kind, device)
            planned(fj, passes)
            check(ref, kind, out, device)
    finally:
        fj.set_option("plan_target_keys", 4096)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_empty_input(fj, device):
    ref = Ref(np.empty(0, np.uint64), np.random.default_rng(0))
    for kind in KINDS:
        check(ref, kind, call(fj, ref, kind, device), device)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_inexact_float_sums_within_the_bound_of_a_sum_in_any_order(fj, device):
    rng = np.random.default_rng(41)
    keys = _dup_keys(rng, 60_001, 9_000)
    ref = Ref(keys, rng, fvals=inexact_values(12, keys.size))
    check(ref, "float", call(fj, ref, "float", device), device, sums_exact=False)
    planned(fj, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["zero", "one_pass", "hbm"])
def test_float_min_max_on_extreme_values(fj, cid):
    """+-inf, +-0.0, denormals, +-max: the minima and maxima are exact (the sums, where +inf meets -inf, are not looked at)"""
    rng = np.random.default_rng(43)
    keys = _dup_keys(rng, 1500 if cid == "zero" else 30_011, 200 if cid == "zero" else 3_000)
    ref = Ref(keys, rng, fvals=extreme_values(13, keys.size))
    r = ref_group_by_agg_float(ref.keys, np.zeros(keys.size))                      # (keys and counts; fsum of inf - inf is an error)
    mn, mx = np.full(ref.g, np.inf), np.full(ref.g, -np.inf)
    inv = np.searchsorted(r["keys"], ref.keys)
    np.minimum.at(mn, inv, ref.fvals); np.maximum.at(mx, inv, ref.fvals)
    fj.set_option("scalar_hbm_table", 1 if cid == "hbm" else 0)
    try:
        for device in (False, True):
            out = call(fj, ref, "float", device, base=1 if cid == "hbm" else 0)
            gk, (cnt, sm, gmn, gmx) = sorted_columns(out, device, ("int64", "float64", "float64", "float64"), ref.g)
            assert np.array_equal(gk, r["keys"]) and np.array_equal(cnt, r["count"])
            assert bool(np.all(gmn == mn)) and bool(np.all(gmx == mx))
    finally:
        fj.set_option("scalar_hbm_table", 0)


# ---- the table's edge and its collisions, crafted (tests/keymix.py) -------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _edge_case(n):
    """n distinct keys in ONE final partition (19) of the 5-bit one-pass plan that n + 5000 rows take at 2048 rows per partition, their
    home slots spread by random hash words 2, every fourth key twice, among 5000 background rows of the other 31 partitions"""
    rng = np.random.default_rng(n)
    one = keymix.craft(5, 19, rng.integers(0, 2**32, size=n, dtype=np.uint64), n, seed=n)
    assert np.unique(one).size == n and np.all(keymix.partition_of(one, 5) == 19)
    bg = rng.integers(0, 2**64, size=6000, dtype=np.uint64)
    bg = bg[keymix.partition_of(bg, 5) != 19][:5000 - one[::4].size]
    keys = np.concatenate([one, one[::4], bg])
    assert 2048 < keys.size <= 5 * 2048                                          # 3 radix bits asked for: the plan's minimum of 5
    rng.shuffle(keys)
    return Ref(keys, rng)


@pytest.mark.gpu
@pytest.mark.parametrize("n,fell_back", [(LIMIT, 0), (LIMIT + 1, 1)], ids=["3840_keys_stay", "3841_keys_fall_back"])
def test_the_edge_of_the_lds_table(fj, n, fell_back):
    ref = _edge_case(n)
    for kind in KINDS:
        for device in (False, True):
            out = call(fj, ref, kind, device)
            lt = fj.last_timings()
            assert lt["fell_back"] == fell_back and lt["path"] == fell_back and lt["emit_ms"] == 0.0, (kind, device, lt)
            if fell_back:
                hbm_timings.check_hbm_form(lt, (kind, device))
            else:
                assert lt["passes"] == 1 and lt["radix_bits"] == 5, lt
            check(ref, kind, out, device)


@functools.lru_cache(maxsize=2)
def _wrap_case(zero_pass):
    """300 keys whose home slot is the table's LAST (hash word 2 = 0xFFF | i << 12): one cluster that wraps past slot 4095 into
    slots 0 .. 298; three copies each, in the last partition of a one-pass plan among background rows, or alone on the flat plan"""
    rng = np.random.default_rng(5 + zero_pass)
    w2 = np.uint64(TS - 1) | (np.arange(300, dtype=np.uint64) << np.uint64(12))
    one = keymix.craft(0, 0, w2, 300, seed=3) if zero_pass else keymix.craft(5, 31, w2, 300, seed=3)
    assert np.all((keymix.mix(one) & np.uint64(TS - 1)) == np.uint64(TS - 1))
    keys = np.concatenate([np.repeat(one, 3), rng.integers(0, 2**64, size=1000 if zero_pass else 6000, dtype=np.uint64)])
    rng.shuffle(keys)
    return Ref(keys, rng)


@pytest.mark.gpu
@pytest.mark.parametrize("zero_pass", [False, True], ids=["one_pass", "zero_pass"])
def test_a_cluster_that_wraps_past_the_last_slot(fj, zero_pass):
    ref = _wrap_case(zero_pass)
    for kind in KINDS:
        out = call(fj, ref, kind, True)
        planned(fj, 0 if zero_pass else 1)
        check(ref, kind, out, True)


# ---- the HBM-table form -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["one_pass", "special_keys_one_pass", "single_row"])
def test_hbm_table_form(fj, cid):
    """FJ_ALGO_SCALAR under scalar_hbm_table = 1: the global table from the start, four typed global atomics per row.  There the
    out-of-band key is raw 2^64 - 1; the special-key case holds it three times"""
    ref = _ref_case(cid)
    fj.set_option("scalar_hbm_table", 1)
    try:
        for kind in KINDS:
            for device in (False, True):
                out = call(fj, ref, kind, device, base=1)
                planned(fj, 0, path=1)
                check(ref, kind, out, device, public=False)
    finally:
        fj.set_option("scalar_hbm_table", 0)


@pytest.mark.gpu
def test_adaptive_below_the_radix_threshold_takes_the_hbm_table(fj):
    ref = _ref_case("n4097")
    fj.set_option("radix_threshold", ref.keys.size + 1)
    try:
        for kind in KINDS:
            out = call(fj, ref, kind, True)
            planned(fj, 0, path=1)
            check(ref, kind, out, True)
    finally:
        fj.set_option("radix_threshold", 0)


# ---- max_groups ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["zero_pass", "one_pass"])
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_max_groups_bounds_the_buffers_and_a_larger_result_is_an_error(fj, cid, device):
    ref = _ref_case(cid)
    g = ref.g
    check(ref, "signed", call(fj, ref, "signed", device, max_groups=g), device)
    check(ref, "float", call(fj, ref, "float", device, max_groups=g + 7), device)
    with pytest.raises(ValueError, match=rf"g = {g}\b"):
        call(fj, ref, "unsigned", device, max_groups=g - 1)
    with pytest.raises(ValueError, match=rf"g = {g}\b"):
        call(fj, ref, "float", device, max_groups=1)
    check(ref, "unsigned", call(fj, ref, "unsigned", device, max_groups=g), device)      # the context is still usable
    check(ref, "unsigned", call(fj, ref, "unsigned", device), device)


@pytest.mark.gpu
def test_max_groups_on_the_hbm_table(fj):
    ref = _ref_case("n4097")
    fj.set_option("radix_threshold", ref.keys.size + 1)
    try:
        with pytest.raises(ValueError, match=rf"g = {ref.g}\b"):
            call(fj, ref, "signed", True, max_groups=ref.g - 1)
        out = call(fj, ref, "signed", True, max_groups=ref.g)
        planned(fj, 0, path=1)
        check(ref, "signed", out, True)
    finally:
        fj.set_option("radix_threshold", 0)


@pytest.mark.gpu
def test_max_groups_of_one_on_a_relation_of_one_key(fj):
    ref = _ref_case("all_equal")
    for device in (False, True):
        for kind in KINDS:
            out = call(fj, ref, kind, device, max_groups=1)
            assert out[0] == 1
            check(ref, kind, out, device)


# ---- the C ABI: planes at stride out_capacity, nothing behind them ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("base", [2, 1], ids=["partitioned", "hbm_table"])
def test_guard_words_behind_the_capacity_stay_intact(fj, base):
    """fj_join_device with out_capacity = g < nb on buffers with a sentinel tail: the result is complete, plane j starts at word
    j * out_capacity, and nothing at or beyond word out_capacity of the keys or word 4 * out_capacity of the planes is touched -
    nor when the capacity is below g, where the call fails after the device work with an error that states g and the capacity"""
    import torch
    from flash_hash_join_amd import _lib, api
    L = _lib.load()
    ref = _ref_case("one_pass")
    keys, vals = ref.dev("keys"), ref.dev("vals")
    nb, g = ref.keys.size, ref.g
    ctx = api.context(0)
    stream = torch.cuda.current_stream(0).cuda_stream
    A5 = int(np.array(0xA5A5A5A5A5A5A5A5, dtype=np.uint64).view(np.int64))
    if base == 1:
        fj.set_option("scalar_hbm_table", 1)
    try:
        for cap in (g, g - 1000, 1):
            assert cap < nb
            ok = torch.full((cap + 64,), A5, dtype=torch.int64, device="cuda")
            ov = torch.full((4 * cap + 64,), A5, dtype=torch.int64, device="cuda")
            cnt = ctypes.c_uint64(0)
            t = _lib.FjTimings()
            with api._ctx_locks.setdefault(0, threading.RLock()):
                rc = L.fj_join_device(ctx, base | GB | ALL | SIGNED, 0, 1, keys.data_ptr(), vals.data_ptr(), nb, None, 0, stream, 64,
                                      ctypes.byref(cnt), ok.data_ptr(), ov.data_ptr(), cap, ctypes.byref(t))
                err = _lib.last_error()
            torch.cuda.synchronize()
            hk, hv = ok.cpu().numpy(), ov.cpu().numpy()
            assert np.all(hk[cap:] == A5) and np.all(hv[4 * cap:] == A5), "a word at or beyond the capacity was written"
            if cap < g:
                assert rc != 0 and str(g) in err and str(cap) in err and int(cnt.value) == g, err
                continue
            assert rc == 0 and int(cnt.value) == g and t.path == (0 if base == 2 else 1) and t.fell_back == 0, err
            check(ref, "signed", (g, 0.0, hk[:g].view(np.uint64), *(hv[j * cap:j * cap + g] for j in range(4))), False, public=False)
    finally:
        fj.set_option("scalar_hbm_table", 0)


@pytest.mark.gpu
def test_host_entry_returns_four_planes_of_exactly_g_words(fj):
    from flash_hash_join_amd import _lib
    L = _lib.load()
    ref = _ref_case("n4097")
    k, v, g = ref.keys, ref.vals, ref.g
    cnt, sec = ctypes.c_uint64(0), ctypes.c_double(0)
    ok, ov = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(L.fj_join_host(GB | ALL | 2, 0, 1, k.ctypes.data, v.ctypes.data, k.size, None, 0, ctypes.byref(cnt), ctypes.byref(sec),
                              ctypes.byref(ok), ctypes.byref(ov)))
    try:
        assert int(cnt.value) == g
        take = lambda p, n: np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint64)), shape=(n,)).copy()
        hk, hv = take(ok, g), take(ov, 4 * g).view(np.int64)
    finally:
        L.fj_free_host(ok)
        L.fj_free_host(ov)
    check(ref, "unsigned", (g, 0.0, hk, *(hv[j * g:(j + 1) * g] for j in range(4))), False, public=False)


# ---- aggs: subsets, orders, the mean ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_aggs_subsets_and_orders(fj, device):
    ref = _ref_case("n4097")
    out = call(fj, ref, "signed", device, aggs=("max", "count"))
    gk, (mx, cnt) = sorted_columns(out, device, ("int64", "int64"), ref.g)
    assert np.array_equal(gk, ref.r["keys"]) and np.array_equal(mx, ref.r["max_s"]) and np.array_equal(cnt, ref.r["count"])
    out = call(fj, ref, "unsigned", device, aggs=["min"])
    gk, (mn,) = sorted_columns(out, device, ("int64" if device else "uint64",), ref.g)
    assert np.array_equal(mn.view(np.uint64), ref.r["min_u"])
    out = call(fj, ref, "float", device, aggs=("mean",))
    gk, (mean,) = sorted_columns(out, device, ("float64",), ref.g)
    assert np.array_equal(gk, ref.f["keys"]) and bool(np.all(mean == ref.f["sum"] / ref.f["count"]))      # exact sums: one rounding, the division's
    out = call(fj, ref, "float", device, aggs=("sum", "mean", "max", "min", "count"))
    gk, (sm, mean, mx, mn, cnt) = sorted_columns(out, device, ("float64", "float64", "float64", "float64", "int64"), ref.g)
    assert all(bool(np.all(a == b)) for a, b in ((sm, ref.f["sum"]), (mean, ref.f["sum"] / ref.f["count"]), (mx, ref.f["max"]),
                                                 (mn, ref.f["min"]), (cnt, ref.f["count"])))


@pytest.mark.gpu
def test_the_same_context_serves_the_single_forms_afterwards(fj):
    """group_by_agg, then group_by_sum on the same context: both right - the wider plan and the four planes leave nothing behind"""
    ref = _ref_case("one_pass")
    check(ref, "signed", call(fj, ref, "signed", True), True)
    g, _, gk, gs = fj.group_by_sum(ref.dev("keys"), ref.dev("vals"))
    gk, gs = gk.cpu().numpy().view(np.uint64), gs.cpu().numpy().view(np.uint64)
    o = np.argsort(gk)
    assert g == ref.g and np.array_equal(gk[o], ref.r["keys"]) and np.array_equal(gs[o], ref.r["sum"])
    check(ref, "unsigned", call(fj, ref, "unsigned", True), True)
