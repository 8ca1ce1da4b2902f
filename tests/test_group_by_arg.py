"""The row that holds each group's minimum / maximum (FJ_ALGO_GROUP_BY | FJ_ALGO_AGG_ARG, csrc/fj_groupby_arg.hip; api.group_by_argmin,
api.group_by_argmax) on an MI355X: the row index and the extreme of every group against the NumPy reference of
tests/test_group_by_arg_cpu.py (a lexsort by key, value and position, checked there on a hand-written case), both sides sorted by key,
exact equality - ties go to the smallest row index, so the result is deterministic.  Nothing is compared with the library itself.

Plans: this form aims at 2048 rows per partition (half of its 4096-slot table), so 2048 rows are the largest flat plan, 2049 the first
one-pass plan (5 bits), 200 003 rows take 7 bits in one pass and, under plan_target_keys = 16, 14 bits in two.  The kernel streams a
partition in rounds of 4096 rows: a partition of up to 4096 rows resolves from registers, the 100 000 rows of a hot key stream twice."""
import ctypes
import functools
import threading

import numpy as np
import pytest

import hbm_timings
import keymix
from test_float_aggregates import exact_values, extreme_values
from test_group_by import _dup_keys, _hot_keys, _special_keys
from test_group_by_arg_cpu import KINDS, ref_group_by_arg

MIN, MAX, SIGNED, GB, FLOAT, ARG = 0x4000, 0x8000, 0x10000, 0x40000, 0x2000000, 0x8000000
TS, LIMIT = 4096, 3840                                                   # the table of fj_group_by_arg_kernel
IDENTITY = {("unsigned", False): 2**64 - 1, ("unsigned", True): 0, ("signed", False): 2**63 - 1, ("signed", True): 2**63,      # (words)
            ("float", False): np.inf, ("float", True): -np.inf}
FORMS = [(kind, is_max) for kind in KINDS for is_max in (False, True)]


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


class Rel:
    """a relation with an integer and a float value column; the references are computed once per form and never changed"""
    def __init__(self, keys, ivals, fvals):
        self.keys = np.ascontiguousarray(keys, dtype=np.uint64)
        self.ivals = np.ascontiguousarray(ivals, dtype=np.uint64)
        self.fvals = np.ascontiguousarray(fvals, dtype=np.float64)
        assert self.ivals.size == self.keys.size == self.fvals.size
        self.n = self.keys.size
        self._ref, self._dev = {}, {}

    def column(self, kind):
        return self.fvals if kind == "float" else self.ivals if kind == "unsigned" else self.ivals.view(np.int64)

    def ref(self, kind, is_max):
        if (kind, is_max) not in self._ref:
            self._ref[kind, is_max] = ref_group_by_arg(self.keys, self.column(kind), kind, is_max)
        return self._ref[kind, is_max]

    def dev(self, name):
        if name not in self._dev:
            self._dev[name] = _dev(getattr(self, name))
        return self._dev[name]


def random_rel(keys, rng):
    """random 64-bit words (no ties) and random doubles"""
    n = keys.size
    return Rel(keys, rng.integers(0, 2**64, size=n, dtype=np.uint64), rng.standard_normal(n) * 1e3)


def call(fj, rel, kind, is_max, device, base=0):
    """group_by_argmin / group_by_argmax with return_values=True (base 0) or api._group_by_arg (ALGO_SCALAR / ALGO_RADIX) on the relation in
    its container: (g, group_keys uint64, row_index int64, values in the column's dtype), as host arrays, dtypes and containers checked.
    The signedness comes from the container where it can: a NumPy uint64 / int64 column unsigned / signed, a device tensor told"""
    from flash_hash_join_amd import api
    keys = rel.dev("keys") if device else rel.keys
    if kind == "float":
        vals, args = (rel.dev("fvals") if device else rel.fvals), dict(float64=True)
    elif device:
        vals, args = rel.dev("ivals"), dict(signed=(kind == "signed"))
    else:
        vals, args = rel.column(kind), dict()
    if base:
        if kind == "float":
            vals = api._float_words("test", "values", vals)
        g, sec, gk, planes = api._group_by_arg(keys, vals, base | (MAX if is_max else MIN) | {"unsigned": 0, "signed": SIGNED, "float": FLOAT}[kind])
        idx, ext = planes[0], (api._as_float64(planes[1]) if kind == "float" else planes[1])
        vdt = "float64" if kind == "float" else "int64"
    else:
        g, sec, gk, idx, ext = (fj.group_by_argmax if is_max else fj.group_by_argmin)(keys, vals, return_values=True, **args)
        vdt = "float64" if kind == "float" else "uint64" if (kind == "unsigned" and not device) else "int64"
    assert isinstance(g, int) and isinstance(sec, float)
    out = []
    for a, dt in ((gk, "int64" if device else "uint64"), (idx, "int64"), (ext, vdt)):
        if device:
            assert a.is_cuda and str(a.dtype) == "torch." + dt, (a.dtype, dt)
            a = a.cpu().numpy()
        assert isinstance(a, np.ndarray) and str(a.dtype) == dt and a.shape == (g,), (a.dtype, dt, a.shape, g)
        out.append(a)
    return g, out[0].view(np.uint64), out[1], out[2]


def check(rel, kind, is_max, out, skip_keys=()):
    """g, the keys, the row indices exactly, and that the indices gather the keys and the values that came back"""
    r = rel.ref(kind, is_max)
    g, gk, idx, ext = out
    assert g == r["keys"].size, (g, r["keys"].size)
    o = np.argsort(gk, kind="stable")
    gk, idx, ext = gk[o], idx[o], ext[o]
    assert np.array_equal(gk, r["keys"]), "the distinct keys"
    keep = ~np.isin(gk, np.asarray(skip_keys, dtype=np.uint64))
    assert np.array_equal(idx[keep], r["index"][keep]), f"row_index: {int(np.sum(idx[keep] != r['index'][keep]))} of {g} differ"
    assert np.all((idx[keep] >= 0) & (idx[keep] < rel.n))
    assert np.array_equal(rel.keys[idx[keep]], gk[keep]), "keys[row_index] == group_keys"
    col = rel.column(kind)
    got, want = ext[keep].view(col.dtype), col[idx[keep]]
    if kind == "float":
        assert bool(np.all(got == want)), "values[row_index] == values (as numbers: which zero comes back is unspecified)"
    else:
        assert np.array_equal(got, want), "values[row_index] == values"
    return gk, idx, ext


def planned(fj, passes, fell_back=0, path=0):
    lt = fj.last_timings()
    assert lt["path"] == path and lt["fell_back"] == fell_back and lt["emit_ms"] == 0.0, lt
    if path == 1:
        hbm_timings.check_hbm_form(lt)
    if passes is not None:
        assert lt["passes"] == passes, lt
    assert lt["join_ms"] == lt["probe_phase_ms"], lt


CASES = {   # id: (keys builder, plan_target_keys, passes, containers) - the table of tests/test_group_by_agg.py
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
def _keys_of(cid):
    return CASES[cid][0](np.random.default_rng(sorted(CASES).index(cid) + 1900))


@functools.lru_cache(maxsize=None)
def _rel_case(cid):
    return random_rel(_keys_of(cid), np.random.default_rng(sorted(CASES).index(cid) + 2900))


def run_forms(fj, rel, device, passes, forms=FORMS, **kw):
    for kind, is_max in forms:
        out = call(fj, rel, kind, is_max, device, **kw)
        planned(fj, passes, path=1 if kw.get("base") == 1 else 0)
        check(rel, kind, is_max, out)


@pytest.mark.gpu
@pytest.mark.parametrize("cid,device", PARITY, ids=[f"{c}-{'device' if d else 'numpy'}" for c, d in PARITY])
def test_row_index_and_extreme_match_the_numpy_reference(fj, cid, device):
    """random 64-bit words and random doubles (no ties) on every plan; the special-key cases hold the marker, the filler, 0 and 2^64 - 1,
    whose value and position (the marker's: in the table's header) come back like any other key's"""
    _, target, passes, _ = CASES[cid]
    rel = _rel_case(cid)
    if cid.startswith("special_keys"):
        gk = rel.ref("unsigned", False)["keys"]
        for k in (keymix.EMPTY_RAW, keymix.FILLER_RAW, 0, 2**64 - 1):
            assert gk[int(np.searchsorted(gk, np.uint64(k)))] == np.uint64(k) and int(np.sum(rel.keys == np.uint64(k))) in (3, 6)
    if cid == "hot_key":
        assert rel.ref("unsigned", False)["keys"].size == 100_001
    fj.set_option("plan_target_keys", target)
    try:
        run_forms(fj, rel, device, passes)
    finally:
        fj.set_option("plan_target_keys", 4096)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_empty_input(fj, device):
    rel = random_rel(np.empty(0, np.uint64), np.random.default_rng(0))
    for kind, is_max in FORMS:
        g, gk, idx, ext = call(fj, rel, kind, is_max, device)
        assert g == 0 and gk.size == 0 and idx.size == 0 and ext.size == 0


# ---- value columns: ties, constants, crafted rounds, identities, zeros and NaN -----------------------------------------------------------
TIE_CASES = ("zero_pass", "one_pass", "hot_key")


@functools.lru_cache(maxsize=None)
def _tie_rel(cid, column):
    keys = _keys_of(cid)
    rng = np.random.default_rng(len(cid) * 7 + len(column))
    small = rng.integers(0, 4, size=keys.size, dtype=np.uint64) if column == "small" else np.full(keys.size, 5, dtype=np.uint64)
    return Rel(keys, small, small.astype(np.float64))


@pytest.mark.gpu
@pytest.mark.parametrize("column", ["small", "equal"])
@pytest.mark.parametrize("cid", TIE_CASES)
def test_ties_go_to_the_smallest_row_index(fj, cid, column):
    """values from {0, 1, 2, 3}: every extreme ties many times; all values equal: every group returns its first row"""
    rel = _tie_rel(cid, column)
    if column == "equal":
        _, first = np.unique(rel.keys, return_index=True)
        for kind, is_max in FORMS:
            assert np.array_equal(rel.ref(kind, is_max)["index"], first)
    for device in CASES[cid][3]:
        run_forms(fj, rel, device, CASES[cid][2])


@functools.lru_cache(maxsize=None)
def _identity_rel(cid, kind, is_max):
    """every second group (by key order) holds nothing but the aggregate's identity; the others random values"""
    keys = _keys_of(cid)
    rng = np.random.default_rng(77)
    rel = random_rel(keys, rng)
    uk, inv = np.unique(keys, return_inverse=True)
    rows = (inv.reshape(-1) % 2) == 0
    iv, fv = rel.ivals.copy(), rel.fvals.copy()
    if kind == "float":
        fv[rows] = IDENTITY[kind, is_max]
    else:
        iv[rows] = np.uint64(IDENTITY[kind, is_max])
    return Rel(keys, iv, fv)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", TIE_CASES)
def test_whole_groups_at_the_identity_still_return_their_first_row(fj, cid):
    """2^64 - 1, 2^63 - 1, 0, -2^63, +inf, -inf: what the value plane holds before its first row; the index is a valid row all the same"""
    _, first = np.unique(_keys_of(cid), return_index=True)
    for kind, is_max in FORMS:
        rel = _identity_rel(cid, kind, is_max)
        assert np.array_equal(rel.ref(kind, is_max)["index"][::2], first[::2])
        for device in CASES[cid][3]:
            run_forms(fj, rel, device, CASES[cid][2], forms=[(kind, is_max)])


CRAFTED = ("only_in_the_last_round", "first_row_and_last_row", "three_times_smallest_in_the_middle")


@functools.lru_cache(maxsize=None)
def _crafted_rel(cid, where, is_max):
    """the long group's rows (the hot key's 100 000, or all 100 003) hold middling values, 2^20 .. 2^40, positive in every kind and exact
    as doubles, except the extreme (7, or 2^50) planted by row order: the kernel streams such a partition in rounds of 4096 rows, twice"""
    keys = _keys_of(cid)
    rng = np.random.default_rng(len(where))
    iv = rng.integers(2**20, 2**40, size=keys.size, dtype=np.uint64)
    uk, cnt = np.unique(keys, return_counts=True)
    rows = np.flatnonzero(keys == uk[np.argmax(cnt)])
    assert rows.size >= 100_000
    plant = {"only_in_the_last_round": [rows[-1]], "first_row_and_last_row": [rows[0], rows[-1]],
             "three_times_smallest_in_the_middle": [rows[rows.size // 2], rows[rows.size // 2 + 30_000], rows[-1]]}[where]
    iv[plant] = np.uint64(2**50 if is_max else 7)
    rel = Rel(keys, iv, iv.astype(np.float64))
    for kind in KINDS:
        r = rel.ref(kind, is_max)
        assert r["index"][int(np.searchsorted(r["keys"], uk[np.argmax(cnt)]))] == plant[0]
    return rel


@pytest.mark.gpu
@pytest.mark.parametrize("where", CRAFTED)
@pytest.mark.parametrize("cid", ["hot_key", "all_equal"])
def test_extremes_planted_by_round_in_a_partition_that_streams_twice(fj, cid, where):
    for is_max in (False, True):
        rel = _crafted_rel(cid, where, is_max)
        run_forms(fj, rel, True, 1, forms=[(kind, is_max) for kind in KINDS])


@functools.lru_cache(maxsize=None)
def _float_rel(cid, column):
    keys = _keys_of(cid)
    n = keys.size
    rng = np.random.default_rng(31)
    if column == "zeros":
        fv = rng.choice(np.array([-0.0, 0.0, -1.0]), n, p=[0.45, 0.45, 0.1])     # the maxima are zeros of either sign, many minima too
    elif column == "extreme":
        fv = extreme_values(17, n)
    else:
        fv = exact_values(19, n)
    return Rel(keys, np.zeros(n, np.uint64), fv)


@pytest.mark.gpu
@pytest.mark.parametrize("column", ["zeros", "extreme", "exact"])
@pytest.mark.parametrize("cid", TIE_CASES)
def test_floats_compare_as_numbers(fj, cid, column):
    """-0.0 and +0.0 tie and the smaller index wins; +-inf, denormals and +-max order as numbers"""
    rel = _float_rel(cid, column)
    if column == "zeros" and cid != "hot_key":
        r = rel.ref("float", True)
        assert np.any(np.signbit(r["value"]) & (r["value"] == 0)) and np.any(~np.signbit(r["value"]) & (r["value"] == 0))
    for device in CASES[cid][3]:
        run_forms(fj, rel, device, CASES[cid][2], forms=[("float", False), ("float", True)])


@pytest.mark.gpu
@pytest.mark.parametrize("cid,base", [("zero_pass", 0), ("one_pass", 0), ("hot_key", 0), ("one_pass", 1)],
                         ids=["zero_pass", "one_pass", "hot_key", "hbm_table"])
def test_a_nan_touches_its_own_group_only(fj, cid, base):
    """two groups hold a NaN (one of either sign bit) among their rows: their value and index are unspecified, the index in [-1, n);
    every other group is exact"""
    keys = _keys_of(cid)
    rng = np.random.default_rng(5)
    uk, cnt = np.unique(keys, return_counts=True)
    multi = uk[cnt >= 2] if np.sum(cnt >= 2) >= 2 else uk
    nan_keys = multi[[0, -1]] if multi.size >= 2 else multi[:1]
    fv = rng.standard_normal(keys.size) * 100.0
    for j, k in enumerate(nan_keys):
        fv[np.flatnonzero(keys == k)[-1]] = np.nan if j == 0 else -np.nan
    rel = Rel(keys, np.zeros(keys.size, np.uint64), fv)
    if base:
        fj.set_option("scalar_hbm_table", 1)
    try:
        for is_max in (False, True):
            out = call(fj, rel, "float", is_max, True, base=base)
            planned(fj, None, path=1 if base else 0)
            gk, idx, ext = check(rel, "float", is_max, out, skip_keys=nan_keys)
            sel = np.isin(gk, nan_keys)
            assert int(np.sum(sel)) == nan_keys.size and np.all((idx[sel] >= -1) & (idx[sel] < rel.n)), idx[sel]
    finally:
        fj.set_option("scalar_hbm_table", 0)


# ---- the HBM-table form -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["zero_pass", "one_pass", "special_keys_one_pass"])
def test_hbm_table_form(fj, cid):
    """FJ_ALGO_SCALAR under scalar_hbm_table = 1: the global table from the start - build, extreme per slot, resolve, sweep.  There the
    out-of-band key is raw 2^64 - 1; the special-key case holds it three times"""
    fj.set_option("scalar_hbm_table", 1)
    try:
        for rel in [_rel_case(cid)] + ([_tie_rel(cid, "small")] if cid in TIE_CASES else []):
            for device in (False, True):
                run_forms(fj, rel, device, 0, base=1)
    finally:
        fj.set_option("scalar_hbm_table", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["zero_pass", "one_pass"])
def test_adaptive_below_the_radix_threshold_takes_the_hbm_table(fj, cid):
    rel = _tie_rel(cid, "small")
    fj.set_option("radix_threshold", rel.n + 1)
    try:
        for kind, is_max in FORMS:
            out = call(fj, rel, kind, is_max, True)
            planned(fj, 0, path=1)
            check(rel, kind, is_max, out)
    finally:
        fj.set_option("radix_threshold", 0)


# ---- the fallback: a partition beyond the 4096-slot table -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _oversized_case():
    """3841 distinct keys in ONE final partition (19) of the 5-bit one-pass plan, every fourth key twice, among 20 000 rows of the other
    31 partitions - built as tests/test_group_by_agg.py builds the edge of its 4096-slot table"""
    n = LIMIT + 1
    rng = np.random.default_rng(n)
    one = keymix.craft(5, 19, rng.integers(0, 2**32, size=n, dtype=np.uint64), n, seed=n)
    assert np.unique(one).size == n and np.all(keymix.partition_of(one, 5) == 19)
    bg = rng.integers(0, 2**64, size=22_000, dtype=np.uint64)
    bg = bg[keymix.partition_of(bg, 5) != 19][:20_000]
    keys = np.concatenate([one, one[::4], bg])
    assert bg.size == 20_000 and 2048 < keys.size <= 32 * 2048                  # one pass of 5 bits
    rng.shuffle(keys)
    small = rng.integers(0, 4, size=keys.size, dtype=np.uint64)
    return random_rel(keys, rng), Rel(keys, small, small.astype(np.float64))


@pytest.mark.gpu
def test_a_partition_beyond_the_lds_table_falls_back_to_the_hbm_table(fj):
    for rel in _oversized_case():
        for device in (False, True):
            for kind, is_max in FORMS:
                out = call(fj, rel, kind, is_max, device)
                lt = fj.last_timings()
                assert lt["fell_back"] == 1 and lt["path"] == 1 and lt["emit_ms"] == 0.0, (kind, is_max, device, lt)
                hbm_timings.check_hbm_form(lt, (kind, is_max, device))
                check(rel, kind, is_max, out)


@functools.lru_cache(maxsize=2)
def _wrap_case(zero_pass):
    """300 keys whose home slot is the table's LAST (hash word 2 = 0xFFF | i << 12): one cluster that wraps past slot 4095 into
    slots 0 .. 298; three copies each with values from {0, 1, 2, 3}, in the last partition of a one-pass plan among background rows,
    or alone on the flat plan"""
    rng = np.random.default_rng(5 + zero_pass)
    w2 = np.uint64(TS - 1) | (np.arange(300, dtype=np.uint64) << np.uint64(12))
    one = keymix.craft(0, 0, w2, 300, seed=3) if zero_pass else keymix.craft(5, 31, w2, 300, seed=3)
    assert np.all((keymix.mix(one) & np.uint64(TS - 1)) == np.uint64(TS - 1))
    keys = np.concatenate([np.repeat(one, 3), rng.integers(0, 2**64, size=1000 if zero_pass else 6000, dtype=np.uint64)])
    rng.shuffle(keys)
    small = rng.integers(0, 4, size=keys.size, dtype=np.uint64)
    return Rel(keys, small, small.astype(np.float64))


@pytest.mark.gpu
@pytest.mark.parametrize("zero_pass", [False, True], ids=["one_pass", "zero_pass"])
def test_a_cluster_that_wraps_past_the_last_slot(fj, zero_pass):
    """the stream's insert and the resolve's read-only probe walk the same wrapped cluster"""
    run_forms(fj, _wrap_case(zero_pass), True, 0 if zero_pass else 1)


# ---- the C ABI: two planes at stride out_capacity, nothing behind them ------------------------------------------------------------------
def _device_call(fj, rel, algo, cap, nb=None):
    """fj_join_device on sentinel-filled buffers of cap + 64 and 2 * cap + 64 words: (rc, err, g, timings, keys, planes) as host arrays"""
    import torch
    from flash_hash_join_amd import _lib, api
    L = _lib.load()
    keys, vals = rel.dev("keys"), rel.dev("ivals")
    A5 = int(np.array(0xA5A5A5A5A5A5A5A5, dtype=np.uint64).view(np.int64))
    ok = torch.full((cap + 64,), A5, dtype=torch.int64, device="cuda")
    ov = torch.full((2 * cap + 64,), A5, dtype=torch.int64, device="cuda")
    cnt = ctypes.c_uint64(0)
    t = _lib.FjTimings()
    with api._ctx_locks.setdefault(0, threading.RLock()):
        rc = L.fj_join_device(api.context(0), algo, 0, 1, keys.data_ptr(), vals.data_ptr(), rel.n if nb is None else nb, None, 0,
                              torch.cuda.current_stream(0).cuda_stream, 64, ctypes.byref(cnt), ok.data_ptr(), ov.data_ptr(), cap, ctypes.byref(t))
        err = _lib.last_error()
    torch.cuda.synchronize()
    return rc, err, int(cnt.value), t, ok.cpu().numpy(), ov.cpu().numpy(), A5


@pytest.mark.gpu
@pytest.mark.parametrize("base", [2, 1], ids=["partitioned", "hbm_table"])
@pytest.mark.parametrize("cid", ["zero_pass", "one_pass"])
def test_guard_words_behind_g_and_behind_the_capacity_stay_intact(fj, cid, base):
    """out_capacity = nb and nb + 13: plane 1 starts at word out_capacity, rows [g, out_capacity) of the keys and of both planes and every
    word behind 2 * out_capacity keep the sentinel"""
    rel = _tie_rel(cid, "small")
    if base == 1:
        fj.set_option("scalar_hbm_table", 1)
    try:
        for cap in (rel.n, rel.n + 13):
            for is_max in (False, True):
                rc, err, g, t, hk, hv, A5 = _device_call(fj, rel, base | GB | ARG | SIGNED | (MAX if is_max else MIN), cap)
                assert rc == 0 and t.path == (0 if base == 2 else 1) and t.fell_back == 0, err
                assert g == rel.ref("signed", is_max)["keys"].size and g < cap
                assert np.all(hk[g:] == A5), "a key word at or beyond row g was written"
                assert np.all(hv[g:cap] == A5) and np.all(hv[cap + g:] == A5), "a plane word at or beyond row g was written"
                check(rel, "signed", is_max, (g, hk[:g].view(np.uint64), hv[:g], hv[cap:cap + g]))
    finally:
        fj.set_option("scalar_hbm_table", 0)


@pytest.mark.gpu
def test_host_entry_returns_two_planes_of_exactly_g_words(fj):
    from flash_hash_join_amd import _lib
    L = _lib.load()
    rel = _rel_case("n4097")
    k, v = rel.keys, rel.ivals
    g = rel.ref("unsigned", True)["keys"].size
    cnt, sec = ctypes.c_uint64(0), ctypes.c_double(0)
    ok, ov = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(L.fj_join_host(GB | ARG | MAX | 2, 0, 1, k.ctypes.data, v.ctypes.data, k.size, None, 0, ctypes.byref(cnt), ctypes.byref(sec),
                              ctypes.byref(ok), ctypes.byref(ov)))
    try:
        assert int(cnt.value) == g
        take = lambda p, n: np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint64)), shape=(n,)).copy()
        hk, hv = take(ok, g), take(ov, 2 * g)
    finally:
        L.fj_free_host(ok)
        L.fj_free_host(ov)
    check(rel, "unsigned", True, (g, hk, hv[:g].view(np.int64), hv[g:]))


# ---- one context, several forms -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_same_context_serves_the_other_group_by_forms_in_between(fj):
    """argmin, group_by_agg, argmax, group_by_min on one context: every result right - two planes, four planes, one plane"""
    rel = _rel_case("one_pass")
    keys, vals = rel.dev("keys"), rel.dev("ivals")
    uk, inv = np.unique(rel.keys, return_inverse=True)
    smin = np.full(uk.size, np.iinfo(np.int64).max, np.int64); np.minimum.at(smin, inv.reshape(-1), rel.ivals.view(np.int64))
    smax = np.full(uk.size, np.iinfo(np.int64).min, np.int64); np.maximum.at(smax, inv.reshape(-1), rel.ivals.view(np.int64))
    check(rel, "signed", False, call(fj, rel, "signed", False, True))
    g, _, gk, cnt, mx = fj.group_by_agg(keys, vals, aggs=("count", "max"), signed=True)
    o = np.argsort(gk.cpu().numpy().view(np.uint64))
    assert g == uk.size and np.array_equal(mx.cpu().numpy()[o], smax) and np.array_equal(cnt.cpu().numpy()[o], np.bincount(inv.reshape(-1)))
    check(rel, "signed", True, call(fj, rel, "signed", True, True))
    g, _, gk, mn = fj.group_by_min(keys, vals, signed=True)
    o = np.argsort(gk.cpu().numpy().view(np.uint64))
    assert g == uk.size and np.array_equal(mn.cpu().numpy()[o], smin)
    check(rel, "float", True, call(fj, rel, "float", True, True))


@pytest.mark.gpu
def test_a_refused_call_leaves_the_context_usable(fj):
    rel = _tie_rel("zero_pass", "small")
    check(rel, "unsigned", False, call(fj, rel, "unsigned", False, True))
    for algo, cap, needle in ((GB | ARG, rel.n, "exactly one of"), (GB | ARG | MIN | MAX, rel.n, "exactly one of"),
                              (GB | ARG | MIN, rel.n - 1, "output capacity")):
        rc, err, g, t, hk, hv, A5 = _device_call(fj, rel, algo, cap)
        assert rc != 0 and needle in err and np.all(hk == A5) and np.all(hv == A5), err
    check(rel, "unsigned", True, call(fj, rel, "unsigned", True, True))
    check(rel, "float", False, call(fj, rel, "float", False, False))
