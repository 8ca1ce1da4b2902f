"""The inverse of the group-by (FJ_ALGO_INVERSE, csrc/fj_groupby.hip; api.factorize / api.unique(return_inverse=True)): the distinct
keys of a relation and, for every row, the dense id of its group at the row's own position.  The C-ABI contract and the argument checks
need no GPU; on an MI355X every plan is checked against NumPy.

Reference: np.unique(keys).size for g, and the keys themselves for the ids - the order of the groups is unspecified, so no id is ever
compared with NumPy's.  What is checked instead, exactly and element by element: the returned keys are distinct, 0 <= codes < g,
uniques[codes] == keys, and np.unique(codes).size == g."""
import ctypes
import functools
import inspect
import os
import re
import threading

import numpy as np
import pytest

import hbm_timings
import keymix
from conftest import ROOT

MANY, LEFT, ANTI, ROW_IDS, FULL, ALL, PO, BO = 0x10, 0x20, 0x40, 0x80, 0x100, 0x200, 0x800, 0x1000
MIN, MAX, SIGNED, GB, INV = 0x4000, 0x8000, 0x10000, 0x40000, 0x100000
GI = GB | INV


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_header_flag_and_python_mirror():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    assert int(re.search(r"#define FJ_ALGO_INVERSE\s+(0x[0-9a-fA-F]+)", hdr).group(1), 16) == 0x100000
    from flash_hash_join_amd import api
    assert api.ALGO_INVERSE == 0x100000


def test_abi_version_and_function_count_are_unchanged():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    assert "FJ_ALGO_INVERSE" in hdr
    assert int(re.search(r"#define FJ_ABI_VERSION (\d+)", hdr).group(1)) == 8
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert len(set(re.findall(r"\b(fj_[a-z0-9_]+)\s*\(", code))) == 40
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_abi_version() == 8 and len(_lib.SYMBOLS) == 40


def test_flash_join_exposes_factorize():
    import flash_join
    from flash_hash_join_amd import api
    assert callable(flash_join.factorize) and "factorize" in api.EXTENSIONS and "factorize" in api.__all__
    assert flash_join.unique is api.unique


def test_unique_takes_return_inverse_last_and_off():
    from flash_hash_join_amd import api
    params = list(inspect.signature(api.unique).parameters.values())
    assert [p.name for p in params] == ["keys", "return_index", "return_counts", "return_inverse"]
    assert params[-1].default is False and params[1].default is False and params[2].default is False
    assert list(inspect.signature(api.factorize).parameters) == ["keys"]


def _device_call(algo, materialize=1, vals=0x20000, pk=None, n_p=0, ok=0x40000, ov=0x50000, cap=100, nb=100):
    from flash_hash_join_amd import _lib
    cnt = ctypes.c_uint64(0)
    rc = _lib.load().fj_join_device(None, algo, 0, materialize, 0x10000, vals, nb, pk, n_p, None, 64, ctypes.byref(cnt), ok, ov, cap, None)
    return rc, _lib.last_error()


DEVICE_REFUSALS = [   # id, keyword arguments of _device_call, needles
    ("bare", dict(algo=INV), ("unknown algo 1048576",)),
    ("bare_with_base", dict(algo=INV | 2), ("unknown algo",)),
    ("with_min_but_no_group_by", dict(algo=INV | MIN), ("unknown algo",)),
    ("build_order", dict(algo=INV | BO), ("unknown algo",)),
    ("min", dict(algo=GI | MIN), ("FJ_ALGO_INVERSE cannot be combined with FJ_ALGO_AGG_MIN",)),
    ("max", dict(algo=GI | MAX | 2), ("FJ_ALGO_INVERSE cannot be combined with FJ_ALGO_AGG_MAX",)),
    ("max_signed", dict(algo=GI | MAX | SIGNED), ("FJ_ALGO_INVERSE cannot be combined with FJ_ALGO_AGG_MAX",)),
    ("signed", dict(algo=GI | SIGNED | 1), ("FJ_ALGO_INVERSE cannot be combined with FJ_ALGO_AGG_SIGNED",)),
    ("row_ids", dict(algo=GI | ROW_IDS), ("FJ_ALGO_INVERSE cannot be combined with FJ_ALGO_ROW_IDS",)),
    ("count_only", dict(algo=GI, materialize=0), ("FJ_ALGO_INVERSE", "materialize = 1")),
    ("count_only_without_buffers", dict(algo=GI | 2, materialize=0, ok=None, ov=None, cap=0, vals=None), ("FJ_ALGO_INVERSE", "materialize = 1")),
    ("no_ids_output", dict(algo=GI, ov=None), ("FJ_ALGO_INVERSE", "d_out_vals")),
    ("no_keys_output", dict(algo=GI | 1, ok=None), ("FJ_ALGO_INVERSE", "d_out_keys")),
    ("capacity", dict(algo=GI, cap=99), ("output capacity 99 < 100",)),
    ("misaligned_keys", dict(algo=GI, ok=0x40004), ("8-byte aligned",)),
    ("misaligned_ids", dict(algo=GI | 2, ov=0x50004), ("8-byte aligned",)),
    # everything FJ_ALGO_GROUP_BY refuses
    ("many", dict(algo=GI | MANY), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_MANY_TO_MANY",)),
    ("left", dict(algo=GI | LEFT), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_LEFT_OUTER",)),
    ("anti", dict(algo=GI | ANTI), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_ANTI",)),
    ("full", dict(algo=GI | FULL), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_FULL_OUTER",)),
    ("all_copies", dict(algo=GI | ALL), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_ALL_COPIES",)),
    ("probe_order", dict(algo=GI | PO), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_PROBE_ORDER",)),
    ("build_order_group_by", dict(algo=GI | BO), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_BUILD_ORDER",)),
    ("probe_keys", dict(algo=GI, pk=0x30000), ("FJ_ALGO_GROUP_BY", "no probe side")),
    ("probe_rows", dict(algo=GI, n_p=7), ("FJ_ALGO_GROUP_BY", "no probe side")),
    ("next_bit", dict(algo=GB | 0x200000), ("unknown algo",)),
    ("next_bit_with_inverse", dict(algo=GI | 0x200000), ("unknown algo",)),
    ("pinned_bit_0x80000", dict(algo=GI | 0x80000), ("unknown algo",)),
    ("pinned_bit_0x20000", dict(algo=GI | 0x20000), ("unknown algo",)),
    ("pinned_bit_0x2000", dict(algo=GI | 0x2000), ("unknown algo",)),
    ("pinned_bit_0x400", dict(algo=GI | 0x400), ("unknown algo",)),
    ("base_3", dict(algo=GI | 3), ("unknown algo",)),
]


@pytest.mark.parametrize("cid,kw,needles", DEVICE_REFUSALS, ids=[r[0] for r in DEVICE_REFUSALS])
def test_invalid_combinations_are_refused_before_any_device_work(cid, kw, needles):
    """A NULL context: the checks come before the context is touched (no GPU needed; the pointers are never dereferenced)."""
    rc, err = _device_call(**kw)
    assert rc != 0 and "null context" not in err, err
    for needle in needles:
        assert needle in err, err


VALID = [(f"{('adaptive', 'scalar', 'radix')[base]}-{fid}", dict(algo=GI | base, **kw)) for base in (0, 1, 2)
         for fid, kw in (("values_ignored", dict()), ("no_values", dict(vals=None)), ("more_capacity_than_rows", dict(cap=5000)),
                         ("more_capacity_no_values", dict(cap=101, vals=None)), ("no_rows", dict(nb=0, cap=0, ok=None, ov=None, vals=None)))]


@pytest.mark.parametrize("cid,kw", VALID, ids=[v[0] for v in VALID])
def test_valid_combinations_reach_the_context(cid, kw):
    rc, err = _device_call(**kw)
    assert rc != 0 and "null context" in err, err


HOST_REFUSALS = [   # id, algo, materialize, values, probe keys, np, needles
    ("bare", INV, 1, True, False, 0, ("unknown algo 1048576",)),
    ("bare_with_min", INV | MIN | 2, 1, True, False, 0, ("unknown algo",)),
    ("min", GI | MIN, 1, True, False, 0, ("FJ_ALGO_INVERSE cannot be combined with FJ_ALGO_AGG_MIN",)),
    ("max_signed", GI | MAX | SIGNED, 1, True, False, 0, ("FJ_ALGO_INVERSE cannot be combined with FJ_ALGO_AGG_MAX",)),
    ("signed", GI | SIGNED, 1, False, False, 0, ("FJ_ALGO_INVERSE cannot be combined with FJ_ALGO_AGG_SIGNED",)),
    ("row_ids", GI | ROW_IDS | 1, 1, False, False, 0, ("FJ_ALGO_INVERSE cannot be combined with FJ_ALGO_ROW_IDS",)),
    ("count_only", GI, 0, False, False, 0, ("FJ_ALGO_INVERSE", "materialize = 1")),
    ("many", GI | MANY, 1, True, False, 0, ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_MANY_TO_MANY",)),
    ("build_order", GI | BO, 1, True, False, 0, ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_BUILD_ORDER",)),
    ("probe_keys", GI, 1, False, True, 0, ("no probe side",)),
    ("probe_rows", GI | 2, 1, False, True, 8, ("no probe side",)),
    ("next_bit", GB | 0x200000, 1, True, False, 0, ("unknown algo",)),
    ("next_bit_with_inverse", GI | 0x200000, 1, True, False, 0, ("unknown algo",)),
    ("pinned_bit_0x80000", GI | 0x80000, 1, True, False, 0, ("unknown algo",)),
    ("base_9", GI | 9, 1, True, False, 0, ("unknown algo",)),
]


def _host_call(algo, materialize, vals, pk, n_p, want_keys=True, want_ids=True):
    from flash_hash_join_amd import _lib
    L = _lib.load()
    k = np.arange(8, dtype=np.uint64)
    cnt, sec = ctypes.c_uint64(0), ctypes.c_double(0)
    ok, ov = ctypes.c_void_p(), ctypes.c_void_p()
    rc = L.fj_join_host(algo, 0, materialize, k.ctypes.data, k.ctypes.data if vals else None, 8, k.ctypes.data if pk else None, n_p,
                        ctypes.byref(cnt), ctypes.byref(sec), ctypes.byref(ok) if want_keys else None, ctypes.byref(ov) if want_ids else None)
    return rc, _lib.last_error(), ok, ov


@pytest.mark.parametrize("cid,algo,materialize,vals,pk,n_p,needles", HOST_REFUSALS, ids=[r[0] for r in HOST_REFUSALS])
def test_host_entry_refusals(cid, algo, materialize, vals, pk, n_p, needles):
    """fj_join_host makes the same checks before its context is created (no GPU needed)."""
    rc, err, ok, ov = _host_call(algo, materialize, vals, pk, n_p)
    assert rc != 0 and "null context" not in err and "HIP device" not in err, err
    for needle in needles:
        assert needle in err, err
    assert not ok.value and not ov.value


@pytest.mark.parametrize("base", [0, 1, 2])
@pytest.mark.parametrize("vals", [True, False], ids=["values_ignored", "no_values"])
@pytest.mark.parametrize("want_keys,want_ids", [(True, True), (True, False), (False, True)], ids=["both", "keys_alone", "ids_alone"])
def test_host_entry_accepts_every_valid_combination(base, vals, want_keys, want_ids):
    """past the argument checks: the call runs where there is a device, and fails on the missing device - never on a flag - elsewhere"""
    from flash_hash_join_amd import _lib
    rc, err, ok, ov = _host_call(GI | base, 1, vals, False, 0, want_keys, want_ids)
    try:
        assert rc == 0 or ("FJ_ALGO" not in err and "unknown algo" not in err), err
    finally:
        _lib.load().fj_free_host(ok)
        _lib.load().fj_free_host(ov)


def test_python_argument_errors():
    from flash_hash_join_amd import api
    k = np.arange(4, dtype=np.uint64)
    with pytest.raises(TypeError, match="keys"):
        api.factorize(np.array(["a", "b", "c", "d"]))
    with pytest.raises(TypeError, match="keys"):
        api.unique(np.array(["a", "b"]), return_inverse=True)
    with pytest.raises(TypeError, match="keys"):
        api.unique(np.array(["a", "b"]), return_index=True, return_inverse=True, return_counts=True)
    with pytest.raises(TypeError):
        api.factorize()                                                # keys is not optional
    with pytest.raises(TypeError):
        api.factorize(k, k)                                            # no value column: the ids are the call's output
    with pytest.raises(ValueError, match="ALGO_INVERSE"):
        api._group_by(k, None, api.ALGO_INVERSE, materialize=False)
    with pytest.raises(ValueError, match="ALGO_INVERSE"):
        api._group_by(k, None, api.ALGO_INVERSE, want_vals=False)


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fj():
    import flash_join
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_device_count() >= 1, "no HIP device: the product path must not silently fall back"
    assert flash_join.initialize() is None
    return flash_join


class Rel:
    """a relation and its reference (the number of distinct keys), computed once"""
    def __init__(self, keys):
        self.keys = np.ascontiguousarray(keys, dtype=np.uint64)
        self.n = self.keys.size
        self.g = int(np.unique(self.keys).size)
        self._dev = None

    def arg(self, device):
        if not device:
            return self.keys
        if self._dev is None:
            import torch
            self._dev = torch.from_numpy(self.keys.view(np.int64)).cuda()
        return self._dev


def _host(a, device):
    if device:
        assert a.is_cuda and str(a.dtype) == "torch.int64", a.dtype
        return a.cpu().numpy()
    assert isinstance(a, np.ndarray), type(a)
    return a


def check_ids(rel, what, g, uniques, codes, device=False, raw=False):
    """the distinct keys and every row's id against the relation itself.  raw: arrays read back from the C ABI (uint64 words)"""
    assert isinstance(g, int) and g == rel.g, (what, g, rel.g)
    uniques, codes = _host(uniques, device), _host(codes, device)
    if not raw:
        assert codes.dtype == np.int64 and uniques.dtype == (np.int64 if device else np.uint64), (what, codes.dtype, uniques.dtype)
    uniques, codes = uniques.view(np.uint64), codes.view(np.int64)
    assert uniques.shape == (g,) and codes.shape == (rel.n,), (what, uniques.shape, codes.shape)
    assert np.unique(uniques).size == g, f"{what}: the returned keys are not distinct"
    if rel.n == 0:
        return
    assert codes.min() >= 0 and codes.max() < g, (what, int(codes.min()), int(codes.max()), g)
    assert np.array_equal(uniques[codes], rel.keys), f"{what}: uniques[codes] != keys in {int(np.count_nonzero(uniques[codes] != rel.keys))} rows"
    assert np.unique(codes).size == g, f"{what}: not every id is used"


def check_timings(lt, what, path, passes, fell_back):
    assert lt["emit_ms"] == 0.0 and lt["join_ms"] == lt["probe_phase_ms"], (what, lt)
    assert lt["path"] == path and lt["fell_back"] == fell_back, (what, lt)
    if path == 1:
        hbm_timings.check_hbm_form(lt, what)
    if passes is not None:
        assert lt["passes"] == passes, (what, lt)


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


CASES = {   # id: (keys builder, plan_target_keys, passes)
    "zero_pass": (lambda rng: _dup_keys(rng, 1000, 37), 4096, 0),
    "single_row": (lambda rng: np.array([0x1234567890ABCDEF], dtype=np.uint64), 4096, 0),
    "all_distinct_zero_pass": (lambda rng: _dup_keys(rng, 3000, 3000), 4096, 0),
    "all_equal_zero_pass": (lambda rng: np.full(777, 42, dtype=np.uint64), 4096, 0),
    "n4097": (lambda rng: _dup_keys(rng, 4097, 1500), 4096, 1),
    "one_pass": (lambda rng: _dup_keys(rng, 200_003, 50_000), 4096, 1),
    "all_distinct": (lambda rng: _dup_keys(rng, 20_011, 20_011), 4096, 1),
    "all_equal": (lambda rng: np.full(100_003, 0xDEADBEEF12345678, dtype=np.uint64), 4096, 1),      # one slot read by every row in stream 2
    "two_pass_10_bits": (lambda rng: _dup_keys(rng, 200_003, 50_000), 256, 2),
    "two_pass_14_bits": (lambda rng: _dup_keys(rng, 200_003, 50_000), 16, 2),
    "hot_key": (_hot_keys, 4096, 1),
    "special_keys_zero_pass": (lambda rng: _special_keys(rng, 500, 0), 4096, 0),
    "special_keys_one_pass": (lambda rng: _special_keys(rng, 20_000, 5), 4096, 1),
}
PARITY = [(cid, device) for cid in CASES for device in (False, True)]


@functools.lru_cache(maxsize=None)
def _case(cid):
    return Rel(CASES[cid][0](np.random.default_rng(sorted(CASES).index(cid) + 500)))


def check_special_keys(rel, what, uniques, codes, device, marker):
    """all copies of the out-of-band key carry ONE id and that id names the key; the other special keys are groups like any other"""
    uniques, codes = _host(uniques, device).view(np.uint64), _host(codes, device)
    for k in (keymix.EMPTY_RAW, keymix.FILLER_RAW, 0, 2**64 - 1):
        rows = np.flatnonzero(rel.keys == np.uint64(k))
        assert rows.size in (3, 6), (what, hex(k), rows.size)          # (raw 0 six times: it is also the raw key of the mixed word 0)
        ids = np.unique(codes[rows])
        assert ids.size == 1 and uniques[ids[0]] == np.uint64(k), (what, hex(k), ids)
    rows = np.flatnonzero(rel.keys == np.uint64(marker))
    assert rows.size == 3 and np.unique(codes[rows]).size == 1 and int(uniques[codes[rows[0]]]) == marker, what


@pytest.mark.gpu
@pytest.mark.parametrize("cid,device", PARITY, ids=[f"{c}-{'device' if d else 'numpy'}" for c, d in PARITY])
def test_factorize_on_the_partitioned_plan(fj, cid, device):
    _, target, passes = CASES[cid]
    rel = _case(cid)
    if cid == "hot_key":
        assert rel.g == 100_001 and rel.n == 200_000
    if cid.startswith("all_distinct"):
        assert rel.g == rel.n
    if cid.startswith("all_equal"):
        assert rel.g == 1
    fj.set_option("plan_target_keys", target)
    try:
        g, sec, codes, uniques = fj.factorize(rel.arg(device))
        lt = fj.last_timings()
    finally:
        fj.set_option("plan_target_keys", 4096)
    assert isinstance(sec, float)
    check_timings(lt, cid, path=0, passes=passes, fell_back=0)
    check_ids(rel, cid, g, uniques, codes, device)
    if cid.startswith("special_keys"):
        check_special_keys(rel, cid, uniques, codes, device, keymix.EMPTY_RAW)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_empty_input(fj, device):
    import torch
    rel = Rel(np.empty(0, np.uint64))
    g, sec, codes, uniques = fj.factorize(rel.arg(device))
    assert g == 0 and isinstance(sec, float)
    check_ids(rel, "empty", g, uniques, codes, device)
    out = fj.unique(rel.arg(device), return_index=True, return_inverse=True, return_counts=True)
    assert out[0] == 0 and len(out) == 6 and all(_host(a, device).shape == (0,) for a in out[2:])
    if not device:
        assert out[2].dtype == np.uint64 and all(a.dtype == np.int64 for a in out[3:])
        return
    # the raw call with nb = 0: g = 0 and not a word of either buffer is written
    from flash_hash_join_amd import _lib, api
    A5 = int(np.array(0xA5A5A5A5A5A5A5A5, dtype=np.uint64).view(np.int64))
    ok = torch.full((64,), A5, dtype=torch.int64, device="cuda")
    ov = torch.full((64,), A5, dtype=torch.int64, device="cuda")
    cnt = ctypes.c_uint64(7)
    with api._ctx_locks.setdefault(0, threading.RLock()):
        _lib.check(_lib.load().fj_join_device(api.context(0), GI | 2, 0, 1, None, None, 0, None, 0, torch.cuda.current_stream(0).cuda_stream, 64,
                                              ctypes.byref(cnt), ok.data_ptr(), ov.data_ptr(), 64, None))
    assert int(cnt.value) == 0 and bool((ok == A5).all()) and bool((ov == A5).all())


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["one_pass", "special_keys_one_pass", "all_equal", "single_row"])
@pytest.mark.parametrize("option,base", [("scalar_hbm_table", 1), ("radix_threshold", 0)])
def test_hbm_table_form(fj, option, base, cid):
    """FJ_ALGO_SCALAR under scalar_hbm_table = 1 and FJ_ALGO_ADAPTIVE below radix_threshold: the global table from the start.  There
    the out-of-band key is raw 2^64 - 1; the special-key case holds it three times beside the LDS tables' marker"""
    from flash_hash_join_amd import api
    rel = _case(cid)
    fj.set_option(option, 1 if base else rel.n + 1)
    try:
        for device in (False, True):
            if base:
                g, sec, uniques, codes = api._group_by(rel.arg(device), None, base | api.ALGO_INVERSE)
            else:
                g, sec, codes, uniques = fj.factorize(rel.arg(device))
            check_timings(fj.last_timings(), cid, path=1, passes=0, fell_back=0)
            check_ids(rel, cid, g, uniques, codes, device)
            if cid.startswith("special_keys"):
                check_special_keys(rel, cid, uniques, codes, device, 2**64 - 1)
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
    return Rel(keys)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_a_partition_beyond_the_lds_table_falls_back_to_the_hbm_table(fj, device):
    """more distinct keys in one partition than the 8192-slot table takes: the other partitions have written ids counted from a cursor
    that is abandoned; the re-run on the HBM table from cursor 0 must define all 29 000 ids again"""
    rel = _oversized_case()
    assert rel.n == 29_000
    g, sec, codes, uniques = fj.factorize(rel.arg(device))
    check_timings(fj.last_timings(), "fallback", path=1, passes=None, fell_back=1)
    check_ids(rel, "fallback", g, uniques, codes, device)


POISON = 0xA5A5A5A5A5A5A5A5


def _raw_device_call(L, api, algo, keys, nb, ok, ov, cap):
    import torch
    from flash_hash_join_amd import _lib
    cnt = ctypes.c_uint64(0)
    t = _lib.FjTimings()
    with api._ctx_locks.setdefault(0, threading.RLock()):
        _lib.check(L.fj_join_device(api.context(0), algo, 0, 1, keys.data_ptr(), None, nb, None, 0, torch.cuda.current_stream(0).cuda_stream, 64,
                                    ctypes.byref(cnt), ok.data_ptr(), ov.data_ptr(), cap, ctypes.byref(t)))
    return int(cnt.value), t


@pytest.mark.gpu
@pytest.mark.parametrize("base", [2, 1], ids=["partitioned", "hbm_table"])
@pytest.mark.parametrize("extra", [0, 1000], ids=["capacity_nb", "capacity_nb_plus_1000"])
def test_guard_words_and_full_definition(fj, base, extra):
    """fj_join_device on poisoned buffers of out_capacity + 64 words, d_build_vals NULL: all nb ids are defined by the call alone (no
    poison survives below nb), and the 64 words behind out_capacity are intact in both buffers"""
    import torch
    from flash_hash_join_amd import _lib, api
    L = _lib.load()
    rel = _case("one_pass")
    keys, nb = rel.arg(True), rel.n
    cap = nb + extra
    A5 = int(np.array(POISON, dtype=np.uint64).view(np.int64))
    if base == 1:
        fj.set_option("scalar_hbm_table", 1)
    try:
        ok = torch.full((cap + 64,), A5, dtype=torch.int64, device="cuda")
        ov = torch.full((cap + 64,), A5, dtype=torch.int64, device="cuda")
        g, t = _raw_device_call(L, api, base | GI, keys, nb, ok, ov, cap)
    finally:
        fj.set_option("scalar_hbm_table", 0)
    assert t.path == (0 if base == 2 else 1) and t.emit_ms == 0.0 and t.fell_back == 0 and t.join_ms == t.probe_phase_ms
    hk, hv = ok.cpu().numpy(), ov.cpu().numpy()
    assert np.all(hk[cap:] == A5) and np.all(hv[cap:] == A5), "a word at or beyond out_capacity was written"
    assert np.all(hv[nb:cap] == A5), "an id beyond the relation's rows was written"
    assert not np.any(hv[:nb] == A5), "an id below nb was left undefined"
    check_ids(rel, "guard words", g, hk[:g], hv[:nb], raw=True)


def _ref_counts(rel, uniques):
    """rows per key from the reference's own grouping (np.unique), aligned with `uniques` through the keys"""
    uk, cnt = np.unique(rel.keys, return_counts=True)
    return cnt[np.searchsorted(uk, uniques)].astype(np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("cid", ["zero_pass", "one_pass"])
def test_unique_with_return_inverse(fj, cid, device):
    rel = _case(cid)
    keys = rel.arg(device)
    # the existing call shapes return what they returned
    assert len(fj.unique(keys)) == 3 and len(fj.unique(keys, return_counts=True)) == 4 and len(fj.unique(keys, return_index=True)) == 4
    assert len(fj.unique(keys, True, True)) == 5

    g, sec, gk, inv = fj.unique(keys, return_inverse=True)
    check_timings(fj.last_timings(), "inverse", path=0, passes=CASES[cid][2], fell_back=0)
    check_ids(rel, "unique(return_inverse)", g, gk, inv, device)

    g, sec, gk, inv, cnt = fj.unique(keys, return_counts=True, return_inverse=True)
    check_ids(rel, "unique(return_inverse, return_counts)", g, gk, inv, device)
    cnt = _host(cnt, device)
    assert cnt.dtype == np.int64 and np.array_equal(cnt, _ref_counts(rel, _host(gk, device).view(np.uint64))), "counts"

    def first_index_is_right(gk, idx):
        gk, idx = _host(gk, device).view(np.uint64), _host(idx, device)
        assert idx.dtype == np.int64 and np.array_equal(rel.keys[idx], gk), "keys[first_index] != unique_keys"
        uk, first = np.unique(rel.keys, return_index=True)
        assert np.array_equal(idx, first[np.searchsorted(uk, gk)]), "an index is not the smallest position of its key"

    g, sec, gk, idx, inv = fj.unique(keys, return_index=True, return_inverse=True)
    assert isinstance(sec, float)
    check_ids(rel, "unique(return_index, return_inverse)", g, gk, inv, device)
    first_index_is_right(gk, idx)

    g, sec, gk, idx, inv, cnt = fj.unique(keys, return_index=True, return_counts=True, return_inverse=True)
    check_ids(rel, "unique(all three)", g, gk, inv, device)
    first_index_is_right(gk, idx)
    assert np.array_equal(_host(cnt, device), _ref_counts(rel, _host(gk, device).view(np.uint64))), "counts"


@pytest.mark.gpu
def test_the_same_context_reused(fj):
    """factorize, a group_by_sum, a factorize of another size on one context: all correct, and no result is left pending"""
    import torch
    from flash_hash_join_amd import _lib, api
    L = _lib.load()
    a, b, c = _case("one_pass"), _case("n4097"), _case("all_distinct")
    g, _, codes, uniques = fj.factorize(a.arg(True))
    check_ids(a, "first factorize", g, uniques, codes, True)
    vals = np.arange(1, b.n + 1, dtype=np.int64)
    with api._ctx_locks.setdefault(0, threading.RLock()):
        gs, _, gk, sums = fj.group_by_sum(b.arg(True), torch.from_numpy(vals).cuda())
        g, _, codes, uniques = fj.factorize(c.arg(True))
        out = torch.empty(c.n, dtype=torch.int64, device="cuda")
        assert L.fj_emit_pairs(api.context(0), out.data_ptr(), out.data_ptr(), c.n, torch.cuda.current_stream(0).cuda_stream, None) != 0, "a result was left pending"
        assert "no counted materialising join is pending" in _lib.last_error()
    check_ids(c, "second factorize", g, uniques, codes, True)
    uk, inv = np.unique(b.keys, return_inverse=True)
    want = np.zeros(uk.size, np.int64)
    np.add.at(want, inv.reshape(-1), vals)
    gk = gk.cpu().numpy().view(np.uint64)
    assert gs == b.g and np.array_equal(sums.cpu().numpy()[np.argsort(gk)], want), "group_by_sum between two factorize calls"
    # the ids do what they are for: a second aggregate of the first relation from ONE grouping
    g, _, codes, uniques = fj.factorize(b.arg(True))
    sums2 = torch.zeros(g, dtype=torch.int64, device="cuda").index_add_(0, codes, torch.from_numpy(vals).cuda())
    assert np.array_equal(sums2.cpu().numpy()[np.argsort(uniques.cpu().numpy().view(np.uint64))], want)


@pytest.mark.gpu
def test_host_entry_returns_g_keys_and_nb_ids_and_drops_a_null_output(fj):
    """fj_join_host on NumPy arrays: *out_keys has exactly g rows, *out_vals exactly nb; NULL for either pointer drops that output"""
    from flash_hash_join_amd import _lib
    L = _lib.load()
    rel = _case("one_pass")
    k = rel.keys
    take = lambda p, rows: np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint64)), shape=(rows,)).copy()
    for want_keys, want_ids in ((True, True), (True, False), (False, True), (False, False)):
        cnt, sec = ctypes.c_uint64(0), ctypes.c_double(0)
        ok, ov = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(L.fj_join_host(GI | 2, 0, 1, k.ctypes.data, None, k.size, None, 0, ctypes.byref(cnt), ctypes.byref(sec),
                                  ctypes.byref(ok) if want_keys else None, ctypes.byref(ov) if want_ids else None))
        try:
            g = int(cnt.value)
            assert g == rel.g and bool(ok.value) == want_keys and bool(ov.value) == want_ids
            t = _lib.FjTimings()
            L.fj_last_timings(ctypes.byref(t))
            assert t.emit_ms == 0.0 and t.path == 0 and t.fell_back == 0 and t.passes == 1 and t.join_ms == t.probe_phase_ms
            if want_keys and want_ids:
                check_ids(rel, "host both", g, take(ok, g), take(ov, rel.n), raw=True)
            elif want_keys:
                uk = take(ok, g)
                assert np.array_equal(np.sort(uk), np.unique(k)), "host keys alone"
            elif want_ids:
                ids = take(ov, rel.n).view(np.int64)                    # (no keys to look the ids up in: they partition the rows as the keys do)
                assert ids.min() >= 0 and ids.max() < g and np.unique(ids).size == g
                first = np.full(g, -1, np.int64)
                first[ids[::-1]] = np.arange(rel.n - 1, -1, -1)
                assert np.array_equal(k[first[ids]], k), "host ids alone: two keys share an id"
        finally:
            L.fj_free_host(ok)
            L.fj_free_host(ov)
