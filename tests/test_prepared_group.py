"""Aggregates of probe batches onto a prepared build side (FJ_ALGO_BUILD_ORDER | FJ_ALGO_REUSE_BUILD [| FJ_ALGO_ACCUMULATE],
csrc/fj_prepared.hip; Index.group_count / group_sum / group_min / group_max).  The C-ABI contract and the argument checks need no GPU;
on an MI355X every form is compared bit for bit with a NumPy reference: the aggregate of a key lands at the key's FIRST build row, every
other row holds 0 (count, sum) or the aggregate's identity (min / max) - or, under out=, what it held before.

Reference: the first-occurrence row of every probe key from tests/test_prepared.py (a stable argsort and searchsorted; no hashing, never
the library), then np.add.at / np.minimum.at / np.maximum.at of the probe values over those rows.  The build sides, batches and
constructions are those of tests/test_prepared.py, so both files share one set of inputs."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import keymix
import test_prepared as TP
from conftest import ROOT

MANY, LEFT, ANTI, ROW_IDS, FULL, ALL, PO, BO, GB = 0x10, 0x20, 0x40, 0x80, 0x100, 0x200, 0x800, 0x1000, 0x40000
AMIN, AMAX, ASIGNED = 0x4000, 0x8000, 0x10000
RETAIN, REUSE, ACC = 0x400000, 0x800000, 0x1000000
U64_MAX, I64_MAX, I64_MIN_U = 2**64 - 1, 2**63 - 1, 2**63
A5 = np.uint64(0xA5A5A5A5A5A5A5A5)
FORMS = ("count", "sum", "min_u", "min_s", "max_u", "max_s")
IDENT = {"count": 0, "sum": 0, "min_u": U64_MAX, "min_s": I64_MAX, "max_u": 0, "max_s": I64_MIN_U}     # the uint64 words


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_header_flag_python_mirror_and_unchanged_abi():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    assert int(re.search(r"#define FJ_ALGO_ACCUMULATE\s+(0x[0-9a-fA-F]+)", hdr).group(1), 16) == ACC == 0x1000000
    assert int(re.search(r"#define FJ_ABI_VERSION (\d+)", hdr).group(1)) == 8
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert len(set(re.findall(r"\b(fj_[a-z0-9_]+)\s*\(", code))) == 40
    assert not re.search(r"#define FJ_ALGO_\w+\s+0x200000\b", hdr), "bit 0x200000 stays unassigned"
    assert "first build row" in hdr.lower() or "FIRST BUILD ROW" in hdr, "the header states the first-occurrence rule"
    from flash_hash_join_amd import _lib, api
    assert api.ALGO_ACCUMULATE == ACC
    assert _lib.load().fj_abi_version() == 8 and len(_lib.SYMBOLS) == 40
    for name in ("group_count", "group_sum", "group_min", "group_max"):
        assert callable(getattr(api.Index, name)) and "first" in getattr(api.Index, name).__doc__.lower() + api.Index.group_count.__doc__.lower()


def _device_call(algo, materialize=1, bk=None, pv=0x20000, nb=0, pk=0x30000, n_p=1000, cnt=0x40000, vals=0x50000, cap=1000, top=64):
    from flash_hash_join_amd import _lib
    c = ctypes.c_uint64(0)
    rc = _lib.load().fj_join_device(None, algo, 0, materialize, bk, pv, nb, pk, n_p, None, top, ctypes.byref(c), cnt, vals, cap, None)
    return rc, _lib.last_error()


REFUSALS = [   # id, keyword arguments of _device_call, needles
    ("bo_retain", dict(algo=BO | RETAIN, bk=0x10000, nb=100), ("unknown algo",)),
    ("bo_retain_reuse", dict(algo=BO | RETAIN | REUSE), ("unknown algo",)),
    ("accumulate_alone", dict(algo=ACC), ("unknown algo",)),
    ("accumulate_base", dict(algo=ACC | 2, bk=0x10000, nb=100), ("unknown algo",)),
    ("bo_accumulate", dict(algo=BO | ACC, bk=0x10000, nb=100), ("unknown algo",)),
    ("reuse_accumulate", dict(algo=REUSE | ACC, pv=None), ("unknown algo",)),
    ("po_reuse_accumulate", dict(algo=PO | REUSE | ACC, pv=None), ("unknown algo",)),
    ("po_accumulate", dict(algo=PO | ACC, bk=0x10000, nb=100), ("unknown algo",)),
    ("gb_accumulate", dict(algo=GB | ACC, bk=0x10000, nb=100, pk=None, n_p=0), ("unknown algo",)),
    ("base_3", dict(algo=BO | REUSE | 3), ("unknown algo",)),
    ("free_bit", dict(algo=BO | REUSE | 0x200000), ("unknown algo",)),
    ("build_keys", dict(algo=BO | REUSE, bk=0x10000), ("FJ_ALGO_REUSE_BUILD takes no build side",)),
    ("build_rows", dict(algo=BO | REUSE | 2, nb=100), ("FJ_ALGO_REUSE_BUILD takes no build side",)),
    ("build_side", dict(algo=BO | REUSE | AMIN, bk=0x10000, nb=100), ("FJ_ALGO_REUSE_BUILD takes no build side",)),
    ("build_side_accumulate", dict(algo=BO | REUSE | ACC, bk=0x10000, nb=100), ("FJ_ALGO_REUSE_BUILD takes no build side",)),
    ("build_keys_counts_only", dict(algo=BO | REUSE, bk=0x10000, pv=None, vals=None), ("FJ_ALGO_REUSE_BUILD takes no build side",)),
    ("row_ids", dict(algo=BO | REUSE | ROW_IDS), ("FJ_ALGO_BUILD_ORDER cannot be combined with FJ_ALGO_ROW_IDS",)),
    ("many", dict(algo=BO | REUSE | MANY), ("FJ_ALGO_BUILD_ORDER cannot be combined with FJ_ALGO_MANY_TO_MANY",)),
    ("left", dict(algo=BO | REUSE | LEFT), ("FJ_ALGO_BUILD_ORDER cannot be combined with FJ_ALGO_LEFT_OUTER",)),
    ("anti", dict(algo=BO | REUSE | ACC | ANTI), ("FJ_ALGO_BUILD_ORDER cannot be combined with FJ_ALGO_ANTI",)),
    ("full", dict(algo=BO | REUSE | FULL), ("FJ_ALGO_BUILD_ORDER cannot be combined with FJ_ALGO_FULL_OUTER",)),
    ("all_copies", dict(algo=BO | REUSE | ALL), ("FJ_ALGO_BUILD_ORDER cannot be combined with FJ_ALGO_ALL_COPIES",)),
    ("probe_order", dict(algo=BO | REUSE | PO), ("FJ_ALGO_BUILD_ORDER cannot be combined with FJ_ALGO_PROBE_ORDER",)),
    ("group_by", dict(algo=BO | REUSE | GB, pk=None, n_p=0), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_BUILD_ORDER",)),
    ("count_only", dict(algo=BO | REUSE, materialize=0), ("materialize = 1",)),
    ("count_only_accumulate", dict(algo=BO | REUSE | ACC, materialize=0), ("materialize = 1",)),
    ("no_output", dict(algo=BO | REUSE, cnt=None, vals=None), ("FJ_ALGO_BUILD_ORDER", "needs an output")),
    ("no_output_accumulate", dict(algo=BO | REUSE | ACC, cnt=None, vals=None, pk=None, n_p=0), ("FJ_ALGO_BUILD_ORDER", "needs an output")),
    ("min_without_values_output", dict(algo=BO | REUSE | AMIN, vals=None), ("FJ_ALGO_AGG_MIN", "needs d_out_vals")),
    ("max_without_values_output", dict(algo=BO | REUSE | AMAX | ASIGNED | ACC, vals=None), ("FJ_ALGO_AGG_MAX", "needs d_out_vals")),
    ("values_output_without_value_column", dict(algo=BO | REUSE, pv=None), ("needs d_build_vals",)),
    ("misaligned_counts", dict(algo=BO | REUSE, cnt=0x40004), ("8-byte aligned",)),
    ("misaligned_values", dict(algo=BO | REUSE | ACC, vals=0x50001), ("8-byte aligned",)),
    ("min_and_max", dict(algo=BO | REUSE | AMIN | AMAX), ("FJ_ALGO_AGG_MIN cannot be combined with FJ_ALGO_AGG_MAX",)),
    ("signed_sum", dict(algo=BO | REUSE | ASIGNED), ("FJ_ALGO_AGG_SIGNED modifies",)),
    ("hash_top_bits", dict(algo=BO | REUSE, top=32), ("hash_top_bits must be 64 or 48",)),
]


@pytest.mark.parametrize("cid,kw,needles", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_invalid_combinations_are_refused_before_any_device_work(cid, kw, needles):
    """A NULL context: the checks come before the context is touched (no GPU needed; the pointers are never dereferenced)."""
    rc, err = _device_call(**kw)
    assert rc != 0 and "null context" not in err, err
    for needle in needles:
        assert needle in err, err


VALID = [   # id, keyword arguments of _device_call
    ("count", dict(algo=BO | REUSE, pv=None, vals=None)),
    ("count_with_a_value_column", dict(algo=BO | REUSE | 1, vals=None)),
    ("sum", dict(algo=BO | REUSE | 2, cnt=None)),
    ("sum_and_counts", dict(algo=BO | REUSE)),
    ("min_unsigned", dict(algo=BO | REUSE | AMIN, cnt=None)),
    ("min_signed", dict(algo=BO | REUSE | AMIN | ASIGNED)),
    ("max_unsigned", dict(algo=BO | REUSE | AMAX)),
    ("max_signed", dict(algo=BO | REUSE | AMAX | ASIGNED | 2, cnt=None)),
    ("count_accumulate", dict(algo=BO | REUSE | ACC, pv=None, vals=None)),
    ("sum_accumulate", dict(algo=BO | REUSE | ACC, cnt=None)),
    ("sum_and_counts_accumulate", dict(algo=BO | REUSE | ACC | 1)),
    ("min_unsigned_accumulate", dict(algo=BO | REUSE | ACC | AMIN)),
    ("min_signed_accumulate", dict(algo=BO | REUSE | ACC | AMIN | ASIGNED, cnt=None)),
    ("max_unsigned_accumulate", dict(algo=BO | REUSE | ACC | AMAX, cnt=None)),
    ("max_signed_accumulate", dict(algo=BO | REUSE | ACC | AMAX | ASIGNED)),
    ("no_probe_rows", dict(algo=BO | REUSE, pk=None, pv=None, n_p=0)),
    ("no_probe_rows_accumulate", dict(algo=BO | REUSE | ACC, pk=None, pv=None, n_p=0)),
    ("hash_top_bits_48", dict(algo=BO | REUSE, top=48)),
    ("capacity_is_checked_on_the_context", dict(algo=BO | REUSE, cap=0)),
]


@pytest.mark.parametrize("cid,kw", VALID, ids=[v[0] for v in VALID])
def test_valid_combinations_reach_the_context(cid, kw):
    rc, err = _device_call(**kw)
    assert rc != 0 and "null context" in err, err


HOST = [   # id, algo, needles
    ("count", BO | REUSE, ("FJ_ALGO_REUSE_BUILD", "fj_join_device")),
    ("sum_accumulate", BO | REUSE | ACC | 2, ("FJ_ALGO_REUSE_BUILD", "FJ_ALGO_ACCUMULATE", "fj_join_device")),
    ("min_signed", BO | REUSE | AMIN | ASIGNED, ("FJ_ALGO_REUSE_BUILD", "fj_join_device")),
    ("accumulate_without_reuse", BO | ACC, ("unknown algo",)),
    ("retain", BO | RETAIN, ("unknown algo",)),
]


@pytest.mark.parametrize("cid,algo,needles", HOST, ids=[r[0] for r in HOST])
def test_host_entry_refuses_both_combinations(cid, algo, needles):
    from flash_hash_join_amd import _lib
    L = _lib.load()
    k = np.arange(8, dtype=np.uint64)
    cnt, sec = ctypes.c_uint64(0), ctypes.c_double(0)
    oc, ov = ctypes.c_void_p(), ctypes.c_void_p()
    rc = L.fj_join_host(algo, 0, 1, k.ctypes.data, k.ctypes.data, 8, k.ctypes.data, 8, ctypes.byref(cnt), ctypes.byref(sec), ctypes.byref(oc), ctypes.byref(ov))
    err = _lib.last_error()
    assert rc != 0 and "null context" not in err and "HIP device" not in err, err
    for needle in needles:
        assert needle in err, err
    assert not oc.value and not ov.value


def test_python_argument_errors():
    import torch
    from flash_hash_join_amd import api
    k = np.arange(6, dtype=np.uint64)
    closed = api.Index(None, 0, 4, 4, False)                             # (no context behind it: what a closed index is; keys only)
    good = np.zeros(4, np.int64)
    calls = {
        "count": lambda **kw: closed.group_count(k, **kw),
        "sum": lambda **kw: closed.group_sum(k, k, **kw),
        "min": lambda **kw: closed.group_min(k, k, **kw),
        "max": lambda **kw: closed.group_max(k, k, signed=False, **kw),
    }
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match="closed"):                # valid arguments: the call reaches the index, which is closed
            call()
        with pytest.raises(RuntimeError, match="closed"):
            call(out=good)
        with pytest.raises(ValueError, match="4 rows"):                  # wrong size
            call(out=np.zeros(5, np.int64))
        with pytest.raises(ValueError, match="4 rows"):
            call(out=np.zeros((2, 2), np.int64))
        with pytest.raises(TypeError, match="int64"):                    # wrong dtype
            call(out=np.zeros(4, np.float64))
        with pytest.raises(TypeError, match="int64"):
            call(out=np.zeros(4, np.int32))
        with pytest.raises(TypeError, match="NumPy array"):              # wrong kind: NumPy keys, another container
            call(out=torch.zeros(4, dtype=torch.int64))
        with pytest.raises(TypeError, match="NumPy array"):
            call(out=[0, 0, 0, 0])
        with pytest.raises(ValueError, match="C-contiguous"):
            call(out=np.zeros(8, np.int64)[::2])
        ro = np.zeros(4, np.int64)
        ro.flags.writeable = False
        with pytest.raises(ValueError, match="writable"):
            call(out=ro)
        if name == "count":
            continue
        with pytest.raises(ValueError, match="together"):                # one flag covers the call
            call(counts_out=good.copy())
        with pytest.raises(ValueError, match="together"):
            call(out=good, return_counts=True)
        with pytest.raises(ValueError, match="4 rows"):
            call(out=good, counts_out=np.zeros(3, np.int64))
        with pytest.raises(RuntimeError, match="closed"):                # counts_out implies return_counts; uint64 storage is accepted
            call(out=good, counts_out=np.zeros(4, np.uint64))
    for meth in (closed.group_sum, closed.group_min, closed.group_max):
        with pytest.raises(ValueError, match="probe_values has 5 elements, probe_keys has 6"):
            meth(k, k[:5])
        with pytest.raises(ValueError, match="probe_values is required"):
            meth(k, None)
        with pytest.raises(RuntimeError, match="closed"):                # longer is fine: the first len(probe_keys) words are read
            meth(k[:5], k)
    with pytest.raises(TypeError, match="signed"):
        closed.group_min(k, k, signed=1)
    with pytest.raises(TypeError, match="cannot convert dtype"):
        closed.group_count(np.array(["a"]))


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fj():
    import flash_join
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_device_count() >= 1, "no HIP device: the product path must not silently fall back"
    assert flash_join.initialize() is None
    return flash_join


def _prior(form, nb, prior):
    if prior is not None:
        return np.asarray(prior).view(np.uint64).copy()
    return np.full(nb, np.uint64(IDENT[form]), dtype=np.uint64)


def ref_group(form, nb, idx_hit, pv_hit, prior=None):
    """the uint64 words of the aggregate at every build row: combined into `prior` (default: the identity) at the first-occurrence rows"""
    out = _prior(form, nb, prior)
    if form == "count":
        np.add.at(out, idx_hit, np.uint64(1))
    elif form == "sum":
        np.add.at(out, idx_hit, pv_hit)                                   # (uint64: wraps modulo 2^64)
    elif form == "min_u":
        np.minimum.at(out, idx_hit, pv_hit)
    elif form == "max_u":
        np.maximum.at(out, idx_hit, pv_hit)
    elif form == "min_s":
        np.minimum.at(out.view(np.int64), idx_hit, pv_hit.view(np.int64))
    else:
        np.maximum.at(out.view(np.int64), idx_hit, pv_hit.view(np.int64))
    return out


def _values(n, seed):
    """full-range words (sums wrap, both signs occur), the four extremes among them"""
    pv = np.random.default_rng(seed).integers(0, 2**64, size=n, dtype=np.uint64)
    if n >= 16:
        pv[5:9] = np.array([0, I64_MAX, I64_MIN_U, U64_MAX], dtype=np.uint64)
    return pv


class GBatch:
    """a probe batch with values and the references of all six forms, computed once and never changed"""
    def __init__(self, bk, pk, seed):
        self.pk, self.pv, self.nb = pk, _values(pk.size, seed), bk.size
        hit, idx = TP.ref_probe_order(bk, pk)
        self.hit, self.idx = hit, idx
        self.m = int(hit.sum())
        self.ih, self.vh = idx[hit], self.pv[hit]
        self._ref, self._dev = {}, None

    def ref(self, form):
        if form not in self._ref:
            self._ref[form] = ref_group(form, self.nb, self.ih, self.vh)
            self._ref[form].flags.writeable = False
        return self._ref[form]

    def ref_onto(self, form, prior):
        return ref_group(form, self.nb, self.ih, self.vh, prior)

    def inputs(self, device):
        if not device:
            return self.pk, self.pv
        if self._dev is None:
            self._dev = (TP._cuda(self.pk), TP._cuda(self.pv))
        return self._dev


class GCase:
    def __init__(self, case, seed=11):
        self.case, self.bk = case, case.bk
        self.batches = [GBatch(case.bk, b.pk, seed + i) for i, b in enumerate(case.batches)]

    def build(self, device):
        return self.case.build(device)


@functools.lru_cache(maxsize=None)
def _gplan(cid, dups):
    return GCase(TP._plan_case(cid, dups))


def _u64(a, device):
    """an output as uint64 words on the host; its container is checked on the way"""
    if device:
        assert a.is_cuda and str(a.dtype) == "torch.int64", a.dtype
        return a.cpu().numpy().view(np.uint64)
    assert isinstance(a, np.ndarray) and a.dtype in (np.int64, np.uint64), a.dtype
    return a.view(np.uint64)


def call(index, form, pk, pv, out=None, counts=False, counts_out=None):
    """(m, values or None, counts or None) of the Index method of `form`, as returned"""
    if form == "count":
        m, sec, c = index.group_count(pk, out=out)
        assert isinstance(m, int) and isinstance(sec, float)
        return m, None, c
    if form == "sum":
        r = index.group_sum(pk, pv, out=out, return_counts=counts, counts_out=counts_out)
    else:
        meth = index.group_min if form.startswith("min") else index.group_max
        r = meth(pk, pv, out=out, return_counts=counts, counts_out=counts_out, signed=form.endswith("_s"))
    assert len(r) == (4 if counts or counts_out is not None else 3)
    return r[0], r[2], (r[3] if len(r) == 4 else None)


def check_gbatch(fj, index, b, device, after=None, one_shot=None, forms=FORMS):
    """the count form alone, every value form alone and together with the counts against the reference; one_shot = build keys: also
    bit-identical to group_join_* on the same inputs (unique build keys)"""
    pk, pv = b.inputs(device)
    note = (lambda fn: after(fn, fj.last_timings())) if after else (lambda fn: None)
    for form in forms:
        m, v, c = call(index, form, pk, pv)
        note(form)
        got = _u64(c if form == "count" else v, device)
        assert got.shape == (b.nb,) and m == b.m, (form, m, b.m)
        assert np.array_equal(got, b.ref(form)), f"{form}: not the aggregate at the key's FIRST build row / the identity elsewhere"
        if form == "count":
            assert int(got.sum()) == b.m
            continue
        m, v2, c2 = call(index, form, pk, pv, counts=True)
        note(form + "+counts")
        assert m == b.m and np.array_equal(_u64(v2, device), b.ref(form)) and np.array_equal(_u64(c2, device), b.ref("count")), form + " with counts"
    if one_shot is not None:
        for form in forms:
            if form == "count":
                P, _, c1 = fj.group_join_count(one_shot, pk)
                v1 = c1
            elif form == "sum":
                P, _, v1, c1 = fj.group_join_sum(one_shot, pk, pv, return_counts=True)
            else:
                fn = fj.group_join_min if form.startswith("min") else fj.group_join_max
                P, _, v1, c1 = fn(one_shot, pk, pv, return_counts=True, signed=form.endswith("_s"))
            assert P == b.m and np.array_equal(_u64(v1, device), b.ref(form)) and np.array_equal(_u64(c1, device), b.ref("count")), "one-shot " + form


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("dups", [True, False], ids=["dups", "unique"])
@pytest.mark.parametrize("cid", [c[0] for c in TP.CASES])
def test_every_plan_against_the_reference_and_the_one_shot_functions(fj, cid, dups, device):
    """np = 0, a batch smaller than a chunk and a batch larger than nb (partitions cut into several items) on the plan the build side's
    size chose; a keys-only index (no build value is read)"""
    _, nb, target, passes, _ = next(c for c in TP.CASES if c[0] == cid)
    g = _gplan(cid, dups)

    def after(fn, lt):
        assert lt["build_phase_ms"] == 0.0 and lt["emit_ms"] == 0.0, (fn, lt)
        if passes is not None:
            assert lt["path"] == 0 and lt["fell_back"] == 0 and passes(lt["passes"]), (fn, lt)
    bk = g.build(device)[0]
    fj.set_option("plan_target_keys", target)
    try:
        with fj.build_index(bk) as index:
            assert index.num_rows == g.bk.size and not index.has_values
            for b in g.batches:
                check_gbatch(fj, index, b, device, after=after, one_shot=None if dups else bk)
    finally:
        fj.set_option("plan_target_keys", 4096)


@functools.lru_cache(maxsize=1)
def _goversized():
    return GCase(TP._oversized_case(), seed=23)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_partitions_beyond_the_lds_table_aggregate_on_the_hbm_table_form(fj, device):
    g = _goversized()

    def after(fn, lt):
        assert lt["path"] == 1 and lt["fell_back"] == 0 and lt["passes"] == 0 and lt["build_phase_ms"] == 0.0, (fn, lt)
    with fj.build_index(*g.build(device)) as index:
        lt = fj.last_timings()
        assert lt["fell_back"] == 1 and lt["path"] == 1, lt
        for b in g.batches:
            check_gbatch(fj, index, b, device, after=after)


def _hbm_index(fj, how, bk, bv=None):
    """an index in the HBM-table form by an option read when the side is prepared"""
    from flash_hash_join_amd import _lib, api
    n = bk.numel() if hasattr(bk, "numel") else bk.size
    if how == "radix_threshold":
        fj.set_option("radix_threshold", n + 1)
        try:
            index = fj.build_index(bk, bv)
        finally:
            fj.set_option("radix_threshold", 0)
    else:                                                                 # scalar_hbm_table = 1 speaks to FJ_ALGO_SCALAR: through the C ABI on the index's context
        import torch
        assert hasattr(bk, "data_ptr"), "device tensors"
        index = fj.build_index(bk[:1])
        cnt, t = ctypes.c_uint64(0), _lib.FjTimings()
        fj.set_option("scalar_hbm_table", 1)
        try:
            _lib.check(_lib.load().fj_join_device(index._ctx, api.ALGO_SCALAR | PO | RETAIN, 0, 1, bk.data_ptr(), None, n, None, 0,
                                                  torch.cuda.current_stream(0).cuda_stream, 64, ctypes.byref(cnt), None, None, 0, ctypes.byref(t)))
        finally:
            fj.set_option("scalar_hbm_table", 0)
        assert t.path == 1 and t.fell_back == 0
        index.num_rows, index.num_keys = n, int(cnt.value)
    return index


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("how", ["scalar_hbm_table", "radix_threshold"])
def test_the_options_that_choose_the_hbm_table_form(fj, how, device):
    g = _gplan("one_pass", True)

    def after(fn, lt):
        assert lt["path"] == 1 and lt["passes"] == 0 and lt["build_phase_ms"] == 0.0, (fn, lt)
    with _hbm_index(fj, how, g.build(True)[0] if how == "scalar_hbm_table" else g.build(device)[0]) as index:
        assert index.num_keys == np.unique(g.bk).size
        for b in g.batches:
            check_gbatch(fj, index, b, device, after=after)


@functools.lru_cache(maxsize=None)
def _gspecial(nb, n_p, arrangement):
    return GCase(TP._special_case(nb, n_p, arrangement), seed=31)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("arrangement", ["both", "build_only", "probe_only"])
@pytest.mark.parametrize("depth,nb,n_p,passes", [("zero_pass", 3000, 50_000, 0), ("one_pass", 100_000, 200_000, 1), ("hbm_table", 3000, 50_000, None)],
                         ids=["zero_pass", "one_pass", "hbm_table"])
def test_special_keys(fj, depth, nb, n_p, passes, arrangement, device):
    """raw 0, raw 2^64 - 1, the LDS tables' empty marker and the filler on the build side, the probe side and both"""
    g = _gspecial(nb, n_p, arrangement)
    S = np.array([0, U64_MAX, keymix.EMPTY_RAW, keymix.FILLER_RAW], dtype=np.uint64)
    assert np.isin(S, g.bk).all() == (arrangement != "probe_only") and np.isin(S, g.batches[0].pk).all() == (arrangement != "build_only")

    def after(fn, lt):
        assert lt["build_phase_ms"] == 0.0 and lt["path"] == (1 if passes is None else 0) and lt["passes"] == (passes or 0), (fn, lt)
    bk = g.build(device)[0]
    with (_hbm_index(fj, "radix_threshold", bk) if passes is None else fj.build_index(bk)) as index:
        check_gbatch(fj, index, g.batches[0], device, after=after)


def _buffer(words, device):
    return TP._cuda(words) if device else words.view(np.int64).copy()


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("table", ["lds", "hbm"])
def test_three_batches_under_out_equal_one_call_on_their_concatenation(fj, table, form, device):
    """a running aggregate: the first call makes the buffers, the next two combine into them (counts beside every value form)"""
    g = _gplan("one_pass", True)
    parts = [g.batches[2], g.batches[1], g.batches[2]]
    whole = _whole(g)
    bk = g.build(device)[0]
    with (_hbm_index(fj, "radix_threshold", bk) if table == "hbm" else fj.build_index(bk)) as index:
        acc = cacc = None
        total = 0
        for i, b in enumerate(parts):
            pk, pv = b.inputs(device)
            if form == "count":
                m, _, c = call(index, form, pk, pv, out=acc)
                assert i == 0 or c is acc
                acc = c
            else:
                m, v, c = call(index, form, pk, pv, out=acc, counts=i == 0, counts_out=cacc)
                assert i == 0 or (v is acc and c is cacc), "out= and counts_out= are returned"
                acc, cacc = v, c
            assert m == b.m, "the count of THIS call"
            total += m
        m1, v1, c1 = call(index, form, *whole.inputs(device), counts=form != "count")
        assert m1 == total == whole.m
        assert np.array_equal(_u64(acc, device), whole.ref(form)) and np.array_equal(_u64(c1 if form == "count" else v1, device), whole.ref(form))
        if form != "count":
            assert np.array_equal(_u64(cacc, device), whole.ref("count")) and np.array_equal(_u64(c1, device), whole.ref("count"))


@functools.lru_cache(maxsize=1)
def _whole_cached():
    g = _gplan("one_pass", True)
    parts = [g.batches[2], g.batches[1], g.batches[2]]
    w = GBatch.__new__(GBatch)
    w.pk, w.pv, w.nb = np.concatenate([p.pk for p in parts]), np.concatenate([p.pv for p in parts]), g.bk.size
    w.ih, w.vh = np.concatenate([p.ih for p in parts]), np.concatenate([p.vh for p in parts])
    w.m, w._ref, w._dev = sum(p.m for p in parts), {}, None
    return w


def _whole(g):
    return _whole_cached()


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("table", ["lds", "hbm"])
def test_prior_contents_under_out_and_none_without_it(fj, table, device):
    """out=: rows without a partner keep what they held, the others combine with it - a prior value below AND above the batch's for
    min / max (full-range random words on both sides); no out=: the library fills, two calls are independent"""
    g = _gplan("one_pass", True)
    b, b2 = g.batches[2], g.batches[1]
    pk, pv = b.inputs(device)
    rng = np.random.default_rng(77)
    bk = g.build(device)[0]
    with (_hbm_index(fj, "radix_threshold", bk) if table == "hbm" else fj.build_index(bk)) as index:
        for form in FORMS:
            prior = rng.integers(0, 2**64, size=b.nb, dtype=np.uint64)
            cprior = rng.integers(0, 2**40, size=b.nb, dtype=np.uint64)
            exp, cexp = b.ref_onto(form, prior), b.ref_onto("count", cprior)
            if form.startswith("m"):
                took = exp != prior
                assert took.any() and (~took & (b.ref("count") > 0)).any(), "the batch wins in some rows and the prior value in others"
            no_partner = b.ref("count") == 0
            assert no_partner.any() and np.array_equal(exp[no_partner], prior[no_partner])
            out, cout = _buffer(prior, device), _buffer(cprior, device)
            if form == "count":
                m, _, c = call(index, form, pk, pv, out=out)
                assert m == b.m and c is out and np.array_equal(_u64(out, device), exp)
            else:
                m, v, c = call(index, form, pk, pv, out=out, counts_out=cout)
                assert m == b.m and v is out and c is cout
                assert np.array_equal(_u64(out, device), exp), form + ": prior contents"
                assert np.array_equal(_u64(cout, device), cexp), form + ": prior counts"
                m, v = call(index, form, pk, pv, out=out)[:2]             # ... and once more without counts: idempotent for min / max, added again for the sum
                assert np.array_equal(_u64(v, device), b.ref_onto(form, exp))
            # no out=: fresh results, nothing left over from the calls above or from each other
            m, v, c = call(index, form, pk, pv, counts=form != "count")
            first = _u64(c if form == "count" else v, device).copy()
            m2, v2, c2 = call(index, form, *b2.inputs(device), counts=form != "count")
            second = _u64(c2 if form == "count" else v2, device)
            assert m == b.m and m2 == b2.m and np.array_equal(first, b.ref(form)) and np.array_equal(second, b2.ref(form)), form + ": accumulated without out="
            assert np.array_equal(_u64(c if form == "count" else v, device), first), "the first result changed under the second call"
        # np == 0 under out=: nothing is touched
        prior = rng.integers(0, 2**64, size=b.nb, dtype=np.uint64)
        out = _buffer(prior, device)
        m, v, _ = call(index, "min_s", *g.batches[0].inputs(device), out=out)
        assert m == 0 and v is out and np.array_equal(_u64(out, device), prior)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("table", ["lds", "hbm"])
def test_values_at_the_extremes_and_the_sign_of_the_container(fj, table, device):
    """0, 2^63 - 1, 2^63 and 2^64 - 1 under both signednesses; a true aggregate that equals the identity is told apart by the counts"""
    ext = np.array([0, I64_MAX, I64_MIN_U, U64_MAX], dtype=np.uint64)
    rng = np.random.default_rng(3)
    bk = np.unique(rng.integers(0, 2**64, size=300, dtype=np.uint64))[:256]
    rng.shuffle(bk)
    bk = np.concatenate([bk, bk[:16]])                                    # 16 duplicated keys: their copies hold the identity
    pk = np.concatenate([bk[:4], rng.choice(bk[8:200], 3000), rng.integers(0, 2**64, size=500, dtype=np.uint64)])   # keys 0..3: one row each
    pv = np.concatenate([ext, rng.choice(ext, 3500)])
    b = GBatch.__new__(GBatch)
    b.pk, b.pv, b.nb, b._ref, b._dev = pk, pv, bk.size, {}, None
    b.hit, b.idx = TP.ref_probe_order(bk, pk)
    b.m, b.ih, b.vh = int(b.hit.sum()), b.idx[b.hit], pv[b.hit]
    for form in ("min_u", "min_s", "max_u", "max_s"):
        alike = (b.ref(form) == np.uint64(IDENT[form]))
        assert (alike & (b.ref("count") > 0)).any() and (alike & (b.ref("count") == 0)).any(), form
    dbk = TP._cuda(bk) if device else bk
    with (_hbm_index(fj, "radix_threshold", dbk) if table == "hbm" else fj.build_index(dbk)) as index:
        check_gbatch(fj, index, b, device)
        # signed=None: a uint64 NumPy column compares unsigned, int64 (NumPy, torch) signed
        dpk, dpv = b.inputs(device)
        m, _, v = index.group_min(dpk, dpv)
        assert np.array_equal(_u64(v, device), b.ref("min_u" if not device else "min_s"))
        m, _, v = index.group_max(dpk, dpv if device else pv.view(np.int64))
        assert np.array_equal(_u64(v, device), b.ref("max_s"))
        m, _, v = index.group_max(dpk, dpv, signed=False)
        assert np.array_equal(_u64(v, device), b.ref("max_u"))


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("table", ["lds", "hbm"])
def test_one_hot_key(fj, table, device):
    """one key carries half of a 200 000-row batch (one accumulator, one output word): correctness only"""
    g = _gplan("one_pass", True)
    base = g.batches[2]
    pk = base.pk[:200_000].copy()
    pk[::2] = g.bk[4]                                                     # (a duplicated build key: its first row takes all of it)
    b = GBatch(g.bk, pk, 41)
    assert int(b.ref("count").max()) >= 100_000
    bk = g.build(device)[0]
    with (_hbm_index(fj, "radix_threshold", bk) if table == "hbm" else fj.build_index(bk)) as index:
        check_gbatch(fj, index, b, device)


def _raw_group(index, algo, pk, pv, cnt_t, val_t, cap, top=64):
    """fj_join_device on the index's own context, device tensors in and out: rc, *out_count, timings"""
    import torch
    from flash_hash_join_amd import _lib
    c, t = ctypes.c_uint64(0), _lib.FjTimings()
    rc = _lib.load().fj_join_device(index._ctx, algo, 0, 1, None, pv.data_ptr() if pv is not None else None, 0, pk.data_ptr(), pk.numel(),
                                    torch.cuda.current_stream(0).cuda_stream, top, ctypes.byref(c),
                                    cnt_t.data_ptr() if cnt_t is not None else None, val_t.data_ptr() if val_t is not None else None, cap, ctypes.byref(t))
    return rc, int(c.value), t


@pytest.mark.gpu
@pytest.mark.parametrize("table", ["lds", "hbm"])
def test_guard_words_around_the_outputs_and_behind_the_values(fj, table):
    """out is a slice of a larger buffer with sentinel words on both sides; probe_values is longer than probe_keys; through the C ABI
    the filling call defines every word below NB of a poisoned buffer and nothing else"""
    import torch
    from flash_hash_join_amd import _lib
    g = _gplan("one_pass", True)
    b = g.batches[2]
    nb = b.nb
    pk, pv = b.inputs(True)
    word = int(np.array(A5, dtype=np.uint64).view(np.int64))
    pv_long = torch.cat([pv, torch.full((4096,), word, dtype=torch.int64, device="cuda")])
    bk = g.build(True)[0]
    with (_hbm_index(fj, "radix_threshold", bk) if table == "hbm" else fj.build_index(bk)) as index:
        for form in ("sum", "min_s", "max_u"):
            big, cbig = (torch.full((64 + nb + 64,), word, dtype=torch.int64, device="cuda") for _ in range(2))
            prior = np.full(nb, np.uint64(IDENT[form]), dtype=np.uint64)
            big[64:64 + nb] = TP._cuda(prior)
            cbig[64:64 + nb] = 0
            m, v, c = call(index, form, pk, pv_long, out=big[64:64 + nb], counts_out=cbig[64:64 + nb])
            hv, hc = big.cpu().numpy().view(np.uint64), cbig.cpu().numpy().view(np.uint64)
            assert m == b.m and np.array_equal(hv[64:64 + nb], b.ref(form)) and np.array_equal(hc[64:64 + nb], b.ref("count")), form
            for h in (hv, hc):
                assert np.all(h[:64] == A5) and np.all(h[64 + nb:] == A5), "a guard word was written"
            # NumPy: a slice of a larger array is combined into in place, its neighbours stay
            nbig = np.full(64 + nb + 64, A5, dtype=np.uint64)
            nbig[64:64 + nb] = prior
            m, v = call(index, form, b.pk, np.concatenate([b.pv, np.full(100, A5)]), out=nbig[64:64 + nb])[:2]
            assert m == b.m and np.array_equal(nbig[64:64 + nb], b.ref(form)) and np.all(nbig[:64] == A5) and np.all(nbig[64 + nb:] == A5)
        # the C ABI, no FJ_ALGO_ACCUMULATE, out_capacity = NB exactly: poisoned buffers are filled by the library
        for algo, form in ((BO | REUSE, "sum"), (BO | REUSE | AMIN | ASIGNED | 2, "min_s"), (BO | REUSE | AMAX | ASIGNED | 1, "max_s")):
            big, cbig = (torch.full((64 + nb + 64,), word, dtype=torch.int64, device="cuda") for _ in range(2))
            rc, m, t = _raw_group(index, algo, pk, pv_long, cbig[64:64 + nb], big[64:64 + nb], nb)
            assert rc == 0, _lib.last_error()
            hv, hc = big.cpu().numpy().view(np.uint64), cbig.cpu().numpy().view(np.uint64)
            assert m == b.m and t.build_phase_ms == 0.0 and t.path == (1 if table == "hbm" else 0)
            assert np.array_equal(hv[64:64 + nb], b.ref(form)) and np.array_equal(hc[64:64 + nb], b.ref("count")), form
            for h in (hv, hc):
                assert np.all(h[:64] == A5) and np.all(h[64 + nb:] == A5), "a guard word was written"
        # refused on the context, which stays usable
        cnt_t = torch.zeros(nb, dtype=torch.int64, device="cuda")
        rc, _, _ = _raw_group(index, BO | REUSE, pk, None, cnt_t, None, nb - 1)
        assert rc != 0 and "output capacity" in _lib.last_error(), _lib.last_error()
        rc, _, _ = _raw_group(index, BO | REUSE | ACC, pk, None, cnt_t, None, nb, top=48)
        assert rc != 0 and "hash_top_bits" in _lib.last_error(), _lib.last_error()
        assert not cnt_t.any()
        rc, m, _ = _raw_group(index, BO | REUSE | ACC, pk, None, cnt_t, None, nb)
        assert rc == 0 and m == b.m and np.array_equal(cnt_t.cpu().numpy().view(np.uint64), b.ref("count")), _lib.last_error()
    L = _lib.load()
    ctx = L.fj_ctx_create(0)
    try:
        index = type("Bare", (), {"_ctx": ctx})
        rc, _, _ = _raw_group(index, BO | REUSE, pk, None, cnt_t, None, nb)
        assert rc != 0 and "without a prepared build side" in _lib.last_error(), _lib.last_error()
    finally:
        L.fj_ctx_destroy(ctx)


@pytest.mark.gpu
def test_isolation_from_lookups_one_shot_joins_and_a_second_index(fj):
    """lookup / isin / lookup_indices before and after group calls are bit-identical (the prepared planes are read, never written); a
    one-shot join on the default context in between disturbs nothing; two live indexes are aggregated alternately"""
    ga, gz = _gplan("one_pass", True), _gplan("zero_pass", False)
    ia, iz = fj.build_index(*ga.build(True)), fj.build_index(*gz.build(False))
    try:
        ba, bz = ga.batches[2], gz.batches[2]
        TP.check_batch(fj, ia, ga.case.batches[2], True)
        before = [x.clone() for x in ia.lookup(ba.inputs(True)[0], return_mask=True)[2:]] + [ia.lookup_indices(ba.inputs(True)[0])[2].clone()]
        acc = None
        for _ in range(2):
            check_gbatch(fj, ia, ba, True, forms=("count", "sum", "max_s"))
            check_gbatch(fj, iz, bz, False, forms=("count", "sum", "min_u"))
            P, _, c1 = fj.group_join_count(gz.build(True)[0], bz.inputs(True)[0])            # one-shot, the default context
            assert P == bz.m
            n, _ = fj.hash_join_count_radix(*ga.build(True), ba.inputs(True)[0])
            assert n == ba.m
            check_gbatch(fj, ia, ga.batches[1], False, forms=("min_s",))                     # (device-built, NumPy batch)
            check_gbatch(fj, iz, gz.batches[1], True, forms=("sum",))                        # (NumPy-built, device batch)
            m, v, _ = call(ia, "sum", *ba.inputs(True), out=acc)
            acc = v
        assert np.array_equal(_u64(acc, True), ba.ref_onto("sum", ba.ref("sum")))
        after = [x for x in ia.lookup(ba.inputs(True)[0], return_mask=True)[2:]] + [ia.lookup_indices(ba.inputs(True)[0])[2]]
        for x, y in zip(before, after):
            assert bool((x == y).all())
        TP.check_batch(fj, ia, ga.case.batches[2], True)
        TP.check_batch(fj, iz, gz.case.batches[2], False)
    finally:
        ia.close()
        iz.close()
    with pytest.raises(RuntimeError, match="closed"):
        ia.group_count(ba.pk)
