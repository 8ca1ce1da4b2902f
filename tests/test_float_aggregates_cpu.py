"""Float64 aggregates (FJ_ALGO_AGG_FLOAT, include/flashjoin.h; the float64= keyword of group_by_* / group_join_* / Index.group_*): the
part of the contract that needs no GPU - the flag's value and its Python mirror, the unchanged ABI, every refusal of the two C entry
points (a NULL context and pointers that are never dereferenced, as in tests/test_group_minmax.py) and the Python argument checks
that are decided before a native call."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

MANY, LEFT, ROW_IDS, PO, BO, GB = 0x10, 0x20, 0x80, 0x800, 0x1000, 0x40000
MIN, MAX, SIGNED, INVERSE = 0x4000, 0x8000, 0x10000, 0x100000
RETAIN, REUSE, ACC, FLOAT = 0x400000, 0x800000, 0x1000000, 0x2000000


def _header():
    return open(os.path.join(ROOT, "include", "flashjoin.h")).read()


def test_header_flag_and_python_mirror():
    hdr = _header()
    assert int(re.search(r"#define FJ_ALGO_AGG_FLOAT\s+(0x[0-9a-fA-F]+)", hdr).group(1), 16) == 0x2000000
    from flash_hash_join_amd import api
    assert api.ALGO_AGG_FLOAT == 0x2000000 == FLOAT
    doc = hdr[hdr.index("FJ_ALGO_AGG_FLOAT"):hdr.index("#define FJ_ALGO_AGG_FLOAT")]
    for word in ("binary64", "UNSPECIFIED ORDER", "-0.0", "NaN", "+infinity", "-infinity", "FJ_ALGO_AGG_SIGNED", "device memory"):
        assert word in doc, word
    # no other flag shares the bit
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    flags = {n: int(v, 16) for n, v in re.findall(r"#define (FJ_ALGO_[A-Z_]+)\s+(0x[0-9a-fA-F]+)", code)}
    assert [n for n, v in flags.items() if v & 0x2000000] == ["FJ_ALGO_AGG_FLOAT"]


def test_abi_version_symbol_count_and_the_unassigned_bit():
    hdr = _header()
    assert int(re.search(r"#define FJ_ABI_VERSION (\d+)", hdr).group(1)) == 8
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert len(set(re.findall(r"\b(fj_[a-z0-9_]+)\s*\(", code))) == 40
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_abi_version() == 8 and len(_lib.SYMBOLS) == 40
    for algo in (0x200000, BO | 0x200000, GB | 0x200000, BO | FLOAT | 0x200000, GB | FLOAT | MIN | 0x200000):
        rc, err = _device_call(algo=algo) if not algo & GB else _device_call(algo=algo, pk=None, n_p=0)
        assert rc != 0 and "unknown algo" in err and "null context" not in err, (hex(algo), err)


def _device_call(algo, materialize=1, pv=0x20000, counts=0x40000, vals=0x50000, cap=100, nb=100, n_p=1000, bk=0x10000, pk=0x30000):
    from flash_hash_join_amd import _lib
    cnt = ctypes.c_uint64(0)
    rc = _lib.load().fj_join_device(None, algo, 0, materialize, bk, pv, nb, pk, n_p, None, 64, ctypes.byref(cnt), counts, vals, cap, None)
    return rc, _lib.last_error()


_GBK = dict(pk=None, n_p=0)        # FJ_ALGO_GROUP_BY takes no probe side
_PREP = dict(bk=None, nb=0)        # FJ_ALGO_BUILD_ORDER | FJ_ALGO_REUSE_BUILD takes no build side
DEVICE_REFUSALS = [   # id, keyword arguments of _device_call, needles
    ("bare", dict(algo=FLOAT), ("unknown algo 33554432",)),
    ("bare_base_2", dict(algo=FLOAT | 2), ("unknown algo",)),
    ("bare_min", dict(algo=FLOAT | MIN), ("unknown algo",)),
    ("probe_order", dict(algo=PO | FLOAT, cap=1000), ("unknown algo",)),
    ("many", dict(algo=MANY | FLOAT), ("unknown algo",)),
    ("left", dict(algo=LEFT | FLOAT, cap=1000), ("unknown algo",)),
    ("probe_order_reuse", dict(algo=PO | REUSE | FLOAT, cap=1000, pv=None, **_PREP), ("unknown algo",)),
    ("bo_signed", dict(algo=BO | FLOAT | SIGNED), ("FJ_ALGO_AGG_FLOAT", "FJ_ALGO_AGG_SIGNED")),
    ("bo_min_signed", dict(algo=BO | FLOAT | MIN | SIGNED), ("FJ_ALGO_AGG_FLOAT", "FJ_ALGO_AGG_SIGNED")),
    ("bo_max_signed_base_2", dict(algo=BO | FLOAT | MAX | SIGNED | 2), ("FJ_ALGO_AGG_FLOAT", "FJ_ALGO_AGG_SIGNED")),
    ("bo_reuse_signed", dict(algo=BO | REUSE | FLOAT | MIN | SIGNED, **_PREP), ("FJ_ALGO_AGG_FLOAT", "FJ_ALGO_AGG_SIGNED")),
    ("bo_reuse_accumulate_signed", dict(algo=BO | REUSE | ACC | FLOAT | SIGNED, **_PREP), ("FJ_ALGO_AGG_FLOAT", "FJ_ALGO_AGG_SIGNED")),
    ("gb_signed", dict(algo=GB | FLOAT | SIGNED, **_GBK), ("FJ_ALGO_AGG_FLOAT", "FJ_ALGO_AGG_SIGNED")),
    ("gb_max_signed", dict(algo=GB | FLOAT | MAX | SIGNED, **_GBK), ("FJ_ALGO_AGG_FLOAT", "FJ_ALGO_AGG_SIGNED")),
    ("bo_row_ids", dict(algo=BO | FLOAT | ROW_IDS), ("FJ_ALGO_ROW_IDS",)),
    ("bo_inverse", dict(algo=BO | FLOAT | INVERSE), ("unknown algo",)),
    ("gb_row_ids", dict(algo=GB | FLOAT | ROW_IDS, **_GBK), ("FJ_ALGO_AGG_FLOAT", "FJ_ALGO_ROW_IDS")),
    ("gb_inverse", dict(algo=GB | FLOAT | INVERSE, **_GBK), ("FJ_ALGO_AGG_FLOAT", "FJ_ALGO_INVERSE")),
    ("gb_min_inverse", dict(algo=GB | FLOAT | MIN | INVERSE, **_GBK), ("FJ_ALGO_AGG_FLOAT", "FJ_ALGO_INVERSE")),
    ("bo_no_value_column", dict(algo=BO | FLOAT, pv=None), ("FJ_ALGO_AGG_FLOAT", "d_build_vals")),
    ("bo_counts_only", dict(algo=BO | FLOAT, pv=None, vals=None), ("FJ_ALGO_AGG_FLOAT", "d_build_vals")),
    ("bo_max_no_value_column", dict(algo=BO | FLOAT | MAX, pv=None), ("FJ_ALGO_AGG_FLOAT", "d_build_vals")),
    ("bo_reuse_no_value_column", dict(algo=BO | REUSE | FLOAT, pv=None, **_PREP), ("FJ_ALGO_AGG_FLOAT", "d_build_vals")),
    ("gb_no_value_column", dict(algo=GB | FLOAT, pv=None, **_GBK), ("FJ_ALGO_AGG_FLOAT", "d_build_vals")),
    ("gb_min_no_value_column", dict(algo=GB | FLOAT | MIN | 1, pv=None, **_GBK), ("FJ_ALGO_AGG_FLOAT", "d_build_vals")),
    ("bo_no_values_output", dict(algo=BO | FLOAT, vals=None), ("FJ_ALGO_AGG_FLOAT", "d_out_vals")),
    ("bo_min_no_values_output", dict(algo=BO | FLOAT | MIN | 2, vals=None), ("FJ_ALGO_AGG_FLOAT", "d_out_vals")),
    ("bo_reuse_no_values_output", dict(algo=BO | REUSE | FLOAT, vals=None, **_PREP), ("FJ_ALGO_AGG_FLOAT", "d_out_vals")),
    ("bo_reuse_accumulate_no_values_output", dict(algo=BO | REUSE | ACC | FLOAT | MAX, vals=None, **_PREP), ("FJ_ALGO_AGG_FLOAT", "d_out_vals")),
    # what the base flags refuse, with their present messages
    ("bo_min_and_max", dict(algo=BO | FLOAT | MIN | MAX), ("FJ_ALGO_AGG_MIN", "FJ_ALGO_AGG_MAX", "one aggregate per call")),
    ("gb_min_and_max", dict(algo=GB | FLOAT | MIN | MAX, **_GBK), ("FJ_ALGO_AGG_MIN", "FJ_ALGO_AGG_MAX", "one aggregate per call")),
    ("bo_retain", dict(algo=BO | RETAIN | FLOAT), ("unknown algo",)),
    ("bo_accumulate_without_reuse", dict(algo=BO | ACC | FLOAT), ("unknown algo",)),
    ("bo_materialize_0", dict(algo=BO | FLOAT, materialize=0), ("FJ_ALGO_BUILD_ORDER", "materialize = 1")),
    ("bo_capacity", dict(algo=BO | FLOAT | MIN, cap=99), ("output capacity",)),
    ("bo_misaligned_values", dict(algo=BO | FLOAT, vals=0x50004), ("8-byte aligned",)),
    ("gb_probe_side", dict(algo=GB | FLOAT), ("FJ_ALGO_GROUP_BY takes no probe side",)),
    ("bo_base_3", dict(algo=BO | FLOAT | 3), ("unknown algo",)),
]


@pytest.mark.parametrize("cid,kw,needles", DEVICE_REFUSALS, ids=[r[0] for r in DEVICE_REFUSALS])
def test_device_entry_refusals_before_any_device_work(cid, kw, needles):
    """A NULL context: the checks come before the context is touched (no GPU needed; the pointers are never dereferenced)."""
    rc, err = _device_call(**kw)
    assert rc != 0 and "null context" not in err, err
    for needle in needles:
        assert needle in err, err


VALID = ([(f"bo_{name}_{'counts' if cnt else 'alone'}_base{base}", dict(algo=BO | FLOAT | agg | base, counts=0x40000 if cnt else None))
          for name, agg in (("sum", 0), ("min", MIN), ("max", MAX)) for cnt in (False, True) for base in (0, 1, 2)] +
         [(f"gb_{name}_base{base}", dict(algo=GB | FLOAT | agg | base, **_GBK)) for name, agg in (("sum", 0), ("min", MIN), ("max", MAX)) for base in (0, 2)] +
         [(f"reuse_{name}{'_accumulate' if acc else ''}", dict(algo=BO | REUSE | FLOAT | agg | acc, **_PREP))
          for name, agg in (("sum", 0), ("min", MIN), ("max", MAX)) for acc in (0, ACC)])


@pytest.mark.parametrize("cid,kw", VALID, ids=[v[0] for v in VALID])
def test_valid_combinations_reach_the_context(cid, kw):
    rc, err = _device_call(**kw)
    assert rc != 0 and "null context" in err, err


HOST_REFUSALS = [   # id, algo, materialize, value column, probe side, want counts, want values, needles
    ("bare", FLOAT, 1, True, True, True, True, ("unknown algo 33554432",)),
    ("bare_max", FLOAT | MAX | 2, 1, True, True, True, True, ("unknown algo",)),
    ("probe_order", PO | FLOAT, 1, True, True, True, True, ("unknown algo",)),
    ("bo_signed", BO | FLOAT | SIGNED, 1, True, True, True, True, ("FJ_ALGO_AGG_FLOAT", "FJ_ALGO_AGG_SIGNED")),
    ("bo_min_signed", BO | FLOAT | MIN | SIGNED, 1, True, True, True, True, ("FJ_ALGO_AGG_FLOAT", "FJ_ALGO_AGG_SIGNED")),
    ("gb_signed", GB | FLOAT | SIGNED, 1, True, False, True, True, ("FJ_ALGO_AGG_FLOAT", "FJ_ALGO_AGG_SIGNED")),
    ("gb_max_signed", GB | FLOAT | MAX | SIGNED, 1, True, False, True, True, ("FJ_ALGO_AGG_FLOAT", "FJ_ALGO_AGG_SIGNED")),
    ("bo_row_ids", BO | FLOAT | ROW_IDS, 1, True, True, True, True, ("FJ_ALGO_ROW_IDS",)),
    ("bo_inverse", BO | FLOAT | INVERSE, 1, True, True, True, True, ("unknown algo",)),
    ("gb_row_ids", GB | FLOAT | ROW_IDS, 1, True, False, True, True, ("FJ_ALGO_AGG_FLOAT", "FJ_ALGO_ROW_IDS")),
    ("gb_inverse", GB | FLOAT | INVERSE, 1, True, False, True, True, ("FJ_ALGO_AGG_FLOAT", "FJ_ALGO_INVERSE")),
    ("bo_no_value_column", BO | FLOAT, 1, False, True, True, True, ("FJ_ALGO_AGG_FLOAT", "build_vals")),
    ("bo_min_no_value_column", BO | FLOAT | MIN, 1, False, True, True, True, ("FJ_ALGO_AGG_FLOAT", "build_vals")),
    ("gb_no_value_column", GB | FLOAT, 1, False, False, True, True, ("FJ_ALGO_AGG_FLOAT", "build_vals")),
    ("gb_max_no_value_column", GB | FLOAT | MAX, 1, False, False, True, True, ("FJ_ALGO_AGG_FLOAT", "build_vals")),
    ("bo_no_values_output", BO | FLOAT, 1, True, True, True, False, ("FJ_ALGO_AGG_FLOAT", "out_vals")),
    ("bo_max_no_values_output", BO | FLOAT | MAX, 1, True, True, True, False, ("FJ_ALGO_AGG_FLOAT", "out_vals")),
    ("bo_reuse", BO | REUSE | FLOAT, 1, True, True, True, True, ("FJ_ALGO_REUSE_BUILD", "is not served here")),
    ("bo_reuse_accumulate", BO | REUSE | ACC | FLOAT | MIN, 1, True, True, True, True, ("FJ_ALGO_ACCUMULATE", "is not served here")),
    ("bo_min_and_max", BO | FLOAT | MIN | MAX, 1, True, True, True, True, ("one aggregate per call",)),
    ("bo_materialize_0", BO | FLOAT, 0, True, True, True, True, ("FJ_ALGO_BUILD_ORDER", "materialize = 1")),
    ("unassigned_bit", BO | FLOAT | 0x200000, 1, True, True, True, True, ("unknown algo",)),
]


@pytest.mark.parametrize("cid,algo,materialize,vals,probe,want_counts,want_vals,needles", HOST_REFUSALS, ids=[r[0] for r in HOST_REFUSALS])
def test_host_entry_refusals(cid, algo, materialize, vals, probe, want_counts, want_vals, needles):
    """fj_join_host makes the same checks before its context is created (no GPU needed)."""
    from flash_hash_join_amd import _lib
    L = _lib.load()
    k = np.arange(8, dtype=np.uint64)
    cnt, sec = ctypes.c_uint64(0), ctypes.c_double(0)
    oc, ov = ctypes.c_void_p(), ctypes.c_void_p()
    rc = L.fj_join_host(algo, 0, materialize, k.ctypes.data, k.ctypes.data if vals else None, 8, k.ctypes.data if probe else None, 8 if probe else 0,
                        ctypes.byref(cnt), ctypes.byref(sec), ctypes.byref(oc) if want_counts else None, ctypes.byref(ov) if want_vals else None)
    err = _lib.last_error()
    assert rc != 0 and "null context" not in err and "HIP device" not in err, err
    for needle in needles:
        assert needle in err, err
    assert not oc.value and not ov.value


def test_the_two_entry_points_refuse_with_the_same_words():
    """identically in fj_join_device and fj_join_host: the text behind the function's name agrees for the float-specific refusals, up to
    the names of the arguments (d_build_vals / build_vals, d_out_vals / out_vals)"""
    from flash_hash_join_amd import _lib
    L = _lib.load()
    k = np.arange(8, dtype=np.uint64)

    def host(algo, vals=True, probe=True, want_vals=True):
        cnt, sec = ctypes.c_uint64(0), ctypes.c_double(0)
        oc, ov = ctypes.c_void_p(), ctypes.c_void_p()
        assert L.fj_join_host(algo, 0, 1, k.ctypes.data, k.ctypes.data if vals else None, 8, k.ctypes.data if probe else None, 8 if probe else 0,
                              ctypes.byref(cnt), ctypes.byref(sec), ctypes.byref(oc), ctypes.byref(ov) if want_vals else None) != 0
        return _lib.last_error().split(": ", 1)[1]

    def device(**kw):
        rc, err = _device_call(**kw)
        assert rc != 0
        return err.split(": ", 1)[1].replace("d_build_vals", "build_vals").replace("d_out_vals", "out_vals")
    assert host(BO | FLOAT | SIGNED) == device(algo=BO | FLOAT | SIGNED)
    assert host(GB | FLOAT | MIN | SIGNED, probe=False) == device(algo=GB | FLOAT | MIN | SIGNED, **_GBK)
    assert host(GB | FLOAT | ROW_IDS, probe=False) == device(algo=GB | FLOAT | ROW_IDS, **_GBK)
    assert host(GB | FLOAT | INVERSE, probe=False) == device(algo=GB | FLOAT | INVERSE, **_GBK)
    assert host(BO | FLOAT, vals=False) == device(algo=BO | FLOAT, pv=None)
    assert host(GB | FLOAT, vals=False, probe=False) == device(algo=GB | FLOAT, pv=None, **_GBK)
    assert host(BO | FLOAT, want_vals=False) == device(algo=BO | FLOAT, vals=None)


# ---- Python: what is decided before a native call ---------------------------------------------------------------------------------
K = np.arange(4, dtype=np.uint64)
F = np.array([0.5, -1.25, 3.0, 8.0])


def _module_calls(api):
    return {"group_by_sum": lambda v, **kw: api.group_by_sum(K, v, **kw),
            "group_by_min": lambda v, **kw: api.group_by_min(K, v, **kw),
            "group_by_max": lambda v, **kw: api.group_by_max(K, v, **kw),
            "group_join_sum": lambda v, **kw: api.group_join_sum(K, K, v, **kw),
            "group_join_min": lambda v, **kw: api.group_join_min(K, K, v, **kw),
            "group_join_max": lambda v, **kw: api.group_join_max(K, K, v, **kw)}


def _fake_index(api):
    """an Index object without a native context: the checks under test come before the context is looked at"""
    return api.Index(None, 0, 4, 4, False)


def _index_calls(api):
    idx = _fake_index(api)
    return {"Index.group_sum": lambda v, **kw: idx.group_sum(K, v, **kw),
            "Index.group_min": lambda v, **kw: idx.group_min(K, v, **kw),
            "Index.group_max": lambda v, **kw: idx.group_max(K, v, **kw)}


def test_the_nine_functions_take_the_keyword_and_it_defaults_to_false():
    import inspect
    import flash_join
    from flash_hash_join_amd import api
    fns = [getattr(api, n) for n in ("group_by_sum", "group_by_min", "group_by_max", "group_join_sum", "group_join_min", "group_join_max")]
    fns += [getattr(api.Index, n) for n in ("group_sum", "group_min", "group_max")]
    for fn in fns:
        p = inspect.signature(fn).parameters["float64"]
        assert p.default is False, fn
        for word in ("float64=True", "NaN"):
            assert word in fn.__doc__ or fn.__name__.endswith("_max"), (fn, word)
    for n in ("group_by_sum", "group_join_sum"):
        assert "UNSPECIFIED ORDER" in getattr(api, n).__doc__ and getattr(flash_join, n) is getattr(api, n)
    assert "UNSPECIFIED ORDER" in api.Index.group_sum.__doc__
    for fn in (api.group_by_min, api.group_join_min, api.Index.group_min):
        assert "-0.0" in fn.__doc__ and "unspecified" in fn.__doc__
    for name in ("group_count", "group_by_count", "group_join_count", "unique", "factorize"):      # no float form of the count forms
        fn = getattr(api, name, None) or getattr(api.Index, name)
        assert "float64" not in inspect.signature(fn).parameters, name


@pytest.mark.parametrize("bad", [np.arange(4, dtype=np.int64), np.arange(4, dtype=np.uint64), np.arange(4, dtype=np.int32),
                                 np.array([True, False, True, True]), np.array(["a", "b", "c", "d"]), np.arange(4, dtype=np.complex128),
                                 [1, 2, 3, 4]],
                         ids=["int64", "uint64", "int32", "bool", "str", "complex", "list_of_ints"])
def test_float64_needs_a_floating_point_column(bad):
    from flash_hash_join_amd import api
    for name, call in {**_module_calls(api), **_index_calls(api)}.items():
        with pytest.raises(TypeError, match="float64=True needs floating-point"):
            call(bad, float64=True)


def test_float64_refuses_integer_torch_tensors():
    import torch
    from flash_hash_join_amd import api
    for name, call in {**_module_calls(api), **_index_calls(api)}.items():
        for t in (torch.arange(4, dtype=torch.int64), torch.ones(4, dtype=torch.bool)):
            with pytest.raises(TypeError, match="float64=True needs floating-point"):
                call(t, float64=True)


@pytest.mark.parametrize("signed", [True, False, np.bool_(True), "yes", 0])
def test_float64_with_signed_is_a_type_error(signed):
    from flash_hash_join_amd import api
    calls = {**_module_calls(api), **_index_calls(api)}
    for name in [n for n in calls if not n.endswith("sum")]:
        with pytest.raises(TypeError, match="signed must be None with float64=True"):
            calls[name](F, float64=True, signed=signed)
    for name in [n for n in calls if n.endswith("sum")]:
        with pytest.raises(TypeError):                          # the sum forms have no such argument at all
            calls[name](F, float64=True, signed=signed)


def test_float64_keeps_the_required_arguments():
    from flash_hash_join_amd import api
    for name, call in {**_module_calls(api), **_index_calls(api)}.items():
        with pytest.raises(ValueError, match="is required"):
            call(None, float64=True)


def test_float_words_are_views_of_float64_and_exact_widenings():
    from flash_hash_join_amd.api import _as_float64, _float_words
    a = np.array([0.5, -0.0, np.inf, -np.inf, 5e-324, np.finfo(np.float64).max])
    w = _float_words("f", "values", a)
    assert w.dtype == np.uint64 and np.shares_memory(w, a) and w[1] == 1 << 63 and w[2] == 0x7FF0000000000000 and w[3] == 0xFFF0000000000000
    assert np.shares_memory(_as_float64(w), a) and np.array_equal(_as_float64(w), a)
    for narrow in (np.float32, np.float16):
        b = np.array([0.5, -1.25, 65504.0, -0.0, np.inf], dtype=narrow)
        w = _float_words("f", "values", b)
        assert w.dtype == np.uint64 and np.array_equal(w.view(np.float64), b.astype(np.float64)) and np.array_equal(w.view(np.float64).astype(narrow), b)
    import torch
    t = torch.tensor([0.5, -2.0, float("inf")], dtype=torch.float64)
    w = _float_words("f", "values", t)
    assert w.dtype == torch.int64 and w.data_ptr() == t.data_ptr() and _as_float64(w).data_ptr() == t.data_ptr()
    for narrow in (torch.float32, torch.float16, torch.bfloat16):
        t = torch.tensor([0.5, -1.25, 3.0], dtype=narrow)
        assert torch.equal(_float_words("f", "values", t).view(torch.float64), t.double())
    with pytest.raises(TypeError, match="float64=True needs floating-point"):
        _float_words("f", "values", np.array([1.0], dtype=np.longdouble) if np.dtype(np.longdouble).itemsize > 8 else np.array([1]))


def test_index_out_must_be_float64_before_any_native_call():
    """the index has no context: a native call would raise "this Index is closed", the checks under test come first"""
    import torch
    from flash_hash_join_amd import api
    idx = _fake_index(api)
    cnt = np.zeros(4, np.int64)
    for meth in (idx.group_sum, idx.group_min, idx.group_max):
        bad = [np.zeros(4, np.int64), np.zeros(4, np.uint64), np.zeros(4, np.float32), [0.0] * 4, torch.zeros(4, dtype=torch.float64),
               np.zeros(8, np.float64)[::2], np.zeros(4, np.int32)]
        ro = np.zeros(4, np.float64); ro.flags.writeable = False
        for out in bad + [ro]:
            with pytest.raises(TypeError, match="float64"):
                meth(K, F, float64=True, out=out)
            with pytest.raises(TypeError, match="float64"):
                meth(K, F, float64=True, out=out, counts_out=cnt)
        with pytest.raises(ValueError, match="the index has 4 rows"):
            meth(K, F, float64=True, out=np.zeros(5, np.float64))
        with pytest.raises(TypeError, match="counts_out must be int64"):                     # the counts stay integers
            meth(K, F, float64=True, out=np.zeros(4, np.float64), counts_out=np.zeros(4, np.float64))
        with pytest.raises(ValueError, match="out and counts_out are given together or not at all"):
            meth(K, F, float64=True, out=np.zeros(4, np.float64), return_counts=True)
        with pytest.raises(ValueError, match="out and counts_out are given together or not at all"):
            meth(K, F, float64=True, counts_out=cnt)
        with pytest.raises(RuntimeError, match="this Index is closed"):                      # a good accumulator reaches the native call
            meth(K, F, float64=True, out=np.zeros(4, np.float64), counts_out=cnt)
    # without the keyword a float64 accumulator is what it was: not an int64 buffer
    with pytest.raises(TypeError, match="out must be int64 or uint64"):
        idx.group_sum(K, K, out=np.zeros(4, np.float64))


def test_without_the_keyword_the_float_errors_are_the_old_ones():
    from flash_hash_join_amd import api
    for fn in (api.group_by_min, api.group_by_max):
        with pytest.raises(TypeError, match="values must be integers"):
            fn(K, F)
        with pytest.raises(TypeError, match="float64=True"):               # ... with a pointer to the keyword
            fn(K, F)
        with pytest.raises(TypeError, match="values must be integers"):
            fn(K, F, float64=False)
