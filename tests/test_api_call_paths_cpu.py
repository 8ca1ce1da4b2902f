"""The host halves of api.py's native-call paths, pinned without a GPU and without the library.

`api._lib.load` is replaced by a small fake library: plain Python with fj_join_host, fj_last_timings and fj_free_host (fj_join_device
raises - NumPy inputs never reach it).  The fake records the twelve arguments of every fj_join_host call, writes a scripted count
and the seconds through the pointers it was given, and points the two output pointers at NumPy arrays the test keeps alive.  Every
row asserts what reached the library - the algo word, which output pointers are None, the row-count argument, the addresses of the
input columns - and what came back: shapes, dtypes, contents, the pointers handed to fj_free_host and last_timings().

n = 6 rows and g = 3 groups: the smallest size at which n, g, P * g and n + g are all distinct; every caller also runs at n = 0, g = 0.

What a failing call does is pinned as it is: `check` raises on the non-zero return code BEFORE anything is read, so nothing is handed
to fj_free_host (the library sets no output pointer when it fails) and last_timings() stays what it was."""
import ctypes

import numpy as np
import pytest

from flash_hash_join_amd import api

TOTAL_MS, SECONDS = 12.5, 0.25
N, G = 6, 3
GROUP_BY = api.ALGO_ADAPTIVE | api.ALGO_GROUP_BY


def aligned(words, dtype=np.uint64):
    """a 16-byte aligned array: the host entry reads it in place, so its address is what reaches the library"""
    words = np.asarray(words, dtype=dtype)
    raw = np.empty(words.nbytes + 16, np.uint8)
    off = -raw.ctypes.data % 16
    a = raw[off:off + words.nbytes].view(dtype).reshape(words.shape)
    a[...] = words
    assert a.ctypes.data % 16 == 0
    return a


class FakeLib:
    """count: an int, or the tuple a full / all-copies join writes.  out0 / out1: what output pointers 11 and 12 are pointed at."""

    def __init__(self, count, out0=None, out1=None, rc=0):
        self.count, self.out, self.rc = count, [out0, out1], rc
        self.calls, self.freed, self.timings_read = [], [], 0

    def fj_join_host(self, *args):
        assert len(args) == 12
        self.calls.append(args)
        cnt = getattr(args[8], "_obj", args[8])              # byref(c_uint64), or the c_uint64 * 3 array itself
        if hasattr(cnt, "value"):
            cnt.value = self.count
        else:
            for i, c in enumerate(self.count if isinstance(self.count, tuple) else (self.count,)):
                cnt[i] = c
        args[9]._obj.value = SECONDS
        if self.rc == 0:
            for slot, arr in zip(args[10:], self.out):
                if slot is not None and arr is not None and arr.size:
                    slot._obj.value = arr.ctypes.data
        return self.rc

    def fj_last_timings(self, ref):
        self.timings_read += 1
        ref._obj.total_ms = TOTAL_MS
        return 0

    def fj_free_host(self, p):
        self.freed.append(p.value if isinstance(p, ctypes.c_void_p) else p)

    def fj_join_device(self, *args):
        raise AssertionError("a NumPy call reached fj_join_device")

    # -- what the rows ask ----------------------------------------------------------------------------------------------------------
    def only_call(self):
        assert len(self.calls) == 1
        return self.calls[0]

    def addresses(self):
        """what a successful call hands to fj_free_host: both output pointers, null (None) where none was asked for or nothing is held"""
        a = self.only_call()
        return [arr.ctypes.data if slot is not None and arr is not None and arr.size else None for slot, arr in zip(a[10:], self.out)]


@pytest.fixture
def install(monkeypatch):
    def _install(count, out0=None, out1=None, rc=0):
        fake = FakeLib(count, out0, out1, rc)
        monkeypatch.setattr(api._lib, "load", lambda: fake)
        monkeypatch.setattr(api._lib, "last_error", lambda: "scripted failure")
        monkeypatch.setattr(api, "_last", None)
        return fake
    return _install


def sent(fake, algo, n_rows, outputs, materialize=1):
    """the shared assertions on what reached the library; outputs: which of the two output pointers were passed"""
    a = fake.only_call()
    assert a[0] == algo, (hex(a[0]), hex(algo))
    assert a[1] == 0 and a[2] == materialize
    assert a[5] == n_rows
    assert (a[10] is not None, a[11] is not None) == outputs
    return a


def came_back_clean(fake):
    """both pointers went to fj_free_host, once each and in order; the timings were read once and published"""
    assert fake.freed == fake.addresses()
    assert fake.timings_read == 1
    assert api.last_timings()["total_ms"] == TOTAL_MS


def fails_as_ever(fake, call):
    """a non-zero return code raises through check; nothing is read, nothing freed, no timings published"""
    with pytest.raises(RuntimeError, match="scripted failure"):
        call()
    assert len(fake.calls) == 1
    assert fake.freed == [] and fake.timings_read == 0 and api.last_timings() is None


KEYS = [5, 7, 5, 9, 7, 5]
VALS = [10, 20, 30, 40, 50, 60]
GK = np.array([9, 5, 7], np.uint64)


# ---- _group_by ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,kw,vals_rows,outputs,materialize", [
    (0, {}, G, (True, True), 1),
    (0, {"want_vals": False}, None, (True, False), 1),
    (0, {"materialize": False}, None, (False, False), 0),
    (api.ALGO_INVERSE, {}, N, (True, True), 1),
    (api.ALGO_ROW_IDS, {}, G, (True, True), 1),
], ids=["plain", "keys_only", "count_only", "inverse", "row_ids"])
def test_group_by(install, flags, kw, vals_rows, outputs, materialize):
    k = aligned(KEYS)
    ov = np.arange(100, 100 + (vals_rows or 0), dtype=np.uint64)
    fake = install(G, GK.copy(), ov)
    g, sec, gk, gv = api._group_by(k, None, flags, **kw)
    a = sent(fake, GROUP_BY | flags, N, outputs, materialize)
    assert a[3] == k.ctypes.data and a[4] is None and a[6] is None and a[7] == 0
    assert (g, sec) == (G, SECONDS)
    if outputs[0]:
        assert gk.dtype == np.uint64 and np.array_equal(gk, GK) and not np.shares_memory(gk, fake.out[0])
    else:
        assert gk is None
    if outputs[1]:
        assert gv.dtype == np.int64 and gv.shape == (vals_rows,) and np.array_equal(gv, ov.view(np.int64))
        assert not np.shares_memory(gv, ov)
    else:
        assert gv is None
    came_back_clean(fake)


def test_group_by_with_a_value_column(install):
    k, v = aligned(KEYS), aligned(VALS)
    fake = install(G, GK.copy(), np.array([40, 100, 70], np.uint64))
    g, sec, gk, gv = api._group_by(k, v, api.ALGO_AGG_MAX)
    a = sent(fake, GROUP_BY | api.ALGO_AGG_MAX, N, (True, True))
    assert a[3] == k.ctypes.data and a[4] == v.ctypes.data
    assert g == G and gv.tolist() == [40, 100, 70] and gv.dtype == np.int64
    came_back_clean(fake)
    with pytest.raises(ValueError, match="values has 5 elements, keys has 6"):
        api._group_by(k, v[:5], 0)
    with pytest.raises(ValueError, match="ALGO_INVERSE: the group ids are the values output"):
        api._group_by(k, None, api.ALGO_INVERSE, want_vals=False)
    assert len(fake.calls) == 1


def test_group_by_of_nothing(install):
    fake = install(0)
    g, sec, gk, gv = api._group_by(np.empty(0, np.uint64), None, 0)
    sent(fake, GROUP_BY, 0, (True, True))
    assert g == 0 and gk.dtype == np.uint64 and gk.shape == (0,) and gv.dtype == np.int64 and gv.shape == (0,)
    came_back_clean(fake)


# ---- _group_rows -------------------------------------------------------------------------------------------------------------------
def test_group_rows(install):
    k = aligned(KEYS)
    words = np.array([3, 0, 2, 5, 1, 4, 0, 1, 4], np.uint64)              # the 6 row indices, then the 3 starts
    fake = install(G, GK.copy(), words)
    g, sec, gk, offsets, row_index = api._group_rows(k)
    a = sent(fake, GROUP_BY | api.ALGO_GROUP_ROWS, N, (True, True))
    assert a[3] == k.ctypes.data and a[4] is None and a[6] is None and a[7] == 0
    assert (g, sec) == (G, SECONDS) and np.array_equal(gk, GK) and gk.dtype == np.uint64
    assert offsets.dtype == np.int64 and offsets.tolist() == [0, 1, 4, N]
    assert row_index.dtype == np.int64 and row_index.tolist() == [3, 0, 2, 5, 1, 4]
    assert not np.shares_memory(row_index, words) and row_index.base is None      # a copy of its own, not a view of the n + g words
    words[:] = 99
    assert row_index.tolist() == [3, 0, 2, 5, 1, 4]
    came_back_clean(fake)


def test_group_rows_of_nothing(install):
    fake = install(0)
    g, sec, gk, offsets, row_index = api._group_rows(np.empty(0, np.uint64))
    sent(fake, GROUP_BY | api.ALGO_GROUP_ROWS, 0, (True, True))
    assert g == 0 and gk.shape == (0,) and offsets.tolist() == [0] and row_index.shape == (0,) and row_index.dtype == np.int64
    came_back_clean(fake)


# ---- the plane forms ---------------------------------------------------------------------------------------------------------------
def _all(k, v, p, **kw):
    return api._group_by_all(k, v, api.ALGO_AGG_SIGNED, **kw)


def _pair(k, v, p, **kw):
    return api._group_by_pair_all(k, v, p, api.ALGO_AGG_SIGNED, **kw)


def _arg(k, v, p, **kw):
    return api._group_by_arg(k, v, api.ALGO_AGG_MIN | api.ALGO_AGG_SIGNED, **kw)


def _merge(k, v, p, **kw):
    return api._group_by_merge(k, p, api.ALGO_AGG_SIGNED, **kw)


PLANE_FORMS = {   # name: call, algo word, planes, the overflow text (None: the form takes no max_groups)
    "all": (_all, GROUP_BY | api.ALGO_AGG_ALL | api.ALGO_AGG_SIGNED, 4, "group_by_agg: the relation has g = 3 distinct keys, max_groups = 2"),
    "pair_all": (_pair, GROUP_BY | api.ALGO_KEY_PAIR | api.ALGO_AGG_ALL | api.ALGO_AGG_SIGNED, 5,
                 "group_by_agg_columns: the relation has g = 3 distinct key tuples, max_groups = 2"),
    "arg": (_arg, GROUP_BY | api.ALGO_AGG_ARG | api.ALGO_AGG_MIN | api.ALGO_AGG_SIGNED, 2, None),
    "merge": (_merge, GROUP_BY | api.ALGO_AGG_ALL | api.ALGO_AGG_MERGE | api.ALGO_AGG_SIGNED, 4,
              "group_by_merge: the partial rows hold g = 3 distinct keys, max_groups = 2"),
}


def plane_inputs(n):
    """keys, a second column (values; the pair form's column B), and the pair form's values / the merge form's (4, n) planes"""
    k, v = aligned(KEYS[:n]), aligned(VALS[:n])
    return k, v, {"pair_all": aligned(np.arange(n) + 7), "merge": aligned(np.arange(4 * n).reshape(4, n))}


def sent_planes(fake, form, k, v, extra, n):
    call, algo, P, _ = PLANE_FORMS[form]
    a = sent(fake, algo, n, (True, True))
    assert a[3] == k.ctypes.data
    assert a[4] == (extra["merge"].ctypes.data if form == "merge" else v.ctypes.data)
    if form == "pair_all":                                   # the value column and its rows go where a join takes its probe side
        assert a[6] == extra["pair_all"].ctypes.data and a[7] == n
    else:
        assert a[6] is None and a[7] == 0


@pytest.mark.parametrize("form", sorted(PLANE_FORMS))
def test_plane_forms(install, form):
    call, algo, P, _ = PLANE_FORMS[form]
    k, v, extra = plane_inputs(N)
    words = np.arange(1000, 1000 + P * G, dtype=np.uint64)
    fake = install(G, GK.copy(), words)
    g, sec, gk, planes = call(k, v, extra.get(form))
    sent_planes(fake, form, k, v, extra, N)
    assert (g, sec) == (G, SECONDS) and gk.dtype == np.uint64 and np.array_equal(gk, GK)
    assert planes.dtype == np.int64 and planes.shape == (P, G) and np.array_equal(planes, words.view(np.int64).reshape(P, G))
    assert not np.shares_memory(planes, words)
    came_back_clean(fake)


@pytest.mark.parametrize("form", sorted(PLANE_FORMS))
def test_plane_forms_of_nothing(install, form):
    call, algo, P, _ = PLANE_FORMS[form]
    k, v, extra = plane_inputs(0)
    fake = install(0)
    g, sec, gk, planes = call(k, v, extra.get(form))
    sent(fake, algo, 0, (True, True))
    assert g == 0 and gk.shape == (0,) and gk.dtype == np.uint64 and planes.shape == (P, 0) and planes.dtype == np.int64
    came_back_clean(fake)


@pytest.mark.parametrize("form", [f for f in sorted(PLANE_FORMS) if PLANE_FORMS[f][3]])
def test_plane_forms_beyond_max_groups(install, form):
    """the host arrays are sized by the library: the bound is checked all the same, after both arrays were read and freed"""
    call, algo, P, text = PLANE_FORMS[form]
    k, v, extra = plane_inputs(N)
    fake = install(G, GK.copy(), np.arange(P * G, dtype=np.uint64))
    with pytest.raises(ValueError) as e:
        call(k, v, extra.get(form), max_groups=2)
    assert str(e.value) == text
    sent_planes(fake, form, k, v, extra, N)
    came_back_clean(fake)
    fake = install(G, GK.copy(), np.arange(P * G, dtype=np.uint64))
    assert call(k, v, extra.get(form), max_groups=3)[0] == G        # the bound itself is room enough


def test_element_counts_are_checked_before_the_call(install):
    fake = install(G)
    k, v, extra = plane_inputs(N)
    for call in (_all, _arg):
        with pytest.raises(ValueError, match="^values has 5 elements, keys has 6$"):
            call(k, v[:5], None)
    with pytest.raises(ValueError, match="^values has 5 elements, the key columns have 6$"):
        _pair(k, v, extra["pair_all"][:5])
    with pytest.raises(ValueError, match=r"_group_by_merge: planes must be a \(4, 6\) array"):
        _merge(k, None, extra["merge"][:, :5])
    assert fake.calls == []


# ---- a failing call, per caller ----------------------------------------------------------------------------------------------------
FAILING = {
    "group_by": lambda k, v, x: api._group_by(k, v, 0),
    "group_rows": lambda k, v, x: api._group_rows(k),
    "all": lambda k, v, x: _all(k, v, None, max_groups=2),
    "pair_all": lambda k, v, x: _pair(k, v, x["pair_all"], max_groups=2),
    "arg": lambda k, v, x: _arg(k, v, None),
    "merge": lambda k, v, x: _merge(k, None, x["merge"], max_groups=2),
    "join": lambda k, v, x: api._join_host(api.ALGO_ADAPTIVE, 0, 1, k, v, k[:4], True),
    "probe_order": lambda k, v, x: api._probe_order_host(api.ALGO_PROBE_ORDER, k, v, k[:4], True, True),
    "group_join": lambda k, v, x: api._group_host(api.ALGO_BUILD_ORDER, k, k, v, True),
}


@pytest.mark.parametrize("caller", sorted(FAILING))
def test_a_failing_call_raises_through_check(install, caller):
    """(the scripted count is g = 3 > max_groups = 2: on the host path the library's error wins, the bound is checked on a result)"""
    k, v, extra = plane_inputs(N)
    fake = install(G, rc=1)
    fails_as_ever(fake, lambda: FAILING[caller](k, v, extra))


# ---- the classifier of a value column, end to end through the public functions -----------------------------------------------------
def _by_min(k, v, **kw):
    return api.group_by_min(k, v, **kw)[3], 1, GROUP_BY | api.ALGO_AGG_MIN


def _by_agg(k, v, **kw):
    return api.group_by_agg(k, v, aggs=("min",), **kw)[3], 4, GROUP_BY | api.ALGO_AGG_ALL


def _by_argmin(k, v, **kw):
    return api.group_by_argmin(k, v, return_values=True, **kw)[4], 2, GROUP_BY | api.ALGO_AGG_ARG | api.ALGO_AGG_MIN


@pytest.mark.parametrize("public", [_by_min, _by_agg, _by_argmin], ids=["group_by_min", "group_by_agg", "group_by_argmin"])
@pytest.mark.parametrize("dtype,kw,flag,out_dtype", [
    (np.uint64, {}, 0, np.uint64),
    (np.int64, {}, api.ALGO_AGG_SIGNED, np.int64),
    (np.uint64, {"signed": True}, api.ALGO_AGG_SIGNED, np.int64),
    (np.float64, {"float64": True}, api.ALGO_AGG_FLOAT, np.float64),
], ids=["uint64", "int64", "uint64_signed", "float64"])
def test_the_value_column_decides_the_flag_and_the_dtype(install, public, dtype, kw, flag, out_dtype):
    k, v = aligned(KEYS), aligned(VALS, dtype)
    fake = install(G, GK.copy(), np.arange(5 * G, dtype=np.uint64))      # (room for the widest form)
    col, P, algo = public(k, v, **kw)
    a = sent(fake, algo | flag, N, (True, True))
    assert a[3] == k.ctypes.data and a[4] == v.ctypes.data                # uint64, int64 and float64 are all read in place
    assert col.dtype == out_dtype and col.shape == (G,)
    assert np.array_equal(col.view(np.uint64), np.arange(P * G, dtype=np.uint64).reshape(P, G)[-1 if P == 2 else 2 if P == 4 else 0])
    came_back_clean(fake)


def test_group_join_min_casts_a_float_column_as_ever(install):
    """float64=False: a NumPy float32 column is not refused by the build-order forms - it is value-cast to words and compared signed"""
    bk, pk, pv = aligned(KEYS), aligned(KEYS[::-1]), aligned(VALS, np.float32)
    mins = np.array([10, 20, 10, 40, 20, 10], np.uint64)
    fake = install(N, None, mins)
    P, sec, vals = api.group_join_min(bk, pk, pv)
    a = sent(fake, api.ALGO_ADAPTIVE | api.ALGO_BUILD_ORDER | api.ALGO_AGG_MIN | api.ALGO_AGG_SIGNED, N, (False, True))
    assert a[3] == bk.ctypes.data and a[6] == pk.ctypes.data and a[7] == N and a[4] not in (None, pv.ctypes.data)
    assert (P, sec) == (N, SECONDS) and vals.dtype == np.int64 and np.array_equal(vals, mins.view(np.int64))
    came_back_clean(fake)


# ---- the joins: _join_host, _probe_order_host, _group_host -------------------------------------------------------------------------
NB, NP = 6, 4
JOINS = {   # name: algo, build values?, the scripted count, rows of the result, values come back?
    "inner": (api.ALGO_ADAPTIVE, True, 3, 3, True),
    "left": (api.ALGO_ADAPTIVE | api.ALGO_LEFT_OUTER, True, 3, NP, True),
    "anti": (api.ALGO_ADAPTIVE | api.ALGO_ANTI, False, 3, 3, False),
    "full": (api.ALGO_ADAPTIVE | api.ALGO_FULL_OUTER, True, (3, 1), NP + 1, True),
    "left_all_copies": (api.ALGO_ADAPTIVE | api.ALGO_LEFT_OUTER | api.ALGO_ALL_COPIES, True, (5, 0, 2), 5 + 2 + 0, True),
    "full_all_copies": (api.ALGO_ADAPTIVE | api.ALGO_FULL_OUTER | api.ALGO_ALL_COPIES, True, (5, 1, 2), 5 + 2 + 1, True),
}


@pytest.mark.parametrize("how", sorted(JOINS))
def test_join_host(install, how):
    algo, with_values, count, rows, vals_back = JOINS[how]
    bk, bv, pk = aligned(KEYS), aligned(VALS), aligned(KEYS[:NP])
    ok, ov = np.arange(200, 200 + rows, dtype=np.uint64), np.arange(300, 300 + rows, dtype=np.uint64)
    fake = install(count, ok, ov)
    res = api._join_host(algo, 0, 1, bk, bv if with_values else None, pk, True)
    a = sent(fake, algo, NB, (True, True))
    assert a[3] == bk.ctypes.data and a[4] == (bv.ctypes.data if with_values else None) and a[6] == pk.ctypes.data and a[7] == NP
    assert res[0] == count and res[1] == SECONDS and len(res) == 4
    assert res[2].dtype == np.uint64 and np.array_equal(res[2], ok) and not np.shares_memory(res[2], ok)
    if vals_back:
        assert res[3].dtype == np.uint64 and np.array_equal(res[3], ov) and not np.shares_memory(res[3], ov)
    else:
        assert res[3] is None
    came_back_clean(fake)


@pytest.mark.parametrize("how", sorted(JOINS))
def test_join_host_without_arrays(install, how):
    """a count, or a materialising join whose pairs nobody asked for: no output pointer goes in and nothing is there to free"""
    algo, with_values, count, rows, vals_back = JOINS[how]
    bk, bv, pk = aligned(KEYS), aligned(VALS), aligned(KEYS[:NP])
    for materialize, return_arrays in ((0, False), (1, False), (0, True)):
        fake = install(count)
        res = api._join_host(algo, 1, materialize, bk, bv if with_values else None, pk, return_arrays)
        a = fake.only_call()
        assert (a[0], a[1], a[2], a[5], a[7], a[10], a[11]) == (algo, 1, materialize, NB, NP, None, None)
        assert res == (count, SECONDS)
        assert fake.freed == [] and fake.timings_read == 1 and api.last_timings()["total_ms"] == TOTAL_MS


def test_join_host_of_nothing(install):
    fake = install(0)
    n, sec, keys, vals = api._join_host(api.ALGO_ADAPTIVE, 0, 1, np.empty(0, np.uint64), np.empty(0, np.uint64), np.empty(0, np.uint64), True)
    sent(fake, api.ALGO_ADAPTIVE, 0, (True, True))
    assert n == 0 and keys.shape == vals.shape == (0,) and keys.dtype == vals.dtype == np.uint64
    came_back_clean(fake)
    with pytest.raises(ValueError, match="build_values has 5 elements, build_keys has 6"):
        api._join_host(api.ALGO_ADAPTIVE, 0, 1, aligned(KEYS), aligned(VALS[:5]), aligned(KEYS), True)


@pytest.mark.parametrize("want_values,want_mask", [(True, True), (True, False), (False, True)])
def test_probe_order_host(install, want_values, want_mask):
    algo = api.ALGO_ADAPTIVE | api.ALGO_PROBE_ORDER
    bk, bv, pk = aligned(KEYS), aligned(VALS), aligned(KEYS[:NP])
    mask, ov = np.array([1, 0, 1, 1], np.uint8), np.arange(300, 300 + NP, dtype=np.uint64)
    fake = install(3, mask, ov)                              # the mask goes where a join's keys go
    m, sec, vals, got_mask = api._probe_order_host(algo, bk, bv, pk, want_values, want_mask)
    a = sent(fake, algo, NB, (want_mask, want_values))
    assert a[3] == bk.ctypes.data and a[4] == bv.ctypes.data and a[6] == pk.ctypes.data and a[7] == NP
    assert (m, sec) == (3, SECONDS)
    if want_values:
        assert vals.dtype == np.uint64 and np.array_equal(vals, ov) and not np.shares_memory(vals, ov)
    else:
        assert vals is None
    if want_mask:
        assert got_mask.dtype == np.uint8 and got_mask.shape == (NP,) and np.array_equal(got_mask, mask) and not np.shares_memory(got_mask, mask)
    else:
        assert got_mask is None
    came_back_clean(fake)


def test_probe_order_host_of_no_probe_rows(install):
    fake = install(0)
    m, sec, vals, mask = api._probe_order_host(api.ALGO_PROBE_ORDER, aligned(KEYS), aligned(VALS), np.empty(0, np.uint64), True, True)
    assert m == 0 and vals.shape == mask.shape == (0,) and vals.dtype == np.uint64 and mask.dtype == np.uint8
    came_back_clean(fake)


@pytest.mark.parametrize("with_values,want_counts", [(True, True), (True, False), (False, True)])
def test_group_host(install, with_values, want_counts):
    algo = api.ALGO_ADAPTIVE | api.ALGO_BUILD_ORDER
    bk, pk, pv = aligned(KEYS), aligned(KEYS[:NP]), aligned(VALS[:NP])
    oc, osum = np.arange(NB, dtype=np.uint64), np.arange(500, 500 + NB, dtype=np.uint64)
    fake = install(NP, oc, osum)
    P, sec, counts, sums = api._group_host(algo, bk, pk, pv if with_values else None, want_counts)
    a = sent(fake, algo, NB, (want_counts, with_values))
    assert a[3] == bk.ctypes.data and a[4] == (pv.ctypes.data if with_values else None) and a[6] == pk.ctypes.data and a[7] == NP
    assert (P, sec) == (NP, SECONDS)
    for got, words, wanted in ((counts, oc, want_counts), (sums, osum, with_values)):
        if wanted:
            assert got.dtype == np.int64 and got.shape == (NB,) and np.array_equal(got, words.view(np.int64)) and not np.shares_memory(got, words)
        else:
            assert got is None
    came_back_clean(fake)
    with pytest.raises(ValueError, match="probe_values has 3 elements, probe_keys has 4"):
        api._group_host(algo, bk, pk, pv[:3], True)


def test_group_host_of_no_build_rows(install):
    fake = install(0)
    P, sec, counts, sums = api._group_host(api.ALGO_BUILD_ORDER, np.empty(0, np.uint64), aligned(KEYS), aligned(VALS), True)
    assert P == 0 and counts.shape == sums.shape == (0,) and counts.dtype == sums.dtype == np.int64
    came_back_clean(fake)
