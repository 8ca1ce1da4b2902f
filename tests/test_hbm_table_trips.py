"""The HBM-table form beyond one trip of its grid-stride loops, on an MI355X: every family through the public
Python API on device tensors, at shapes where a thread of every launch takes a second trip, the sweeps serve the out-of-band slot in
a trip of its own, the outer probe's workgroups reuse their LDS cursors and the tile scan carries over three rounds.

The caps as read from the sources, the shapes derived from them (R1, R1d, R1e, J, G), the references (GroupRef, JoinRef: plain NumPy on
raw keys - a stable argsort with reduceat, np.searchsorted; no hashing, never the library) and the proof that each shape tells a
one-trip kernel from a correct one are tests/test_hbm_table_trips_cpu.py; its docstring lists the thresholds:
  rows of a gt_grid launch 4 194 304 | table build 1 048 576 | probe-order probe 4 194 304 | outer probe 8 388 608 | full join's
  sweep 2 097 152 | slots of a sweep trip 4 194 304 | fill 1 048 576 words | scan round 1024 tiles of 8192 slots
  R1 n = 4 195 365 (cap 2^24, 2 049 tiles) | J nb = 2 098 213, np = 8 392 741 (cap 2^23) | G nb = 4 195 365, np = 100 003

Every call runs under radix_threshold = n + 1 (two relations: nb + 1; restored in any case) and must report path == 1, passes == 0,
fell_back == 0 and pass hbm_timings.check_hbm_form.  Every result is compared for equality; where the order of the output is
unspecified, both sides are put in key order (or probe-row order) first, as the family's own test file does.

Not covered here, on purpose: the fallback route at these sizes (gt_fallback calls the same *_global function), the NumPy entry (the
same kernels) and duplicates="all" / the many-to-many joins (no HBM-table form).

TIMES on an MI355X machine (pytest --durations=0, one run, setup + call; a shape's reference and upload are charged to the first test
that asks for them - the NumPy references dominate, the kernels take milliseconds):
  3.47 s  test_j_left_anti_semi_join (JoinRef of J)              0.54 s  test_r1_group_by_sum_min_max[float]
  3.33 s  test_r1_unique_distinct_count_group_by_count_factorize 0.52 s  test_r1_group_by_sum_min_max[unsigned]
          (GroupRef of R1, the library's first call)             0.45 s  test_j_lookup_isin_lookup_indices
  2.46 s  test_r1d_every_row_a_group_of_its_own                  0.41 s  test_r1_group_by_sum_min_max[signed]
  1.03 s  test_r1e_at_the_threshold_and_one_row_behind_it[1]     0.38 s  test_r1_group_rows_and_group_by_collect
  1.01 s  test_j_group_join                                      0.34 s  test_j_join_indices
  1.00 s  test_r1e_at_the_threshold_and_one_row_behind_it[0]     0.28 s  test_r1_factorize_columns
  0.96 s  test_j_full_join                                       0.27 s  test_r1_group_by_argmin_argmax[unsigned | signed | float], each
  0.74 s  test_j_prepared_index                                  0.27 s  test_r1_group_by_merge_of_one_row_partials
  0.65 s  test_r1_group_by_agg                                   0.07 s  test_g_group_join_over_more_build_rows_than_one_trip
  this file: 21 tests, 18.7 s.  tests/test_group_rows.py in the same run: 53 tests, 0.3 s (its largest relation has 200 003 rows).

WOULD THEY FAIL?  Once, while this file was written, it ran against four scratch builds of the library whose loops dropped work, and
failed as it should: every gt_grid row kernel skipping every second trip (all of R1, R1d, R1e[1], G and the group_* tests of J fail;
R1e[0], one trip exactly, passes); the sweeps and fj_fill64_kernel skipping every second trip and the scan carrying one round only (all
of R1, R1d, R1e, G, group_join, Index.group fail); the outer probe, the probe-order probe and the full join's sweep skipping every
second trip (every J test but group_join fails); the LDS cursors of fj_oj_reserve and s_cnt of the sweep not reset between trips
(left / anti / full join and join_indices fail)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import hbm_timings
import test_group_rows as GR
import test_hbm_table_trips_cpu as TC

pytestmark = pytest.mark.gpu
FILL = 0xABCDEF0123456789                                 # a fill value above 2^63: its int64 storage is negative
KINDS = ("unsigned", "signed", "float")


@pytest.fixture(scope="module")
def fj():
    import flash_join
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_device_count() >= 1, "no HIP device: the product path must not silently fall back"
    assert flash_join.initialize() is None
    for name, value in (("plan_target_keys", 4096), ("scalar_hbm_table", 0), ("radix_threshold", 0)):
        assert flash_join.get_option(name) == value, f"option {name} is not at its default"
    return flash_join


@pytest.fixture(scope="module")
def T():
    """the shapes' columns on the device: uploaded once, never changed, dropped with the module"""
    import torch
    cache = {}

    def get(name):
        if name not in cache:
            d = {"r1": TC.r1, "r1d": TC.r1d, "r1e0": lambda: TC.r1e(0), "r1e1": lambda: TC.r1e(1), "j": TC.j, "g": TC.gshape}[name]()
            cols = {k: v for k, v in vars(d).items() if k in ("keys", "w", "f", "bk", "bv", "pk", "pw", "pf") and not (name == "g" and k == "bk")}
            cache[name] = SimpleNamespace(**{k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).cuda() for k, v in cols.items()})
            torch.cuda.synchronize()
        return cache[name]
    yield get
    cache.clear()


class hbm:
    """radix_threshold above the (build) relation for the calls inside, restored in any case"""
    def __init__(self, fj, nb):
        self.fj, self.nb = fj, nb

    def __enter__(self):
        self.fj.set_option("radix_threshold", self.nb + 1)

    def __exit__(self, *exc):
        self.fj.set_option("radix_threshold", 0)
        return False


def after(fj, what):
    lt = fj.last_timings()
    assert lt["path"] == 1 and lt["passes"] == 0 and lt["fell_back"] == 0, (what, lt)
    hbm_timings.check_hbm_form(lt, what)


def host(t):
    assert t.is_cuda, type(t)
    return t.cpu().numpy()


def u64(t):
    a = host(t)
    assert a.dtype == np.int64, a.dtype
    return a.view(np.uint64)


def typed(t, kind):
    """an aggregate column as the reference's dtype: the words as uint64 / int64, or float64"""
    a = host(t)
    assert a.dtype == (np.float64 if kind == "float" else np.int64), (kind, a.dtype)
    return a.view(np.uint64) if kind == "unsigned" else a


def column(d, kind, probe=False):
    w, f = (d.pw, d.pf) if probe else (d.w, d.f)
    return w if kind == "unsigned" else w.view(np.int64) if kind == "signed" else f


def api_kind(kind):
    """the keyword arguments that make the API read a torch.int64 / torch.float64 column as `kind`"""
    return {"float64": True} if kind == "float" else {"signed": kind == "signed"}


@functools.lru_cache(maxsize=None)
def agg_ref(name, kind):
    d = {"r1": TC.r1, "r1d": TC.r1d, "r1e0": lambda: TC.r1e(0), "r1e1": lambda: TC.r1e(1)}[name]()
    return TC.group_ref(name).agg(column(d, kind))


def by_key(ref, what, g, gk):
    """the permutation that puts the returned keys into the reference's order: the g distinct keys, sorted"""
    k = u64(gk)
    assert g == ref.g and k.shape == (ref.g,), (what, g, ref.g, k.shape)
    o = np.argsort(k, kind="stable")
    assert np.array_equal(k[o], ref.uniq), f"{what}: the returned keys are not the relation's distinct keys"
    return o


def check_codes(ref, what, uniques, codes):
    k, c = u64(uniques), host(codes)
    assert c.dtype == np.int64 and c.shape == (ref.n,) and c.min() >= 0 and c.max() < ref.g, what
    assert np.array_equal(k[c], ref.keys), f"{what}: uniques[codes] != keys in {int(np.count_nonzero(k[c] != ref.keys))} rows"


def check_agg(fj, T, name, kind, max_groups=None):
    ref, want, t = TC.group_ref(name), agg_ref(name, kind), T(name)
    what = f"group_by_agg {name} {kind} max_groups={max_groups}"
    g, _, gk, cnt, sm, mn, mx = fj.group_by_agg(t.keys, t.f if kind == "float" else t.w, max_groups=max_groups, **api_kind(kind))
    after(fj, what)
    o = by_key(ref, what, g, gk)
    assert np.array_equal(host(cnt)[o], ref.counts), what
    assert np.array_equal(typed(sm, kind)[o], want.sum), what
    assert np.array_equal(typed(mn, kind)[o], want.min) and np.array_equal(typed(mx, kind)[o], want.max), what


def check_factorize(fj, T, name):
    ref = TC.group_ref(name)
    g, _, codes, uniques = fj.factorize(T(name).keys)
    after(fj, f"factorize {name}")
    by_key(ref, f"factorize {name}", g, uniques)
    check_codes(ref, f"factorize {name}", uniques, codes)


def check_rows(fj, T, name):
    ref = TC.group_ref(name)
    g, _, gk, off, rows = fj.group_rows(T(name).keys)
    after(fj, f"group_rows {name}")
    GR.check_csr(ref, f"group_rows {name}", g, gk, off, rows, device=True)
    by_key(ref, f"group_rows {name}", g, gk)


# ---- R1 ------------------------------------------------------------------------------------------------------------------------------------
def test_r1_unique_distinct_count_group_by_count_factorize(fj, T):
    ref, k = TC.group_ref("r1"), T("r1").keys
    with hbm(fj, ref.n):
        g, _, gk = fj.unique(k)
        after(fj, "unique")
        by_key(ref, "unique", g, gk)
        g, _, gk, idx = fj.unique(k, return_index=True)
        after(fj, "unique index")
        assert np.array_equal(host(idx)[by_key(ref, "unique index", g, gk)], ref.first)
        g, _, gk, inv, cnt = fj.unique(k, return_inverse=True, return_counts=True)
        after(fj, "unique inverse")
        assert np.array_equal(host(cnt)[by_key(ref, "unique inverse", g, gk)], ref.counts)
        check_codes(ref, "unique inverse", gk, inv)
        g, _, gk, idx, inv, cnt = fj.unique(k, return_index=True, return_counts=True, return_inverse=True)
        after(fj, "unique index inverse counts")
        o = by_key(ref, "unique index inverse counts", g, gk)
        assert np.array_equal(host(idx)[o], ref.first) and np.array_equal(host(cnt)[o], ref.counts)
        check_codes(ref, "unique index inverse counts", gk, inv)
        g, _ = fj.distinct_count(k)
        after(fj, "distinct_count")
        assert g == ref.g
        g, _, gk, cnt = fj.group_by_count(k)
        after(fj, "group_by_count")
        assert np.array_equal(host(cnt)[by_key(ref, "group_by_count", g, gk)], ref.counts)
        check_factorize(fj, T, "r1")


@pytest.mark.parametrize("kind", KINDS)
def test_r1_group_by_sum_min_max(fj, T, kind):
    ref, want, t = TC.group_ref("r1"), agg_ref("r1", kind), T("r1")
    col = t.f if kind == "float" else t.w
    with hbm(fj, ref.n):
        if kind != "signed":                                               # (the integer sum is taken modulo 2^64: it has no sign)
            g, _, gk, sm = fj.group_by_sum(t.keys, col, float64=kind == "float")
            after(fj, f"group_by_sum {kind}")
            assert np.array_equal(typed(sm, kind)[by_key(ref, "group_by_sum", g, gk)], want.sum), kind
        g, _, gk, mn = fj.group_by_min(t.keys, col, **api_kind(kind))
        after(fj, f"group_by_min {kind}")
        assert np.array_equal(typed(mn, kind)[by_key(ref, "group_by_min", g, gk)], want.min), kind
        g, _, gk, mx = fj.group_by_max(t.keys, col, **api_kind(kind))
        after(fj, f"group_by_max {kind}")
        assert np.array_equal(typed(mx, kind)[by_key(ref, "group_by_max", g, gk)], want.max), kind


def test_r1_group_by_agg(fj, T):
    with hbm(fj, TC.r1().n):
        for kind in KINDS:
            check_agg(fj, T, "r1", kind)
        check_agg(fj, T, "r1", "unsigned", max_groups=TC.group_ref("r1").g)


@pytest.mark.parametrize("kind", KINDS)
def test_r1_group_by_argmin_argmax(fj, T, kind):
    ref, want, t = TC.group_ref("r1"), agg_ref("r1", kind), T("r1")
    with hbm(fj, ref.n):
        for fn, rows, ext in ((fj.group_by_argmin, want.argmin, want.min), (fj.group_by_argmax, want.argmax, want.max)):
            g, _, gk, idx, vals = fn(t.keys, t.f if kind == "float" else t.w, return_values=True, **api_kind(kind))
            after(fj, f"{fn.__name__} {kind}")
            o = by_key(ref, fn.__name__, g, gk)
            assert np.array_equal(host(idx)[o], rows), (fn.__name__, kind)
            assert np.array_equal(typed(vals, kind)[o], ext), (fn.__name__, kind)


def test_r1_group_by_merge_of_one_row_partials(fj, T):
    import torch
    ref, t = TC.group_ref("r1"), T("r1")
    ones = torch.ones_like(t.keys)
    with hbm(fj, ref.n):
        for kind in ("unsigned", "float"):
            want, col = agg_ref("r1", kind), (t.f if kind == "float" else t.w)
            g, _, gk, cnt, sm, mn, mx = fj.group_by_merge(t.keys, ones, col, col, col, **api_kind(kind))
            after(fj, f"group_by_merge {kind}")
            o = by_key(ref, "group_by_merge", g, gk)
            assert np.array_equal(host(cnt)[o], ref.counts), kind
            assert np.array_equal(typed(sm, kind)[o], want.sum) and np.array_equal(typed(mn, kind)[o], want.min) and np.array_equal(typed(mx, kind)[o], want.max), kind


def test_r1_factorize_columns(fj, T):
    """the pair (keys & 255, keys >> 8) has the groups of the keys: 256 first columns, so equal first columns abound"""
    ref, r, t = TC.group_ref("r1"), TC.r1(), T("r1")
    a, b = t.keys & 255, (t.keys >> 8) & ((1 << 56) - 1)                  # (int64 storage: the shift is arithmetic, the mask makes it logical)
    assert np.array_equal(u64(a), r.keys & np.uint64(255)) and np.array_equal(u64(b), r.keys >> np.uint64(8))
    with hbm(fj, ref.n):
        g, _, codes, first = fj.factorize_columns([a, b])
        after(fj, "factorize_columns")
    fi, c = host(first), host(codes)
    assert g == ref.g and fi.shape == (ref.g,) and c.shape == (ref.n,) and c.min() >= 0 and c.max() < ref.g
    k = r.keys[fi]
    o = np.argsort(k, kind="stable")
    assert np.array_equal(k[o], ref.uniq) and np.array_equal(fi[o], ref.first), "first_index: the first row of every distinct pair"
    assert np.array_equal(k[c], r.keys), "codes"
    # two pairs with equal first columns and different second columns stay apart - before and behind the cut
    low = r.keys & np.uint64(255)
    for i in (7, ref.n - 2):
        j = int(np.flatnonzero((low == low[i]) & (r.keys != r.keys[i]))[-1])
        assert c[i] != c[j] and low[i] == low[j], (i, j)


def test_r1_group_rows_and_group_by_collect(fj, T):
    import torch
    ref, r, t = TC.group_ref("r1"), TC.r1(), T("r1")
    with hbm(fj, ref.n):
        check_rows(fj, T, "r1")
        vals = torch.stack((torch.arange(ref.n, dtype=torch.int64, device=t.keys.device), t.w), dim=1)
        g, _, gk, off, got = fj.group_by_collect(t.keys, vals)
        after(fj, "group_by_collect")
    assert tuple(got.shape) == (ref.n, 2) and got.dtype == torch.int64
    GR.check_csr(ref, "group_by_collect", g, gk, off, got[:, 0].contiguous(), device=True)
    rows = host(got[:, 0].contiguous())
    assert np.array_equal(u64(got[:, 1].contiguous()), r.w[rows]), "the second column travels with the row"


# ---- R1d, R1e --------------------------------------------------------------------------------------------------------------------------------
def test_r1d_every_row_a_group_of_its_own(fj, T):
    ref, k = TC.group_ref("r1d"), T("r1d").keys
    assert ref.g == ref.n
    with hbm(fj, ref.n):
        g, _, gk, inv = fj.unique(k, return_inverse=True)
        after(fj, "unique inverse r1d")
        by_key(ref, "unique inverse r1d", g, gk)
        check_codes(ref, "unique inverse r1d", gk, inv)
        check_factorize(fj, T, "r1d")
        check_rows(fj, T, "r1d")
        check_agg(fj, T, "r1d", "unsigned")


@pytest.mark.parametrize("extra", [0, 1])
def test_r1e_at_the_threshold_and_one_row_behind_it(fj, T, extra):
    name = f"r1e{extra}"
    with hbm(fj, TC.r1e(extra).n):
        check_agg(fj, T, name, "signed")
        check_factorize(fj, T, name)
        check_rows(fj, T, name)


# ---- J ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def jwant():
    """J's expected rows in canonical order: matched (key, value) pairs by key, misses sorted, unmatched build rows by (key, value)"""
    d, ref = TC.j(), TC.join_ref("j")
    w = SimpleNamespace()
    hk = d.pk[ref.hit]
    o = np.argsort(hk, kind="stable")
    w.hit_keys, w.hit_vals = hk[o], d.bv[ref.build_idx[ref.hit]][o]
    w.miss_keys = np.sort(d.pk[~ref.hit])
    w.hit_rows, w.miss_rows = np.flatnonzero(ref.hit), np.flatnonzero(~ref.hit)
    un = ref.unmatched_build_rows
    o = np.lexsort((d.bv[un], d.bk[un]))
    w.un_rows, w.un_keys, w.un_vals = un, d.bk[un][o], d.bv[un][o]
    return w


def check_left_rows(what, m, keys, vals, fill):
    """rows [0, m) the matched pairs, rows [m, np) the unmatched probe keys with the fill value"""
    ref, w = TC.join_ref("j"), jwant()
    k, v = u64(keys), u64(vals)
    assert m == ref.m and k.shape == v.shape == (ref.pk.size,), (what, m, ref.m, k.shape)
    o = np.argsort(k[:m], kind="stable")
    assert np.array_equal(k[:m][o], w.hit_keys) and np.array_equal(v[:m][o], w.hit_vals), f"{what}: the matched pairs"
    assert np.array_equal(np.sort(k[m:]), w.miss_keys) and np.all(v[m:] == np.uint64(fill)), f"{what}: the unmatched probe rows"


def test_j_left_anti_semi_join(fj, T):
    ref, w, t = TC.join_ref("j"), jwant(), T("j")
    with hbm(fj, ref.b.n):
        m, _, k, v = fj.left_join(t.bk, t.bv, t.pk, return_arrays=True)
        after(fj, "left_join")
        check_left_rows("left_join", m, k, v, 0)
        m, _, k, v = fj.left_join(t.bk, t.bv, t.pk, return_arrays=True, fill_value=FILL, duplicates="first")
        after(fj, "left_join fill")
        check_left_rows("left_join fill", m, k, v, FILL)
        u, _, k = fj.anti_join(t.bk, t.pk, return_arrays=True)
        after(fj, "anti_join")
        assert u == ref.pk.size - ref.m and np.array_equal(np.sort(u64(k)), w.miss_keys)
        u, _ = fj.anti_join_count(t.bk, t.pk)
        after(fj, "anti_join_count")
        assert u == ref.pk.size - ref.m
        s, _, k = fj.semi_join(t.bk, t.pk, return_arrays=True)
        after(fj, "semi_join")
        assert s == ref.m and np.array_equal(np.sort(u64(k)), w.hit_keys)


def test_j_full_join(fj, T):
    ref, w, t = TC.join_ref("j"), jwant(), T("j")
    npr = ref.pk.size
    with hbm(fj, ref.b.n):
        for what, kw, fill in (("full_join", {}, 0), ("full_join fill", {"fill_value": FILL, "duplicates": "first"}, FILL)):
            m, r, _, k, v = fj.full_join(t.bk, t.bv, t.pk, return_arrays=True, **kw)
            after(fj, what)
            assert r == w.un_rows.size and k.shape[0] == npr + r, (what, r, w.un_rows.size)
            check_left_rows(what, m, k[:npr], v[:npr], fill)
            bk_, bv_ = u64(k[npr:]), u64(v[npr:])
            o = np.lexsort((bv_, bk_))
            assert np.array_equal(bk_[o], w.un_keys) and np.array_equal(bv_[o], w.un_vals), f"{what}: the unmatched build rows, every copy"


def test_j_join_indices(fj, T):
    ref, w, t = TC.join_ref("j"), jwant(), T("j")
    npr, m = ref.pk.size, ref.m

    def matched(what, pi, bi):
        o = np.argsort(pi, kind="stable")
        assert np.array_equal(pi[o], w.hit_rows) and np.array_equal(bi[o], ref.build_idx[w.hit_rows]), f"{what}: (probe row, first build row)"

    with hbm(fj, ref.b.n):
        n, _, pi, bi = fj.join_indices(t.bk, t.pk, how="inner")
        after(fj, "inner")
        assert n == m and pi.shape[0] == m
        matched("inner", host(pi), host(bi))
        n, _, pi, bi = fj.join_indices(t.bk, t.pk, how="left")
        after(fj, "left")
        pi, bi = host(pi), host(bi)
        assert n == m and pi.shape == bi.shape == (npr,)
        matched("left", pi[:m], bi[:m])
        assert np.array_equal(np.sort(pi[m:]), w.miss_rows) and np.all(bi[m:] == -1)
        u, _, pi, none = fj.join_indices(t.bk, t.pk, how="anti")
        after(fj, "anti")
        assert u == npr - m and none is None and np.array_equal(np.sort(host(pi)), w.miss_rows)
        n, r, _, pi, bi = fj.join_indices(t.bk, t.pk, how="full")
        after(fj, "full")
        pi, bi = host(pi), host(bi)
        assert n == m and r == w.un_rows.size and pi.shape == bi.shape == (npr + r,)
        matched("full", pi[:m], bi[:m])
        assert np.array_equal(np.sort(pi[m:npr]), w.miss_rows) and np.all(bi[m:npr] == -1)
        assert np.all(pi[npr:] == -1) and np.array_equal(np.sort(bi[npr:]), w.un_rows), "full: the unmatched build rows"


def check_probe_order(fj, what, fn, d, ref):
    """lookup with its mask, lookup with a fill value, isin, lookup_indices - fn: the module's functions or an Index's methods"""
    vals = np.where(ref.hit, d.bv[np.maximum(ref.build_idx, 0)], np.uint64(0))
    m, _, v, mask = fn.lookup(return_mask=True)
    after(fj, f"{what} lookup")
    assert m == ref.m and np.array_equal(u64(v), vals) and np.array_equal(host(mask), ref.hit.astype(np.uint8)), f"{what} lookup"
    m, _, v = fn.lookup(fill_value=FILL)
    after(fj, f"{what} lookup fill")
    assert m == ref.m and np.array_equal(u64(v), np.where(ref.hit, vals, np.uint64(FILL))), f"{what} lookup fill"
    m, _, mask = fn.isin()
    after(fj, f"{what} isin")
    assert m == ref.m and np.array_equal(host(mask), ref.hit.astype(np.uint8)), f"{what} isin"
    m, _, idx = fn.lookup_indices()
    after(fj, f"{what} lookup_indices")
    assert m == ref.m and np.array_equal(host(idx), ref.build_idx), f"{what} lookup_indices"


def test_j_lookup_isin_lookup_indices(fj, T):
    d, ref, t = TC.j(), TC.join_ref("j"), T("j")
    fn = SimpleNamespace(lookup=lambda **kw: fj.lookup(t.bk, t.bv, t.pk, **kw), isin=lambda: fj.isin(t.pk, t.bk),
                         lookup_indices=lambda: fj.lookup_indices(t.bk, t.pk))
    with hbm(fj, ref.b.n):
        check_probe_order(fj, "module", fn, d, ref)


GROUP_CALLS = [("unsigned", ("count", "sum", "min", "max")), ("signed", ("min", "max")), ("float", ("sum", "min", "max"))]


def check_group(fj, what, fn, d, ref, spread):
    """count, sum, min and max with their counts, unsigned; min and max signed; sum, min and max float64.  spread: per-key aggregates
    to build rows - every copy (group_join_*) or the first row alone (Index.group_*)"""
    counts = spread(ref.key_counts, np.int64(0))
    P = int(counts.sum())
    for kind, aggs in GROUP_CALLS:
        col = column(d, kind, probe=True)
        for agg in aggs:
            if agg == "count":
                got = fn(agg, kind)
                after(fj, f"{what} count")
                assert got[0] == P and np.array_equal(host(got[2]), counts), f"{what} count"
                continue
            p, _, vals, cnt = fn(agg, kind)
            after(fj, f"{what} {agg} {kind}")
            want = spread(ref.key_agg(agg, col), TC.identity(agg, col.dtype))
            assert p == P and np.array_equal(host(cnt), counts), f"{what} {agg} {kind}: the counts"
            assert np.array_equal(typed(vals, kind), want), f"{what} {agg} {kind}"


def test_j_group_join(fj, T):
    d, ref, t = TC.j(), TC.join_ref("j"), T("j")

    def fn(agg, kind):
        if agg == "count":
            return fj.group_join_count(t.bk, t.pk)
        pv = t.pf if kind == "float" else t.pw
        if agg == "sum":
            return fj.group_join_sum(t.bk, t.pk, pv, return_counts=True, float64=kind == "float")
        return getattr(fj, f"group_join_{agg}")(t.bk, t.pk, pv, return_counts=True, **api_kind(kind))
    with hbm(fj, ref.b.n):
        check_group(fj, "group_join", fn, d, ref, lambda per_key, ident: ref.per_build_row(per_key))
    assert ref.m == int(ref.key_counts.sum())


def test_j_prepared_index(fj, T):
    """build_index on the HBM table, then every Index method with J's probe side"""
    d, ref, t = TC.j(), TC.join_ref("j"), T("j")
    with hbm(fj, ref.b.n):
        index = fj.build_index(t.bk, t.bv)
        after(fj, "build_index")
    with index:
        assert (index.num_rows, index.num_keys) == (ref.b.n, ref.b.g)
        fn = SimpleNamespace(lookup=lambda **kw: index.lookup(t.pk, **kw), isin=lambda: index.isin(t.pk), lookup_indices=lambda: index.lookup_indices(t.pk))
        check_probe_order(fj, "Index", fn, d, ref)

        def gfn(agg, kind):
            if agg == "count":
                return index.group_count(t.pk)
            pv = t.pf if kind == "float" else t.pw
            if agg == "sum":
                return index.group_sum(t.pk, pv, return_counts=True, float64=kind == "float")
            return getattr(index, f"group_{agg}")(t.pk, pv, return_counts=True, **api_kind(kind))
        check_group(fj, "Index.group", gfn, d, ref, ref.at_first_rows)


# ---- G -----------------------------------------------------------------------------------------------------------------------------------------
def test_g_group_join_over_more_build_rows_than_one_trip(fj, T):
    d, ref, t, tb = TC.gshape(), TC.join_ref("g"), T("g"), T("r1")
    counts = ref.per_build_row(ref.key_counts)
    with hbm(fj, ref.b.n):
        P, _, cnt = fj.group_join_count(tb.keys, t.pk)
        after(fj, "group_join_count")
        assert P == int(counts.sum()) and np.array_equal(host(cnt), counts)
        P, _, vals, cnt = fj.group_join_max(tb.keys, t.pk, t.pw, return_counts=True, signed=True)
        after(fj, "group_join_max")
        want = ref.per_build_row(ref.key_agg("max", d.pw.view(np.int64)))
        assert P == int(counts.sum()) and np.array_equal(host(cnt), counts) and np.array_equal(host(vals), want)
