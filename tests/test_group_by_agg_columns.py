"""Four aggregates per two-column key in one call on an MI355X (FJ_ALGO_GROUP_BY | FJ_ALGO_KEY_PAIR | FJ_ALGO_AGG_ALL,
csrc/fj_groupby_pair_agg.hip; api.group_by_agg_columns): every plan depth, the marker word, two pairs on one combined word (in the
table and on the marker, with b == 0 and b == 2^64 - 1 - the resting values of the slots' bmax and bmin), the table's edge and its wrap,
the HBM form from the start and beyond one trip of its grid-stride loops, a hot pair, max_groups, the three kinds and the Python surface.

The reference is ref_pair_agg of tests/test_group_by_agg_columns_cpu.py (np.lexsort + reduceat, never the library); both sides are put
in (a, b) order before they are compared, with ==.  Float values are multiples of 2^-10 below 2^10 in magnitude: every partial sum of
at most 2^20 of them is exact in binary64, so the order of the atomic adds does not show.  Beside the values every test asserts what
fj_timings says: passes, path, fell_back, emit_ms == 0 and join_ms == probe_phase_ms."""
import functools

import numpy as np
import pytest

import hbm_timings
import keymix
from test_factorize_columns_cpu import SALT, pair64
from test_float_aggregates import exact_values
from test_group_by_agg_columns_cpu import KINDS, ref_pair_agg

TS, LIMIT = 2048, 1920                                                   # the table of fj_group_by_pair_agg_kernel
U64 = np.uint64
pytestmark = pytest.mark.gpu


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
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def a_for(words, b):
    """column A that puts the pairs (A, b) on the combined words `words`: a = w ^ mix(b ^ C)"""
    a = np.asarray(words, dtype=U64) ^ keymix.mix(np.asarray(b, dtype=U64) ^ U64(SALT))
    assert np.array_equal(pair64(a, b), np.asarray(words, dtype=U64))
    return a


def values(kind, seed, n):
    """the value column of `kind` in its own dtype: uint64 words, the same words as int64, or exact float64"""
    if kind == "float":
        return exact_values(seed, n)
    w = np.random.default_rng(seed).integers(0, 2**64, size=n, dtype=U64)
    return w if kind == "unsigned" else w.view(np.int64)


class Case:
    """key columns, a value column of one kind and their reference, computed once and never changed"""
    def __init__(self, kind, a, b, v=None, seed=1):
        self.kind = kind
        self.a, self.b = np.ascontiguousarray(a, dtype=U64), np.ascontiguousarray(b, dtype=U64)
        self.v = values(kind, seed, self.a.size) if v is None else v
        self.ref = ref_pair_agg(self.a, self.b, self.v, kind)
        self.g = self.ref[0].size
        self._dev = None

    def args(self, device):
        if not device:
            return [self.a, self.b], self.v
        if self._dev is None:
            self._dev = tuple(_dev(x) for x in (self.a, self.b, self.v))
        return [self._dev[0], self._dev[1]], self._dev[2]

    def kw(self, device):
        """what makes the API read the column as `kind` (NumPy columns carry their sign in the dtype, torch.int64 does not)"""
        return {"float64": True} if self.kind == "float" else ({"signed": self.kind == "signed"} if device else {})


def run(fj, c, device, **kw):
    cols, v = c.args(device)
    return fj.group_by_agg_columns(cols, v, **c.kw(device), **kw)


def check(c, out, device=None):
    g, sec, (ga, gb), cnt, sm, mn, mx = out
    assert isinstance(sec, float) and g == c.g, (g, c.g)
    if device is not None:
        assert all(hasattr(x, "is_cuda") and x.is_cuda for x in (ga, gb, cnt, sm, mn, mx)) if device else all(isinstance(x, np.ndarray) for x in (ga, gb, cnt, sm, mn, mx))
    ga, gb, cnt, sm, mn, mx = (_np(x) for x in (ga, gb, cnt, sm, mn, mx))
    assert all(x.shape == (g,) for x in (ga, gb, cnt, sm, mn, mx))
    ga, gb = ga.view(U64), gb.view(U64)
    o = np.lexsort((gb, ga))
    ra, rb, rcnt, rsum, rmin, rmax = c.ref
    assert np.array_equal(ga[o], ra) and np.array_equal(gb[o], rb), "the groups are not the relation's distinct pairs"
    assert cnt.dtype == np.int64 and np.array_equal(cnt[o], rcnt), "counts"
    if c.kind == "float":
        assert sm.dtype == mn.dtype == mx.dtype == np.float64
        assert np.array_equal(sm[o], rsum), "sums"
        assert np.array_equal(mn[o], rmin) and np.array_equal(mx[o], rmax), "min / max"
    else:
        view = U64 if c.kind == "unsigned" else np.int64
        assert np.array_equal(sm.view(U64)[o], rsum), "sums (modulo 2^64)"
        assert np.array_equal(mn.view(view)[o], rmin) and np.array_equal(mx.view(view)[o], rmax), "min / max"


def planned(fj, passes, fell_back=0, path=None, what=None):
    lt = fj.last_timings()
    path = fell_back if path is None else path
    assert lt["path"] == path and lt["fell_back"] == fell_back and lt["passes"] == (0 if path else passes), (what, lt)
    assert lt["emit_ms"] == 0.0 and lt["join_ms"] == lt["probe_phase_ms"], (what, lt)
    if path:
        hbm_timings.check_hbm_form(lt, what)
    return lt


class option:
    def __init__(self, fj, name, value, rest):
        self.fj, self.name, self.value, self.rest = fj, name, value, rest

    def __enter__(self):
        self.fj.set_option(self.name, self.value)

    def __exit__(self, *exc):
        self.fj.set_option(self.name, self.rest)
        return False


# ---- 1. the zero-pass plan ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("n", [1, 2, 63, 1000])
def test_zero_pass_plan(fj, n, device):
    rng = np.random.default_rng(n)
    side = 2 if n < 10 else 5 if n < 100 else 20                          # 4, 25, 400 possible pairs: most groups hold several rows
    a, b = rng.integers(0, side, size=n, dtype=U64) * U64(0x9E3779B97F4A7C15), rng.integers(0, side, size=n, dtype=U64)
    for kind in KINDS:
        c = Case(kind, a, b, seed=n)
        for base in (0, 2):
            check(c, run(fj, c, device) if base == 0 else _with_base(fj, c, device, base), device)
            planned(fj, 0, what=(n, kind, device, base))


def _with_base(fj, c, device, base, max_groups=None):
    """the library call of group_by_agg_columns under another base value (ALGO_SCALAR, ALGO_RADIX), its result in the API's shape"""
    from flash_hash_join_amd import api
    cols, v = c.args(device)
    cols, _ = api._key_columns("test", "columns", cols)
    flags = base | (api.ALGO_AGG_FLOAT if c.kind == "float" else api.ALGO_AGG_SIGNED if c.kind == "signed" else 0)
    if c.kind == "float":
        v = api._float_words("test", "values", v)
    g, sec, ga, planes = api._group_by_pair_all(cols[0], cols[1], v, flags, max_groups)
    gb = planes[0] if device else planes[0].view(U64)
    return (g, sec, (ga, gb), *api._agg_columns(planes[1:], ("count", "sum", "min", "max"), c.kind == "float", c.kind == "unsigned" and not device))


@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_an_empty_relation(fj, device):
    e = np.empty(0, U64)
    for kind in KINDS:
        c = Case(kind, e, e)
        out = run(fj, c, device)
        assert out[0] == 0 and all(_np(x).shape == (0,) for x in (*out[2], *out[3:]))
        check(c, out, device)


# ---- 2. one-pass and two-pass plans --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grid_case(kind, n):
    """n rows whose pairs are drawn from 300 x 300 values (about n / 3 pairs when n is 20 000; 90 000 pairs at most)"""
    rng = np.random.default_rng(n)
    pool_a, pool_b = rng.integers(0, 2**64, size=300, dtype=U64), rng.integers(0, 2**64, size=300, dtype=U64)
    npairs = min(n // 3, 60_000)
    pa, pb = rng.integers(0, 300, size=npairs), rng.integers(0, 300, size=npairs)
    pick = np.concatenate([np.arange(npairs), rng.integers(0, npairs, size=n - npairs)])
    rng.shuffle(pick)
    c = Case(kind, pool_a[pa[pick]], pool_b[pb[pick]], seed=n)
    w = pair64(c.ref[0], c.ref[1])
    assert np.unique(w).size == c.g, "distinct pairs have distinct words: the reference input alone takes the LDS path"
    return c


PLANS = [("one_pass", 20_011, 4096, 1), ("two_pass", 200_003, 256, 2)]


@pytest.mark.parametrize("pid,n,target,passes", PLANS, ids=[p[0] for p in PLANS])
def test_partitioned_plans(fj, pid, n, target, passes):
    for kind in KINDS:
        c = _grid_case(kind, n)
        for device in ((True, False) if kind == "unsigned" else (True,)):
            with option(fj, "plan_target_keys", target, 4096):
                out = run(fj, c, device)
                lt = planned(fj, passes, what=(pid, kind, device))
            assert lt["radix_bits"] == (5 if passes == 1 else 10), lt
            check(c, out, device)


# ---- 3. the marker word ---------------------------------------------------------------------------------------------------------------------
def _among(rng, a, b, copies, n_bg):
    """`copies` rows of every pair (a[i], b[i]) shuffled among n_bg random background rows"""
    a = np.concatenate([np.repeat(a, copies), rng.integers(0, 2**64, size=n_bg, dtype=U64)])
    b = np.concatenate([np.repeat(b, copies), rng.integers(0, 2**20, size=n_bg, dtype=U64)])
    o = rng.permutation(a.size)
    return a[o], b[o]


@pytest.mark.parametrize("n_bg,passes", [(400, 0), (20_000, 1)], ids=["zero_pass", "one_pass"])
@pytest.mark.parametrize("nb_marker,fell_back", [(1, 0), (2, 1)], ids=["one_pair_on_the_marker", "two_pairs_on_the_marker"])
def test_the_marker_word(fj, nb_marker, fell_back, n_bg, passes):
    """pairs whose combined word is the raw key of the empty marker: the out-of-band group - and, with two different b, a collision there"""
    rng = np.random.default_rng(30 + nb_marker)
    b = np.array([7, 2**63 + 5][:nb_marker], dtype=U64)
    a = a_for(np.full(nb_marker, keymix.EMPTY_RAW, dtype=U64), b)
    assert np.all(keymix.mix(pair64(a, b)) == U64(keymix.EMPTY_MIXED))
    a, b = _among(rng, a, b, 5, n_bg)
    for kind in KINDS:
        c = Case(kind, a, b, seed=31)
        for device in (False, True):
            out = run(fj, c, device)
            planned(fj, passes, fell_back, what=(kind, device))
            check(c, out, device)


# ---- 4. two pairs on one ordinary word ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _collision_columns(n_bg):
    rng = np.random.default_rng(40 + n_bg)
    w = rng.integers(1, 2**63, size=1, dtype=U64)
    b = np.array([0, 2**64 - 1], dtype=U64)                               # what a slot's bmax and bmin hold at rest
    a = a_for(np.repeat(w, 2), b)
    assert a[0] != a[1] and keymix.mix(w)[0] != U64(keymix.EMPTY_MIXED)
    return _among(rng, a, b, 3, n_bg)


@pytest.mark.parametrize("n_bg,passes", [(400, 0), (20_000, 1)], ids=["zero_pass", "one_pass"])
def test_two_pairs_on_one_word_fall_back_and_stay_exact(fj, n_bg, passes):
    a, b = _collision_columns(n_bg)
    for kind in KINDS:
        c = Case(kind, a, b, seed=41)
        for device in ((False, True) if kind == "unsigned" else (True,)):
            out = run(fj, c, device)
            planned(fj, passes, fell_back=1, path=1, what=(kind, device))
            check(c, out, device)


# ---- 5. the table's edge ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _edge_columns(n):
    """n distinct pairs whose WORDS lie in ONE final partition (19) of the 5-bit one-pass plan that n + n / 4 + 20 000 rows take at 1024
    rows per partition, their home slots spread by random hash words 2, every fourth pair twice, among 20 000 rows of the other 31"""
    rng = np.random.default_rng(n)
    words = keymix.craft(5, 19, rng.integers(0, 2**32, size=n, dtype=U64), n, seed=n)
    assert np.unique(words).size == n and np.all(keymix.partition_of(words, 5) == 19)
    b = rng.integers(0, 2**64, size=n, dtype=U64)
    a = a_for(words, b)
    ba, bb = rng.integers(0, 2**64, size=22_000, dtype=U64), rng.integers(0, 2**64, size=22_000, dtype=U64)
    keep = np.flatnonzero(keymix.partition_of(pair64(ba, bb), 5) != 19)[:20_000]
    ba, bb = ba[keep], bb[keep]
    a, b = np.concatenate([a, a[::4], ba]), np.concatenate([b, b[::4], bb])
    assert keep.size == 20_000 and 16 * 1024 < a.size <= 32 * 1024                 # 5 radix bits
    assert np.bincount(keymix.partition_of(pair64(ba, bb), 5), minlength=32).max() < LIMIT
    o = rng.permutation(a.size)
    return a[o], b[o]


@pytest.mark.parametrize("n,fell_back", [(LIMIT, 0), (LIMIT + 1, 1)], ids=["1920_pairs_stay", "1921_pairs_fall_back"])
def test_the_edge_of_the_lds_table(fj, n, fell_back):
    a, b = _edge_columns(n)
    for kind in KINDS:
        c = Case(kind, a, b, seed=n)
        for device in ((False, True) if kind == "unsigned" else (True,)):
            out = run(fj, c, device)
            lt = planned(fj, 1, fell_back, what=(kind, device))
            if not fell_back:
                assert lt["radix_bits"] == 5, lt
            check(c, out, device)


@pytest.mark.parametrize("zero_pass", [False, True], ids=["one_pass", "zero_pass"])
def test_a_cluster_that_wraps_past_the_last_slot(fj, zero_pass):
    """300 words whose home slot is the table's LAST (hash word 2 = 0x7FF | i << 11): one cluster that wraps past slot 2047 into slots
    0 .. 298; three rows each, in the last partition of a 5-bit one-pass plan among background rows, or alone on the flat plan"""
    rng = np.random.default_rng(5 + zero_pass)
    w2 = U64(TS - 1) | (np.arange(300, dtype=U64) << U64(11))
    words = keymix.craft(0, 0, w2, 300, seed=3) if zero_pass else keymix.craft(5, 31, w2, 300, seed=3)
    assert np.all((keymix.mix(words) & U64(TS - 1)) == U64(TS - 1))
    b = rng.integers(0, 2**64, size=300, dtype=U64)
    a, b = _among(rng, a_for(words, b), b, 3, 100 if zero_pass else 20_000)
    for kind in KINDS:
        c = Case(kind, a, b, seed=50 + zero_pass)
        out = run(fj, c, True)
        planned(fj, 0 if zero_pass else 1, what=kind)
        check(c, out, True)


# ---- 6. the HBM form from the start ---------------------------------------------------------------------------------------------------------
HBM_INPUTS = {"grid": lambda kind: _grid_case(kind, 20_011), "collision": lambda kind: Case(kind, *_collision_columns(20_000), seed=41),
              "edge": lambda kind: Case(kind, *_edge_columns(LIMIT + 1), seed=LIMIT + 1)}


@pytest.mark.parametrize("name", list(HBM_INPUTS))
def test_hbm_form_from_the_start(fj, name):
    with option(fj, "scalar_hbm_table", 1, 0):
        for kind in KINDS:
            c = HBM_INPUTS[name](kind)
            for device in ((True, False) if kind == "unsigned" else (True,)):
                out = _with_base(fj, c, device, 1)
                planned(fj, 0, fell_back=0, path=1, what=(name, kind, device))
                check(c, out, device)


def test_hbm_form_beyond_one_trip_of_its_grid_stride_loops(fj):
    """R1 of tests/test_hbm_table_trips_cpu.py: 4 195 365 rows, more than the 4 194 304 of one trip of a gt_grid launch, over a table of
    2^24 slots, four trips of the sweep.  The pair (keys & 255, keys >> 8) has the groups of the keys, so the reference is R1's own"""
    import test_hbm_table_trips_cpu as TC
    r, ref = TC.r1(), TC.group_ref("r1")
    want = ref.agg(r.w)
    assert ref.n > 4096 * 1024
    k = _dev(r.keys)
    a, b, v = k & 255, (k >> 8) & ((1 << 56) - 1), _dev(r.w)
    with option(fj, "radix_threshold", ref.n + 1, 0):
        g, _, (ga, gb), cnt, sm, mn, mx = fj.group_by_agg_columns([a, b], v, signed=False)
        planned(fj, 0, fell_back=0, path=1, what="r1")
    key = (_np(gb).view(U64) << U64(8)) | _np(ga).view(U64)
    o = np.argsort(key, kind="stable")
    assert g == ref.g and np.array_equal(key[o], ref.uniq) and np.array_equal(_np(cnt)[o], ref.counts)
    assert np.array_equal(_np(sm).view(U64)[o], want.sum) and np.array_equal(_np(mn).view(U64)[o], want.min) and np.array_equal(_np(mx).view(U64)[o], want.max)


# ---- 7. a hot pair --------------------------------------------------------------------------------------------------------------------------
def test_one_pair_with_100_000_rows(fj):
    rng = np.random.default_rng(7)
    a = np.concatenate([np.full(100_000, 0xC0FFEE, dtype=U64), rng.integers(0, 1000, size=100_000, dtype=U64)])
    b = np.concatenate([np.full(100_000, 42, dtype=U64), np.arange(100_000, dtype=U64)])       # single pairs: b is distinct
    o = rng.permutation(a.size)
    for kind in KINDS:
        c = Case(kind, a[o], b[o], seed=70)
        assert c.g == 100_001 and int(c.ref[2].max()) == 100_000
        out = run(fj, c, True)
        planned(fj, 1, what=kind)
        check(c, out, True)


# ---- 8. max_groups ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("form", ["zero_pass", "one_pass", "hbm"])
def test_max_groups_bounds_the_buffers_and_a_larger_result_is_an_error(fj, form, device):
    n = 900 if form == "zero_pass" else 20_011
    rng = np.random.default_rng(n)
    c = Case("signed", rng.integers(0, 40, size=n, dtype=U64), rng.integers(0, 30, size=n, dtype=U64), seed=80)
    with option(fj, "radix_threshold", n + 1 if form == "hbm" else 0, 0):
        out = run(fj, c, device, max_groups=c.g)
        planned(fj, {"zero_pass": 0, "one_pass": 1, "hbm": 0}[form], path=int(form == "hbm"), what=form)
        if device:
            assert all(x.shape[0] == c.g for x in (*out[2], *out[3:])), "buffers of g rows"
        check(c, out, device)
        with pytest.raises(ValueError, match=rf"g = {c.g} distinct key tuples, max_groups = {c.g - 1}"):
            run(fj, c, device, max_groups=c.g - 1)
        check(c, run(fj, c, device), device)                              # the context is usable
        check(c, run(fj, c, device, max_groups=10 * n), device)


# ---- 9. kinds -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_signed_extremes_and_unsigned_words(fj, device):
    a = np.array([1, 1, 1, 2, 2, 1, 2], dtype=U64)
    b = np.array([9, 9, 8, 9, 9, 9, 9], dtype=U64)
    s = np.array([-2**63, 2**63 - 1, -1, -2**63, -2**63, 0, 5], dtype=np.int64)
    c = Case("signed", a, b, v=s)
    assert c.ref[4].tolist() == [-1, -2**63, -2**63] and c.ref[5].tolist() == [-1, 2**63 - 1, 5]
    check(c, run(fj, c, device), device)
    c = Case("unsigned", a, b, v=s.view(U64))
    assert c.ref[4].tolist() == [2**64 - 1, 0, 5] and c.ref[5].tolist() == [2**64 - 1, 2**63, 2**63]
    out = run(fj, c, device)
    check(c, out, device)
    if not device:
        assert out[5].dtype == U64 and out[6].dtype == U64 and out[4].dtype == np.int64       # a NumPy uint64 column: its own dtype for min / max


@pytest.mark.parametrize("form", ["lds", "hbm"])
def test_float_zeros_and_a_nan_in_one_group(fj, form):
    rng = np.random.default_rng(90)
    a, b = rng.integers(0, 12, size=600, dtype=U64), rng.integers(0, 9, size=600, dtype=U64)
    v = exact_values(91, 600)
    zero = (a == 3) & (b == 4)
    v[zero] = np.where(rng.random(int(zero.sum())) < 0.5, 0.0, -0.0)          # a group of zeros of both signs: either zero may come back
    nan = (a == 5) & (b == 1)
    assert zero.sum() >= 2 and nan.sum() >= 2
    with option(fj, "radix_threshold", 601 if form == "hbm" else 0, 0):
        c = Case("float", a, b, v=v.copy())
        zi = int(np.flatnonzero((c.ref[0] == 3) & (c.ref[1] == 4))[0])
        assert c.ref[3][zi] == 0.0 and c.ref[4][zi] == 0.0 and c.ref[5][zi] == 0.0
        for device in (False, True):
            check(c, run(fj, c, device), device)
            planned(fj, 0, path=int(form == "hbm"), what=form)
        v[np.flatnonzero(nan)[0]] = np.nan
        c2 = Case("float", a, b, v=v)
        g, _, (ga, gb), cnt, sm, mn, mx = run(fj, c2, True)
        ga, gb = _np(ga).view(U64), _np(gb).view(U64)
        o = np.lexsort((gb, ga))
        other = ~((c.ref[0] == 5) & (c.ref[1] == 1))                         # every other group is exact; the NaN's group keeps its count
        assert g == c.g and np.array_equal(_np(cnt)[o], c.ref[2])
        for got, want in ((sm, c.ref[3]), (mn, c.ref[4]), (mx, c.ref[5])):
            assert np.array_equal(_np(got)[o][other], want[other])
        assert np.isnan(_np(sm)[o][~other]).all()


# ---- 10. the Python surface ----------------------------------------------------------------------------------------------------------------
def test_subsets_and_orders_of_aggs(fj):
    c = _grid_case("float", 20_011)
    ra, rb, rcnt, rsum, rmin, rmax = c.ref
    for device in (False, True):
        g, _, (ga, gb), mx, mean, cnt = run(fj, c, device, aggs=("max", "mean", "count"))
        o = np.lexsort((_np(gb).view(U64), _np(ga).view(U64)))
        assert np.array_equal(_np(mx)[o], rmax) and np.array_equal(_np(cnt)[o], rcnt) and np.array_equal(_np(mean)[o], rsum / rcnt)
        out = run(fj, c, device, aggs=("sum",))
        assert len(out) == 4 and np.array_equal(_np(out[3])[np.lexsort((_np(out[2][1]).view(U64), _np(out[2][0]).view(U64)))], rsum)
    c = _grid_case("signed", 20_011)
    g, _, (ga, gb), mn, cnt = run(fj, c, True, aggs=["min", "count"])
    o = np.lexsort((_np(gb).view(U64), _np(ga).view(U64)))
    assert np.array_equal(_np(mn)[o], c.ref[4]) and np.array_equal(_np(cnt)[o], c.ref[2])


@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_one_column_is_group_by_agg(fj, device):
    c = _grid_case("unsigned", 20_011)
    (a, _), v = c.args(device)
    g, _, cols, *aggs = fj.group_by_agg_columns([a], v, signed=False)
    g1, _, gk, *aggs1 = fj.group_by_agg(a, v, signed=False)
    assert g == g1 and isinstance(cols, tuple) and len(cols) == 1
    o, o1 = np.argsort(_np(cols[0]).view(U64)), np.argsort(_np(gk).view(U64))
    assert np.array_equal(_np(cols[0])[o], _np(gk)[o1]) and all(np.array_equal(_np(x)[o], _np(y)[o1]) for x, y in zip(aggs, aggs1))
    g, _, cols, *aggs = fj.group_by_agg_columns(a, v, signed=False)           # a single array is one column
    assert g == g1 and len(cols) == 1 and len(aggs) == 4


@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("ncols", [3, 4])
def test_three_and_four_columns(fj, ncols, device):
    n = 20_011
    rng = np.random.default_rng(ncols)
    cols = [rng.integers(0, 6, size=n, dtype=U64) * U64(0x0123456789ABCDEF + 2 * i) for i in range(ncols)]
    v = values("signed", 100 + ncols, n)
    order = np.lexsort(tuple(reversed(cols)))
    sc = [c[order] for c in cols]
    starts = np.flatnonzero(np.r_[True, np.logical_or.reduce([c[1:] != c[:-1] for c in sc])])
    want_cnt = np.diff(np.r_[starts, n])
    want_sum = np.add.reduceat(v[order].view(U64), starts)
    want_min, want_max = np.minimum.reduceat(v[order], starts), np.maximum.reduceat(v[order], starts)
    g, sec, gcols, cnt, sm, mn, mx = fj.group_by_agg_columns([_dev(c) for c in cols] if device else cols, _dev(v) if device else v)
    assert g == starts.size and len(gcols) == ncols and isinstance(sec, float)
    gc = [_np(c).view(U64) for c in gcols]
    o = np.lexsort(tuple(reversed(gc)))
    assert all(np.array_equal(x[o], y[starts]) for x, y in zip(gc, sc)), "the distinct tuples"
    assert np.array_equal(_np(cnt)[o], want_cnt) and np.array_equal(_np(sm).view(U64)[o], want_sum)
    assert np.array_equal(_np(mn)[o], want_min) and np.array_equal(_np(mx)[o], want_max)


@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_counts_without_a_value_column(fj, device):
    c = _grid_case("unsigned", 20_011)
    cols, _ = c.args(device)
    out = fj.group_by_agg_columns(cols, None, aggs=("count",))
    planned(fj, 1)
    assert len(out) == 4
    g, _, (ga, gb), cnt = out
    o = np.lexsort((_np(gb).view(U64), _np(ga).view(U64)))
    assert g == c.g and np.array_equal(_np(ga).view(U64)[o], c.ref[0]) and np.array_equal(_np(cnt)[o], c.ref[2])


def test_side_stream_and_a_strided_view(fj):
    """the call runs on the current stream of the inputs' device; a strided view is a legal key column"""
    import torch
    c = _grid_case("signed", 20_011)
    (a, b), v = c.args(True)
    wide = torch.stack((a, torch.zeros_like(a)), dim=1)                    # column A as every second word of a (n, 2) tensor
    view = wide[:, 0]
    assert not view.is_contiguous()
    s = torch.cuda.Stream(device=a.device)
    s.wait_stream(torch.cuda.current_stream(a.device))
    with torch.cuda.stream(s):
        out = fj.group_by_agg_columns([view, b], v, signed=True)
        planned(fj, 1)
    s.synchronize()
    assert out[2][0].device == a.device
    check(c, out, True)


# ---- 11. agreement with the composition -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [20_011, 200_003])
def test_agreement_with_factorize_columns_and_group_by_agg(fj, n):
    c = _grid_case("signed", n)
    (a, b), v = c.args(True)
    g, _, (ga, gb), cnt, sm, mn, mx = fj.group_by_agg_columns([a, b], v, signed=True)
    g2, _, codes, first = fj.factorize_columns([a, b])
    g3, _, gk, cnt2, sm2, mn2, mx2 = fj.group_by_agg(codes, v, signed=True)
    a2, b2 = a[first[gk]], b[first[gk]]                                    # the two gathers through first_index
    assert g == g2 == g3 == c.g
    o = np.lexsort((_np(gb).view(U64), _np(ga).view(U64)))
    o2 = np.lexsort((_np(b2).view(U64), _np(a2).view(U64)))
    for x, y in ((ga, a2), (gb, b2), (cnt, cnt2), (sm, sm2), (mn, mn2), (mx, mx2)):
        assert np.array_equal(_np(x)[o], _np(y)[o2])
