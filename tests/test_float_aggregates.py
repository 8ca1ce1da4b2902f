"""Float64 aggregates on an MI355X (FJ_ALGO_AGG_FLOAT; the float64= keyword of group_by_sum/min/max, group_join_sum/min/max and
Index.group_sum/min/max): every dispatch form the integer aggregates are tested on - the LDS table on the zero-pass plan and on a
one-pass radix plan, the HBM table by option, the whole-call fallback of a partition beyond the LDS table - for NumPy inputs and for
device tensors, against plain NumPy references written here (np.unique + np.bincount for sums, a stable sort + reduceat for min / max,
math.fsum for inexact sums).  Nothing is compared with the library itself.

Value domains.  "exact": k * 2^-10 with integer k in [-2^20, 2^20] and at most 2^16 rows per group, so every partial sum in any order
is a multiple of 2^-10 below 2^27 in magnitude - exactly representable - and the result must EQUAL the reference.  "inexact": standard
normal times 10^u, u uniform in [-6, 6], accepted within n_g * 2^-52 * sum(|v|) of math.fsum per group, the textbook bound of a
floating-point sum of n_g terms in any order (each of the n_g - 1 additions rounds a partial sum that is at most sum(|v|) (1 + eps)^n
in magnitude by at most eps = 2^-53 relative; to first order (n_g - 1) * 2^-53 * sum(|v|), doubled here to absorb the higher orders)."""
import functools
import math

import numpy as np
import pytest

import keymix

INF = float("inf")
IDENT = {"sum": 0.0, "min": INF, "max": -INF}
OPS = ("sum", "min", "max")
FMAX, DENORM = np.finfo(np.float64).max, 5e-324


@pytest.fixture(scope="module")
def fj():
    import flash_join
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_device_count() >= 1, "no HIP device: the product path must not silently fall back"
    assert flash_join.initialize() is None
    return flash_join


# ---- NumPy references ------------------------------------------------------------------------------------------------------------
def group_ref(keys, vals, op):
    """(sorted distinct keys, aggregate per key, rows per key)"""
    uk, codes, counts = np.unique(keys, return_inverse=True, return_counts=True)
    if op == "sum":
        return uk, np.bincount(codes, weights=vals, minlength=uk.size), counts.astype(np.int64)
    order = np.argsort(keys, kind="stable")
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    red = (np.minimum if op == "min" else np.maximum).reduceat(vals[order], starts)
    return uk, red, counts.astype(np.int64)


def join_ref(bk, pk, pv, op, first_only):
    """(aggregate per build row, count per build row, probe rows with a partner): a build row without a partner holds the identity
    and count 0; first_only: the Index rule - the aggregate at a key's FIRST build row, the identity in every further copy"""
    uk, agg, counts = group_ref(pk, pv, op)
    idx = np.minimum(np.searchsorted(uk, bk), uk.size - 1)
    hit = uk[idx] == bk
    if first_only:
        first = np.zeros(bk.size, dtype=bool)
        first[np.unique(bk, return_index=True)[1]] = True
        hit &= first
    out = np.full(bk.size, IDENT[op])
    cnt = np.zeros(bk.size, dtype=np.int64)
    out[hit], cnt[hit] = agg[idx[hit]], counts[idx[hit]]
    return out, cnt, int(np.isin(pk, bk).sum())


# ---- the dispatch forms ----------------------------------------------------------------------------------------------------------
SPECIAL = np.array([keymix.EMPTY_RAW, 2**64 - 1, 0], dtype=np.uint64)      # the LDS tables' marker, the HBM table's marker, raw zero


class Case:
    """rel: the relation of group_by_* and the probe side of the joins; bk: the build side of the joins - most of rel's keys, some of
    them several times, and keys that no row of rel carries"""

    def __init__(self, name, rel, bk, option, check, passes):
        """check: what fj.last_timings() must say after a one-shot call; passes: the radix passes of the plan, None on the HBM table"""
        self.name, self.rel, self.bk, self.option, self.check, self.passes = name, rel, bk, option, check, passes
        self.n = rel.size


def _rel(rng, n, g, hot=0):
    """n rows over g random keys and the three special ones (five rows each); hot: that many rows of ONE more key"""
    uk = np.unique(rng.integers(1, 2**64 - 1, size=g + 8, dtype=np.uint64))[:g]
    body = rng.choice(uk, n - 5 * SPECIAL.size - hot)
    hot_key = np.uint64(0x0123456789ABCDEF)
    rel = np.concatenate([np.repeat(SPECIAL, 5), body, np.full(hot, hot_key, dtype=np.uint64)])
    rng.shuffle(rel)
    return rel


def _bk(rng, rel, nb, absent=20, left_out=5):
    """nb build rows: the keys of rel but `left_out` of them, `absent` keys that rel does not hold, copies up to nb"""
    uk = np.unique(rel)
    keep = np.setdiff1d(uk, SPECIAL)
    present = np.concatenate([SPECIAL, keep[:keep.size - left_out]])
    none = np.setdiff1d(rng.integers(1, 2**64 - 1, size=absent + 4, dtype=np.uint64), uk)[:absent]
    assert none.size == absent and nb >= present.size + absent
    bk = np.concatenate([present, none, rng.choice(present, nb - present.size - absent)])
    rng.shuffle(bk)
    return bk


def _lds(passes):
    def check(lt):
        assert lt["path"] == 0 and lt["fell_back"] == 0 and lt["passes"] == passes, lt
    return check


def _hbm(lt):
    assert lt["path"] == 1 and lt["fell_back"] == 0 and lt["passes"] == 0, lt


def _fallback(lt):
    assert lt["path"] == 1 and lt["fell_back"] == 1, lt


@functools.lru_cache(maxsize=None)
def case(name):
    rng = np.random.default_rng(["zero_pass", "one_pass", "hbm", "hot", "fallback"].index(name) + 4000)
    if name == "zero_pass":                                   # a few thousand rows, ~300 groups; 400 build rows
        rel = _rel(rng, 3000, 300)
        return Case(name, rel, _bk(rng, rel, 400), None, _lds(0), 0)
    if name == "one_pass":                                    # 3951 rows: the smallest relation / build side that takes a radix pass
        rel = _rel(rng, 3951, 1500)                           # (csrc/fj_plan.hip: beyond FJ_PLAN_BUMP_KEYS = 3950 rows the plan has 5 bits)
        return Case(name, rel, _bk(rng, rel, 3951), None, _lds(1), 1)
    if name == "hbm":                                         # the same sizes on the global table (radix_threshold above them)
        rel = _rel(rng, 4097, 1500)
        return Case(name, rel, _bk(rng, rel, 4097), ("radix_threshold", 4098), _hbm, None)
    if name == "hot":                                         # one key owns half the rows: one LDS address under every atomic
        rel = _rel(rng, 3950, 300, hot=1975)                  # (3950 rows: the largest relation of the zero-pass plan)
        assert (rel == np.uint64(0x0123456789ABCDEF)).sum() == 1975
        return Case(name, rel, _bk(rng, rel, 400), None, _lds(0), 0)
    # 9000 distinct keys in ONE final partition (19) of the 5-bit plan that 29 000 rows take: beyond the 7680 keys of the LDS table
    low = np.unique(rng.integers(0, 2**59, size=9100, dtype=np.uint64))[:9000]
    one = keymix.unmix((np.uint64(19) << np.uint64(59)) | low)
    assert np.unique(one).size == 9000 and np.all(keymix.hash_w1(one) >> np.uint32(27) == 19)
    other = np.setdiff1d(rng.integers(1, 2**64 - 1, size=5600, dtype=np.uint64), one)[:5500]
    uk = np.concatenate([one, other])
    rel = np.repeat(uk, 2)                                     # 14 500 keys, two rows each: 29 000 rows
    rng.shuffle(rel)
    present = np.concatenate([one, other[:5400]])              # 14 400 keys twice + 200 absent ones: 29 000 build rows
    none = np.setdiff1d(rng.integers(1, 2**64 - 1, size=210, dtype=np.uint64), uk)[:200]
    bk = np.concatenate([present, present, none])
    rng.shuffle(bk)
    assert rel.size == bk.size == 29_000
    return Case(name, rel, bk, None, _fallback, None)


FORMS = ["zero_pass", "one_pass", "hbm", "hot", "fallback"]
CONTAINERS = [pytest.param(False, id="numpy"), pytest.param(True, id="device")]


class option:
    def __init__(self, fj, c):
        self.fj, self.opt = fj, c.option

    def __enter__(self):
        if self.opt:
            self.fj.set_option(*self.opt)

    def __exit__(self, *exc):
        if self.opt:
            self.fj.set_option(self.opt[0], 0)
        return False


# ---- values ----------------------------------------------------------------------------------------------------------------------
def exact_values(seed, n):
    return np.random.default_rng(seed).integers(-2**20, 2**20 + 1, size=n).astype(np.float64) * 2.0**-10


def inexact_values(seed, n):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 6, size=n)


def extreme_values(seed, n):
    """+-inf, +-0.0, the smallest denormal, +-max, numbers of both signs and equal magnitude, and ordinary ones between them"""
    rng = np.random.default_rng(seed)
    mag = np.abs(rng.standard_normal(32)) * 10.0 ** rng.integers(-3, 4, size=32)
    pool = np.concatenate([[INF, -INF, 0.0, -0.0, DENORM, -DENORM, FMAX, -FMAX, 1.0, -1.0], mag, -mag])
    v = np.where(rng.random(n) < 0.6, rng.choice(pool, n), rng.standard_normal(n) * 100.0)
    return v


# ---- containers and calls ----------------------------------------------------------------------------------------------------------
def dev(a):
    import torch
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def put(device, *arrays):
    return tuple(dev(a) for a in arrays) if device else arrays


def f64(a, device, n):
    """a float aggregate as returned: float64 where the inputs live"""
    if device:
        assert a.is_cuda and str(a.dtype) == "torch.float64" and tuple(a.shape) == (n,), (a.dtype, a.shape)
        return a.cpu().numpy()
    assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.shape == (n,), (a.dtype, a.shape)
    return a


def i64(a, device, n):
    if device:
        assert a.is_cuda and str(a.dtype) == "torch.int64" and tuple(a.shape) == (n,), (a.dtype, a.shape)
        return a.cpu().numpy()
    assert isinstance(a, np.ndarray) and a.dtype == np.int64 and a.shape == (n,), (a.dtype, a.shape)
    return a


def u64(a, device):
    return a.cpu().numpy().view(np.uint64) if device else a.view(np.uint64)


def same(got, ref):
    """== on every element (-0.0 == 0.0: the sign of a zero is not pinned); a NaN equals nothing and fails"""
    return got.shape == ref.shape and bool(np.all(got == ref))


def run_group_by(fj, c, op, vals, device):
    """(aggregates in the order of the sorted distinct keys, the sorted keys)"""
    keys, v = put(device, c.rel, vals)
    g, sec, gk, gv = getattr(fj, "group_by_" + op)(keys, v, float64=True)
    c.check(fj.last_timings())
    assert isinstance(g, int) and isinstance(sec, float)
    gk, gv = u64(gk, device), f64(gv, device, g)
    order = np.argsort(gk, kind="stable")
    return gv[order], gk[order]


def run_group_join(fj, c, op, vals, device):
    bk, pk, v = put(device, c.bk, c.rel, vals)
    P, sec, agg, cnt = getattr(fj, "group_join_" + op)(bk, pk, v, return_counts=True, float64=True)
    c.check(fj.last_timings())
    P1, _, agg1 = getattr(fj, "group_join_" + op)(bk, pk, v, float64=True)          # the values alone: P from the hits / the extra count launch
    return f64(agg, device, c.bk.size), i64(cnt, device, c.bk.size), P, f64(agg1, device, c.bk.size), P1


def build_index(fj, c, device):
    (bk,) = put(device, c.bk)
    with option(fj, c):
        index = fj.build_index(bk)
    lt = fj.last_timings()                                     # (the plan's passes are checked on the calls that use the index)
    assert lt["path"] == (1 if c.passes is None else 0) and lt["fell_back"] == (1 if c.name == "fallback" else 0), lt
    return index


def run_index(fj, index, c, op, vals, device, **kw):
    pk, v = put(device, c.rel, vals)
    r = getattr(index, "group_" + op)(pk, v, float64=True, **kw)
    lt = fj.last_timings()
    assert lt["build_phase_ms"] == 0.0 and lt["path"] == (1 if c.passes is None else 0) and lt["passes"] == (c.passes or 0), lt
    return r


# ---- 1. exact sums ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("device", CONTAINERS)
@pytest.mark.parametrize("form", FORMS)
def test_exact_sums_equal_bincount(fj, form, device):
    c = case(form)
    vals = exact_values(11, c.n)
    uk, codes = np.unique(c.rel, return_inverse=True)
    ref = np.bincount(codes, weights=vals)
    assert np.bincount(codes).max() <= 2**16 and (form != "hot" or np.bincount(codes).max() == 1975)
    with option(fj, c):
        got, gk = run_group_by(fj, c, "sum", vals, device)
        assert np.array_equal(gk, uk) and same(got, ref), "group_by_sum"
        # every copy of a duplicated build key carries the key's sum; a build row without a partner 0.0 and count 0
        rsum, rcnt, m = join_ref(c.bk, c.rel, vals, "sum", False)
        assert np.unique(c.bk).size < c.bk.size and (rcnt == 0).sum() >= 20
        agg, cnt, P, agg1, P1 = run_group_join(fj, c, "sum", vals, device)
        assert same(agg, rsum) and same(agg1, rsum) and np.array_equal(cnt, rcnt) and P == P1 == int(rcnt.sum()), "group_join_sum"
    # the prepared side: the sum at the key's FIRST build row, 0.0 in every further copy
    fsum, fcnt, m = join_ref(c.bk, c.rel, vals, "sum", True)
    assert (fsum != rsum).any()
    with build_index(fj, c, device) as index:
        m1, _, s1 = run_index(fj, index, c, "sum", vals, device)
        m2, _, s2, c2 = run_index(fj, index, c, "sum", vals, device, return_counts=True)
        assert m1 == m2 == m and same(f64(s1, device, c.bk.size), fsum) and same(f64(s2, device, c.bk.size), fsum), "Index.group_sum"
        assert np.array_equal(i64(c2, device, c.bk.size), fcnt)


# ---- 2. inexact sums ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("device", CONTAINERS)
def test_inexact_sums_within_the_bound_of_a_sum_in_any_order(fj, device):
    c = case("one_pass")
    vals = inexact_values(12, c.n)
    order = np.argsort(c.rel, kind="stable")
    uk, starts, counts = np.unique(c.rel[order], return_index=True, return_counts=True)
    sv = vals[order]
    ref = np.array([math.fsum(sv[s:s + n]) for s, n in zip(starts, counts)])
    bound = counts * 2.0**-52 * np.add.reduceat(np.abs(sv), starts)

    def close(got, idx, what):
        err = np.abs(got - ref[idx])
        worst = int(np.argmax(err - bound[idx]))
        print(f"{what}: largest |got - fsum| / bound = {np.max(err / bound[idx]):.3g}")
        assert np.all(err <= bound[idx]), (what, got[worst], ref[idx][worst], bound[idx][worst])
    got, gk = run_group_by(fj, c, "sum", vals, device)
    assert np.array_equal(gk, uk)
    close(got, np.arange(uk.size), "group_by_sum")
    idx = np.minimum(np.searchsorted(uk, c.bk), uk.size - 1)
    hit = uk[idx] == c.bk
    agg = run_group_join(fj, c, "sum", vals, device)[0]
    assert np.all(agg[~hit] == 0.0)
    close(agg[hit], idx[hit], "group_join_sum")
    first = np.zeros(c.bk.size, dtype=bool)
    first[np.unique(c.bk, return_index=True)[1]] = True
    with build_index(fj, c, device) as index:
        s = f64(run_index(fj, index, c, "sum", vals, device)[2], device, c.bk.size)
    assert np.all(s[~(hit & first)] == 0.0)
    close(s[hit & first], idx[hit & first], "Index.group_sum")


# ---- 3. min / max -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("device", CONTAINERS)
@pytest.mark.parametrize("form", FORMS)
def test_min_max_equal_reduceat_on_extreme_values(fj, form, device):
    c = case(form)
    vals = extreme_values(13, c.n)
    for x in (INF, -INF, DENORM, FMAX, -FMAX):
        assert (vals == x).any()
    assert (np.signbit(vals) & (vals == 0)).any() and (~np.signbit(vals) & (vals == 0)).any()
    with build_index(fj, c, device) as index:
        for op in ("min", "max"):
            uk, ref, counts = group_ref(c.rel, vals, op)
            with option(fj, c):
                got, gk = run_group_by(fj, c, op, vals, device)
                assert np.array_equal(gk, uk) and same(got, ref), "group_by_" + op
                rv, rcnt, m = join_ref(c.bk, c.rel, vals, op, False)
                agg, cnt, P, agg1, P1 = run_group_join(fj, c, op, vals, device)
                assert same(agg, rv) and same(agg1, rv) and np.array_equal(cnt, rcnt) and P == P1 == int(rcnt.sum()), "group_join_" + op
                assert (cnt == 0).sum() >= 20 and np.all(agg[cnt == 0] == IDENT[op]), "a build row without a partner: the identity and count 0"
            fv, fcnt, m = join_ref(c.bk, c.rel, vals, op, True)
            m1, _, v1 = run_index(fj, index, c, op, vals, device)
            m2, _, v2, c2 = run_index(fj, index, c, op, vals, device, return_counts=True)
            assert m1 == m2 == m and same(f64(v1, device, c.bk.size), fv) and same(f64(v2, device, c.bk.size), fv), "Index.group_" + op
            assert np.array_equal(i64(c2, device, c.bk.size), fcnt) and np.all(f64(v2, device, c.bk.size)[fcnt == 0] == IDENT[op])


# ---- 4. the marker key ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("device", CONTAINERS)
@pytest.mark.parametrize("form", ["zero_pass", "one_pass", "hbm"])
def test_the_marker_key_in_all_nine_functions(fj, form, device):
    """the key whose mixed form is the LDS tables' empty marker (and raw 2^64 - 1, the HBM table's) never enters a table: its rows
    combine into the accumulator in the kernel's header"""
    c = case(form)
    assert keymix.mix(np.array([keymix.EMPTY_RAW], dtype=np.uint64))[0] == np.uint64(keymix.EMPTY_MIXED)
    vals = exact_values(14, c.n)
    with build_index(fj, c, device) as index:
        for marker in (np.uint64(keymix.EMPTY_RAW), np.uint64(2**64 - 1)):
            rows = vals[c.rel == marker]
            assert rows.size == 5
            want = {"sum": rows.sum(), "min": rows.min(), "max": rows.max()}
            at = np.flatnonzero(c.bk == marker)
            assert at.size >= 1
            for op in OPS:
                with option(fj, c):
                    got, gk = run_group_by(fj, c, op, vals, device)
                    assert got[np.searchsorted(gk, marker)] == want[op], ("group_by_" + op, hex(int(marker)))
                    agg, cnt = run_group_join(fj, c, op, vals, device)[:2]
                    assert np.all(agg[at] == want[op]) and np.all(cnt[at] == 5), ("group_join_" + op, hex(int(marker)))
                r = run_index(fj, index, c, op, vals, device, return_counts=True)
                v, n = f64(r[2], device, c.bk.size), i64(r[3], device, c.bk.size)
                assert v[at[0]] == want[op] and n[at[0]] == 5 and np.all(v[at[1:]] == IDENT[op]) and np.all(n[at[1:]] == 0), ("Index.group_" + op, hex(int(marker)))


# ---- 5. a running aggregate ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("device", CONTAINERS)
@pytest.mark.parametrize("form", ["zero_pass", "one_pass", "hbm"])
def test_three_batches_under_out_equal_the_aggregate_of_their_concatenation(fj, form, device):
    """out= / counts_out= are combined into in place and returned.  The batches of 20 000 and 30 000 rows are cut into several work
    items - the zero-pass plan slices a flat probe side into one item per 32 chunks of 256 rows, a radix plan tiles every partition -
    so several workgroups combine into one row of `out` with the global float atomic (the HBM-table form: every hit is one)."""
    c = case(form)
    rng = np.random.default_rng(15)
    uk = np.unique(c.rel)
    sizes = (20_000, 100, 30_000)
    pks = [rng.choice(uk, n) for n in sizes]
    pvs = [exact_values(16 + i, n) for i, n in enumerate(sizes)]
    all_k, all_v = np.concatenate(pks), np.concatenate(pvs)
    assert np.unique(all_k, return_counts=True)[1].max() <= 2**16
    nb = c.bk.size
    with build_index(fj, c, device) as index:
        for op in OPS:
            ref, rcnt, m_all = join_ref(c.bk, all_k, all_v, op, True)
            acc, cnt = np.full(nb, IDENT[op]), np.zeros(nb, dtype=np.int64)
            if device:
                acc, cnt = dev(acc), dev(cnt)
            total = 0
            for pk, pv in zip(pks, pvs):
                k, v = put(device, pk, pv)
                m, sec, out, cout = getattr(index, "group_" + op)(k, v, float64=True, out=acc, counts_out=cnt)
                assert out is acc and cout is cnt, "out= and counts_out= are the objects that come back"
                total += m
            assert total == m_all
            assert same(f64(acc, device, nb), ref) and np.array_equal(i64(cnt, device, nb), rcnt), "Index.group_" + op
            k, v = put(device, all_k, all_v)                   # ... and one call on the concatenation, without out=
            m, _, one, cone = getattr(index, "group_" + op)(k, v, float64=True, return_counts=True)
            assert m == m_all and same(f64(one, device, nb), ref) and np.array_equal(i64(cone, device, nb), rcnt)


# ---- 6. NaN containment ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("device", CONTAINERS)
@pytest.mark.parametrize("form", ["zero_pass", "hbm"])
def test_a_nan_stays_in_its_group(fj, form, device):
    c = case(form)
    clean = exact_values(17, c.n)
    uk = np.unique(c.rel)
    victim = uk[uk.size // 2]
    assert victim in c.bk and not np.isin(victim, SPECIAL)
    vals = clean.copy()
    vals[np.flatnonzero(c.rel == victim)[0]] = np.nan
    at_g = int(np.searchsorted(uk, victim))
    at_b = c.bk == victim
    with build_index(fj, c, device) as index:
        for op in OPS:
            ref = group_ref(c.rel, clean, op)[1]
            rv = join_ref(c.bk, c.rel, clean, op, False)[0]
            fv = join_ref(c.bk, c.rel, clean, op, True)[0]
            with option(fj, c):
                got, gk = run_group_by(fj, c, op, vals, device)
                agg = run_group_join(fj, c, op, vals, device)[0]
            v = f64(run_index(fj, index, c, op, vals, device)[2], device, c.bk.size)
            others = np.arange(uk.size) != at_g
            assert same(got[others], ref[others]), "group_by_" + op
            assert same(agg[~at_b], rv[~at_b]), "group_join_" + op
            assert same(v[~at_b], fv[~at_b]), "Index.group_" + op
            if op == "sum":
                assert np.isnan(got[at_g]) and np.all(np.isnan(agg[at_b])) and np.isnan(v[np.flatnonzero(at_b)[0]])


# ---- 7. nothing moved ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_without_the_keyword_nothing_moved(fj):
    import torch
    c = case("zero_pass")
    vals = np.abs(exact_values(18, c.n)) + 0.75                 # fractions: the value-cast truncates them
    words = vals.astype(np.uint64)
    assert (words != vals).any()
    uk, codes = np.unique(c.rel, return_inverse=True)
    ref = np.zeros(uk.size, dtype=np.uint64)
    np.add.at(ref, codes, words)
    for kw in ({}, {"float64": False}):
        g, _, gk, gv = fj.group_by_sum(c.rel, vals, **kw)         # NumPy float64 in: value-cast to uint64 words, integer sums
        assert gv.dtype == np.int64 and np.array_equal(gv.view(np.uint64)[np.argsort(gk)], ref)
        P, _, sums = fj.group_join_sum(uk, c.rel, vals, **kw)
        assert sums.dtype == np.int64 and np.array_equal(sums.view(np.uint64), ref)
        with pytest.raises(TypeError, match="device tensors must be int64/uint64"):
            fj.group_by_sum(dev(c.rel), dev(vals), **kw)
        with pytest.raises(TypeError, match="device tensors must be int64/uint64"):
            fj.group_join_sum(dev(uk), dev(c.rel), dev(vals), **kw)
        with pytest.raises(TypeError, match="values must be integers"):
            fj.group_by_min(c.rel, vals, **kw)
        with pytest.raises(TypeError, match="values must be 64-bit integers"):
            fj.group_by_max(dev(c.rel), dev(vals), **kw)
    with fj.build_index(uk) as index:
        m, _, s = index.group_sum(c.rel, vals)
        assert s.dtype == np.int64 and np.array_equal(s.view(np.uint64), ref)
        with pytest.raises(TypeError, match="device tensors must be int64/uint64"):
            index.group_sum(dev(c.rel), dev(vals))
        with pytest.raises(TypeError, match="out must be int64"):
            index.group_sum(dev(c.rel), dev(words), out=torch.zeros(uk.size, dtype=torch.float64, device="cuda"))
        # an integer call returns int64, with and without the keyword spelled out
        for kw in ({}, {"float64": False}):
            m, _, s, n = index.group_sum(c.rel, words, return_counts=True, **kw)
            assert s.dtype == np.int64 and n.dtype == np.int64 and np.array_equal(s.view(np.uint64), ref)
            m, _, lo = index.group_min(dev(c.rel), dev(words), **kw)
            assert str(lo.dtype) == "torch.int64"
    g, _, gk, gv = fj.group_by_max(c.rel, words.view(np.int64), float64=False)
    assert gv.dtype == np.int64
    P, _, lo = fj.group_join_min(dev(uk), dev(c.rel), dev(words))
    assert str(lo.dtype) == "torch.int64"


# ---- narrower floats, DLPack, empty sides ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_float32_float16_and_dlpack_inputs(fj):
    import torch
    c = case("zero_pass")
    v16 = (np.random.default_rng(19).integers(-512, 513, size=c.n) / 4.0).astype(np.float16)      # exact in float16
    ref = group_ref(c.rel, v16.astype(np.float64), "sum")[1]
    for v in (v16, v16.astype(np.float32)):
        g, _, gk, gv = fj.group_by_sum(c.rel, v, float64=True)
        assert gv.dtype == np.float64 and same(gv[np.argsort(gk)], ref)
        g, _, gk, gv = fj.group_by_sum(dev(c.rel), torch.from_numpy(v).cuda(), float64=True)
        assert str(gv.dtype) == "torch.float64" and same(gv.cpu().numpy()[np.argsort(u64(gk, True))], ref)

    class Foreign:                                             # a device array of another library: only the DLPack protocol
        def __init__(self, t):
            self.t = t

        def __dlpack__(self, **kw):
            return self.t.__dlpack__(**kw)

        def __dlpack_device__(self):
            return self.t.__dlpack_device__()
    g, _, gk, gv = fj.group_by_min(Foreign(dev(c.rel)), Foreign(dev(v16.astype(np.float64))), float64=True)
    assert str(gv.dtype) == "torch.float64" and same(gv.cpu().numpy()[np.argsort(u64(gk, True))], group_ref(c.rel, v16.astype(np.float64), "min")[1])


@pytest.mark.gpu
@pytest.mark.parametrize("device", CONTAINERS)
def test_empty_sides(fj, device):
    c = case("zero_pass")
    none_k, none_v = put(device, np.empty(0, np.uint64), np.empty(0, np.float64))
    (bk,) = put(device, c.bk)
    for op in OPS:
        g, _, gk, gv = getattr(fj, "group_by_" + op)(none_k, none_v, float64=True)
        assert g == 0 and f64(gv, device, 0).size == 0
        P, _, agg, cnt = getattr(fj, "group_join_" + op)(bk, none_k, none_v, return_counts=True, float64=True)
        assert P == 0 and np.all(f64(agg, device, c.bk.size) == IDENT[op]) and not i64(cnt, device, c.bk.size).any()
        P, _, agg = getattr(fj, "group_join_" + op)(none_k, bk, put(device, np.ones(c.bk.size))[0], float64=True)
        assert P == 0 and f64(agg, device, 0).size == 0
    with fj.build_index(bk) as index:
        for op in OPS:
            m, _, v = getattr(index, "group_" + op)(none_k, none_v, float64=True)
            assert m == 0 and np.all(f64(v, device, c.bk.size) == IDENT[op])
