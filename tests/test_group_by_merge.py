"""Merging partial group-by results (FJ_ALGO_GROUP_BY | FJ_ALGO_AGG_ALL | FJ_ALGO_AGG_MERGE, csrc/fj_groupby_merge.hip;
api.group_by_merge, api.GroupByAccumulator) on an MI355X: every column of one call against the NumPy reference ref_merge
(tests/test_group_by_merge_cpu.py, checked there on a hand-written case), both sides sorted by key.  Integers must match bit for bit;
float values are multiples of 2^-10 below 2^10 (exact_values of tests/test_float_aggregates.py, and sums of a few of them), so a sum
in any order is exact and needs no tolerance.  Nothing is compared with the library itself, except where the property under test
is that two of its forms agree - and then both are compared with NumPy too.

Plans: this form aims at 1024 partial rows per partition (half of its 2048-slot table), so 1024 rows are the largest flat plan; 20 000 to
32 768 rows take 5 bits in one pass, 200 000 rows 8 bits in one pass."""
import functools

import numpy as np
import pytest

import hbm_timings
import keymix
from test_float_aggregates import exact_values
from test_group_by import _dup_keys, _values_for
from test_group_by_agg_cpu import ref_group_by_agg, ref_group_by_agg_float
from test_group_by_merge_cpu import IDENTITY, KINDS, ref_merge

SIGNED, FLOAT = 0x10000, 0x2000000
TS, LIMIT = 2048, 1920                                                   # the table of fj_group_by_merge_kernel
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


class Partials:
    """partial rows - keys and four columns of words - of one kind, and their reference, computed once and never changed"""
    def __init__(self, kind, keys, counts, sums, mins, maxs):
        self.kind = kind
        self.keys = np.ascontiguousarray(keys, dtype=np.uint64)
        self.words = [np.ascontiguousarray(c).reshape(-1).view(np.uint64) for c in (counts, sums, mins, maxs)]
        assert all(w.shape == self.keys.shape for w in self.words)
        self.r = ref_merge(self.keys, *self.words, kind)
        self.g = self.r["keys"].size

    def columns(self, device):
        """the arguments of group_by_merge in the container under test, with the dtypes a caller of that kind holds"""
        if self.kind == "float":
            cols = [self.words[0].view(np.int64)] + [w.view(np.float64) for w in self.words[1:]]
        elif self.kind == "signed" or device:
            cols = [w.view(np.int64) for w in self.words]
        else:
            cols = [self.words[0].view(np.int64)] + list(self.words[1:])       # NumPy uint64 columns compare unsigned
        keys = self.keys
        return ([_dev(keys)] + [_dev(c) for c in cols]) if device else ([keys] + cols)

    def args(self, device):
        if self.kind == "float":
            return dict(float64=True)
        return dict(signed=(self.kind == "signed")) if device else dict()


def random_partials(kind, keys, seed):
    """every row as if it stood for 1 .. 5 input rows: a count, and sum, min <= max of that many values"""
    rng = np.random.default_rng(seed)
    n = keys.size
    counts = rng.integers(1, 6, size=n).astype(np.uint64)
    if kind == "float":
        a, b = exact_values(seed + 1, n), exact_values(seed + 2, n)
        return Partials(kind, keys, counts, a + b, np.minimum(a, b), np.maximum(a, b))
    a, b = _values_for(rng, keys), _values_for(rng, keys)
    dt = np.int64 if kind == "signed" else np.uint64
    return Partials(kind, keys, counts, a + b, np.minimum(a.view(dt), b.view(dt)), np.maximum(a.view(dt), b.view(dt)))


def merge(fj, p, device, base=0, **kw):
    """group_by_merge (base 0) or api._group_by_merge (ALGO_SCALAR / ALGO_RADIX) -> (g, seconds, keys, counts, sums, mins, maxs)"""
    from flash_hash_join_amd import api
    if not base:
        return fj.group_by_merge(*p.columns(device), **p.args(device), **kw)
    k, planes = api._pack_partials("test", [tuple([p.keys] + p.words)] if not device else [tuple(_dev(a) for a in [p.keys] + p.words)],
                                   ("device", 0) if device else "numpy")
    g, sec, gk, out = api._group_by_merge(k, planes, base | {"unsigned": 0, "signed": SIGNED, "float": FLOAT}[p.kind], **kw)
    return (g, sec, gk, out[0], out[1], out[2], out[3])


def check(p, out, device=None):
    """all four columns of one call, aligned with its keys, against the reference; device given: the outputs' container too"""
    g, sec, gk = out[:3]
    assert isinstance(g, int) and isinstance(sec, float) and g == p.g and len(out) == 7, (g, p.g)
    if device is not None:
        assert all(hasattr(a, "is_cuda") and a.is_cuda for a in out[2:]) if device else all(isinstance(a, np.ndarray) for a in out[2:])
    gk = _np(gk).view(np.uint64)
    order = np.argsort(gk, kind="stable")
    cols = [np.ascontiguousarray(_np(c)).view(np.uint64)[order] for c in out[3:]]
    assert all(c.shape == (g,) for c in cols)
    r = p.r
    assert np.array_equal(gk[order], r["keys"]), "the distinct keys"
    assert np.array_equal(cols[0], r["count"]), "count"
    if p.kind == "float":
        for name, c in zip(("sum", "min", "max"), cols[1:]):
            assert bool(np.all(c.view(np.float64) == r[name])), "float " + name
    else:
        for name, c in zip(("sum", "min", "max"), cols[1:]):
            assert np.array_equal(c, r[name]), name


def planned(fj, passes=None, fell_back=0, path=0):
    lt = fj.last_timings()
    assert lt["path"] == path and lt["fell_back"] == fell_back and lt["emit_ms"] == 0.0, lt
    if path == 1:
        hbm_timings.check_hbm_form(lt)
    if passes is not None:
        assert lt["passes"] == passes, lt
    assert lt["join_ms"] == lt["probe_phase_ms"], lt


# ---- 1. the zero-pass plan ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("n,distinct", [(300, 40), (1, 1), (1024, 1024)], ids=["300_rows_40_keys", "one_row", "1024_rows_all_distinct"])
def test_zero_pass_plan(fj, n, distinct, device):
    keys = _dup_keys(np.random.default_rng(n), n, distinct)
    for kind in KINDS:
        p = random_partials(kind, keys, 7 * n)
        assert p.g == distinct
        out = merge(fj, p, device)
        planned(fj, 0)
        check(p, out, device)
        if not device and kind == "unsigned":
            assert out[5].dtype == np.uint64 and out[6].dtype == np.uint64 and out[3].dtype == np.int64 and out[4].dtype == np.int64
        if kind == "float":
            assert str(out[4].dtype).endswith("float64") and str(out[3].dtype).endswith("int64")


@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_no_rows(fj, device):
    for kind in KINDS:
        p = random_partials(kind, np.empty(0, np.uint64), 3)
        check(p, merge(fj, p, device), device)
        check(p, merge(fj, p, device, base=2))


# ---- 2. the partitioned plan -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _partitioned_case(kind):
    """200 000 partial rows over 50 000 keys; raw 2^64 - 1, raw 0 and the raw key whose mix is the empty marker in 4 rows each"""
    rng = np.random.default_rng(200)
    keys = _dup_keys(rng, 200_000, 50_000)
    special = np.array([2**64 - 1, 0, keymix.EMPTY_RAW], dtype=np.uint64)
    keys[rng.choice(keys.size, 12, replace=False)] = np.repeat(special, 4)
    p = random_partials(kind, keys, 201)
    for k in special:
        assert np.count_nonzero(p.keys == k) >= 4
    return p


@pytest.mark.parametrize("base", [2, 0], ids=["radix", "adaptive"])
def test_partitioned_plan_with_the_special_keys(fj, base):
    for kind in KINDS:
        p = _partitioned_case(kind)
        for device in ((True, False) if kind == "unsigned" else (True,)):
            out = merge(fj, p, device, base=base)
            planned(fj, 1)
            assert fj.last_timings()["radix_bits"] == 8
            check(p, out)


# ---- 3. counts and sums beyond 32 bits ------------------------------------------------------------------------------------------------
def _wide_case(n_other):
    rng = np.random.default_rng(n_other)
    keys = np.concatenate([np.full(3, 0xC0FFEE, np.uint64), np.full(2, keymix.EMPTY_RAW, np.uint64), _dup_keys(rng, n_other, n_other // 3)])
    p = random_partials("unsigned", keys, n_other + 1)
    cnt, sm = p.words[0].copy(), p.words[1].copy()
    cnt[:5] = np.uint64(2**33)
    sm[:3] = np.array([2**63, 2**63, 7], dtype=np.uint64)                 # wraps to 7
    order = rng.permutation(keys.size)
    p = Partials("unsigned", keys[order], cnt[order], sm[order], p.words[2][order], p.words[3][order])
    i = int(np.searchsorted(p.r["keys"], np.uint64(0xC0FFEE)))
    assert p.r["count"][i] == 3 * 2**33 and p.r["sum"][i] == 7
    assert p.r["count"][int(np.searchsorted(p.r["keys"], np.uint64(keymix.EMPTY_RAW)))] == 2**34
    return p


@pytest.mark.parametrize("form", ["lds_zero_pass", "lds_one_pass", "hbm"])
def test_counts_beyond_32_bits_and_sums_that_wrap(fj, form):
    p = _wide_case(500 if form == "lds_zero_pass" else 5000)
    fj.set_option("scalar_hbm_table", 1 if form == "hbm" else 0)
    try:
        for device in (False, True):
            out = merge(fj, p, device, base=1 if form == "hbm" else 2)
            planned(fj, {"lds_zero_pass": 0, "lds_one_pass": 1, "hbm": 0}[form], path=1 if form == "hbm" else 0)
            check(p, out)
    finally:
        fj.set_option("scalar_hbm_table", 0)


# ---- 4. rows that stand for no input row ----------------------------------------------------------------------------------------------
def _identity_case(kind):
    """key 1: three rows of count 0 that hold the identities; key 2: two such rows and one real row; key 3: the words of -5 and 3;
    key 4 (float): -0.0 and +0.0; the marker key: identity rows only"""
    u = lambda *a: np.array(a, dtype=np.uint64)
    s0, mn0, mx0 = IDENTITY[kind]
    if kind == "float":
        f = lambda *a: np.array(a, dtype=np.float64).view(np.uint64)
        real, a, b = f(2.5)[0], f(-0.0)[0], f(0.0)[0]
        rows = [(1, 0, s0, mn0, mx0)] * 3 + [(2, 0, s0, mn0, mx0), (2, 4, f(10.0)[0], real, f(4.0)[0]), (2, 0, s0, mn0, mx0)] + \
               [(3, 1, f(-5.0)[0], f(-5.0)[0], f(-5.0)[0]), (3, 1, f(3.0)[0], f(3.0)[0], f(3.0)[0])] + [(4, 1, a, a, a), (4, 1, b, b, b)]
    else:
        m5 = 2**64 - 5
        rows = [(1, 0, s0, mn0, mx0)] * 3 + [(2, 0, s0, mn0, mx0), (2, 4, 10, 2, 4), (2, 0, s0, mn0, mx0)] + [(3, 1, m5, m5, m5), (3, 1, 3, 3, 3)]
    rows += [(keymix.EMPTY_RAW, 0, s0, mn0, mx0)] * 2
    cols = [u(*c) for c in zip(*rows)]
    return Partials(kind, *cols)


@pytest.mark.parametrize("form", ["lds", "hbm"])
def test_rows_of_count_zero_that_hold_the_identities(fj, form):
    fj.set_option("scalar_hbm_table", 1 if form == "hbm" else 0)
    try:
        for kind in KINDS:
            p = _identity_case(kind)
            r, (s0, mn0, mx0) = p.r, IDENTITY[kind]
            # the reference itself, spelled out: key 1 keeps count 0 and the identities, key 2 is its real row, key 3 takes the kind's order
            assert r["keys"][:3].tolist() == [1, 2, 3] and r["count"][:3].tolist() == [0, 4, 2]
            ident = np.array([s0, mn0, mx0], dtype=np.uint64)
            got1 = np.array([np.array([r[n][0]]).view(np.uint64)[0] for n in ("sum", "min", "max")], dtype=np.uint64)
            assert np.array_equal(got1, ident), "key 1: the identities"
            if kind == "unsigned":
                assert (r["min"][1], r["max"][1], r["min"][2], r["max"][2]) == (2, 4, 3, 2**64 - 5)
            elif kind == "signed":
                assert (r["min"][1], r["max"][1]) == (2, 4) and r["min"].view(np.int64)[2] == -5 and r["max"].view(np.int64)[2] == 3
            else:
                assert (r["min"][1], r["max"][1], r["min"][2], r["max"][2]) == (2.5, 4.0, -5.0, 3.0)
                assert r["min"][3] == 0.0 and r["max"][3] == 0.0 and r["sum"][3] == 0.0       # -0.0 == +0.0: either zero may come back
            for device in (False, True):
                out = merge(fj, p, device, base=1 if form == "hbm" else 0)
                planned(fj, 0, path=1 if form == "hbm" else 0)
                check(p, out)
    finally:
        fj.set_option("scalar_hbm_table", 0)


# ---- 5. the table's edge and the fallback ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _edge_keys(n):
    """n distinct keys in ONE final partition (19) of the 5-bit one-pass plan that n + n / 4 + 20 000 rows take at 1024 rows per
    partition, their home slots spread by random hash words 2, every fourth key twice, among 20 000 rows of the other 31 partitions"""
    rng = np.random.default_rng(n)
    one = keymix.craft(5, 19, rng.integers(0, 2**32, size=n, dtype=np.uint64), n, seed=n)
    assert np.unique(one).size == n and np.all(keymix.partition_of(one, 5) == 19)
    bg = rng.integers(0, 2**64, size=22_000, dtype=np.uint64)
    bg = bg[keymix.partition_of(bg, 5) != 19][:20_000]
    keys = np.concatenate([one, one[::4], bg])
    assert bg.size == 20_000 and 16 * 1024 < keys.size <= 32 * 1024                 # 5 radix bits
    assert np.bincount(keymix.partition_of(bg, 5), minlength=32).max() < LIMIT      # no other partition comes near the limit
    rng.shuffle(keys)
    return keys


@pytest.mark.parametrize("n,fell_back", [(LIMIT, 0), (LIMIT + 1, 1)], ids=["1920_keys_stay", "1921_keys_fall_back"])
def test_the_edge_of_the_lds_table(fj, n, fell_back):
    keys = _edge_keys(n)
    for kind in KINDS:
        p = random_partials(kind, keys, n)
        for device in ((False, True) if kind == "unsigned" else (True,)):
            out = merge(fj, p, device)
            lt = fj.last_timings()
            assert lt["fell_back"] == fell_back and lt["path"] == fell_back and lt["emit_ms"] == 0.0, (kind, device, lt)
            if fell_back:
                hbm_timings.check_hbm_form(lt, (kind, device))
            else:
                assert lt["passes"] == 1 and lt["radix_bits"] == 5, lt
            check(p, out)


@pytest.mark.parametrize("zero_pass", [False, True], ids=["one_pass", "zero_pass"])
def test_a_cluster_that_wraps_past_the_last_slot(fj, zero_pass):
    """300 keys whose home slot is the table's LAST (hash word 2 = 0x7FF | i << 11): one cluster that wraps past slot 2047 into slots
    0 .. 298; three rows each, in the last partition of a 5-bit one-pass plan among background rows, or alone on the flat plan"""
    rng = np.random.default_rng(5 + zero_pass)
    w2 = np.uint64(TS - 1) | (np.arange(300, dtype=np.uint64) << np.uint64(11))
    one = keymix.craft(0, 0, w2, 300, seed=3) if zero_pass else keymix.craft(5, 31, w2, 300, seed=3)
    assert np.all((keymix.mix(one) & np.uint64(TS - 1)) == np.uint64(TS - 1))
    keys = np.concatenate([np.repeat(one, 3), rng.integers(0, 2**64, size=100 if zero_pass else 20_000, dtype=np.uint64)])
    rng.shuffle(keys)
    for kind in KINDS:
        p = random_partials(kind, keys, 50 + zero_pass)
        out = merge(fj, p, True)
        planned(fj, 0 if zero_pass else 1)
        check(p, out, True)


def test_the_fallback_input_on_the_hbm_table(fj):
    keys = _edge_keys(LIMIT + 1)
    fj.set_option("scalar_hbm_table", 1)
    try:
        for kind in KINDS:
            p = random_partials(kind, keys, LIMIT + 1)
            out = merge(fj, p, True, base=1)
            planned(fj, 0, path=1)
            check(p, out)
    finally:
        fj.set_option("scalar_hbm_table", 0)


# ---- 6. a hot key -----------------------------------------------------------------------------------------------------------------------
def test_one_key_with_100_000_partial_rows(fj):
    rng = np.random.default_rng(6)
    single = np.unique(rng.integers(0, 2**64, size=100_100, dtype=np.uint64))[:100_001]
    keys = np.concatenate([np.full(100_000, single[-1]), single[:100_000]])
    rng.shuffle(keys)
    for kind in KINDS:
        p = random_partials(kind, keys, 60)
        assert p.g == 100_001 and int(p.r["count"].max()) >= 100_000
        out = merge(fj, p, True)
        planned(fj, 1)
        check(p, out)


# ---- 7. max_groups ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("n,distinct", [(900, 300), (30_000, 7_000)], ids=["zero_pass", "one_pass"])
def test_max_groups_bounds_the_buffers_and_a_larger_result_is_an_error(fj, n, distinct, device):
    p = random_partials("signed", _dup_keys(np.random.default_rng(n), n, distinct), n)
    check(p, merge(fj, p, device, max_groups=p.g), device)
    with pytest.raises(ValueError, match=rf"g = {p.g} distinct keys, max_groups = {p.g - 1}"):
        merge(fj, p, device, max_groups=p.g - 1)
    check(p, merge(fj, p, device), device)                                # the context is usable
    check(p, merge(fj, p, device, max_groups=10 * n), device)


def test_max_groups_on_the_hbm_table(fj):
    p = random_partials("unsigned", _dup_keys(np.random.default_rng(77), 5000, 1200), 77)
    fj.set_option("radix_threshold", p.keys.size + 1)
    try:
        check(p, merge(fj, p, True, max_groups=p.g), True)
        planned(fj, 0, path=1)
        with pytest.raises(ValueError, match=rf"g = {p.g} distinct keys"):
            merge(fj, p, True, max_groups=p.g - 1)
        check(p, merge(fj, p, True), True)
    finally:
        fj.set_option("radix_threshold", 0)


# ---- 8. the property that matters: group, cut anywhere, merge = group the whole -------------------------------------------------------------
class Relation:
    """300 000 rows over 20 000 keys, an integer and an exact float value column, 7 pieces (one empty, one of a single row) and the
    NumPy references of the whole - computed once"""
    def __init__(self):
        rng = np.random.default_rng(88)
        self.keys = _dup_keys(rng, 300_000, 20_000)
        self.vals = _values_for(rng, self.keys)
        self.fvals = exact_values(89, self.keys.size)
        c = np.sort(rng.choice(np.arange(1, self.keys.size - 1), 4, replace=False))
        self.cuts = [0, int(c[0]), int(c[1]), int(c[1]), int(c[2]), int(c[2]) + 1, int(c[3]), self.keys.size]      # 6 cut points
        sizes = np.diff(self.cuts)
        assert sizes.size == 7 and 0 in sizes and 1 in sizes and sizes.sum() == self.keys.size
        self.r = ref_group_by_agg(self.keys, self.vals)
        self.f = ref_group_by_agg_float(self.keys, self.fvals)
        self.g = self.r["keys"].size

    def pieces(self, kind, device, lo=0, hi=7):
        """[(keys, values)] of the pieces lo .. hi in the container under test"""
        vals = self.fvals if kind == "float" else self.vals.view(np.int64) if (kind == "signed" or device) else self.vals
        wrap = _dev if device else (lambda a: a)
        return [(wrap(self.keys[a:b]), wrap(vals[a:b])) for a, b in zip(self.cuts[lo:hi], self.cuts[lo + 1:hi + 1])]

    def whole(self, kind, device):
        vals = self.fvals if kind == "float" else self.vals.view(np.int64) if (kind == "signed" or device) else self.vals
        return (_dev(self.keys), _dev(vals)) if device else (self.keys, vals)

    def args(self, kind, device):
        return dict(float64=True) if kind == "float" else dict(signed=(kind == "signed")) if device else dict()

    def check(self, kind, out, aggs=("count", "sum", "min", "max")):
        """the columns `aggs` of one result against NumPy's aggregates of the whole relation"""
        g, sec, gk = out[:3]
        assert g == self.g and len(out) == 3 + len(aggs)
        gk = _np(gk).view(np.uint64)
        order = np.argsort(gk, kind="stable")
        assert np.array_equal(gk[order], self.r["keys"]), "the distinct keys"
        sfx = "_u" if kind == "unsigned" else "_s"
        for name, col in zip(aggs, out[3:]):
            col = np.ascontiguousarray(_np(col))[order]
            if name == "count":
                assert np.array_equal(col, self.r["count"]), name
            elif kind == "float":
                want = self.f["sum"] / self.f["count"] if name == "mean" else self.f[name]
                assert col.dtype == np.float64 and bool(np.all(col == want)), name
            elif name == "sum":
                assert np.array_equal(col.view(np.uint64), self.r["sum"]), name
            else:
                assert np.array_equal(col.view(self.r[name + sfx].dtype), self.r[name + sfx]), name + sfx


@functools.lru_cache(maxsize=1)
def relation():
    return Relation()


@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("kind", KINDS)
def test_merging_the_groups_of_the_pieces_equals_grouping_the_whole(fj, kind, device):
    rel = relation()
    args = rel.args(kind, device)
    parts = [fj.group_by_agg(k, v, **args) for k, v in rel.pieces(kind, device)]
    assert [p[0] for p in parts].count(0) == 1 and 1 in [p[0] for p in parts]
    merged = fj.group_by_merge(*[[p[2 + j] for p in parts] for j in range(5)], **args)
    assert fj.last_timings()["passes"] == 1 and fj.last_timings()["fell_back"] == 0
    rel.check(kind, merged)
    whole = fj.group_by_agg(*rel.whole(kind, device), **args)
    rel.check(kind, whole)
    for a, b in zip(merged[3:], whole[3:]):                               # the same dtypes as the one-call form
        assert a.dtype == b.dtype, (a.dtype, b.dtype)


# ---- 9. the accumulator -------------------------------------------------------------------------------------------------------------------
def policy_merges(batch_keys, compact_at):
    """the library merge calls the documented policy makes before result(): a batch adds its distinct keys to the pending rows, and
    once they reach max(rows of the state, compact_at) state and pending become the new state - the distinct keys seen so far"""
    merges = state = pending = 0
    seen = np.empty(0, np.uint64)
    for k in batch_keys:
        seen = np.union1d(seen, k)
        pending += np.unique(k).size
        if pending >= max(state, compact_at):
            merges, state, pending = merges + 1, seen.size, 0
    return merges, pending


@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("kind", KINDS)
def test_accumulator_over_seven_batches(fj, kind, device):
    rel = relation()
    want_merges, want_pending = policy_merges([rel.keys[a:b] for a, b in zip(rel.cuts[:-1], rel.cuts[1:])], 1000)
    assert want_merges >= 2
    args = rel.args(kind, device)
    with fj.GroupByAccumulator(compact_at=1000, **args) as acc:
        for k, v in rel.pieces(kind, device):
            g_batch, sec = acc.update(k, v)
            assert isinstance(g_batch, int) and isinstance(sec, float) and g_batch == np.unique(_np(k)).size
        assert acc.merges == want_merges and acc.pending_rows == want_pending and acc.rows_seen == rel.keys.size
        first = acc.result()
        rel.check(kind, first)
        assert acc.pending_rows == 0 and acc.num_groups == rel.g and acc.merges == want_merges + (1 if want_pending else 0)
        second = acc.result()
        assert second[0] == first[0] and second[1] == 0.0 and acc.merges == want_merges + (1 if want_pending else 0)
        for a, b in zip(first[2:], second[2:]):
            assert np.array_equal(_np(a), _np(b))
        if kind == "float":
            rel.check(kind, acc.result(aggs=("mean", "count")), aggs=("mean", "count"))
        else:
            with pytest.raises(ValueError, match="'mean' needs float64=True"):
                acc.result(aggs=("mean",))
            rel.check(kind, acc.result(aggs=("max", "count")), aggs=("max", "count"))
        # a batch of the other container kind is refused and changes nothing
        k, v = rel.pieces(kind, not device, 0, 1)[0]
        with pytest.raises(TypeError, match="one container kind and one device|of one kind and on one device"):
            acc.update(k, v)
        assert acc.rows_seen == rel.keys.size and acc.pending_rows == 0
        k, v = rel.pieces(kind, device, 0, 1)[0]
        acc.update(k, v)
        assert acc.rows_seen == rel.keys.size + _np(k).size and acc.result()[0] == rel.g


@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_two_accumulators_over_the_halves_merge_into_the_whole(fj, device):
    rel = relation()
    for kind in KINDS:
        args = rel.args(kind, device)
        a, b = fj.GroupByAccumulator(compact_at=1000, **args), fj.group_by_accumulator(compact_at=10**9, **args)
        for k, v in rel.pieces(kind, device, 0, 4):
            a.update(k, v)
        for k, v in rel.pieces(kind, device, 4, 7):
            b.update(k, v)
        assert b.merges == 0 and b.pending_rows > 0                       # b never compacted: its pending partials travel
        a.merge(b)
        assert a.rows_seen == rel.keys.size and b.rows_seen == rel.cuts[7] - rel.cuts[4]
        rel.check(kind, a.result())
        with fj.GroupByAccumulator(**args) as c:                         # ... and a's merged state travels as well
            c.merge(a)
            assert c.rows_seen == rel.keys.size
            rel.check(kind, c.result())
        a.close(); b.close()


def test_merging_index_results_that_hold_rows_without_a_partner(fj):
    """Index.group_sum / group_min / group_max with their counts: a build row without a partner has count 0 and the identities"""
    rng = np.random.default_rng(99)
    bk = np.unique(rng.integers(0, 2**64, size=3000, dtype=np.uint64))
    pk = rng.choice(bk[:2000], 40_000)                                    # the last build keys never appear
    pv = _values_for(rng, pk)
    halves = []
    with fj.build_index(bk) as idx:
        for sl in (slice(0, 25_000), slice(25_000, 40_000)):
            _, _, sums, counts = idx.group_sum(pk[sl], pv[sl], return_counts=True)
            mins, maxs = idx.group_min(pk[sl], pv[sl], signed=False)[2], idx.group_max(pk[sl], pv[sl], signed=False)[2]
            halves.append((bk, counts, sums, mins, maxs))
    assert int(np.count_nonzero(halves[0][1] == 0)) >= bk.size - 2000
    r = ref_group_by_agg(pk, pv)
    with fj.GroupByAccumulator(signed=False, compact_at=1000) as acc:
        for h in halves:
            acc.merge(h)
        assert acc.merges >= 1 and acc.rows_seen == pk.size
        g, sec, gk, cnt, sm, mn, mx = acc.result()
    assert g == bk.size
    order = np.argsort(gk)
    gk, cnt, sm, mn, mx = (np.ascontiguousarray(a[order]).view(np.uint64) for a in (gk, cnt, sm, mn, mx))
    assert np.array_equal(gk, bk)
    hit = np.isin(bk, r["keys"])
    assert np.array_equal(cnt[hit], r["count"].view(np.uint64)) and np.array_equal(sm[hit], r["sum"])
    assert np.array_equal(mn[hit], r["min_u"]) and np.array_equal(mx[hit], r["max_u"])
    s0, mn0, mx0 = IDENTITY["unsigned"]
    assert not cnt[~hit].any() and np.all(sm[~hit] == s0) and np.all(mn[~hit] == np.uint64(mn0)) and np.all(mx[~hit] == mx0)
