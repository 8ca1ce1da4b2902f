"""One table of forms x routes over the host drivers that share the plan scaffold (csrc/fj_plan.hip: pair_open / pair_items / pair_close,
rel_open / rel_close, gt_open / gt_close / gt_fallback): every extension form on every route its driver can take - an empty side, the
zero-pass plan, one pass, more passes, the global table from the start, the forced fallback onto it - and, for the forms with a
first-occurrence rerun, every partitioned route once more over duplicated build keys.

Each cell asserts two things.  The result equals a NumPy reference (sorted where the order is unspecified; integer words only, float
sums are not part of this table).  And the plan facts of fj_timings equal the literal tuple in PINNED: path, passes, radix_bits,
partitions, fell_back, lds_retries, bloom_level, sampled_hit_bp, build_phase_ms == 0, emit_ms == 0, probe_phase_ms == join_ms.  The
literals were recorded from the library BEFORE the drivers moved onto the shared scaffold; they are what the scaffold must reproduce,
not what it happens to give.  Where a form refuses a route the cell pins the exception's type and message instead."""
import functools

import numpy as np
import pytest

import keymix
from test_factorize_columns_cpu import pair64, SALT

NB_SMALL, NP_SMALL = 1000, 5000          # the zero-pass plan
NB, NP = 20_000, 60_000                  # one pass at the default options (5 radix bits), more under plan_target_keys = 16
SKEW = 9000                              # distinct build keys in ONE final partition of that 5-bit plan: beyond every LDS table


@pytest.fixture(scope="module")
def api():
    from flash_hash_join_amd import _lib, api
    assert _lib.load().fj_device_count() >= 1, "no HIP device: the product path must not silently fall back"
    api.initialize()
    return api


# ---- the rows ---------------------------------------------------------------------------------------------------------------
class Pair:
    """a build and a probe relation, their device copies and the first-occurrence reference, computed once"""
    def __init__(self, bk, pk, seed):
        rng = np.random.default_rng(seed)
        self.bk, self.pk = np.ascontiguousarray(bk, dtype=np.uint64), np.ascontiguousarray(pk, dtype=np.uint64)
        self.bv = (np.arange(self.bk.size, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)      # distinct per row, never 0
        self.pv = rng.integers(0, 2**64, size=self.pk.size, dtype=np.uint64)
        order = np.argsort(self.bk, kind="stable")
        sb = self.bk[order]
        if sb.size:
            lo = np.minimum(np.searchsorted(sb, self.pk, "left"), sb.size - 1)
            self.hit = sb[lo] == self.pk
            self.idx = np.where(self.hit, order[lo], -1).astype(np.int64)                 # the smallest build row of the key
        else:
            self.hit, self.idx = np.zeros(self.pk.size, dtype=bool), np.full(self.pk.size, -1, np.int64)
        self.m = int(self.hit.sum())
        self.unique_build = np.unique(self.bk).size == self.bk.size

    @functools.cached_property
    def dev(self):
        return tuple(_dev(a) for a in (self.bk, self.bv, self.pk, self.pv))

    @functools.cached_property
    def per_build_row(self):
        """(counts, sums modulo 2^64) of the probe rows of every build row's key"""
        keys, inv = np.unique(self.pk, return_inverse=True)
        cnt, sm = np.bincount(inv, minlength=keys.size).astype(np.uint64), np.zeros(keys.size, dtype=np.uint64)
        np.add.at(sm, inv, self.pv)
        if not keys.size:
            return np.zeros(self.bk.size, np.uint64), np.zeros(self.bk.size, np.uint64)
        at = np.minimum(np.searchsorted(keys, self.bk), keys.size - 1)
        found = keys[at] == self.bk
        return np.where(found, cnt[at], 0).astype(np.uint64), np.where(found, sm[at], 0).astype(np.uint64)


class Rel:
    """one relation under a two-column key with a value column, and its reference: the distinct pairs in NumPy's order, their first
    rows, and count, sum (modulo 2^64), unsigned minimum and maximum of the values per pair"""
    def __init__(self, a, b, seed):
        rng = np.random.default_rng(seed)
        self.a, self.b = np.ascontiguousarray(a, dtype=np.uint64), np.ascontiguousarray(b, dtype=np.uint64)
        self.n = self.a.size
        self.v = rng.integers(0, 2**64, size=self.n, dtype=np.uint64)
        if self.n:
            self.pairs, self.first, inv = np.unique(np.stack([self.a, self.b], 1), axis=0, return_index=True, return_inverse=True)
            inv = inv.reshape(-1)
        else:
            self.pairs, self.first, inv = np.empty((0, 2), np.uint64), np.empty(0, np.int64), np.empty(0, np.int64)
        self.g = int(self.pairs.shape[0])
        self.count = np.bincount(inv, minlength=self.g).astype(np.uint64)
        self.sum = np.zeros(self.g, np.uint64); np.add.at(self.sum, inv, self.v)
        self.min = np.full(self.g, 2**64 - 1, np.uint64); np.minimum.at(self.min, inv, self.v)
        self.max = np.zeros(self.g, np.uint64); np.maximum.at(self.max, inv, self.v)

    @functools.cached_property
    def dev(self):
        return tuple(_dev(x) for x in (self.a, self.b, self.v))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _distinct(rng, n):
    k = np.unique(rng.integers(1, 2**62, size=n + 64, dtype=np.uint64))[:n]       # (below 2^62: the misses live above)
    rng.shuffle(k)
    assert k.size == n
    return k


def _with_dups(rng, bk):
    """10 % of the rows become copies of earlier keys (their values differ: a value is the row's own)"""
    d = bk.size // 10
    bk = bk.copy()
    bk[bk.size - d:] = bk[:d]
    return bk[rng.permutation(bk.size)]


def _probe_of(rng, bk, n_p):
    miss = rng.integers(2**62, 2**63, size=n_p - n_p // 2, dtype=np.uint64)
    pk = np.concatenate([rng.choice(bk, n_p // 2), miss]) if bk.size else rng.integers(2**62, 2**63, size=n_p, dtype=np.uint64)
    return pk[rng.permutation(pk.size)]


def _skewed_keys(rng, dups):
    """SKEW distinct keys of partition 7 of the 5-bit plan and NB - SKEW keys of its other partitions: NB rows, so the plan stays.
    dups: the last 10 % of the rows are copies of keys of partition 7 instead"""
    cand = np.arange(1, 400_000, dtype=np.uint64)
    part = keymix.partition_of(cand, 5)
    bk = np.concatenate([cand[part == 7][:SKEW], cand[part != 7][:NB - SKEW]])
    if dups:
        bk[NB - NB // 10:] = bk[:NB // 10]
    assert bk.size == NB and np.unique(bk[keymix.partition_of(bk, 5) == 7]).size == SKEW
    return bk[rng.permutation(NB)]


@functools.lru_cache(maxsize=None)
def pair_rows(shape, dups=False):
    rng = np.random.default_rng(["empty_build", "empty_probe", "small", "large", "skewed"].index(shape) + 10 * dups)
    nb, n_p = {"empty_build": (0, NP_SMALL), "empty_probe": (NB_SMALL, 0), "small": (NB_SMALL, NP_SMALL)}.get(shape, (NB, NP))
    bk = _skewed_keys(rng, dups) if shape == "skewed" else _with_dups(rng, _distinct(rng, nb)) if dups else _distinct(rng, nb)
    return Pair(bk, _probe_of(rng, bk, n_p), seed=99)


@functools.lru_cache(maxsize=None)
def rel_rows(shape):
    rng = np.random.default_rng(["empty", "small", "large", "skewed"].index(shape) + 50)
    if shape == "empty":
        return Rel(np.empty(0, np.uint64), np.empty(0, np.uint64), seed=98)
    if shape == "skewed":     # SKEW distinct COMBINED WORDS (what the passes partition) in partition 7 of the 5-bit plan, each once
        low = np.unique(rng.integers(0, 2**59, size=SKEW + 100, dtype=np.uint64))[:SKEW]
        words = keymix.unmix((np.uint64(7) << np.uint64(59)) | low)
        b = rng.integers(0, 2**64, size=SKEW, dtype=np.uint64)
        a = words ^ keymix.mix(b ^ np.uint64(SALT))
        assert np.array_equal(pair64(a, b), words) and np.all(keymix.partition_of(words, 5) == 7)
        bg = rng.integers(0, 2**64, size=(2, NB - SKEW), dtype=np.uint64)
        a, b = np.concatenate([a, bg[0]]), np.concatenate([b, bg[1]])
    else:                     # every pair about three times
        n = NB_SMALL if shape == "small" else NB
        va, vb = rng.integers(0, 2**64, size=64, dtype=np.uint64), rng.integers(0, 2**64, size=n // 192 + 2, dtype=np.uint64)
        pick = rng.integers(0, va.size * vb.size, size=n)
        a, b = va[pick % va.size], vb[pick // va.size]
    o = rng.permutation(a.size)
    return Rel(a[o], b[o], seed=98)


# ---- the routes: id -> (rows of a two-relation form, rows of a one-relation form, option, its value or how to derive it) -----------
ROUTES = {
    "empty_build": ("empty_build", "empty", None, None),
    "empty_probe": ("empty_probe", None, None, None),
    "zero_pass": ("small", "small", None, None),
    "one_pass": ("large", "large", None, None),
    "more_passes": ("large", "large", "plan_target_keys", 16),
    "global_table": ("large", "large", "radix_threshold", NB + 1),
    "fallback": ("skewed", "skewed", None, None),
}
PARTITIONED = ("zero_pass", "one_pass", "more_passes", "fallback")


# ---- the forms: each returns nothing and asserts its result against the reference ----------------------------------------------------
def _sorted_pairs(k, v):
    o = np.lexsort((v, k))
    return k[o], v[o]


def _assert_pairs(got_k, got_v, want_k, want_v, what):
    gk, gv = _sorted_pairs(got_k, got_v)
    wk, wv = _sorted_pairs(want_k, want_v)
    assert np.array_equal(gk, wk) and np.array_equal(gv, wv), what


def _check_lookup(r, m, vals, mask):
    assert m == r.m
    assert np.array_equal(mask.cpu().numpy(), r.hit.astype(np.uint8)), "mask"
    want = np.zeros(r.pk.size, np.uint64)
    want[r.hit] = r.bv[r.idx[r.hit]]
    assert np.array_equal(_u64(vals), want), "values: the first occurrence's, 0 where there is no partner"


def f_lookup(api, r):
    bk, bv, pk, _ = r.dev
    m, _, vals, mask = api.lookup(bk, bv, pk, return_mask=True)
    _check_lookup(r, m, vals, mask)


def f_isin(api, r):
    bk, _, pk, _ = r.dev
    m, _, mask = api.isin(pk, bk)
    assert m == r.m and np.array_equal(mask.cpu().numpy(), r.hit.astype(np.uint8))


def f_lookup_indices(api, r):
    bk, _, pk, _ = r.dev
    m, _, idx = api.lookup_indices(bk, pk)
    assert m == r.m and np.array_equal(idx.cpu().numpy(), r.idx)


def _check_left(r, m, keys, vals, n_p):
    assert m == r.m
    _assert_pairs(keys[:m], vals[:m], r.pk[r.hit], r.bv[r.idx[r.hit]], "matched rows")
    assert np.array_equal(np.sort(keys[m:n_p]), np.sort(r.pk[~r.hit])) and not vals[m:n_p].any(), "unmatched rows"


def f_left_join(api, r):
    bk, bv, pk, _ = r.dev
    m, _, keys, vals = api.left_join(bk, bv, pk, return_arrays=True)
    assert keys.shape[0] == r.pk.size
    _check_left(r, m, _u64(keys), _u64(vals), r.pk.size)


def f_anti_join(api, r):
    bk, _, pk, _ = r.dev
    u, _, keys = api.anti_join(bk, pk, return_arrays=True)
    assert u == r.pk.size - r.m and np.array_equal(np.sort(_u64(keys)[:u]), np.sort(r.pk[~r.hit]))


def f_full_join(api, r):
    bk, bv, pk, _ = r.dev
    m, rest, _, keys, vals = api.full_join(bk, bv, pk, return_arrays=True)
    keys, vals, n_p = _u64(keys), _u64(vals), r.pk.size
    alone = ~np.isin(r.bk, r.pk)
    assert rest == int(alone.sum()) and keys.shape[0] == n_p + rest
    _check_left(r, m, keys, vals, n_p)
    _assert_pairs(keys[n_p:], vals[n_p:], r.bk[alone], r.bv[alone], "build rows without a partner, every copy")


def f_group_join_count(api, r):
    bk, _, pk, _ = r.dev
    P, _, counts = api.group_join_count(bk, pk)
    assert np.array_equal(_u64(counts), r.per_build_row[0]) and P == int(r.per_build_row[0].sum())


def f_group_join_sum(api, r):
    bk, _, pk, pv = r.dev
    P, _, sums = api.group_join_sum(bk, pk, pv)
    assert np.array_equal(_u64(sums), r.per_build_row[1]) and P == int(r.per_build_row[0].sum())


def f_join_indices_many(api, r):
    assert r.unique_build                                    # (then the pairs are the first occurrences')
    bk, _, pk, _ = r.dev
    n, _, pi, bi = api.join_indices(bk, pk, how="inner", many_to_many=True)
    assert n == r.m
    _assert_pairs(_u64(pi)[:n], _u64(bi)[:n], np.flatnonzero(r.hit).astype(np.uint64), r.idx[r.hit].astype(np.uint64), "pairs")


def f_index_lookup(api, r):
    bk, bv, pk, _ = r.dev
    with api.build_index(bk, bv) as ix:
        m, _, vals, mask = ix.lookup(pk, return_mask=True)
    _check_lookup(r, m, vals, mask)


def f_index_group_sum(api, r):
    assert r.unique_build                                    # (then the first build row of a key is its only one)
    bk, _, pk, pv = r.dev
    with api.build_index(bk) as ix:
        m, _, sums = ix.group_sum(pk, pv)
    assert m == r.m and np.array_equal(_u64(sums), r.per_build_row[1])


def f_factorize_columns(api, r):
    a, b, _ = r.dev
    g, _, codes, first = api.factorize_columns([a, b])
    codes, first = codes.cpu().numpy(), first.cpu().numpy()
    assert g == r.g and codes.shape == (r.n,) and first.shape == (g,)
    assert np.array_equal(np.sort(first), np.sort(r.first)), "first_index: the smallest row of every pair"
    if r.n:
        assert codes.min() >= 0 and codes.max() < g
        assert np.array_equal(r.a[first][codes], r.a) and np.array_equal(r.b[first][codes], r.b)


def f_group_by_agg_columns(api, r):
    a, b, v = r.dev
    g, _, (ga, gb), cnt, sm, mn, mx = api.group_by_agg_columns([a, b], v, signed=False)
    assert g == r.g
    ga, gb = _u64(ga)[:g], _u64(gb)[:g]
    o = np.lexsort((gb, ga))                                 # NumPy's order of the distinct pairs
    assert np.array_equal(ga[o], r.pairs[:, 0]) and np.array_equal(gb[o], r.pairs[:, 1])
    for got, want, what in ((cnt, r.count, "count"), (sm, r.sum, "sum"), (mn, r.min, "min"), (mx, r.max, "max")):
        assert np.array_equal(_u64(got)[:g][o], want), what


TWO = {"lookup": f_lookup, "isin": f_isin, "lookup_indices": f_lookup_indices, "left_join": f_left_join, "anti_join": f_anti_join,
       "full_join": f_full_join, "group_join_count": f_group_join_count, "group_join_sum": f_group_join_sum,
       "join_indices_many": f_join_indices_many, "index_lookup": f_index_lookup, "index_group_sum": f_index_group_sum}
ONE = {"factorize_columns": f_factorize_columns, "group_by_agg_columns": f_group_by_agg_columns}
RERUN = ("lookup", "left_join", "full_join", "group_join_sum")       # a first-occurrence rerun (group_join_sum alone: the count form once more)

CELLS = [(form, route, False) for form in TWO for route in ROUTES]
CELLS += [(form, route, True) for form in RERUN for route in PARTITIONED]
CELLS += [(form, route, False) for form in ONE for route in ROUTES if ROUTES[route][1]]     # (one relation: there is no probe side to be empty)


def facts(lt):
    return (lt["path"], lt["passes"], lt["radix_bits"], lt["partitions"], lt["fell_back"], lt["lds_retries"], lt["bloom_level"],
            lt["sampled_hit_bp"], lt["build_phase_ms"] == 0.0, lt["emit_ms"] == 0.0, lt["probe_phase_ms"] == lt["join_ms"])


def run_cell(api, form, route, dups):
    """the cell's facts, or ("raises", type name, message); the result is asserted on the way"""
    two_rows, one_rows, option, value = ROUTES[route]
    rows = pair_rows(two_rows, dups) if form in TWO else rel_rows(one_rows)
    before = api.get_option(option) if option else None
    if option:
        api.set_option(option, value)
    try:
        try:
            (TWO.get(form) or ONE[form])(api, rows)
        except (RuntimeError, ValueError, MemoryError) as e:
            return ("raises", type(e).__name__, str(e))
        return facts(api.last_timings())
    finally:
        if option:
            api.set_option(option, before)


# (path, passes, radix_bits, partitions, fell_back, lds_retries, bloom_level, sampled_hit_bp, build_phase_ms == 0, emit_ms == 0,
#  probe_phase_ms == join_ms) per (form, route, duplicated build keys)
PINNED = {
    ('lookup', 'empty_build', False): (0, 0, 0, 0, 0, 0, 0, -1, True, True, True),
    ('lookup', 'empty_probe', False): (0, 0, 0, 0, 0, 0, 0, -1, True, True, True),
    ('lookup', 'zero_pass', False): (0, 0, 0, 1, 0, 0, 0, -1, False, True, False),
    ('lookup', 'one_pass', False): (0, 1, 5, 32, 0, 0, 0, -1, False, True, False),
    ('lookup', 'more_passes', False): (0, 2, 11, 2048, 0, 0, 0, -1, False, True, False),
    ('lookup', 'global_table', False): (1, 0, 0, 1, 0, 0, 0, -1, False, True, True),
    ('lookup', 'fallback', False): (1, 0, 0, 1, 1, 0, 0, -1, False, True, True),
    ('isin', 'empty_build', False): (0, 0, 0, 0, 0, 0, 0, -1, True, True, True),
    ('isin', 'empty_probe', False): (0, 0, 0, 0, 0, 0, 0, -1, True, True, True),
    ('isin', 'zero_pass', False): (0, 0, 0, 1, 0, 0, 0, -1, False, True, False),
    ('isin', 'one_pass', False): (0, 1, 5, 32, 0, 0, 0, -1, False, True, False),
    ('isin', 'more_passes', False): (0, 2, 11, 2048, 0, 0, 0, -1, False, True, False),
    ('isin', 'global_table', False): (1, 0, 0, 1, 0, 0, 0, -1, False, True, True),
    ('isin', 'fallback', False): (1, 0, 0, 1, 1, 0, 0, -1, False, True, True),
    ('lookup_indices', 'empty_build', False): (0, 0, 0, 0, 0, 0, 0, -1, True, True, True),
    ('lookup_indices', 'empty_probe', False): (0, 0, 0, 0, 0, 0, 0, -1, True, True, True),
    ('lookup_indices', 'zero_pass', False): (0, 0, 0, 1, 0, 0, 0, -1, False, True, False),
    ('lookup_indices', 'one_pass', False): (0, 1, 5, 32, 0, 0, 0, -1, False, True, False),
    ('lookup_indices', 'more_passes', False): (0, 2, 11, 2048, 0, 0, 0, -1, False, True, False),
    ('lookup_indices', 'global_table', False): (1, 0, 0, 1, 0, 0, 0, -1, False, True, True),
    ('lookup_indices', 'fallback', False): (1, 0, 0, 1, 1, 0, 0, -1, False, True, True),
    ('left_join', 'empty_build', False): (0, 0, 0, 0, 0, 0, 0, -1, True, True, True),
    ('left_join', 'empty_probe', False): (0, 0, 0, 0, 0, 0, 0, -1, True, True, True),
    ('left_join', 'zero_pass', False): (0, 0, 0, 1, 0, 0, 0, -1, False, True, False),
    ('left_join', 'one_pass', False): (0, 1, 5, 32, 0, 0, 0, -1, False, True, False),
    ('left_join', 'more_passes', False): (0, 2, 11, 2048, 0, 0, 0, -1, False, True, False),
    ('left_join', 'global_table', False): (1, 0, 0, 1, 0, 0, 0, -1, False, True, True),
    ('left_join', 'fallback', False): (1, 0, 0, 1, 1, 0, 0, -1, False, True, True),
    ('anti_join', 'empty_build', False): (0, 0, 0, 0, 0, 0, 0, -1, True, True, True),
    ('anti_join', 'empty_probe', False): (0, 0, 0, 0, 0, 0, 0, -1, True, True, True),
    ('anti_join', 'zero_pass', False): (0, 0, 0, 1, 0, 0, 0, -1, False, True, False),
    ('anti_join', 'one_pass', False): (0, 1, 5, 32, 0, 0, 0, -1, False, True, False),
    ('anti_join', 'more_passes', False): (0, 2, 11, 2048, 0, 0, 0, -1, False, True, False),
    ('anti_join', 'global_table', False): (1, 0, 0, 1, 0, 0, 0, -1, False, True, True),
    ('anti_join', 'fallback', False): (0, 1, 5, 32, 0, 0, 0, -1, False, True, False),
    ('full_join', 'empty_build', False): (0, 0, 0, 0, 0, 0, 0, -1, True, True, True),
    ('full_join', 'empty_probe', False): (0, 0, 0, 0, 0, 0, 0, -1, True, False, True),
    ('full_join', 'zero_pass', False): (0, 0, 0, 1, 0, 0, 0, -1, False, False, False),
    ('full_join', 'one_pass', False): (0, 1, 5, 32, 0, 0, 0, -1, False, False, False),
    ('full_join', 'more_passes', False): (0, 2, 11, 2048, 0, 0, 0, -1, False, False, False),
    ('full_join', 'global_table', False): (1, 0, 0, 1, 0, 0, 0, -1, False, False, True),
    ('full_join', 'fallback', False): (1, 0, 0, 1, 1, 0, 0, -1, False, False, True),
    ('group_join_count', 'empty_build', False): (0, 0, 0, 0, 0, 0, 0, -1, True, True, True),
    ('group_join_count', 'empty_probe', False): (0, 0, 0, 0, 0, 0, 0, -1, True, True, True),
    ('group_join_count', 'zero_pass', False): (0, 0, 0, 1, 0, 0, 0, -1, False, True, False),
    ('group_join_count', 'one_pass', False): (0, 1, 5, 32, 0, 0, 0, -1, False, True, False),
    ('group_join_count', 'more_passes', False): (0, 2, 11, 2048, 0, 0, 0, -1, False, True, False),
    ('group_join_count', 'global_table', False): (1, 0, 0, 1, 0, 0, 0, -1, False, True, True),
    ('group_join_count', 'fallback', False): (1, 0, 0, 1, 1, 0, 0, -1, False, True, True),
    ('group_join_sum', 'empty_build', False): (0, 0, 0, 0, 0, 0, 0, -1, True, True, True),
    ('group_join_sum', 'empty_probe', False): (0, 0, 0, 0, 0, 0, 0, -1, True, True, True),
    ('group_join_sum', 'zero_pass', False): (0, 0, 0, 1, 0, 0, 0, -1, False, True, False),
    ('group_join_sum', 'one_pass', False): (0, 1, 5, 32, 0, 0, 0, -1, False, True, False),
    ('group_join_sum', 'more_passes', False): (0, 2, 11, 2048, 0, 0, 0, -1, False, True, False),
    ('group_join_sum', 'global_table', False): (1, 0, 0, 1, 0, 0, 0, -1, False, True, True),
    ('group_join_sum', 'fallback', False): (1, 0, 0, 1, 1, 0, 0, -1, False, True, True),
    ('join_indices_many', 'empty_build', False): (0, 0, 0, 0, 0, 0, 0, -1, True, True, True),
    ('join_indices_many', 'empty_probe', False): (0, 0, 0, 0, 0, 0, 0, -1, True, True, True),
    ('join_indices_many', 'zero_pass', False): (0, 0, 0, 1, 0, 0, 0, -1, False, False, False),
    ('join_indices_many', 'one_pass', False): (0, 1, 5, 32, 0, 0, 0, -1, False, False, False),
    ('join_indices_many', 'more_passes', False): (0, 2, 11, 2048, 0, 0, 0, -1, False, False, False),
    ('join_indices_many', 'global_table', False): (0, 1, 5, 32, 0, 0, 0, -1, False, False, False),
    ('join_indices_many', 'fallback', False): ('raises', 'RuntimeError', 'many-to-many join: a final partition holds more than 4096 build rows (a build key with thousands of duplicates?); not supported'),
    ('index_lookup', 'empty_build', False): (0, 0, 0, 1, 0, 0, 0, -1, True, True, True),
    ('index_lookup', 'empty_probe', False): (0, 0, 0, 1, 0, 0, 0, -1, True, True, True),
    ('index_lookup', 'zero_pass', False): (0, 0, 0, 1, 0, 0, 0, -1, True, True, False),
    ('index_lookup', 'one_pass', False): (0, 1, 5, 32, 0, 0, 0, -1, True, True, False),
    ('index_lookup', 'more_passes', False): (0, 2, 11, 2048, 0, 0, 0, -1, True, True, False),
    ('index_lookup', 'global_table', False): (1, 0, 0, 1, 0, 0, 0, -1, True, True, True),
    ('index_lookup', 'fallback', False): (1, 0, 0, 1, 0, 0, 0, -1, True, True, True),
    ('index_group_sum', 'empty_build', False): (0, 0, 0, 1, 0, 0, 0, -1, True, True, True),
    ('index_group_sum', 'empty_probe', False): (0, 0, 0, 1, 0, 0, 0, -1, True, True, True),
    ('index_group_sum', 'zero_pass', False): (0, 0, 0, 1, 0, 0, 0, -1, True, True, False),
    ('index_group_sum', 'one_pass', False): (0, 1, 5, 32, 0, 0, 0, -1, True, True, False),
    ('index_group_sum', 'more_passes', False): (0, 2, 11, 2048, 0, 0, 0, -1, True, True, False),
    ('index_group_sum', 'global_table', False): (1, 0, 0, 1, 0, 0, 0, -1, True, True, True),
    ('index_group_sum', 'fallback', False): (1, 0, 0, 1, 0, 0, 0, -1, True, True, True),
    ('lookup', 'zero_pass', True): (0, 0, 0, 1, 0, 0, 0, -1, False, True, False),
    ('lookup', 'one_pass', True): (0, 1, 5, 32, 0, 0, 0, -1, False, True, False),
    ('lookup', 'more_passes', True): (0, 2, 11, 2048, 0, 0, 0, -1, False, True, False),
    ('lookup', 'fallback', True): (1, 0, 0, 1, 1, 0, 0, -1, False, True, True),
    ('left_join', 'zero_pass', True): (0, 0, 0, 1, 0, 0, 0, -1, False, True, False),
    ('left_join', 'one_pass', True): (0, 1, 5, 32, 0, 0, 0, -1, False, True, False),
    ('left_join', 'more_passes', True): (0, 2, 11, 2048, 0, 0, 0, -1, False, True, False),
    ('left_join', 'fallback', True): (1, 0, 0, 1, 1, 0, 0, -1, False, True, True),
    ('full_join', 'zero_pass', True): (0, 0, 0, 1, 0, 0, 0, -1, False, False, False),
    ('full_join', 'one_pass', True): (0, 1, 5, 32, 0, 0, 0, -1, False, False, False),
    ('full_join', 'more_passes', True): (0, 2, 11, 2048, 0, 0, 0, -1, False, False, False),
    ('full_join', 'fallback', True): (1, 0, 0, 1, 1, 0, 0, -1, False, False, True),
    ('group_join_sum', 'zero_pass', True): (0, 0, 0, 1, 0, 0, 0, -1, False, True, False),
    ('group_join_sum', 'one_pass', True): (0, 1, 5, 32, 0, 0, 0, -1, False, True, False),
    ('group_join_sum', 'more_passes', True): (0, 2, 11, 2048, 0, 0, 0, -1, False, True, False),
    ('group_join_sum', 'fallback', True): (1, 0, 0, 1, 1, 0, 0, -1, False, True, True),
    ('factorize_columns', 'empty_build', False): (0, 0, 0, 0, 0, 0, 0, -1, True, True, True),
    ('factorize_columns', 'zero_pass', False): (0, 0, 0, 1, 0, 0, 0, -1, False, True, True),
    ('factorize_columns', 'one_pass', False): (0, 1, 5, 32, 0, 0, 0, -1, False, True, True),
    ('factorize_columns', 'more_passes', False): (0, 2, 11, 2048, 0, 0, 0, -1, False, True, True),
    ('factorize_columns', 'global_table', False): (1, 0, 0, 1, 0, 0, 0, -1, False, True, True),
    ('factorize_columns', 'fallback', False): (1, 0, 0, 1, 1, 0, 0, -1, False, True, True),
    ('group_by_agg_columns', 'empty_build', False): (0, 0, 0, 0, 0, 0, 0, -1, True, True, True),
    ('group_by_agg_columns', 'zero_pass', False): (0, 0, 0, 1, 0, 0, 0, -1, False, True, True),
    ('group_by_agg_columns', 'one_pass', False): (0, 1, 5, 32, 0, 0, 0, -1, False, True, True),
    ('group_by_agg_columns', 'more_passes', False): (0, 2, 11, 2048, 0, 0, 0, -1, False, True, True),
    ('group_by_agg_columns', 'global_table', False): (1, 0, 0, 1, 0, 0, 0, -1, False, True, True),
    ('group_by_agg_columns', 'fallback', False): (1, 0, 0, 1, 1, 0, 0, -1, False, True, True),
}


def test_the_table_is_complete():
    assert set(PINNED) == set(CELLS) and len(set(CELLS)) == len(CELLS)
    assert {f for f, _, _ in CELLS} == set(TWO) | set(ONE) and {r for _, r, _ in CELLS} == set(ROUTES)


def test_the_rows_are_what_the_routes_need():
    """(no GPU) sizes, duplicates and the skew the GPU cells rely on"""
    assert pair_rows("small").bk.size == NB_SMALL and pair_rows("large").bk.size == NB and pair_rows("large").pk.size == NP
    for shape in ("small", "large", "skewed"):
        r, d = pair_rows(shape), pair_rows(shape, True)
        assert r.unique_build and 0 < r.m < r.pk.size
        assert d.bk.size == r.bk.size and np.unique(d.bk).size == d.bk.size - d.bk.size // 10
    assert rel_rows("small").n == NB_SMALL and rel_rows("large").n == NB and rel_rows("skewed").n == NB
    assert 1 < rel_rows("small").g < NB_SMALL and rel_rows("skewed").g == NB
    words = pair64(rel_rows("skewed").a, rel_rows("skewed").b)
    assert np.unique(words[keymix.partition_of(words, 5) == 7]).size >= SKEW


@pytest.mark.gpu
@pytest.mark.parametrize("form,route,dups", CELLS, ids=[f"{f}-{r}{'-dups' if d else ''}" for f, r, d in CELLS])
def test_cell(api, form, route, dups):
    got = run_cell(api, form, route, dups)
    print(form, route, dups, got)
    assert got == PINNED[form, route, dups]
