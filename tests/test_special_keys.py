"""The hash-domain empty marker and filler keys on every join path.

Every 64-bit value is a legal key; the kernels keep that promise with out-of-band code for FJ_EMPTY_KEY (all ones).  Chunk pools and
LDS tables hold MIXED keys, so on every partitioned kernel the marker is the raw key keymix.EMPTY_RAW = unmix(2^64 - 1) and the wide
kernel's filler (W_POISON2) is keymix.FILLER_RAW; raw 2^64 - 1 is the marker on the HBM-table path only.  keymix.special_raw_keys
lists them with their neighbours; the CPU tests below pin that list to the sources, the GPU tests plant it in random 64-bit keys and
compare every public function, on every path the suite knows how to force, with a sort-based NumPy reference - exactly: sorted pair
sets, counts, gather maps, the -1 / fill_value ranges.

Reference: oracle.np_join / np_inner_join (stable argsort + searchsorted), test_full_join._np_full, test_outer_all_copies._np_ref,
test_row_ids.ref_indices - no hashing anywhere, never the library.

Data: four arrangements (specials on both sides / the build side only / the probe side only / neither) x three variants:
  marker_x3        a duplicate-free build side in which the marker alone appears three times, with distinct values
  marker_hot       the marker takes 20 000 probe rows (80 chunks of its partition's probe list)
  marker_unprobed  two copies of the marker on the build side, none on the probe side: a FULL join owes both copies to the r
                   unmatched build rows (in the other variants of "both" the marker's build row IS probed)
A variant changes the sides its arrangement plants on; the partition-edge keys of special_raw_keys are planted for every radix_bits
in 0..20, so they sit in the last / first partition of whatever plan a case takes.
The two-pass plan (3M build rows) runs on device tensors only: the host entry copies and calls the same fj_join_device."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import keymix
from conftest import ROOT

U64_MAX = np.uint64(2**64 - 1)
MARKER = np.uint64(keymix.EMPTY_RAW)
ODD = np.uint64(0x9E3779B97F4A7C15)
MANY, LEFT, ANTI, ROW_IDS, FULL, ALL = 0x10, 0x20, 0x40, 0x80, 0x100, 0x200
HOT_ROWS = 20_000

COUNT_FUNCS = ["adaptive_join_count", "adaptive_join_count_bloom", "hash_join_count", "hash_join_count_bloom",
               "hash_join_count_radix", "hash_join_count_radix_bloom"]
MAT_FUNCS = ["adaptive_join", "adaptive_join_bloom", "hash_join", "hash_join_bloom", "hash_join_radix", "hash_join_radix_bloom"]
ARRANGEMENTS = ["both", "build_only", "probe_only", "neither"]
VARIANTS = ["marker_x3", "marker_hot", "marker_unprobed"]


def _specials():
    """names and raw keys of special_raw_keys(radix_bits) for radix_bits 0..20, each key once"""
    names, keys = [], []
    for rb in range(21):
        for n, k in zip(*keymix.special_raw_keys(rb)):
            if n not in names and k not in keys:                      # (mix(0) == 0: raw zero IS mixed zero)
                names.append(n)
                keys.append(k)
    return names, np.array(keys, dtype=np.uint64)


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def _source(name):
    with open(os.path.join(ROOT, "flash_hash_join_amd", "csrc", name)) as f:
        return f.read()


def test_the_special_list_stands_for_the_kernels_own_constants():
    m = re.search(r"#define\s+FJ_EMPTY_KEY\s+(0x[0-9a-fA-F]+)", _source("fj_common.h"))
    assert m, "csrc/fj_common.h no longer defines FJ_EMPTY_KEY: tests/keymix.py special_raw_keys stands for nothing"
    assert int(m.group(1), 16) == keymix.EMPTY_MIXED, f"FJ_EMPTY_KEY is {m.group(1)}, keymix.EMPTY_MIXED {keymix.EMPTY_MIXED:#x}: update tests/keymix.py"
    m = re.search(r"constexpr\s+u64\s+W_POISON2\s*=\s*(0x[0-9a-fA-F]+)", _source("fj_join_wide.hip"))
    assert m, "csrc/fj_join_wide.hip no longer defines W_POISON2: tests/keymix.py FILLER_MIXED stands for nothing"
    assert int(m.group(1), 16) == keymix.FILLER_MIXED, f"W_POISON2 is {m.group(1)}, keymix.FILLER_MIXED {keymix.FILLER_MIXED:#x}: update tests/keymix.py"


def test_empty_raw_is_the_known_word():
    assert keymix.EMPTY_RAW == 0xff804af1fc8405c4
    assert keymix.FILLER_RAW == 0xc68a9155edf8d673
    assert int(keymix.mix(np.array([2**64 - 1], dtype=np.uint64))[0]) == 0xc01a328255bf9528      # raw 2^64 - 1: an ordinary key of the hash domain


@pytest.mark.parametrize("radix_bits", [0, 5, 9, 17, 31])
def test_special_keys_are_the_library_s_unmix_of_the_listed_words(radix_bits):
    from flash_hash_join_amd import _lib
    L = _lib.load()
    words = keymix.special_mixed_words(radix_bits)
    names, raw = keymix.special_raw_keys(radix_bits)
    assert names[:len(words)] == [n for n, _ in words] and names[len(words):] == ["raw_all_ones", "raw_zero"]
    assert len(set(names)) == len(names) and np.unique(raw).size == raw.size - 1       # mix(0) == 0: raw zero is mixed zero, listed under both names
    for (name, w), k in zip(words, raw.tolist()):
        assert L.fj_key_unmix64(w) == k and L.fj_key_mix64(k) == w, name
    assert raw[-2] == U64_MAX and raw[-1] == 0
    mixed = dict(words)
    assert mixed["marker"] == 2**64 - 1 and mixed["marker_minus_1"] == 2**64 - 2 and mixed["mixed_zero"] == 0 and mixed["mixed_one"] == 1
    assert mixed["wide_filler"] == 0x00000000FFFFFFFF and mixed["high_word_ones"] == 0xFFFFFFFF00000000
    last, first = mixed[f"last_partition_low_ones_{radix_bits}"], mixed[f"first_partition_low_ones_{radix_bits}"]
    assert last & 0xFFFFFFFF == first & 0xFFFFFFFF == 0xFFFFFFFF                      # the home slot of the marker and the filler
    assert last not in (mixed["marker"], mixed["wide_filler"]) and first not in (mixed["marker"], mixed["wide_filler"])
    if radix_bits:
        assert last >> (64 - radix_bits) == (1 << radix_bits) - 1 and first >> (64 - radix_bits) == 0
    assert raw[0] == keymix.EMPTY_RAW and raw[4] == keymix.FILLER_RAW


def test_the_planted_set_and_the_case_generator():
    names, keys = _specials()
    assert np.unique(keys).size == keys.size == 6 + 2 * 21 + 1
    for arrangement in ARRANGEMENTS:
        for variant in VARIANTS:
            d = _make(3000, 50_000, arrangement, variant)
            on_b, on_p = arrangement in ("both", "build_only"), arrangement in ("both", "probe_only")
            assert np.isin(keys, d.bk).all() == on_b and np.isin(keys, d.bk).any() == on_b
            want_p = keys if variant != "marker_unprobed" else keys[keys != MARKER]
            assert np.isin(want_p, d.pk).all() == on_p and np.isin(keys, d.pk).any() == on_p
            nm = int((d.bk == MARKER).sum())
            assert nm == (0 if not on_b else {"marker_x3": 3, "marker_hot": 1, "marker_unprobed": 2}[variant])
            u, c = np.unique(d.bk, return_counts=True)
            assert np.all(c[u != MARKER] == 1), "a build key other than the marker is duplicated"
            assert np.unique(d.bv).size == d.bv.size
            if on_p and variant == "marker_hot":
                assert int((d.pk == MARKER).sum()) >= HOT_ROWS
            if arrangement == "probe_only":                            # every special probe row must come back unmatched
                assert np.isin(d.full[3], keys).sum() == np.isin(d.pk, keys).sum() > 0
            if arrangement == "build_only" or (on_b and variant == "marker_unprobed"):
                assert int((d.full[4] == MARKER).sum()) == nm           # the marker among the r unmatched build rows, once per copy


# ---- data and reference ------------------------------------------------------------------------------------------------------
def _canon(k, v):
    from oracle.oracle import canon_pairs
    return canon_pairs(np.asarray(k).view(np.uint64), np.asarray(v).view(np.uint64))


class Case:
    def __init__(self, bk, bv, pk):
        self.bk, self.bv, self.pk = bk, bv, pk
        self._dev = None

    @functools.cached_property
    def full(self):
        """(m, matched keys, matched values, unmatched probe keys, unmatched build keys, their values): first occurrence"""
        from test_full_join import _np_full
        m, k, v, anti, rk, rv = _np_full(self.bk, self.bv, self.pk)
        return (m,) + _canon(k, v) + (anti,) + _canon(rk, rv)                   # (pairs in canonical order: sorted once)

    @functools.cached_property
    def allc(self):
        """(P, pair keys, pair values, unmatched probe keys, unmatched build keys, their values): every copy"""
        from test_outer_all_copies import _np_ref
        P, k, v, anti, rk, rv = _np_ref(self.bk, self.bv, self.pk)
        return (P,) + _canon(k, v) + (anti,) + _canon(rk, rv)

    @functools.cached_property
    def first_idx(self):
        from test_row_ids import ref_indices, _pairs
        return _pairs(*ref_indices(self.bk, self.pk))

    @functools.cached_property
    def many_idx(self):
        from test_row_ids import ref_indices, _pairs
        return _pairs(*ref_indices(self.bk, self.pk, many=True))

    def args(self, device):
        if not device:
            return self.bk, self.bv, self.pk
        if self._dev is None:
            import torch
            self._dev = tuple(torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda() for a in (self.bk, self.bv, self.pk))
        return self._dev


@functools.lru_cache(maxsize=4)
def _make(nb, n_p, arrangement, variant, hit=0.5):
    _, S = _specials()
    rng = np.random.default_rng(nb % 1000 + 7 * ARRANGEMENTS.index(arrangement) + 31 * VARIANTS.index(variant))
    on_b, on_p = arrangement in ("both", "build_only"), arrangement in ("both", "probe_only")
    plain = np.unique(rng.integers(0, 2**64, size=nb, dtype=np.uint64))
    plain = plain[~np.isin(plain, S)]
    rng.shuffle(plain)
    extra_b = []
    if on_b:
        extra_b = [S] + {"marker_x3": [np.full(2, MARKER)], "marker_hot": [], "marker_unprobed": [np.full(1, MARKER)]}[variant]
    bk = np.concatenate([plain] + extra_b)
    bk = bk[rng.permutation(bk.size)]
    bv = (np.arange(bk.size, dtype=np.uint64) + np.uint64(1)) * ODD                  # distinct: every copy of a key is recognisable
    nhit = int(n_p * hit)
    miss = rng.integers(0, 2**64, size=n_p - nhit, dtype=np.uint64)
    miss = miss[~np.isin(miss, S) & ~np.isin(miss, plain)]
    extra_p = []
    if on_p:
        Sp = S if variant != "marker_unprobed" else S[S != MARKER]
        extra_p = [np.repeat(Sp, 3)] + ([np.full(HOT_ROWS, MARKER)] if variant == "marker_hot" else [])
    pk = np.concatenate([rng.choice(plain[: max(1, plain.size * 7 // 10)], nhit), miss] + extra_p)      # 30 % of the build rows are never probed
    pk = pk[rng.permutation(pk.size)]
    return Case(bk, bv, pk)


def _u64(a):
    return a.cpu().numpy().view(np.uint64) if hasattr(a, "cpu") else np.asarray(a).view(np.uint64)


def _i64(a):
    return _u64(a).view(np.int64)


def _same_pairs(k1, v1, k2, v2):
    """(k2, v2): a Case's reference pairs, already in canonical order"""
    a = _canon(_u64(k1), _u64(v1))
    return a[0].size == k2.size and np.array_equal(a[0], k2) and np.array_equal(a[1], v2)


def _sorted(a):
    return np.sort(_u64(a).reshape(-1))


def _same_idx(pi, bi, epi, ebi):
    from test_row_ids import _pairs
    a = _pairs(_i64(pi), _i64(bi))                                     # (epi, ebi): a Case's reference, already sorted
    return a[0].size == epi.size and np.array_equal(a[0], epi) and np.array_equal(a[1], ebi)


# ---- the checks: every public function against the reference ---------------------------------------------------------------------
def check_counts(fj, d, device, funcs=COUNT_FUNCS, after=None, many=True):
    a = d.args(device)
    m, P, n_p = d.full[0], d.allc[0], d.pk.size
    for fn in funcs:
        n = getattr(fj, fn)(*a)[0]
        print(f"{fn}: {n} (expected {m})")
        assert n == m, fn
        if after:
            after(fn, fj.last_timings())
    for fn, n, exp in (("semi_join_count", fj.semi_join_count(a[0], a[2])[0], m), ("anti_join_count", fj.anti_join_count(a[0], a[2])[0], n_p - m)):
        print(f"{fn}: {n} (expected {exp})")
        assert n == exp, fn
        if after:
            after(fn, fj.last_timings())
    if many:
        n = fj.inner_join_count(*a)[0]
        print(f"inner_join_count: {n} (expected {P})")
        assert n == P


def check_pairs(fj, d, device, funcs=MAT_FUNCS, after=None, first=True):
    """first=False (the HBM table's inner join: inserts race as in the reference's scalar path, hash_join.cpp:125, so ANY copy of a
    duplicated build key may give the value): the keys are exact, every value is the value of a build row with that key."""
    a = d.args(device)
    m, ek, ev = d.full[:3]
    by_val = np.argsort(d.bv)
    for fn in funcs:
        n, _, k, v = getattr(fj, fn)(*a, return_arrays=True)
        lt = fj.last_timings()
        print(f"{fn}: {n} pairs (expected {m})")
        if first:
            assert n == m and _same_pairs(k, v, ek, ev), f"{fn}: pairs differ from np_join (first occurrence)"
        else:
            k, v = _u64(k), _u64(v)
            row = by_val[np.minimum(np.searchsorted(d.bv[by_val], v), d.bv.size - 1)]
            assert n == m and np.array_equal(np.sort(k), ek), f"{fn}: matched keys"
            assert np.array_equal(d.bv[row], v) and np.array_equal(d.bk[row], k), f"{fn}: a value is not a build row's of that key"
        assert getattr(fj, fn)(*a)[0] == m, fn
        if after:
            after(fn, lt)


def check_extensions(fj, d, device, after=None, fill=2**64 - 3, many=True):
    """inner_join, left_join, anti_join, semi_join, full_join - keys / values, duplicates "first" and "all" """
    a = d.args(device)
    n_p = d.pk.size
    m, ek, ev, anti, rk, rv = d.full
    P, ik, iv, _, _, _ = d.allc
    u_exp, r_exp = anti.size, rk.size
    note = (lambda fn: after(fn, fj.last_timings())) if after else (lambda fn: None)
    if many:
        n, _, k, v = fj.inner_join(*a, return_arrays=True)
        assert n == P and _same_pairs(k, v, ik, iv), "inner_join: pairs differ from np_inner_join"
    n, _, k, v = fj.left_join(*a, return_arrays=True, fill_value=fill)
    note("left_join")
    k, v = _u64(k), _u64(v)
    assert n == m and k.size == n_p and _same_pairs(k[:m], v[:m], ek, ev), "left_join: matched rows"
    assert np.array_equal(_sorted(k[m:]), _sorted(anti)) and np.all(v[m:] == np.uint64(fill)), "left_join: unmatched rows"
    n, _, k = fj.anti_join(a[0], a[2], return_arrays=True)
    note("anti_join")
    assert n == u_exp and np.array_equal(_sorted(k), _sorted(anti)), "anti_join"
    n, _, k = fj.semi_join(a[0], a[2], return_arrays=True)
    note("semi_join")
    assert n == m and np.array_equal(_sorted(k), _sorted(ek)), "semi_join"
    n, r, _, k, v = fj.full_join(*a, return_arrays=True, fill_value=fill)
    note("full_join")
    k, v = _u64(k), _u64(v)
    print(f"full_join: m={n} (expected {m}) r={r} (expected {r_exp})")
    assert (n, r) == (m, r_exp) and k.size == n_p + r
    assert _same_pairs(k[:m], v[:m], ek, ev), "full_join: matched rows"
    assert np.array_equal(_sorted(k[m:n_p]), _sorted(anti)) and np.all(v[m:n_p] == np.uint64(fill)), "full_join: unmatched probe rows"
    assert _same_pairs(k[n_p:], v[n_p:], rk, rv), "full_join: unmatched build rows differ from (bk, bv)[~isin(bk, pk)]"
    if not many:
        return
    n, u, _, k, v = fj.left_join(*a, return_arrays=True, fill_value=fill, duplicates="all")
    k, v = _u64(k), _u64(v)
    assert (n, u) == (P, u_exp) and k.size == P + u and _same_pairs(k[:P], v[:P], ik, iv), "left_join(all): pairs"
    assert np.array_equal(_sorted(k[P:]), _sorted(anti)) and np.all(v[P:] == np.uint64(fill)), "left_join(all): unmatched rows"
    n, u, r, _, k, v = fj.full_join(*a, return_arrays=True, fill_value=fill, duplicates="all")
    k, v = _u64(k), _u64(v)
    print(f"full_join(all): P={n} (expected {P}) u={u} (expected {u_exp}) r={r} (expected {r_exp})")
    assert (n, u, r) == (P, u_exp, r_exp) and k.size == P + u + r and _same_pairs(k[:P], v[:P], ik, iv), "full_join(all): pairs"
    assert np.array_equal(_sorted(k[P:P + u]), _sorted(anti)) and np.all(v[P:P + u] == np.uint64(fill)), "full_join(all): unmatched probe rows"
    assert _same_pairs(k[P + u:], v[P + u:], rk, rv), "full_join(all): unmatched build rows"


def check_indices(fj, d, device, after=None, many=True):
    """join_indices: every how, many_to_many, duplicates="all" """
    from test_outer_all_copies import _check_row_ids
    a = d.args(device)
    bk, pk = d.bk, d.pk
    n_p = pk.size
    epi, ebi = d.first_idx
    mpi, mbi = d.many_idx
    m, P = epi.size, mpi.size
    hit = np.zeros(n_p, dtype=bool)
    hit[epi] = True
    miss = np.flatnonzero(~hit)
    rest = np.flatnonzero(~np.isin(bk, pk))
    note = (lambda fn: after(fn, fj.last_timings())) if after else (lambda fn: None)
    n, _, pi, bi = fj.join_indices(a[0], a[2])
    note("join_indices(inner)")
    assert n == m and _same_idx(pi, bi, epi, ebi), "inner: not (probe row, FIRST build row)"
    n, _, pi, bi = fj.join_indices(a[0], a[2], how="left")
    note("join_indices(left)")
    pi, bi = _i64(pi), _i64(bi)
    assert n == m and pi.size == n_p and _same_idx(pi[:m], bi[:m], epi, ebi), "left: matched range"
    assert np.array_equal(np.sort(pi[m:]), miss) and np.all(bi[m:] == -1), "left: unmatched range"
    n, _, pi, none = fj.join_indices(a[0], a[2], how="anti")
    note("join_indices(anti)")
    assert n == miss.size and none is None and np.array_equal(np.sort(_i64(pi)), miss), "anti"
    n, _, pi, none = fj.join_indices(a[0], a[2], how="semi")
    note("join_indices(semi)")
    assert n == m and none is None and np.array_equal(np.sort(_i64(pi)), np.sort(epi)), "semi"
    n, r, _, pi, bi = fj.join_indices(a[0], a[2], how="full")
    note("join_indices(full)")
    pi, bi = _i64(pi), _i64(bi)
    assert (n, r) == (m, rest.size) and pi.size == n_p + r and _same_idx(pi[:m], bi[:m], epi, ebi), "full: matched range"
    assert np.array_equal(np.sort(pi[m:n_p]), miss) and np.all(bi[m:n_p] == -1), "full: unmatched probe range"
    assert np.all(pi[n_p:] == -1) and np.array_equal(np.sort(bi[n_p:]), rest), "full: every unmatched build row exactly once"
    if not many:
        return
    for kw in (dict(many_to_many=True), dict(duplicates="all")):
        n, _, pi, bi = fj.join_indices(a[0], a[2], **kw)
        assert n == P and _same_idx(pi, bi, mpi, mbi), f"inner {kw}: pair set"
    n, u, _, pi, bi = fj.join_indices(a[0], a[2], how="left", duplicates="all")
    assert (n, u) == (P, miss.size) and _same_idx(_i64(pi)[:P], _i64(bi)[:P], mpi, mbi), "left(all): pair set"
    _check_row_ids(bk, pk, P, u, 0, pi, bi, full=False)
    assert np.array_equal(np.sort(_i64(pi)[P:]), miss)
    n, u, r, _, pi, bi = fj.join_indices(a[0], a[2], how="full", duplicates="all")
    assert (n, u, r) == (P, miss.size, rest.size) and _same_idx(_i64(pi)[:P], _i64(bi)[:P], mpi, mbi), "full(all): pair set"
    _check_row_ids(bk, pk, P, u, r, pi, bi)
    assert np.array_equal(np.sort(_i64(pi)[P:P + u]), miss)


def check_all(fj, d, device, after=None):
    check_counts(fj, d, device, after=after)
    check_pairs(fj, d, device, after=after)
    check_extensions(fj, d, device, after=after)
    check_indices(fj, d, device, after=after)


# ---- GPU -------------------------------------------------------------------------------------------------------------------
OPTION_DEFAULTS = {"plan_target_keys": 4096, "join_wide": 2, "persistent_min_items": 8192, "mat_single_pass": 1, "lab_hooks": 0,
                   "scalar_hbm_table": 0, "radix_threshold": 0}


@pytest.fixture(scope="module")
def fj():
    import flash_join
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_device_count() >= 1, "no HIP device: the product path must not silently fall back"
    assert flash_join.initialize() is None
    return flash_join


@pytest.fixture
def opts(fj):
    """set(name, value); every option is back at its default after the test"""
    yield fj.set_option
    for name, value in OPTION_DEFAULTS.items():
        fj.set_option(name, value)


DEPTHS = {   # id: nb, np, plan_target_keys, passes of an N:1 plan
    "zero_pass": (3000, 50_000, 4096, lambda p: p == 0),
    "one_pass": (100_000, 200_000, 4096, lambda p: p == 1),
    "two_pass": (3_000_000, 500_000, 4096, lambda p: p == 2),
    "deep": (60_000, 150_000, 32, lambda p: p >= 2),
}
GRID = [(a, v) for a in ARRANGEMENTS for v in VARIANTS]
GRID_IDS = [f"{a}-{v}" for a, v in GRID]


def _streamed(fn, device):
    """a counting inner join on host arrays: the host entry streams the probe side under its copy (fj_stream_*: its own table form for
    a zero-pass plan, no bloom precheck) - exact like every other call, but it reports that form's path"""
    return not device and (fn in COUNT_FUNCS or fn == "semi_join_count")


def _planned(passes, device):
    """the partitioned plan, at this depth, without the HBM-table fallback - of every N:1 call (the many-to-many plan aims at
    half as many rows per partition and is checked on its own)"""
    def after(fn, lt):
        if _streamed(fn, device):
            return
        assert lt["path"] == 0 and lt["fell_back"] == 0 and passes(lt["passes"]), (fn, lt)
    return after


@pytest.mark.gpu
@pytest.mark.parametrize("depth,device", [("zero_pass", False), ("zero_pass", True), ("one_pass", False), ("one_pass", True),
                                          ("deep", False), ("deep", True), ("two_pass", True)],
                         ids=["zero_pass-numpy", "zero_pass-device", "one_pass-numpy", "one_pass-device", "deep-numpy", "deep-device", "two_pass-device"])
@pytest.mark.parametrize("arrangement,variant", GRID, ids=GRID_IDS)
def test_every_function_at_every_plan_depth(fj, opts, depth, device, arrangement, variant):
    nb, n_p, target, passes = DEPTHS[depth]
    d = _make(nb, n_p, arrangement, variant)
    opts("plan_target_keys", target)
    check_all(fj, d, device, after=_planned(passes, device))
    if depth in ("two_pass", "deep"):
        fj.inner_join_count(*d.args(device))
        assert fj.last_timings()["path"] == 0 and fj.last_timings()["passes"] >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("depth", ["one_pass", "deep"])
@pytest.mark.parametrize("knob,value", [("join_wide", 0), ("join_wide", 1), ("persistent_min_items", 1), ("persistent_min_items", 1 << 30)],
                         ids=["cuckoo_kernel", "wide_kernel", "persistent_kernel", "no_persistent_kernel"])
@pytest.mark.parametrize("arrangement,variant", GRID, ids=GRID_IDS)
def test_counting_kernels(fj, opts, knob, value, depth, arrangement, variant):
    """The counting joins on the wide (16384-slot, filled with all ones, refilled with W_POISON2 before the last partition) and the
    cuckoo kernel, on the persistent kernel and without it.  Many partitions per workgroup on the deep plan."""
    nb, n_p, target, passes = DEPTHS[depth]
    d = _make(nb, n_p, arrangement, variant)
    opts("plan_target_keys", target)
    opts(knob, value)

    for device in (False, True):
        def after(fn, lt):
            if not _streamed(fn, device):
                assert lt["path"] == 0 and lt["fell_back"] == 0 and lt["lds_retries"] == 0 and passes(lt["passes"]), (fn, lt)
        check_counts(fj, d, device, after=after)


@pytest.mark.gpu
@pytest.mark.parametrize("arrangement,variant", GRID, ids=GRID_IDS)
def test_bloom_functions_keep_the_marker(fj, opts, arrangement, variant):
    """The *_bloom functions on a plan of at least two passes: the precheck runs (bloom_level >= 1) and the marker passes its own
    filter - every copy of a hot marker, too."""
    nb, n_p, target, passes = DEPTHS["deep"]
    d = _make(nb, n_p, arrangement, variant)
    opts("plan_target_keys", target)

    def after(fn, lt):
        assert lt["path"] == 0 and lt["fell_back"] == 0 and lt["passes"] >= 2 and lt["bloom_level"] >= 1, (fn, lt)
    for device in (False, True):
        check_counts(fj, d, device, funcs=["hash_join_count_radix_bloom", "hash_join_count_bloom"])
        a = d.args(device)
        for fn in ("hash_join_count_radix_bloom", "hash_join_count_bloom"):
            assert getattr(fj, fn)(*a)[0] == d.full[0]
            if not _streamed(fn, device):
                after(fn, fj.last_timings())
        check_pairs(fj, d, device, funcs=["hash_join_radix_bloom", "hash_join_bloom"], after=after)


@pytest.mark.gpu
@pytest.mark.parametrize("single,hooks,persistent", [(1, 0, 8192), (0, 0, 8192), (1, 32, 8192), (1, 64, 1), (0, 64, 1), (1, 0, 1)],
                         ids=["single_pass", "count_then_emit", "emit_on_the_tagged_kernel", "emit_retry_every_7th", "emit_retry_every_7th_two_phase",
                              "persistent_emit"])
@pytest.mark.parametrize("arrangement,variant", GRID, ids=GRID_IDS)
def test_materialising_joins(fj, opts, single, hooks, persistent, arrangement, variant):
    """mat_single_pass 1 / 0; lab hook 32 puts the emitting pass on the tagged kernel, hook 64 sends every 7th item of the persistent
    emit kernel down its retry path (the scoreboard's 0xFFFF code and an empty_val that must survive the pending round)."""
    nb, n_p, target, passes = DEPTHS["one_pass"]
    d = _make(nb, n_p, arrangement, variant)
    opts("mat_single_pass", single)
    opts("lab_hooks", hooks)
    opts("persistent_min_items", persistent)

    def after(fn, lt):
        assert lt["path"] == 0 and lt["fell_back"] == 0 and lt["passes"] == 1, (fn, lt)
        if hooks == 64 and fn == "hash_join_radix" and not (d.bk == MARKER).sum() > 1:
            assert lt["lds_retries"] >= 1, (fn, lt)                    # (duplicates send the join to the first-occurrence form instead)
    for device in (False, True):
        check_pairs(fj, d, device, after=after)
        a = d.args(device)
        n, _, pi, bi = fj.join_indices(a[0], a[2])
        after("join_indices", fj.last_timings())
        assert n == d.full[0] and _same_idx(pi, bi, *d.first_idx)
        n, _, k, v = fj.inner_join(*a, return_arrays=True)
        assert n == d.allc[0] and _same_pairs(k, v, *d.allc[1:3])


def _last_partition_candidates():
    from test_row_ids import _hash_w1
    cand = np.arange(1, 1_000_000, dtype=np.uint64)
    part = _hash_w1(cand) >> np.uint32(27)                             # top 5 hash bits: the partition of a 32-partition plan
    assert _hash_w1(np.array([MARKER]))[0] >> np.uint32(27) == 31       # the marker's partition is the last one
    return cand, cand[part == 31], cand[part != 31]


@functools.lru_cache(maxsize=1)
def _ladder_case(n_last, arrangement, variant):
    """n_last distinct keys in the LAST of the plan's 32 partitions - the marker's - plus 3000 elsewhere, the specials planted by
    arrangement / variant as in _make"""
    _, S = _specials()
    cand, last, rest = _last_partition_candidates()
    assert last.size >= n_last
    on_b, on_p = arrangement in ("both", "build_only"), arrangement in ("both", "probe_only")
    rng = np.random.default_rng(n_last)
    extra_b = []
    if on_b:
        extra_b = [S] + {"marker_x3": [np.full(2, MARKER)], "marker_hot": [], "marker_unprobed": [np.full(1, MARKER)]}[variant]
    bk = np.concatenate([last[:n_last], rest[:3000]] + extra_b)
    bk = bk[rng.permutation(bk.size)]
    bv = (np.arange(bk.size, dtype=np.uint64) + np.uint64(1)) * ODD
    extra_p = []
    if on_p:
        Sp = S if variant != "marker_unprobed" else S[S != MARKER]
        extra_p = [np.repeat(Sp, 3)] + ([np.full(HOT_ROWS, MARKER)] if variant == "marker_hot" else [])
    pk = np.concatenate([last[:n_last:2], rest[:3000:3], cand[-60000:]] + extra_p)
    pk = pk[rng.permutation(pk.size)]
    return Case(bk, bv, pk)


@pytest.mark.gpu
@pytest.mark.parametrize("arrangement,variant", GRID, ids=GRID_IDS)
def test_overflow_ladder_beyond_the_cuckoo_table(fj, arrangement, variant):
    """6000 build keys in the marker's partition: too many for the cuckoo table, fine for the tagged one - that partition's items are
    redone (lds_retries >= 1), no HBM-table fallback.  N:1 functions only: the many-to-many kernels refuse a partition of more than
    4096 build rows by contract."""
    d = _ladder_case(6000, arrangement, variant)
    for device in (False, True):
        a = d.args(device)
        assert fj.hash_join_count_radix(*a)[0] == d.full[0]
        lt = fj.last_timings()
        assert lt["path"] == 0 and lt["fell_back"] == 0 and lt["lds_retries"] >= 1, lt
        check_counts(fj, d, device, many=False)
        check_pairs(fj, d, device, funcs=["hash_join_radix", "adaptive_join"], after=lambda fn, lt: lt["fell_back"] == 0 or pytest.fail(f"{fn}: {lt}"))
        check_extensions(fj, d, device, many=False)
        check_indices(fj, d, device, many=False)


@pytest.mark.gpu
@pytest.mark.parametrize("arrangement,variant", GRID, ids=GRID_IDS)
def test_overflow_ladder_beyond_the_lds_table(fj, arrangement, variant):
    """9000 keys in the marker's partition: the inner join re-partitions that partition alone (lds_retries >= 2); 20 000: the full
    join runs again on the HBM table (fell_back == 1), where raw 2^64 - 1 is the marker."""
    d = _ladder_case(9000, arrangement, variant)
    for device in (False, True):
        a = d.args(device)
        n, _, pi, bi = fj.join_indices(a[0], a[2])
        lt = fj.last_timings()
        assert n == d.first_idx[0].size and _same_idx(pi, bi, *d.first_idx)
        assert lt["fell_back"] == 0 and lt["lds_retries"] >= 2, lt
        check_pairs(fj, d, device, funcs=["hash_join_radix"])
        check_counts(fj, d, device, funcs=["hash_join_count_radix"], many=False)
    d = _ladder_case(20000, arrangement, variant)
    for device in (False, True):
        a = d.args(device)
        m, r = fj.full_join(*a)[:2]
        assert fj.last_timings()["fell_back"] == 1, fj.last_timings()
        assert (m, r) == (d.full[0], d.full[4].size)
        fj.join_indices(a[0], a[2], how="full")
        assert fj.last_timings()["fell_back"] == 1, fj.last_timings()
        check_extensions(fj, d, device, many=False)
        check_indices(fj, d, device, many=False)
        check_counts(fj, d, device, many=False)
        check_pairs(fj, d, device, funcs=["hash_join_radix"])


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["scalar_hbm_table", "radix_threshold"])
@pytest.mark.parametrize("arrangement,variant", GRID, ids=GRID_IDS)
def test_hbm_table_paths(fj, opts, route, arrangement, variant):
    """The HBM table stores raw keys: raw 2^64 - 1 is its marker (flags[0] / empty_val and the matched-bitmap word behind the table),
    the mixed specials are ordinary keys - both are planted."""
    from flash_hash_join_amd import api
    nb, n_p, _, _ = DEPTHS["one_pass"]
    d = _make(nb, n_p, arrangement, variant)
    m, ek, ev, anti, rk, rv = d.full
    n_p = d.pk.size

    def on_table(fn, lt):
        assert lt["path"] == 1, (fn, lt)
    if route == "radix_threshold":
        opts("radix_threshold", 10**9)
        for device in (False, True):
            check_counts(fj, d, device, funcs=["adaptive_join_count", "adaptive_join_count_bloom"], after=on_table)
            check_pairs(fj, d, device, funcs=["adaptive_join", "adaptive_join_bloom"], after=on_table, first=False)
            check_extensions(fj, d, device, after=on_table)
            check_indices(fj, d, device, after=on_table)
        return
    opts("scalar_hbm_table", 1)
    for device in (False, True):
        a = d.args(device)
        check_counts(fj, d, device, funcs=["hash_join_count", "hash_join_count_bloom"], after=lambda fn, lt: fn.startswith("hash_join") and on_table(fn, lt))
        check_pairs(fj, d, device, funcs=["hash_join", "hash_join_bloom"], after=on_table, first=False)
        S = api.ALGO_SCALAR
        n, _, k, v = api._join(S | LEFT, 0, 1, *a, True)
        on_table("left", fj.last_timings())
        k, v = _u64(k), _u64(v)
        assert n == m and _same_pairs(k[:m], v[:m], ek, ev) and np.array_equal(_sorted(k[m:]), _sorted(anti)) and np.all(v[m:] == 0)
        n, _, k, _ = api._join(S | ANTI, 0, 1, a[0], None, a[2], True)
        on_table("anti", fj.last_timings())
        assert n == anti.size and np.array_equal(_sorted(k), _sorted(anti))
        assert api._join(S | ANTI, 0, 0, a[0], None, a[2], False)[0] == anti.size
        on_table("anti_count", fj.last_timings())
        (n, r), _, k, v = api._join(S | FULL, 0, 1, *a, True)
        on_table("full", fj.last_timings())
        k, v = _u64(k), _u64(v)
        assert (n, r) == (m, rk.size) and k.size == n_p + r and _same_pairs(k[:m], v[:m], ek, ev)
        assert np.array_equal(_sorted(k[m:n_p]), _sorted(anti)) and np.all(v[m:n_p] == 0) and _same_pairs(k[n_p:], v[n_p:], rk, rv)
        epi, ebi = d.first_idx
        n, _, pi, bi = api._join(S | ROW_IDS, 0, 1, a[0], None, a[2], True)
        on_table("row_ids", fj.last_timings())
        assert n == m and _same_idx(pi, bi, epi, ebi)
        n, _, pi, bi = api._join(S | ROW_IDS | LEFT, 0, 1, a[0], None, a[2], True)
        on_table("row_ids_left", fj.last_timings())
        assert n == m and _same_idx(_i64(pi)[:m], _i64(bi)[:m], epi, ebi) and np.all(_i64(bi)[m:] == -1)
        (n, r), _, pi, bi = api._join(S | ROW_IDS | FULL, 0, 1, a[0], None, a[2], True)
        on_table("row_ids_full", fj.last_timings())
        pi, bi = _i64(pi), _i64(bi)
        assert (n, r) == (m, rk.size) and _same_idx(pi[:m], bi[:m], epi, ebi) and np.all(bi[m:n_p] == -1) and np.all(pi[n_p:] == -1)
        assert np.array_equal(np.sort(bi[n_p:]), np.flatnonzero(~np.isin(d.bk, d.pk)))


@pytest.mark.gpu
@pytest.mark.parametrize("algo", [2, 2 | MANY, 2 | ROW_IDS, 2 | MANY | ROW_IDS, LEFT | ALL, FULL | ALL | ROW_IDS],
                         ids=["n_to_1", "many_to_many", "n_to_1_row_ids", "many_row_ids", "left_all", "full_all_row_ids"])
@pytest.mark.parametrize("arrangement,variant", GRID, ids=GRID_IDS)
def test_two_phase_form_of_the_c_abi(fj, algo, arrangement, variant):
    """fj_join_device counts (no output buffers), fj_emit_pairs writes the pending result; then the same join in one call."""
    import torch
    from flash_hash_join_amd import _lib, api
    L = _lib.load()
    nb, n_p, _, _ = DEPTHS["one_pass"]
    d = _make(nb, n_p, arrangement, variant)
    dbk, dbv, dpk = d.args(True)
    ctx = api.context(0)
    stream = torch.cuda.current_stream(0).cuda_stream
    cnt = (ctypes.c_uint64 * 3)(0, 0, 0)
    P, ik, iv, anti, rk, rv = d.allc
    if algo & ALL:
        exp = (P, rk.size if algo & FULL else 0, anti.size)
    else:
        exp = (P if algo & MANY else d.full[0], 0, 0)
    rows = sum(exp)

    def verify(k, v):
        k, v = _u64(k), _u64(v)
        if algo == LEFT | ALL:
            assert _same_pairs(k[:P], v[:P], ik, iv) and np.array_equal(_sorted(k[P:]), _sorted(anti)) and np.all(v[P:] == 0)
        elif algo & ALL:
            from test_outer_all_copies import _check_row_ids
            assert _same_idx(k[:P], v[:P], *d.many_idx)
            _check_row_ids(d.bk, d.pk, P, anti.size, rk.size, k, v)
        elif algo & ROW_IDS:
            assert _same_idx(k, v, *(d.many_idx if algo & MANY else d.first_idx))
        elif algo & MANY:
            assert _same_pairs(k, v, ik, iv)
        else:
            assert _same_pairs(k, v, d.full[1], d.full[2])
    with api._ctx_locks.setdefault(0, __import__("threading").RLock()):
        _lib.check(L.fj_join_device(ctx, algo, 0, 1, dbk.data_ptr(), dbv.data_ptr(), d.bk.size, dpk.data_ptr(), d.pk.size, stream, 64,
                                    cnt, None, None, 0, None))                        # counted, rows pending
        assert (int(cnt[0]), int(cnt[1]), int(cnt[2])) == exp
        ok = torch.full((rows + 1,), 12345, dtype=torch.int64, device="cuda")
        ov = torch.full((rows + 1,), 12345, dtype=torch.int64, device="cuda")
        _lib.check(L.fj_emit_pairs(ctx, ok.data_ptr(), ov.data_ptr(), rows, stream, None))
        assert int(ok[rows]) == 12345 and int(ov[rows]) == 12345, "a row behind the result was written"
        verify(ok[:rows], ov[:rows])
        ok.fill_(12345); ov.fill_(12345)
        cnt2 = (ctypes.c_uint64 * 3)(0, 0, 0)
        _lib.check(L.fj_join_device(ctx, algo, 0, 1, dbk.data_ptr(), dbv.data_ptr(), d.bk.size, dpk.data_ptr(), d.pk.size, stream, 64,
                                    cnt2, ok.data_ptr(), ov.data_ptr(), rows + 1, None))   # one call
        assert list(cnt2) == list(cnt) and int(ok[rows]) == 12345 and int(ov[rows]) == 12345
        verify(ok[:rows], ov[:rows])


@pytest.mark.gpu
@pytest.mark.parametrize("top", [64, 48])
@pytest.mark.parametrize("arrangement,variant", GRID, ids=GRID_IDS)
def test_streamed_join_with_both_sides_in_pieces(fj, top, arrangement, variant):
    """fj_stream_open / append_build / append_probe / finish == the one-shot join of the same rows == the reference"""
    from flash_hash_join_amd import api
    from flash_hash_join_amd.lab import LabEngine
    nb, n_p, _, _ = DEPTHS["one_pass"]
    d = _make(nb, n_p, arrangement, variant)
    bk, bv, pk = d.args(True)
    exp = d.full[0]
    assert api.join_device(api.ALGO_RADIX, 0, 0, bk, bv, pk, hash_top_bits=top)[0] == exp
    eng = LabEngine("cuda:0")
    bcuts = [bk.numel() * i // 3 for i in range(4)]
    pcuts = [pk.numel() * i // 4 for i in range(5)]
    for probe_first in (True, False):
        eng.stream_open(bk.numel(), 3, pk.numel(), 4, top)
        if probe_first:
            for i in range(4):
                eng.stream_append(pk[pcuts[i]: pcuts[i + 1]])
            eng.stream_advance_probe()
        for i in range(3):
            eng.stream_append_build(bk[bcuts[i]: bcuts[i + 1]])
        if not probe_first:
            for i in range(4):
                eng.stream_append(pk[pcuts[i]: pcuts[i + 1]])
        assert eng.stream_finish() == exp
    eng.stream_begin(bk, bv, pk.numel(), 4, top)                              # probe side in pieces over a whole build side
    for i in range(4):
        eng.stream_append(pk[pcuts[i]: pcuts[i + 1]].clone())
    assert eng.stream_finish() == exp


@pytest.mark.gpu
@pytest.mark.parametrize("arrangement,variant", GRID, ids=GRID_IDS)
def test_shuffled_chunk_form_and_the_wire_format(fj, arrangement, variant):
    """shuffle_pack / stream_append_chunks under a plan whose first pass has 512 buckets: the 7-byte wire format (1792-byte chunks:
    the top hash byte lives in the directory word) round-trips the specials, and the owner's join of the chunks equals the one-shot
    join of the same rows - counting, and with values when the build side has no duplicate."""
    import torch
    from flash_hash_join_amd.lab import LabEngine
    nb_total = 300_000_000
    nb, n_p, _, _ = DEPTHS["one_pass"]
    d = _make(nb, n_p, arrangement, variant)
    bk, bv, pk = d.args(True)
    eng = LabEngine("cuda:0")
    f0 = eng.shuffle_plan(nb_total, 1)
    assert f0 >= 8 and eng.shuffle_chunk_bytes(nb_total, 1) == 1792
    m, ek, ev = d.full[:3]
    assert fj.hash_join_count_radix(bk, bv, pk)[0] == m
    unique = np.unique(d.bk).size == d.bk.size
    bch, bdir, bused, bvals = eng.shuffle_pack(bk, bv, nb_total, 1)
    pcuts = [(pk.numel() * i // 2) & ~1 for i in range(2)] + [pk.numel()]
    ppieces = [eng.shuffle_pack(pk[pcuts[i]: pcuts[i + 1]], None, nb_total, 1) for i in range(2)]
    torch.cuda.synchronize()
    for rel, packs in ((d.bk, [(bch, bdir)]), (d.pk, [(p[0], p[1]) for p in ppieces])):
        seen = []
        for ch, dw in packs:
            keys, bucket, cnt = keymix.unpack_wire(ch[0].cpu().numpy(), dw[0].cpu().numpy(), f0)
            assert np.array_equal((keymix.hash_w1(keys) >> np.uint32(32 - f0)).astype(np.int64), bucket)
            seen.append(keys)
        assert np.array_equal(np.sort(np.concatenate(seen)), np.sort(rel)), "the wire format lost or changed a key"
    for with_vals in ([False, True] if unique else [False]):
        eng.stream_open_shuffled(nb_total, 1, 0, bused[0] * 256 + 1024, 1, sum(p[2][0] for p in ppieces) * 256 + 1024, 2, with_vals=with_vals)
        eng.stream_append_chunks(0, bch[0].clone(), bdir[0].clone(), bvals[0] if with_vals else None)
        for p in ppieces:
            eng.stream_append_chunks(1, p[0][0].clone(), p[1][0].clone())
        n = eng.stream_finish()
        lt = fj.last_timings()
        assert n == m and lt["fell_back"] == 0 and lt["passes"] >= 2, (n, m, lt)
        if with_vals:
            k, v = eng.emit_pairs(n)
            assert _same_pairs(k, v, ek, ev)


@pytest.mark.gpu
@pytest.mark.parametrize("target", [4096, 32], ids=["plan_4096", "plan_32"])
@pytest.mark.parametrize("arrangement,variant", GRID, ids=GRID_IDS)
def test_dense_build_broadcast_form(fj, opts, target, arrangement, variant):
    """bcast_pack / bcast_probe / bcast_join (fj_count_join_wide<DENSE>) of two ranks' blocks == the one-shot join of the same rows;
    both widths of the high-word plane (plan_target_keys 4096 / 32).  The form needs unique build keys: the marker's extra copies
    are dropped from this build side (marker_x3 keeps its one marker row)."""
    import torch
    from flash_hash_join_amd.lab import LabEngine
    nb, n_p, _, _ = DEPTHS["one_pass"]
    d = _make(nb, n_p, arrangement, variant)
    ubk = d.bk[np.sort(np.unique(d.bk, return_index=True)[1])]
    from oracle.oracle import np_join
    exp = np_join(ubk, ubk, d.pk)
    assert exp == d.full[0]                                             # (N:1: a duplicate adds no match)
    opts("plan_target_keys", target)
    eng = LabEngine("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()
    assert fj.hash_join_count_radix(t(ubk), t(ubk), t(d.pk))[0] == exp
    nbt = int(ubk.size)
    assert eng.bcast_plan(nbt) is not None
    bks = [t(ubk[: nbt // 3]), t(ubk[nbt // 3:])]
    pks = [t(d.pk[: d.pk.size // 2]), t(d.pk[d.pk.size // 2:])]
    sizes = [int(b.numel()) for b in bks]
    rbs = [eng.bcast_region_bytes(nbt, n) for n in sizes]
    offs = [0, rbs[0]]
    base = torch.empty(sum(rbs), dtype=torch.uint8, device="cuda:0")
    bits, nparts, _ = eng.bcast_plan(nbt)
    empty = torch.empty(16, dtype=torch.int64, device="cuda:0")[:0]
    for pieces in (1, 3):
        for r in range(2):
            eng.bcast_pack(bks[r], nbt, base[offs[r]: offs[r] + rbs[r]], pieces)
            assert eng.bcast_pack_bounds(pieces)[-1] == sizes[r]
            eng.bcast_probe(empty, nbt)
            assert eng.bcast_finish() == 0
        total = 0
        for r in range(2):
            eng.bcast_pack(bks[r], nbt, base[offs[r]: offs[r] + rbs[r]], pieces)
            eng.bcast_probe(pks[r], nbt)
            for q in range(pieces):
                eng.bcast_join(base, offs, sizes, nparts * q // pieces, nparts * (q + 1) // pieces)
            total += eng.bcast_finish()
        assert total == exp, (pieces, total, exp)
