"""Group ids for multi-column keys on an MI355X (FJ_ALGO_KEY_PAIR, csrc/fj_groupby_pair.hip; api.factorize_columns / api.encode_keys):
every plan depth, the out-of-band words, pairs crafted to share ONE combined word, a partition beyond the LDS table, the HBM form from
the start, guard words, three columns, the shared dictionary of two relations.  Each case on NumPy arrays and on device tensors.

Reference: np.unique(np.stack(columns, 1), axis=0, return_index=True).  The order of the groups is unspecified, so no id is compared
with NumPy's.  Checked exactly: g; 0 <= codes < g with every id used; c[first_index][codes] == c for every column; first_index equals
NumPy's first indices, aligned through the tuples.  The argument checks and the C-ABI refusals are tests/test_factorize_columns_cpu.py."""
import ctypes
import functools
import threading

import numpy as np
import pytest

import hbm_timings
import keymix
from test_factorize_columns_cpu import GB, INV, PAIR, SALT, pair64

GIP = GB | INV | PAIR
POISON = 0xA5A5A5A5A5A5A5A5
SPECIAL_WORDS = (keymix.EMPTY_RAW, keymix.FILLER_RAW, 0, 2**64 - 1)


@pytest.fixture(scope="module")
def fj():
    import flash_join
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_device_count() >= 1, "no HIP device: the product path must not silently fall back"
    assert flash_join.initialize() is None
    return flash_join


class Rel:
    """a relation of key columns and its reference (the distinct tuples in NumPy's order, their first rows), computed once"""
    def __init__(self, cols):
        self.cols = [np.ascontiguousarray(c, dtype=np.uint64) for c in cols]
        self.n = self.cols[0].size
        assert all(c.shape == (self.n,) for c in self.cols)
        if self.n:
            self.tuples, self.first = np.unique(np.stack(self.cols, 1), axis=0, return_index=True)
        else:
            self.tuples, self.first = np.empty((0, len(self.cols)), np.uint64), np.empty(0, np.int64)
        self.g = int(self.tuples.shape[0])
        self._dev = None

    def arg(self, device):
        if not device:
            return list(self.cols)
        if self._dev is None:
            import torch
            self._dev = [torch.from_numpy(c.view(np.int64)).cuda() for c in self.cols]
        return list(self._dev)


def _host(a, device):
    if device:
        assert a.is_cuda and str(a.dtype) == "torch.int64", a.dtype
        return a.cpu().numpy()
    assert isinstance(a, np.ndarray), type(a)
    return a


def check(rel, what, g, codes, first_index, device=False, raw=False):
    """raw: arrays read back from the C ABI (uint64 words)"""
    assert isinstance(g, int) and g == rel.g, (what, g, rel.g)
    codes, first_index = _host(codes, device), _host(first_index, device)
    if not raw:
        assert codes.dtype == np.int64 and first_index.dtype == np.int64, (what, codes.dtype, first_index.dtype)
    codes, first_index = codes.view(np.int64), first_index.view(np.int64)
    assert codes.shape == (rel.n,) and first_index.shape == (g,), (what, codes.shape, first_index.shape)
    if rel.n == 0:
        return
    assert codes.min() >= 0 and codes.max() < g, (what, int(codes.min()), int(codes.max()), g)
    assert np.unique(codes).size == g, f"{what}: not every id is used"
    assert first_index.min() >= 0 and first_index.max() < rel.n, (what, int(first_index.min()), int(first_index.max()))
    for j, c in enumerate(rel.cols):
        bad = int(np.count_nonzero(c[first_index][codes] != c))
        assert bad == 0, f"{what}: columns[{j}][first_index][codes] != columns[{j}] in {bad} rows"
    got = np.stack([c[first_index] for c in rel.cols], 1)
    o = np.lexsort(tuple(got[:, j] for j in reversed(range(got.shape[1]))))
    assert np.array_equal(got[o], rel.tuples), f"{what}: the tuples at first_index are not the distinct tuples"
    assert np.array_equal(first_index[o], rel.first), f"{what}: a first_index is not the smallest row of its tuple"


def check_timings(lt, what, path, passes, fell_back):
    assert lt["emit_ms"] == 0.0 and lt["join_ms"] == lt["probe_phase_ms"], (what, lt)
    assert lt["path"] == path and lt["fell_back"] == fell_back, (what, lt)
    if path == 1:
        hbm_timings.check_hbm_form(lt, what)
    if passes is not None:
        assert lt["passes"] == passes, (what, lt)


def _grid_rows(rng, n, na, nb_, present=None):
    """n rows over na x nb_ values (64-bit words drawn at random: neither column alone decides a group); present: only that many
    of the pairs occur, every one of them at least once"""
    va = np.unique(rng.integers(0, 2**64, size=na + 8, dtype=np.uint64))[:na]
    vb = np.unique(rng.integers(0, 2**64, size=nb_ + 8, dtype=np.uint64))[:nb_]
    rng.shuffle(va); rng.shuffle(vb)
    pairs = rng.permutation(na * nb_)[:present if present else na * nb_]
    pick = np.concatenate([pairs, rng.choice(pairs, n - pairs.size)]) if n > pairs.size else pairs[:n]
    rng.shuffle(pick)
    return [va[pick // nb_], vb[pick % nb_]]


def _distinct_pairs(rng, n):
    i = np.arange(n, dtype=np.uint64)
    a = (rng.integers(0, 1 << 20, size=n, dtype=np.uint64) << np.uint64(2)) | (i % np.uint64(3))
    b = i // np.uint64(3) + rng.integers(0, 2**63, dtype=np.uint64)    # (every b three times, a may repeat across them: the pairs do not)
    return [a, b]


def _hot_pair(rng):
    single = _distinct_pairs(rng, 100_001)
    a = np.concatenate([np.full(100_000, single[0][-1]), single[0][:100_000]])
    b = np.concatenate([np.full(100_000, single[1][-1]), single[1][:100_000]])
    o = rng.permutation(a.size)                                        # the hot pair's rows are spread through the input
    return [a[o], b[o]]


def _swapped(rng):
    """(x, y), (y, x), (x, x) and (y, y) for 300 value pairs, three copies each: a symmetric combine would merge the first two"""
    x = rng.integers(0, 2**64, size=300, dtype=np.uint64)
    y = rng.integers(0, 2**64, size=300, dtype=np.uint64)
    a, b = np.concatenate([x, y, x, y]), np.concatenate([y, x, x, y])
    o = rng.permutation(np.repeat(np.arange(a.size), 3))
    return [a[o], b[o]]


def _raw_extremes(rng):
    """raw 0 and 2^64 - 1 in either column, beside ordinary words"""
    v = np.array([0, 2**64 - 1, 1, 2**63, 0x1234567890ABCDEF], dtype=np.uint64)
    a, b = np.repeat(v, v.size), np.tile(v, v.size)
    o = rng.permutation(np.repeat(np.arange(a.size), 3))
    return [a[o], b[o]]


def _pairs_on_words(rng, words, per_word):
    """per_word distinct pairs on each combined word: a = w ^ mix(b ^ C) for random b"""
    w = np.repeat(np.array(words, dtype=np.uint64), per_word)
    b = rng.integers(0, 2**64, size=w.size, dtype=np.uint64)
    a = w ^ keymix.mix(b ^ np.uint64(SALT))
    assert np.array_equal(pair64(a, b), w) and np.unique(b).size == b.size
    return a, b


def _among(rng, a, b, copies, background):
    bg = rng.integers(0, 2**64, size=(2, background), dtype=np.uint64)
    a, b = np.concatenate([np.repeat(a, copies), bg[0]]), np.concatenate([np.repeat(b, copies), bg[1]])
    o = rng.permutation(a.size)
    return [a[o], b[o]]


def _special_words(rng, background):
    """one pair on each of the combined words the kernels treat out of band or could confuse with it, three copies each"""
    a, b = _pairs_on_words(rng, SPECIAL_WORDS, 1)
    return _among(rng, a, b, 3, background)


def _collisions(rng, background, word=None):
    """5 distinct pairs on ONE combined word, three copies each"""
    word = int(rng.integers(0, 2**64, dtype=np.uint64)) if word is None else word
    a, b = _pairs_on_words(rng, [word], 5)
    return _among(rng, a, b, 3, background)


def _oversized(rng):
    """9000 distinct combined words whose mixed forms carry the radix digits of ONE final partition of the 5-bit plan that 29 000 rows
    take (partition 19), each once, among 20 000 background rows"""
    low = np.unique(rng.integers(0, 2**59, size=9100, dtype=np.uint64))[:9000]
    words = keymix.unmix((np.uint64(19) << np.uint64(59)) | low)
    assert np.unique(words).size == 9000 and np.all(keymix.hash_w1(words) >> np.uint32(27) == 19)
    b = rng.integers(0, 2**64, size=9000, dtype=np.uint64)
    a = words ^ keymix.mix(b ^ np.uint64(SALT))
    assert np.array_equal(pair64(a, b), words)
    return _among(rng, a, b, 1, 20_000)


CASES = {   # id: (columns builder, plan_target_keys, passes, fell_back)
    "zero_pass": (lambda rng: _grid_rows(rng, 1000, 7, 6, present=37), 4096, 0, 0),
    "single_row": (lambda rng: [np.array([0x1234567890ABCDEF], dtype=np.uint64), np.array([42], dtype=np.uint64)], 4096, 0, 0),
    "all_equal": (lambda rng: [np.full(777, 42, dtype=np.uint64), np.full(777, 2**64 - 7, dtype=np.uint64)], 4096, 0, 0),
    "all_distinct": (lambda rng: _distinct_pairs(rng, 3000), 4096, 0, 0),
    "n4097": (lambda rng: _grid_rows(rng, 4097, 50, 40), 4096, 1, 0),
    "one_pass": (lambda rng: _grid_rows(rng, 200_003, 250, 200), 4096, 1, 0),
    "two_pass": (lambda rng: _grid_rows(rng, 200_003, 250, 200), 16, 2, 0),
    "hot_pair": (_hot_pair, 4096, 1, 0),
    "swapped_and_diagonal": (_swapped, 4096, 0, 0),
    "raw_extremes": (_raw_extremes, 4096, 0, 0),
    "special_words_zero_pass": (lambda rng: _special_words(rng, 500), 4096, 0, 0),
    "special_words_one_pass": (lambda rng: _special_words(rng, 20_000), 4096, 1, 0),
    "collisions_zero_pass": (lambda rng: _collisions(rng, 485), 4096, None, 1),
    "collisions_one_pass": (lambda rng: _collisions(rng, 19_985), 4096, None, 1),
    "collisions_on_the_marker": (lambda rng: _collisions(rng, 19_985, keymix.EMPTY_RAW), 4096, None, 1),
    "oversized_partition": (_oversized, 4096, None, 1),
}
PARITY = [(cid, device) for cid in CASES for device in (False, True)]


@functools.lru_cache(maxsize=None)
def _case(cid):
    return Rel(CASES[cid][0](np.random.default_rng(sorted(CASES).index(cid) + 900)))


def test_the_cases_are_what_they_say():
    """(no GPU) the shapes the GPU tests rely on"""
    assert _case("zero_pass").g == 37 and _case("zero_pass").n == 1000
    assert _case("all_equal").g == 1 and _case("all_distinct").g == 3000
    one = _case("one_pass")
    assert one.n == 200_003 and one.g > 40_000 and np.unique(one.cols[0]).size == 250 and np.unique(one.cols[1]).size == 200
    assert _case("hot_pair").g == 100_001 and _case("hot_pair").n == 200_000
    assert _case("swapped_and_diagonal").g == 1200
    assert _case("raw_extremes").g == 25
    for cid, rows in (("collisions_zero_pass", 500), ("collisions_one_pass", 20_000), ("collisions_on_the_marker", 20_000)):
        rel = _case(cid)
        w, cnt = np.unique(pair64(*rel.cols), return_counts=True)
        assert rel.n == rows and rel.g == rows - 10 and w.size == rows - 14 and cnt.max() == 15, cid      # 5 pairs x 3 copies on one word
    assert np.count_nonzero(pair64(*_case("collisions_on_the_marker").cols) == np.uint64(keymix.EMPTY_RAW)) == 15
    for cid in ("special_words_zero_pass", "special_words_one_pass"):
        w = pair64(*_case(cid).cols)
        assert all(np.count_nonzero(w == np.uint64(s)) == 3 for s in SPECIAL_WORDS), cid
    assert _case("oversized_partition").n == 29_000 and _case("oversized_partition").g == 29_000


@pytest.mark.gpu
@pytest.mark.parametrize("cid,device", PARITY, ids=[f"{c}-{'device' if d else 'numpy'}" for c, d in PARITY])
def test_factorize_columns(fj, cid, device):
    _, target, passes, fell_back = CASES[cid]
    rel = _case(cid)
    fj.set_option("plan_target_keys", target)
    try:
        g, sec, codes, first_index = fj.factorize_columns(rel.arg(device))
        lt = fj.last_timings()
    finally:
        fj.set_option("plan_target_keys", 4096)
    assert isinstance(sec, float)
    check_timings(lt, cid, path=1 if fell_back else 0, passes=0 if fell_back else passes, fell_back=fell_back)
    check(rel, cid, g, codes, first_index, device)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_empty_input(fj, device):
    import torch
    rel = Rel([np.empty(0, np.uint64), np.empty(0, np.uint64)])
    g, sec, codes, first_index = fj.factorize_columns(rel.arg(device))
    assert g == 0 and isinstance(sec, float)
    check(rel, "empty", g, codes, first_index, device)
    if not device:
        return
    # the raw call with nb = 0: g = 0 and not a word of either buffer is written
    from flash_hash_join_amd import _lib, api
    A5 = int(np.array(POISON, dtype=np.uint64).view(np.int64))
    ok = torch.full((64,), A5, dtype=torch.int64, device="cuda")
    ov = torch.full((64,), A5, dtype=torch.int64, device="cuda")
    cnt = ctypes.c_uint64(7)
    with api._ctx_locks.setdefault(0, threading.RLock()):
        _lib.check(_lib.load().fj_join_device(api.context(0), GIP | 2, 0, 1, None, None, 0, None, 0, torch.cuda.current_stream(0).cuda_stream, 64,
                                              ctypes.byref(cnt), ok.data_ptr(), ov.data_ptr(), 64, None))
    assert int(cnt.value) == 0 and bool((ok == A5).all()) and bool((ov == A5).all())


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["one_pass", "special_words_one_pass", "collisions_one_pass", "all_equal", "single_row"])
@pytest.mark.parametrize("option,base", [("scalar_hbm_table", 1), ("radix_threshold", 0)])
def test_hbm_table_form(fj, option, base, cid):
    """FJ_ALGO_SCALAR under scalar_hbm_table = 1 (the raw call) and FJ_ALGO_ADAPTIVE below radix_threshold: the table of row indices
    from the start.  It compares pairs, so pairs on one combined word are groups like any other and nothing falls back"""
    from flash_hash_join_amd import api
    rel = _case(cid)
    fj.set_option(option, 1 if base else rel.n + 1)
    try:
        for device in (False, True):
            if base:
                a, b = rel.arg(device)
                g, sec, first_index, codes = api._group_by(a, b, base | api.ALGO_INVERSE | api.ALGO_KEY_PAIR)
                first_index = api._first_rows(first_index)
            else:
                g, sec, codes, first_index = fj.factorize_columns(rel.arg(device))
            check_timings(fj.last_timings(), cid, path=1, passes=0, fell_back=0)
            check(rel, cid, g, codes, first_index, device)
    finally:
        fj.set_option(option, 0)


def _raw_device_call(L, api, algo, a, b, nb, ok, ov, cap):
    import torch
    from flash_hash_join_amd import _lib
    cnt = ctypes.c_uint64(0)
    t = _lib.FjTimings()
    with api._ctx_locks.setdefault(0, threading.RLock()):
        _lib.check(L.fj_join_device(api.context(0), algo, 0, 1, a.data_ptr(), b.data_ptr(), nb, None, 0, torch.cuda.current_stream(0).cuda_stream, 64,
                                    ctypes.byref(cnt), ok.data_ptr(), ov.data_ptr(), cap, ctypes.byref(t)))
    return int(cnt.value), t


@pytest.mark.gpu
@pytest.mark.parametrize("base", [2, 1], ids=["partitioned", "hbm_table"])
@pytest.mark.parametrize("extra", [0, 1000], ids=["capacity_nb", "capacity_nb_plus_1000"])
def test_guard_words_and_full_definition(fj, base, extra):
    """fj_join_device on poisoned buffers of out_capacity + 64 words: all nb ids are defined by the call alone (no poison survives
    below nb), no id at or beyond nb is written, and the 64 words behind out_capacity are intact in both buffers"""
    import torch
    from flash_hash_join_amd import _lib, api
    L = _lib.load()
    rel = _case("one_pass")
    (a, b), nb = rel.arg(True), rel.n
    cap = nb + extra
    A5 = int(np.array(POISON, dtype=np.uint64).view(np.int64))
    if base == 1:
        fj.set_option("scalar_hbm_table", 1)
    try:
        ok = torch.full((cap + 64,), A5, dtype=torch.int64, device="cuda")
        ov = torch.full((cap + 64,), A5, dtype=torch.int64, device="cuda")
        g, t = _raw_device_call(L, api, base | GIP, a, b, nb, ok, ov, cap)
    finally:
        fj.set_option("scalar_hbm_table", 0)
    assert t.path == (0 if base == 2 else 1) and t.emit_ms == 0.0 and t.fell_back == 0 and t.join_ms == t.probe_phase_ms
    hk, hv = ok.cpu().numpy(), ov.cpu().numpy()
    assert np.all(hk[cap:] == A5) and np.all(hv[cap:] == A5), "a word at or beyond out_capacity was written"
    assert np.all(hv[nb:cap] == A5), "an id beyond the relation's rows was written"
    assert not np.any(hv[:nb] == A5), "an id below nb was left undefined"
    check(rel, "guard words", g, hv[:nb], hk[:g], raw=True)


@functools.lru_cache(maxsize=1)
def _three_columns():
    rng = np.random.default_rng(31)
    v = [rng.integers(0, 2**64, size=30, dtype=np.uint64) for _ in range(3)]
    return Rel([v[j][rng.integers(0, 30, size=20_011)] for j in range(3)])


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_three_columns_fold_left_to_right(fj, device):
    rel = _three_columns()
    assert rel.n == 20_011 and 10_000 < rel.g <= 27_000
    g, sec, codes, first_index = fj.factorize_columns(rel.arg(device))
    assert isinstance(sec, float) and sec > 0
    check(rel, "three columns", g, codes, first_index, device)
    g2, _, codes2, first2 = fj.factorize_columns(tuple(rel.arg(device)[:2]))      # a tuple of two: one call
    check(Rel(rel.cols[:2]), "two of three", g2, codes2, first2, device)


@functools.lru_cache(maxsize=1)
def _two_relations():
    """5000 distinct build pairs with values; 20 000 probe rows, half of them build pairs (with repeats), half pairs of their own"""
    rng = np.random.default_rng(5)
    pool = _grid_rows(rng, 15_000, 150, 100, present=15_000)           # 15 000 distinct pairs over 150 x 100 values
    assert np.unique(np.stack(pool, 1), axis=0).shape[0] == 15_000
    build = [c[:5000] for c in pool]
    values = rng.integers(0, 2**63, size=5000, dtype=np.uint64)
    hit = rng.integers(0, 5000, size=10_000)
    miss = rng.integers(5000, 15_000, size=10_000)
    match = np.concatenate([hit, np.full(10_000, -1)])
    probe = [np.concatenate([c[hit], c[miss]]) for c in pool]
    o = rng.permutation(20_000)
    return build, values, [c[o] for c in probe], match[o]


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_encode_keys_feeds_the_joins(fj, device):
    import torch
    build, values, probe, match = _two_relations()
    to = (lambda c: torch.from_numpy(c.view(np.int64)).cuda()) if device else (lambda c: c)
    g, sec, bc, pc = fj.encode_keys([to(c) for c in build], tuple(to(c) for c in probe))
    assert isinstance(g, int) and isinstance(sec, float)
    both = Rel([np.concatenate([x, y]) for x, y in zip(build, probe)])
    assert g == both.g and 5000 < g <= 15_000
    hb, hp = _host(bc, device), _host(pc, device)
    assert hb.dtype == np.int64 and hp.dtype == np.int64 and hb.shape == (5000,) and hp.shape == (20_000,)
    codes = np.concatenate([hb, hp])
    assert codes.min() >= 0 and codes.max() < g and np.unique(codes).size == g
    ref_inv = np.unique(np.stack(both.cols, 1), axis=0, return_inverse=True)[1].reshape(-1)
    assert np.unique(np.stack([codes, ref_inv], 1), axis=0).shape[0] == g, "equal tuples and equal codes are not the same thing"
    # the codes are ordinary keys: a join on them is the join on the tuples
    out = fj.inner_join(bc, to(values), pc, return_arrays=True)
    rows = np.flatnonzero(match >= 0)
    want_k, want_v = fj.sort_pairs(hp[rows].view(np.uint64), values[match[rows]])
    got_k, got_v = fj.sort_pairs(_host(out[-2], device), _host(out[-1], device))
    assert out[0] == rows.size == 10_000
    assert np.array_equal(got_k.view(np.uint64), want_k) and np.array_equal(got_v.view(np.uint64), want_v)
    m, _, idx = fj.lookup_indices(bc, pc)
    assert m == 10_000 and np.array_equal(_host(idx, device), match), "lookup_indices on the codes names other build rows"
    # a single array per side is a one-column key
    g1, _, b1, p1 = fj.encode_keys(to(build[0]), to(probe[0]))
    col = np.concatenate([build[0], probe[0]])
    c1 = np.concatenate([_host(b1, device), _host(p1, device)])
    assert g1 == np.unique(col).size and np.unique(np.stack([c1.view(np.uint64), col], 1), axis=0).shape[0] == g1


@pytest.mark.gpu
def test_the_same_context_reused(fj):
    """factorize_columns, a factorize, a group_by_sum and a factorize_columns of another size on one context: all correct, and no
    result is left pending"""
    import torch
    from flash_hash_join_amd import _lib, api
    from test_factorize import Rel as Rel1, check_ids
    L = _lib.load()
    a, b, c = _case("one_pass"), _case("n4097"), _case("special_words_one_pass")
    g, _, codes, first_index = fj.factorize_columns(a.arg(True))
    check(a, "first factorize_columns", g, codes, first_index, True)
    one = Rel1(b.cols[0])
    vals = np.arange(1, b.n + 1, dtype=np.int64)
    with api._ctx_locks.setdefault(0, threading.RLock()):
        g1, _, codes1, uniques1 = fj.factorize(one.arg(True))
        gs, _, gk, sums = fj.group_by_sum(one.arg(True), torch.from_numpy(vals).cuda())
        g, _, codes, first_index = fj.factorize_columns(c.arg(True))
        out = torch.empty(c.n, dtype=torch.int64, device="cuda")
        assert L.fj_emit_pairs(api.context(0), out.data_ptr(), out.data_ptr(), c.n, torch.cuda.current_stream(0).cuda_stream, None) != 0, "a result was left pending"
        assert "no counted materialising join is pending" in _lib.last_error()
    check(c, "second factorize_columns", g, codes, first_index, True)
    check_ids(one, "factorize in between", g1, uniques1, codes1, True)
    uk, inv = np.unique(one.keys, return_inverse=True)
    want = np.zeros(uk.size, np.int64)
    np.add.at(want, inv.reshape(-1), vals)
    gk = gk.cpu().numpy().view(np.uint64)
    assert gs == one.g and np.array_equal(sums.cpu().numpy()[np.argsort(gk)], want), "group_by_sum between two factorize_columns calls"
    # the codes do what they are for: an aggregate per PAIR through the single-key entry
    g, _, codes, first_index = fj.factorize_columns(b.arg(True))
    gs, _, gk, sums = fj.group_by_sum(codes, torch.from_numpy(vals).cuda())
    want = np.zeros(g, np.int64)
    np.add.at(want, codes.cpu().numpy(), vals)
    assert gs == g and np.array_equal(sums.cpu().numpy()[np.argsort(gk.cpu().numpy())], want)
