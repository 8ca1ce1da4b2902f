"""The rows of every group on an MI355X (FJ_ALGO_GROUP_BY | FJ_ALGO_GROUP_ROWS, csrc/fj_groupby_rows.hip; api.group_rows /
api.group_by_collect): the distinct keys, the relation's row indices in group-contiguous order and the offsets of the groups - a CSR of
row indices.  What needs no GPU is tests/test_group_rows_cpu.py.

Reference: NumPy on the inputs, no tolerance.  The order of the groups and of the rows inside a group is unspecified, so nothing is
compared with an argsort of NumPy's.  A result is correct iff, exactly and for every row: group_keys are g = np.unique(keys).size
distinct keys; offsets[0] == 0, offsets[g] == n and np.diff(offsets) >= 1; np.sort(row_index) == arange(n); and
keys[row_index] == np.repeat(group_keys, np.diff(offsets))."""
import ctypes
import functools
import threading

import numpy as np
import pytest

import hbm_timings
import keymix

GB, ROWS = 0x40000, 0x40000000
GR = GB | ROWS
TS = 8192                                                             # slots of the LDS table (csrc/fj_group_dev.h)


@pytest.fixture(scope="module")
def fj():
    import flash_join
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_device_count() >= 1, "no HIP device: the product path must not silently fall back"
    assert flash_join.initialize() is None
    return flash_join


class Rel:
    """a relation and its reference (the number of distinct keys), computed once"""
    def __init__(self, keys):
        self.keys = np.ascontiguousarray(keys, dtype=np.uint64)
        self.n = self.keys.size
        self.g = int(np.unique(self.keys).size)
        self._dev = None

    def arg(self, device):
        if not device:
            return self.keys
        if self._dev is None:
            import torch
            self._dev = torch.from_numpy(self.keys.view(np.int64)).cuda()
        return self._dev


def _host(a, device):
    if device:
        assert a.is_cuda and str(a.dtype) == "torch.int64", a.dtype
        return a.cpu().numpy()
    assert isinstance(a, np.ndarray), type(a)
    return a


def check_csr(rel, what, g, group_keys, offsets, row_index, device=False, raw=False):
    """the four conditions of the module's docstring, every row.  raw: arrays read back from the C ABI (uint64 words)"""
    assert isinstance(g, int) and g == rel.g, (what, g, rel.g)
    gk, off, rows = _host(group_keys, device), _host(offsets, device), _host(row_index, device)
    if not raw:
        assert off.dtype == np.int64 and rows.dtype == np.int64 and gk.dtype == (np.int64 if device else np.uint64), (what, gk.dtype, off.dtype, rows.dtype)
    gk, off, rows = gk.view(np.uint64), off.view(np.int64), rows.view(np.int64)
    assert gk.shape == (g,) and off.shape == (g + 1,) and rows.shape == (rel.n,), (what, gk.shape, off.shape, rows.shape)
    assert np.unique(gk).size == g, f"{what}: the returned keys are not distinct"
    assert off[0] == 0 and off[g] == rel.n, (what, int(off[0]), int(off[g]), rel.n)
    sizes = np.diff(off)
    assert np.all(sizes >= 1), f"{what}: {int(np.count_nonzero(sizes < 1))} groups without a row (or starts out of order)"
    assert np.array_equal(np.sort(rows), np.arange(rel.n)), f"{what}: row_index is no permutation of the rows"
    want = np.repeat(gk, sizes)
    assert np.array_equal(rel.keys[rows], want), f"{what}: keys[row_index] != repeat(group_keys, sizes) in {int(np.count_nonzero(rel.keys[rows] != want))} rows"
    return gk, off, rows


def check_timings(lt, what, path, passes, fell_back):
    assert lt["emit_ms"] == 0.0 and lt["join_ms"] == lt["probe_phase_ms"], (what, lt)
    assert lt["path"] == path and lt["fell_back"] == fell_back, (what, lt)
    if path == 1:
        hbm_timings.check_hbm_form(lt, what)
    if passes is not None:
        assert lt["passes"] == passes, (what, lt)


def _dup_keys(rng, n, distinct):
    pool = np.unique(rng.integers(0, 2**64, size=distinct + 64, dtype=np.uint64))[:distinct]
    rng.shuffle(pool)
    keys = np.concatenate([pool, rng.choice(pool, n - distinct)]) if n > distinct else pool[:n].copy()
    rng.shuffle(keys)
    return keys


def _hot_keys(rng):
    single = np.unique(rng.integers(0, 2**64, size=100_100, dtype=np.uint64))[:100_001]
    keys = np.concatenate([np.full(100_000, single[-1]), single[:100_000]])
    rng.shuffle(keys)                                                  # the hot key's rows are spread through the input
    return keys


def _special_keys(rng, background, bits):
    """the hash domain's special keys (tests/keymix.py: the marker, the wide kernel's filler and their neighbours, raw 0 and raw
    2^64 - 1), three copies each, among `background` random rows"""
    _, raw = keymix.special_raw_keys(bits)
    keys = np.concatenate([np.repeat(raw, 3), rng.integers(0, 2**64, size=background, dtype=np.uint64)])
    rng.shuffle(keys)
    return keys


def _wrapping_chain(rng, bits, partition, background):
    """300 keys whose home slot is ONE slot two below the table's end - the probe chain of all but two of them wraps to slot 0 - with
    1 to 5 copies each, among `background` random rows"""
    crafted = keymix.craft(bits, partition, TS - 2, 300, seed=11)
    assert np.unique(crafted).size == 300 and np.all((keymix.mix(crafted) & np.uint64(TS - 1)) == TS - 2)
    if bits:
        assert np.all(keymix.partition_of(crafted, bits) == partition)
    keys = np.concatenate([np.repeat(crafted, 1 + np.arange(300) % 5), rng.integers(0, 2**64, size=background, dtype=np.uint64)])
    rng.shuffle(keys)
    return keys


CASES = {   # id: (keys builder, plan_target_keys, passes)
    "zero_pass": (lambda rng: _dup_keys(rng, 1000, 37), 4096, 0),
    "single_row": (lambda rng: np.array([0x1234567890ABCDEF], dtype=np.uint64), 4096, 0),
    "all_distinct_zero_pass": (lambda rng: _dup_keys(rng, 3000, 3000), 4096, 0),
    "all_equal_zero_pass": (lambda rng: np.full(777, 42, dtype=np.uint64), 4096, 0),
    "n4097": (lambda rng: _dup_keys(rng, 4097, 1500), 4096, 1),
    "one_pass": (lambda rng: _dup_keys(rng, 200_003, 50_000), 4096, 1),
    "all_distinct": (lambda rng: _dup_keys(rng, 20_011, 20_011), 4096, 1),
    "all_equal": (lambda rng: np.full(100_003, 0xDEADBEEF12345678, dtype=np.uint64), 4096, 1),      # one slot's cursor takes every row
    "two_pass_10_bits": (lambda rng: _dup_keys(rng, 200_003, 50_000), 256, 2),
    "two_pass_14_bits": (lambda rng: _dup_keys(rng, 200_003, 50_000), 16, 2),                       # many nearly empty partitions
    "hot_key": (_hot_keys, 4096, 1),
    "special_keys_zero_pass": (lambda rng: _special_keys(rng, 500, 0), 4096, 0),
    "special_keys_one_pass": (lambda rng: _special_keys(rng, 20_000, 5), 4096, 1),
    "wrapping_chain_zero_pass": (lambda rng: _wrapping_chain(rng, 0, 0, 0), 4096, 0),
    "wrapping_chain_one_pass": (lambda rng: _wrapping_chain(rng, 5, 29, 20_000), 4096, 1),        # (20 900 rows take a 5-bit plan: one partition holds the chain)
}
PARITY = [(cid, device) for cid in CASES for device in (False, True)]


@functools.lru_cache(maxsize=None)
def _case(cid):
    return Rel(CASES[cid][0](np.random.default_rng(sorted(CASES).index(cid) + 900)))


def check_special_keys(rel, what, gk, off, rows, marker, last_in_partition_bits=None):
    """every special key is a group of exactly its three rows (raw 0: six where it is also the raw key of the mixed word 0); the
    out-of-band key's group owns its three rows too, and on the partitioned plan it is the LAST group of its partition"""
    for k in (keymix.EMPTY_RAW, keymix.FILLER_RAW, 0, 2**64 - 1, marker):
        r = np.flatnonzero(gk == np.uint64(k))
        assert r.size == 1, (what, hex(k))
        mine = np.sort(rows[off[r[0]]:off[r[0] + 1]])
        assert np.array_equal(mine, np.flatnonzero(rel.keys == np.uint64(k))) and mine.size in (3, 6), (what, hex(k), mine)
    if last_in_partition_bits is not None:
        part = keymix.partition_of(gk, last_in_partition_bits)
        r = int(np.flatnonzero(gk == np.uint64(marker))[0])
        assert r == np.flatnonzero(part == part[r]).max(), f"{what}: the marker key's group is not the last of its partition"
        assert np.all(np.diff(np.flatnonzero(part == part[r])) == 1), f"{what}: a partition's groups are not contiguous"


@pytest.mark.gpu
@pytest.mark.parametrize("cid,device", PARITY, ids=[f"{c}-{'device' if d else 'numpy'}" for c, d in PARITY])
def test_group_rows_on_the_partitioned_plan(fj, cid, device):
    _, target, passes = CASES[cid]
    rel = _case(cid)
    if cid == "hot_key":
        assert rel.g == 100_001 and rel.n == 200_000
    if cid.startswith("all_distinct"):
        assert rel.g == rel.n
    if cid.startswith("all_equal"):
        assert rel.g == 1
    fj.set_option("plan_target_keys", target)
    try:
        g, sec, gk, off, rows = fj.group_rows(rel.arg(device))
        lt = fj.last_timings()
    finally:
        fj.set_option("plan_target_keys", 4096)
    assert isinstance(sec, float)
    check_timings(lt, cid, path=0, passes=passes, fell_back=0)
    gk, off, rows = check_csr(rel, cid, g, gk, off, rows, device)
    if cid.startswith("special_keys"):
        check_special_keys(rel, cid, gk, off, rows, keymix.EMPTY_RAW, lt["radix_bits"])


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_empty_input(fj, device):
    import torch
    rel = Rel(np.empty(0, np.uint64))
    g, sec, gk, off, rows = fj.group_rows(rel.arg(device))
    assert g == 0 and isinstance(sec, float)
    check_csr(rel, "empty", g, gk, off, rows, device)
    assert _host(off, device).tolist() == [0]
    vals = np.empty((0, 3), np.float32)
    out = fj.group_by_collect(rel.arg(device), torch.from_numpy(vals).cuda() if device else vals)
    assert out[0] == 0 and tuple(out[4].shape) == (0, 3)
    if not device:
        return
    # the raw call with nb = 0: g = 0 and not a word of either buffer is written
    from flash_hash_join_amd import _lib, api
    A5 = int(np.array(0xA5A5A5A5A5A5A5A5, dtype=np.uint64).view(np.int64))
    ok = torch.full((64,), A5, dtype=torch.int64, device="cuda")
    ov = torch.full((128,), A5, dtype=torch.int64, device="cuda")
    cnt = ctypes.c_uint64(7)
    with api._ctx_locks.setdefault(0, threading.RLock()):
        _lib.check(_lib.load().fj_join_device(api.context(0), GR | 2, 0, 1, None, None, 0, None, 0, torch.cuda.current_stream(0).cuda_stream, 64,
                                              ctypes.byref(cnt), ok.data_ptr(), ov.data_ptr(), 64, None))
    assert int(cnt.value) == 0 and bool((ok == A5).all()) and bool((ov == A5).all())


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["one_pass", "special_keys_one_pass", "all_equal", "single_row"])
@pytest.mark.parametrize("option,base", [("scalar_hbm_table", 1), ("radix_threshold", 0)])
def test_hbm_table_form(fj, option, base, cid):
    """FJ_ALGO_SCALAR under scalar_hbm_table = 1 and FJ_ALGO_ADAPTIVE below radix_threshold: the global table from the start.  There
    the out-of-band key is raw 2^64 - 1; the special-key case holds it three times beside the LDS tables' marker"""
    import torch
    from flash_hash_join_amd import _lib, api
    rel = _case(cid)
    fj.set_option(option, 1 if base else rel.n + 1)
    try:
        for device in (False, True):
            if base:
                g, gk, off, rows, t = _c_abi_call(api, _lib, base | GR, rel, device)
                assert t.path == 1 and t.passes == 0 and t.fell_back == 0 and t.emit_ms == 0.0 and t.join_ms == t.probe_phase_ms, cid
                gk, off, rows = check_csr(rel, cid, g, gk, off, rows, raw=True)
            else:
                g, sec, gk, off, rows = fj.group_rows(rel.arg(device))
                check_timings(fj.last_timings(), cid, path=1, passes=0, fell_back=0)
                gk, off, rows = check_csr(rel, cid, g, gk, off, rows, device)
            if cid.startswith("special_keys"):
                check_special_keys(rel, cid, gk, off, rows, 2**64 - 1)
    finally:
        fj.set_option(option, 0)


def _c_abi_call(api, _lib, algo, rel, device):
    """the C ABI with a base of the caller's choice (api.group_rows asks for FJ_ALGO_ADAPTIVE): fj_join_device on device tensors, else
    fj_join_host; (g, keys, offsets with n appended, rows, the call's fj_timings) - the arrays as NumPy words"""
    import torch
    L = _lib.load()
    cnt = ctypes.c_uint64(0)
    t = _lib.FjTimings()
    n = rel.n
    if device:
        ok = torch.empty(n, dtype=torch.int64, device="cuda")
        ov = torch.empty(2 * n, dtype=torch.int64, device="cuda")
        with api._ctx_locks.setdefault(0, threading.RLock()):
            _lib.check(L.fj_join_device(api.context(0), algo, 0, 1, rel.arg(True).data_ptr(), None, n, None, 0, torch.cuda.current_stream(0).cuda_stream, 64,
                                        ctypes.byref(cnt), ok.data_ptr(), ov.data_ptr(), n, ctypes.byref(t)))
        g = int(cnt.value)
        hk, hv = ok.cpu().numpy(), ov.cpu().numpy()
        return g, hk[:g], np.append(hv[n:n + g], n), hv[:n], t
    sec = ctypes.c_double(0)
    ok, ov = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(L.fj_join_host(algo, 0, 1, rel.keys.ctypes.data, None, n, None, 0, ctypes.byref(cnt), ctypes.byref(sec), ctypes.byref(ok), ctypes.byref(ov)))
    try:
        g = int(cnt.value)
        L.fj_last_timings(ctypes.byref(t))
        take = lambda p, rows: np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint64)), shape=(rows,)).copy()
        words = take(ov, n + g).view(np.int64)
        return g, take(ok, g), np.append(words[n:], n), words[:n], t
    finally:
        L.fj_free_host(ok)
        L.fj_free_host(ov)


@functools.lru_cache(maxsize=1)
def _oversized_case():
    """9000 distinct keys whose mixed words carry the radix digits of ONE final partition of the 5-bit plan that 38 000 rows take
    (partition 19: the top five bits of hash word 1), each twice, among 20 000 background rows"""
    rng = np.random.default_rng(78)
    low = np.unique(rng.integers(0, 2**59, size=9100, dtype=np.uint64))[:9000]
    one = keymix.unmix((np.uint64(19) << np.uint64(59)) | low)
    assert np.unique(one).size == 9000 and np.all(keymix.hash_w1(one) >> np.uint32(27) == 19)
    keys = np.concatenate([one, one, rng.integers(0, 2**64, size=20_000, dtype=np.uint64)])
    rng.shuffle(keys)
    return Rel(keys)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_a_partition_beyond_the_lds_table_falls_back_to_the_hbm_table(fj, device):
    """more distinct keys in one partition than the 8192-slot table takes: the count kernel sees it, the place kernel writes nothing,
    and the re-run on the HBM table defines all n + g words"""
    rel = _oversized_case()
    assert rel.n == 38_000
    g, sec, gk, off, rows = fj.group_rows(rel.arg(device))
    check_timings(fj.last_timings(), "fallback", path=1, passes=None, fell_back=1)
    check_csr(rel, "fallback", g, gk, off, rows, device)


POISON = 0xA5A5A5A5A5A5A5A5


@pytest.mark.gpu
@pytest.mark.parametrize("base", [2, 1], ids=["partitioned", "hbm_table"])
@pytest.mark.parametrize("extra", [0, 1000], ids=["capacity_nb", "capacity_nb_plus_1000"])
def test_guard_words_and_full_definition(fj, base, extra):
    """fj_join_device on poisoned buffers, d_build_vals NULL: d_out_keys of out_capacity + 64 words, d_out_vals of 2 * out_capacity + 64.
    No poison survives in the rows [0, nb) or the starts [0, g); the rows [nb, out_capacity) are untouched; the 64 guard words behind
    2 * out_capacity and behind out_capacity of d_out_keys are intact"""
    import torch
    from flash_hash_join_amd import _lib, api
    L = _lib.load()
    rel = _case("one_pass")
    keys, nb = rel.arg(True), rel.n
    cap = nb + extra
    A5 = int(np.array(POISON, dtype=np.uint64).view(np.int64))
    if base == 1:
        fj.set_option("scalar_hbm_table", 1)
    try:
        ok = torch.full((cap + 64,), A5, dtype=torch.int64, device="cuda")
        ov = torch.full((2 * cap + 64,), A5, dtype=torch.int64, device="cuda")
        cnt = ctypes.c_uint64(0)
        t = _lib.FjTimings()
        with api._ctx_locks.setdefault(0, threading.RLock()):
            _lib.check(L.fj_join_device(api.context(0), base | GR, 0, 1, keys.data_ptr(), None, nb, None, 0, torch.cuda.current_stream(0).cuda_stream, 64,
                                        ctypes.byref(cnt), ok.data_ptr(), ov.data_ptr(), cap, ctypes.byref(t)))
        g = int(cnt.value)
    finally:
        fj.set_option("scalar_hbm_table", 0)
    assert t.path == (0 if base == 2 else 1) and t.emit_ms == 0.0 and t.fell_back == 0 and t.join_ms == t.probe_phase_ms
    hk, hv = ok.cpu().numpy(), ov.cpu().numpy()
    assert np.all(hk[cap:] == A5), "a word at or beyond out_capacity of d_out_keys was written"
    assert np.all(hv[2 * cap:] == A5), "a word at or beyond 2 * out_capacity of d_out_vals was written"
    assert np.all(hv[nb:cap] == A5), "a row word at or beyond nb was written"
    assert not np.any(hv[:nb] == A5), "a row word below nb was left undefined"
    assert not np.any(hv[cap:cap + g] == A5), "a start below g was left undefined"
    assert not np.any(hk[:g] == A5), "a key below g was left undefined"
    check_csr(rel, "guard words", g, hk[:g], np.append(hv[cap:cap + g], nb), hv[:nb], raw=True)


@pytest.mark.gpu
def test_the_same_context_reused(fj):
    """group_rows, a factorize, a group_rows of another size on one context: all correct, the context survives, nothing is left pending"""
    import torch
    from flash_hash_join_amd import _lib, api
    L = _lib.load()
    a, b, c = _case("one_pass"), _case("n4097"), _case("all_distinct")
    g, _, gk, off, rows = fj.group_rows(a.arg(True))
    check_csr(a, "first group_rows", g, gk, off, rows, True)
    with api._ctx_locks.setdefault(0, threading.RLock()):
        gf, _, codes, uniques = fj.factorize(b.arg(True))
        g, _, gk, off, rows = fj.group_rows(c.arg(True))
        out = torch.empty(c.n, dtype=torch.int64, device="cuda")
        assert L.fj_emit_pairs(api.context(0), out.data_ptr(), out.data_ptr(), c.n, torch.cuda.current_stream(0).cuda_stream, None) != 0, "a result was left pending"
        assert "no counted materialising join is pending" in _lib.last_error()
    check_csr(c, "second group_rows", g, gk, off, rows, True)
    uniques, codes = uniques.cpu().numpy().view(np.uint64), codes.cpu().numpy()
    assert gf == b.g and np.array_equal(uniques[codes], b.keys), "factorize between two group_rows calls"
    # the CSR does what it is for: a median per group from ONE grouping, against NumPy's
    vals = np.random.default_rng(5).integers(-1000, 1000, size=b.n).astype(np.int64)
    g, _, gk, off, rows = fj.group_rows(b.arg(True))
    gk, off, rows = check_csr(b, "third group_rows", g, gk, off, rows, True)
    got = np.array([np.median(vals[rows[off[i]:off[i + 1]]]) for i in range(g)])
    want = np.array([np.median(vals[b.keys == k]) for k in gk])
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_inputs_from_a_side_stream_and_outputs_consumed_right_after(fj):
    """the keys are produced on a non-default stream right before the call - behind work that keeps the stream busy - and the outputs
    feed a torch gather right after it, all on that stream: the call runs in stream order and its outputs are ordinary tensors there"""
    import torch
    rel = _case("one_pass")
    base = rel.arg(True)
    side = torch.cuda.Stream()
    big = torch.zeros(1 << 26, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(8):
            big.add_(1)                                                # the stream is busy when the keys are made
        keys = base ^ big[:rel.n].to(torch.int64).sub_(8)              # == base only once the eight adds have run
        g, sec, gk, off, rows = fj.group_rows(keys)
        gathered = keys[rows]                                          # consumed at once, on the same stream
        sizes = off[1:] - off[:-1]
        want = torch.repeat_interleave(gk, sizes)
        same = bool((gathered == want).all())
    side.synchronize()
    assert same, "keys[row_index] != repeat(group_keys, sizes) on the side stream"
    check_csr(rel, "side stream", g, gk, off, rows, True)


@pytest.mark.gpu
def test_host_entry_returns_g_keys_and_nb_plus_g_words_and_drops_a_null_output(fj):
    """fj_join_host on NumPy arrays: *out_keys has exactly g keys, *out_vals exactly nb + g words - the row indices, then the starts;
    NULL for either pointer drops that output"""
    from flash_hash_join_amd import _lib
    L = _lib.load()
    rel = _case("one_pass")
    k = rel.keys
    take = lambda p, rows: np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint64)), shape=(rows,)).copy()
    for want_keys, want_rows in ((True, True), (True, False), (False, True), (False, False)):
        cnt, sec = ctypes.c_uint64(0), ctypes.c_double(0)
        ok, ov = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(L.fj_join_host(GR | 2, 0, 1, k.ctypes.data, None, k.size, None, 0, ctypes.byref(cnt), ctypes.byref(sec),
                                  ctypes.byref(ok) if want_keys else None, ctypes.byref(ov) if want_rows else None))
        try:
            g = int(cnt.value)
            assert g == rel.g and bool(ok.value) == want_keys and bool(ov.value) == want_rows
            t = _lib.FjTimings()
            L.fj_last_timings(ctypes.byref(t))
            assert t.emit_ms == 0.0 and t.path == 0 and t.fell_back == 0 and t.passes == 1 and t.join_ms == t.probe_phase_ms
            if want_keys and want_rows:
                words = take(ov, rel.n + g).view(np.int64)
                check_csr(rel, "host both", g, take(ok, g), np.append(words[rel.n:], rel.n), words[:rel.n], raw=True)
            elif want_keys:
                assert np.array_equal(np.sort(take(ok, g)), np.unique(k)), "host keys alone"
            elif want_rows:
                words = take(ov, rel.n + g).view(np.int64)              # (no keys to compare with: every range holds ONE key, and no two ranges the same)
                rows, off = words[:rel.n], np.append(words[rel.n:], rel.n)
                assert off[0] == 0 and np.all(np.diff(off) >= 1) and np.array_equal(np.sort(rows), np.arange(rel.n))
                first = k[rows[off[:-1]]]
                assert np.array_equal(k[rows], np.repeat(first, np.diff(off))) and np.unique(first).size == g
        finally:
            L.fj_free_host(ok)
            L.fj_free_host(ov)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("shape", ["1d", "2d"])
def test_group_by_collect(fj, shape, device):
    """values[row_index] of a checked row_index: the values keep their dtype and trailing dimensions, and every range of the result
    holds exactly the values of its group's rows"""
    import torch
    rel = _case("n4097")
    rng = np.random.default_rng(6)
    vals = rng.standard_normal(rel.n).astype(np.float32) if shape == "1d" else rng.integers(-2**15, 2**15, size=(rel.n, 3)).astype(np.int16)
    g, sec, gk, off, got = fj.group_by_collect(rel.arg(device), torch.from_numpy(vals).cuda() if device else vals)
    assert isinstance(sec, float)
    if device:
        assert got.is_cuda and got.dtype == (torch.float32 if shape == "1d" else torch.int16)
        got = got.cpu().numpy()
    assert got.dtype == vals.dtype and got.shape == vals.shape
    # the row order inside a group is unspecified: compare through a row_index of the same call's grouping - the values are distinct
    # enough to identify their rows (1-D), and otherwise per group as sorted sets of rows
    gk_h, off_h = _host(gk, device).view(np.uint64), _host(off, device)
    assert off_h[0] == 0 and off_h[g] == rel.n and np.all(np.diff(off_h) >= 1) and np.unique(gk_h).size == g == rel.g
    order = np.argsort(rel.keys, kind="stable")
    uk, first = np.unique(rel.keys[order], return_index=True)
    bounds = np.append(first, rel.n)
    for i in range(g):
        j = int(np.searchsorted(uk, gk_h[i]))
        want = vals[order[bounds[j]:bounds[j + 1]]]
        mine = got[off_h[i]:off_h[i + 1]]
        assert mine.shape == want.shape, (i, mine.shape, want.shape)
        key = (lambda a: np.sort(a)) if shape == "1d" else (lambda a: a[np.lexsort(a.T[::-1])])
        assert np.array_equal(key(mine), key(want)), f"group {i}: the collected values are not its rows' values"
    # and against the gather of a checked row_index of another call
    g2, _, gk2, off2, rows2 = fj.group_rows(rel.arg(device))
    gk2, off2, rows2 = check_csr(rel, "collect", g2, gk2, off2, rows2, device)
    mine = {int(gk_h[i]): np.sort(got[off_h[i]:off_h[i + 1]].reshape(off_h[i + 1] - off_h[i], -1), axis=0) for i in range(g)}
    for i in range(g2):
        want = np.sort(vals[rows2[off2[i]:off2[i + 1]]].reshape(off2[i + 1] - off2[i], -1), axis=0)
        assert np.array_equal(mine[int(gk2[i])], want)
