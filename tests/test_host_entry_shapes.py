"""The nine result shapes of the host-buffer entry (fj_join_host, csrc/fj_hostentry.hip) against the device entry on the same inputs:
fj_join_device into buffers of the capacity the host entry uses, plus fj_emit_pairs where the form counts first.  Count word(s) and
every returned word are compared bit for bit - rows sorted first where their order is unspecified, groups sorted by their key - and the
counts against NumPy.  Sizes: an empty build side, an empty probe side, one row, 300 rows over about 40 keys (more than one 256-row
chunk and g < nb: the stride-capacity planes are cut to stride g), 300 distinct rows (g == nb)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MANY, LEFT, ANTI, ROW_IDS, FULL, ALL, PO, BO = 0x10, 0x20, 0x40, 0x80, 0x100, 0x200, 0x800, 0x1000
MIN, MAX, SIGNED, GB, INV, AALL, AARG, AMERGE, PAIR, ROWS = 0x4000, 0x8000, 0x10000, 0x40000, 0x100000, 0x4000000, 0x8000000, 0x10000000, 0x20000000, 0x40000000
GOLDEN = np.uint64(0x9E3779B97F4A7C15)

SIZES = {   # id: (nb, distinct build keys, np)
    "empty_build": (0, 0, 300), "empty_probe": (300, 40, 0), "one_row": (1, 1, 1), "dups": (300, 40, 300), "distinct": (300, 300, 300),
}
_cache = {}


def _inputs(size):
    """(bk, bv, pk, pv): build keys with `distinct` different values, about half of the probe rows with a partner, value columns"""
    if size not in _cache:
        nb, distinct, n_p = SIZES[size]
        rng = np.random.default_rng(nb * 1000 + distinct + n_p)
        ids = (np.arange(distinct, dtype=np.uint64) + np.uint64(1)) * GOLDEN
        bk = np.concatenate([ids, rng.choice(ids, nb - distinct)]) if nb else np.empty(0, np.uint64)
        rng.shuffle(bk)
        pool = np.concatenate([ids, (np.arange(max(distinct, 1), dtype=np.uint64) + np.uint64(5000)) * GOLDEN])
        pk = rng.choice(pool, n_p).astype(np.uint64)
        bv = rng.integers(0, 2**64, size=nb, dtype=np.uint64)
        pv = rng.integers(0, 2**64, size=n_p, dtype=np.uint64)
        for a in (bk, bv, pk, pv):
            a.setflags(write=False)
        _cache[size] = (bk, bv, pk, pv)
    return _cache[size]


@pytest.fixture(scope="module")
def L():
    import flash_join
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_device_count() >= 1, "no HIP device"
    flash_join.initialize()
    return _lib.load()


def _ptr(a):
    return a.ctypes.data if a is not None else None


def _host(L, algo, materialize, bk, bv, nb, pk, n_p, ncounts, want_k, want_v, sizes):
    """fj_join_host; sizes(counts) -> (bytes of *out_keys, words of *out_vals).  Returns (counts, key bytes or None, value words or None)."""
    from flash_hash_join_amd import _lib
    cnt = (ctypes.c_uint64 * 3)(7, 7, 7)
    sec = ctypes.c_double(0)
    ok, ov = ctypes.c_void_p(), ctypes.c_void_p()
    try:
        _lib.check(L.fj_join_host(algo, 0, materialize, _ptr(bk), _ptr(bv), nb, _ptr(pk), n_p, cnt, ctypes.byref(sec),
                                  ctypes.byref(ok) if want_k else None, ctypes.byref(ov) if want_v else None))
        counts = [int(cnt[i]) for i in range(ncounts)]
        assert all(int(cnt[i]) == 7 for i in range(ncounts, 3)), "a count word beyond the form's was written"
        kbytes, vwords = sizes(counts)
        take = lambda p, n: np.frombuffer(ctypes.string_at(p.value, n), dtype=np.uint8).copy() if n else np.empty(0, np.uint8)
        keys = vals = None
        if want_k and materialize:
            assert ok.value or not kbytes
            keys = take(ok, kbytes)
        if want_v and materialize:
            assert ov.value or not vwords
            vals = take(ov, vwords * 8).view(np.uint64)
        return counts, keys, vals
    finally:
        L.fj_free_host(ok)
        L.fj_free_host(ov)


def _device(L, algo, materialize, bk, bv, nb, pk, n_p, ncounts, krows, vrows, cap, emit_rows=None):
    """fj_join_device on device copies into buffers of krows / vrows words (None: a null pointer) and capacity `cap`; emit_rows: a
    function of the counts - the call is made without buffers and fj_emit_pairs writes that many rows.  Returns (counts, ok, ov) as
    NumPy words."""
    import torch
    from flash_hash_join_amd import _lib, api
    ctx = api.context(0)
    stream = torch.cuda.current_stream(0).cuda_stream
    dev = lambda a: torch.from_numpy(a.view(np.int64).copy()).cuda() if a is not None and a.size else None
    d_bk, d_bv, d_pk = dev(bk), dev(bv), dev(pk)
    p = lambda t: t.data_ptr() if t is not None else None
    buf = lambda rows: torch.full((max(rows, 1),), 0x5A5A5A5A, dtype=torch.int64, device="cuda") if rows is not None else None
    cnt = (ctypes.c_uint64 * 3)(7, 7, 7)
    if emit_rows is None:
        ok, ov = buf(krows), buf(vrows)
        _lib.check(L.fj_join_device(ctx, algo, 0, materialize, p(d_bk), p(d_bv), nb, p(d_pk), n_p, stream, 64, cnt, p(ok), p(ov), cap, None))
        counts = [int(cnt[i]) for i in range(ncounts)]
    else:
        _lib.check(L.fj_join_device(ctx, algo, 0, materialize, p(d_bk), p(d_bv), nb, p(d_pk), n_p, stream, 64, cnt, None, None, 0, None))
        counts = [int(cnt[i]) for i in range(ncounts)]
        rows = emit_rows(counts)
        ok, ov = buf(rows), buf(rows)
        if rows or (algo & ALL):                                         # (a join without a pair leaves nothing pending; all-copies always does)
            _lib.check(L.fj_emit_pairs(ctx, p(ok), p(ov), rows, stream, None))
    torch.cuda.synchronize()
    host = lambda t: t.cpu().numpy().view(np.uint64) if t is not None else None
    return counts, host(ok), host(ov)


def _sorted_pairs(k, v, *ranges):
    """rows sorted within each of the ranges [a, b): one (n, 2) array"""
    out = np.stack([k, v], axis=1)
    for a, b in ranges:
        part = out[a:b]
        out[a:b] = part[np.lexsort((part[:, 1], part[:, 0]))]
    return out


def _mult(bk, pk):
    """build rows per probe key"""
    u, c = np.unique(bk, return_counts=True)
    pos = np.searchsorted(u, pk)
    pos[pos >= u.size] = 0
    return np.where(u[pos] == pk, c[pos], 0) if u.size else np.zeros(pk.size, np.int64)


# ---- the joins -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("algo", [2, 0, MANY | 2, ROW_IDS | 2], ids=["radix", "adaptive", "many", "row_ids"])
def test_pending_pairs(L, size, algo):
    bk, bv, pk, _ = _inputs(size)
    hc, hk, hv = _host(L, algo, 1, bk, bv, bk.size, pk, pk.size, 1, True, True, lambda c: (c[0] * 8, c[0]))
    dc, dk, dv = _device(L, algo, 1, bk, bv, bk.size, pk, pk.size, 1, None, None, 0, emit_rows=lambda c: c[0])
    exp = int(_mult(bk, pk).sum()) if algo & MANY else int(np.isin(pk, bk).sum())
    assert hc == dc == [exp]
    n = exp
    hk = hk.view(np.uint64) if hk is not None and hk.size else np.empty(0, np.uint64)
    hv = hv if hv is not None else np.empty(0, np.uint64)
    assert np.array_equal(_sorted_pairs(hk[:n], hv[:n], (0, n)), _sorted_pairs(dk[:n], dv[:n], (0, n)))
    # the counting form hands nothing out
    hc0, k0, v0 = _host(L, algo & ~ROW_IDS, 0, bk, bv, bk.size, pk, pk.size, 1, True, True, lambda c: (0, 0))
    assert hc0 == [exp] and k0 is None and v0 is None


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("algo", [LEFT | ALL | 2, FULL | ALL, FULL | ALL | ROW_IDS | 2], ids=["left", "full", "full_row_ids"])
def test_all_copies(L, size, algo):
    bk, bv, pk, _ = _inputs(size)
    rows = lambda c: c[0] + c[1] + c[2]
    hc, hk, hv = _host(L, algo, 1, bk, bv, bk.size, pk, pk.size, 3, True, True, lambda c: (rows(c) * 8, rows(c)))
    dc, dk, dv = _device(L, algo, 1, bk, bv, bk.size, pk, pk.size, 3, None, None, 0, emit_rows=rows)
    P, u = int(_mult(bk, pk).sum()), int((~np.isin(pk, bk)).sum())
    r = int((~np.isin(bk, pk)).sum()) if algo & FULL else 0
    assert hc == dc == [P, r, u]
    n = P + u + r
    ranges = ((0, P), (P, P + u), (P + u, n))
    assert np.array_equal(_sorted_pairs(hk.view(np.uint64), hv, *ranges), _sorted_pairs(dk[:n], dv[:n], *ranges))


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("algo", [FULL | 2, FULL | ROW_IDS], ids=["full", "full_row_ids"])
def test_full_outer(L, size, algo):
    bk, bv, pk, _ = _inputs(size)
    nb, n_p = bk.size, pk.size
    hc, hk, hv = _host(L, algo, 1, bk, bv, nb, pk, n_p, 2, True, True, lambda c: ((n_p + c[1]) * 8, n_p + c[1]))
    dc, dk, dv = _device(L, algo, 1, bk, bv, nb, pk, n_p, 2, n_p + nb, n_p + nb, n_p + nb)
    m, r = int(np.isin(pk, bk).sum()), int((~np.isin(bk, pk)).sum())
    assert hc == dc == [m, r]
    n = n_p + r
    ranges = ((0, m), (m, n_p), (n_p, n))
    assert np.array_equal(_sorted_pairs(hk.view(np.uint64), hv, *ranges), _sorted_pairs(dk[:n], dv[:n], *ranges))


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("algo,want_v", [(LEFT | 2, True), (LEFT | ROW_IDS, True), (ANTI | 2, True), (ANTI, False), (ANTI | ROW_IDS | 2, False)],
                         ids=["left", "left_row_ids", "anti", "anti_keys_only", "anti_row_ids_keys_only"])
def test_left_outer_and_anti(L, size, algo, want_v):
    bk, bv, pk, _ = _inputs(size)
    nb, n_p = bk.size, pk.size
    left = bool(algo & LEFT)
    rows = (lambda c: n_p) if left else (lambda c: c[0])
    hc, hk, hv = _host(L, algo, 1, bk, bv, nb, pk, n_p, 1, True, want_v, lambda c: (rows(c) * 8, rows(c) if left else 0))
    dc, dk, dv = _device(L, algo, 1, bk, bv, nb, pk, n_p, 1, n_p, n_p if left else None, n_p)
    m = int(np.isin(pk, bk).sum())
    assert hc == dc == [m if left else n_p - m]
    n = rows(hc)
    if left:
        ranges = ((0, m), (m, n_p))
        assert np.array_equal(_sorted_pairs(hk.view(np.uint64), hv, *ranges), _sorted_pairs(dk[:n], dv[:n], *ranges))
    else:
        assert np.array_equal(np.sort(hk.view(np.uint64)), np.sort(dk[:n]))
    # the counting anti join: no array
    if not left:
        assert _host(L, algo & ~ROW_IDS, 0, bk, bv, nb, pk, n_p, 1, True, want_v, lambda c: (0, 0))[0] == [n_p - m]


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("want_k,want_v", [(True, True), (True, False), (False, True)], ids=["both", "mask_only", "values_only"])
@pytest.mark.parametrize("algo", [PO | 2, PO | ROW_IDS], ids=["values", "row_ids"])
def test_probe_order(L, size, algo, want_k, want_v):
    bk, bv, pk, _ = _inputs(size)
    nb, n_p = bk.size, pk.size
    hc, hk, hv = _host(L, algo, 1, bk, bv, nb, pk, n_p, 1, want_k, want_v, lambda c: (n_p, n_p))
    # the mask is np BYTES of d_out_keys: a buffer of whole words holds them
    dc, dk, dv = _device(L, algo, 1, bk, bv, nb, pk, n_p, 1, (n_p + 7) // 8 if want_k else None, n_p if want_v else None, n_p)
    assert hc == dc == [int(np.isin(pk, bk).sum())]
    if want_k:
        assert np.array_equal(hk, dk.view(np.uint8)[:n_p]) and np.array_equal(hk.astype(bool), np.isin(pk, bk))
    if want_v:
        assert np.array_equal(hv, dv[:n_p])


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("algo,want_k,want_v", [(BO | 2, True, True), (BO, True, False), (BO | 2, False, True), (BO | MIN | SIGNED, True, True), (BO | MAX | 2, False, True)],
                         ids=["sum_both", "counts_only", "sums_only", "min_signed_both", "max_only"])
def test_build_order(L, size, algo, want_k, want_v):
    bk, _, pk, pv = _inputs(size)
    nb, n_p = bk.size, pk.size
    hc, hk, hv = _host(L, algo, 1, bk, pv, nb, pk, n_p, 1, want_k, want_v, lambda c: (nb * 8, nb))
    dc, dk, dv = _device(L, algo, 1, bk, pv, nb, pk, n_p, 1, nb if want_k else None, nb if want_v else None, nb)
    assert hc == dc == [int(_mult(bk, pk).sum())]
    if want_k:
        assert np.array_equal(hk.view(np.uint64), dk[:nb])
    if want_v:
        assert np.array_equal(hv, dv[:nb])


# ---- group-by on one relation ----------------------------------------------------------------------------------------------------
GROUP_SIZES = [s for s in SIZES if s != "empty_probe"]          # (no probe side: that size is "dups" again)


def _by_key(keys, *columns):
    order = np.lexsort(tuple(reversed((keys,) + columns[:1]))) if columns else np.argsort(keys, kind="stable")
    return [keys[order]] + [c[order] for c in columns]


@pytest.mark.parametrize("size", GROUP_SIZES)
@pytest.mark.parametrize("want_k,want_v", [(True, True), (True, False), (False, True)], ids=["both", "keys_only", "aggregates_only"])
@pytest.mark.parametrize("algo,with_values", [(GB | 2, False), (GB, True), (GB | MAX | 2, True), (GB | MIN | SIGNED, True), (GB | ROW_IDS | 2, False)],
                         ids=["count", "sum", "max", "min_signed", "row_ids"])
def test_plain_group_by(L, size, algo, with_values, want_k, want_v):
    bk, bv, _, _ = _inputs(size)
    nb = bk.size
    vals = bv if with_values else None
    hc, hk, hv = _host(L, algo, 1, bk, vals, nb, None, 0, 1, want_k, want_v, lambda c: (c[0] * 8, c[0]))
    dc, dk, dv = _device(L, algo, 1, bk, vals, nb, None, 0, 1, nb, nb, nb)
    g = np.unique(bk).size
    assert hc == dc == [g]
    dk, dv = _by_key(dk[:g], dv[:g])
    if want_k and want_v:
        hk, hv = _by_key(hk.view(np.uint64), hv)
        assert np.array_equal(hk, dk) and np.array_equal(hv, dv)
    elif want_k:
        assert np.array_equal(np.sort(hk.view(np.uint64)), dk)
    else:
        assert np.array_equal(np.sort(hv), np.sort(dv))
    # materialize = 0: the number of distinct keys alone
    assert _host(L, algo & ~ROW_IDS, 0, bk, vals, nb, None, 0, 1, want_k, want_v, lambda c: (0, 0)) == ([g], None, None)


@pytest.mark.parametrize("size", GROUP_SIZES)
@pytest.mark.parametrize("algo,want_k,want_v", [(GB | INV | 2, True, True), (GB | INV, False, True), (GB | INV | 2, True, False), (GB | INV | PAIR, True, True)],
                         ids=["both", "ids_only", "ids_not_taken", "key_pair"])
def test_inverse(L, size, algo, want_k, want_v):
    bk, bv, _, _ = _inputs(size)
    nb = bk.size
    pair = bool(algo & PAIR)
    second = (bv & np.uint64(1)) if pair else None                       # a second key column of two values
    hc, hk, hv = _host(L, algo, 1, bk, second, nb, None, 0, 1, want_k, want_v, lambda c: (c[0] * 8, nb))
    dc, dk, dv = _device(L, algo, 1, bk, second, nb, None, 0, 1, nb, nb, nb)
    g = np.unique(np.stack([bk, second], axis=1), axis=0).shape[0] if pair else np.unique(bk).size
    assert hc == dc == [g]
    ids_d = dv[:nb].astype(np.int64)
    if want_k and want_v:                                                 # g keys (KEY_PAIR: first rows) and nb ids that index them
        ids_h = hv.astype(np.int64)
        assert np.array_equal(np.sort(hk.view(np.uint64)), np.sort(dk[:g]))
        if nb:
            assert ids_h.max() < g and np.array_equal(hk.view(np.uint64)[ids_h], dk[:g][ids_d])
            if not pair:
                assert np.array_equal(hk.view(np.uint64)[ids_h], bk)
    elif want_v:                                                          # the ids alone: the same partition of the rows
        ids_h = hv.astype(np.int64)
        assert np.unique(np.stack([ids_h, ids_d], axis=1), axis=0).shape[0] == g and np.unique(ids_h).size == g
    else:                                                                 # nobody takes the ids: the plain distinct form
        assert hv is None and np.array_equal(np.sort(hk.view(np.uint64)), np.sort(dk[:g]))


@pytest.mark.parametrize("size", GROUP_SIZES)
@pytest.mark.parametrize("algo,planes", [(GB | AALL | 2, 4), (GB | AALL | SIGNED, 4), (GB | AARG | MIN | 2, 2), (GB | AARG | MAX | SIGNED, 2),
                                         (GB | AALL | AMERGE | 2, 4), (GB | AALL | PAIR, 5)],
                         ids=["agg_all", "agg_all_signed", "argmin", "argmax_signed", "merge", "pair_agg"])
def test_plane_forms(L, size, algo, planes):
    bk, bv, _, _ = _inputs(size)
    nb = bk.size
    pk, n_p = None, 0
    if algo & AMERGE:                                                    # partial rows: four planes of nb words (counts >= 1)
        rng = np.random.default_rng(nb)
        vals = np.concatenate([rng.integers(1, 9, size=nb, dtype=np.uint64), bv, bv, bv])
    elif algo & PAIR:                                                    # the second key column, and the value column as the probe side
        vals, pk, n_p = bv & np.uint64(1), bv, nb
    else:
        vals = bv
    cap = max(nb, 1)
    hc, hk, hv = _host(L, algo, 1, bk, vals, nb, pk, n_p, 1, True, True, lambda c: (c[0] * 8, planes * c[0]))
    dc, dk, dv = _device(L, algo, 1, bk, vals, nb, pk, n_p, 1, cap, planes * cap, cap)
    g = np.unique(np.stack([bk, vals], axis=1), axis=0).shape[0] if algo & PAIR else np.unique(bk).size
    assert hc == dc == [g]
    h = _by_key(hk.view(np.uint64), *[hv[i * g:(i + 1) * g] for i in range(planes)])       # host: stride g
    d = _by_key(dk[:g], *[dv[i * cap:i * cap + g] for i in range(planes)])                 # device: stride cap
    for a, b in zip(h, d):
        assert np.array_equal(a, b)
    if not algo & (AMERGE | AARG):
        count_plane = 1 if algo & PAIR else 0
        assert int(h[1 + count_plane].sum()) == nb


@pytest.mark.parametrize("size", GROUP_SIZES)
@pytest.mark.parametrize("want_k,want_v", [(True, True), (True, False), (False, True)], ids=["both", "keys_only", "rows_only"])
@pytest.mark.parametrize("base", [0, 2], ids=["adaptive", "radix"])
def test_group_rows(L, size, base, want_k, want_v):
    bk, _, _, _ = _inputs(size)
    nb = bk.size
    cap = max(nb, 1)
    hc, hk, hv = _host(L, GB | ROWS | base, 1, bk, None, nb, None, 0, 1, want_k, want_v, lambda c: (c[0] * 8, nb + c[0]))
    dc, dk, dv = _device(L, GB | ROWS | base, 1, bk, None, nb, None, 0, 1, cap, 2 * cap, cap)
    g = np.unique(bk).size
    assert hc == dc == [g]

    def groups(rows, starts):
        """the sorted rows of every group, the groups in the order of their smallest row"""
        ends = np.append(starts[1:], nb).astype(np.int64)
        gs = [tuple(np.sort(rows[int(a):int(b)]).tolist()) for a, b in zip(starts.astype(np.int64), ends)]
        return sorted(gs)

    d_groups = groups(dv[:nb], dv[cap:cap + g])
    if want_k:
        assert np.array_equal(np.sort(hk.view(np.uint64)), np.sort(dk[:g]))
    if want_v:
        assert groups(hv[:nb], hv[nb:nb + g]) == d_groups
        assert sorted(int(x) for grp in d_groups for x in grp) == list(range(nb))
        if want_k and nb:                                                 # group j of the rows is key j
            assert all(bk[int(hv[int(a)])] == k for k, a in zip(hk.view(np.uint64), hv[nb:nb + g]))
