"""Build-order min / max joins (FJ_ALGO_BUILD_ORDER | FJ_ALGO_AGG_MIN / FJ_ALGO_AGG_MAX [| FJ_ALGO_AGG_SIGNED], csrc/fj_group.hip;
api.group_join_min / group_join_max): one minimum or maximum of a probe-side value column per build row, at the build row's position.
The C-ABI contract, the refusals and the argument checks need no GPU; on an MI355X the four forms (min / max, unsigned / signed) are
compared element for element with a NumPy reference on every plan the sum form is tested on.

Reference: a stable sort of the probe keys, np.minimum.reduceat / np.maximum.reduceat over the probe values in that order (uint64, or
their int64 view for the signed forms), searchsorted back to the build rows; a build row without a partner holds the aggregate's
identity.  No hashing anywhere, never the library."""
import ctypes
import functools
import os
import re
import zlib

import numpy as np
import pytest

import hbm_timings
import keymix
from conftest import ROOT

MANY, LEFT, ANTI, ROW_IDS, FULL, ALL, PO, BO = 0x10, 0x20, 0x40, 0x80, 0x100, 0x200, 0x800, 0x1000
MIN, MAX, SIGNED = 0x4000, 0x8000, 0x10000
U64_MAX, I64_MAX, I64_MIN = 2**64 - 1, 2**63 - 1, 2**63                # the words
IDENTITY = {("min", False): U64_MAX, ("min", True): I64_MAX, ("max", False): 0, ("max", True): I64_MIN}
FORMS = [("min", False), ("min", True), ("max", False), ("max", True)]


def ref_counts(bk, pk):
    bk, pk = np.asarray(bk, dtype=np.uint64), np.asarray(pk, dtype=np.uint64)
    sp = np.sort(pk, kind="stable")
    return (np.searchsorted(sp, bk, "right") - np.searchsorted(sp, bk, "left")).astype(np.int64)


def ref_minmax(bk, pk, pv, op, signed):
    """the uint64 words of the aggregate, aligned with bk; the identity where a build key has no probe row"""
    bk, pk, pv = (np.asarray(a, dtype=np.uint64) for a in (bk, pk, pv))
    out = np.full(bk.size, IDENTITY[(op, signed)], dtype=np.uint64)
    if pk.size == 0 or bk.size == 0:
        return out
    order = np.argsort(pk, kind="stable")
    sp, sv = pk[order], pv[order]
    starts = np.flatnonzero(np.concatenate([[True], sp[1:] != sp[:-1]]))
    col = sv.view(np.int64) if signed else sv
    red = (np.minimum if op == "min" else np.maximum).reduceat(col, starts).view(np.uint64)
    ukeys = sp[starts]
    idx = np.minimum(np.searchsorted(ukeys, bk), ukeys.size - 1)
    hit = ukeys[idx] == bk
    out[hit] = red[idx[hit]]
    return out


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_header_flags_and_python_mirrors():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    from flash_hash_join_amd import api
    for name, value in (("AGG_MIN", 0x4000), ("AGG_MAX", 0x8000), ("AGG_SIGNED", 0x10000)):
        assert int(re.search(r"#define FJ_ALGO_%s\s+(0x[0-9a-fA-F]+)" % name, hdr).group(1), 16) == value
        assert getattr(api, "ALGO_" + name) == value
    assert "counts" in hdr[hdr.index("FJ_ALGO_AGG_MIN"):hdr.index("#define FJ_ALGO_AGG_MIN")]     # the identity note points to the counts


def test_abi_version_and_function_count_are_unchanged():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    assert int(re.search(r"#define FJ_ABI_VERSION (\d+)", hdr).group(1)) == 8
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert len(set(re.findall(r"\b(fj_[a-z0-9_]+)\s*\(", code))) == 40
    for name in ("FJ_ALGO_AGG_MIN", "FJ_ALGO_AGG_MAX", "FJ_ALGO_AGG_SIGNED"):
        assert re.search(r"#define %s\b" % name, code)
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_abi_version() == 8 and len(_lib.SYMBOLS) == 40


def test_flash_join_exposes_the_two_functions():
    import flash_join
    from flash_hash_join_amd import api
    for name in ("group_join_min", "group_join_max"):
        assert callable(getattr(flash_join, name)) and name in api.EXTENSIONS and name in api.__all__


def _device_call(algo, materialize=1, pv=0x20000, counts=0x40000, vals=0x50000, cap=100, nb=100, n_p=1000):
    from flash_hash_join_amd import _lib
    cnt = ctypes.c_uint64(0)
    rc = _lib.load().fj_join_device(None, algo, 0, materialize, 0x10000, pv, nb, 0x30000, n_p, None, 64, ctypes.byref(cnt), counts, vals, cap, None)
    return rc, _lib.last_error()


DEVICE_REFUSALS = [   # id, keyword arguments of _device_call, needles
    ("min_and_max", dict(algo=BO | MIN | MAX), ("FJ_ALGO_AGG_MIN", "FJ_ALGO_AGG_MAX", "one aggregate per call")),
    ("min_and_max_signed", dict(algo=BO | MIN | MAX | SIGNED | 2), ("FJ_ALGO_AGG_MIN", "FJ_ALGO_AGG_MAX")),
    ("signed_alone", dict(algo=BO | SIGNED), ("FJ_ALGO_AGG_SIGNED", "FJ_ALGO_AGG_MIN", "no sign")),
    ("signed_alone_counts_only", dict(algo=BO | SIGNED | 1, vals=None, pv=None), ("FJ_ALGO_AGG_SIGNED",)),
    ("bare_min", dict(algo=MIN), ("unknown algo 16384",)),
    ("bare_max", dict(algo=MAX | 2), ("unknown algo",)),
    ("bare_signed", dict(algo=SIGNED), ("unknown algo 65536",)),
    ("bare_min_signed", dict(algo=MIN | SIGNED), ("unknown algo",)),
    ("probe_order_min", dict(algo=PO | MIN, cap=1000), ("unknown algo",)),
    ("many_max", dict(algo=MANY | MAX | 2), ("unknown algo",)),
    ("left_min_signed", dict(algo=LEFT | MIN | SIGNED, cap=1000), ("unknown algo",)),
    ("min_without_values_output", dict(algo=BO | MIN, vals=None), ("FJ_ALGO_AGG_MIN", "d_out_vals")),
    ("max_signed_without_values_output", dict(algo=BO | MAX | SIGNED | 2, vals=None), ("FJ_ALGO_AGG_MAX", "d_out_vals")),
    ("min_without_probe_values", dict(algo=BO | MIN, pv=None), ("d_build_vals",)),
    ("max_only_without_probe_values", dict(algo=BO | MAX | SIGNED, pv=None, counts=None), ("d_build_vals",)),
    # everything FJ_ALGO_BUILD_ORDER already refuses, with its present message
    ("many", dict(algo=BO | MIN | MANY), ("FJ_ALGO_BUILD_ORDER cannot be combined with FJ_ALGO_MANY_TO_MANY",)),
    ("row_ids", dict(algo=BO | MAX | ROW_IDS), ("FJ_ALGO_BUILD_ORDER cannot be combined with FJ_ALGO_ROW_IDS",)),
    ("probe_order", dict(algo=BO | MIN | SIGNED | PO), ("FJ_ALGO_BUILD_ORDER cannot be combined with FJ_ALGO_PROBE_ORDER",)),
    ("count", dict(algo=BO | MIN, materialize=0), ("FJ_ALGO_BUILD_ORDER", "materialize = 1")),
    ("no_output", dict(algo=BO | MAX, counts=None, vals=None), ("FJ_ALGO_BUILD_ORDER", "needs an output")),
    ("capacity", dict(algo=BO | MIN | SIGNED, cap=99), ("output capacity",)),
    ("misaligned_values", dict(algo=BO | MAX | 2, vals=0x50004), ("8-byte aligned",)),
    ("misaligned_counts", dict(algo=BO | MIN, counts=0x40004), ("8-byte aligned",)),
    ("base_3", dict(algo=BO | MIN | 3), ("unknown algo",)),
]


@pytest.mark.parametrize("cid,kw,needles", DEVICE_REFUSALS, ids=[r[0] for r in DEVICE_REFUSALS])
def test_invalid_combinations_are_refused_before_any_device_work(cid, kw, needles):
    """A NULL context: the checks come before the context is touched (no GPU needed; the pointers are never dereferenced)."""
    rc, err = _device_call(**kw)
    assert rc != 0 and "null context" not in err, err
    for needle in needles:
        assert needle in err, err


VALID = [(f"{'min' if agg == MIN else 'max'}_{'signed' if sg else 'unsigned'}_{'counts' if cnt else 'alone'}_base{base}",
          dict(algo=BO | agg | sg | base, counts=0x40000 if cnt else None))
         for agg in (MIN, MAX) for sg in (0, SIGNED) for cnt in (False, True) for base in (0, 1, 2)]


@pytest.mark.parametrize("cid,kw", VALID, ids=[v[0] for v in VALID])
def test_valid_combinations_reach_the_context(cid, kw):
    rc, err = _device_call(**kw)
    assert rc != 0 and "null context" in err, err


def test_the_skipped_bits_and_the_next_free_bit_are_still_unknown():
    for algo in (0x400, 0x2000, 0x20000, BO | 0x400, BO | 0x2000, BO | 0x20000, BO | MIN | 0x400, BO | MAX | SIGNED | 0x2000, BO | MIN | 0x20000):
        rc, err = _device_call(algo=algo)
        assert rc != 0 and "unknown algo" in err and "null context" not in err, (hex(algo), err)
    for algo, needle in ((0x400, "unknown algo 1024"), (0x2000, "unknown algo 8192"), (0x20000, "unknown algo 131072")):
        assert needle in _device_call(algo=algo)[1]


HOST_REFUSALS = [   # id, algo, materialize, probe values, want counts, want values, needles
    ("min_and_max", BO | MIN | MAX, 1, True, True, True, ("FJ_ALGO_AGG_MIN", "FJ_ALGO_AGG_MAX", "one aggregate per call")),
    ("signed_alone", BO | SIGNED, 1, True, True, True, ("FJ_ALGO_AGG_SIGNED", "no sign")),
    ("bare_min", MIN, 1, True, True, True, ("unknown algo 16384",)),
    ("bare_max", MAX | 2, 1, True, True, True, ("unknown algo",)),
    ("bare_signed", SIGNED, 1, True, True, True, ("unknown algo 65536",)),
    ("probe_order_min", PO | MIN, 1, True, True, True, ("unknown algo",)),
    ("min_without_values_output", BO | MIN, 1, True, True, False, ("FJ_ALGO_AGG_MIN", "out_vals")),
    ("max_signed_without_values_output", BO | MAX | SIGNED, 1, True, True, False, ("FJ_ALGO_AGG_MAX", "out_vals")),
    ("min_without_probe_values", BO | MIN, 1, False, True, True, ("build_vals",)),
    ("many", BO | MAX | MANY, 1, True, True, True, ("FJ_ALGO_BUILD_ORDER cannot be combined with FJ_ALGO_MANY_TO_MANY",)),
    ("count", BO | MIN | SIGNED, 0, True, True, True, ("FJ_ALGO_BUILD_ORDER", "materialize = 1")),
    ("no_output", BO | MAX, 1, True, False, False, ("needs an output",)),
    ("skipped_bit", BO | MIN | 0x2000, 1, True, True, True, ("unknown algo",)),
    ("next_bit", BO | MIN | 0x20000, 1, True, True, True, ("unknown algo",)),
    ("base_9", BO | MAX | 9, 1, True, True, True, ("unknown algo",)),
]


@pytest.mark.parametrize("cid,algo,materialize,pv,want_counts,want_vals,needles", HOST_REFUSALS, ids=[r[0] for r in HOST_REFUSALS])
def test_host_entry_refusals(cid, algo, materialize, pv, want_counts, want_vals, needles):
    """fj_join_host makes the same checks before its context is created (no GPU needed)."""
    from flash_hash_join_amd import _lib
    L = _lib.load()
    k = np.arange(8, dtype=np.uint64)
    cnt, sec = ctypes.c_uint64(0), ctypes.c_double(0)
    oc, ov = ctypes.c_void_p(), ctypes.c_void_p()
    rc = L.fj_join_host(algo, 0, materialize, k.ctypes.data, k.ctypes.data if pv else None, 8, k.ctypes.data, 8, ctypes.byref(cnt), ctypes.byref(sec),
                        ctypes.byref(oc) if want_counts else None, ctypes.byref(ov) if want_vals else None)
    err = _lib.last_error()
    assert rc != 0 and "null context" not in err and "HIP device" not in err, err
    for needle in needles:
        assert needle in err, err
    assert not oc.value and not ov.value


def test_python_argument_errors():
    from flash_hash_join_amd import api
    k = np.arange(4, dtype=np.uint64)
    for fn in (api.group_join_min, api.group_join_max):
        with pytest.raises(ValueError, match="probe_values has 3 elements"):
            fn(k, k, k[:3])
        with pytest.raises(ValueError, match="probe_values has 5 elements"):
            fn(k, k, np.arange(5, dtype=np.int64), return_counts=True, signed=False)
        with pytest.raises(ValueError, match="probe_values is required"):
            fn(k, k, None)
        with pytest.raises(TypeError):
            fn(k, k)                                                   # probe_values is not optional
        with pytest.raises(TypeError, match="probe_values"):
            fn(k, k, np.array(["a", "b", "c", "d"]))
        with pytest.raises(TypeError, match="signed"):
            fn(k, k, k, signed="yes")
        with pytest.raises(TypeError):
            fn(k, k, k, fill_value=0)                                  # there is none: the counts tell "no partner" apart


def test_numpy_reference_on_a_hand_written_case():
    T = 2**63
    bk = np.array([5, 7, 9, 7, 11, 13, 2, 3], dtype=np.uint64)           # 7 twice, 9 without a probe row
    pk = np.array([7, 5, 7, 5, 11, 13, 2, 3, 7, 100], dtype=np.uint64)
    pv = np.array([10, 1, T + 7, T + 5, U64_MAX, T - 1, 0, T, 3, 42], dtype=np.uint64)   # 11, 13, 2, 3: the only value is an identity
    counts = ref_counts(bk, pk)
    assert counts.dtype == np.int64 and counts.tolist() == [2, 3, 0, 3, 1, 1, 1, 1] and int(counts.sum()) == 12
    exp = {("min", False): [1, 3, U64_MAX, 3, U64_MAX, T - 1, 0, T],
           ("min", True): [T + 5, T + 7, T - 1, T + 7, U64_MAX, T - 1, 0, T],        # T + 5 is -2^63 + 5
           ("max", False): [T + 5, T + 7, 0, T + 7, U64_MAX, T - 1, 0, T],
           ("max", True): [1, 10, T, 10, U64_MAX, T - 1, 0, T]}
    for (op, signed), want in exp.items():
        got = ref_minmax(bk, pk, pv, op, signed)
        assert got.dtype == np.uint64 and got.tolist() == want, (op, signed, got.tolist())
    # a true aggregate that equals the identity reads like "no partner"; the counts tell them apart
    umin = ref_minmax(bk, pk, pv, "min", False)
    assert umin[2] == umin[4] == U64_MAX and counts[2] == 0 and counts[4] == 1
    assert ref_minmax(bk, pk, pv, "min", True).tolist() != umin.tolist() and exp[("max", True)] != exp[("max", False)]
    for form in FORMS:
        assert ref_minmax(bk, np.empty(0, np.uint64), np.empty(0, np.uint64), *form).tolist() == [IDENTITY[form]] * 8
        assert ref_minmax(np.empty(0, np.uint64), pk, pv, *form).size == 0


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fj():
    import flash_join
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_device_count() >= 1, "no HIP device: the product path must not silently fall back"
    assert flash_join.initialize() is None
    return flash_join


def _plant(bk, pk, pv):
    """the four identities (0, 2^64 - 1, 2^63 - 1, 2^63): each on one probe row that hits, and each on EVERY row of one hit key - the
    key whose true aggregate equals the identity of one form"""
    hit_rows = np.flatnonzero(np.isin(pk, bk))
    if bk.size < 16 or hit_rows.size < 64:
        return pv
    keys, first, cnt = np.unique(pk[hit_rows], return_index=True, return_counts=True)
    small = np.flatnonzero(cnt <= 64)                                  # (not the hot key)
    assert small.size >= 8
    words = np.array([0, U64_MAX, I64_MAX, I64_MIN], dtype=np.uint64)
    for j, w in enumerate(words):
        pv[pk == keys[small[j]]] = w                                   # all of the key's rows
        pv[hit_rows[first[small[4 + j]]]] = w                          # one row of another key
    return pv


def _case(nb, n_p, hit, seed, dups=True):
    rng = np.random.default_rng(seed)
    bk = rng.integers(0, 2**64, size=nb, dtype=np.uint64)
    if not dups:
        bk = np.unique(bk)
        rng.shuffle(bk)
        nb = bk.size
    if nb >= 8:
        bk[0], bk[1] = 0, np.uint64(U64_MAX)                              # raw zero and raw 2^64 - 1: the HBM table's empty marker
        bk[2], bk[3] = keymix.EMPTY_RAW, keymix.FILLER_RAW                # the LDS tables' empty marker and the wide kernel's filler
        if dups:
            d = max(1, nb // 20)
            bk[nb - d:] = bk[4:4 + d]                                     # duplicated build keys
            bk[nb - d - 1] = keymix.EMPTY_RAW                             # ... the marker among them
    nhit = int(n_p * hit) if nb else 0
    parts = [rng.choice(bk, nhit)] if nhit else []                        # (probe keys repeat)
    parts.append(rng.integers(1, 2**63, size=n_p - nhit, dtype=np.uint64) * np.uint64(2) + np.uint64(2**63))   # ~never a build key
    pk = np.concatenate(parts)[:n_p] if n_p else np.empty(0, np.uint64)
    if n_p >= 16 and 0.0 < hit < 1.0:
        pk[:8] = np.array([0, 2**64 - 1, keymix.EMPTY_RAW, keymix.FILLER_RAW] * 2, dtype=np.uint64)   # ... on the probe side too
    rng.shuffle(pk)
    pv = rng.integers(0, 2**64, size=pk.size, dtype=np.uint64)            # full width: about half have the top bit set
    return bk, pk, _plant(bk, pk, pv)


class Ref:
    """a case and its references, computed once and never modified"""
    def __init__(self, bk, pk, pv):
        self.bk, self.pk, self.pv = bk, pk, pv
        self.counts = ref_counts(bk, pk)
        self.P = int(self.counts.sum())
        self.vals = {form: ref_minmax(bk, pk, pv, *form) for form in FORMS}
        for a in (self.bk, self.pk, self.pv, self.counts, *self.vals.values()):
            a.setflags(write=False)
        self._dev = None

    def args(self, device):
        if not device:
            return self.bk, self.pk, self.pv
        if self._dev is None:
            import torch
            self._dev = tuple(torch.from_numpy(np.array(a).view(np.int64)).cuda() for a in (self.bk, self.pk, self.pv))
        return self._dev

    def check_data(self, hit_lo=0.4, hit_hi=0.6):
        """what the test relies on in its own data"""
        n_p = self.pk.size
        hits = int(np.isin(self.pk, self.bk).sum())
        assert hit_lo * n_p <= hits <= hit_hi * n_p, (hits, n_p)
        for op in ("min", "max"):
            assert (self.vals[(op, False)] != self.vals[(op, True)]).any(), "signed and unsigned agree everywhere: the case tests no sign"
        top = int((self.pv >> np.uint64(63)).sum())
        assert 0.4 * n_p < top < 0.6 * n_p
        if self.bk.size >= 16:
            hv = self.pv[np.isin(self.pk, self.bk)]
            for w in (0, U64_MAX, I64_MAX, I64_MIN):
                assert (hv == np.uint64(w)).any()
            for form in FORMS:                                            # a hit key whose true aggregate is the form's identity
                assert ((self.vals[form] == np.uint64(IDENTITY[form])) & (self.counts > 0)).any(), form


def _host(a, dtype=np.int64):
    if hasattr(a, "cpu"):
        assert a.is_cuda and str(a.dtype) == "torch.int64", a.dtype
        return a.cpu().numpy()
    assert isinstance(a, np.ndarray) and a.dtype == dtype, (a.dtype, dtype)
    return a


def check_all_forms(fj, r, device, after=None):
    """group_join_min and group_join_max, unsigned and signed, without and with the counts - element for element; after(name, timings)"""
    bk, pk, pv = r.args(device)
    nb = r.bk.size
    note = (lambda fn: after(fn, fj.last_timings())) if after else (lambda fn: None)
    P0, _, counts0 = fj.group_join_count(bk, pk)
    assert P0 == r.P and np.array_equal(_host(counts0), r.counts)
    order = np.argsort(r.bk, kind="stable")
    same = r.bk[order][1:] == r.bk[order][:-1]
    for op, signed in FORMS:
        fn = fj.group_join_min if op == "min" else fj.group_join_max
        name = f"group_join_{op}(signed={signed})"
        want, ident = r.vals[(op, signed)], np.uint64(IDENTITY[(op, signed)])
        # the values alone; the sign from the container where the container has one (a NumPy uint64 / int64 column)
        if device:
            P, sec, vals = fn(bk, pk, pv, signed=None if signed else False)
            out_dtype = np.int64
        else:
            P, sec, vals = fn(bk, pk, pv.view(np.int64) if signed else pv)
            out_dtype = np.int64 if signed else np.uint64
        note(name)
        assert isinstance(P, int) and isinstance(sec, float)
        vals = _host(vals, out_dtype).view(np.uint64)
        assert vals.shape == (nb,) and np.array_equal(vals, want), name + ": values"
        assert P == r.P == P0, name + ": P is the sum of all counts, duplicated build keys included"
        # ... and with the counts; the sign forced
        P, _, vals, counts = fn(bk, pk, pv, return_counts=True, signed=signed)
        note(name + " with counts")
        vals, counts = _host(vals, np.int64 if signed or device else np.uint64).view(np.uint64), _host(counts)
        assert np.array_equal(vals, want) and np.array_equal(counts, r.counts), name + ": both outputs"
        assert P == r.P == int(counts.sum())
        assert np.all(vals[counts == 0] == ident), name + ": a row without a partner holds the identity"
        v = vals[order]
        assert np.all(v[1:][same] == v[:-1][same]), name + ": every copy of a duplicated build key holds the same value"


CASES = [   # id, nb, np, plan_target_keys, duplicates, passes
    ("nb0", 0, 1000, 4096, True, None),
    ("nb1", 1, 1000, 4096, True, None),
    ("np0", 1000, 0, 4096, True, None),
    ("zero_pass", 3000, 200_000, 4096, True, lambda p: p == 0),
    ("zero_pass_unique", 3000, 200_000, 4096, False, lambda p: p == 0),
    ("one_pass", 200_000, 1_000_000, 4096, True, lambda p: p == 1),
    ("deep", 60_000, 400_000, 32, True, lambda p: p >= 2),
]


@functools.lru_cache(maxsize=None)
def _ref_case(cid):
    _, nb, n_p, _, dups, _ = next(c for c in CASES if c[0] == cid)
    return Ref(*_case(nb, n_p, 0.5, seed=zlib.crc32(cid.encode()) % 1000, dups=dups))


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("cid", [c[0] for c in CASES])
def test_parity_with_the_numpy_reference(fj, cid, device):
    _, nb, n_p, target, dups, passes = next(c for c in CASES if c[0] == cid)
    r = _ref_case(cid)
    if nb >= 8:
        assert (np.unique(r.bk).size < r.bk.size) == dups
    if n_p and nb:
        r.check_data()
    if cid == "np0":
        assert all((r.vals[form] == np.uint64(IDENTITY[form])).all() for form in FORMS) and not r.counts.any()
    if cid == "one_pass":                                                 # the empty marker and the filler key on both sides, with partners
        for raw in (keymix.EMPTY_RAW, keymix.FILLER_RAW):
            assert (r.bk == raw).any() and (r.pk == raw).any()

    def after(fn, lt):
        if passes is not None:
            assert lt["path"] == 0 and lt["fell_back"] == 0 and passes(lt["passes"]) and lt["emit_ms"] == 0.0, (fn, lt)
    fj.set_option("plan_target_keys", target)
    try:
        check_all_forms(fj, r, device, after=after)
    finally:
        fj.set_option("plan_target_keys", 4096)


@functools.lru_cache(maxsize=1)
def _hot_key_case():
    rng = np.random.default_rng(11)
    bk = np.unique(rng.integers(0, 2**64, size=200_000, dtype=np.uint64))[:199_951]
    hot = bk[1234]
    bk = np.concatenate([bk, np.full(49, hot)])                        # one key with 50 copies
    rng.shuffle(bk)
    assert bk.size == 200_000
    pk = np.concatenate([np.full(200_000, hot), rng.choice(bk, 100_000), rng.integers(0, 2**64, size=300_000, dtype=np.uint64)])
    rng.shuffle(pk)
    return Ref(bk, pk, _plant(bk, pk, rng.integers(0, 2**64, size=pk.size, dtype=np.uint64)))


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_a_hot_key(fj, device):
    """one key has 50 copies on the build side and a third of the probe rows: its LDS accumulator takes them all, every copy reads it"""
    r = _hot_key_case()
    r.check_data()
    assert r.counts.max() >= 200_000 and (r.counts == r.counts.max()).sum() == 50

    def after(fn, lt):
        assert lt["path"] == 0 and lt["fell_back"] == 0, (fn, lt)
    check_all_forms(fj, r, device, after=after)


@pytest.mark.gpu
def test_the_same_call_twice_returns_the_same_arrays(fj):
    """accumulators and outputs are filled per call: a second call on the same context adds nothing to the first"""
    r = _ref_case("one_pass")
    for device in (False, True):
        for _ in range(2):
            check_all_forms(fj, r, device)


@pytest.mark.gpu
@pytest.mark.parametrize("base", [2, 1], ids=["partitioned", "hbm_table"])
@pytest.mark.parametrize("flag,form", [(MIN, ("min", True)), (MAX, ("max", True))], ids=["min_signed", "max_signed"])
def test_direct_call_defines_every_row_and_nothing_else(fj, base, flag, form):
    """fj_join_device on buffers pre-filled with 0xA5 and 64 guard words behind word nb, the signed forms (their identities are no
    memset pattern): every word below nb is defined by the call alone, the guards are intact, and no result is left pending."""
    import threading
    import torch
    from flash_hash_join_amd import _lib, api
    L = _lib.load()
    r = _ref_case("one_pass")
    bk, pk, pv = r.args(True)
    nb, n_p = r.bk.size, r.pk.size
    ctx = api.context(0)
    stream = torch.cuda.current_stream(0).cuda_stream
    A5 = int(np.array(0xA5A5A5A5A5A5A5A5, dtype=np.uint64).view(np.int64))
    oc = torch.full((nb + 64,), A5, dtype=torch.int64, device="cuda")
    ov = torch.full((nb + 64,), A5, dtype=torch.int64, device="cuda")
    ov_alone = torch.full((nb + 64,), A5, dtype=torch.int64, device="cuda")
    cnt, cnt_alone = ctypes.c_uint64(0), ctypes.c_uint64(0)
    t = _lib.FjTimings()
    if base == 1:
        fj.set_option("scalar_hbm_table", 1)
    try:
        with api._ctx_locks.setdefault(0, threading.RLock()):
            # a pending result first: the build-order call drops it
            _lib.check(L.fj_join_device(ctx, 2, 0, 1, bk.data_ptr(), bk.data_ptr(), nb, pk.data_ptr(), n_p, stream, 64, ctypes.byref(cnt), None, None, 0, None))
            _lib.check(L.fj_join_device(ctx, base | BO | flag | SIGNED, 0, 1, bk.data_ptr(), pv.data_ptr(), nb, pk.data_ptr(), n_p, stream, 64,
                                        ctypes.byref(cnt), oc.data_ptr(), ov.data_ptr(), nb, ctypes.byref(t)))
            assert L.fj_emit_pairs(ctx, oc.data_ptr(), oc.data_ptr(), nb, stream, None) != 0, "a result was left pending"
            _lib.check(L.fj_join_device(ctx, base | BO | flag | SIGNED, 0, 1, bk.data_ptr(), pv.data_ptr(), nb, pk.data_ptr(), n_p, stream, 64,
                                        ctypes.byref(cnt_alone), None, ov_alone.data_ptr(), nb + 64, None))     # (more capacity than rows: still nb words)
    finally:
        fj.set_option("scalar_hbm_table", 0)
    assert t.path == (0 if base == 2 else 1) and t.emit_ms == 0.0
    hc, hv, hva = oc.cpu().numpy(), ov.cpu().numpy().view(np.uint64), ov_alone.cpu().numpy().view(np.uint64)
    assert int(cnt.value) == r.P == int(cnt_alone.value)
    guard = np.uint64(0xA5A5A5A5A5A5A5A5)
    assert np.all(hc[nb:] == A5) and np.all(hv[nb:] == guard) and np.all(hva[nb:] == guard), "a word behind word nb was written"
    assert np.array_equal(hc[:nb], r.counts) and np.array_equal(hv[:nb], r.vals[form]) and np.array_equal(hva[:nb], r.vals[form])
    assert np.all(hv[:nb][r.counts == 0] == np.uint64(IDENTITY[form])) and (r.counts == 0).any()


@functools.lru_cache(maxsize=1)
def _oversized_case():
    cand = np.arange(1, 5_000_000, dtype=np.uint64)
    part = keymix.hash_w1(cand) >> np.uint32(23)                       # top 9 hash bits: the final partition of a 9-bit plan
    sel = []
    for p in range(140):
        c = cand[part == p][:8500]
        assert c.size == 8500
        sel.append(c)
    one = np.concatenate(sel)
    rng = np.random.default_rng(5)
    rng.shuffle(one)
    bk = np.concatenate([one, one[:2000], np.array([2**64 - 1, 2**64 - 1, 0], dtype=np.uint64)])
    pk = np.concatenate([bk[::3], bk[::7], np.arange(5_000_000, 5_500_000, dtype=np.uint64), np.full(5, 2**64 - 1, dtype=np.uint64)])
    return Ref(bk, pk, _plant(bk, pk, rng.integers(0, 2**64, size=pk.size, dtype=np.uint64)))


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_partitions_beyond_the_lds_table_fall_back_to_the_hbm_table(fj, device):
    """140 of the plan's 512 partitions hold 8500 distinct build keys each - beyond the 8192-slot table: the whole join runs again on
    the HBM table (fell_back == 1) with identity-filled accumulators, whatever the partitioned attempt left in the outputs"""
    r = _oversized_case()
    r.check_data()

    def after(fn, lt):
        assert lt["fell_back"] == 1 and lt["path"] == 1, (fn, lt)
        hbm_timings.check_hbm_form(lt, fn)
    check_all_forms(fj, r, device, after=after)


@pytest.mark.gpu
def test_scalar_hbm_table_path(fj):
    """hash_join's base value (FJ_ALGO_SCALAR) under scalar_hbm_table = 1: the global table from the start, every form"""
    from flash_hash_join_amd import api
    r = Ref(*_case(50_000, 300_000, 0.5, seed=7))
    r.check_data()
    bk, pk, pv = r.args(True)
    fj.set_option("scalar_hbm_table", 1)
    try:
        for op, signed in FORMS:
            S = api.ALGO_SCALAR | api.ALGO_BUILD_ORDER | (api.ALGO_AGG_MIN if op == "min" else api.ALGO_AGG_MAX) | (api.ALGO_AGG_SIGNED if signed else 0)
            for want_counts in (False, True):
                P, _, counts, vals = api.join_device(S, 0, 1, bk, pv, pk, want_counts=want_counts)
                assert fj.last_timings()["path"] == 1 and fj.last_timings()["fell_back"] == 0
                hbm_timings.check_hbm_form(fj.last_timings())
                assert P == r.P
                assert (counts is None) if not want_counts else np.array_equal(counts.cpu().numpy(), r.counts)
                assert np.array_equal(vals.cpu().numpy().view(np.uint64), r.vals[(op, signed)]), (op, signed, want_counts)
            P, _, counts, vals = api._group_host(S, r.bk, r.pk, r.pv, True)
            assert fj.last_timings()["path"] == 1
            hbm_timings.check_hbm_form(fj.last_timings())
            assert P == r.P and np.array_equal(counts, r.counts) and np.array_equal(vals.view(np.uint64), r.vals[(op, signed)])
    finally:
        fj.set_option("scalar_hbm_table", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_radix_threshold_sends_the_adaptive_base_to_the_hbm_table(fj, device):
    r = Ref(*_case(50_000, 300_000, 0.5, seed=8))
    r.check_data()

    def after(fn, lt):
        assert lt["path"] == 1 and lt["fell_back"] == 0, (fn, lt)
        hbm_timings.check_hbm_form(lt, fn)
    fj.set_option("radix_threshold", r.bk.size + 1)
    try:
        check_all_forms(fj, r, device, after=after)
    finally:
        fj.set_option("radix_threshold", 0)


@pytest.mark.gpu
def test_device_form_writes_into_fresh_buffers_whatever_they_held(fj):
    """the device-tensor form allocates with torch.empty: fill the allocator's cache with a non-zero pattern of the same size first"""
    import torch
    r = _ref_case("zero_pass")
    bk, pk, pv = r.args(True)
    for op, signed in FORMS:
        fn = fj.group_join_min if op == "min" else fj.group_join_max
        for _ in range(2):
            junk = [torch.full((r.bk.size,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda") for _ in range(4)]
            del junk
            P, _, vals, counts = fn(bk, pk, pv, return_counts=True, signed=signed)
            assert P == r.P and np.array_equal(counts.cpu().numpy(), r.counts)
            assert np.array_equal(vals.cpu().numpy().view(np.uint64), r.vals[(op, signed)]), (op, signed)
