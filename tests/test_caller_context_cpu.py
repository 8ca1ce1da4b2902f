"""How a caller hands work in - the table that tests/test_caller_context.py drives on an MI355X, and what needs no GPU about it.

CASES holds one row per public entry point that takes device tensors (and per form of an entry that takes another path through
api.py): the call, the names of its "real" inputs (made once per shape by data()), its NumPy reference, and which of its inputs are
keys and which are values.  The references are the ones the other test files use - oracle.np_join / np_inner_join, ref_probe_order /
ref_lookup (test_probe_order.py), ref_indices (test_row_ids.py), ref_group / ref_minmax (test_group_join.py, test_group_minmax.py),
ref_group_by (test_group_by.py), ref_group_by_agg, ref_group_by_arg, ref_merge, ref_group of test_prepared_group.py and group_ref /
join_ref / exact_values of test_float_aggregates.py.  Nothing is compared with the library itself.

Poison.  The GPU file fills every input buffer with valid data of the same shape and dtype that is NOT the real data and lets the
real data arrive late; a call that reads too early computes the reference of the poison, not a fault.  Build keys (and the keys of
a one-relation group-by) are the constant POISON_BUILD, probe keys the constant POISON_PROBE - neither occurs in the real data -
values, counts and planes are zero, `out=` / `counts_out=` accumulators hold POISON_ACC (float: POISON_FACC), which no real
accumulator holds.  Checked here, per row and shape, on the references alone:
  * all inputs poisoned: EVERY output the GPU test compares differs from the real one;
  * the half-poisoned mixes - real keys with poison values, poison keys with real values: each result differs from the real one in
    at least one output (real keys with poison values leave a key output as it is, so "every" cannot hold there), and every output
    that depends on a value input differs under the first mix, every output at all under the second.
An input the entry takes and never reads (the value column of a counting join) belongs to no mix.

Completeness.  Every name in api.REFERENCE_EXPORTS + api.EXTENSIONS, every form in FORMS (the Index methods with and without
out= / counts_out=, GroupByAccumulator.update / merge / result, the other paths of join_indices / left_join / full_join / unique) is
covered by a row or listed in EXCLUDED with its reason; every row covers something no other row covers, so removing a row fails."""
import functools

import numpy as np
import pytest

from oracle.oracle import np_inner_join, np_join
from test_float_aggregates import exact_values, group_ref, join_ref
from test_group_by import ref_group_by
from test_group_by_agg_cpu import ref_group_by_agg
from test_group_by_arg_cpu import ref_group_by_arg
from test_group_by_merge_cpu import ref_merge
from test_group_join import ref_group
from test_group_minmax import ref_minmax
from test_prepared_group import IDENT as INDEX_IDENT, ref_group as ref_index_group
from test_probe_order import ref_lookup, ref_probe_order
from test_row_ids import _pairs, ref_indices

POISON_BUILD = np.uint64(0x1111111111111111)
POISON_PROBE = np.uint64(0x2222222222222222)
POISON_ACC = np.uint64(0x3333333333333333)
POISON_FACC = -3.0e9
GUARD = np.uint64(0x5A5A5A5A5A5A5A5A)                 # what the bases of the view tests hold around the viewed elements
FILL = 2**64 - 3                                        # fill_value of the rows that take one (test_probe_order.py)

# the kind of every input name: "bkey" / "pkey" (keys), "val" (uint64 words), "fval" (float64), "acc" / "facc" (accumulators)
KIND = dict(bk="bkey", rel="bkey", k0="bkey", k1="bkey", k2="bkey", mk="bkey", pk="pkey",
            bv="val", pv="val", rv="val", v0="val", v1="val", v2="val", mc="val", ms="val", mn="val", mx="val",
            rf="fval", pf="fval", acc="acc", cacc="acc", facc="facc")
SHAPES = {   # name: build rows, distinct build keys, probe rows, rows of the one-relation group-bys (None: the build side itself)
    "one_pass": (60_000, 9_000, 200_003, None),
    "zero_pass": (300, 120, 2_000, 1_500),
}


class Data:
    """the real inputs of one shape, as NumPy arrays that nothing changes"""


@functools.lru_cache(maxsize=None)
def data(shape):
    nb, distinct, n_p, n_rel = SHAPES[shape]
    rng = np.random.default_rng(7000 + sorted(SHAPES).index(shape))
    words = lambda n: rng.integers(1, 2**64, size=n, dtype=np.uint64)                       # never zero: zero is the poison
    uk = np.unique(rng.integers(0, 2**63, size=distinct + 64, dtype=np.uint64) * np.uint64(2) + np.uint64(1))[:distinct]      # odd keys
    rng.shuffle(uk)
    d = Data()
    d.shape = shape
    d.bk = np.concatenate([uk, rng.choice(uk, nb - distinct)])                              # every key, most of them several times
    rng.shuffle(d.bk)
    d.bv = words(nb)
    hit = rng.random(n_p) < 0.30
    d.pk = np.where(hit, rng.choice(uk[:distinct * 8 // 9], n_p), rng.integers(0, 2**63, size=n_p, dtype=np.uint64) * np.uint64(2))
    d.pv, d.pf = words(n_p), exact_values(11, n_p)                                          # (a ninth of the build keys has no probe row; even keys never match)
    if n_rel is None:
        d.rel, d.rv = d.bk, d.bv
    else:
        gk = np.unique(rng.integers(0, 2**63, size=260, dtype=np.uint64) * np.uint64(2) + np.uint64(1))[:200]
        d.rel, d.rv = np.concatenate([gk, rng.choice(gk, n_rel - gk.size)]), words(n_rel)
        rng.shuffle(d.rel)
    n = d.rel.size
    d.rf = exact_values(12, n)
    # three batches for GroupByAccumulator: every batch leads with one row of every key seen so far, so that it holds at least as
    # many groups as the merged state and the policy of _take merges after each one (compact_at=1); cut a, b of the rows between them
    a, b = n // 6, n // 2
    d.k0, d.v0 = d.rel[:a], d.rv[:a]
    lead1, lead2 = np.unique(d.rel[:b]), np.unique(d.rel)
    d.k1, d.v1 = np.concatenate([lead1, d.rel[a:b]]), np.concatenate([words(lead1.size), d.rv[a:b]])
    d.k2, d.v2 = np.concatenate([lead2, d.rel[b:]]), np.concatenate([words(lead2.size), d.rv[b:]])
    # partial rows for group_by_merge: what group_by_agg (signed) returns for three pieces of the relation, by the reference
    parts = [ref_group_by_agg(d.rel[lo:hi], d.rv[lo:hi]) for lo, hi in ((0, a), (a, b), (b, n))]
    d.mk = np.concatenate([p["keys"] for p in parts])
    d.mc = np.concatenate([p["count"].view(np.uint64) for p in parts])
    d.ms = np.concatenate([p["sum"] for p in parts])
    d.mn = np.concatenate([p["min_s"].view(np.uint64) for p in parts])
    d.mx = np.concatenate([p["max_s"].view(np.uint64) for p in parts])
    # running aggregates of an Index over earlier batches: sums (words), counts, float sums
    d.acc, d.cacc, d.facc = words(nb), rng.integers(1, 1000, size=nb, dtype=np.uint64), exact_values(13, nb)
    for name in KIND:
        arr = getattr(d, name)
        arr.setflags(write=False)
        assert not np.isin(arr.view(np.uint64), [POISON_BUILD, POISON_PROBE, POISON_ACC, GUARD]).any(), name
        assert arr.dtype == (np.float64 if KIND[name] in ("fval", "facc") else np.uint64), name
    assert not (d.facc == POISON_FACC).any()
    return d


def poison(name, n):
    kind = KIND[name]
    if kind in ("bkey", "pkey", "acc"):
        return np.full(n, {"bkey": POISON_BUILD, "pkey": POISON_PROBE, "acc": POISON_ACC}[kind], dtype=np.uint64)
    if kind == "facc":
        return np.full(n, POISON_FACC)
    return np.zeros(n, dtype=np.float64 if kind == "fval" else np.uint64)


# ---- canonical forms: what a result is compared as, for the library's output and the reference alike ----------------------------------
def u64(x):
    return np.ascontiguousarray(np.asarray(x)).reshape(-1).view(np.uint64)


def i64(x):
    return np.ascontiguousarray(np.asarray(x)).reshape(-1).view(np.int64)


def pairs(k, v):
    """(key, value) pairs in the order of sort_pairs: by key, then value, as unsigned words"""
    k, v = u64(k), u64(v)
    o = np.lexsort((v, k))
    return k[o], v[o]


def by_key(gk, *cols):
    """group keys sorted, and the columns aligned with them in that order"""
    gk = u64(gk)
    o = np.argsort(gk, kind="stable")
    return (gk[o],) + tuple(np.asarray(c).reshape(-1)[o] for c in cols)


def codes_by_key(gk, codes):
    """group ids that index gk, as ids that index the sorted gk (np.unique's inverse)"""
    gk = u64(gk)
    rank = np.empty(gk.size, np.int64)
    rank[np.argsort(gk, kind="stable")] = np.arange(gk.size)
    return rank[i64(codes)] if gk.size else i64(codes)


class Row:
    """id; covers: the exports / forms this row stands for; args: names of its inputs (attributes of Data); call(fj, t, ix) with t the
    inputs by name where the caller put them and ix the prepared Index of `index=True` rows; canon(result, a) and ref(a, d): the named
    outputs of the library's result / of the NumPy reference on the inputs `a` (NumPy, flattened), compared with same(); unread: inputs
    the entry never reads; deep: also run under plan_target_keys = 16; after(fj, raw, put): a second step on the default stream, once
    the first one's stream is drained (build_index: probe the index); family: which kernel family the row reaches"""

    def __init__(self, id, covers, args, call, canon, ref, family, unread=(), deep=False, index=False, after=None):
        self.id, self.covers, self.args, self.call, self.canon, self.ref = id, tuple(covers), tuple(args), call, canon, ref
        self.family, self.unread, self.deep, self.index, self.after = family, tuple(unread), deep, index, after

    def keys(self):
        return [n for n in self.args if KIND[n] in ("bkey", "pkey")]

    def values(self):
        return [n for n in self.args if KIND[n] not in ("bkey", "pkey") and n not in self.unread]

    def accumulators(self):
        return [n for n in self.args if KIND[n] in ("acc", "facc")]

    def real(self, d):
        return {n: getattr(d, n) for n in self.args}

    def __repr__(self):
        return self.id


CASES = []


def row(*a, **kw):
    CASES.append(Row(*a, **kw))


def _unmatched(a):
    return a["pk"][~np.isin(a["pk"], a["bk"])]


def _rest(a):
    """the build rows whose key is not among the probe keys"""
    return np.flatnonzero(~np.isin(a["bk"], a["pk"]))


# -- the reference's twelve joins: six counting, six materialising -------------------------------------------------------------------------
def _count_join(name, oracle=np_join, unread=("bv",), args=("bk", "bv", "pk")):
    row(name, [name], args, lambda fj, t, ix: getattr(fj, name)(*(t[n] for n in args)),
        lambda r, a: {"n": int(r[0])}, lambda a, d: {"n": int(oracle(a["bk"], a["bk"], a["pk"]))},
        "count join", unread=unread, deep="bloom" in name)


def _pair_join(name, oracle=np_join):
    def canon(r, a):
        k, v = pairs(r[2], r[3])
        return {"n": int(r[0]), "keys": k, "values": v}

    def ref(a, d):
        n, k, v = oracle(a["bk"], a["bv"], a["pk"], return_arrays=True)
        k, v = pairs(k, v)
        return {"n": int(n), "keys": k, "values": v}
    row(name, [name], ("bk", "bv", "pk"), lambda fj, t, ix: getattr(fj, name)(t["bk"], t["bv"], t["pk"], return_arrays=True), canon, ref,
        "materialising join", deep="bloom" in name)


for _n in ("adaptive_join_count", "adaptive_join_count_bloom", "hash_join_count_radix", "hash_join_count", "hash_join_count_radix_bloom", "hash_join_count_bloom"):
    _count_join(_n)
for _n in ("adaptive_join", "adaptive_join_bloom", "hash_join_radix", "hash_join", "hash_join_radix_bloom", "hash_join_bloom"):
    _pair_join(_n)

# -- many-to-many, outer, anti, semi ------------------------------------------------------------------------------------------------------------
_count_join("inner_join_count", np_inner_join)
_pair_join("inner_join", np_inner_join)
_count_join("semi_join_count", unread=(), args=("bk", "pk"))
row("anti_join_count", ["anti_join_count"], ("bk", "pk"), lambda fj, t, ix: fj.anti_join_count(t["bk"], t["pk"]),
    lambda r, a: {"u": int(r[0])}, lambda a, d: {"u": int(_unmatched(a).size)}, "outer join")
row("anti_join", ["anti_join"], ("bk", "pk"), lambda fj, t, ix: fj.anti_join(t["bk"], t["pk"], return_arrays=True),
    lambda r, a: {"u": int(r[0]), "keys": np.sort(u64(r[2]))}, lambda a, d: {"u": int(_unmatched(a).size), "keys": np.sort(_unmatched(a))}, "outer join")
row("semi_join", ["semi_join"], ("bk", "pk"), lambda fj, t, ix: fj.semi_join(t["bk"], t["pk"], return_arrays=True),
    lambda r, a: {"s": int(r[0]), "keys": np.sort(u64(r[2]))},
    lambda a, d: {"s": int(np.isin(a["pk"], a["bk"]).sum()), "keys": np.sort(a["pk"][np.isin(a["pk"], a["bk"])])}, "materialising join")


def _outer_canon(names, full):
    """rows [0, P) pairs, then the unmatched probe keys with FILL, then (full) the r build rows without a partner; names: the counts
    in front of the seconds"""
    def canon(r, a):
        counts = len(names)
        c = [int(x) for x in r[:counts]]
        k, v = u64(r[counts + 1]), u64(r[counts + 2])
        P = c[0]
        end = k.size - (c[-1] if full else 0)
        out = dict(zip(names, c))
        out["pair_keys"], out["pair_values"] = pairs(k[:P], v[:P])
        out["unmatched_keys"], out["unmatched_values"] = np.sort(k[P:end]), v[P:end]
        if full:
            out["rest_keys"], out["rest_values"] = pairs(k[end:], v[end:])
        return out
    return canon


def _outer_ref(oracle, names, full):
    def ref(a, d):
        P, k, v = oracle(a["bk"], a["bv"], a["pk"], return_arrays=True)
        un, rest = _unmatched(a), _rest(a)
        out = dict(zip(names, [int(P)] + ([int(un.size)] if "u" in names else []) + ([int(rest.size)] if full else [])))
        out["pair_keys"], out["pair_values"] = pairs(k, v)
        out["unmatched_keys"], out["unmatched_values"] = np.sort(un), np.full(un.size, np.uint64(FILL))
        if full:
            out["rest_keys"], out["rest_values"] = pairs(a["bk"][rest], a["bv"][rest])
        return out
    return ref


_B3 = ("bk", "bv", "pk")
row("left_join", ["left_join"], _B3, lambda fj, t, ix: fj.left_join(t["bk"], t["bv"], t["pk"], return_arrays=True, fill_value=FILL),
    _outer_canon(("P",), False), _outer_ref(np_join, ("P",), False), "outer join")
row("left_join[all]", ["left_join[all]"], _B3, lambda fj, t, ix: fj.left_join(t["bk"], t["bv"], t["pk"], return_arrays=True, fill_value=FILL, duplicates="all"),
    _outer_canon(("P", "u"), False), _outer_ref(np_inner_join, ("P", "u"), False), "all-copies outer", deep=True)
row("full_join", ["full_join"], _B3, lambda fj, t, ix: fj.full_join(t["bk"], t["bv"], t["pk"], return_arrays=True, fill_value=FILL),
    _outer_canon(("P", "r"), True), _outer_ref(np_join, ("P", "r"), True), "outer join")
row("full_join[all]", ["full_join[all]"], _B3, lambda fj, t, ix: fj.full_join(t["bk"], t["bv"], t["pk"], return_arrays=True, fill_value=FILL, duplicates="all"),
    _outer_canon(("P", "u", "r"), True), _outer_ref(np_inner_join, ("P", "u", "r"), True), "all-copies outer")


# -- gather maps ------------------------------------------------------------------------------------------------------------------------------
def _indices(form, kw, counts, how, many, full):
    names = {1: ("n",), 2: ("n", "u") if not full else ("n", "r"), 3: ("n", "u", "r")}[counts]

    def canon(r, a):
        out = dict(zip(names, (int(x) for x in r[:counts])))
        out["pairs"] = np.stack(_pairs(r[counts + 1], r[counts + 2]))       # (probe row, build row), one output: a left join names every probe row whatever the keys are
        return out

    def ref(a, d):
        pi, bi = ref_indices(a["bk"], a["pk"], "anti" if how == "anti" else "inner", many)
        c = [pi.size]
        if how in ("left", "full"):
            miss = np.flatnonzero(~np.isin(a["pk"], a["bk"])).astype(np.int64)
            pi, bi = np.concatenate([pi, miss]), np.concatenate([bi, np.full(miss.size, -1, np.int64)])
            if many:
                c.append(miss.size)
        if full:
            rest = _rest(a).astype(np.int64)
            pi, bi = np.concatenate([pi, np.full(rest.size, -1, np.int64)]), np.concatenate([bi, rest])
            c.append(rest.size)
        out = dict(zip(names, (int(x) for x in c)))
        out["pairs"] = np.stack(_pairs(pi, None if form == "semi" else bi))      # (a semi join names probe rows only)
        return out
    row(f"join_indices[{form}]", [f"join_indices[{form}]"] + (["join_indices"] if form == "inner" else []), ("bk", "pk"),
        lambda fj, t, ix: fj.join_indices(t["bk"], t["pk"], **kw), canon, ref, "all-copies outer" if "all" in form else "materialising join")


_indices("inner", dict(how="inner"), 1, "inner", False, False)
_indices("left", dict(how="left"), 1, "left", False, False)
_indices("anti", dict(how="anti"), 1, "anti", False, False)
_indices("semi", dict(how="semi"), 1, "inner", False, False)
_indices("full", dict(how="full"), 2, "full", False, True)
_indices("many", dict(how="inner", many_to_many=True), 1, "inner", True, False)
_indices("left,all", dict(how="left", duplicates="all"), 2, "left", True, False)
_indices("full,all", dict(how="full", duplicates="all"), 3, "full", True, True)


# -- probe-order joins ----------------------------------------------------------------------------------------------------------------------
def _lookup_canon(r, a):
    return {"m": int(r[0]), "values": u64(r[2]), "mask": np.asarray(r[3]).reshape(-1).astype(bool)}


def _lookup_ref(bk, bv, pk):
    hit, idx, vals = ref_lookup(bk, bv, pk, FILL)
    return {"m": int(hit.sum()), "values": vals, "mask": hit}


row("lookup", ["lookup"], _B3, lambda fj, t, ix: fj.lookup(t["bk"], t["bv"], t["pk"], fill_value=FILL, return_mask=True),
    _lookup_canon, lambda a, d: _lookup_ref(a["bk"], a["bv"], a["pk"]), "probe-order")
row("isin", ["isin"], ("bk", "pk"), lambda fj, t, ix: fj.isin(t["pk"], t["bk"]),
    lambda r, a: {"m": int(r[0]), "mask": np.asarray(r[2]).reshape(-1).astype(bool)},
    lambda a, d: {"m": int(ref_probe_order(a["bk"], a["pk"])[0].sum()), "mask": ref_probe_order(a["bk"], a["pk"])[0]}, "probe-order")
row("lookup_indices", ["lookup_indices"], ("bk", "pk"), lambda fj, t, ix: fj.lookup_indices(t["bk"], t["pk"]),
    lambda r, a: {"m": int(r[0]), "build_idx": i64(r[2])},
    lambda a, d: {"m": int(ref_probe_order(a["bk"], a["pk"])[0].sum()), "build_idx": ref_probe_order(a["bk"], a["pk"])[1]}, "probe-order")

# -- build-order aggregate joins ---------------------------------------------------------------------------------------------------------------
row("group_join_count", ["group_join_count"], ("bk", "pk"), lambda fj, t, ix: fj.group_join_count(t["bk"], t["pk"]),
    lambda r, a: {"P": int(r[0]), "counts": i64(r[2])},
    lambda a, d: {"P": int(ref_group(a["bk"], a["pk"])[0].sum()), "counts": ref_group(a["bk"], a["pk"])[0]}, "build-order")
_G3 = ("bk", "pk", "pv")


def _group_join_ref(a, d):
    counts, sums = ref_group(a["bk"], a["pk"], a["pv"])
    return {"P": int(counts.sum()), "values": sums, "counts": counts}


row("group_join_sum", ["group_join_sum"], _G3, lambda fj, t, ix: fj.group_join_sum(t["bk"], t["pk"], t["pv"], return_counts=True),
    lambda r, a: {"P": int(r[0]), "values": u64(r[2]), "counts": i64(r[3])}, _group_join_ref, "build-order")
for _op in ("min", "max"):
    row(f"group_join_{_op}", [f"group_join_{_op}"], _G3,
        lambda fj, t, ix, _op=_op: getattr(fj, f"group_join_{_op}")(t["bk"], t["pk"], t["pv"], return_counts=True, signed=True),
        lambda r, a: {"P": int(r[0]), "values": u64(r[2]), "counts": i64(r[3])},
        lambda a, d, _op=_op: {"P": int(ref_group(a["bk"], a["pk"])[0].sum()), "values": ref_minmax(a["bk"], a["pk"], a["pv"], _op, True),
                               "counts": ref_group(a["bk"], a["pk"])[0]}, "build-order")


def _group_join_float_ref(a, d):
    out, cnt, P = join_ref(a["bk"], a["pk"], a["pf"], "sum", False)
    return {"P": int(cnt.sum()), "values": out, "counts": cnt}


row("group_join_sum[float64]", ["group_join_sum[float64]"], ("bk", "pk", "pf"),
    lambda fj, t, ix: fj.group_join_sum(t["bk"], t["pk"], t["pf"], return_counts=True, float64=True),
    lambda r, a: {"P": int(r[0]), "values": np.asarray(r[2]).reshape(-1), "counts": i64(r[3])}, _group_join_float_ref, "build-order")


# -- group-by on one relation -------------------------------------------------------------------------------------------------------------------
def _gb(a):
    return ref_group_by(a["rel"], a["rv"] if "rv" in a else np.zeros(a["rel"].size, np.uint64))


row("unique", ["unique"], ("rel",), lambda fj, t, ix: fj.unique(t["rel"]),
    lambda r, a: {"g": int(r[0]), "keys": np.sort(u64(r[2]))}, lambda a, d: {"g": int(_gb(a)["keys"].size), "keys": _gb(a)["keys"]}, "group-by")


def _unique_all_canon(r, a):
    gk, first, counts = by_key(r[2], r[3], r[5])
    return {"g": int(r[0]), "keys": gk, "first_index": i64(first), "inverse": codes_by_key(r[2], r[4]), "counts": i64(counts)}


def _unique_all_ref(a, d):
    uk, first, inv, cnt = np.unique(a["rel"], return_index=True, return_inverse=True, return_counts=True)
    return {"g": int(uk.size), "keys": uk, "first_index": first.astype(np.int64), "inverse": inv.reshape(-1).astype(np.int64), "counts": cnt.astype(np.int64)}


row("unique[index,inverse,counts]", ["unique[index,inverse,counts]"], ("rel",),
    lambda fj, t, ix: fj.unique(t["rel"], return_index=True, return_counts=True, return_inverse=True), _unique_all_canon, _unique_all_ref, "group-by")
row("distinct_count", ["distinct_count"], ("rel",), lambda fj, t, ix: fj.distinct_count(t["rel"]),
    lambda r, a: {"g": int(r[0])}, lambda a, d: {"g": int(np.unique(a["rel"]).size)}, "group-by")
row("group_by_count", ["group_by_count"], ("rel",), lambda fj, t, ix: fj.group_by_count(t["rel"]),
    lambda r, a: dict(zip(("keys", "counts"), by_key(r[2], i64(r[3]))), g=int(r[0])),
    lambda a, d: {"g": int(_gb(a)["keys"].size), "keys": _gb(a)["keys"], "counts": _gb(a)["count"]}, "group-by")
for _op, _col, _kw in (("sum", "sum", {}), ("min", "min_s", {"signed": True}), ("max", "max_s", {"signed": True})):
    row(f"group_by_{_op}", [f"group_by_{_op}"], ("rel", "rv"), lambda fj, t, ix, _op=_op, _kw=_kw: getattr(fj, f"group_by_{_op}")(t["rel"], t["rv"], **_kw),
        lambda r, a: dict(zip(("keys", "values"), by_key(r[2], u64(r[3]))), g=int(r[0])),
        lambda a, d, _col=_col: {"g": int(_gb(a)["keys"].size), "keys": _gb(a)["keys"], "values": u64(_gb(a)[_col])}, "group-by")
row("group_by_sum[float64]", ["group_by_sum[float64]"], ("rel", "rf"), lambda fj, t, ix: fj.group_by_sum(t["rel"], t["rf"], float64=True),
    lambda r, a: dict(zip(("keys", "values"), by_key(r[2], np.asarray(r[3]).reshape(-1))), g=int(r[0])),
    lambda a, d: dict(zip(("keys", "values"), group_ref(a["rel"], a["rf"], "sum")[:2]), g=int(np.unique(a["rel"]).size)), "group-by")
row("factorize", ["factorize"], ("rel",), lambda fj, t, ix: fj.factorize(t["rel"]),
    lambda r, a: {"g": int(r[0]), "uniques": np.sort(u64(r[3])), "codes": codes_by_key(r[3], r[2])},
    lambda a, d: dict(zip(("uniques", "codes"), np.unique(a["rel"], return_inverse=True)), g=int(np.unique(a["rel"]).size)), "factorize")


def _agg_canon(r, a):
    gk, c, s, mn, mx = by_key(r[2], i64(r[3]), u64(r[4]), u64(r[5]), u64(r[6]))
    return {"g": int(r[0]), "keys": gk, "count": c, "sum": s, "min": mn, "max": mx}


def _agg_ref(keys, vals):
    e = ref_group_by_agg(keys, vals)
    return {"g": int(e["keys"].size), "keys": e["keys"], "count": e["count"], "sum": e["sum"], "min": u64(e["min_s"]), "max": u64(e["max_s"])}


def _merge_ref(keys, counts, sums, mins, maxs):
    e = ref_merge(keys, counts, sums, mins, maxs, "signed")
    return {"g": int(e["keys"].size), "keys": e["keys"], "count": i64(e["count"]), "sum": e["sum"], "min": e["min"], "max": e["max"]}


row("group_by_agg", ["group_by_agg"], ("rel", "rv"), lambda fj, t, ix: fj.group_by_agg(t["rel"], t["rv"], signed=True),
    _agg_canon, lambda a, d: _agg_ref(a["rel"], a["rv"]), "group_by_agg", deep=True)
for _op in ("argmin", "argmax"):
    row(f"group_by_{_op}", [f"group_by_{_op}"], ("rel", "rv"),
        lambda fj, t, ix, _op=_op: getattr(fj, f"group_by_{_op}")(t["rel"], t["rv"], signed=True, return_values=True),
        lambda r, a: dict(zip(("keys", "index", "value"), by_key(r[2], i64(r[3]), u64(r[4]))), g=int(r[0])),
        lambda a, d, _op=_op: dict(ref_group_by_arg(a["rel"], a["rv"], "signed", _op == "argmax"), g=int(np.unique(a["rel"]).size)),
        "argmin", deep=_op == "argmin")
_M5 = ("mk", "mc", "ms", "mn", "mx")
row("group_by_merge", ["group_by_merge"], _M5, lambda fj, t, ix: fj.group_by_merge(*(t[n] for n in _M5), signed=True),
    _agg_canon, lambda a, d: _merge_ref(*(a[n] for n in _M5)), "merge", deep=True)


def _accumulate(fj, t, ix):
    with fj.group_by_accumulator(signed=True, compact_at=1) as acc:
        for i in range(3):
            acc.update(t[f"k{i}"], t[f"v{i}"])
            assert acc.pending_rows == 0 and acc.merges == i + 1, (i, acc.pending_rows, acc.merges)      # a merge after every batch
        return acc.result()


def _accumulate_merge(fj, t, ix):
    with fj.GroupByAccumulator(signed=True, compact_at=1) as acc:
        acc.update(t["k0"], t["v0"])
        acc.merge(tuple(t[n] for n in _M5))
        return acc.result()


def _accumulate_merge_ref(a, d):
    e = ref_group_by_agg(a["k0"], a["v0"])
    cat = lambda x, y: np.concatenate([u64(x), u64(y)])
    return _merge_ref(cat(e["keys"], a["mk"]), cat(e["count"], a["mc"]), cat(e["sum"], a["ms"]), cat(e["min_s"], a["mn"]), cat(e["max_s"], a["mx"]))


row("GroupByAccumulator", ["GroupByAccumulator", "group_by_accumulator", "GroupByAccumulator.update", "GroupByAccumulator.result"],
    ("k0", "v0", "k1", "v1", "k2", "v2"), _accumulate, _agg_canon,
    lambda a, d: _agg_ref(np.concatenate([a["k0"], a["k1"], a["k2"]]), np.concatenate([a["v0"], a["v1"], a["v2"]])), "merge")
row("GroupByAccumulator.merge", ["GroupByAccumulator.merge"], ("k0", "v0") + _M5, _accumulate_merge, _agg_canon, _accumulate_merge_ref, "merge")


# -- a prepared build side: built late, and probed late -------------------------------------------------------------------------------------------
def _probe_the_late_index(fj, index, put):
    with index:
        return index.lookup(put("pk"), fill_value=FILL, return_mask=True)


row("build_index", ["build_index"], ("bk", "bv"), lambda fj, t, ix: fj.build_index(t["bk"], t["bv"]), _lookup_canon,
    lambda a, d: _lookup_ref(a["bk"], a["bv"], d.pk), "prepared index", after=_probe_the_late_index)
row("Index.lookup", ["Index.lookup"], ("pk",), lambda fj, t, ix: ix.lookup(t["pk"], fill_value=FILL, return_mask=True), _lookup_canon,
    lambda a, d: _lookup_ref(d.bk, d.bv, a["pk"]), "prepared index", index=True)
row("Index.isin", ["Index.isin"], ("pk",), lambda fj, t, ix: ix.isin(t["pk"]),
    lambda r, a: {"m": int(r[0]), "mask": np.asarray(r[2]).reshape(-1).astype(bool)},
    lambda a, d: {"m": int(ref_probe_order(d.bk, a["pk"])[0].sum()), "mask": ref_probe_order(d.bk, a["pk"])[0]}, "prepared index", index=True)
row("Index.lookup_indices", ["Index.lookup_indices"], ("pk",), lambda fj, t, ix: ix.lookup_indices(t["pk"]),
    lambda r, a: {"m": int(r[0]), "build_idx": i64(r[2])},
    lambda a, d: {"m": int(ref_probe_order(d.bk, a["pk"])[0].sum()), "build_idx": ref_probe_order(d.bk, a["pk"])[1]}, "prepared index", index=True)


def _index_group(form, out):
    """Index.group_<form>, without accumulators (fresh outputs, the identity where a build row has no partner) or with them"""
    op = form.split("_")[0]
    ref_form = {"count": "count", "sum": "sum", "min": "min_s", "max": "max_s"}[op]
    args = ("pk",) + (("pv",) if op != "count" else ()) + ((("acc",) if op != "count" else ()) + ("cacc",) if out else ())

    def call(fj, t, ix):
        if op == "count":
            return ix.group_count(t["pk"], out=t["cacc"] if out else None)
        kw = dict(out=t["acc"], counts_out=t["cacc"]) if out else dict(return_counts=True)
        if op != "sum":
            kw["signed"] = True
        return getattr(ix, "group_" + op)(t["pk"], t["pv"], **kw)

    def canon(r, a):
        if op == "count":
            return {"m": int(r[0]), "counts": u64(r[2])}
        return {"m": int(r[0]), "values": u64(r[2]), "counts": u64(r[3])}

    def ref(a, d):
        hit, idx = ref_probe_order(d.bk, a["pk"])
        e = {"m": int(hit.sum()), "counts": ref_index_group("count", d.bk.size, idx[hit], None, a["cacc"] if out else None)}
        if op != "count":
            e["values"] = ref_index_group(ref_form, d.bk.size, idx[hit], a["pv"][hit], a["acc"] if out else None)
        return e
    name = f"Index.group_{op}" + ("[out]" if out else "")
    row(name, [name], args, call, canon, ref, "prepared index", index=True)


for _op in ("count", "sum", "min", "max"):
    _index_group(_op, False)
    _index_group(_op, True)


def _index_float_ref(a, d):
    hit, idx = ref_probe_order(d.bk, a["pk"])
    out = a["facc"].copy()
    np.add.at(out, idx[hit], a["pf"][hit])                                 # exact in any order: multiples of 2^-10 (test_float_aggregates.py)
    return {"m": int(hit.sum()), "values": out, "counts": ref_index_group("count", d.bk.size, idx[hit], None, a["cacc"])}


row("Index.group_sum[float64,out]", ["Index.group_sum[float64,out]"], ("pk", "pf", "facc", "cacc"),
    lambda fj, t, ix: ix.group_sum(t["pk"], t["pf"], out=t["facc"], counts_out=t["cacc"], float64=True),
    lambda r, a: {"m": int(r[0]), "values": np.asarray(r[2]).reshape(-1), "counts": u64(r[3])}, _index_float_ref, "prepared index", index=True)

BY_ID = {r.id: r for r in CASES}
EXCLUDED = {
    "initialize": "takes no tensor argument",
}
FORMS = (   # beyond the exported names: every form that takes a path of its own through api.py
    ["Index.lookup", "Index.isin", "Index.lookup_indices"]
    + [f"Index.group_{op}{out}" for op in ("count", "sum", "min", "max") for out in ("", "[out]")]
    + ["GroupByAccumulator.update", "GroupByAccumulator.merge", "GroupByAccumulator.result"]
    + ["left_join[all]", "full_join[all]", "unique[index,inverse,counts]"]
    + [f"join_indices[{f}]" for f in ("inner", "left", "anti", "semi", "full", "many", "left,all", "full,all")]
    + ["group_by_sum[float64]", "group_join_sum[float64]", "Index.group_sum[float64,out]"])
# the marked subset that also runs under plan_target_keys = 16: two-pass plans, the bloom precheck, the retry paths
DEEP = [r.id for r in CASES if r.deep]
# one row per kernel family and a few more: what runs on a second device, and - the first of each family - through the NumPy entry
REPRESENTATIVE = ["hash_join_count_radix", "adaptive_join_count_bloom", "adaptive_join", "hash_join_radix_bloom", "inner_join", "left_join",
                  "left_join[all]", "full_join[all]", "join_indices[left]", "lookup", "isin", "group_join_sum", "group_join_min",
                  "group_by_sum", "unique[index,inverse,counts]", "group_by_agg", "group_by_argmin", "group_by_merge", "GroupByAccumulator",
                  "factorize", "build_index", "Index.lookup", "Index.group_sum[out]"]
FAMILIES = ("count join", "materialising join", "all-copies outer", "probe-order", "build-order", "group_by_agg", "argmin", "merge", "factorize",
            "prepared index")


def same(got, ref):
    """exact equality of one output: an int, or an array of one shape and dtype kind (floats: ==, the exact domain needs no tolerance)"""
    if isinstance(ref, (int, np.integer)):
        return isinstance(got, (int, np.integer)) and int(got) == int(ref)
    got, ref = np.asarray(got), np.asarray(ref)
    return got.shape == ref.shape and got.dtype.kind == ref.dtype.kind and bool(np.array_equal(got, ref))


@functools.lru_cache(maxsize=None)
def expected(row_id, shape):
    """the reference of a row on the real inputs of a shape: computed once, shared, never changed"""
    r, d = BY_ID[row_id], data(shape)
    return r.ref(r.real(d), d)


def mixes(r, d):
    """name -> inputs: everything poisoned; real keys with poison values; poison keys with real values (where the row has both)"""
    real = r.real(d)
    p = {n: poison(n, real[n].size) for n in r.args}
    out = {"all poison": p}
    if r.keys() and r.values():
        out["real keys, poison values"] = {n: (real[n] if n in r.keys() or n in r.unread else p[n]) for n in r.args}
        out["poison keys, real values"] = {n: (p[n] if n in r.keys() else real[n]) for n in r.args}
    return out


# ---- the tests ------------------------------------------------------------------------------------------------------------------------------
def test_every_export_is_covered_or_excluded_with_a_reason():
    from flash_hash_join_amd import api
    required = list(api.REFERENCE_EXPORTS) + list(api.EXTENSIONS) + FORMS
    covered = {c for r in CASES for c in r.covers}
    missing = [n for n in required if n not in covered and n not in EXCLUDED]
    assert not missing, f"neither covered by a row of CASES nor listed in EXCLUDED: {missing}"
    assert all(isinstance(v, str) and v and "\n" not in v for v in EXCLUDED.values())
    assert not [n for n in EXCLUDED if n in covered], "excluded and covered at once"
    stale = [n for n in list(covered) + list(EXCLUDED) if n not in required]
    assert not stale, f"names that are no export and no listed form: {stale}"
    for n in api.REFERENCE_EXPORTS + api.EXTENSIONS:
        assert hasattr(api, n), n


def test_every_row_covers_something_of_its_own():
    """so that removing any row from CASES fails the completeness test"""
    assert len(BY_ID) == len(CASES)
    for r in CASES:
        others = {c for o in CASES if o is not r for c in o.covers}
        assert [c for c in r.covers if c not in others], f"row {r.id} covers nothing that another row does not"


def test_a_removed_row_and_a_new_export_fail_the_completeness_test(monkeypatch):
    from flash_hash_join_amd import api
    test_every_export_is_covered_or_excluded_with_a_reason()
    monkeypatch.setattr(api, "EXTENSIONS", api.EXTENSIONS + ["a_join_nobody_listed"])
    with pytest.raises(AssertionError, match="a_join_nobody_listed"):
        test_every_export_is_covered_or_excluded_with_a_reason()
    monkeypatch.undo()
    for i in (0, len(CASES) // 2, len(CASES) - 1):
        gone = CASES.pop(i)
        try:
            with pytest.raises(AssertionError, match="neither covered"):
                test_every_export_is_covered_or_excluded_with_a_reason()
        finally:
            CASES.insert(i, gone)


def test_the_subsets_name_rows_and_reach_every_family():
    assert set(DEEP) >= {"adaptive_join_bloom", "adaptive_join_count_bloom", "hash_join_radix_bloom", "hash_join_bloom", "hash_join_count_radix_bloom",
                         "hash_join_count_bloom", "left_join[all]", "group_by_agg", "group_by_argmin", "group_by_merge"}
    assert all(n in BY_ID for n in REPRESENTATIVE) and len(set(REPRESENTATIVE)) == len(REPRESENTATIVE)
    assert {BY_ID[n].family for n in REPRESENTATIVE} >= set(FAMILIES)
    assert 3 * len(REPRESENTATIVE) >= len(CASES)                          # a third of the table


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_the_shapes_are_what_the_gpu_file_says(shape):
    nb, distinct, n_p, n_rel = SHAPES[shape]
    d = data(shape)
    assert d.bk.size == d.bv.size == nb and np.unique(d.bk).size == distinct and d.pk.size == d.pv.size == n_p
    assert 0.25 < np.isin(d.pk, d.bk).mean() < 0.35 and (~np.isin(d.bk, d.pk)).any()
    assert d.rel.size == (n_rel or nb) and d.k0.size + d.k1.size + d.k2.size > d.rel.size
    # the batches of the accumulator: each holds every key of the ones before it
    assert np.isin(d.k0, d.k1).all() and np.isin(d.k1, d.k2).all()


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("r", CASES, ids=lambda r: r.id)
def test_poison_shows_in_the_reference(r, shape):
    d = data(shape)
    exp = expected(r.id, shape)
    assert exp and all(KIND[n] for n in r.args) and not set(r.unread) - set(r.args)
    results = {name: r.ref(a, d) for name, a in mixes(r, d).items()}
    for name, got in results.items():
        assert got.keys() == exp.keys()
        differ = [k for k in exp if not same(got[k], exp[k])]
        assert differ, f"{r.id} / {shape}: the reference on '{name}' equals the reference on the real inputs"
        if name == "all poison":
            assert differ == list(exp), f"{r.id} / {shape}: outputs that all-poison inputs leave as they are: {[k for k in exp if k not in differ]}"
    if len(results) == 3:
        caught = {k for name in ("real keys, poison values", "poison keys, real values") for k in exp if not same(results[name][k], exp[k])}
        assert caught == set(exp), f"{r.id} / {shape}: outputs that no half-poisoned mix changes: {set(exp) - caught}"
    # the canonical form of the reference's own outputs is itself (canon and ref speak of the same names)
    assert all(same(exp[k], exp[k]) for k in exp)


def test_poison_is_valid_data_of_the_same_shape_and_dtype():
    d = data("zero_pass")
    for name in KIND:
        real, p = getattr(d, name), poison(name, getattr(d, name).size)
        assert p.shape == real.shape and p.dtype == real.dtype and not np.array_equal(p, real), name
        assert np.unique(p).size == 1, name
        if KIND[name] not in ("val", "fval"):                              # a constant that the real data never holds
            assert not np.isin(p.view(np.uint64)[:1], real.view(np.uint64)).any(), name
    assert POISON_BUILD != POISON_PROBE
