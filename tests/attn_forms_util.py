"""One table of launch forms for the cached-attention kernels, shared by tests/test_attn_forms_host.py (CPU) and
tests/test_gpu_attn_forms.py (GPU).

launch_bfp_attention_decode dispatches decode_scores_kernel / decode_pv_kernel<DC, RG, GQ, PG, WN> and launch_bfp_attention_extend
dispatches bfp_attention_extend_kernel<DC, GQ, PG, WN>: DC = D / 32 chunks of the head dim, RG ragged lengths, GQ grouped queries,
PG paged cache, WN sliding window.  CASES holds at least one small case for every form either launcher can dispatch, `form_of`
says which form a call launches, and the predicates below say -- as pure functions of a case's numbers -- that the case puts
each of its switches to work.  Oracle, inputs and bounds are tests/window_util.py's, the paged caches tests/paged_util.py's.

Page size: P = 32 throughout.  A page is then exactly one V pair (two K tiles), so every edge of a decode split -- a multiple of
32 keys from the row's first pair -- is a page edge.  A split edge OFF a page edge needs P >= 64: the non-window paged decode forms
carry a second case at P = 64 whose splits = 2 edge is key 96, inside page 1."""
import functools
import math
import sys
from dataclasses import dataclass
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import paged_util  # noqa: E402
from window_util import DEV, bits, check, i32, inputs, oracle, par  # noqa: E402,F401

WIDTHS = (4, 6, 9)
TAIL = 10                       # the keys of the second append: the first piece ends inside a tile, which the second re-quantises
T, F = True, False
# (RG, GQ, PG, WN) of the decode launcher, (GQ, PG, WN) of the extend launcher, in the order the width rotation counts them
DECODE_SWITCHES = ((F, F, F, F), (F, T, F, F), (T, F, F, F), (T, T, F, F), (T, F, T, F), (T, T, T, F),
                   (T, F, F, T), (T, T, F, T), (T, F, T, T), (T, T, T, T))
EXTEND_SWITCHES = ((F, F, F), (T, F, F), (F, T, F), (T, T, F), (F, F, T), (T, F, T), (F, T, T), (T, T, T))


@dataclass(frozen=True)
class Case:
    kind: str                   # "decode" | "extend"
    D: int
    width: int
    ragged: bool                # the call brings lengths= (three cache rows); else every row holds lengths[0] keys (cache.length)
    group: int
    paged: bool
    window: object              # W or None
    M: int
    lengths: tuple              # per cache row, the queries' own keys included
    counts: object = None       # extend, ragged: queries per cache row
    causal: bool = True         # True: scale_div = sqrt(D); False: q_scale = D ** -0.5
    splits: tuple = ()          # decode: every value the case runs at (None: the default)
    P: int = 32
    note: str = ""

    @property
    def form(self):
        return form_of(self.kind, self.D, self.lengths if self.ragged else None, self.group, self.paged, self.window)

    @property
    def id(self):
        return "%s<%s>%s" % (self.kind, ",".join(str(x).lower() for x in self.form), self.note and "-" + self.note)

    @property
    def B(self):
        return len(self.lengths)

    @property
    def L(self):
        return max(self.lengths)

    @property
    def capacity(self):
        return -(-self.L // self.P) * self.P if self.paged else -(-self.L // 64) * 64

    def queries(self, b):
        """queries of cache row b that have an output (0: an empty slot, zeros)"""
        c = self.M if self.counts is None else self.counts[b]
        return 0 if c > self.lengths[b] else c

    @property
    def scaling(self):
        return dict(causal=True, scale_div=math.sqrt(self.D)) if self.causal else dict(causal=False, q_scale=float(np.float32(self.D ** -0.5)))


def form_of(kind, D, lengths, group, paged, window):
    """the template arguments a call of ops.bfp_attention_decode / ops.bfp_attention_extend launches: (DC, RG, GQ, PG, WN) /
    (DC, GQ, PG, WN).  ops.py passes group == 1 as G = 0 (the GQ = false kernels); the windowed kernels exist in the ragged form only, so
    a uniform windowed call has Python supply the lengths (ops._window_lengths) and launches RG = true; a paged cache without lengths is
    refused before any launch"""
    if D % 32 or not 32 <= D <= 128:
        raise ValueError(f"head dim {D}")
    if paged and lengths is None:
        raise ValueError("no uniform paged launch")
    dc, gq, pg, wn = D // 32, group != 1, bool(paged), window is not None
    if kind == "decode":
        return (dc, lengths is not None or wn, gq, pg, wn)
    if kind == "extend":
        return (dc, gq, pg, wn)
    raise ValueError(kind)


# ---- the launchers' host arithmetic, restated (tests/test_attn_forms_host.py holds each against the library's export) ------------
def group_width(G, M):
    return max(d for d in range(1, G + 1) if G % d == 0 and d * M <= 16)


def window_span(M, L, W):
    return W + M - 1 + 31 if W is not None and W < L and W + M - 1 + 31 < L else L


def splits_of(rows, span, override):
    NP = -(-span // 32)
    want = override or -(-512 // rows)
    if not override:
        want = min(want, NP // 2)
    want = max(min(want, 64, NP), 1)
    pps = -(-NP // want)
    return -(-NP // pps), pps


def launch_rows(c):
    return c.B * (c.group // group_width(c.group, c.M) if c.group > 1 else 1)


def partition(c, splits):
    """(S, key pairs per split) of decode case c at `splits`"""
    return splits_of(launch_rows(c), window_span(c.M, c.L, c.window), splits)


# ---- predicates: a case that carries a switch must put it to work --------------------------------------------------------------
def rg_ok(c):
    """three cache rows: one at max_length, one strictly shorter and non-empty that ends inside a 16-key tile, one empty slot"""
    if len(c.lengths) != 3 or c.lengths[0] != c.L:
        return False
    short_ok = c.queries(1) > 0 and c.lengths[1] < c.L and c.lengths[1] % 16 != 0
    empty_ok = c.lengths[2] < c.M if c.kind == "decode" else c.counts is not None and c.counts[2] == 0
    return short_ok and empty_ok and c.queries(0) > 0 and c.queries(2) == 0


def gq_ok(c):
    """decode: more than one head a launch row AND more than one launch row a cache row; extend: G = 2"""
    if c.kind == "extend":
        return c.group == 2
    gw = group_width(c.group, c.M)
    return gw > 1 and c.group // gw > 1


def pg_ok(c):
    """P = 32 (or the P = 64 second case), a row of at least three pages; decode: every explicit split edge lies inside the longest row,
    all of them on page edges at P = 32, some on and some off at P = 64"""
    if c.P not in (32, 64) or -(-c.L // c.P) < 3:
        return False
    if c.kind == "extend":
        return True
    edges = [e for s in c.splits if s and s > 1 for e in split_edges(c, s)]
    on = [e % c.P == 0 for e in edges]
    return bool(edges) and all(0 < e < c.L for e in edges) and (all(on) if c.P == 32 else any(on) and not all(on))


def split_edges(c, splits):
    """the first key of every split but the first, for the longest row"""
    S, pps = partition(c, splits)
    p0 = max(c.L - c.M - c.window + 1, 0) // 32 if c.window else 0
    return [32 * (p0 + pps * s) for s in range(1, S)]


def wn_decode_ok(c):
    """the first query's lower edge lo > 0 lies in the second tile of a key pair (tile 2 p0 is skipped); with M > 1 some explicit split
    count gives one pair a split, and then the last column sees no key of the first split"""
    lo = c.L - c.M - c.window + 1
    if lo <= 0 or lo % 32 < 16:
        return False
    if c.M == 1:
        return True
    one_pair = [s for s in c.splits if s and partition(c, s) == (s, 1) and s > 1]
    last_lo = c.L - 1 - c.window + 1                       # the last column's first visible key
    return bool(one_pair) and last_lo >= 32 * (lo // 32 + 1)


def wn_extend_ok(c):
    """row 0: two query blocks behind about 30 past keys; the second block's walk starts at an odd 32-key step; the last block's tile
    count `need` is odd"""
    n, m = c.lengths[0], c.queries(0)
    st0 = max(n - m + 64 - c.window + 1, 0) >> 5
    need = (n - m + min(127, m - 1)) // 16 + 1
    return 64 < m <= 128 and 24 <= n - m <= 36 and st0 % 2 == 1 and need % 2 == 1


def plain_decode_ok(c):
    """a non-window decode: at least 65 keys, run at two splits and at the default, and not every run has the same number of splits"""
    return c.L >= 65 and 2 in c.splits and None in c.splits and partition(c, 2)[0] == 2 and len({partition(c, s)[0] for s in c.splits}) > 1


def fill_ok(c):
    """the two-piece fill re-quantises an open K tile: every row longer than TAIL keys has a first piece that ends inside a tile"""
    return all((n - TAIL) % 16 != 0 for n in c.lengths if n > TAIL) and any(n > TAIL for n in c.lengths)


def scaling_ok(c):
    return c.causal or c.window is None


# ---- the table ----------------------------------------------------------------------------------------------------------------
def _width(dc, i):
    return WIDTHS[(dc + i) % 3]


def _decode_cases():
    out = []
    for dc in (1, 2, 3, 4):
        D = 32 * dc
        for i, (rg, gq, pg, wn) in enumerate(DECODE_SWITCHES):
            G, M = ((6, 4) if dc == 3 else (4, 7)) if gq else (1, 7)
            L, W = (117, 20) if wn else (75, None)
            lengths = (L, 70 if wn else 41, min(3, M - 1)) if rg else (L, L)
            base = dict(kind="decode", D=D, width=_width(dc, i), ragged=rg, group=G, paged=pg, window=W, M=M, lengths=lengths, splits=(2, None))
            out.append(Case(**base))
            if pg and gq and not wn:
                out.append(Case(**dict(base, causal=False, width=_width(dc, i + 1), note="noncausal")))
            if pg and not wn:
                out.append(Case(**dict(base, lengths=(131,) + lengths[1:], P=64, splits=(2, 5, None), width=_width(dc, i + 2), note="p64")))
    return out


def _extend_cases():
    out = []
    for dc in (1, 2, 3, 4):
        D = 32 * dc
        for i, (gq, pg, wn) in enumerate(EXTEND_SWITCHES):
            base = dict(kind="extend", D=D, width=_width(dc, i), ragged=True, group=2 if gq else 1, paged=pg, window=33 if wn else None,
                        M=70, lengths=(100, 57, 40), counts=(70, 33, 0))
            out.append(Case(**base))
            if pg and gq and not wn:
                out.append(Case(**dict(base, causal=False, width=_width(dc, i + 1), note="noncausal")))
    return out


CASES = _decode_cases() + _extend_cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
ALL_ON = [c for c in CASES if all(c.form[1:]) and not c.note]         # every switch on, DC = 1 .. 4: the stale-LDS screen's cases


def forms(kind):
    return {c.form for c in CASES if c.kind == kind}


# ---- inputs and the oracle, once a case ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def arrays(c):
    """q [B * G, M, D], k, v [B, L, D] (window_util.inputs; read-only)"""
    seed = sum(ord(ch) for ch in c.id)
    q, k, v = inputs(c.B * c.group, c.M, c.L, c.D, seed)
    k, v = k[:c.B], v[:c.B]
    for a in (q, k, v):
        a.setflags(write=False)
    return q, k, v


def _all_keys(q, k, v, width):
    """non-causal: every query sees every key -- window_util.oracle with one query a batch entry (its causal mask then hides nothing)"""
    B, M, D = q.shape
    out = oracle(q.reshape(B * M, 1, D), np.repeat(k, M, 0), np.repeat(v, M, 0), width, None, 1.0)
    return out.reshape(B, M, D)


@functools.lru_cache(maxsize=None)
def reference(c):
    """per cache row b: the fp64-softmax oracle of its G query rows' real queries on ITS keys, [G, queries(b), D] -- None for an empty
    slot"""
    q, k, v = arrays(c)
    refs = []
    for b, n in enumerate(c.lengths):
        m = c.queries(b)
        if m == 0:
            refs.append(None)
            continue
        qb = q[b * c.group:(b + 1) * c.group, :m]
        kb, vb = np.repeat(k[b:b + 1, :n], c.group, 0), np.repeat(v[b:b + 1, :n], c.group, 0)
        if c.causal:
            ref = oracle(qb, kb, vb, c.width, c.window, math.sqrt(c.D))
        else:
            ref = _all_keys((qb * np.float32(c.D ** -0.5)).astype(np.float32), kb, vb, c.width)
        ref.setflags(write=False)
        refs.append(ref)
    return tuple(refs)


# ---- GPU side ------------------------------------------------------------------------------------------------------------------------
def fill(c, k, v, lengths, paged=None):
    """a cache of len(lengths) rows, row b holding k[b, :lengths[b]], filled in two appends (all but the last TAIL keys, then those):
    paged -> a PagedKVCache of page size c.P with paged_util's out-of-order tables, else a KVCache; uniform when the case is"""
    import torch
    from mi355q import ops
    paged = c.paged if paged is None else paged
    B = len(lengths)
    first = [max(n - TAIL, 0) for n in lengths]
    kt, vt = torch.from_numpy(np.array(k)).to(DEV), torch.from_numpy(np.array(v)).to(DEV)
    if not c.ragged and not paged:
        cache = ops.KVCache(B, c.capacity, c.D, par(c.width), par(c.width), DEV)
        cache.append(kt[:, :first[0]].contiguous(), vt[:, :first[0]].contiguous())
        cache.append(kt[:, first[0]:lengths[0]].contiguous(), vt[:, first[0]:lengths[0]].contiguous())
        return cache
    plan = None
    if paged:
        cache, plan = paged_util.make_paged(B, c.D, c.P, c.capacity // c.P, c.width)
    else:
        cache = ops.KVCache(B, c.capacity, c.D, par(c.width), par(c.width), DEV)
    # second piece: row b's keys first[b] .. lengths[b] - 1 at the front of its input rows
    k2, v2 = torch.zeros(B, TAIL, c.D, device=DEV), torch.zeros(B, TAIL, c.D, device=DEV)
    for b, n in enumerate(lengths):
        k2[b, :n - first[b]] = kt[b, first[b]:n]
        v2[b, :n - first[b]] = vt[b, first[b]:n]
    n1 = max(max(first), 1)
    for before, cnt, kk, vv in (([0] * B, first, kt[:, :n1].contiguous(), vt[:, :n1].contiguous()),
                                (first, [n - f for n, f in zip(lengths, first)], k2, v2)):
        if paged:
            paged_util.grow(cache, plan, [a + n for a, n in zip(before, cnt)])
        cache.append(kk, vv, lengths=i32(before), counts=i32(cnt), max_length=max(before))
    return cache


def repeated(values, rep):
    return [x for x in values for _ in range(rep)]


def attend(c, q, cache, splits=None, group=None, window="case", rep=1):
    """the case's call (decode: at `splits`); group / window override the case's for a twin, rep > 1: on a cache that holds every row rep
    times"""
    from mi355q import ops
    kw = dict(c.scaling, group=c.group if group is None else group, window=c.window if window == "case" else window)
    if c.ragged:
        kw.update(lengths=i32(repeated(c.lengths, rep)), max_length=c.L)
    if c.kind == "decode":
        return ops.bfp_attention_decode(q, cache, splits=splits, **kw)
    if c.ragged and c.counts is not None:
        kw.update(counts=i32(repeated(c.counts, rep)))
    return ops.bfp_attention_extend(q, cache, **kw)
