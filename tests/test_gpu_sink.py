"""Attention sinks on the block_fp KV cache (ops.bfp_attention_decode / bfp_attention_extend with sinks=S beside window=W): every compiled
sink kernel form against the fp64-softmax oracle (tests/sink_util.py), the bit identities with the windowed, unwindowed, contiguous and
group-1 calls, the edges of the sink piece, a TinyLlama with sliding_window and attention_sinks, and the stale-LDS screen.
Not held: an extend of m <= 16 against a decode of the same queries bit for bit -- tests/test_gpu_window_extend.py does not hold that for
windows either (the two kernels differ), so only the oracle bound joins them here as there."""
import ctypes
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import sink_util as U  # noqa: E402
from paged_util import fill_both, pool_pages  # noqa: E402
from window_util import DEV, bits, check, filled, i32, inputs  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
NAN16 = 0x7FC1                # a bf16 NaN (as int16)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- every compiled form once ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", U.CASES, ids=lambda c: c.id)
def test_every_compiled_form_against_the_oracle(c):
    """rows of 80, 18 and 0 keys, W = 20, S = 4: row 0 has p0 = 1 (decode, lo = 56 in the pair's second tile) / a second query block with
    st0 = 1 and need = 5 (extend); each real row against the oracle, exact zeros for the empty row and behind counts[b]; the paged forms
    also give the contiguous call's bits"""
    import torch
    from mi355q import ops
    B, G, D, n = len(U.LENGTHS), c.group, c.D, max(U.LENGTHS)
    assert U.p0_of(U.LENGTHS[0], c.M if c.kind == "decode" else 70 - 64, U.WINDOW) >= 1
    q, k, v = inputs(B * G, c.M, n, D, seed=7 * c.form[0] + G)
    k, v = k[:B], v[:B]
    paged, contig = fill_both(_t(k), _t(v), list(U.LENGTHS), D, U.PAGE, -(-n // U.PAGE))
    kw = dict(scale_div=8.0, lengths=i32(U.LENGTHS), max_length=n, window=U.WINDOW, sinks=U.SINKS, group=G)
    if c.kind == "decode":
        fn = ops.bfp_attention_decode
    else:
        fn, kw["counts"] = ops.bfp_attention_extend, i32(c.counts)
    out = fn(_t(q), paged if c.paged else contig, **kw)
    torch.cuda.synchronize()
    if c.paged:
        assert torch.equal(bits(out), bits(fn(_t(q), contig, **kw)))
    out = out.cpu().numpy()
    for b, L in enumerate(U.LENGTHS):
        m = c.queries(b)
        rows = slice(b * G, b * G + G)
        assert not out[rows, m:].any(), f"row {b}: not exact zeros behind its {m} queries"
        if m:
            ref = U.oracle(q[rows, :m], np.repeat(k[b:b + 1, :L], G, 0), np.repeat(v[b:b + 1, :L], G, 0), 6, U.WINDOW, 8.0, U.SINKS)
            check(out[rows, :m], ref)


# ---- bit identities -------------------------------------------------------------------------------------------------------------
def _both(q, cache, **kw):
    from mi355q import ops
    M = q.shape[-2]
    outs = [ops.bfp_attention_extend(q, cache, **{k_: v_ for k_, v_ in kw.items() if k_ != "splits"})]
    if M <= 16:
        outs.append(ops.bfp_attention_decode(q, cache, **kw))
    return outs


@pytest.mark.parametrize("M", [5, 70])
def test_no_sinks_is_the_windowed_call(M):
    import torch
    q, k, v = inputs(2, M, 100, 64, seed=3)
    cache, qt = filled(k, v, 6, capacity=112), _t(q)
    kw = dict(scale_div=8.0, lengths=i32([100, 90]), max_length=100, window=20)
    for ref, a, b in zip(_both(qt, cache, **kw), _both(qt, cache, sinks=0, **kw), _both(qt, cache, sinks=None, **kw)):
        assert torch.equal(bits(a), bits(ref)) and torch.equal(bits(b), bits(ref))


@pytest.mark.parametrize("S", [1, 4, 16])
def test_sinks_inside_every_window_are_the_windowed_call(S):
    """rows whose every query has lower bound 0 (L_b <= W): the sinks lie inside the window, the bits are window=W's.  The decode of one
    query -- where that is the issue's L_b - M - W + 1 <= 0 -- with max_length at the rows' and, one split forced, far above them (the
    sink call's partition is that of span + 32 keys, the windowed call's that of span: equal bits need equal splits and pairs a split).
    With M > 1 the condition L_b - M - W + 1 <= 0 bounds query 0 alone: a later query's window may begin behind key 0, where its
    sinks ARE further keys by the semantics, so M = 5 is held where L_b <= W"""
    import torch
    from mi355q import ops
    q, k, v = inputs(2, 5, 18, 64, seed=S)
    cache, qt = filled(k, v, 6, capacity=96), _t(q)
    L = i32([18, 12])
    for M, W, extra in ((1, 20, dict(max_length=18)), (1, 18, dict(max_length=96, splits=1)), (5, 18, dict(max_length=18)),
                        (5, 19, dict(max_length=96, splits=1))):
        kw = dict(scale_div=8.0, lengths=L, window=W, **extra)
        for got, ref in zip(_both(qt[:, :M].contiguous(), cache, sinks=S, **kw), _both(qt[:, :M].contiguous(), cache, **kw)):
            assert torch.equal(bits(got), bits(ref)), (M, W)
    assert not torch.equal(bits(ops.bfp_attention_decode(qt, cache, scale_div=8.0, lengths=L, max_length=18, window=3, sinks=S)),
                           bits(ops.bfp_attention_decode(qt, cache, scale_div=8.0, lengths=L, max_length=18, window=3)))


@pytest.mark.parametrize("M", [5, 70])
def test_window_over_every_key_is_the_unwindowed_call(M):
    import torch
    q, k, v = inputs(2, M, 100, 64, seed=9)
    cache, qt = filled(k, v, 6, capacity=112), _t(q)
    kw = dict(scale_div=8.0, lengths=i32([100, 80]), max_length=100)
    for W in (100, 10 ** 6):
        for S in (1, 16):
            for got, ref in zip(_both(qt, cache, window=W, sinks=S, **kw), _both(qt, cache, **kw)):
                assert torch.equal(bits(got), bits(ref)), (W, S)


@pytest.mark.parametrize("M", [5, 70])
def test_grouped_is_group_one_on_the_repeated_cache(M):
    import torch
    B, G, L, W, S = 2, 2, 100, 20, 4
    q, k, v = inputs(B * G, M, L, 64, seed=2)
    k, v = k[:B], v[:B]
    kw = dict(scale_div=8.0, window=W, sinks=S, max_length=L, splits=2)
    got = _both(_t(q), filled(k, v, 6), group=G, lengths=i32([L, L - 9]), **kw)
    ref = _both(_t(q), filled(np.repeat(k, G, 0), np.repeat(v, G, 0), 6), lengths=i32([L, L, L - 9, L - 9]), **kw)
    for a, b in zip(got, ref):
        assert torch.equal(bits(a), bits(b))


# ---- edges ----------------------------------------------------------------------------------------------------------------------
EDGES = [  # M, L, W, S, splits
    (5, 80, 20, 16, None), (5, 80, 20, 1, None), (5, 80, 1, 4, None), (8, 80, 3, 4, None),
    (5, 100, 20, 4, None),      # lo = 76: p0 = 2, the pair's FIRST tile
    (5, 84, 20, 4, None),       # lo = 60: p0 = 1, the pair's second tile -- the sink pair and the window's first pair are adjacent
    (5, 72, 20, 4, None),       # lo = 48: p0 = 1, the pair's first tile
    (5, 45, 20, 4, None),       # lo = 21: p0 = 0 and the window begins in tile 1 -- tile 0 is read for its sinks alone
    (3, 131, 24, 4, 1), (3, 131, 24, 4, 64), (16, 131, 40, 7, 3),
]


@pytest.mark.parametrize("M,L,W,S,splits", EDGES)
def test_decode_edges(M, L, W, S, splits):
    B, D = 2, 64
    q, k, v = inputs(B, M, L, D, seed=L + W + S)
    from mi355q import ops
    out = ops.bfp_attention_decode(_t(q), filled(k, v, 6), scale_div=8.0, window=W, sinks=S, splits=splits).cpu().numpy()
    check(out, U.oracle(q, k, v, 6, W, 8.0, S))


@pytest.mark.parametrize("M,L,W,S", [(70, 100, 1, 4), (70, 100, 20, 16), (70, 100, 20, 1), (130, 200, 33, 4), (7, 90, 3, 4)])
def test_extend_edges(M, L, W, S):
    B, D = 2, 64
    q, k, v = inputs(B, M, L, D, seed=L + W + S)
    from mi355q import ops
    out = ops.bfp_attention_extend(_t(q), filled(k, v, 6), scale_div=8.0, window=W, sinks=S).cpu().numpy()
    check(out, U.oracle(q, k, v, 6, W, 8.0, S))


def test_trimmed_paged_row_keeps_page_zero():
    """rows of 200, 131 and 40 keys, P = 32, W = 24, S = 4: trim(..., sinks=4) keeps logical page 0 and gives back pages 1 .. k, whose
    entries then name a page of NaN patterns; decode and extend still give the contiguous cache's bits"""
    import torch
    from mi355q import ops
    lengths, W, S, D, M, P = [200, 131, 40], 24, 4, 64, 20, 32
    B, n = len(lengths), max(lengths)
    torch.manual_seed(4)
    k, v = torch.randn(B, n, D, device=DEV), torch.randn(B, n, D, device=DEV)
    paged, contig = fill_both(k, v, lengths, D, P, -(-n // P))
    q = torch.randn(B, M, D, device=DEV)
    kw = dict(scale_div=8.0, lengths=i32(lengths), max_length=n, window=W, sinks=S)
    calls = [(ops.bfp_attention_decode, q[:, :4].contiguous(), dict(kw, splits=2)), (ops.bfp_attention_decode, q[:, :1].contiguous(), kw),
             (ops.bfp_attention_extend, q, kw)]
    refs = [fn(qq, contig, **kw_) for fn, qq, kw_ in calls]
    held = [list(r) for r in paged.held]
    paged.trim(lengths, W + M, sinks=S)
    gone = [max(lengths[b] - (W + M) + 1, 0) // P for b in range(B)]
    assert gone[0] >= 3 and gone[2] == 0
    for b in range(B):
        assert paged.held[b] == held[b][:1] + [None] * max(gone[b] - 1, 0) + held[b][max(gone[b], 1):]
    for pool in (paged.kq, paged.vq):
        pool_pages(paged, pool)[paged.pad_page].fill_(NAN16)
    for (fn, qq, kw_), ref in zip(calls, refs):
        got = fn(qq, paged, **kw_)
        assert bool(torch.isfinite(got).all()) and torch.equal(bits(got), bits(ref)), fn.__name__


# ---- model ----------------------------------------------------------------------------------------------------------------------
PROMPT, STEPS, WINDOW, SINKS = 5, 30, 8, 2


def _w(width):
    return dict(name="block_fp", is_ptq=True, bypass=False, data_in_width=width, data_in_exponent_width=8, data_in_exponent_bias=127,
                data_in_block_size=[1, 16], weight_width=width, weight_exponent_width=8, weight_exponent_bias=127,
                weight_block_size=[1, 16], bias_width=width, bias_exponent_width=8, bias_exponent_bias=127, bias_block_size=[16])


def _model(layers, width, sinks=SINKS, seed=0, scale=4.0):
    import torch
    from mi355q import harness as H
    torch.manual_seed(seed)
    cfg = H.TinyLlamaConfig(vocab_size=97, hidden_size=128, intermediate_size=256, num_layers=layers, num_heads=4, max_positions=48,
                            sliding_window=WINDOW, num_kv_heads=2, attention_sinks=sinks)
    model = H.TinyLlamaForCausalLM(cfg, H.expand_llama_quant_config(_w(width), layers))
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.ndim == 2 and "embed" not in n:
                p.mul_(scale)
    return model.to(DEV)


def _ids(B=2):
    import torch
    return torch.randint(0, 97, (B, PROMPT + STEPS + 1), generator=torch.Generator().manual_seed(5)).to(DEV)


def _teacher_forced(model, ids, state):
    import torch
    B = ids.shape[0]
    kw = (lambda n: dict(counts=[n] * B)) if state.paged else (lambda n: {})      # (a paged state is always addressed in the ragged form)
    with torch.no_grad():
        out = [model(ids[:, :PROMPT], cache=state, **kw(PROMPT))[0][:, -1]]
        for t in range(PROMPT, PROMPT + STEPS):
            out.append(model(ids[:, t:t + 1], cache=state, **kw(1))[0][:, -1])
    return torch.stack(out, 1).cpu().numpy()


def _rel(a, ref):
    return float(np.abs(a - ref).max()) / max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("width", [6, 8])
def test_model_with_sinks(width):
    """2 layers, sliding_window 8, attention_sinks 2, a prompt of 5 and 30 steps (position 0 leaves the window at step 4).  The bound is
    that of tests/test_gpu_window_model.py, formed as there: twice the worst relative logit difference of the mode "fp32" route from the
    full forward on the ONE-layer model, floor 1e-3"""
    import torch
    from mi355q import harness as H
    ids = _ids()
    m1 = _model(1, width)
    a = _teacher_forced(m1, ids, H.DecodeState(m1, 2, ids.shape[1], "fp32"))
    with torch.no_grad():
        full = np.stack([m1(ids[:, :t + 1])[0][:, -1].cpu().numpy() for t in range(PROMPT - 1, PROMPT + STEPS)], 1)
    bound = max(2 * max(_rel(a[:, s], full[:, s]) for s in range(STEPS + 1)), 1e-3)
    model = _model(2, width)
    ref = _teacher_forced(model, ids, H.DecodeState(model, 2, ids.shape[1], "fp32"))
    state = H.DecodeState(model, 2, ids.shape[1], "block_fp")
    assert state.sinks == SINKS
    got = _teacher_forced(model, ids, state)
    paged_state = H.PagedDecodeState(model, 2, ids.shape[1], "block_fp", page_size=32)
    paged = _teacher_forced(model, ids, paged_state)
    for name, x in (("contiguous", got), ("paged", paged)):
        worst = max(_rel(x[:, s], ref[:, s]) for s in range(STEPS + 1))
        print("width", width, name, "block_fp vs fp32", worst, "bound", bound)
        assert worst <= bound, name
    most = -(-(WINDOW + 1) // 32) + 2
    assert all(sum(p is not None for p in row) <= most for c in paged_state.kv for row in c.held)
    # the sinks move the logits once position 0 has left the window, and not before
    unsunk = _model(2, width, sinks=None)
    plain = _teacher_forced(unsunk, ids, H.DecodeState(unsunk, 2, ids.shape[1], "block_fp"))
    assert np.array_equal(plain[:, :WINDOW - PROMPT + 1], got[:, :WINDOW - PROMPT + 1]) and _rel(got, plain) > 1e-3
    # chunked prefill: chunks of 3 through the decode kernel behind a non-empty cache, against mode "fp32" fed the same chunks
    r = H.generate(model, ids[:, :PROMPT + 12], 4, mode="fp32", chunk=3)[1].cpu().numpy()
    g = H.generate(model, ids[:, :PROMPT + 12], 4, mode="block_fp", chunk=3)[1].cpu().numpy()
    print("chunk 3, block_fp vs fp32", _rel(g, r))
    assert _rel(g, r) <= bound


# ---- stale LDS ------------------------------------------------------------------------------------------------------------------
PATTERNS = (None, 0x00000000, 0xFFFFFFFF, 0x7FC00000, 0x3F800000, 0x00000001, 0x80000000)      # None: the run without the poison


@pytest.fixture(scope="module")
def poison():
    import torch
    so = ROOT / "tools" / "lds_poison" / "liblds_poison.so"
    if not so.exists():
        pytest.fail("tools/lds_poison/liblds_poison.so is not built (__graft_entry__.build())")
    lib = ctypes.CDLL(str(so))

    def fill(pattern):
        if pattern is None:
            return
        rc = lib.lds_poison(ctypes.c_uint(pattern), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
    return fill


@pytest.mark.parametrize("dc", [1, 2, 3, 4])
def test_stale_lds_all_switches(poison, dc):
    """the grouped paged sink forms at every DC, decode (3 splits) and extend (70 queries), behind every pattern of tools/lds_poison:
    the bits of the run without it"""
    import torch
    from mi355q import ops
    D, G, n = 32 * dc, 2, 117
    lengths = [117, 87]
    torch.manual_seed(dc)
    paged, _ = fill_both(torch.randn(2, n, D, device=DEV), torch.randn(2, n, D, device=DEV), lengths, D, 32, 4)
    q = torch.randn(2 * G, 70, D, device=DEV)
    q8 = q[:, :8].contiguous()
    kw = dict(group=G, scale_div=math.sqrt(D), lengths=i32(lengths), max_length=n, window=20, sinks=4)
    for attend in (lambda: ops.bfp_attention_decode(q8, paged, splits=3, **kw), lambda: ops.bfp_attention_extend(q, paged, **kw)):
        outs = []
        for p in PATTERNS:
            poison(p)
            outs.append(attend().clone())
        torch.cuda.synchronize()
        assert bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0
        for p, o in zip(PATTERNS[1:], outs[1:]):
            assert torch.equal(bits(o), bits(outs[0])), f"output depends on stale LDS (pattern {p:#010x})"
