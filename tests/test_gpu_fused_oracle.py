"""The round-6 fused epilogues against the fp64 oracle, not against the same library with the switch off
(tests/test_gpu_gated.py holds them to the separate launches).  The gated MLP epilogue (mi355q_bfp_gemm_aligned_gated:
silu(gate) * up, csrc/mi355q_gemm_v9g.hip) and the relu epilogue (mi355q_bfp_gemm_aligned_relu, epi_op 2) write the
consumer's block_fp-quantised operand as tiled bf16; it is decoded on the host (oracle/compare.py) and held to

    quantise( op( round_fp32( x_q . w_q^T + b ) ) )

with x_q, w_q the oracle's quantised operands, the product in float64 (exact: x_q, w_q carry <= 8 significant bits, K <= 4096),
rounded once to fp32 as the reference's F.linear output is, and the reference's op in fp32 as torch writes it.  Each element must
equal the oracle's quantisation of h (1 - delta), h or h (1 + delta) (delta: the fp32 rounding the kernel's own accumulation
order is allowed); the fraction of elements where those three disagree is bounded, so that the rule is not vacuous.  The
quantiser-edge cases feed designed values through the bias (x = 0: the epilogue adds the bias as given) and are held EXACTLY
(delta = 0).  The slow paths (an overflowed activation bucket; a tile with more exception entries than its LDS holds) meet the
same rule."""
import numpy as np
import pytest

from oracle import compare as C
from oracle import np_oracle as O

pytestmark = pytest.mark.gpu

DELTA = 2.0 ** -20          # product + epilogue: fp32 accumulation over <= 4096 / 16 block terms, the bias add, silu and the multiply
AMBIGUOUS_MAX = 1e-2        # measured on the MI355X: at most 4.1e-3 over the fixed cases, 2.1e-2 in the sweep (bound 5e-2 there:
                            # coarse operands make sums that land exactly on 2^k, whose whole block is then ambiguous)


def _operands(M, I, K, seed, wx=6, ww=6, bias=False, x_exc=0, w_exc=0, wild_rows=0):
    """(copied from tests/test_gpu_gated.py, with the host tensors returned too)"""
    import torch
    from mi355q import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) * torch.exp(0.5 * torch.randn(M, 1, generator=g))
    wg, wu = torch.randn(I, K, generator=g) * 0.05, torch.randn(I, K, generator=g) * 0.05
    r = np.random.default_rng(seed)
    for _ in range(x_exc):                                   # exception blocks: far above / below their rows' window
        row, kb = int(r.integers(M)), int(r.integers(K // 16))
        x[row, kb * 16:kb * 16 + 16] *= float(r.choice([1 / 512.0, 300.0]))
    for _ in range(w_exc):
        row, kb = int(r.integers(I)), int(r.integers(K // 16))
        (wg if r.integers(2) else wu)[row, kb * 16:kb * 16 + 16] *= float(r.choice([1 / 512.0, 300.0]))
    for row in range(min(wild_rows, M)):                     # every one of the first rows: an exception block (a bucket overflows)
        kb = int(r.integers(K // 16))
        x[row, kb * 16:kb * 16 + 16] *= 2000.0
    bg = bu = None
    if bias:
        bg, bu = torch.randn(I, generator=g) * 0.05, torch.randn(I, generator=g) * 0.05
    return x, wg, wu, bg, bu


def _aligned_x(x, wx=6):
    import torch
    from mi355q import ops
    return ops.block_fp_quantize_aligned_rows(x.to("cuda:0"), wx, 8, 127)


def _aligned_w(w, ww=6):
    from mi355q import ops
    _, wm, we = ops.block_fp_quantize(w.to("cuda:0"), ww, 8, 127, [1, 16], False, want_fake=False, want_packed=True)
    return ops.bfp_align_rows(wm, we, ww - 1, 127)


def _product(x, ws, bs, wx=6, ww=6):
    """fp32 (x_q . w_q^T + b) per weight in ws: the oracle's quantised operands, the product in float64 (on the device: exact
    products, a float64 sum -- far below the one fp32 rounding at the end), rounded once; and the magnitudes |x_q| . |w_q|^T + |b|
    that the kernel's own fp32 rounding scales with"""
    import torch
    xq = torch.from_numpy(O.block_fp_quantize(x.numpy(), wx, 8, 127, [1, 16], True)).double().cuda()
    out, mags = [], []
    for w, b in zip(ws, bs):
        wq = torch.from_numpy(O.block_fp_quantize(w.numpy(), ww, 8, 127, [1, 16], False)).double().cuda()
        y = xq @ wq.t()
        mag = xq.abs() @ wq.abs().t()
        if b is not None:
            y = y + b.double().cuda()
            mag = mag + b.double().cuda().abs()
        out.append(y.float().cpu())
        mags.append(mag.cpu().numpy())
    return out, mags


def _slack_gated(g, u, mags):
    """an fp32 rounding of each product term (2^-24 of the terms' magnitude, twice over) carried through silu(g) * u"""
    return 2.0 ** -23 * (mags[0] * np.abs(u.double().numpy()) * 1.1 + mags[1] * np.abs(g.double().numpy()))


def _slack_relu(mags):
    return 2.0 ** -23 * mags[0]


def _gated(x, wg, wu, bg, bu, qw, qew=8, qeb=127, wx=6, ww=6, xa=None, may_decline=False):
    import torch
    from mi355q import ops
    I = wg.shape[0]
    xa = _aligned_x(x, wx) if xa is None else xa
    w_gu = ops.interleave_gate_up(_aligned_w(wg, ww), _aligned_w(wu, ww))
    if w_gu is None and may_decline:                         # (the pair does not qualify: re-bucketed exception lists too long)
        return None, xa
    assert w_gu is not None
    b_gu = None if bg is None else torch.stack((bg.reshape(I // 16, 16), bu.reshape(I // 16, 16)), dim=1).reshape(-1).contiguous().cuda()
    xt = ops.bfp_gemm_aligned_gated(xa, w_gu, qw, qew, qeb, b_gu)
    assert xt is not None
    torch.cuda.synchronize()
    return C.decode_bf16_tiled(xt, x.shape[0], I), xa


def _relu(x, w, b, qw, qew=8, qeb=127, wx=6, ww=6):
    import torch
    from mi355q import ops
    xa = _aligned_x(x, wx)
    xt = ops.bfp_gemm_aligned_relu(xa, _aligned_w(w, ww), qw, qew, qeb, None if b is None else b.cuda())
    assert xt is not None
    torch.cuda.synchronize()
    return C.decode_bf16_tiled(xt, x.shape[0], w.shape[0]), xa


def _h_gated(g, u):
    import torch
    return (torch.nn.functional.silu(g) * u).double().numpy()


def _h_relu(y):
    import torch
    return torch.relu(y).double().numpy()


def _check(tag, got, h64, qw, delta=DELTA, qew=8, qeb=127, amb_max=AMBIGUOUS_MAX, slack=None):
    m = C.match_quantised(got, h64, qw, qew, qeb, delta, bf16=True, slack=slack)
    print(f"{tag}: {m.total} values, {m.mismatched} mismatched, ambiguous fraction {m.ambiguous_fraction:.2e}")
    assert m.mismatched == 0, (tag, m.mismatched, m.first)
    assert m.ambiguous_fraction <= amb_max, (tag, m.ambiguous_fraction)
    return m


# (M, I, K, consumer width, bias): M at the 16-row piece and 256-row tile tails, every I and K of the issue at least once
SHAPES = [(1, 128, 256, 3, False), (15, 384, 2048, 4, True), (17, 1408, 256, 5, False), (255, 128, 4096, 6, True),
          (257, 384, 256, 7, False), (300, 1408, 2048, 8, True), (2047, 384, 4096, 9, False), (17, 11008, 2048, 6, True),
          (2047, 1408, 256, 6, True), (300, 11008, 256, 4, False)]


@pytest.mark.parametrize("M,I,K,qw,bias", SHAPES)
def test_gated_epilogue_against_the_oracle(M, I, K, qw, bias):
    x, wg, wu, bg, bu = _operands(M, I, K, seed=M * 7 + I + K, bias=bias, x_exc=12, w_exc=20)
    got, xa = _gated(x, wg, wu, bg, bu, qw)
    (g, u), mags = _product(x, (wg, wu), (bg, bu))
    _check(f"gated M={M} I={I} K={K} q{qw}", got, _h_gated(g, u), qw, slack=_slack_gated(g, u, mags))


@pytest.mark.parametrize("M,N,K,qw,bias", SHAPES)
def test_relu_epilogue_against_the_oracle(M, N, K, qw, bias):
    """with rows and 16-column blocks that are negative throughout: whole blocks are zero after relu (the epilogue fills their
    maximum with 1, the reference with the tensor's smallest block maximum -- all-zero blocks pass through either way)"""
    x, w, _, b, _ = _operands(M, N, K, seed=M * 5 + N + K + 1, bias=bias, x_exc=10, w_exc=16)
    neg_rows = list(range(0, M, 5))
    x[:, :16] *= 0.1
    x[neg_rows, 0] = 2.0 ** 26                               # with w[:, 0] = -1: these rows are negative in every column
    w[:, 0] = -1.0
    if b is not None:
        b[32:48] = -2.0 ** 30                                # whole blocks negative in every row
        b[N - 16:] = -2.0 ** 30
    got, _ = _relu(x, w, b, qw)
    (y,), mags = _product(x, (w,), (b,))
    h = _h_relu(y)
    zero_blocks = (h.reshape(M, -1, 16) == 0).all(-1)
    assert zero_blocks.all(1).any() and zero_blocks.sum() >= len(neg_rows) * N // 32         # (whole rows and blocks of zeros)
    _check(f"relu M={M} N={N} K={K} q{qw}", got, h, qw, slack=_slack_relu(mags))


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("kw", [dict(M=512, I=256, K=512, wild_rows=200), dict(M=512, I=256, K=512, x_exc=150, w_exc=150),
                                dict(M=300, I=384, K=2048, wild_rows=300), dict(M=257, I=1408, K=2048, x_exc=400, w_exc=600)],
                         ids=["bucket_overflow", "lds_overflow", "bucket_overflow_k2048", "lds_overflow_k2048"])
def test_epilogue_slow_paths_against_the_oracle(kw, bias):
    """the overflowed activation bucket (the blockwise-exact product into the scratch, converted tile by tile) and the tile with
    more exception entries than its LDS holds (atomics behind the stores, then the conversion), both epilogues: the same
    exact-or-ambiguous rule as the fast path -- not test_gated_epilogue_slow_paths' 7 % of the maximum"""
    kw = dict(kw)
    M, I, K = kw.pop("M"), kw.pop("I"), kw.pop("K")
    x, wg, wu, bg, bu = _operands(M, I, K, seed=M + I + K + 7, bias=bias, **kw)
    got, xa = _gated(x, wg, wu, bg, bu, 6)
    if "wild_rows" in kw:
        assert int(xa.sparse[0]) != 0                        # (the bucket did overflow)
    (g, u), mags = _product(x, (wg, wu), (bg, bu))
    _check(f"gated slow {kw} bias={bias}", got, _h_gated(g, u), 6, slack=_slack_gated(g, u, mags))
    slack = _slack_relu(mags)
    got, xa = _relu(x, wg, bg, 5)
    if "wild_rows" in kw:
        assert int(xa.sparse[0]) != 0
    _check(f"relu slow {kw} bias={bias}", got, _h_relu(g), 5, slack=slack)


# ---- the epilogue's own quantiser (gated_quant, csrc/mi355q_gemm_v9.hip) on designed inputs: x = 0, so that the epilogue
#      sees exactly the bias it is given (gated: up's bias 1, h = silu(gate's bias))
def _edge_rows(mbits, r, positive=False, scale_pow=0):
    """rows of 16-value blocks, each block a designed case for a quantiser with `mbits` mantissa bits"""
    f = np.float32
    s = 2.0 ** scale_pow
    rows = []

    def row_of(blocks):
        out = np.concatenate(blocks).astype(np.float32)
        return out if not positive else np.abs(out)

    blocks = []
    for k in (-10, -3, 0, 1, 5, 12):                        # block max exactly 2^k, just below and just above it
        for top in (2.0 ** k, np.nextafter(f(2.0 ** k), f(0)), np.nextafter(f(2.0 ** k), f(np.inf)),
                    np.float32(2.0 ** k * (1 + 3 * 2.0 ** -23)), np.float32(2.0 ** k * (1 - 2.0 ** -24))):
            b = r.uniform(-1, 1, 16) * top
            b[r.integers(16)] = top                          # (the maximum; it also rounds up to 2^mbits and must clamp)
            blocks.append(b * s)
    rows.append(row_of(blocks[:len(blocks) // 2]))
    rows.append(row_of(blocks[len(blocks) // 2:]))
    blocks = []
    for e in (-6, -2, 0, 3, 9):                              # mantissa ties, both parities, in blocks of maximum 0.75 * 2^e
        step = 2.0 ** (e - mbits)
        j = np.arange(16) % max(2 ** mbits - 1, 2)
        b = (j + 0.5) * step * np.where(np.arange(16) % 3 == 0, -1, 1)
        b[0] = 0.75 * 2.0 ** e
        blocks.append(b * s)
    rows.append(row_of(blocks))
    return [np.asarray(rw, dtype=np.float32) for rw in rows]


def _tiny_rows(mbits):
    """values <= 1e-8 (passed through unquantised), -0.0, and a row whose every block maximum lies in (1e-8, 2^(mbits - 28)]:
    the quantiser's general branch"""
    f = np.float32
    a = np.array([1e-8, -1e-8, np.nextafter(f(1e-8), f(0)), np.nextafter(f(1e-8), f(1)), 0.0, -0.0, 3e-9, -7e-12,
                  1.0, 0.3, 1e-8 * 0.5, 2e-8, 5e-8, -4e-8, 0.0, 9.9e-9], dtype=f)
    hi = 2.0 ** (mbits - 28)
    gen = []
    for i, top in enumerate(np.linspace(1.01e-8, hi, 8)):
        b = np.linspace(-1, 1, 16) * top * (0.3 + 0.05 * i)
        b[i] = top
        gen.append(b)
    gen.append(np.full(16, hi))
    gen.append(np.array([hi * (j + 0.5) / 2 ** mbits for j in range(16)]))   # ties in the general branch
    return [np.concatenate([a, a * 0.5, -a, a[::-1]]).astype(f), np.concatenate(gen).astype(f)]


def _clamp_row():
    """with a 4-bit exponent of bias 7 (e in [-7, 8]): maxima far above 2^8 (the mantissa saturates) and blocks below 2^-7"""
    r = np.random.default_rng(11)
    blocks = [r.uniform(-1, 1, 16) * t for t in (2.0 ** 8, 2.0 ** 9, 3e3, 1e5, 2.0 ** -7, 2.0 ** -9, 1e-4, 2.0 ** -7 * 0.99)]
    for b, t in zip(blocks, (2.0 ** 8, 2.0 ** 9, 3e3, 1e5, 2.0 ** -7, 2.0 ** -9, 1e-4, 2.0 ** -7 * 0.99)):
        b[3] = t
    return np.concatenate(blocks).astype(np.float32)


def _designed_runs(qw):
    r = np.random.default_rng(qw)
    mb = qw - 1
    runs = [(row, 8, 127) for row in _edge_rows(mb, r)] + [(row, 8, 127) for row in _tiny_rows(mb)] + [(_clamp_row(), 4, 7)]
    return runs


@pytest.mark.parametrize("qw", [3, 6, 9])
def test_relu_epilogue_quantiser_edges(qw):
    """relu(b) exactly (x = 0): every value is held to the oracle with delta = 0"""
    import torch
    for i, (row, qew, qeb) in enumerate(_designed_runs(qw)):
        N = row.size
        pad = (-N) % 128
        b = torch.from_numpy(np.concatenate([row, np.zeros(pad, np.float32)]))
        M, K = 17, 256
        x = torch.zeros(M, K)
        w = torch.randn(N + pad, K, generator=torch.Generator().manual_seed(i)) * 0.05
        got, _ = _relu(x, w, b, qw, qew, qeb)
        h = np.broadcast_to(_h_relu(b[None, :]), got.shape)
        _check(f"relu edges q{qw} run {i} (e{qew}/{qeb})", got, h, qw, delta=0.0, qew=qew, qeb=qeb, amb_max=0.0)


@pytest.mark.parametrize("qw", [3, 6, 9])
def test_gated_epilogue_quantiser_edges(qw):
    """h = silu(g) * 1 with g the gate's bias (x = 0, up's bias 1): the designed values pass silu exactly where silu is the
    identity in fp32 (g >= 18: sigmoid rounds to 1) or a halving (|g| < 2^-25: sigmoid rounds to 1/2) -- the large edges are
    scaled into the first range, the small ones doubled, and whatever then lies outside these ranges is set to 0; both are
    asserted on the host, so every value the quantiser sees is designed; held with delta = 0"""
    import torch
    mb = qw - 1
    r = np.random.default_rng(100 + qw)
    big = [np.where(np.abs(row) >= 18.0, row, 0.0).astype(np.float32) for row in _edge_rows(mb, r, positive=True, scale_pow=14)]
    small = [np.where(np.abs(row * 2) < 2.0 ** -25, row * 2, 0.0).astype(np.float32) for row in _tiny_rows(mb)]
    for i, row in enumerate(big + small):
        I = row.size
        pad = (-I) % 128
        g = torch.from_numpy(np.concatenate([row, np.zeros(pad, np.float32)]))
        u = torch.ones_like(g)
        M, K = 17, 256
        x = torch.zeros(M, K)
        wg, wu = (torch.randn(I + pad, K, generator=torch.Generator().manual_seed(i + s)) * 0.05 for s in (0, 1))
        got, _ = _gated(x, wg, wu, g, u, qw)
        h = np.broadcast_to(_h_gated(g[None, :], u[None, :]), got.shape)
        if i < len(big):
            assert np.array_equal(h[0], g.double().numpy())             # (silu is the identity on these)
        else:
            assert np.array_equal(h[0], g.double().numpy() / 2)         # (... and a halving on these)
        _check(f"gated edges q{qw} run {i}", got, h, qw, delta=0.0, amb_max=0.0)


def test_seeded_random_sweep():
    """40 random cases of both epilogues: shapes, consumer widths, operand widths, bias, exception counts, overflowed buckets"""
    r = np.random.default_rng(2024)
    worst, declined = 0.0, 0
    for case in range(40):
        op = "gated" if case % 2 == 0 else "relu"
        M = int(r.choice([int(r.integers(1, 40)), int(r.integers(200, 700))]))
        I = 128 * int(r.integers(1, 9))
        K = 128 * int(r.integers(2, 17))
        qw, wx, ww = int(r.integers(3, 10)), int(r.integers(3, 9)), int(r.integers(3, 9))
        kw = dict(bias=bool(r.integers(2)), x_exc=int(r.integers(0, 60)), w_exc=int(r.integers(0, 80)),
                  wild_rows=int(r.choice([0, 0, 0, 300])))
        x, wg, wu, bg, bu = _operands(M, I, K, seed=1000 + case, **kw)
        tag = f"sweep {case} {op} M={M} I={I} K={K} q{qw} x{wx} w{ww} {kw}"
        if op == "gated":
            got, _ = _gated(x, wg, wu, bg, bu, qw, wx=wx, ww=ww, may_decline=True)
            if got is None:
                declined += 1
                continue
            (g, u), mags = _product(x, (wg, wu), (bg, bu), wx, ww)
            m = _check(tag, got, _h_gated(g, u), qw, amb_max=0.05, slack=_slack_gated(g, u, mags))
        else:
            got, _ = _relu(x, wg, bg, qw, wx=wx, ww=ww)
            (y,), mags = _product(x, (wg,), (bg,), wx, ww)
            m = _check(tag, got, _h_relu(y), qw, amb_max=0.05, slack=_slack_relu(mags))
        worst = max(worst, m.ambiguous_fraction)
    print(f"sweep: worst ambiguous fraction {worst:.2e}; gated pairs declined by interleave_gate_up: {declined} of 20")
    assert declined <= 10
    import torch
    for case in range(8):                                    # the mixed contraction: layers with outlier channels
        M, K, N = int(r.integers(1, 600)), 128 * int(r.integers(4, 25)), 128 * int(r.integers(1, 5))
        cfg = _lin_cfg()
        lin, w0, b0 = _lin(K, N, cfg, seed=3000 + case)
        x = _outlier_x(M, K, seed=4000 + case)
        with torch.no_grad():
            for _ in range(2):
                y = lin(x.cuda())
        e = _rel(y.cpu().numpy(), O.bfp_linear_int(x.numpy(), w0, b0, cfg))
        print(f"sweep mixed {case} M={M} K={K} N={N}: mixed {lin._mixed is not None}, rel err {e:.2e}")
        assert e <= 1e-5, (case, e)


def test_gated_mlp_after_an_in_place_bias_edit_and_requantize():
    """gated_mlp keeps the interleaved gate / up operand and bias on the gate layer (linear.py, `_gated_pair`): after new fp32
    values are loaded into the layers, up.bias edited in place and requantize(), the next gated_mlp must use the new bias --
    held to the oracle (gate, up, silu * up in fp32, down: O.bfp_linear_int), before and after"""
    import torch
    import mi355q.quantize as Q
    from mi355q.quantize.quantized_modules.linear import gated_mlp
    cfg = dict(name="block_fp", is_ptq=True, bypass=False, data_in_width=6, data_in_exponent_width=8, data_in_exponent_bias=127,
               data_in_block_size=[1, 16], weight_width=6, weight_exponent_width=8, weight_exponent_bias=127, weight_block_size=[1, 16],
               bias_width=6, bias_exponent_width=8, bias_exponent_bias=127, bias_block_size=[16])
    H, I, M = 512, 512, 300
    torch.manual_seed(9)
    fps = [torch.nn.Linear(H, I), torch.nn.Linear(H, I), torch.nn.Linear(I, H)]
    cfgs = [dict(cfg, mi355q_align="rows"), dict(cfg, mi355q_align="rows"), dict(cfg, mi355q_align="blocks", mi355q_fused_activation=True)]
    gate, up, down = (Q.get_quantized_cls("linear", c).from_float(fp, c).to("cuda:0") for fp, c in zip(fps, cfgs))
    w0 = [fp.weight.detach().clone() for fp in fps]
    b0 = [fp.bias.detach().clone() for fp in fps]
    x = (torch.randn(M, H, generator=torch.Generator().manual_seed(1)) * 2).cuda()

    def oracle(b):
        xn = x.cpu().numpy()
        g = torch.from_numpy(O.bfp_linear_int(xn, w0[0].numpy(), b[0].numpy(), cfg))
        u = torch.from_numpy(O.bfp_linear_int(xn, w0[1].numpy(), b[1].numpy(), cfg))
        h = (torch.nn.functional.silu(g) * u).numpy()
        return O.bfp_linear_int(h, w0[2].numpy(), b[2].numpy(), cfg)

    def run():
        with torch.no_grad():
            for _ in range(2):                                # (the first PTQ forward quantises and packs the weights)
                down(torch.nn.functional.silu(gate(x)) * up(x))
            y = gated_mlp(x, gate, up, down)
        assert y is not None, "gated_mlp did not take the fused path"
        return y.cpu().numpy()

    for step in range(2):
        if step == 1:
            with torch.no_grad():
                for lin, w, b in zip((gate, up, down), w0, b0):
                    lin.weight.copy_(w.cuda())
                    lin.bias.copy_(b.cuda())
                b0[1] = b0[1] + 0.5
                up.bias.add_(0.5)                             # (in place: the version moves, the storage stays)
                for lin in (gate, up, down):
                    lin.requantize()
        y, ref = run(), oracle(b0)
        err = float(np.abs(y - ref).max() / np.abs(ref).max())
        print(f"gated_mlp step {step}: max error {err:.2e} of the maximum")
        assert err < 1e-3, (step, err)


# ---- the attention pass writing the out-projection's quantised operand (ops.bfp_attention(consumer=...)), with and without
#      rotary on load: decoded and held to the oracle attention (copied from tests/test_gpu_attention.py), quantised by the oracle
_FMIN = np.finfo(np.float32).min


def _attn_cfg(width):
    return dict(name="block_fp", is_ptq=True, bypass=False, data_in_width=width, data_in_exponent_width=8,
                data_in_exponent_bias=127, data_in_block_size=[1, 16], weight_width=width, weight_exponent_width=8,
                weight_exponent_bias=127, weight_block_size=[1, 16])


def _attn_oracle(q, k, v, c0, c1, causal=False, scale_div=None):
    w = O.matmul_quantized(q, np.swapaxes(k, -1, -2), c0)
    if scale_div:
        w = (w / np.float32(scale_div)).astype(np.float32)
    tq, tk = w.shape[-2:]
    if causal:
        m = np.triu(np.full((tq, tk), _FMIN, np.float32), 1 + tk - tq)
        with np.errstate(over="ignore"):
            w = np.maximum(w + m, _FMIN)
    e = np.exp((w - w.max(-1, keepdims=True)).astype(np.float64))
    p = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    return O.matmul_quantized(p, v, c1)


def _rotate_half(t):
    import torch
    h = t.shape[-1] // 2
    return torch.cat((-t[..., h:], t[..., :h]), dim=-1)


@pytest.mark.parametrize("H,M,T,D,cw,rope", [(4, 256, 256, 128, 6, True), (4, 256, 256, 128, 6, False), (2, 1536, 1536, 64, 4, True),
                                              (3, 100, 320, 64, 4, False), (2, 72, 256, 128, 8, False)])
def test_attention_consumer_operand_against_the_oracle(H, M, T, D, cw, rope):
    """the tiled operand against quantise(oracle attention), per element within the attention tolerance (1e-3 of the output's
    scale) plus one quantisation step of the element's block; with rope, the reference's rotary (q cos + rotate_half(q) sin in
    fp32, modeling_llama.py) applied on the host first.  At least EXACT_MIN of the values must be exactly the oracle's"""
    import math
    import torch
    from mi355q import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(H * 7 + M + T + D + cw)
    q = torch.randn(1, H, M, D, generator=g) * 1.5                                  # (ragged M < T: the last M queries, causal)
    k = torch.randn(1, H, T, D, generator=g)
    v = torch.randn(1, H, T, D, generator=g) * torch.exp(torch.randn(1, H, 1, D, generator=g))
    par = (6, 8, 127, 6, 8, 127)
    rp, qh, kh = None, q, k
    if rope:
        assert M == T
        inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
        emb = torch.cat([torch.outer(torch.arange(M).float(), inv)] * 2, dim=-1)
        cos, sin = torch.round(emb.cos() * 128) / 128, torch.round(emb.sin() * 128) / 128
        pos = torch.arange(M)[None]
        rp = (cos.to(dev).contiguous(), sin.to(dev).contiguous(), pos.to(dev).contiguous())
        qh, kh = q * cos + _rotate_half(q) * sin, k * cos + _rotate_half(k) * sin
    got = ops.bfp_attention(q.to(dev), k.to(dev), v.to(dev), par, par, causal=True, scale_div=math.sqrt(D), token_major=True, rope=rp,
                            consumer=(cw, 8, 127))
    torch.cuda.synchronize()
    assert isinstance(got, ops.TiledBf16) and (got.rows, got.cols) == (M, H * D)
    dec = C.decode_bf16_tiled(got.buf, M, H * D)
    ref = _attn_oracle(qh.numpy()[0], kh.numpy()[0], v.numpy()[0], _attn_cfg(6), _attn_cfg(6), causal=True, scale_div=math.sqrt(D))
    ref = np.ascontiguousarray(ref.transpose(1, 0, 2)).reshape(M, H * D)            # token-major [M, H D]
    want = O.block_fp_quantize(ref, cw, 8, 127, [1, 16], True)
    code = O.bfp_encode(ref, cw, 8, 127, [1, 16], True)
    step = np.repeat(np.ldexp(1.0, code.exp - (cw - 1)).reshape(M, -1), 16, axis=1)
    err = np.abs(dec.astype(np.float64) - want)
    scale = float(np.abs(ref).max())
    exact = float((dec == want).mean())
    print(f"attention consumer H={H} M={M} T={T} D={D} q{cw} rope={rope}: exact {exact:.4f}, max err {err.max():.2e} of scale {scale:.2f}")
    assert (err <= 1e-3 * scale + step).all(), float((err - 1e-3 * scale - step).max())
    assert exact >= EXACT_MIN, exact


EXACT_MIN = 0.99            # measured on the MI355X: every value exact (1.0000) in each case here


# ---- the mixed contraction (a layer with outlier channels takes `_mixed`) on the fused steps, and the hybrid weight storage
def _lin_cfg(**extra):
    return dict(name="block_fp", is_ptq=True, bypass=False, data_in_width=6, data_in_exponent_width=8, data_in_exponent_bias=127,
                data_in_block_size=[1, 16], weight_width=6, weight_exponent_width=8, weight_exponent_bias=127, weight_block_size=[1, 16],
                bias_width=6, bias_exponent_width=8, bias_exponent_bias=127, bias_block_size=[16], **extra)


def _lin(K, N, cfg, seed=0):
    import torch
    import mi355q.quantize as Q
    torch.manual_seed(seed)
    fp = torch.nn.Linear(K, N, bias=True)
    lin = Q.get_quantized_cls("linear", cfg).from_float(fp, cfg).to("cuda:0")
    return lin, fp.weight.detach().numpy().copy(), fp.bias.detach().numpy().copy()


def _outlier_x(M, K, seed, outliers=True):
    import torch
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) * torch.exp(torch.randn(M, 1, generator=g))
    if outliers:
        x[:, 5::97] *= 80.0                                  # outlier channels: the rows fit no window, class 1 takes them
    return x


def _rel(y, ref):
    return float(np.abs(np.asarray(y, np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("M,K,N", [(512, 1024, 512), (300, 2048, 384), (17, 4096, 256)])
def test_mixed_layer_fused_steps_against_the_oracle(M, K, N):
    """forward_after(x, "relu"), forward_after(gate, "silu_mul", up) and forward_residual(x, r) on a layer that took the mixed
    contraction: O.bfp_linear_int on the pre-op'd input (+ r), and the mixed launch really ran"""
    import torch
    from mi355q import ops
    cfg = _lin_cfg()
    lin, w0, b0 = _lin(K, N, cfg, seed=M + K)
    x = _outlier_x(M, K, seed=1)
    up = _outlier_x(M, K, seed=2, outliers=False)
    xd, upd = x.cuda(), up.cuda()
    res = torch.randn(M, N, generator=torch.Generator().manual_seed(3))
    calls, real = [], ops.bfp_gemm_mixed
    ops.bfp_gemm_mixed = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        with torch.no_grad():
            for _ in range(2):
                lin(xd)
            assert lin._mixed is not None, "the layer did not take the mixed contraction"
            n0 = len(calls)
            y_relu = lin.forward_after(xd, "relu").cpu().numpy()
            y_silu = lin.forward_after(xd, "silu_mul", upd).cpu().numpy()
            y_res = lin.forward_residual(xd, res.cuda()).cpu().numpy()
            torch.cuda.synchronize()
    finally:
        ops.bfp_gemm_mixed = real
    h_silu = (torch.nn.functional.silu(x) * up).numpy()
    e = (_rel(y_relu, O.bfp_linear_int(torch.relu(x).numpy(), w0, b0, cfg)),
         _rel(y_silu, O.bfp_linear_int(h_silu, w0, b0, cfg)),
         _rel(y_res, O.bfp_linear_int(x.numpy(), w0, b0, cfg).astype(np.float64) + res.numpy()))
    print(f"mixed M={M} K={K} N={N}: mixed launches {len(calls) - n0} of 3; rel err relu {e[0]:.2e} silu_mul {e[1]:.2e} residual {e[2]:.2e}")
    assert len(calls) - n0 >= 1, "no fused step took the mixed launch"
    assert max(e) <= 1e-5, e


@pytest.mark.parametrize("M", [300, 17])
def test_hybrid_storage_linear_against_the_oracle(M):
    """mi355q_weight_storage = "hybrid" on the per-block route (mi355q_align = "blocks": the weights packed at width + 0.5 bits,
    expanded per forward) at K = 11008, ragged M: O.bfp_linear_int, before and after requantize()"""
    import torch
    K, N = 11008, 384
    cfg = _lin_cfg(mi355q_weight_storage="hybrid", mi355q_align="blocks", mi355q_keep_master=True)
    lin, w0, b0 = _lin(K, N, cfg, seed=11)
    for step in range(2):
        if step == 1:
            lin.requantize()
        x = _outlier_x(M, K, seed=20 + step, outliers=False)
        with torch.no_grad():
            for _ in range(2):
                y = lin(x.cuda())
        assert lin._uses_bf16_route(), "not on the per-block route"
        assert lin._w_packed is not None, "the weights are not held packed"
        e = _rel(y.cpu().numpy(), O.bfp_linear_int(x.numpy(), w0, b0, cfg))
        print(f"hybrid M={M} K={K} step {step}: rel err {e:.2e}")
        assert e <= 1e-5, (step, e)
