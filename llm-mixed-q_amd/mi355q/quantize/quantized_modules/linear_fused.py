"""Several quantised `Linear` layers as one pass: the gated (Llama) and ReLU (OPT) MLPs, the q / k / v and gate / up groups, and the
unquantised head.  Each is written on the layers' own named predicates (`_LinearBase._settled`, `_on_plain_row_route`, ...) and
falls back to the separate calls whenever its layers do not qualify."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops
from .linear import _LinearBase


def _fusable_input(x) -> bool:
    return (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and 2 <= x.ndim <= 3
            and not (torch.is_grad_enabled() and x.requires_grad))


def _mlp_qualifies(x, producers, consumer, norm, norm_len: int, out_multiple: int):
    """the conditions gated_mlp and relu_mlp share: settled block_fp PTQ layers, the producers on the plain row-scale int8 route
    with one plan, the consumer on the per-block route with weights it can hand over as tiled bf16.  -> the producers' plan or None"""
    from ...sharded import RowShardedLinear
    first, layers = producers[0], (*producers, consumer)
    if any(isinstance(l, RowShardedLinear) or not isinstance(l, _LinearBase) for l in layers) or not _fusable_input(x):
        return None
    if not all(l._settled() for l in layers):
        return None
    c, dc = first.config, consumer.config
    if (c.get("mi355q_fused_gate_up", True) in (False, "off") or not dc.get("mi355q_fused_activation", False) or dc["data_in_width"] > 9
            or consumer.in_features != first.out_features or first.in_features % 128 or first.in_features < 256
            or first.out_features % out_multiple or (norm is not None and len(norm) != norm_len)):
        return None
    plan = first._int8_plan(x)
    if plan is None or consumer._int8_plan(x.new_empty((1, consumer.in_features))) is None:
        return None
    if not all(l._on_plain_row_route() for l in producers):
        return None
    if not consumer._uses_bf16_route() or (consumer._w_packed is not None and consumer._w_packed.row_scale_flavour):
        return None
    return plan


def gated_mlp(x, gate, up, down, norm=None, residual=None):
    """down(silu(gate(x)) * up(x)) [+ residual] for block_fp PTQ layers (modeling_llama.py:216, the Llama MLP) as TWO launches
    behind the activation quantiser instead of four: x -- with LlamaRMSNorm applied by its quantiser when `norm` = (weight, eps) --
    against gate's and up's weights INTERLEAVED in chunks of 16 rows (ops.interleave_gate_up, built once per pair), whose store
    epilogue forms silu(gate) * up in registers, quantises it with down's activation quantiser and writes down's tiled bf16
    operand (ops.bfp_gemm_aligned_gated: the two [tokens, intermediate] fp32 tensors are never written, the separate
    silu-mul-quantise launch -- 180 MB read, 45 MB written per Llama-7B layer at 2048 tokens -- is gone); then down's product on the
    bf16 flavour of the tile GEMM, the residual in its stores.  Same bits as grouped_linear + down.forward_after.  Returns None
    whenever the pair / the consumer does not qualify (first PTQ forward, gate / up not on the row-scale int8 route, down not on
    the per-block route, shapes, autograd ...): the caller then takes that path."""
    plan = _mlp_qualifies(x, (gate, up), down, norm, 2, 128)
    if (plan is None or gate.in_features != up.in_features or gate.out_features != up.out_features
            or (gate.bias is None) != (up.bias is None) or up._int8_plan(x) != plan or not gate._same_x_quantiser(up)):
        return None
    with torch.no_grad():
        pair = gate.__dict__.get("_gated_pair")
        key = (id(up), gate.weight._version, up.weight._version, gate._packed[0].tiled.data_ptr(), up._packed[0].tiled.data_ptr(),
               None if gate.bias is None else gate.bias._version, None if up.bias is None else up.bias._version)
        if pair is None or pair[0] != key:
            w_gu = ops.interleave_gate_up(gate._packed[0], up._packed[0])
            b_gu = None
            if w_gu is not None and gate.bias is not None:
                I = gate.out_features
                b_gu = torch.stack((gate.bias.data.reshape(I // 16, 16), up.bias.data.reshape(I // 16, 16)), dim=1).reshape(-1).contiguous()
            pair = gate.__dict__["_gated_pair"] = (key, w_gu, b_gu)
        _, w_gu, b_gu = pair
        if w_gu is None:
            return None
        x2 = x.reshape(-1, gate.in_features)
        xa = ops.block_fp_quantize_aligned_rows(x2, *gate.consumer_quantiser(), bucket_cap=gate._x_cap, pre=gate._norm_pre(norm))
        xt = ops.bfp_gemm_aligned_gated(xa, w_gu, *down.consumer_quantiser(), b_gu)
        if xt is None:
            return None
        return down._consumer_product(xt, x2.shape[0], x.shape[:-1], residual, x.device)


def relu_mlp(x, fc1, fc2, norm=None, residual=None):
    """fc2(relu(fc1(x))) [+ residual] for block_fp PTQ layers (modeling_opt.py:412-420, the OPT MLP) as TWO launches behind the
    activation quantiser: fc1's product with relu and fc2's activation quantiser in its store epilogue (ops.bfp_gemm_aligned_relu:
    the [tokens, ffn] fp32 tensor is never written, the relu-quantise launch is gone), then fc2's product on the bf16 flavour of the
    tile GEMM.  `norm` = (weight, bias, eps): OPT's final_layer_norm applied by fc1's quantiser.  Same bits as fc1 + fc2.forward_after.
    Returns None whenever the layers do not qualify (the caller then takes that path): gated_mlp's conditions with one producer."""
    if _mlp_qualifies(x, (fc1,), fc2, norm, 3, 32) is None:
        return None
    with torch.no_grad():
        x2 = x.reshape(-1, fc1.in_features)
        xa = ops.block_fp_quantize_aligned_rows(x2, *fc1.consumer_quantiser(), bucket_cap=fc1._x_cap, pre=fc1._norm_pre(norm))
        xt = ops.bfp_gemm_aligned_relu(xa, fc1._packed[0], *fc2.consumer_quantiser(), fc1.bias)
        if xt is None:
            return None
        return fc2._consumer_product(xt, x2.shape[0], x.shape[:-1], residual, x.device)


FP32_SPLIT_MIN_ROWS = 128     # (fewer tokens: the product is bound by the weight bytes, and the split operand is 3 x the fp32 one)


def fp32_linear(x, linear: nn.Linear, mode: str = "split"):
    """F.linear(x, linear.weight, linear.bias) for a layer the reference leaves UNQUANTISED -- the language-model head
    (modeling_llama.py:772,866; modeling_opt.py:942-944: nn.Linear in fp32) -- as an fp32-equivalent product on the bf16 MFMA:
    both operands as three bf16 parts, the six part products side by side along K in ONE launch of the bf16 tile GEMM
    (ops.fp32_split_tile / fp32_gemm_split; csrc/mi355q_split.hip).  Closer to an fp64 product than the vendor fp32 GEMM and 1.7 x
    faster at Llama-7B's head.  The weights' operand is built once and kept on the module (rebuilt when the parameter is written).
    `mode` "vendor", gradients wanted, a CPU tensor, fewer than FP32_SPLIT_MIN_ROWS tokens or in_features % 32 != 0: torch's
    F.linear, counted as a vendor GEMM."""
    w = linear.weight
    M = x.numel() // max(1, x.shape[-1])
    ok = (mode == "split" and torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and w.dtype == torch.float32 and w.device == x.device
          and linear.in_features % 32 == 0 and M >= FP32_SPLIT_MIN_ROWS and not (torch.is_grad_enabled() and (x.requires_grad or w.requires_grad)))
    if not ok:
        ops.count_vendor_gemm("fp32_linear (unquantised layer, vendor fp32 GEMM)")
        return F.linear(x, w, linear.bias)
    try:
        key = (w.data_ptr(), w._version, str(w.device))
    except RuntimeError:                      # (inference-mode tensors have no version counter: keyed by storage alone)
        key = (w.data_ptr(), None, str(w.device))
    cached = linear.__dict__.get("_mi355q_split_weight")
    if cached is None or cached[0] != key:
        with torch.no_grad():
            cached = (key, ops.fp32_split_tile(w.detach().contiguous(), 1))
        linear.__dict__["_mi355q_split_weight"] = cached
    with torch.no_grad():
        x2 = x.reshape(-1, linear.in_features).contiguous()
        y = ops.fp32_gemm_split(ops.fp32_split_tile(x2, 0), cached[1], M, linear.out_features, linear.in_features, bias=linear.bias)
    return y.reshape(*x.shape[:-1], linear.out_features)


def grouped_linear(x, layers, norm=None):
    """[layer(x) for layer in layers] for block_fp PTQ Linear layers that take the SAME input and have the same shape and
    widths -- the q / k / v projections of an attention block, gate / up of a gated MLP, which the reference's modules
    call one after the other (modeling_opt.py:231-245, modeling_llama.py:216, 283-287) -- as ONE activation quantisation
    and ONE launch of the tile GEMM over all their column tiles (ops.bfp_gemm_aligned_multi): the separate products
    leave compute units idle (2048 -> 2048: 128 tiles each) or waste most of a second round (4096 -> 11008: 344 tiles).
    Bit-identical to the separate calls; falls back to them whenever the group does not qualify (first PTQ forward,
    other arithmetics, the per-block bf16 route, differing shapes ...).

    `norm` = (weight, eps): the layers take LlamaRMSNorm(x) (modeling_llama.py:81-92, 236-238: the input of q / k / v and of
    gate / up, which nothing else reads), `norm` = (weight, bias, eps): nn.LayerNorm(x) (OPT's self_attn_layer_norm in
    front of q / k / v and final_layer_norm in front of fc1, modeling_opt.py:391-415) -- and the quantiser, which holds a
    whole row per workgroup, applies the norm itself, so the normalised tensor is never written.  Then the mean of squares is summed in the kernel's own fixed
    order: results agree with the separate norm to within the last-bit differences any two fp32 summation orders
    show (torch's own CPU and GPU reductions included), not bit for bit."""
    layers = list(layers)
    from ...sharded import RowShardedLinear
    if all(isinstance(l, RowShardedLinear) for l in layers):
        if all(l.keep_local for l in layers):
            # head-sharded q / k / v (sharded.shard_model(heads=True)): the rank's own heads, no collective here
            return grouped_linear(x, [l.local for l in layers], norm=norm)
        # row-sharded projections (sharded.shard_model): this rank's shards as one group, one all-gather per projection
        for l in layers:                                       # (each product straight into its rank's segment of its gather buffer)
            l._aim_at_gather_buffer(x)
        try:
            ys = grouped_linear(x, [l.local for l in layers], norm=norm)
        finally:
            for l in layers:
                l.local._out_hint = None
        if len(layers) == 2 and layers[0].gather == "quantised" and layers[0].consumer_pre == "silu_mul":
            # Llama's gate / up in front of down_proj (sharded.shard_model(gather="quantised")): both shards of a rank cover the
            # same columns, so silu(gate) * up and down_proj's quantiser run on the rank's own slice; ONE all-gather, of the
            # tiled bf16 operand.  The second result is None: down_proj.forward_after(gate, "silu_mul", None) reads the first
            return [layers[0].gather_output(ys[0], other=ys[1]), None]
        return [l.gather_output(y) for l, y in zip(layers, ys)]
    first = layers[0]

    def normed():
        if len(norm) == 3:
            return F.layer_norm(x, (x.shape[-1],), norm[0], norm[1], norm[2])
        w, eps = norm
        v = x.to(torch.float32).pow(2).mean(-1, keepdim=True)
        return w * (x * torch.rsqrt(v + eps)).to(x.dtype)

    def alike(l, plan):                                    # (same contraction, same plan, same activation quantiser as `first`)
        return l.in_features == first.in_features and l._int8_plan(x) == plan and l._same_x_quantiser(first)
    # (a layer that packed its weights on arrival and has not seen activations yet may join the row group while its int8 operand is
    #  resident: `pending_ok`; at rest it waits for its first forward, `_on_plain_row_route(packed_ok=True)`)
    ok = (len(layers) in ((1, 2, 3) if norm is not None else (2, 3)) and not (torch.is_grad_enabled() and x.requires_grad)
          and all(isinstance(l, _LinearBase) and l._settled(pending_ok=True) for l in layers))
    if ok:
        plan = first._int8_plan(x)
        ok = plan is not None and (norm is None or (x.is_cuda and x.dtype == torch.float32)) and all(
            l._on_plain_row_route(packed_ok=True) and l.out_features == first.out_features and alike(l, plan) for l in layers)
    if ok:
        x2 = x.reshape(-1, first.in_features)
        with torch.no_grad():
            xa = ops.block_fp_quantize_aligned_rows(x2, *first.consumer_quantiser(), bucket_cap=first._x_cap, pre=first._norm_pre(norm))
            # one launch, or the split of the group that takes fewer rounds over the chip (ops.grouped_launch_plan)
            # (width-bit storage: a launch's members expand into scratch slots 0 .. g - 1 first -- round 5; before, a packed layer
            #  kept its group off this path: separate launches, the norm by six torch kernels)
            outs, at = [], 0
            for g in ops.grouped_launch_plan(x2.shape[0], first.out_features, len(layers)):
                part = layers[at:at + g]
                at += g
                was = [l._w_packed.expand(i) if l._w_packed is not None else l._packed[0] for i, l in enumerate(part)]
                hints = [l._take_out(x2.shape[0]) for l in part]
                if g == 1:
                    ys = [ops.bfp_gemm_aligned(xa, was[0], part[0].bias, out=hints[0])]
                else:
                    ys = ops.bfp_gemm_aligned_multi(xa, was, [l.bias for l in part], outs=hints)
                if ys is None:
                    outs = None
                    break
                outs.extend(ys)
        if outs is not None:
            return [y.reshape(*x.shape[:-1], first.out_features) for y in outs]
    # The per-block-exponent route (bf16 tile GEMM: inputs no row window fits -- every Linear of a model whose hidden channels
    # differ in magnitude): ONE activation operand for the group, LlamaRMSNorm applied by its quantiser; the products stay separate
    # launches.  (Before round 5 such a group fell back to the torch norm -- six elementwise kernels -- and quantised x once per layer.)
    if (len(layers) >= 1 and (norm is None or len(norm) == 2) and _fusable_input(x)
            and all(isinstance(l, _LinearBase) and l._settled() for l in layers)):
        plan = first._int8_plan(x)
        if (plan is not None and (norm is not None or len(layers) > 1)
                and all(l._uses_bf16_route() and alike(l, plan)
                        and (l._w_packed is None or not l._w_packed.row_scale_flavour or len(layers) == 1) for l in layers)):
            x2 = x.reshape(-1, first.in_features).contiguous()
            with torch.no_grad():
                xt = ops.block_fp_quantize_bf16_tiled(x2, *first.consumer_quantiser(), pre=first._norm_pre(norm))
                outs = []
                for l in layers:           # (a packed layer's expand() shares one scratch operand: each product before the next expand)
                    y = ops.bf16_gemm_tiled(xt, l._bf16_weight_operand(x.device), x2.shape[0], l.out_features, l.in_features, l.bias,
                                            out=l._take_out(x2.shape[0]))
                    outs.append(y.reshape(*x.shape[:-1], l.out_features))
            return outs
    h = x if norm is None else normed()
    return [l(h) for l in layers]
