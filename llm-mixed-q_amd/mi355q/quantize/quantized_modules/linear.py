"""Quantised `nn.Linear` classes with the reference's contract
(`models/quantize/quantized_modules/linear.py:31-101, 113-203`): subclass of nn.Linear, ctor
`(in_features, out_features, bias, device, dtype, config)`, attributes `config, bypass, is_ptq,
weight_requires_quantisation, x_quantizer, w_quantizer, b_quantizer`, `from_float`, `__repr__`.

MI355X path of `LinearBlockFP` in PTQ mode (the hot path):
  first forward : W <- Qw(W), b <- Qb(b) in place (as the reference, linear.py:66-70) AND the int8
                  mantissas + uint8 shared exponents of W are packed once and kept on the module;
  every forward : x -> quantise+pack kernel -> exponent-align -> int8-MFMA block GEMM -> fp32 y (+ b), no fake-quant
                  tensor and no fp32 GEMM.  Operands no row window fits (post-activation inputs, weights with outlier
                  input channels) keep every block's exponent: x -> quantise straight into tiled bf16 -> the bf16
                  flavour of the same tile GEMM (values exact in bf16, products exact in fp32).
Formats whose contraction is not an int8 dot (block_minifloat, block_log, exotic block shapes,
QAT) quantise with the HIP fake-quant kernels and contract with the stock fp32 GEMM on the GPU.
"""
from __future__ import annotations

from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops
from ..quantizers import QUANTIZER_MAP
from . import linear_policy as policy

# config-key suffixes each quantiser takes, per operand prefix (linear.py:113-203)
_PARAMS = {
    "block_fp": dict(width="width", exponent_width="exponent_width", exponent_bias="exponent_bias",
                     block_size="block_size"),
    "block_minifloat": dict(width="width", exponent_width="exponent_width",
                            exponent_bias_width="exponent_bias_width", block_size="block_size"),
    "block_log": dict(width="width", exponent_bias_width="exponent_bias_width", block_size="block_size"),
    "integer": dict(width="width", frac_width="frac_width"),
    "minifloat_ieee": dict(width="width", exponent_width="exponent_width", exponent_bias="exponent_bias"),
    "minifloat_denorm": dict(width="width", exponent_width="exponent_width", exponent_bias="exponent_bias"),
    # the reference passes exponent_width to log_quantizer, which rejects it
    "log": dict(width="width", exponent_width="exponent_width", exponent_bias="exponent_bias"),
}
_BLOCKED = ("block_fp", "block_minifloat", "block_log")


def _make_quantizer(arith: str, config: dict, prefix: str, skip_first_dim: bool):
    kw = {arg: config[f"{prefix}_{suffix}"] for arg, suffix in _PARAMS[arith].items()}
    if arith in _BLOCKED:
        kw["skip_first_dim"] = skip_first_dim
    elif arith == "integer":
        kw["is_signed"] = True
    return partial(QUANTIZER_MAP[arith], **kw)


def _capturing_graph() -> bool:
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def _bf16_planes(t):
    """fp32 [rows, K] -> (hi, lo) with hi + lo = t to 2^-17 relative: hi = t rounded to bf16, lo the remainder (rounded to bf16
    when it is tiled).  A gradient is not a quantised value: one bf16 plane would cost it 2^-9."""
    hi = t.to(torch.bfloat16).to(torch.float32)
    return hi, t - hi


class _TileLinear(torch.autograd.Function):
    """y = x_q . W_q^T + b_q on the bf16 tile GEMM (operands exact in bf16, fp32 accumulation), and its backward as two more
    products on the same kernel: dX = dY . W_q, dW = dY^T . x_q, db = sum dY (reference: torch.autograd through F.linear,
    quantized_modules/linear.py:72-76; the quantisers' straight-through estimators stay where they are).  dY enters as two
    bf16 planes (hi + lo): four launches per backward."""

    @staticmethod
    def forward(ctx, xq, wq, bq):
        K, N = wq.shape[1], wq.shape[0]
        x2 = xq.reshape(-1, K).contiguous()
        y = ops.bf16_gemm_tiled(ops.bf16_tile(x2), ops.bf16_tile(wq.contiguous()), x2.shape[0], N, K, bq)
        ctx.save_for_backward(x2, wq)
        ctx.lead, ctx.has_bias = xq.shape[:-1], bq is not None
        return y.reshape(*xq.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x2, wq = ctx.saved_tensors
        M, K, N = x2.shape[0], x2.shape[1], wq.shape[0]
        dy2 = dy.reshape(M, N).contiguous().to(torch.float32)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:                              # dX [M, K] = dY [M, N] . (W_q^T [K, N])^T
            wt = ops.bf16_tile(wq.t().contiguous())
            hi, lo = _bf16_planes(dy2)
            dx = ops.bf16_gemm_tiled(ops.bf16_tile(hi), wt, M, K, N)
            dx += ops.bf16_gemm_tiled(ops.bf16_tile(lo), wt, M, K, N)
            dx = dx.reshape(*ctx.lead, K)
        if ctx.needs_input_grad[1]:                              # dW [N, K] = dY^T [N, M] . (x_q^T [K, M])^T
            xt = ops.bf16_tile(x2.t().contiguous())
            hi, lo = _bf16_planes(dy2.t().contiguous())
            dw = ops.bf16_gemm_tiled(ops.bf16_tile(hi), xt, N, K, M)
            dw += ops.bf16_gemm_tiled(ops.bf16_tile(lo), xt, N, K, M)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = dy2.sum(0)
        return dx, dw, db


class _LinearBase(nn.Linear):
    arith: str = None

    def __init__(self, in_features: int, out_features: int, bias: bool = True, device=None, dtype=None,
                 config: dict = None) -> None:
        super().__init__(in_features, out_features, bias, device, dtype)
        self.config = config
        self.bypass = config.get("bypass", False)
        self.is_ptq = config.get("is_ptq", False)
        self.weight_requires_quantisation = True if self.is_ptq else False
        self.x_quantizer = self.w_quantizer = self.b_quantizer = None
        self._packed = None          # (aligned W operand, its tiled mantissas, weight._version, bias._version)
        # exponent alignment of the packed operands (an implementation knob, not part of the reference config):
        # "rows" = one exponent per row (row-scale int8 GEMM), "blocks" = every block keeps its exponent (bf16 tile GEMM),
        # "auto" = rows when the weights and the first activations fit it, re-checked on a doubling schedule
        # (the alignment per 256-value group, "groups", went in round 5 with its int32-chain kernel)
        self.align = config.get("mi355q_align", "auto")
        self._align_mode, self._calls, self._row_overflows = None, 0, 0
        self._w_bf16 = None          # (tiled bf16 weights, weight._version) of the per-block-exponent route
        self._mx_w, self._mx_calls, self._mx_version = None, 0, -1      # W4A4 on the MX scaled MFMA: the weights' operand
        # implementation knobs next to "mi355q_align" (not part of the reference config):
        #   mi355q_weight_storage = "packed": keep the weights at rest as width-bit mantissas + one byte per block
        #       (width + 0.5 bits per value, ops.PackedWeights) and stream them into a shared scratch operand every forward;
        #   mi355q_keep_master = True: keep the fp32 weights / bias the layer was given, so that requantize() can quantise
        #       them again (other widths included) without a checkpoint reload (the search loop)
        #   mi355q_mixed = "auto" (default) / False: layers whose activations (or weights) carry OUTLIER CHANNELS -- block columns that
        #       lie outside their rows' exponent window in a large share of the rows -- split in_features into two classes of block
        #       columns and run ONE launch of the mixed contraction (ops.bfp_gemm_mixed: class 0 on the int8 MFMA, class 1 on the
        #       bf16 MFMA) instead of the whole layer on the bf16 flavour (round 6)
        #   mi355q_small_m = "off" (default) / "packed": forward() of at most ops.SMALL_M_MAX rows on a layer that keeps packed
        #       weights runs the small-batch product that reads them in place (`_small_m_takes`)
        self._mixed = None           # dict(classes, wa0, w1): the column split and the weights' two operands
        self._w_packed = None
        self._pending_flavour = None
        self._master = None
        self._fp32_released = False
        self._x_cap = policy.initial_x_cap(self.align)
        if not self.bypass:
            self._setup_quantizers(config)
        if self._packs_at_load():
            self.register_load_state_dict_post_hook(lambda module, incompatible: module._loaded_new_weights())

    # ---- mi355q_weight_storage = "packed": the weights are quantised and packed WHEN THEY ARRIVE -- when the module reaches
    #      the GPU (from_float(...).to(device), model.to(device)) and when a state dict is loaded into it -- not at the first
    #      forward: a model loaded for inference holds width + 0.5 bits per weight before it has seen a token (SURVEY 8f.2,
    #      quantized_modules/linear.py:66-70 is where the reference does the same work, at the first forward)
    def _packs_at_load(self) -> bool:
        return (not self.bypass and self.is_ptq and self.arith == "block_fp"
                and self.config.get("mi355q_weight_storage", "int8") == "packed")

    def _pack_if_arrived(self):
        if self._packs_at_load() and self.weight_requires_quantisation and self.weight.is_cuda and self.weight.numel():
            self.pack_now()

    def _loaded_new_weights(self):
        with torch.no_grad():
            self.weight_requires_quantisation = True          # (fresh fp32 values: quantise them again)
            self._packed, self._w_bf16, self._w_packed, self._pending_flavour, self._mixed = None, None, None, None, None
            if self._master is not None:
                self._master = (self.weight.detach().clone(), None if self.bias is None else self.bias.detach().clone())
            self._pack_if_arrived()

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        if self.__dict__.get("config") is not None:
            pend = self.__dict__.get("_pending_flavour")
            if pend is not None and pend[0].device != self.weight.device:
                self._pending_flavour = None        # (moved again before its first forward: the repack route decides, forward())
            with torch.no_grad():
                self._pack_if_arrived()
        return out

    def _setup_quantizers(self, config: dict):
        self.x_quantizer = _make_quantizer(self.arith, config, "data_in", True)
        self.w_quantizer = _make_quantizer(self.arith, config, "weight", False)
        self.b_quantizer = _make_quantizer(self.arith, config, "bias", False) if self.bias is not None else None

    # -- int8 block GEMM eligibility ------------------------------------------------------
    def _int8_plan(self, x: torch.Tensor):
        """(x_mbits, w_mbits, x_bias, w_bias) when the contraction is an int8 x int8 block dot on
        the MFMA path: block_fp both sides, [1,16] blocks along in_features, widths <= 8."""
        if self.arith != "block_fp" or not x.is_cuda or x.dtype != torch.float32 or x.ndim < 2:
            return None
        key = (x.ndim, x.shape[-2] if x.ndim == 3 else 0, id(self.config))
        cached = self.__dict__.get("_plan_cache")
        if cached is not None and cached[0] == key:
            return cached[1]
        plan = policy.int8_plan(self.config, self.arith, self.in_features, self.out_features, *key[:2])
        self.__dict__["_plan_cache"] = (key, plan)
        return plan

    @torch.no_grad()
    def _quantise_weights_once(self, pack: bool, x_sample=None):
        """linear.py:66-70 plus the one-off packing of the int8 operand"""
        c = self.config
        if c.get("mi355q_keep_master", False) and self._master is None:
            self._master = (self.weight.detach().clone(), None if self.bias is None else self.bias.detach().clone())
        self._mx_w = None
        if pack and self._mx_config_ok():
            # W4A4 on the MX scaled MFMA (csrc/mi355q_mx.hip): the operand from the RAW weights (block_fp is not idempotent), kept
            # only if every 32-group of W fits the format (one host read, here where the weights are packed anyway)
            mw = ops.block_fp_quantize_mx(self.weight.data.contiguous(), c["weight_width"], c["weight_exponent_width"], c["weight_exponent_bias"],
                                          reuse=False, keep_source=False)
            if _capturing_graph() or int(mw.bad[0]) == 0:
                self._mx_w = mw
        if pack:
            wq, wm, we = ops.block_fp_quantize(self.weight.data, c["weight_width"], c["weight_exponent_width"],
                                               c["weight_exponent_bias"], c["weight_block_size"], False,
                                               want_packed=True)
            self.weight.copy_(wq)
        else:
            self.weight.copy_(self.w_quantizer(self.weight.data))
        if self.bias is not None:
            self.bias.copy_(self.b_quantizer(self.bias.data))
        self.weight_requires_quantisation = False
        self._mx_version = self.weight._version
        if pack:
            self._pack_operands(wm, we, x_sample)
            # packed on arrival (no activation seen yet, `_pack_if_arrived`): the integers stay until the first forward has
            # decided which flavour the layer's activations call for (`_finalise_packed_flavour`)
            self._pending_flavour = (wm, we) if x_sample is None and self._packs_at_load() else None

    def _pack_operands(self, wm, we, x_sample):
        c = self.config
        self._choose_align_mode(wm, we, x_sample)
        self._align_weights(wm, we)
        versions = self._versions()
        if self._mixed is not None:
            self._mixed["version"] = versions
        # "packed": every layer at rest as width-bit mantissas + a byte per block, expanded per forward; "hybrid" (round 6): only the
        # layers on the per-block-exponent route -- whose resident operand is 16 bits a value, and whose expand pass is a third of a
        # Llama layer's -- while the row-scale layers keep their int8 operands (8.5 bits a value) and every fused path that needs them
        storage = c.get("mi355q_weight_storage", "int8")
        packed_storage = storage == "packed" and self._align_mode == "rows"
        self._w_packed = None
        if self._uses_bf16_route():
            # per-block exponents: the quantised weights (already in .weight) as tiled bf16; the int8 operand is not
            # needed on this route (the exact-integer blockwise kernel, mi355q_blocks_gemm = "int8", keeps it)
            if packed_storage or (storage == "hybrid" and self._align_mode == "rows"):
                self._w_packed = ops.pack_block_exponent_weights(wm, we, c["weight_width"], self._weight_bias_value())
                self._packed = (None, self._w_packed.packed, *versions)
            else:
                self._packed = (None, self._tiled_bf16_weights(None), *versions)
        elif packed_storage and self._x_cap != ops.ROW_NO_ALIGN:
            self._w_packed = ops.pack_row_aligned_weights(wm, we, self._packed[0], c["weight_width"], self._weight_bias_value())
            self._packed = (None, self._w_packed.packed, *versions)

    @torch.no_grad()
    def _finalise_packed_flavour(self, x):
        """first forward of a layer that packed its weights on arrival: the activation-dependent half of the route decision
        (`_choose_align_mode`), from the kept integers; then they go"""
        wm, we = self._pending_flavour
        self._pending_flavour = None
        if not self._fp32_released and self._packed is not None:
            self._x_cap = policy.initial_x_cap(self.align)
            self._pack_operands(wm, we, x)

    def _weight_bias_value(self):
        return policy.weight_bias(self.config)

    def _versions(self):
        return (self.weight._version, None if self.bias is None else self.bias._version)

    def _choose_align_mode(self, wm, we, x_sample):
        """rows, per-block exponents or the mixed split (`policy.align_decision`), from one-off host reads at pack time: the overflow
        word and the fullest exception bucket of the weights and -- where those fit -- of the sample activations"""
        c, K, N = self.config, self.in_features, self.out_features
        w_fill = x_fill = None
        M = 0
        if policy.align_is_measured(K, self.align):
            wa = ops.bfp_align_rows(wm, we, c["weight_width"] - 1, self._weight_bias_value())
            w_fill = ops.row_list_fill(wa.sparse, N)
            if x_sample is not None and policy.rows_fit(w_fill):
                xa = ops.block_fp_quantize_aligned_rows(x_sample.reshape(-1, K), *self.consumer_quantiser(), bucket_cap=ops.ROW_BUCKET_CAP_MAX)
                x_fill, M = ops.row_list_fill(xa.sparse, xa.rows, xa.list_cap), xa.rows
        d = policy.align_decision(K, N, M, self.align, w_fill, x_fill)
        cap = d.x_cap
        if d.try_mixed:
            after = d.x_cap_if_mixed if self._try_mixed(wm, we, x_sample) else d.x_cap_if_not
            cap = cap if after is None else after
        if cap is not None:
            self._x_cap = cap

    @staticmethod
    def _outlier_share(codes, spare: int):
        """codes [rows, blocks] (biased block exponents): per block column, the share of the rows in which the block lies
        outside a window of spare + 1 exponents centred on the row's median exponent"""
        c = codes.to(torch.int16)
        med = c.median(dim=1, keepdim=True).values
        out = (c < med - spare // 2) | (c > med + (spare - spare // 2))
        return out.float().mean(0)

    def _try_mixed(self, wm, we, x_sample) -> bool:
        """The mixed contraction for a layer whose rows fit no exponent window AS A WHOLE (README.md:9-11 of the reference: a few
        input channels tens of times larger than the rest): block columns that are outliers in more than a quarter of the rows --
        of the sample activations or of the weights -- become class 1 (tiled bf16, every block its own exponent); if they are at
        most half of the columns and the remaining class 0 fits the row-scale route's exception buckets on both operands, the layer
        runs ONE launch with class 0 on the int8 MFMA (ops.bfp_gemm_mixed) instead of all of it on the bf16 flavour.  Decided once
        per packing from the first activations, like the row / block decision itself; results never depend on it."""
        c, K = self.config, self.in_features
        self._mixed = None
        if (x_sample is None or not policy.mixed_config_ok(c, K, self.align) or not x_sample.is_cuda or x_sample.dtype != torch.float32):
            return False
        nb = K // 16
        x2 = x_sample.reshape(-1, K)
        _, _, xe = ops.block_fp_quantize(x2, *self.consumer_quantiser(), [1, 16], True, want_fake=False, want_packed=True)
        share = torch.maximum(self._outlier_share(xe.view(-1, nb), 8 - c["data_in_width"]),
                              self._outlier_share(we.view(-1, nb), 8 - c["weight_width"]))
        n1 = policy.mixed_class1_blocks(int((share > policy.MIXED_OUTLIER_SHARE).sum()), nb)
        if n1 == 0:
            return False
        blocks1 = torch.topk(share, n1).indices.cpu().tolist()
        classes = ops.ColumnClasses(K, blocks1, x2.device)
        N = self.out_features
        wa0 = ops.bfp_align_rows(wm.view(N, K)[:, classes.cols0].contiguous(), we.view(N, nb)[:, classes.blocks0].contiguous(),
                                 c["weight_width"] - 1, self._weight_bias_value())
        w_fill = ops.row_list_fill(wa0.sparse, N)
        if not policy.rows_fit(w_fill):
            return False
        x0, _ = ops.block_fp_quantize_classes(x2, classes, *self.consumer_quantiser(), bucket_cap=ops.ROW_BUCKET_CAP_MAX)
        if not policy.mixed_fits(w_fill, ops.row_list_fill(x0.sparse, x0.rows, x0.list_cap)):
            return False
        # (the weights' class-1 operand: the fake-quantised values already in .weight, as tiled bf16)
        w1 = ops.bf16_tile(self.weight.data[:, classes.cols1].contiguous())
        self._mixed = dict(classes=classes, wa0=wa0, w1=w1, version=None)
        return True

    def _uses_bf16_route(self) -> bool:
        return self._align_mode == "rows" and policy.uses_bf16_route(self.config, self.in_features, self._x_cap)

    def _hold_packed(self, wa, tiled):
        """the layer's packed weights: the aligned operand (None where the route needs none) and the tiled buffer.  The one place
        `_align_mode` leaves None: "rows" says that the layer holds packed operands (`_x_cap` and `_mixed` say which route)"""
        self._align_mode, self._packed = "rows", (wa, tiled, *self._versions())

    def _align_weights(self, wm, we):
        if not ops.row_align_supported(self.in_features):     # (bf16 route only: `_pack_operands` sets the operand)
            return self._hold_packed(None, None)
        wa = ops.bfp_align_rows(wm, we, self.config["weight_width"] - 1, self._weight_bias_value())
        self._hold_packed(wa, wa.tiled)

    def _packed_is_current(self) -> bool:
        p = self._packed
        return (p is not None and p[2] == self.weight._version and p[1].device == self.weight.device
                and (self.bias is None or p[3] == self.bias._version))

    def _settled(self, pending_ok: bool = False) -> bool:
        """a block_fp PTQ layer in its steady state: weights quantised in place, the packed operand current, and the flavour a
        layer packed on arrival still owes its first forward decided (`pending_ok`: or not)"""
        return (self.arith == "block_fp" and self.is_ptq and not self.bypass and not self.weight_requires_quantisation
                and (pending_ok or self._pending_flavour is None) and self._packed_is_current())

    def _on_row_route(self) -> bool:
        return self._align_mode == "rows" and not self._uses_bf16_route()

    def _on_plain_row_route(self, packed_ok: bool = False) -> bool:
        """the row-scale int8 route with 120-entry activation buckets, no mixed split and the int8 operand resident (`packed_ok`: or
        at rest in its row-scale flavour, once the first forward has settled that)"""
        return (self._on_row_route() and self._mixed is None and self._x_cap == ops.ROW_BUCKET_CAP
                and (self._w_packed is None or (packed_ok and self._w_packed.row_scale_flavour and self._pending_flavour is None)))

    def _same_x_quantiser(self, other) -> bool:
        return self.consumer_quantiser() == other.consumer_quantiser()

    def _tiled_bf16_weights(self, device, contiguous: bool = False, released: str = None):
        """the quantised weights (.weight) as the tiled bf16 operand, tiled again when they were written or moved (`device` None:
        now).  `contiguous`: the caller accepts strided weights; `released`: what the caller can no longer do once the fp32 weights
        are gone (None: it never asked)"""
        w = self._w_bf16
        if w is None or w[1] != self.weight._version or w[0].device != device:
            if released is not None and self._fp32_released:
                raise RuntimeError(f"mi355q: the fp32 weights were released; this layer cannot {released} any more")
            data = self.weight.data.contiguous() if contiguous else self.weight.data
            self._w_bf16 = (ops.bf16_tile(data), self.weight._version)
        return self._w_bf16[0]

    @torch.no_grad()
    def _repack_quantised_weights(self, x_sample):
        """the module was moved to another device after its first forward: pack again from .weight, which holds the
        quantised values -- a quantised tensor re-encodes exactly only through a cast (the quantiser is not idempotent,
        SURVEY 8a quirk 7), so the route from here on is the per-block-exponent one (tiled bf16).  Weights edited in
        place after the first forward are NOT repacked: like the reference they are used as they are (fp32 GEMM) until
        requantize()."""
        if not policy.bf16_operands_ok(self.config, self.in_features):
            return False
        self._x_cap, self._mixed = ops.ROW_NO_ALIGN, None
        self._hold_packed(None, self._tiled_bf16_weights(None, contiguous=True))
        return True

    def requantize(self, config: dict = None):
        """Search-loop helper (the reference rebuilds the model and reloads the checkpoint for every trial,
        search/search.py:753-763): make the next forward quantise and pack the weights again.  With
        config["mi355q_keep_master"] the fp32 weights / bias the layer was first given are restored here, so the caller
        reloads nothing; `config` switches the layer to another quantisation config (other widths) on the way.  Without a
        master copy the caller loads new fp32 values into .weight / .bias first (after a first forward they hold
        quantised values)."""
        if config is not None:
            keep = {k: v for k, v in self.config.items() if k.startswith("mi355q_") and k not in config}
            self.config = dict(config, **keep)
            self.bypass = self.config.get("bypass", False)
            self.is_ptq = self.config.get("is_ptq", False)
            self.align = self.config.get("mi355q_align", "auto")
            if not self.bypass:
                self._setup_quantizers(self.config)
        if self._master is not None:
            with torch.no_grad():
                if self._fp32_released:
                    self.weight.data = torch.empty_like(self._master[0])
                    self._fp32_released = False
                self.weight.copy_(self._master[0])
                if self.bias is not None:
                    self.bias.copy_(self._master[1])
        elif self._fp32_released:
            raise RuntimeError("mi355q: requantize() needs fp32 weights: they were released and no master copy is kept")
        self.weight_requires_quantisation = True if self.is_ptq else False
        self._packed, self._align_mode, self._calls, self._row_overflows = None, None, 0, 0
        self._w_bf16, self._w_packed, self._pending_flavour, self._mixed = None, None, None, None
        self._x_cap = policy.initial_x_cap(self.align)

    @torch.no_grad()
    def pack_now(self, x_sample=None):
        """Quantise and pack the weights NOW instead of at the first forward (a loader calls this right after it filled
        .weight / .bias: pack at load).  Without an activation sample the activation route is decided at
        the first forward."""
        if self.bypass or not self.is_ptq or not self.weight_requires_quantisation:
            return self
        probe = x_sample if x_sample is not None else torch.empty(1, self.in_features, device=self.weight.device)
        self._quantise_weights_once(pack=self._int8_plan(probe) is not None, x_sample=x_sample)
        return self

    def release_fp32_weight(self):
        """Drop the fp32 copy of the (already packed) weights: what stays resident is the packed operand -- with
        config["mi355q_weight_storage"] = "packed" width + 0.5 bits per value.  .weight becomes an empty Parameter;
        only the packed routes work afterwards (requantize() brings the weights back if a master copy is kept)."""
        if self._packed is None:
            raise RuntimeError("mi355q: nothing packed yet (run a forward or pack_now() first)")
        # the MX route's exact in-launch fallback reads the fp32 weights: that operand goes with them
        self._mx_w = None
        self.weight.data = torch.empty(0, dtype=self.weight.dtype, device=self.weight.device)
        self._packed = (self._packed[0], self._packed[1], self.weight._version, self._packed[3])
        if self._w_bf16 is not None:
            self._w_bf16 = (self._w_bf16[0], self.weight._version)
        self._fp32_released = True
        return self

    def weight_storage_bits(self) -> float:
        """bits per weight value of what the layer keeps packed (excluding the fp32 Parameter, see release_fp32_weight)"""
        if self._w_packed is not None:
            return self._w_packed.bits_per_value()
        if self._packed is None:
            return 32.0
        n = self.out_features * self.in_features
        if self._packed[0] is not None:
            wa = self._packed[0]
            return 8.0 * (wa.tiled.numel() + wa.exp.numel()) / n
        return 8.0 * self._packed[1].numel() / n

    def forward(self, x):
        from ...sharded import ShardedRows
        if isinstance(x, ShardedRows):
            # the gathered output of a row-sharded layer, still in the collective's rank-major layout: the row-aligned int8
            # route reads it in place; every other route takes the re-assembled tensor
            if self._settled() and self._on_row_route():
                plan = self._int8_plan(x.buf[0])
                if plan is not None:
                    with torch.no_grad():
                        return self._forward_int8(x, plan)
            x = x.dense()
        from ...sharded import ShardedTiledBf16
        if isinstance(x, ShardedTiledBf16):
            if x.pre_applied is not None:
                raise RuntimeError(f"mi355q: a quantised gather that applied {x.pre_applied!r} reached forward(); call forward_after")
            return self._forward_quantised_gather(x)
        if self.bypass:
            ops.count_vendor_gemm("linear.bypass")
            return F.linear(x, self.weight, self.bias)
        if self.is_ptq:
            plan = self._int8_plan(x)
            differentiated = torch.is_grad_enabled() and x.requires_grad      # (someone wants d/dx through this layer)
            with torch.no_grad():
                if self.weight_requires_quantisation:
                    self._quantise_weights_once(pack=plan is not None, x_sample=x)
                elif self._pending_flavour is not None:
                    self._finalise_packed_flavour(x)
                p = self._packed
                if (plan is not None and p is not None and p[1].device != self.weight.device
                        and p[2] == self.weight._version and (self.bias is None or p[3] == self.bias._version)):
                    self._repack_quantised_weights(x)        # the module was moved: same (quantised) values, new device
                if plan is not None and self._mx_w is not None and self._mx_takes(x):
                    return self._forward_mx(x)
                if plan is not None and self._packed_is_current():
                    if self._small_m_takes(x):
                        return self._forward_small_m(x)
                    return self._forward_int8(x, plan)
                if not differentiated and self._values_exact_in_bf16(x):
                    return self._forward_bf16_values(x)
                if not differentiated and self._padded_block_fp_ok(x):
                    return self._forward_block_fp_padded(x)
                x = self.x_quantizer(x)
            ops.count_vendor_gemm("linear.ptq_fallthrough")
            return F.linear(x, self.weight, self.bias)
        x = self.x_quantizer(x)
        w = self.w_quantizer(self.weight)
        bias = self.b_quantizer(self.bias) if self.bias is not None else None
        if self._qat_on_tile_gemm(x):
            return _TileLinear.apply(x, w, bias)
        ops.count_vendor_gemm("linear.qat_fp32")
        return F.linear(x, w, bias)

    def _small_m_takes(self, x) -> bool:
        """config["mi355q_small_m"] = "packed" (default "off"): a forward() of at most ops.SMALL_M_MAX rows on a layer that holds its
        weights at rest (`_w_packed`, either flavour: mi355q_weight_storage = "packed" / "hybrid") reads them straight from that form
        (ops.bfp_linear_packed_small) instead of expanding them into the tile GEMM's operand first.  Not the mixed contraction; larger
        batches, forward_after / forward_tiled / forward_residual and sharded inputs keep their routes."""
        return self._w_packed is not None and self._mixed is None and policy.small_m_takes(self.config, self.in_features, x.numel())

    def _forward_small_m(self, x):
        x2 = x.reshape(-1, self.in_features)
        y = ops.bfp_linear_packed_small(x2, self._w_packed, *self.consumer_quantiser(), self.bias, out=self._take_out(x2.shape[0]))
        return y.reshape(*x.shape[:-1], self.out_features)

    def _qat_on_tile_gemm(self, xq) -> bool:
        """QAT (is_ptq = False, linear.py:72-76: x, W and b re-quantised every call, straight-through gradients): the product
        F.linear(x_q, W_q, b_q) and its two backward products on the bf16 flavour of the tile GEMM instead of the library's fp32
        GEMM at a sixteenth of its rate -- when the quantised values are exact in bf16 (block_fp of <= 9 bits, minifloats of
        <= 7 mantissa bits, powers of two) and every contraction length is a whole number of 64-byte K-steps.
        config["mi355q_qat_gemm"] = "fp32" keeps F.linear."""
        if not (xq.is_cuda and xq.dtype == torch.float32 and self.weight.dtype == torch.float32):
            return False
        return policy.qat_on_tile_gemm(self.config, self.arith, self.in_features, self.out_features, xq.numel() // self.in_features,
                                       self.arith != "block_fp" and self._values_exact_in_bf16(xq))

    # -- W4A4 on the MX scaled matrix instruction ------------------------------------------------------------------------
    def _mx_config_ok(self) -> bool:
        """config["mi355q_mx"]: "auto" (default) -- block_fp operands of <= 4 bits each (every mantissa exact in FP6 e2m3 with
        three exponents of reach inside a 32-group; at 5 bits the reach is two and Gaussian data already trips it), [1,16] blocks
        along in_features, in_features % 128 == 0, launches of >= 192 tiles of 256 x 256 (below that the small-tile int8 kernel
        wins: profiles/r05_mx_w4a4.txt); True -- every launch that fits the format (<= 5 bits); False -- never"""
        return (policy.mx_config_ok(self.config, self.arith, self.is_ptq, self.bypass, self.in_features)
                and self.weight.is_cuda and self.weight.dtype == torch.float32 and not self._fp32_released)

    def _mx_takes(self, x) -> bool:
        if not (x.is_cuda and x.dtype == torch.float32 and 2 <= x.ndim <= 3) or self._mx_w is None or self._fp32_released:
            return False
        if self._mx_w.c16.device != x.device or self._mx_version != self.weight._version:
            return False
        return policy.mx_takes(self.config, x.numel() // self.in_features, self.out_features)

    def _forward_mx(self, x):
        x2 = x.reshape(-1, self.in_features).contiguous()
        xop = ops.block_fp_quantize_mx(x2, *self.consumer_quantiser())
        y = ops.mx_gemm(xop, self._mx_w, self.weight.data, self.bias)
        # a 32-group of the activations that does not fit the format sends the launch to its exact (slow) route: look at the
        # flag on a doubling schedule of calls and leave this route if it is ever up (never while a graph is being recorded)
        self._mx_calls += 1
        if self._mx_calls & (self._mx_calls - 1) == 0 and not _capturing_graph():
            if int(xop.bad[0]) != 0:
                self._mx_w = None
        return y.reshape(*x.shape[:-1], self.out_features)

    def _values_exact_in_bf16(self, xq) -> bool:   # (xq: the layer's input, quantised or not: only its placement matters)
        """block_minifloat / block_log PTQ layers (linear.py:145-203; likewise the un-blocked minifloat_ieee / minifloat_denorm
        and integer ones, :104-110, 206-263): the fake-quantised values -- minifloats with at most 7 mantissa bits, signed
        powers of two, fixed point of at most 9 bits -- are exact in bf16 and a product of two of them exact in fp32, so
        `F.linear(x_q, W_q, b_q)` is the bf16 flavour of the tile GEMM (fp32 accumulation, fp32 output) instead of a
        library fp32 GEMM at a seventh of its rate.  config["mi355q_values_gemm"] = "fp32" keeps F.linear."""
        return (policy.values_exact_in_bf16(self.config, self.arith, self.in_features) and xq.is_cuda and xq.dtype == torch.float32
                and self.weight.dtype == torch.float32 and xq.ndim >= 2 and not self.weight_requires_quantisation)

    @torch.no_grad()
    def _forward_quantised_gather(self, x):
        """x: sharded.ShardedTiledBf16 -- this layer's operand as the ranks quantised and gathered it (one tiled bf16 segment
        per rank): the bf16 flavour of the tile GEMM with x in column segments against the tiled quantised weights"""
        c = self.config
        if (self.arith != "block_fp" or self.bypass or not self.is_ptq
                or x.quantiser != self.consumer_quantiser() or x.features != self.in_features):
            raise RuntimeError("mi355q: this quantised gather was prepared for another layer / quantiser")
        if not 2 <= c["weight_width"] <= 9:
            raise RuntimeError(f"mi355q: a quantised gather feeds the bf16 tile GEMM, whose operands hold block_fp values of at most 9 "
                               f"bits exactly; this layer's weight_width is {c['weight_width']} (shard it with gather='dense')")
        if self.weight_requires_quantisation:
            self._quantise_weights_once(pack=False)          # (linear.py:66-70: weights and bias quantised in place; no int8 operand needed)
        wt = self._tiled_bf16_weights(x.device, released="take the bf16 route")
        M = 1
        for d in x.lead:
            M *= int(d)
        P = x.buf.shape[0]
        y = ops.bf16_gemm_tiled(x.buf if P > 1 else x.buf[0], wt, M, self.out_features, self.in_features, self.bias,
                                segments=P)
        return y.reshape(*x.lead, self.out_features)

    def _padded_block_fp_ok(self, x) -> bool:
        """block_fp layers whose in_features is a multiple of the block (16) but not of the tile kernels' K-step (64): the
        contraction is padded with all-zero blocks -- they quantise to zeros and add nothing -- and runs on the bf16 flavour of
        the tile GEMM (a block_fp value of width <= 9 is exact in bf16, products exact in fp32) instead of dropping to the
        library fp32 GEMM.  config["mi355q_pad_k"] = False keeps F.linear."""
        return (x.is_cuda and x.dtype == torch.float32 and self.weight.dtype == torch.float32 and not self.weight_requires_quantisation
                and policy.padded_block_fp_ok(self.config, self.arith, self.in_features, self.out_features, x.ndim,
                                              x.shape[-2] if x.ndim == 3 else 0))

    def _forward_block_fp_padded(self, x):
        K = self.in_features
        Kp = (K + 63) // 64 * 64
        x2 = F.pad(x.reshape(-1, K), (0, Kp - K))
        w = self.__dict__.get("_w_bf16_padded")
        if w is None or w[1] != self.weight._version or w[0].device != x.device:
            w = self.__dict__["_w_bf16_padded"] = (ops.bf16_tile(F.pad(self.weight.data, (0, Kp - K))), self.weight._version)
        xt = ops.block_fp_quantize_bf16_tiled(x2, *self.consumer_quantiser())
        y = ops.bf16_gemm_tiled(xt, w[0], x2.shape[0], self.out_features, Kp, self.bias)
        return y.reshape(*x.shape[:-1], self.out_features)

    def _forward_bf16_values(self, x):
        """x (NOT yet quantised) -> x quantiser -> tiled bf16 -> tile GEMM against the tiled quantised weights"""
        c = self.config
        x2 = x.reshape(-1, self.in_features).contiguous()
        wt = self._tiled_bf16_weights(x.device, contiguous=True)
        xs = [1, self.in_features] if x.ndim == 2 else [1, x.shape[-2], self.in_features]
        if (self.arith == "block_minifloat" and x.ndim <= 3
                and ops.resolve_blocking(xs, c["data_in_block_size"], True)[3:] == (1, 16)):
            # one pass: the block_minifloat values straight into the tiled bf16 operand
            xt = ops.block_minifloat_quantize_bf16_tiled(x2, c["data_in_width"], c["data_in_exponent_width"],
                                                         c["data_in_exponent_bias_width"])
        else:
            # (block_log's all-zero blocks take their value from a reduction over the whole tensor: its own two launches)
            xt = ops.bf16_tile(self.x_quantizer(x).reshape(-1, self.in_features).contiguous())
        y = ops.bf16_gemm_tiled(xt, wt, x2.shape[0], self.out_features, self.in_features, self.bias)
        return y.reshape(*x.shape[:-1], self.out_features)

    def forward_after(self, x, op, other=None, residual=None):
        """self(relu(x)) (op = "relu": OPT's fc2 behind its activation_fn, modeling_opt.py:412-420) or
        self(silu(x) * other) (op = "silu_mul": Llama's down_proj, modeling_llama.py:216) with the elementwise step read by
        the layer's x quantiser itself -- the reference runs it as torch kernels whose result the quantiser reads back
        (three passes over the [tokens, ffn] tensor instead of one).  Same arithmetic, rounded to fp32 operation by
        operation; whenever the fused quantisers do not apply (first PTQ forward, QAT, bypass, other arithmetics, the
        group flavour) the step runs as torch ops in front of forward().  `residual`: residual + the result (forward_residual)."""
        from ...sharded import ShardedRows, ShardedTiledBf16
        if residual is not None:
            if isinstance(x, (ShardedRows, ShardedTiledBf16)):
                return residual + self.forward_after(x, op, other)
            y = self._forward_after(x, op, other, residual)
            return y
        return self._forward_after(x, op, other, None)

    def _forward_after(self, x, op, other, residual):
        from ...sharded import ShardedRows, ShardedTiledBf16
        if op not in ("relu", "silu_mul") or ((op == "silu_mul") != (other is not None) and not isinstance(x, ShardedTiledBf16)):
            raise ValueError("forward_after: op is 'relu' (no other) or 'silu_mul' (with other)")
        if isinstance(x, ShardedTiledBf16):
            if x.pre_applied != op:
                raise RuntimeError(f"mi355q: a quantised gather that applied {x.pre_applied!r} reached forward_after({op!r})")
            return self._forward_quantised_gather(x)
        if isinstance(x, ShardedRows):
            # fc1's gathered output in the collective's rank-major layout (sharded.shard_model(gather="segments")): the
            # row-aligned route reads the P segments in place with the relu in front; anything else re-assembles it
            if op == "relu" and self._settled() and self._on_row_route():
                plan = self._int8_plan(x.buf[0])
                if plan is not None:
                    with torch.no_grad():
                        return self._forward_int8(x, plan, pre=("relu", None))
            x = x.dense()
        # (a layer packed when its weights arrived still carries both flavours: its first forward must see the POST-op
        #  activations to settle the route and drop the other one -- ADVICE r3 -- so it goes through forward() once)
        fused = (self._settled() and x.is_cuda and x.dtype == torch.float32 and not (torch.is_grad_enabled() and (x.requires_grad or (
                     other is not None and other.requires_grad)))
                 and (other is None or (other.shape == x.shape and other.dtype == x.dtype and other.device == x.device)))
        if fused:
            plan = self._int8_plan(x)
            fused = plan is not None and self._align_mode == "rows"
        if fused:
            with torch.no_grad():
                o2 = None if other is None else other.reshape(-1, self.in_features)
                if residual is not None and self._residual_fits(x, residual):
                    return self._forward_int8(x, plan, pre=(op, o2), residual=residual)
                y = self._forward_int8(x, plan, pre=(op, o2))
            return y if residual is None else residual + y
        y = self(F.relu(x) if op == "relu" else F.silu(x) * other)
        return y if residual is None else residual + y

    def _bf16_weight_operand(self, device):
        """the quantised weights as the tiled bf16 operand of the per-block-exponent route"""
        if self._w_packed is not None and not self._w_packed.row_scale_flavour:
            return self._w_packed.expand()                   # width-bit storage -> scratch tiled bf16
        return self._tiled_bf16_weights(device, released="switch routes")

    def _residual_fits(self, x, residual) -> bool:
        """can `residual + self(x)` run as one launch?  (the per-block-exponent route's product adds it in its stores)"""
        return (residual is not None and torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and self._settled()
                and self._int8_plan(x) is not None and (self._uses_bf16_route() or self._residual_rides_the_int8_product())
                and self._residual_operand_ok(residual, x.shape[:-1]) and residual.device == x.device
                and not (torch.is_grad_enabled() and x.requires_grad))

    def _residual_rides_the_int8_product(self) -> bool:
        """the row-scale int8 route in its one-launch form (ops.bfp_gemm_aligned(residual=...), round 6): 120-entry activation buckets,
        K a multiple of 128, not the mixed contraction; dense input (a ShardedRows input keeps the separate add)"""
        return (self._align_mode == "rows" and self._mixed is None and self._packed is not None
                and policy.residual_rides_the_int8_product(self.in_features, self._x_cap))

    def _residual_operand_ok(self, residual, lead) -> bool:
        """`residual` can ride in a product's stores (mi355q_bf16_gemm_tiled_res): fp32, contiguous, [.., out_features]"""
        return (torch.is_tensor(residual) and residual.is_cuda and residual.dtype == torch.float32 and residual.is_contiguous()
                and tuple(residual.shape) == tuple(lead) + (self.out_features,) and self.out_features % 4 == 0
                and residual.data_ptr() % 16 == 0 and not (torch.is_grad_enabled() and residual.requires_grad))

    def _consumer_product(self, xt, rows, lead, residual, device):
        """this layer's product on the per-block route from its OWN quantised activations as a tiled bf16 buffer, reshaped to
        [*lead, out_features]; `residual` rides in the stores where it can (`_residual_operand_ok`) and is added behind otherwise"""
        with torch.no_grad():
            res2 = residual.reshape(-1, self.out_features) if residual is not None and self._residual_operand_ok(residual, lead) else None
            y = ops.bf16_gemm_tiled(xt, self._bf16_weight_operand(device), rows, self.out_features, self.in_features, self.bias,
                                    out=self._take_out(rows), residual=res2)
        y = y.reshape(*lead, self.out_features)
        return y if residual is None or res2 is not None else residual + y

    @staticmethod
    def _norm_pre(norm):
        """`norm` = (weight, eps): LlamaRMSNorm, (weight, bias, eps): nn.LayerNorm -> the activation quantisers' `pre=`"""
        if norm is None:
            return None
        return ("rmsnorm", norm[0], norm[1]) if len(norm) == 2 else ("layernorm", norm[0], norm[2], norm[1])

    def forward_residual(self, x, residual):
        """residual + self(x) (modeling_llama.py:259, modeling_opt.py:375, 425: the add a decoder layer puts behind o_proj / fc2) --
        in the product's stores where the layer runs on the per-block-exponent route (same bits), as two steps otherwise"""
        if self._residual_fits(x, residual):
            with torch.no_grad():
                return self._forward_int8(x, self._int8_plan(x), residual=residual)
        return residual + self(x)

    def accepts_tiled_input(self) -> bool:
        """can a producer hand this layer its quantised activations as a tiled bf16 operand (`forward_tiled`)?  block_fp PTQ on the
        per-block-exponent route with its weights packed: the attention pass then writes o_proj's operand itself."""
        return (self._settled() and self._uses_bf16_route() and self.config["data_in_width"] <= 9 and self.in_features % 32 == 0
                and ops.resolve_blocking([1, self.in_features], self.config["data_in_block_size"], True)[3:] == (1, 16))

    def consumer_quantiser(self):
        """(width, exponent width, exponent bias) of this layer's activation quantiser, for a producer that applies it"""
        c = self.config
        return (c["data_in_width"], c["data_in_exponent_width"], c["data_in_exponent_bias"])

    def forward_tiled(self, xt, lead, residual=None):
        """self(x) [+ residual] for x given as `ops.TiledBf16` [rows, in_features] -- this layer's OWN quantised activations, formed by
        the producer (ops.bfp_attention(consumer=self.consumer_quantiser())): the per-block product alone.  `lead`: the leading shape
        of the result (rows = prod(lead))."""
        assert self.accepts_tiled_input() and xt.cols == self.in_features
        return self._consumer_product(xt.buf, xt.rows, lead, residual, xt.buf.device)

    def _take_out(self, rows):
        """where the caller wants this call's product stored (sharded.RowShardedLinear: its rank's segment of the all-gather buffer,
        so that the collective runs in place), once; None: a fresh tensor"""
        out, self._out_hint = self.__dict__.get("_out_hint"), None
        if out is not None and out.shape == (rows, self.out_features) and out.dtype == torch.float32 and out.is_contiguous():
            return out
        return None

    def _forward_int8(self, x, plan, pre=None, residual=None):
        quantiser = self.consumer_quantiser()
        from ...sharded import ShardedRows
        segments = isinstance(x, ShardedRows)                  # (forward() sends these here on the row-aligned route only)
        x2 = x.buf if segments else x.reshape(-1, self.in_features)
        if self._uses_bf16_route():
            # Activations (or weights) no row window fits: every block keeps its exponent.  A block_fp value of width <= 9
            # is exact in bf16 and a product of two of them exact in fp32, so the product is the bf16 flavour of the tile
            # GEMM (fp32 accumulation, fp32 output): x through the HIP quantiser straight into tiled bf16, the in-place
            # quantised weights tiled once.  |x| <= 1e-8 pass-through elements are rounded to bf16 there (<= 2e-11 each).
            # config["mi355q_blocks_gemm"] = "int8": the blockwise-exact int8 kernel instead (exact integer block dots,
            # several times slower).
            wt = self._bf16_weight_operand(x.device)
            xt = ops.block_fp_quantize_bf16_tiled(x2.contiguous(), *quantiser, pre=pre)
            y = ops.bf16_gemm_tiled(xt, wt, x2.shape[0], self.out_features, self.in_features, self.bias, out=self._take_out(x2.shape[0]),
                                    residual=None if residual is None else residual.reshape(-1, self.out_features))
            return y.reshape(*x.shape[:-1], self.out_features)
        if self._mixed is not None and self._mixed["version"] == self._versions():
            return self._forward_mixed(x, x2, segments, pre, residual)
        assert residual is None or not segments, "a residual behind a segmented input: the caller adds"
        # one fused kernel: quantise + pack + row-align + tile
        xa = ops.block_fp_quantize_aligned_rows(x2, *quantiser, bucket_cap=self._x_cap, pre=pre, segments=segments)
        wa = self._w_packed.expand() if self._w_packed is not None else self._packed[0]
        y = ops.bfp_gemm_aligned(xa, wa, self.bias, out=self._take_out(x2.shape[0]),
                                 residual=None if residual is None else residual.reshape(-1, self.out_features))
        if self.align == "auto" and self._x_cap != ops.ROW_NO_ALIGN and self._overflow_repeats(xa.sparse):
            self._x_cap = ops.ROW_NO_ALIGN                    # activations stopped fitting: no alignment from now on
        return y.reshape(*x.shape[:-1], self.out_features)

    def _overflow_repeats(self, sparse) -> bool:
        """results never depend on the mode (an overflowing exception bucket only sends the GEMM to its slow blockwise kernel, the
        mixed launch to its exact fallback): look at the overflow word on a doubling schedule of calls, and say when it was up
        twice -- the layer then leaves row mode (not while a HIP graph is being recorded: the read is a host synchronisation)"""
        if ops._capturing():
            return False
        self._calls += 1
        if self._calls & (self._calls - 1) == 0 and int(sparse[0]) != 0:
            self._row_overflows += 1
            return self._row_overflows >= 2
        return False

    def _forward_mixed(self, x, x2, segments, pre, residual):
        """the mixed contraction: one pass of the class-aware quantiser over x, one launch of the tile kernel (class 0 on the int8
        MFMA, class 1 on the bf16 MFMA); an elementwise step in front, row segments or a residual behind run as torch ops here"""
        m = self._mixed
        if segments:
            x2 = x.dense().reshape(-1, self.in_features)
        if pre is not None:
            x2 = F.relu(x2) if pre[0] == "relu" else F.silu(x2) * pre[1].reshape(-1, self.in_features)
        x0, x1 = ops.block_fp_quantize_classes(x2, m["classes"], *self.consumer_quantiser(), bucket_cap=self._x_cap)
        y = ops.bfp_gemm_mixed(x0, m["wa0"], x1, m["w1"], m["classes"].K1, self.bias, out=self._take_out(x2.shape[0]))
        assert y is not None, "mi355q: the mixed contraction was chosen for a shape the library does not take"
        if self.align == "auto" and self._overflow_repeats(x0.sparse):
            self._mixed, self._x_cap = None, ops.ROW_NO_ALIGN     # (as on the row route; from now on the per-block route)
        lead = x.shape[:-1]
        y = y.reshape(*lead, self.out_features)
        return y if residual is None else residual + y

    @classmethod
    def from_float(cls, linear_fp32: nn.Linear, config: dict):
        linear = cls(linear_fp32.in_features, linear_fp32.out_features, bias=linear_fp32.bias is not None,
                     config=config)
        with torch.no_grad():
            linear.weight.copy_(linear_fp32.weight)
            if linear.bias is not None:
                linear.bias.copy_(linear_fp32.bias)
        return linear

    def __repr__(self):
        return "{}(in_features={}, out_features={}, bias={}, bypass={}, is_ptq={}, x/w/b-width={}/{}/{})".format(
            self.__class__.__name__, self.in_features, self.out_features, self.bias is not None, self.bypass,
            self.is_ptq, self.config["data_in_width"], self.config["weight_width"],
            self.config.get("bias_width", "NA"))


def _linear_class(name: str, arith: str):
    return type(name, (_LinearBase,), {"arith": arith, "__module__": __name__,
                                       "__doc__": f"nn.Linear with {arith} input / weight / bias quantisers"})


LinearBlockFP = _linear_class("LinearBlockFP", "block_fp")
LinearBlockMinifloat = _linear_class("LinearBlockMinifloat", "block_minifloat")
LinearBlockLog = _linear_class("LinearBlockLog", "block_log")
LinearInteger = _linear_class("LinearInteger", "integer")
LinearLog = _linear_class("LinearLog", "log")
LinearMinifloatDenorm = _linear_class("LinearMinifloatDenorm", "minifloat_denorm")
LinearMinifloatIEEE = _linear_class("LinearMinifloatIEEE", "minifloat_ieee")

from .linear_fused import FP32_SPLIT_MIN_ROWS, fp32_linear, gated_mlp, grouped_linear, relu_mlp  # noqa: E402,F401  (written on _LinearBase)
