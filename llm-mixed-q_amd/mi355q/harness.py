"""Minimal OPT-style and Llama-style decoder harnesses over the registry API, and the perplexity loop.

NOT a port of the reference's HF model files (those are callers of the path and out of scope,
SURVEY.md section 2 rows 8-9): this is just enough model to drive the hot path the way
`OPTQuantizedDecoderLayer` does -- q/k/v/out_proj, fc1, fc2 through `get_quantized_cls("linear")`,
the two attention products through `get_quantized_func("bmm")`, 3-D inputs into the attention
projections, 2-D into the MLP, an unquantised lm_head (reference modeling_opt.py:143-330, 333-441,
934-1109) -- so that loss / perplexity parity of the HIP path can be checked on model-shaped random
weights (no checkpoint or Wikitext2 copy exists in this environment).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .quantize import fp32_linear, gated_mlp, get_quantized_cls, get_quantized_func, grouped_linear, relu_mlp
from .quantize.model_quant_config import parse_llama_quantized_config, parse_opt_quantized_config


def _attention_consumer(c1: dict, proj, hs, B: int):
    """(width, exponent width, exponent bias) of the out-projection's activation quantiser when the attention pass may write that
    layer's operand itself (config["mi355q_fused_attention_output"]; ops.bfp_attention(consumer=...)): one batch element, heads not
    sharded, the Linear on the per-block route -- else None"""
    if not c1.get("mi355q_fused_attention_output", False) or hs is not None or B != 1:
        return None
    ok = getattr(proj, "accepts_tiled_input", None)
    return proj.consumer_quantiser() if ok is not None and ok() else None


def _one_pass_attention(c0: dict, c1: dict) -> str:
    """which one-pass attention function config["mi355q_fused_attention"] of the second product switches on: "block_fp" (the second
    product is block_fp: attention_block_fp with its consumer / rotary / token-major shortcuts), "block_minifloat" (BOTH products are
    block_minifloat: attention_block_minifloat, plain fp32 output and none of the shortcuts), or None (knob off or absent, any other
    format)"""
    if not c1.get("mi355q_fused_attention", False):
        return None
    if c1["name"] == "block_fp":
        return "block_fp"
    return "block_minifloat" if c0.get("name") == c1["name"] == "block_minifloat" else None


def _project_attention_output(o, proj, out, B, T, width, residual):
    """out_proj / o_proj behind the attention function: on its tiled operand (ops.TiledBf16) where the pass wrote one"""
    if isinstance(o, ops.TiledBf16):
        return proj.forward_tiled(o, (B, T), residual=residual)
    return out(o.transpose(1, 2).reshape(B, T, width))


@dataclass
class TinyOPTConfig:
    vocab_size: int = 512
    hidden_size: int = 256
    ffn_dim: int = 1024
    num_layers: int = 2
    num_heads: int = 4
    max_positions: int = 128
    init_std: float = 0.02        # HF OPT initializer range (modeling_opt.py:472-477)


def expand_quant_config(config: dict, num_layers: int) -> dict:
    """TOML-level dict -> per-layer node configs, as the reference's `parse_opt_quantized_config`
    (quant_config_opt.py:61-113: [default], optional [linear] / [bmm], [model_layer], [model_layer_<i>]).  A bare
    [default] body (a dict with a "name" key) is accepted as shorthand for {"default": body}."""
    if "default" not in config and "name" in config:
        config = {"default": dict(config)}
    return parse_opt_quantized_config(config, num_layers)


class _Attention(nn.Module):
    def __init__(self, cfg: TinyOPTConfig, qc: dict):
        super().__init__()
        self.h, self.nh, self.hd = cfg.hidden_size, cfg.num_heads, cfg.hidden_size // cfg.num_heads
        self.scaling = self.hd ** -0.5
        self.qc = qc
        for name in ("q_proj", "k_proj", "v_proj", "out_proj"):
            setattr(self, name, get_quantized_cls("linear", qc[name])(self.h, self.h, bias=True, config=qc[name]))

    def forward(self, x, mask, norm=None, residual=None, key_mask=None):
        """`residual`: returns residual + attention (config["mi355q_fused_residual"] of out_proj: the add in out_proj's stores where
        that layer's route has it, Linear.forward_residual).
        `key_mask` [B, T]: a padded batch (the model's attention_mask); `mask` is then the dense [B, 1, T, T] mask it stands for."""
        out_ = lambda o: self.out_proj(o) if residual is None else self.out_proj.forward_residual(o, residual)
        # head-sharded (sharded.shard_model(heads=True)): q / k / v arrive as this rank's heads only, the core runs on those, and
        # ONE all-gather of its output stands in front of out_proj
        hs = getattr(self, "mi355q_head_shard", None)
        if hs is None:
            out = out_
        else:
            from .sharded import gather_heads
            out = lambda o: out_(gather_heads(o, hs[0], hs[1]))
        B, T, _ = x.shape
        nh = self.nh if hs is None else self.q_proj.local.out_features // self.hd
        shape = lambda t: t.view(B, T, nh, self.hd).transpose(1, 2).contiguous().view(B * nh, T, self.hd)
        c1 = self.qc["bmm_1"]
        one_pass = _one_pass_attention(self.qc["bmm_0"], c1)
        if one_pass is not None:
            # both products, the mask and the softmax in one pass per 16 queries (the harness' mask is the causal one); the
            # kernel reads the [heads, T, hd] views of the projections in place: no `_shape(...).contiguous()` copies
            heads = lambda t: t.view(B, T, nh, self.hd).transpose(1, 2)
            if c1.get("mi355q_grouped_linear", False):       # q / k / v projections: one quantisation, one GEMM launch
                qp, kp, vp = grouped_linear(x, (self.q_proj, self.k_proj, self.v_proj), norm=norm)
            else:
                qp, kp, vp = self.q_proj(x), self.k_proj(x), self.v_proj(x)
            # (q * scaling, modeling_opt.py:231: formed where the attention pass packs its Q fragments -- q_scale)
            pad = {} if key_mask is None else {"key_mask": key_mask}
            o = get_quantized_func("attention", c1)(heads(qp), heads(kp), heads(vp), self.qc["bmm_0"], c1, causal=True,
                                                    q_scale=self.scaling, **pad,
                                                    consumer=_attention_consumer(c1, self.out_proj, hs, B) if one_pass == "block_fp" else None)
            return _project_attention_output(o, self.out_proj, out, B, T, nh * self.hd, residual)
        q = shape(self.q_proj(x) * self.scaling)
        k, v = shape(self.k_proj(x)), shape(self.v_proj(x))
        w = get_quantized_func("bmm", self.qc["bmm_0"])(q, k.transpose(1, 2), config=self.qc["bmm_0"])
        if c1["name"] in ("block_fp", "block_minifloat") and c1.get("mi355q_fused_softmax", False) and key_mask is None:
            # mask add, clamp and softmax folded into the product kernel (the harness' mask is the causal one)
            o = get_quantized_func("softmax_bmm", c1)(w, v, config=c1, causal=True)
        else:
            w = w.view(B, nh, T, T) + mask
            w = torch.max(w, w.new_full((), torch.finfo(w.dtype).min)).view(B * nh, T, T)
            p = F.softmax(w, dim=-1)
            o = get_quantized_func("bmm", c1)(p, v, config=c1)
        o = o.view(B, nh, T, self.hd).transpose(1, 2).reshape(B, T, nh * self.hd)
        return out(o)

    def decode(self, x, state, idx):
        """the new tokens' attention against the cache of layer `idx` (DecodeState): the reference's `past_key_value` branch
        (modeling_opt.py:208-245) -- projections of the new tokens only, keys and values appended, then the core"""
        if getattr(self, "mi355q_head_shard", None) is not None:
            raise NotImplementedError("incremental decoding of head-sharded models")
        B, n, _ = x.shape
        heads = lambda t: t.view(B, n, self.nh, self.hd).transpose(1, 2)
        q, k, v = heads(self.q_proj(x) * self.scaling), heads(self.k_proj(x)), heads(self.v_proj(x))
        o = state.attend(idx, q, k, v, self.qc["bmm_0"], self.qc["bmm_1"], None, "bmm")
        return self.out_proj(o.transpose(1, 2).reshape(B, n, self.nh * self.hd))


class _DecoderLayer(nn.Module):
    def __init__(self, cfg: TinyOPTConfig, qc: dict):
        super().__init__()
        self.self_attn = _Attention(cfg, qc["self_attn"])
        self.self_attn_layer_norm = nn.LayerNorm(cfg.hidden_size)
        self.final_layer_norm = nn.LayerNorm(cfg.hidden_size)
        self.fc1 = get_quantized_cls("linear", qc["fc1"])(cfg.hidden_size, cfg.ffn_dim, bias=True, config=qc["fc1"])
        self.fc2 = get_quantized_cls("linear", qc["fc2"])(cfg.ffn_dim, cfg.hidden_size, bias=True, config=qc["fc2"])

    def forward(self, x, mask, key_mask=None):
        c1 = self.self_attn.qc["bmm_1"]
        pad = {} if key_mask is None else {"key_mask": key_mask}
        fused_norm = (self.fc1.config.get("mi355q_fused_norm", False) and c1.get("mi355q_grouped_linear", False)
                      and _one_pass_attention(self.self_attn.qc["bmm_0"], c1) is not None)
        ln = lambda m: (m.weight, m.bias, m.eps)
        fres = self.fc2.config.get("mi355q_fused_residual", False)      # the residual adds in out_proj's / fc2's stores
        if fused_norm:      # the LayerNorms are applied by the quantiser of the projections they feed (grouped_linear(norm=...))
            x = self.self_attn(x, mask, norm=ln(self.self_attn_layer_norm), residual=x, **pad) if fres else x + self.self_attn(x, mask, norm=ln(self.self_attn_layer_norm), **pad)
        else:
            x = self.self_attn(self.self_attn_layer_norm(x), mask, residual=x, **pad) if fres else x + self.self_attn(self.self_attn_layer_norm(x), mask, **pad)
        shape = x.shape
        h = x.reshape(-1, shape[-1])                       # the MLP sees a 2-D activation (modeling_opt.py:412)
        if fused_norm and self.fc2.config.get("mi355q_fused_activation", False):
            # round 6: fc1's product with relu and fc2's quantiser in its store epilogue (relu_mlp); None when the layers do not
            # qualify (fc1 not on the row-scale int8 route, fc2 not on the per-block route ...): the launches below, as before
            hr = h.contiguous()
            y = relu_mlp(h, self.fc1, self.fc2, norm=ln(self.final_layer_norm), residual=hr if fres else None)
            if y is not None:
                return (y if fres else h + y).view(shape)
        if fused_norm:
            f1 = grouped_linear(h, (self.fc1,), norm=ln(self.final_layer_norm))[0]
        else:
            f1 = None
        if self.fc2.config.get("mi355q_fused_activation", False):    # relu read by fc2's x quantiser (Linear.forward_after)
            f = f1 if fused_norm else self.fc1(self.final_layer_norm(h))
            h = self.fc2.forward_after(f, "relu", residual=h.contiguous()) if fres else h + self.fc2.forward_after(f, "relu")
        elif fused_norm:
            h = h + self.fc2(F.relu(f1))
        else:
            h = h + self.fc2(F.relu(self.fc1(self.final_layer_norm(h))))
        return h.view(shape)

    def decode(self, x, state, idx):
        x = x + self.self_attn.decode(self.self_attn_layer_norm(x), state, idx)
        shape = x.shape
        h = x.reshape(-1, shape[-1])
        return (h + self.fc2(F.relu(self.fc1(self.final_layer_norm(h))))).view(shape)


class TinyOPTForCausalLM(nn.Module):
    def __init__(self, cfg: TinyOPTConfig, quant_config: dict):
        super().__init__()
        self.cfg = cfg
        self.embed_tokens = nn.Embedding(cfg.vocab_size, cfg.hidden_size)
        self.embed_positions = nn.Embedding(cfg.max_positions, cfg.hidden_size)
        self.layers = nn.ModuleList(_DecoderLayer(cfg, quant_config[f"model_layer_{i}"]) for i in range(cfg.num_layers))
        self.final_layer_norm = nn.LayerNorm(cfg.hidden_size)
        self.lm_head = nn.Linear(cfg.hidden_size, cfg.vocab_size, bias=False)     # not quantised (modeling_opt.py:942-944)
        self.mi355q_lm_head = "split"
        self.mi355q_pad_position = None          # row 1 of the reference's position table: a pad position's embedding (forward)
        self.apply(self._init)

    def _init(self, m):
        if isinstance(m, nn.Linear):
            m.weight.data.normal_(0.0, self.cfg.init_std)
            if m.bias is not None:
                m.bias.data.zero_()
        elif isinstance(m, nn.Embedding):
            m.weight.data.normal_(0.0, self.cfg.init_std)

    @torch.no_grad()
    def load_reference_state_dict(self, sd: dict):
        """load a state dict with the reference's (HF OPT) names: `model.decoder.` prefix, learned positions stored
        with an offset of 2 (modeling_opt.py:115-140)"""
        own = {}
        for k, v in sd.items():
            k = k.removeprefix("model.decoder.")
            v = torch.as_tensor(v)
            if k == "embed_positions.weight":
                self.mi355q_pad_position = v[1].detach().clone().float()
            own[k] = v[2:2 + self.cfg.max_positions] if k == "embed_positions.weight" else v
        self.load_state_dict(own, strict=True)
        return self

    def reference_state_dict(self) -> dict:
        """this model's parameters under the reference's names (inverse of load_reference_state_dict)"""
        out = {}
        for k, v in self.state_dict().items():
            v = v.detach()
            if k == "embed_positions.weight":
                head = torch.zeros(2, v.shape[1], dtype=v.dtype, device=v.device)
                if self.mi355q_pad_position is not None:
                    head[1] = self.mi355q_pad_position.to(device=v.device, dtype=v.dtype)
                v = torch.cat([head, v])
            out[k if k.startswith("lm_head") else "model.decoder." + k] = v
        return out

    def forward(self, input_ids, labels=None, cache=None, counts=None, attention_mask=None):
        """`cache` (a DecodeState): input_ids holds only the NEW tokens, whose positions start at the cache's length; returns their
        logits (the prompt goes through the same call).  None: the whole sequence, as ever.
        `counts` (with a cache): a ragged batch -- input_ids [B, n] is right-padded and row b holds counts[b] real tokens, at
        positions lengths[b] .. lengths[b] + counts[b] - 1 of ITS sequence; logits at padded positions are unspecified.
        `attention_mask` [B, T], non-zero = a real token (full forward only): a padded batch as the reference runs it -- pad positions
        stay in every operand and quantiser block, every layer's softmax masks them as keys (the registry's attention(key_mask=...)),
        and the learned positions count real tokens only.  None: today's call."""
        if cache is not None:
            _refuse_mask_with_cache(attention_mask)
            return _forward_cached(self, input_ids, labels, cache, counts)
        if counts is not None:
            raise ValueError("forward(counts=...) belongs to a cached call (cache=DecodeState)")
        B, T = input_ids.shape
        if attention_mask is None:
            pos = torch.arange(T, device=input_ids.device)
            x = self.embed_tokens(input_ids) + self.embed_positions(pos)[None]
            mask = torch.full((T, T), torch.finfo(x.dtype).min, device=x.device).triu(1)[None, None]
            pad = {}
        else:
            key_mask = _check_attention_mask(attention_mask, input_ids)
            # the reference's learned positions (modeling_opt.py:115-140): cumsum(mask) * mask - 1, plus an offset of 2 into its table.  A
            # pad position gets -1, i.e. row 1 of that table, which lies in the two offset rows this model's table drops: kept by
            # load_reference_state_dict as mi355q_pad_position, zeros (what reference_state_dict writes there) for a model made here
            live = key_mask != 0
            pos = (torch.cumsum(live.long(), dim=1) * live.long() - 1).clamp_(min=0)
            pad_row = self.mi355q_pad_position
            pad_row = torch.zeros(self.cfg.hidden_size, device=input_ids.device) if pad_row is None else pad_row.to(input_ids.device)
            x = self.embed_tokens(input_ids) + torch.where(live[..., None], self.embed_positions(pos), pad_row)
            neg = torch.finfo(x.dtype).min
            mask = (torch.full((T, T), neg, device=x.device).triu(1)[None, None]
                    + torch.where(key_mask != 0, 0.0, neg).to(x.dtype)[:, None, None, :]).clamp_(min=neg)      # (HF's expanded [B, 1, T, T] mask)
            pad = {"key_mask": key_mask}
        for layer in self.layers:
            x = layer(x, mask, **pad)
        # (unquantised, modeling_opt.py:942-944: fp32-equivalent on the bf16 MFMA -- quantized_modules.linear.fp32_linear; "vendor" = F.linear)
        logits = fp32_linear(self.final_layer_norm(x), self.lm_head, self.mi355q_lm_head)
        loss = None
        if labels is not None:
            loss = F.cross_entropy(logits[:, :-1].reshape(-1, logits.shape[-1]), labels[:, 1:].reshape(-1))
        return logits, loss


@dataclass
class TinyLlamaConfig:
    vocab_size: int = 512
    hidden_size: int = 256
    intermediate_size: int = 512
    num_layers: int = 2
    num_heads: int = 4
    max_positions: int = 128
    rms_eps: float = 1e-6
    init_std: float = 0.02
    attention_sinks: int = None    # attention sinks (StreamingLLM; needs sliding_window): the first `attention_sinks` keys stay visible, 0 .. 16; None: none
    sliding_window: int = None     # sliding-window attention (Mistral): a query sees its last `sliding_window` keys, its own included; None: all
    num_kv_heads: int = None       # grouped-query attention: K / V heads, each shared by num_heads // num_kv_heads query heads; None: num_heads

    def __post_init__(self):
        w = self.sliding_window
        if w is not None and (isinstance(w, bool) or not isinstance(w, int) or w < 1):
            raise ValueError(f"TinyLlamaConfig: sliding_window = {w!r} is not an integer >= 1")
        s = self.attention_sinks
        if s is not None and (isinstance(s, bool) or not isinstance(s, int) or not 0 <= s <= ops.SINKS_MAX):
            raise ValueError(f"TinyLlamaConfig: attention_sinks = {s!r} is not an integer in 0 .. {ops.SINKS_MAX}")
        if s is not None and w is None:
            raise ValueError(f"TinyLlamaConfig: attention_sinks = {s!r} without sliding_window: sinks are what a windowed query keeps seeing")
        if self.num_kv_heads is not None and (self.num_kv_heads < 1 or self.num_heads % self.num_kv_heads != 0):
            raise ValueError(f"TinyLlamaConfig: num_kv_heads = {self.num_kv_heads} does not divide num_heads = {self.num_heads}")


def expand_llama_quant_config(config: dict, num_layers: int) -> dict:
    """the same through `parse_llama_quantized_config` (quant_config_llama.py:70-130)"""
    if "default" not in config and "name" in config:
        config = {"default": dict(config)}
    return parse_llama_quantized_config(config, num_layers)


class _RMSNorm(nn.Module):
    def __init__(self, n, eps):
        super().__init__()
        self.weight, self.eps = nn.Parameter(torch.ones(n)), eps

    def forward(self, x):
        v = x.to(torch.float32).pow(2).mean(-1, keepdim=True)
        return self.weight * (x * torch.rsqrt(v + self.eps)).to(x.dtype)


def _check_attention_mask(attention_mask, input_ids):
    """attention_mask [B, T] of the models' full forward -> the key mask the layers take (on input_ids' device)"""
    if not isinstance(attention_mask, torch.Tensor) or tuple(attention_mask.shape) != tuple(input_ids.shape):
        raise ValueError(f"forward(attention_mask=...): [B, T] = {tuple(input_ids.shape)} expected, got "
                         f"{tuple(attention_mask.shape) if isinstance(attention_mask, torch.Tensor) else type(attention_mask).__name__}")
    return (attention_mask != 0).to(device=input_ids.device, dtype=torch.int32).contiguous()


def _refuse_mask_with_cache(attention_mask):
    if attention_mask is not None:
        raise NotImplementedError("forward(cache=..., attention_mask=...): a cached call serves unequal sequences by DecodeState's ragged route "
                                  "(counts=), which keeps no pad key in the cache; attention_mask belongs to the full forward")


def _causal_mask(n: int, L: int, window, dtype, device, sinks=None):
    """the additive mask [n, L] of n queries at the last n of L positions (the offset of modeling_llama.py:53-79): finfo.min above the
    horizon and, with a sliding window, below it -- query i at p = L - n + i sees keys max(0, p - window + 1) .. p -- but for the first
    `sinks` columns, whose lower mask is lifted (attention sinks: keys 0 .. sinks - 1 stay visible up to the horizon)"""
    mask = torch.full((n, L), torch.finfo(dtype).min, device=device).triu(1 + L - n)
    if window is not None:
        below = torch.full((n, L), torch.finfo(dtype).min, device=device).tril(L - n - int(window))
        if sinks:
            below[:, :int(sinks)] = 0
        mask = mask + below
    return mask


def _repeat_kv(t, G: int):
    """[B, nkv, n, hd] -> [B, nkv * G, n, hd], head j a copy of KV head j // G (HF Llama's repeat_kv: expand + reshape)"""
    B, nkv, n, hd = t.shape
    return t[:, :, None].expand(B, nkv, G, n, hd).reshape(B, nkv * G, n, hd)


class _LlamaAttention(nn.Module):
    """Llama-style attention over the registry API the way the reference's LlamaQuantizedAttention drives it
    (modeling_llama.py:289-344): bias-free projections, rotary embedding through
    get_quantized_func("rotary_positional_encoding"), 4-D products through get_quantized_func("matmul").
    Grouped-query attention (cfg.num_kv_heads < cfg.num_heads): k_proj / v_proj make nkv heads, query head j uses KV head
    j // (nh // nkv) -- HF Llama's repeat_kv.  The full forward repeats k and v to nh heads right behind the head reshape; the cached
    route keeps nkv heads and passes the group size to the cache's attention functions."""

    def __init__(self, cfg: TinyLlamaConfig, qc: dict):
        super().__init__()
        self.h, self.nh, self.hd = cfg.hidden_size, cfg.num_heads, cfg.hidden_size // cfg.num_heads
        self.nkv = cfg.num_heads if cfg.num_kv_heads is None else cfg.num_kv_heads
        self.window = cfg.sliding_window
        self.qc = qc
        for name in ("q_proj", "k_proj", "v_proj", "o_proj"):
            out = self.nkv * self.hd if name in ("k_proj", "v_proj") else self.h
            setattr(self, name, get_quantized_cls("linear", qc[name])(self.h, out, bias=False, config=qc[name]))
        inv = 1.0 / (10000.0 ** (torch.arange(0, self.hd, 2).float() / self.hd))
        t = torch.arange(cfg.max_positions).float()
        emb = torch.cat([torch.outer(t, inv)] * 2, dim=-1)
        self.register_buffer("cos", emb.cos()[None, None], persistent=False)       # [1, 1, pos, hd]
        self.register_buffer("sin", emb.sin()[None, None], persistent=False)

    def forward(self, x, mask, position_ids, norm=None, residual=None, key_mask=None):
        """`key_mask` [B, T]: a padded batch (the model's attention_mask); `mask` is then the dense [B, 1, T, T] mask it stands for"""
        out_ = lambda o: self.o_proj(o) if residual is None else self.o_proj.forward_residual(o, residual)
        pad = {} if key_mask is None else {"key_mask": key_mask}
        hs = getattr(self, "mi355q_head_shard", None)         # (head-sharded: see _Attention.forward)
        if hs is None:
            out = out_
        else:
            from .sharded import gather_heads
            out = lambda o: out_(gather_heads(o, hs[0], hs[1]))
        B, T, _ = x.shape
        nh = self.nh if hs is None else self.q_proj.local.out_features // self.hd
        shape = lambda t: t.view(B, T, -1, self.hd).transpose(1, 2)
        if self.qc["matmul_1"].get("mi355q_grouped_linear", False):
            q, k, v = (shape(t) for t in grouped_linear(x, (self.q_proj, self.k_proj, self.v_proj), norm=norm))
        else:
            if norm is not None:
                # (the layer asked for the fused norm but this module's own knobs do not group the projections -- the knobs
                #  ride per node: the norm is applied here, the RMSNorm expression of the reference, never skipped)
                weight, eps = norm
                var = x.to(torch.float32).pow(2).mean(-1, keepdim=True)
                x = weight * (x * torch.rsqrt(var + eps)).to(x.dtype)
            q, k, v = shape(self.q_proj(x)), shape(self.k_proj(x)), shape(self.v_proj(x))
        if self.nkv != self.nh:
            k, v = _repeat_kv(k, self.nh // self.nkv), _repeat_kv(v, self.nh // self.nkv)
        rc = self.qc["rotary_positional_encoding"]
        c1 = self.qc["matmul_1"]
        # (sliding window: the fused causal paths take no additive mask, so a windowed model with T > W takes the mask route below)
        windowed = self.window is not None and T > self.window
        one_pass = None if windowed else _one_pass_attention(self.qc["matmul_0"], c1)
        fused = one_pass is not None
        if one_pass == "block_fp" and c1.get("mi355q_fused_rotary", False):
            # (the rotary embedding applied where the attention pass loads q and k: attention_block_fp(rope=...))
            o = get_quantized_func("attention", c1)(q, k, v, self.qc["matmul_0"], c1, causal=True, scale_div=math.sqrt(self.hd),
                                                    rope=(self.cos[:, :, :T], self.sin[:, :, :T], position_ids, rc),
                                                    consumer=_attention_consumer(c1, self.o_proj, hs, B), **pad)
            return _project_attention_output(o, self.o_proj, out, B, T, nh * self.hd, residual)
        q, k = get_quantized_func("rotary_positional_encoding", rc)(q, k, self.cos[:, :, :T], self.sin[:, :, :T],
                                                                   position_ids, config=rc)
        if fused:
            o = get_quantized_func("attention", c1)(q, k, v, self.qc["matmul_0"], c1, causal=True, scale_div=math.sqrt(self.hd), **pad,
                                                    consumer=_attention_consumer(c1, self.o_proj, hs, B) if one_pass == "block_fp" else None)
            return _project_attention_output(o, self.o_proj, out, B, T, nh * self.hd, residual)
        w = get_quantized_func("matmul", self.qc["matmul_0"])(q, k.transpose(2, 3), config=self.qc["matmul_0"])
        if c1["name"] in ("block_fp", "block_minifloat") and c1.get("mi355q_fused_softmax", False) and not windowed and key_mask is None:
            o = get_quantized_func("softmax_matmul", c1)(w / math.sqrt(self.hd), v, config=c1, causal=True)
        else:
            w = w / math.sqrt(self.hd) + mask
            w = torch.max(w, w.new_full((), torch.finfo(w.dtype).min))
            p = F.softmax(w, dim=-1, dtype=torch.float32).to(q.dtype)
            o = get_quantized_func("matmul", c1)(p, v, config=c1)
        return out(o.transpose(1, 2).reshape(B, T, nh * self.hd))

    def decode(self, x, state, idx, position_ids):
        """the new tokens' attention against the cache of layer `idx` (modeling_llama.py:282-306): the rotary embedding through the
        registry's function at the new positions, the TURNED k into the cache as in the reference, then the core.  Grouped-query
        attention: k, v stay [B, nkv, n, hd] -- the embedding is element-wise per head, so the turned k has the bits turning the
        repeated k would give -- and the state's caches hold nkv heads"""
        if getattr(self, "mi355q_head_shard", None) is not None:
            raise NotImplementedError("incremental decoding of head-sharded models")
        B, n, _ = x.shape
        heads = lambda t: t.view(B, n, -1, self.hd).transpose(1, 2)
        q, k, v = heads(self.q_proj(x)), heads(self.k_proj(x)), heads(self.v_proj(x))
        rc, end = self.qc["rotary_positional_encoding"], state.position_end(n)
        q, k = get_quantized_func("rotary_positional_encoding", rc)(q, k, self.cos[:, :, :end], self.sin[:, :, :end], position_ids, config=rc)
        o = state.attend(idx, q, k, v, self.qc["matmul_0"], self.qc["matmul_1"], math.sqrt(self.hd), "matmul")
        return self.o_proj(o.transpose(1, 2).reshape(B, n, self.nh * self.hd))


class _LlamaLayer(nn.Module):
    def __init__(self, cfg: TinyLlamaConfig, qc: dict):
        super().__init__()
        self.self_attn = _LlamaAttention(cfg, qc["self_attn"])
        self.input_layernorm = _RMSNorm(cfg.hidden_size, cfg.rms_eps)
        self.post_attention_layernorm = _RMSNorm(cfg.hidden_size, cfg.rms_eps)
        lin = lambda name, i, o: get_quantized_cls("linear", qc["mlp"][name])(i, o, bias=False, config=qc["mlp"][name])
        self.gate_proj = lin("gate_proj", cfg.hidden_size, cfg.intermediate_size)
        self.up_proj = lin("up_proj", cfg.hidden_size, cfg.intermediate_size)
        self.down_proj = lin("down_proj", cfg.intermediate_size, cfg.hidden_size)

    def forward(self, x, mask, position_ids, key_mask=None):
        gc = self.gate_proj.config
        pad = {} if key_mask is None else {"key_mask": key_mask}
        fused_norm = gc.get("mi355q_grouped_linear", False) and gc.get("mi355q_fused_norm", False)
        fres = self.down_proj.config.get("mi355q_fused_residual", False)      # the residual adds in o_proj's / down_proj's stores
        if fused_norm:      # the norms are applied by the quantiser of the projections they feed (grouped_linear(norm=...))
            n1, n2 = self.input_layernorm, self.post_attention_layernorm
            x = (self.self_attn(x, mask, position_ids, norm=(n1.weight, n1.eps), residual=x, **pad) if fres
                 else x + self.self_attn(x, mask, position_ids, norm=(n1.weight, n1.eps), **pad))
            if self.down_proj.config.get("mi355q_fused_activation", False):
                # round 6: gate / up interleaved in ONE product whose epilogue writes down_proj's quantised operand (gated_mlp); None
                # when the layers do not qualify: the grouped launch + the quantiser that reads silu(gate) * up, as before
                y = gated_mlp(x, self.gate_proj, self.up_proj, self.down_proj, norm=(n2.weight, n2.eps), residual=x if fres else None)
                if y is not None:
                    return y if fres else x + y
            gate, up = grouped_linear(x, (self.gate_proj, self.up_proj), norm=(n2.weight, n2.eps))
            if self.down_proj.config.get("mi355q_fused_activation", False):
                return self.down_proj.forward_after(gate, "silu_mul", up, residual=x) if fres else x + self.down_proj.forward_after(gate, "silu_mul", up)
            return x + self.down_proj(F.silu(gate) * up)
        x = (self.self_attn(self.input_layernorm(x), mask, position_ids, residual=x, **pad) if fres
             else x + self.self_attn(self.input_layernorm(x), mask, position_ids, **pad))
        h = self.post_attention_layernorm(x)
        if self.gate_proj.config.get("mi355q_grouped_linear", False):
            gate, up = grouped_linear(h, (self.gate_proj, self.up_proj))
        else:
            gate, up = self.gate_proj(h), self.up_proj(h)
        if self.down_proj.config.get("mi355q_fused_activation", False):    # silu(gate) * up read by down_proj's x quantiser
            return self.down_proj.forward_after(gate, "silu_mul", up, residual=x) if fres else x + self.down_proj.forward_after(gate, "silu_mul", up)
        return x + self.down_proj(F.silu(gate) * up)                      # (modeling_llama.py:208-240)

    def decode(self, x, state, idx, position_ids):
        x = x + self.self_attn.decode(self.input_layernorm(x), state, idx, position_ids)
        h = self.post_attention_layernorm(x)
        return x + self.down_proj(F.silu(self.gate_proj(h)) * self.up_proj(h))


class TinyLlamaForCausalLM(nn.Module):
    def __init__(self, cfg: TinyLlamaConfig, quant_config: dict):
        super().__init__()
        self.cfg = cfg
        self.embed_tokens = nn.Embedding(cfg.vocab_size, cfg.hidden_size)
        self.layers = nn.ModuleList(_LlamaLayer(cfg, quant_config[f"model_layer_{i}"]) for i in range(cfg.num_layers))
        self.norm = _RMSNorm(cfg.hidden_size, cfg.rms_eps)
        self.lm_head = nn.Linear(cfg.hidden_size, cfg.vocab_size, bias=False)
        self.mi355q_lm_head = "split"
        for m in self.modules():
            if isinstance(m, (nn.Linear, nn.Embedding)):
                m.weight.data.normal_(0.0, cfg.init_std)

    @torch.no_grad()
    def load_reference_state_dict(self, sd: dict):
        """load a state dict with the reference's (HF Llama) names: `model.` prefix, `layers.i.mlp.*` projections,
        `rotary_emb.inv_freq` buffers skipped (the tables are rebuilt from the same formula)"""
        own = {}
        for k, v in sd.items():
            k = k.removeprefix("model.").replace(".mlp.", ".")
            if k.endswith("rotary_emb.inv_freq"):
                continue
            own[k] = torch.as_tensor(v)
        self.load_state_dict(own, strict=True)
        return self

    def reference_state_dict(self) -> dict:
        out = {}
        for k, v in self.state_dict().items():
            for proj in ("gate_proj", "up_proj", "down_proj"):
                k = k.replace("." + proj, ".mlp." + proj)
            out[k if k.startswith("lm_head") else "model." + k] = v.detach()
        return out

    def forward(self, input_ids, labels=None, cache=None, counts=None, attention_mask=None):
        """`cache` (a DecodeState), `counts`, `attention_mask`: see TinyOPTForCausalLM.forward.  The positions stay 0 .. T - 1 for every
        row, padded or not (the reference's default position_ids, modeling_llama.py)."""
        if cache is not None:
            _refuse_mask_with_cache(attention_mask)
            return _forward_cached(self, input_ids, labels, cache, counts)
        if counts is not None:
            raise ValueError("forward(counts=...) belongs to a cached call (cache=DecodeState)")
        B, T = input_ids.shape
        position_ids = torch.arange(T, device=input_ids.device)[None].expand(B, T)
        x = self.embed_tokens(input_ids)
        mask = _causal_mask(T, T, self.cfg.sliding_window, x.dtype, x.device, self.cfg.attention_sinks)[None, None]
        pad = {}
        if attention_mask is not None:
            key_mask = _check_attention_mask(attention_mask, input_ids)
            neg = torch.finfo(x.dtype).min
            mask = (mask + torch.where(key_mask != 0, 0.0, neg).to(x.dtype)[:, None, None, :]).clamp_(min=neg)
            pad = {"key_mask": key_mask}
        for layer in self.layers:
            x = layer(x, mask, position_ids, **pad)
        # (unquantised, modeling_llama.py:772,866: fp32-equivalent on the bf16 MFMA -- quantized_modules.linear.fp32_linear; "vendor" = F.linear)
        logits = fp32_linear(self.norm(x), self.lm_head, self.mi355q_lm_head)
        loss = None
        if labels is not None:
            loss = F.cross_entropy(logits[:, :-1].reshape(-1, logits.shape[-1]), labels[:, 1:].reshape(-1))
        return logits, loss


# ---- incremental decoding ---------------------------------------------------------------------------------------------------
class DecodeState:
    """One cache per layer and the current length, for `model(new_ids, cache=state)`.
    mode "block_fp": ops.KVCache + the split-key decode kernel -- both attention products block_fp [1,16] with widths <= 9 and a
        head_dim the kernel takes, else ValueError here, naming the reason.
    mode "block": EACH layer gets the cache of its own format -- ops.KVCache where both products are block_fp (the calls of mode
        "block_fp", unchanged), ops.MinifloatKVCache where both are block_minifloat; any other format, a bypassed product or two
        formats in one layer: ValueError here, naming the layer.  A block_minifloat layer's prompt runs, behind its append, the
        registry steps of the layer's full forward (the products, the mask, the softmax) -- or, with config["mi355q_fused_attention"]
        of its second product, the registry's one-pass function (attention_block_minifloat).  What the block_minifloat cache has no kernel
        for is refused by name: extend=True, a sliding-window model, pages; a mixed call and more than 16 new tokens behind a non-empty
        cache keep raising NotImplementedError.
    mode "fp32": the reference's literal route for ANY arithmetic (modeling_llama.py:301-344): torch.cat of fp32 K / V per layer, the
        products through the registry's functions, the causal mask [n, L] with the offset of modeling_llama.py:53-79.
    Ragged batches (`model(ids, cache=state, counts=[...])`, mode "block_fp" only): `lengths` holds every sequence's own length on the
    host, and two int32 device tensors [batch x KV heads] hold them per cache row as the kernels read them -- "before" this call (every
    layer's append) and "after" it (every layer's decode; 0 for a row that takes no token in this call, which then costs nothing).
    They are shared by all layers and written once a call.  Each sequence decodes as if it were alone: no pad key ever enters a
    block of the cache.  The reference's left padding + attention_mask is NOT reproduced -- under block quantisation a pad key
    shares a 16-key block with real keys and moves their exponent.
    extend=True (mode "block_fp"; accepted and ignored by "fp32", which has no limit): chunked prefill.  Calls the default state
    refuses -- more than 16 new tokens behind a non-empty cache, a mixed call (one row starts its sequence while others continue),
    unequal counts behind non-empty rows -- run on ops.bfp_attention_extend: one ragged append, one extend call with every row's
    own length and its own number of queries.
    Grouped-query attention (k, v with fewer heads than q): the caches and the per-row tensors have batch x KV heads rows, the decode
    and extend functions get group = heads // KV heads; the prefill routes and mode "fp32" repeat k / v to the query heads at use
    (mode "fp32" concatenates them un-repeated).
    Sliding window (model.cfg.sliding_window = W; TinyLlama only): every route bounds a query to its last W keys.  Mode "block_fp" passes
    window= to the decode and extend functions; a prompt (or a ragged prefill with a row) longer than W runs on the windowed extend
    kernel behind its own append, whatever `extend` says -- the prefill attention function has no window; mode "fp32" adds the window to
    its additive mask.  A paged state gives back, after every call, the pages no later query can see (PagedKVCache.trim).
    Attention sinks (model.cfg.attention_sinks = S, with a sliding window): every route above passes sinks= next to window=, mode "fp32"
    lifts the mask's first S columns, and a paged state's trim keeps logical page 0.
    Paged caches: PagedDecodeState below (this constructor's parameters stay as they are)."""
    paged = False

    @property
    def cached(self) -> bool:
        """the layers hold quantised caches (modes "block_fp" and "block"; "fp32" keeps fp32 K / V tensors)"""
        return self.mode != "fp32"

    def __init__(self, model, batch: int, capacity: int, mode: str = "block_fp", extend: bool = False):
        from .quantize.quantized_functions import decode_cache_kind, decode_cache_params
        if mode not in ("block_fp", "block", "fp32"):
            raise ValueError(f"DecodeState: mode {mode!r} is neither 'block_fp' nor 'block' nor 'fp32'")
        if mode == "block":
            if extend:
                raise NotImplementedError("DecodeState(mode='block'): extend=True: no extend (chunked prefill) kernel reads the block_minifloat cache")
            if getattr(model.cfg, "sliding_window", None) is not None:
                raise NotImplementedError("DecodeState(mode='block'): a sliding-window model: no windowed kernel reads the block_minifloat cache")
            if self.paged:
                raise NotImplementedError("DecodeState(mode='block'): page_size: the block_minifloat cache is not paged")
        attns = [layer.self_attn for layer in model.layers]
        if any(getattr(a, "mi355q_head_shard", None) is not None for a in attns):
            raise NotImplementedError("incremental decoding of head-sharded models")
        self.mode, self.batch, self.length = mode, int(batch), 0
        self.window = getattr(model.cfg, "sliding_window", None)
        self.sinks = getattr(model.cfg, "attention_sinks", None) or None       # (0 is the plain window)
        self.extend = bool(extend) and mode == "block_fp"
        self.lengths, self.ragged, self._call = [0] * self.batch, self.paged, None
        self.capacity = (int(capacity) + 15) // 16 * 16
        if self.capacity > model.cfg.max_positions + 15:
            raise ValueError(f"DecodeState: capacity {capacity} exceeds the model's {model.cfg.max_positions} positions")
        self.kv = [None] * len(attns)
        if self.cached:
            dev = next(model.parameters()).device
            for i, a in enumerate(attns):
                c0, c1 = (a.qc["bmm_0"], a.qc["bmm_1"]) if "bmm_0" in a.qc else (a.qc["matmul_0"], a.qc["matmul_1"])
                try:
                    kind, qk, pv = ("block_fp",) + decode_cache_params(c0, c1, a.hd) if mode == "block_fp" else decode_cache_kind(c0, c1, a.hd)
                except ValueError as e:
                    raise ValueError(f"DecodeState(mode={mode!r}), layer {i}: {e}") from None
                rows = self.batch * getattr(a, "nkv", a.nh)
                self.kv[i] = self._new_cache(rows, a.hd, qk, pv, dev) if kind == "block_fp" else \
                    ops.MinifloatKVCache(rows, self.capacity, a.hd, qk, pv, dev)
            if len({getattr(a, "nkv", a.nh) for a in attns}) == 1:    # (else: no ragged use; the per-row tensors are one set for all layers)
                self.heads = getattr(attns[0], "nkv", attns[0].nh)    # cache rows a sequence: the KV heads
                self.rows_before, self.rows_after, self._rows_counts = (torch.zeros(self.batch * self.heads, dtype=torch.int32, device=dev)
                                                                        for _ in range(3))

    def _new_cache(self, rows, hd, qk, pv, dev):
        return ops.KVCache(rows, self.capacity, hd, qk, pv, dev)

    def reset(self) -> None:
        self.length = 0
        self.lengths, self.ragged, self._call = [0] * self.batch, self.paged, None
        for i, c in enumerate(self.kv):
            if self.cached:
                c.reset()
            else:
                self.kv[i] = None

    def release(self, b: int) -> None:
        """sequence b is finished: its length becomes 0, so that a new sequence can start in slot b while the others continue (with
        extend=True: the mixed route); paged caches give its pages back to every layer's pool.  Nothing is cleared."""
        if not self.cached:
            raise NotImplementedError("DecodeState.release with mode='fp32': its rows have one common length")
        if not 0 <= int(b) < self.batch:
            raise ValueError(f"DecodeState.release: sequence {b} outside 0 .. {self.batch - 1}")
        b = int(b)
        if self.paged:
            for c in self.kv:
                heads = c.B // self.batch
                c.release(range(b * heads, (b + 1) * heads))
        self.lengths[b] = 0
        self.length, self.ragged = max(self.lengths), True      # (from here on the rows differ in length: the ragged routes)

    def _copy_check(self, what: str, seqs) -> list:
        if not self.paged:
            raise NotImplementedError(f"DecodeState.{what}: only a paged state can fork or reorder its sequences (page_size=...: full pages are "
                                      "shared by reference, the contiguous caches would copy every row)")
        if self._call is not None:
            raise RuntimeError(f"DecodeState.{what} inside a cached call")
        seqs = [int(b) for b in seqs]
        if any(not 0 <= b < self.batch for b in seqs):
            raise ValueError(f"DecodeState.{what}: sequences {seqs} outside 0 .. {self.batch - 1}")
        return seqs

    def fork(self, src, dst) -> None:
        """sequence dst, which is empty, becomes a copy of sequence src where it stands (PagedKVCache.fork on the sequence's cache rows --
        its KV heads -- in every layer; src, dst may be equal-length lists: one launch a layer).  Every layer is checked before any
        changes: a fork the pools cannot serve raises RuntimeError and leaves the state as it was."""
        one = isinstance(dst, int)
        src, dst = self._copy_check("fork", [src] if one else src), self._copy_check("fork", [dst] if one else dst)
        if len(src) != len(dst) or any(self.lengths[d] for d in dst):
            raise ValueError(f"DecodeState.fork: {len(src)} sources for {len(dst)} sequences, which must be empty (lengths "
                             f"{[self.lengths[d] for d in dst]})")
        for dry in (True, False):
            for c in self.kv:
                heads = c.B // self.batch
                rows = lambda seqs: [b * heads + h for b in seqs for h in range(heads)]
                c.fork(rows(src), rows(dst), [self.lengths[b] for b in src for _ in range(heads)], dry_run=dry)
        for s_, d in zip(src, dst):
            self.lengths[d] = self.lengths[s_]
        self.length, self.ragged = max(self.lengths), True

    def reorder(self, beam_idx) -> None:
        """sequence b becomes what sequence beam_idx[b] was -- the reference's `_reorder_cache(past_key_values, beam_idx)` -- in every layer
        (PagedKVCache.reorder: one launch a layer), the host lengths with it.  Every layer is checked before any changes.  A
        sliding-window state works unchanged: the partial page is the newest and never trimmed, trimmed pages stay trimmed."""
        beam_idx = self._copy_check("reorder", beam_idx.tolist() if isinstance(beam_idx, torch.Tensor) else beam_idx)
        if len(beam_idx) != self.batch:
            raise ValueError(f"DecodeState.reorder: {len(beam_idx)} indices for a batch of {self.batch}")
        for dry in (True, False):
            for c in self.kv:
                heads = c.B // self.batch
                c.reorder([b * heads + h for b in beam_idx for h in range(heads)], [l for l in self.lengths for _ in range(heads)], dry_run=dry)
        self.lengths = [self.lengths[b] for b in beam_idx]
        self.length, self.ragged = max(self.lengths), True

    def position_end(self, n: int) -> int:
        """rows of the rotary tables a call with n new tokens reads"""
        return (max(self.lengths) if self._call is not None else self.length) + n

    def begin_ragged(self, counts, n: int, max_positions: int):
        """One ragged call: checks, the route, and the per-row tensors -- before any layer's cache is written.  -> positions [B, n]
        (host list of lists; padded positions repeat the row's last one)"""
        if not self.cached:
            raise NotImplementedError("counts= with mode='fp32': the reference serves unequal prompts by left padding + attention_mask, "
                                      "which under block quantisation gives different numbers (a pad key shares a 16-key block of K^T "
                                      "with real keys and moves their exponent); ragged batches run on the block_fp cache only")
        if not hasattr(self, "rows_before"):
            raise NotImplementedError("ragged batches of a model whose layers differ in their number of heads")
        counts = [int(c) for c in counts]
        if len(counts) != self.batch or any(not 0 <= c <= n for c in counts):
            raise ValueError(f"forward(counts=...): {len(counts)} counts outside 0 .. {n} for a batch of {self.batch}")
        before = list(self.lengths)
        after = [l + c for l, c in zip(before, counts)]
        if max(after) > min(self.capacity, max_positions) or max(before) + n > self.capacity:
            raise ValueError(f"forward(counts=...): lengths {before} + {n} tokens exceed the capacity {self.capacity} "
                             f"or the model's {max_positions} positions")
        active = [b for b, c in enumerate(counts) if c > 0]
        if all(l == 0 for l in before) or (active and all(before[b] == 0 for b in active)):
            route = "prefill"                                  # (also: sequences that start in released slots while NO other row takes a token)
        elif all(before[b] > 0 and counts[b] == n for b in active) and n <= ops.DECODE_MAX_QUERIES:
            route = "decode"
        elif self.extend:
            route = "extend"                                   # (mixed, unequal counts, n > 16: every row at its own (length, count))
        elif any(before[b] == 0 for b in active):
            raise NotImplementedError(f"a mixed call: rows {[b for b in active if before[b] == 0]} start a sequence while others continue theirs "
                                      "(prefill and decode in one call)")
        elif n > ops.DECODE_MAX_QUERIES:
            raise NotImplementedError(f"{n} new tokens behind non-empty block_fp cache rows (at most {ops.DECODE_MAX_QUERIES} a call)")
        else:
            raise NotImplementedError(f"unequal counts {counts} behind non-empty rows: the decode kernel takes the same number of "
                                      "queries for every row that takes any")
        rows = lambda xs: torch.tensor(xs, dtype=torch.int32).repeat_interleave(self.heads)
        if self.paged:      # pages for every layer, checked for all of them before any table changes (and before any cache is written)
            need = rows(after).tolist()
            for c in self.kv:
                c.ensure(need, dry_run=True)
            for c in self.kv:
                c.ensure(need)
        self.rows_before.copy_(rows(before))
        self.rows_after.copy_(rows([a if c > 0 else 0 for a, c in zip(after, counts)]))      # (a row without a token: no decode work)
        self._rows_counts.copy_(rows(counts))
        self._call = dict(route=route, counts=counts, after=after, max_before=max(before), max_after=max(after))
        self.ragged = True
        return [[min(l + j, max(l + c - 1, 0)) for j in range(n)] for l, c in zip(before, counts)]

    def end_ragged(self) -> None:
        self.lengths, self._call = self._call["after"], None
        self.length = max(self.lengths)
        if self.paged and self.window is not None:
            # sliding window: the pages wholly behind every later query's window go back to the pool, in every layer
            for c in self.kv:
                heads = c.B // self.batch
                c.trim([l for l in self.lengths for _ in range(heads)], self.window, self.sinks or 0)

    def _reference_steps(self, q, k, v, c0, c1, scale_div, style):
        """the reference's steps (modeling_llama.py:309-344) for n queries at the last n of k's L positions: the two products through
        the registry's functions, the causal mask [n, L] with the offset of modeling_llama.py:53-79 -- what mode "fp32" runs on its
        concatenated K / V and what a block_minifloat layer's prompt runs in mode "block"""
        B, nh, n, hd = q.shape
        if k.shape[1] != nh:                                    # (grouped queries: the un-repeated K / V are kept, repeated at use)
            k, v = _repeat_kv(k, nh // k.shape[1]), _repeat_kv(v, nh // k.shape[1])
        L = k.shape[2]
        if style == "bmm":
            fold = lambda t: t.reshape(B * nh, t.shape[2], hd)
            q, k, v = fold(q), fold(k), fold(v)
        w = get_quantized_func(style, c0)(q, k.transpose(-1, -2), config=c0)
        if scale_div:
            w = w / scale_div
        mask = _causal_mask(n, L, self.window, w.dtype, w.device, self.sinks)
        w = torch.max(w + mask, w.new_full((), torch.finfo(w.dtype).min))
        p = F.softmax(w, dim=-1, dtype=torch.float32).to(q.dtype)
        return get_quantized_func(style, c1)(p, v, config=c1).view(B, nh, n, hd)

    def _attend_ragged(self, idx, q, k, v, c0, c1, scale_div, style="matmul"):
        B, nh, n, hd = q.shape
        call, cache = self._call, self.kv[idx]
        gq = {} if k.shape[1] == nh else dict(group=nh // k.shape[1])      # (grouped queries: k, v have the KV heads only)
        if self.window is not None:
            gq["window"] = self.window
            if self.sinks:
                gq["sinks"] = self.sinks
        full = all(c == n for c in call["counts"])
        cache.append(k, v, lengths=self.rows_before, counts=None if full else self._rows_counts, max_length=call["max_before"])
        if call["route"] == "decode":
            return get_quantized_func("attention_decode", c1)(q, cache, c0, c1, causal=True, scale_div=scale_div, lengths=self.rows_after,
                                                              max_length=call["max_after"], **gq).reshape(B, nh, n, hd)
        if call["route"] == "extend" or (call["route"] == "prefill" and self.window is not None and max(call["counts"]) > self.window):
            # (a windowed prefill with a row longer than the window: the extend kernel behind the append -- a row that starts at 0 is the
            #  row whose queries are all its keys; max_length bounds the lengths and must hold the n query columns, which may all be padding behind the largest count)
            return get_quantized_func("attention_extend", c1)(q, cache, c0, c1, causal=True, scale_div=scale_div, lengths=self.rows_after,
                                                              counts=self._rows_counts, max_length=max(call["max_after"], n), **gq
                                                              ).reshape(B, nh, n, hd)
        if "group" in gq:
            k, v = _repeat_kv(k, gq["group"]), _repeat_kv(v, gq["group"])
        # ragged prefill: every sequence's own queries against its own keys, one call of the existing attention function each (what
        # the sequence alone runs); prefill is not the hot path here
        o = q.new_zeros(B, nh, n, hd)
        for b, c in enumerate(call["counts"]):
            if c and isinstance(cache, ops.MinifloatKVCache) and not c1.get("mi355q_fused_attention", False):
                # (config["mi355q_fused_attention"] off: the layer's full-forward steps; on: attention_block_minifloat below)
                o[b, :, :c] = self._reference_steps(q[b:b + 1, :, :c], k[b:b + 1, :, :c], v[b:b + 1, :, :c], c0, c1, scale_div, style)[0]
            elif c:
                o[b, :, :c] = get_quantized_func("attention", c1)(q[b:b + 1, :, :c], k[b:b + 1, :, :c], v[b:b + 1, :, :c], c0, c1, causal=True,
                                                                  scale_div=scale_div).reshape(nh, c, hd)
        return o

    def attend(self, idx, q, k, v, c0, c1, scale_div, style):
        """q, k, v [B, heads, n, hd] of the new tokens (q scaled / turned already) -> attention output [B, heads, n, hd]"""
        B, nh, n, hd = q.shape
        if self._call is not None:
            return self._attend_ragged(idx, q, k, v, c0, c1, scale_div, style)
        if self.length + n > self.capacity:
            raise ValueError(f"DecodeState: {self.length} + {n} tokens exceed the capacity {self.capacity}")
        if self.cached:
            cache = self.kv[idx]
            assert cache.length == self.length
            wide = self.length and n > ops.DECODE_MAX_QUERIES
            if wide and not self.extend:                        # (before the append: a refused call leaves every layer's cache as it was)
                raise NotImplementedError(f"{n} new tokens behind a non-empty block_fp cache (at most {ops.DECODE_MAX_QUERIES} a call)")
            cache.append(k, v)
            gq = {} if k.shape[1] == nh else dict(group=nh // k.shape[1])  # (grouped queries: k, v have the KV heads only)
            if self.window is not None:
                gq["window"] = self.window
                if self.sinks:
                    gq["sinks"] = self.sinks
                wide = wide or (self.length == 0 and n > self.window)      # (a prompt longer than the window: the windowed extend kernel)
            if self.length == 0 and isinstance(cache, ops.MinifloatKVCache) and not c1.get("mi355q_fused_attention", False):
                # the prompt of a block_minifloat layer without config["mi355q_fused_attention"]: the steps of the layer's full forward
                # (with it: attention_block_minifloat below, as a block_fp layer's prompt takes attention_block_fp)
                return self._reference_steps(q, k, v, c0, c1, scale_div, style)
            if self.length == 0 and not wide:
                # the prompt's own queries against the prompt: the existing attention function (M = n)
                if "group" in gq:
                    k, v = _repeat_kv(k, gq["group"]), _repeat_kv(v, gq["group"])
                return get_quantized_func("attention", c1)(q, k, v, c0, c1, causal=True, scale_div=scale_div).reshape(B, nh, n, hd)
            return get_quantized_func("attention_extend" if wide else "attention_decode", c1)(q, cache, c0, c1, causal=True,
                                                                                              scale_div=scale_div, **gq).reshape(B, nh, n, hd)
        if self.kv[idx] is not None:
            k, v = torch.cat([self.kv[idx][0], k], dim=2), torch.cat([self.kv[idx][1], v], dim=2)
        self.kv[idx] = (k, v)
        return self._reference_steps(q, k, v, c0, c1, scale_div, style)


class PagedDecodeState(DecodeState):
    """DecodeState(model, batch, capacity, mode, extend) on paged caches: with `page_size` (a power of two >= 32; mode "block_fp" only)
    every layer gets an ops.PagedKVCache of `num_pages` pages (default: enough for every row at `capacity`) with max_pages =
    ceil(capacity / page_size) -- `num_pages` may be far below batch x capacity, a sequence holds pages for the keys it has.  Every
    call runs through the ragged routes (a call without counts is the call with counts = [n] * batch); pages are handed out for ALL
    layers before any cache is written (a call the pool cannot serve raises RuntimeError and leaves every layer as it was); and
    `release(b)` gives sequence b's pages back, so that a new sequence can start in slot b on them.  The numbers are the contiguous
    state's, bit for bit.  page_size=None builds exactly a DecodeState."""

    def __init__(self, model, batch: int, capacity: int, mode: str = "block_fp", extend: bool = False, page_size: int = None,
                 num_pages: int = None):
        self.paged = page_size is not None
        if self.paged and mode == "block":
            raise NotImplementedError("PagedDecodeState(mode='block'): page_size: the block_minifloat cache is not paged")
        if self.paged and mode != "block_fp":
            raise ValueError("PagedDecodeState: page_size belongs to mode 'block_fp' (the fp32 route is not paged)")
        if num_pages is not None and not self.paged:
            raise ValueError("PagedDecodeState: num_pages without page_size")
        if self.paged and len({getattr(layer.self_attn, "nkv", layer.self_attn.nh) for layer in model.layers}) != 1:
            # (a paged state runs every call through the ragged routes, whose per-row tensors are one set for all layers)
            raise NotImplementedError("PagedDecodeState: paged caches for a model whose layers differ in their number of KV heads")
        self.page_size, self.num_pages = page_size, num_pages
        super().__init__(model, batch, capacity, mode, extend)

    def _new_cache(self, rows, hd, qk, pv, dev):
        if not self.paged:
            return super()._new_cache(rows, hd, qk, pv, dev)
        max_pages = -(-self.capacity // int(self.page_size))
        return ops.PagedKVCache(rows, hd, qk, pv, dev, page_size=self.page_size, max_pages=max_pages,
                                num_pages=rows * max_pages if self.num_pages is None else self.num_pages)


def _refuse_beyond_mantissa_cache(cls, model, mode, extend):
    """the three refusals every state on a mantissa cache opens with: what no kernel of the storage serves, by the state's name and by
    what the class calls its storage (STORAGE; a plural where the state chooses among several)"""
    name, noun = cls.__name__, cls.STORAGE
    if mode != "block_fp":
        is_a = "are block_fp caches" if noun.endswith("s") else "is a block_fp cache"
        raise ValueError(f"{name}: mode {mode!r}: the {noun} {is_a} (mode 'fp32' keeps fp32 K / V)")
    if extend:
        raise NotImplementedError(f"{name}: extend=True: no extend (chunked prefill) kernel reads the {noun}")
    if getattr(model.cfg, "sliding_window", None) is not None:
        raise NotImplementedError(f"{name}: a sliding-window model: no windowed kernel reads the {noun}")


class PackedDecodeState(DecodeState):
    """DecodeState(model, batch, capacity, mode) on ops.PackedKVCache: every layer's K and V as int8 mantissas with one exponent byte
    per block of 16, 17/32 of the cache bytes and of a decode step's K / V traffic.  The numbers are DecodeState's, bit for bit
    (ops.PackedKVCache names the one exception, inputs of magnitude <= 1e-8).  What the packed cache has no kernel for is refused
    here, by name: extend=True (chunked prefill), a sliding-window model, and mode "fp32", which has no quantised cache at all.  A
    prompt runs the prefill attention function on its fp32 K / V, as in DecodeState: it reads no cache."""

    STORAGE = "int8-mantissa cache"

    def __init__(self, model, batch: int, capacity: int, mode: str = "block_fp", extend: bool = False):
        _refuse_beyond_mantissa_cache(type(self), model, mode, extend)
        super().__init__(model, batch, capacity, mode, extend)

    def _new_cache(self, rows, hd, qk, pv, dev):
        try:
            return ops.PackedKVCache(rows, self.capacity, hd, qk, pv, dev)
        except ValueError as e:
            raise ValueError(f"PackedDecodeState: {e}") from None


class NibbleDecodeState(DecodeState):
    """DecodeState(model, batch, capacity, mode) on ops.NibbleKVCache: every layer's K and V as 4-bit mantissas, two to a byte, with one
    exponent byte per block of 16 -- 9/32 of the cache bytes and of a decode step's K / V traffic, for models whose cached attention
    operands all have width <= 4 (else ValueError here, naming the width).  The numbers are DecodeState's and PackedDecodeState's, bit
    for bit (ops.PackedKVCache names the one exception, inputs of magnitude <= 1e-8).  What the nibble cache has no kernel for is
    refused here, by name: extend=True (chunked prefill), a sliding-window model, and mode "fp32", which has no quantised cache at all."""

    STORAGE = "4-bit-mantissa cache"

    def __init__(self, model, batch: int, capacity: int, mode: str = "block_fp", extend: bool = False):
        _refuse_beyond_mantissa_cache(type(self), model, mode, extend)
        super().__init__(model, batch, capacity, mode, extend)

    def _new_cache(self, rows, hd, qk, pv, dev):
        try:
            return ops.NibbleKVCache(rows, self.capacity, hd, qk, pv, dev)
        except ValueError as e:
            raise ValueError(f"NibbleDecodeState: {e}") from None


class NarrowestDecodeState(DecodeState):
    """DecodeState(model, batch, capacity, mode) with the narrowest storage EACH layer allows, for a model whose layers differ in their
    attention widths: ops.NibbleKVCache where both cached operands (the y sides of the layer's two products) have width <= 4, else
    ops.PackedKVCache where both have width <= 8, else ops.KVCache.  `kinds` says which layer got what: a list of "nibble" / "int8" /
    "bf16", one entry per layer.  The three storages give the same bits for the same keys, so the numbers are DecodeState's.
    Contiguous only, and the refusals of the packed states, by name: extend=True, a sliding-window model, mode "fp32"."""

    STORAGE = "mantissa caches"

    def __init__(self, model, batch: int, capacity: int, mode: str = "block_fp", extend: bool = False):
        _refuse_beyond_mantissa_cache(type(self), model, mode, extend)
        self.kinds = []
        super().__init__(model, batch, capacity, mode, extend)

    def _new_cache(self, rows, hd, qk, pv, dev):
        widest = max(int(qk[3]), int(pv[3]))
        kind, cls = ("nibble", ops.NibbleKVCache) if widest <= 4 else ("int8", ops.PackedKVCache) if widest <= 8 else ("bf16", ops.KVCache)
        self.kinds.append(kind)
        return cls(rows, self.capacity, hd, qk, pv, dev)


class PagedPackedDecodeState(PagedDecodeState):
    """PagedDecodeState(model, batch, capacity, mode, extend, page_size, num_pages) on ops.PagedPackedKVCache: paged caches of int8
    mantissas, 17/32 of the paged state's K and V bytes and of a decode step's K / V traffic, with its release / fork / reorder and its
    ragged prefill and decode routes as inherited -- the numbers are PagedDecodeState's, bit for bit (ops.PackedKVCache names the one
    exception, inputs of magnitude <= 1e-8).  `page_size` is mandatory.  What this storage has no kernel for is refused here, by name:
    extend=True (chunked prefill), a sliding-window model, and mode "fp32"; a mixed call and a call with more than 16 new tokens behind
    a non-empty row therefore keep raising DecodeState's NotImplementedError."""

    STORAGE = PackedDecodeState.STORAGE

    def __init__(self, model, batch: int, capacity: int, mode: str = "block_fp", extend: bool = False, page_size: int = None,
                 num_pages: int = None):
        if mode == "block_fp" and page_size is None:        # (behind the refusal of another mode, in front of the other two)
            raise ValueError("PagedPackedDecodeState: page_size is mandatory (the contiguous int8-mantissa state is PackedDecodeState)")
        _refuse_beyond_mantissa_cache(type(self), model, mode, extend)
        super().__init__(model, batch, capacity, mode, extend, page_size, num_pages)

    def _new_cache(self, rows, hd, qk, pv, dev):
        max_pages = -(-self.capacity // int(self.page_size))
        try:
            return ops.PagedPackedKVCache(rows, hd, qk, pv, dev, page_size=self.page_size, max_pages=max_pages,
                                          num_pages=rows * max_pages if self.num_pages is None else self.num_pages)
        except ValueError as e:
            raise ValueError(f"PagedPackedDecodeState: {e}") from None


def _forward_cached(model, input_ids, labels, state: DecodeState, counts=None):
    if labels is not None:
        raise ValueError("forward(cache=...): labels belong to the full forward")
    B, n = input_ids.shape
    if B != state.batch:
        raise ValueError(f"forward(cache=...): batch {B}, the cache was made for {state.batch}")
    if counts is None and state.ragged:
        counts = [n] * B                                    # (a state whose rows differ in length has no common position range)
    if counts is not None:
        # ragged: per-row positions; the route is chosen and refused before any layer's cache is written
        position_ids = torch.tensor(state.begin_ragged(counts, n, model.cfg.max_positions), dtype=torch.long).to(input_ids.device)
        try:
            if isinstance(model, TinyOPTForCausalLM):
                x = model.embed_tokens(input_ids) + model.embed_positions(position_ids)
                for i, layer in enumerate(model.layers):
                    x = layer.decode(x, state, i)
                x = model.final_layer_norm(x)
            else:
                x = model.embed_tokens(input_ids)
                for i, layer in enumerate(model.layers):
                    x = layer.decode(x, state, i, position_ids)
                x = model.norm(x)
        except BaseException:
            state._call = None
            raise
        state.end_ragged()
        return fp32_linear(x, model.lm_head, model.mi355q_lm_head), None
    if state.length + n > model.cfg.max_positions:
        raise ValueError(f"forward(cache=...): {state.length} + {n} tokens exceed the model's {model.cfg.max_positions} positions")
    pos = torch.arange(state.length, state.length + n, device=input_ids.device)
    if isinstance(model, TinyOPTForCausalLM):
        x = model.embed_tokens(input_ids) + model.embed_positions(pos)[None]
        for i, layer in enumerate(model.layers):
            x = layer.decode(x, state, i)
        x = model.final_layer_norm(x)
    else:
        position_ids = pos[None].expand(B, n).contiguous()
        x = model.embed_tokens(input_ids)
        for i, layer in enumerate(model.layers):
            x = layer.decode(x, state, i, position_ids)
        x = model.norm(x)
    state.length += n
    state.lengths = [state.length] * B
    return fp32_linear(x, model.lm_head, model.mi355q_lm_head), None


# generate's kv_storage: the state class and what its refusals call the storage
_KV_STORAGES = {"int8": (PackedDecodeState, PackedDecodeState.STORAGE), "nibble": (NibbleDecodeState, NibbleDecodeState.STORAGE),
                "narrowest": (NarrowestDecodeState, "per-layer choice of " + NarrowestDecodeState.STORAGE)}


def _new_state(model, batch, capacity, mode, extend, page_size, num_pages, kv_storage=None):
    if kv_storage is not None:
        if kv_storage not in _KV_STORAGES:
            raise ValueError(f"generate: kv_storage = {kv_storage!r} is neither None (bf16 values) nor 'int8' (mantissa bytes) nor 'nibble' "
                             "(4-bit mantissas) nor 'narrowest' (per layer, the narrowest of the three its widths allow)")
        if page_size is not None or num_pages is not None:
            raise NotImplementedError(f"generate: kv_storage={kv_storage!r} with page_size / num_pages: the {_KV_STORAGES[kv_storage][1]} is not paged")
        return _KV_STORAGES[kv_storage][0](model, batch, capacity, mode, extend=extend)
    if page_size is None and num_pages is None:
        return DecodeState(model, batch, capacity, mode, extend=extend)
    return PagedDecodeState(model, batch, capacity, mode, extend=extend, page_size=page_size, num_pages=num_pages)


@torch.no_grad()
def generate(model, prompt_ids, new_tokens: int, mode: str = "block_fp", chunk: int = None, page_size: int = None, num_pages: int = None,
             kv_storage: str = None):
    """greedy decoding: the prompt in one cached call, then one token a call.  Returns (ids [B, prompt + new_tokens], logits
    [B, new_tokens, vocab]: the logits each new token was picked from).
    `prompt_ids` may be a list of 1-D id tensors of DIFFERENT lengths (mode "block_fp"): one ragged prefill, then one token a row a
    call, every sequence decoded as if it were alone; returns (a list of id tensors [len_b + new_tokens], logits as above).
    `chunk`: chunked prefill -- the prompt goes in calls of at most `chunk` tokens through a state with extend=True; for a list of
    prompts every call gives each row whatever it has left, up to `chunk`.
    `page_size` / `num_pages`: paged caches (PagedDecodeState); the tokens and logits are those of the contiguous caches.
    `kv_storage`: None keeps the caches' values as bf16; "int8" stores mantissa bytes (PackedDecodeState: 17/32 of the cache bytes, the
    same tokens and logits; not with `chunk`, pages or a sliding-window model); "nibble" stores 4-bit mantissas (NibbleDecodeState: 9/32
    of the cache bytes, for models whose cached attention operands have width <= 4; the same tokens and logits, the same refusals);
    "narrowest" gives each layer the narrowest of the three storages its widths allow (NarrowestDecodeState)."""
    if chunk is not None and int(chunk) < 1:
        raise ValueError(f"generate: chunk = {chunk} < 1")
    if isinstance(prompt_ids, (list, tuple)):
        lens = [int(p.numel()) for p in prompt_ids]
        B, dev = len(lens), prompt_ids[0].device
        state = _new_state(model, B, max(lens) + new_tokens, mode, chunk is not None, page_size, num_pages, kv_storage)
        if chunk is None:
            ids = torch.zeros(B, max(lens), dtype=prompt_ids[0].dtype, device=dev)
            for b, p in enumerate(prompt_ids):
                ids[b, :lens[b]] = p
            out = model(ids, cache=state, counts=lens)[0]
            logits = out[torch.arange(B, device=dev), torch.tensor(lens, device=dev) - 1]      # (each row's last REAL position)
        else:
            done, last = [0] * B, [None] * B
            while any(d < l for d, l in zip(done, lens)):
                counts = [min(int(chunk), l - d) for d, l in zip(done, lens)]
                ids = torch.zeros(B, max(counts), dtype=prompt_ids[0].dtype, device=dev)
                for b, p in enumerate(prompt_ids):
                    ids[b, :counts[b]] = p.reshape(-1)[done[b]:done[b] + counts[b]]
                out = model(ids, cache=state, counts=counts)[0]
                for b, c in enumerate(counts):
                    done[b] += c
                    if c and done[b] == lens[b]:
                        last[b] = out[b, c - 1]                # (the row's last REAL position, in the call that ends its prompt)
            logits = torch.stack(last)
        rows, steps = [p.reshape(-1) for p in prompt_ids], []
        for i in range(new_tokens):
            steps.append(logits)
            tok = logits.argmax(-1, keepdim=True)
            rows = [torch.cat([r, t]) for r, t in zip(rows, tok)]
            if i + 1 < new_tokens:
                logits = model(tok, cache=state, counts=[1] * B)[0][:, -1]
        return rows, torch.stack(steps, dim=1)
    B, T = prompt_ids.shape
    state = _new_state(model, B, T + new_tokens, mode, chunk is not None, page_size, num_pages, kv_storage)
    ids, steps = prompt_ids, []
    step = int(chunk) if chunk is not None else max(T, 1)
    for t0 in range(0, max(T, 1), step):
        logits = model(prompt_ids[:, t0:t0 + step], cache=state)[0][:, -1]
    for i in range(new_tokens):
        steps.append(logits)
        tok = logits.argmax(-1, keepdim=True)
        ids = torch.cat([ids, tok], dim=1)
        if i + 1 < new_tokens:
            logits = model(tok, cache=state)[0][:, -1]
    return ids, torch.stack(steps, dim=1)


@torch.no_grad()
def beam_search(model, prompt_ids, new_tokens: int, num_beams: int, page_size: int = 32, num_pages: int = None, chunk: int = None,
                kv_storage: str = None):
    """beam search on paged caches: ONE prefill of the B prompts, each then forked into its `num_beams` slots (PagedDecodeState.fork: the
    prompt's full pages by reference, its partial page and open tile copied), and per step one cached call over B * num_beams rows,
    log_softmax, the top num_beams of num_beams * vocab candidates per prompt, and `reorder(beam_idx)` -- the reference's
    `_reorder_cache`, which here copies one partial page a row instead of every row's K and V.  Scores are sums of log-probabilities; no
    length penalty and no EOS (the harness has none).  -> (ids [B, num_beams, T + new_tokens], scores [B, num_beams]), best beam first.
    `prompt_ids` may be a list of 1-D id tensors of different lengths: ids is then a list of [num_beams, len_b + new_tokens].
    `num_pages` (per layer) defaults to every cache row at its capacity plus the one page a row a reorder draws before it gives any back;
    `chunk`: chunked prefill, as in generate.
    `kv_storage`: None keeps the pages' values as bf16; "int8" stores mantissa bytes (PagedPackedDecodeState: 17/32 of the K / V bytes,
    the same ids and scores; not with `chunk`, which needs the extend kernel, nor a sliding-window model)."""
    if page_size is None:
        raise NotImplementedError("beam_search: page_size=None: only a paged state can fork or reorder its sequences")
    if kv_storage not in (None, "int8"):
        raise ValueError(f"beam_search: kv_storage = {kv_storage!r} is neither None (bf16 values) nor 'int8' (mantissa bytes)")
    if kv_storage is not None and chunk is not None:
        raise NotImplementedError("beam_search: kv_storage='int8' with chunk: no extend (chunked prefill) kernel reads the int8-mantissa cache")
    if chunk is not None and int(chunk) < 1:
        raise ValueError(f"beam_search: chunk = {chunk} < 1")
    ragged = isinstance(prompt_ids, (list, tuple))
    prompts = [p.reshape(-1) for p in prompt_ids]
    lens, B, nb, dev = [int(p.numel()) for p in prompts], len(prompts), int(num_beams), prompts[0].device
    if not 1 <= nb <= model.cfg.vocab_size or new_tokens < 1 or min(lens) < 1:
        raise ValueError(f"beam_search: num_beams = {num_beams} outside 1 .. the vocabulary's {model.cfg.vocab_size}, new_tokens = {new_tokens} "
                         f"< 1 or an empty prompt (lengths {lens})")
    N, capacity = B * nb, max(lens) + new_tokens
    if num_pages is None:
        a = model.layers[0].self_attn
        num_pages = N * getattr(a, "nkv", a.nh) * (-(-((capacity + 15) // 16 * 16) // int(page_size)) + 1)
    state = (PagedDecodeState if kv_storage is None else PagedPackedDecodeState)(model, N, capacity, "block_fp", extend=chunk is not None,
                                                                                 page_size=page_size, num_pages=num_pages)
    # the prompts in slots 0, nb, 2 nb, ...; the other slots take no token
    done, last, step = [0] * B, [None] * B, max(lens) if chunk is None else int(chunk)
    while any(d < l for d, l in zip(done, lens)):
        counts = [min(step, l - d) for d, l in zip(done, lens)]
        ids = torch.zeros(N, max(counts), dtype=prompts[0].dtype, device=dev)
        for b, p in enumerate(prompts):
            ids[b * nb, :counts[b]] = p[done[b]:done[b] + counts[b]]
        out = model(ids, cache=state, counts=[counts[s // nb] if s % nb == 0 else 0 for s in range(N)])[0]
        for b, c in enumerate(counts):
            done[b] += c
            if c and done[b] == lens[b]:
                last[b] = out[b * nb, c - 1]                   # (the prompt's last REAL position, in the call that ends it)
    if nb > 1:
        state.fork([b * nb for b in range(B) for _ in range(nb - 1)], [b * nb + j for b in range(B) for j in range(1, nb)])
    logits = torch.stack(last)[:, None].expand(B, nb, -1)      # every beam of a prompt starts as the prompt
    scores = torch.full((B, nb), float("-inf"), device=dev)
    scores[:, 0] = 0.0                                         # (so the first step's candidates are beam 0's num_beams best tokens)
    seqs, base = [p[None].expand(nb, -1) for p in prompts], torch.arange(B, device=dev)[:, None] * nb
    for i in range(new_tokens):
        V = logits.shape[-1]
        cand = (F.log_softmax(logits.float(), dim=-1) + scores[..., None]).reshape(B, nb * V)
        scores, idx = cand.topk(nb, dim=-1)                     # (sorted: best first)
        beam, tok = idx // V, idx % V
        seqs = [torch.cat([s_[beam[b]], tok[b][:, None].to(s_.dtype)], dim=1) for b, s_ in enumerate(seqs)]
        if i + 1 < new_tokens:
            if i:                                              # (after the first step the slots of a prompt still hold the same keys)
                state.reorder((base + beam).reshape(-1))
            logits = model(tok.reshape(N, 1).to(prompts[0].dtype), cache=state)[0][:, -1].reshape(B, nb, V)
    for s in range(N):
        state.release(s)
    return (seqs if ragged else torch.stack(seqs)), scores


@torch.no_grad()
def eval_lm_perplexity(model, batches, device=None):
    """Reference eval/eval_lm.py:41-63: per batch loss * batch * seq_len summed, ppl = exp(sum / tokens)."""
    total, num_samples, seq_len, batch_size = 0.0, 0, None, None
    for input_ids in batches:
        if device is not None:
            input_ids = input_ids.to(device)
        batch_size, seq_len = input_ids.shape
        _, loss = model(input_ids, labels=input_ids)
        total += loss.item() * batch_size * seq_len
        num_samples += batch_size
    reduced = total / (seq_len * num_samples)
    try:
        ppl = math.exp(reduced)
    except OverflowError:
        ppl = float("inf")
    return {"loss": reduced, "perplexity": ppl, "num_samples": num_samples, "seq_len": seq_len, "batch_size": batch_size}
