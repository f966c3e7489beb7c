"""Shared by the 4-bit-mantissa KV cache tests (tests/test_kv4_host.py, tests/test_gpu_kv4_*.py): a numpy restatement of the piece layout
of csrc/mi355q_kvp.h, written from the header's text and not from the kernels; block_fp configs whose Q / P side (data_in_*) and cached
side (weight_*) differ in width; and tiny Llama models whose layers differ in their attention widths."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "llm-mixed-q_amd", ROOT):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

PIECE, CODES = 288, 256


# ---- the layout: a piece is 256 mantissa bytes, byte 8 (l >> 1) + j = slot j of lane 2 (l >> 1) in bits 0 .. 3 and of lane
# 2 (l >> 1) + 1 in bits 4 .. 7, then 32 exponent-code bytes
def pack_lanes(m):
    """m int [64 lanes, 8 slots], |m| <= 7 -> the 256 mantissa bytes"""
    m = np.asarray(m, np.int64)
    assert m.shape == (64, 8) and np.abs(m).max() <= 7
    lo, hi = m[0::2] & 0xF, m[1::2] & 0xF                    # [32 lane pairs, 8 slots]
    return (lo | (hi << 4)).astype(np.uint8).reshape(256)


def unpack_lanes(b):
    """the 256 mantissa bytes -> int [64 lanes, 8 slots], each nibble sign-extended"""
    b = np.asarray(b, np.uint8).reshape(32, 8).astype(np.int64)
    m = np.empty((64, 8), np.int64)
    m[0::2], m[1::2] = b & 0xF, b >> 4
    return np.where(m >= 8, m - 16, m)


def k_piece_pack(m, codes):
    """one K piece: m int [16 keys of the tile, 32 d of the chunk], codes [32] (the block of d = 32 c + i: byte 256 + i) -> 288 bytes.
    Lane (key = lane % 16, g = lane / 16) holds d = 8 g + j in slot j"""
    lanes = np.empty((64, 8), np.int64)
    for l in range(64):
        lanes[l] = np.asarray(m)[l % 16, 8 * (l // 16):8 * (l // 16) + 8]
    return np.concatenate([pack_lanes(lanes), np.asarray(codes, np.uint8).reshape(32)])


def k_piece_unpack(piece):
    """288 bytes -> (m int [16 keys, 32 d], codes [32] by d)"""
    lanes, m = unpack_lanes(piece[:CODES]), np.empty((16, 32), np.int64)
    for l in range(64):
        m[l % 16, 8 * (l // 16):8 * (l // 16) + 8] = lanes[l]
    return m, np.asarray(piece[CODES:PIECE], np.int64)


def _v_key(g, j):
    return 16 * (j // 4) + 4 * g + (j & 3)


def v_piece_pack(m, codes):
    """one V piece: m int [32 keys of the pair, 16 d], codes [32] BY KEY -> 288 bytes.  Lane (d = lane % 16, g = lane / 16) holds key
    16 (j / 4) + 4 g + (j & 3) in slot j; that key's exponent is byte 256 + 8 g + j (slot order)"""
    lanes, out = np.empty((64, 8), np.int64), np.empty(32, np.uint8)
    for l in range(64):
        for j in range(8):
            lanes[l, j] = np.asarray(m)[_v_key(l // 16, j), l % 16]
    for g in range(4):
        for j in range(8):
            out[8 * g + j] = codes[_v_key(g, j)]
    return np.concatenate([pack_lanes(lanes), out])


def v_piece_unpack(piece):
    """288 bytes -> (m int [32 keys, 16 d], codes [32] by key)"""
    lanes, m, codes = unpack_lanes(piece[:CODES]), np.empty((32, 16), np.int64), np.empty(32, np.int64)
    for l in range(64):
        for j in range(8):
            m[_v_key(l // 16, j), l % 16] = lanes[l, j]
    for g in range(4):
        for j in range(8):
            codes[_v_key(g, j)] = piece[CODES + 8 * g + j]
    return m, codes


def unpack_cache(k4, v4, B, C, D, width, bias=127):
    """the raw bytes of a NibbleKVCache -> (K, V) float64 [B, C (V: 32 ceil(C / 32)), D]: mantissa * 2^(code - bias - (width - 1))"""
    k4 = np.asarray(k4, np.uint8).reshape(B, C // 16, D // 32, PIECE)
    v4 = np.asarray(v4, np.uint8).reshape(B, (C + 31) // 32, D // 16, PIECE)
    K, V = np.zeros((B, C, D)), np.zeros((B, v4.shape[1] * 32, D))
    for b in range(B):
        for t in range(C // 16):
            for c in range(D // 32):
                m, codes = k_piece_unpack(k4[b, t, c])
                K[b, 16 * t:16 * t + 16, 32 * c:32 * c + 32] = np.ldexp(m.astype(np.float64), (codes - bias - (width - 1))[None, :])
        for s in range(v4.shape[1]):
            for dt in range(D // 16):
                m, codes = v_piece_unpack(v4[b, s, dt])
                V[b, 32 * s:32 * s + 32, 16 * dt:16 * dt + 16] = np.ldexp(m.astype(np.float64), (codes - bias - (width - 1))[:, None])
    return K, V


# ---- configs and models
def cfg2(x_width, y_width):
    """block_fp [1, 16] with data_in_* = the Q / P side and weight_* = the cached side"""
    return dict(name="block_fp", is_ptq=True, bypass=False, data_in_width=x_width, data_in_exponent_width=8, data_in_exponent_bias=127,
                data_in_block_size=[1, 16], weight_width=y_width, weight_exponent_width=8, weight_exponent_bias=127,
                weight_block_size=[1, 16])


def par2(x_width, y_width):
    return (x_width, 8, 127, y_width, 8, 127)


def oracle2(q, k, v, x_width, y_width, scale_div):
    """window_util.oracle (causal, no window) for the config cfg2(x_width, y_width)"""
    from oracle import np_oracle as O
    fmin = np.finfo(np.float32).min
    w = O.matmul_quantized(q, np.swapaxes(k, -1, -2), cfg2(x_width, y_width))
    w = (w / np.float32(scale_div)).astype(np.float32)
    tq, tk = w.shape[-2:]
    with np.errstate(over="ignore"):
        w = np.maximum(w + np.triu(np.full((tq, tk), fmin, np.float32), 1 + tk - tq), fmin)
    e = np.exp((w - w.max(-1, keepdims=True)).astype(np.float64))
    return O.matmul_quantized((e / e.sum(-1, keepdims=True)).astype(np.float32), v, cfg2(x_width, y_width))


def _node(width):
    return dict(name="block_fp", is_ptq=True, bypass=False, data_in_width=width, data_in_exponent_width=8, data_in_exponent_bias=127,
                data_in_block_size=[1, 16], weight_width=width, weight_exponent_width=8, weight_exponent_bias=127,
                weight_block_size=[1, 16], bias_width=width, bias_exponent_width=8, bias_exponent_bias=127, bias_block_size=[16])


def tiny_llama(attention_widths, num_kv_heads=None, seed=0, scale=4.0, **cfg_kw):
    """the tiny Llama of tests/test_gpu_gqa_model.py (hidden 128, 4 heads, every Linear block_fp of width 6, weights scaled by 4) with one
    layer per entry of attention_widths: both attention products of layer i have that width on both sides"""
    import torch
    from mi355q import harness as H
    torch.manual_seed(seed)
    layers = len(attention_widths)
    cfg = H.TinyLlamaConfig(vocab_size=97, hidden_size=128, intermediate_size=256, num_layers=layers, num_heads=4, max_positions=48,
                            num_kv_heads=num_kv_heads, **cfg_kw)
    qc = H.expand_llama_quant_config(_node(6), layers)
    for i, w in enumerate(attention_widths):
        for name in ("matmul_0", "matmul_1"):
            qc[f"model_layer_{i}"]["self_attn"][name] = dict(qc[f"model_layer_{i}"]["self_attn"][name], data_in_width=w, weight_width=w)
    model = H.TinyLlamaForCausalLM(cfg, qc)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.ndim == 2 and "embed" not in n:
                p.mul_(scale)
    return model
