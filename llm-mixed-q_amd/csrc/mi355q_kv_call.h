// The argument check of the KV-cache exports (mi355q_api.hip, from mi355q_bfp_kv_cache_bytes to mi355q_bfp_attention_extend_sink):
// ONE checked descriptor for what used to be 21 copies of shape check, NULL check, quantiser decoding, alignment check and stride loop.
// Host code only -- no kernel, no launch, no HIP call: an export fills a KvCall, kv_call_check() refuses it with the export's return
// code or fills a KvChecked with what the launchers of mi355q_decode.h / mi355q_extend.h / mi355q_kvp.h / mi355q_kvbm.h take, and the export launches.
// What differs between two exports of one (storage, operation) is data: KV_EXPORTS below.  A returned code is ABI: the ORDER of the
// checks is recorded in tests/golden/kv_api_codes.json, and mi355q_debug_kv_call (mi355q_api.hip) shows this function to the tests.
#ifndef MI355Q_KV_CALL_H
#define MI355Q_KV_CALL_H
#include <stdint.h>

#include <cmath>

#include "mi355q.h"
#include "mi355q_internal.h"
#include "mi355q_decode.h"
#include "mi355q_kvp.h"
#include "mi355q_kvbm.h"
#include "mi355q_linear_call.h"

namespace mi355q {

// the block_fp quantiser of one operand: {width, exponent width, exponent bias} at pr; a quantised value must fit bf16's 8 significant bits
inline int decode_quant_args(const int32_t* pr, QuantArgs& a) {
    if (const int rc = block_fp_args(a, pr[0], pr[1], pr[2], {9, MI355Q_E_BADARG, MI355Q_E_UNSUPPORTED})) return rc;
    a.b0 = 1; a.b1 = 16;
    return 0;
}
// the quantisers of the CACHED operands (the y side of qk_params and pv_params); `widest`: kvp_widest() of a mantissa storage (8 where
// a mantissa must fit a byte, 4 a nibble), 9 where the cache stores bf16
inline int cached_quant_args(const int32_t* qk_params, const int32_t* pv_params, QuantArgs& ak, QuantArgs& av, int widest) {
    int rc;
    if ((rc = decode_quant_args(qk_params + 3, ak)) != 0 || (rc = decode_quant_args(pv_params + 3, av)) != 0) return rc;
    return qk_params[3] > widest || pv_params[3] > widest ? MI355Q_E_UNSUPPORTED : 0;
}
// the block_minifloat quantiser of one operand: {width, exponent width, exponent bias width} at pr.  Exponent width 1 .. 8, mantissa
// bits width - exponent width - 1 in 1 .. 7 (a quantised value must be exact in bf16), bias width 1 .. 8; anything else is unsupported
inline int bm_quant_args(const int32_t* pr, QuantArgs& a) {
    const int mbits = pr[0] - pr[1] - 1;
    if (pr[1] < 1 || pr[1] > 8 || mbits < 1 || mbits > 7 || pr[2] < 1 || pr[2] > 8) return MI355Q_E_UNSUPPORTED;
    a.b0 = 1; a.b1 = 16;
    block_minifloat_fill(a, mbits, pr[1], pr[2]);
    return 0;
}
// the quantisers of a block_minifloat call: the cached operands' (y sides: append) or Q's and P's (x sides: decode)
inline int bm_quant_pair(const int32_t* qk_params, const int32_t* pv_params, int side, QuantArgs& a, QuantArgs& b) {
    int rc;
    if ((rc = bm_quant_args(qk_params + side, a)) != 0 || (rc = bm_quant_args(pv_params + side, b)) != 0) return rc;
    return 0;
}
inline int decode_cache_shape(int64_t B, int64_t C, int64_t D) {
    if (B < 1 || C < 1 || D < 1 || B > 65535) return MI355Q_E_BADARG;
    if (C % 16 != 0 || D % 32 != 0 || D > 128 || C > (1LL << 30)) return MI355Q_E_UNSUPPORTED;
    return 0;
}
// the pools' shape and the rows' table: BADARG for a page size that is no power of two >= 32; `pg` gets the kernels' view
inline int paged_shape(int64_t B, int64_t max_pages, int64_t num_pages, int64_t P, int64_t D, const int32_t* block_table, KvPages* pg) {
    if (P < 32 || (P & (P - 1)) != 0 || B < 1 || B > 65535 || D < 1 || max_pages < 1 || num_pages < 1) return MI355Q_E_BADARG;
    if (D % 32 != 0 || D > 128 || P > (1LL << 30) || max_pages > (1LL << 30) / P || num_pages > 0x7FFFFFFFLL) return MI355Q_E_UNSUPPORTED;
    if (pg) {
        int lg = 5;
        while ((1LL << lg) < P) ++lg;
        *pg = KvPages{block_table, (int)max_pages, (int)num_pages, lg};
    }
    return 0;
}
// the cache behind a *_window call: block_table != NULL the paged pools (paged_shape); NULL the contiguous cache of capacity
// C = max_pages * P keys a row (decode_cache_shape; num_pages is not used)
inline int window_cache_shape(int64_t B, int64_t max_pages, int64_t num_pages, int64_t P, int64_t D, const int32_t* block_table, KvPages* pg) {
    if (block_table) return paged_shape(B, max_pages, num_pages, P, D, block_table, pg);
    if (max_pages < 1 || P < 1 || max_pages > (1LL << 30) / P) return MI355Q_E_BADARG;
    return decode_cache_shape(B, max_pages * P, D);
}

enum KvStorage { KV_BF16, KV_INT8, KV_PAGED, KV_INT8_PAGED, KV_INT4 };   // KV_PAGED: the cache comes as (max_pages, num_pages, P) and a block
                                                                // table; KV_INT8_PAGED: both -- int8-mantissa pieces in paged pools;
                                                                // KV_INT4: two 4-bit mantissas a byte (mi355q_kvp.h), contiguous only
constexpr bool kv_mantissas(KvStorage s) { return s == KV_INT8 || s == KV_INT8_PAGED || s == KV_INT4; }   // mantissa and exponent bytes, rebuilt by the kernels
constexpr KvMantissa kv_mantissa(KvStorage s) { return s == KV_INT4 ? KV_M4 : KV_M8; }                    // which, where kv_mantissas(s)
constexpr bool kv_paged(KvStorage s) { return s == KV_PAGED || s == KV_INT8_PAGED; }
enum KvOp { KV_BYTES, KV_APPEND, KV_DEQUANT, KV_DECODE, KV_EXTEND };
enum : unsigned {
    KV_LENGTHS = 1,     // `lengths` is mandatory (else: not taken, or optional -- NULL is the uniform form)
    KV_GROUPED = 2,     // the *_grouped exports: G < 1 is refused and G goes through as it is, so G = 1 runs the grouped form
                        // (else G < 0 is refused and G <= 1 becomes 0, the ungrouped kernels)
    KV_WINDOW = 4,      // the *_window exports: causal and window >= 1 or BADARG, window clamped to L, causal passed as 1;
                        // block_table == NULL is the contiguous cache of max_pages * P keys
    KV_MINIFLOAT = 8,   // the mi355q_bm_* exports: qk_params / pv_params are block_minifloat's {width, exponent width, exponent bias
                        // width} (bm_quant_args) and the launchers are those of mi355q_kvbm.h; storage and layout stay KV_BF16's
    KV_SINKS = 16,      // the *_sink exports (with KV_WINDOW): sinks outside 0 .. 16 is BADARG; the launchers are those of mi355q_sink.h
};
// the exports in the order of include/mi355q.h (mi355q_debug_kv_call's export id)
enum KvExport {
    KVX_CACHE_BYTES, KVX_APPEND, KVX_DECODE_FP32, KVX_DECODE, KVX_APPEND_RAGGED, KVX_DECODE_FP32_RAGGED, KVX_DECODE_RAGGED, KVX_EXTEND,
    KVX_DECODE_GROUPED, KVX_EXTEND_GROUPED, KVX_PAGED_BYTES, KVX_APPEND_PAGED, KVX_DECODE_FP32_PAGED, KVX_DECODE_PAGED, KVX_EXTEND_PAGED,
    KVX_KV8_CACHE_BYTES, KVX_KV8_APPEND, KVX_KV8_DECODE_FP32, KVX_DECODE_KV8, KVX_DECODE_WINDOW, KVX_EXTEND_WINDOW,
    KVX_KV8P_BYTES, KVX_KV8P_APPEND, KVX_KV8P_DECODE_FP32, KVX_KV8P_DECODE, KVX_BM_APPEND, KVX_BM_DECODE,
    KVX_NONE_27,        // no export: mi355q_debug_kv_call_all has always refused id 27, the first id behind the block_minifloat
                        // exports, and tests/test_kvbm_host.py holds it to that -- the id stays refused and the next exports start at 28
    KVX_KV4_CACHE_BYTES, KVX_KV4_APPEND, KVX_KV4_DECODE_FP32, KVX_DECODE_KV4,
    KVX_NONE_32,        // no export either: tests/test_kv4_host.py holds id 32, the first id behind the 4-bit-mantissa exports, refused
    KVX_DECODE_SINK, KVX_EXTEND_SINK, KVX_COUNT
};
constexpr bool kvx_hole(int id) { return id == KVX_NONE_27 || id == KVX_NONE_32; }

// one call of a KV-cache export: the form (what KV_EXPORTS says of the export), then the raw arguments; what an export does not
// take stays 0 / NULL.  L is the host's length: L of the uniform exports, max_length of the others.  k / v: the append's new rows or
// the dequantiser's outputs.  Nothing here is dereferenced by the check but qk_params, pv_params and strides.
struct KvCall {
    KvStorage storage;
    KvOp op;
    unsigned form;
    const void *kq, *vq, *stage, *k, *v, *q, *out, *workspace;
    const int32_t *lengths, *counts, *block_table;
    const int64_t *k_bytes, *v_bytes, *stage_bytes;
    int64_t B, C, max_pages, num_pages, P, D, M, L, n;
    int32_t G, causal;
    int64_t window;
    int32_t splits;
    const int32_t *qk_params, *pv_params;
    const int64_t* strides;
    int64_t sinks;              // the *_sink exports' (KV_SINKS); behind every field the other exports fill

    KvCall& cache(const void* kq_, const void* vq_, const void* stage_, int64_t B_, int64_t C_, int64_t D_) {
        kq = kq_; vq = vq_; stage = stage_; B = B_; C = C_; D = D_;
        return *this;
    }
    KvCall& pools(const void* kq_, const void* vq_, const void* stage_, const int32_t* table, int64_t B_, int64_t max_pages_,
                  int64_t num_pages_, int64_t P_, int64_t D_) {
        kq = kq_; vq = vq_; stage = stage_; block_table = table; B = B_; max_pages = max_pages_; num_pages = num_pages_; P = P_; D = D_;
        return *this;
    }
    KvCall& sizes(const int64_t* k_bytes_, const int64_t* v_bytes_, const int64_t* stage_bytes_) {
        k_bytes = k_bytes_; v_bytes = v_bytes_; stage_bytes = stage_bytes_;
        return *this;
    }
    KvCall& rows(const void* k_, const void* v_, int64_t n_) {
        k = k_; v = v_; n = n_;
        return *this;
    }
    KvCall& lens(const int32_t* lengths_, const int32_t* counts_, int64_t L_) {
        lengths = lengths_; counts = counts_; L = L_;
        return *this;
    }
    KvCall& query(const void* q_, const void* out_, const void* workspace_, int64_t M_, int32_t G_, int32_t causal_, int64_t window_,
                  int32_t splits_) {
        q = q_; out = out_; workspace = workspace_; M = M_; G = G_; causal = causal_; window = window_; splits = splits_;
        return *this;
    }
    KvCall& sunk(int64_t sinks_) {
        sinks = sinks_;
        return *this;
    }
    KvCall& quant(const int32_t* qk, const int32_t* pv, const int64_t* strides_) {
        qk_params = qk; pv_params = pv; strides = strides_;
        return *this;
    }
};
constexpr KvCall KV_EXPORTS[KVX_COUNT] = {
    {KV_BF16, KV_BYTES, 0},           {KV_BF16, KV_APPEND, 0},          {KV_BF16, KV_DEQUANT, 0},          {KV_BF16, KV_DECODE, 0},
    {KV_BF16, KV_APPEND, KV_LENGTHS}, {KV_BF16, KV_DEQUANT, KV_LENGTHS}, {KV_BF16, KV_DECODE, KV_LENGTHS}, {KV_BF16, KV_EXTEND, 0},
    {KV_BF16, KV_DECODE, KV_GROUPED}, {KV_BF16, KV_EXTEND, KV_GROUPED},
    {KV_PAGED, KV_BYTES, 0},          {KV_PAGED, KV_APPEND, KV_LENGTHS}, {KV_PAGED, KV_DEQUANT, KV_LENGTHS},
    {KV_PAGED, KV_DECODE, KV_LENGTHS}, {KV_PAGED, KV_EXTEND, KV_LENGTHS},
    {KV_INT8, KV_BYTES, 0},           {KV_INT8, KV_APPEND, KV_LENGTHS}, {KV_INT8, KV_DEQUANT, KV_LENGTHS}, {KV_INT8, KV_DECODE, KV_LENGTHS},
    {KV_PAGED, KV_DECODE, KV_LENGTHS | KV_WINDOW}, {KV_PAGED, KV_EXTEND, KV_LENGTHS | KV_WINDOW},
    {KV_INT8_PAGED, KV_BYTES, 0},     {KV_INT8_PAGED, KV_APPEND, KV_LENGTHS}, {KV_INT8_PAGED, KV_DEQUANT, KV_LENGTHS},
    {KV_INT8_PAGED, KV_DECODE, KV_LENGTHS},
    {KV_BF16, KV_APPEND, KV_LENGTHS | KV_MINIFLOAT}, {KV_BF16, KV_DECODE, KV_LENGTHS | KV_MINIFLOAT},
    {KV_BF16, KV_BYTES, 0},           // (KVX_NONE_27: never looked up)
    {KV_INT4, KV_BYTES, 0},           {KV_INT4, KV_APPEND, KV_LENGTHS}, {KV_INT4, KV_DEQUANT, KV_LENGTHS}, {KV_INT4, KV_DECODE, KV_LENGTHS},
    {KV_BF16, KV_BYTES, 0},           // (KVX_NONE_32: never looked up)
    {KV_PAGED, KV_DECODE, KV_LENGTHS | KV_WINDOW | KV_SINKS}, {KV_PAGED, KV_EXTEND, KV_LENGTHS | KV_WINDOW | KV_SINKS},
};

// what the launchers take of a call that passed
struct KvChecked {
    KvCache c;                  // storage KV_BF16 / KV_PAGED (C: the row's logical capacity)
    KvpCache cp;                // storage KV_INT8 / KV_INT8_PAGED / KV_INT4: kv_mantissa(storage)'s pieces (C: the row's logical capacity)
    KvPages pg;
    const KvPages* pages;       // &pg with a block table, else NULL
    QuantArgs aq, ap, ak, av;   // Q and P (decode, extend); the cached K and V (append; mantissa storage: every operation)
    int G, causal;              // normalised: 0 the ungrouped kernels; causal 0 / 1
    long long window;           // clamped to L; 0: none
    long long sinks;            // the *_sink exports': 0 .. 16; else 0
    long long st[4];
    const long long* strides;   // st or NULL (decode / extend: fill_qo_strides' contiguous default); the append's are always st
};

// true: launch with `k`.  false: return rc (an MI355Q_E_* code, or 0 where there is nothing to do)
inline bool kv_call_check(const KvCall& d, KvChecked& k, int& rc) {
    const bool attn = d.op == KV_DECODE || d.op == KV_EXTEND, mant = kv_mantissas(d.storage), paged_form = kv_paged(d.storage);
    const int widest = mant ? kvp_widest(kv_mantissa(d.storage)) : 9;     // (the widest cached operand the storage holds)
    const bool windowed = (d.form & KV_WINDOW) != 0, minifloat = (d.form & KV_MINIFLOAT) != 0;
    const auto stop = [&rc](int code) { rc = code; return false; };
    const auto misaligned = [](std::initializer_list<const void*> ptrs, uintptr_t to) {      // (an optional NULL passes)
        uintptr_t bits = 0;
        for (const void* p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
        return bits % to != 0;
    };
    k = KvChecked{};
    // what is refused before the cache's shape is looked at
    if (d.op == KV_BYTES && (!d.k_bytes || !d.v_bytes || !d.stage_bytes)) return stop(MI355Q_E_BADARG);
    if (attn && (d.M < 0 || d.L < 0 || d.splits < 0 || d.G < ((d.form & KV_GROUPED) ? 1 : 0) || (windowed && (d.window < 1 || !d.causal))))
        return stop(MI355Q_E_BADARG);
    if (attn && (d.form & KV_SINKS) && (d.sinks < 0 || d.sinks > 16)) return stop(MI355Q_E_BADARG);
    // the cache's shape; `cap`: the keys a row can hold
    if (!paged_form) rc = decode_cache_shape(d.B, d.C, d.D);
    else if (windowed) rc = window_cache_shape(d.B, d.max_pages, d.num_pages, d.P, d.D, d.block_table, &k.pg);
    else rc = paged_shape(d.B, d.op == KV_BYTES ? 1 : d.max_pages, d.num_pages, d.P, d.D, d.block_table, &k.pg);      // (pools have no table)
    if (rc) return false;
    if (d.op == KV_BYTES) return true;
    const long long cap = paged_form ? d.max_pages * d.P : d.C;
    const bool no_table = paged_form && !windowed && !d.block_table, no_lengths = (d.form & KV_LENGTHS) && !d.lengths;
    const bool no_cache = !d.kq || !d.vq || no_lengths || no_table;

    if (d.op == KV_APPEND) {
        if (d.L < 0 || d.n < 0 || !d.qk_params || !d.pv_params) return stop(MI355Q_E_BADARG);
        if (d.L + d.n > cap) return stop(paged_form ? MI355Q_E_BADARG : MI355Q_E_UNSUPPORTED);        // (nothing is written)
        if (mant && (rc = cached_quant_args(d.qk_params, d.pv_params, k.ak, k.av, widest)) != 0) return false;    // (mantissas: before the early 0)
        if (d.n == 0) return stop(0);
        if (no_cache || !d.stage || !d.k || !d.v) return stop(MI355Q_E_BADARG);
        if (!mant && (rc = minifloat ? bm_quant_pair(d.qk_params, d.pv_params, 3, k.ak, k.av) : cached_quant_args(d.qk_params, d.pv_params, k.ak, k.av, widest)) != 0)
            return false;
        if (misaligned({d.kq, d.vq, d.stage, d.k, d.v}, 16) || misaligned({d.lengths, d.counts, d.block_table}, 4)) return stop(MI355Q_E_ALIGN);
        const long long dflt[4] = {d.n * d.D, d.D, d.n * d.D, d.D};
        for (int i = 0; i < 4; ++i) {
            if (d.strides && d.strides[i] % 4) return stop(MI355Q_E_ALIGN);
            k.st[i] = d.strides ? d.strides[i] : dflt[i];
        }
        k.strides = k.st;
    } else if (d.op == KV_DEQUANT) {
        if (d.L < 0 || d.L > cap || (mant && (!d.qk_params || !d.pv_params))) return stop(MI355Q_E_BADARG);
        if (mant && (rc = cached_quant_args(d.qk_params, d.pv_params, k.ak, k.av, widest)) != 0) return false;
        if (d.L == 0) return stop(0);
        if (no_cache || !d.k || !d.v) return stop(MI355Q_E_BADARG);
    } else {
        // decode: the last M <= 16 positions, a workspace, at most 65535 launch rows; extend: any M, none of the three
        const bool decode = d.op == KV_DECODE;
        if (paged_form && d.L > cap) return stop(MI355Q_E_BADARG);                                   // (paged form: before the M range)
        if (d.M < 1 || (decode && d.M > 16) || d.L < d.M) return stop(MI355Q_E_UNSUPPORTED);
        k.G = (d.form & KV_GROUPED) || d.G > 1 ? d.G : 0;
        if (decode && k.G && d.B * (k.G / decode_group_width(k.G, d.M)) > 65535) return stop(MI355Q_E_UNSUPPORTED);   // (the grid's second dimension)
        if (d.L > cap || no_cache || !d.q || !d.out || (decode && !d.workspace) || !d.qk_params || !d.pv_params || (d.counts && !d.lengths))
            return stop(MI355Q_E_BADARG);
        if (minifloat) {
            // (the cached operands' parameters are checked too: a cache the append would refuse is refused here)
            if ((rc = bm_quant_pair(d.qk_params, d.pv_params, 0, k.aq, k.ap)) != 0 || (rc = bm_quant_pair(d.qk_params, d.pv_params, 3, k.ak, k.av)) != 0)
                return false;
        } else if ((rc = decode_quant_args(d.qk_params, k.aq)) != 0 || (rc = decode_quant_args(d.pv_params, k.ap)) != 0 ||
                   (mant && (rc = cached_quant_args(d.qk_params, d.pv_params, k.ak, k.av, widest)) != 0))
            return false;
        if (misaligned({d.q, d.kq, d.vq, d.out, d.workspace}, 16) || misaligned({d.lengths, d.counts, d.block_table}, 4)) return stop(MI355Q_E_ALIGN);
        if (d.strides) {
            for (int i = 0; i < 4; ++i) {
                if (d.strides[i] % 4) return stop(MI355Q_E_ALIGN);
                k.st[i] = d.strides[i];
            }
            k.strides = k.st;
        }
        k.causal = windowed || d.causal != 0;
        k.window = !windowed ? 0 : d.window > d.L ? d.L : d.window;      // (a window over every key the call can hold: the same mask)
        k.sinks = (d.form & KV_SINKS) ? d.sinks : 0;
    }
    void *const kq = const_cast<void*>(d.kq), *const vq = const_cast<void*>(d.vq);         // (the one cast; the element type is the storage's)
    float* const stage = static_cast<float*>(const_cast<void*>(d.stage));
    if (mant) k.cp = KvpCache{static_cast<uint8_t*>(kq), static_cast<uint8_t*>(vq), stage, d.B, cap, (int)d.D};
    else k.c = KvCache{static_cast<uint16_t*>(kq), static_cast<uint16_t*>(vq), stage, d.B, cap, (int)d.D};
    k.pages = paged_form && d.block_table ? &k.pg : nullptr;
    rc = 0;
    return true;
}

}  // namespace mi355q
#endif
