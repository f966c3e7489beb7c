// Stand-alone host program (its own main, no GPU, nothing loaded into Python): csrc/mi355q_kv_call.h's kv_call_check over rows of
// tests/golden/kv_api_codes.json / .npz, for a sanitizer build.  Reads the lines `python tools/record_kv_api_codes.py --dump N` writes:
//   export id, recorded code, the 27 flat arguments of mi355q_debug_kv_call, then for qk_params, pv_params and strides a 0 / 1 "given"
//   and their 6, 6 and 4 values
// and exits 1 at the first row whose code differs or that would launch.  Behind them: the rows below for the four ids of the paged
// int8-mantissa cache (KVX_KV8P_*), which the recorded table does not hold -- a valid call of each, which must pass with the paged view
// and the int8 cache filled, and its refusals with the code written next to them -- and, the same way, rows for the two ids of the
// block_minifloat cache (KVX_BM_APPEND, KVX_BM_DECODE), whose quantiser words are (width, exponent width, exponent bias width).  Build and run: see the Makefile next to this file.
#include <cstdio>
#include <string>

#include "mi355q_kv_call.h"

using namespace mi355q;

// the paged int8-mantissa ids: {id, what differs from the valid call, expected code, expected "would launch"}
struct NewRow {
    KvExport id;
    const char* what;
    int code;
    bool go;
};

static int new_rows() {
    const int32_t good[6] = {6, 8, 127, 6, 8, 127}, w9[6] = {6, 8, 127, 9, 8, 127};
    int64_t nb[3];
    const void* a = reinterpret_cast<const void*>(static_cast<uintptr_t>(0x10000));
    const int32_t* a32 = static_cast<const int32_t*>(a);
    const NewRow rows[] = {
        {KVX_KV8P_BYTES, "", 0, true},         {KVX_KV8P_BYTES, "P48", MI355Q_E_BADARG, false},
        {KVX_KV8P_APPEND, "", 0, true},        {KVX_KV8P_APPEND, "P48", MI355Q_E_BADARG, false},
        {KVX_KV8P_APPEND, "over", MI355Q_E_BADARG, false},          // L + n > max_pages * P: the paged form's code
        {KVX_KV8P_APPEND, "w9 n0", MI355Q_E_UNSUPPORTED, false},    // the int8 check, before the early 0
        {KVX_KV8P_APPEND, "n0", 0, false},     {KVX_KV8P_APPEND, "notable", MI355Q_E_BADARG, false},
        {KVX_KV8P_APPEND, "odd", MI355Q_E_ALIGN, false},
        {KVX_KV8P_DECODE_FP32, "", 0, true},   {KVX_KV8P_DECODE_FP32, "over", MI355Q_E_BADARG, false},
        {KVX_KV8P_DECODE_FP32, "w9 n0", MI355Q_E_UNSUPPORTED, false}, {KVX_KV8P_DECODE_FP32, "n0", 0, false},
        {KVX_KV8P_DECODE, "", 0, true},        {KVX_KV8P_DECODE, "over", MI355Q_E_BADARG, false},
        {KVX_KV8P_DECODE, "w9", MI355Q_E_UNSUPPORTED, false},       {KVX_KV8P_DECODE, "M17", MI355Q_E_UNSUPPORTED, false},
        {KVX_KV8P_DECODE, "notable", MI355Q_E_BADARG, false},       {KVX_KV8P_DECODE, "odd", MI355Q_E_ALIGN, false},
    };
    int n = 0;
    for (const NewRow& r : rows) {
        const std::string w = r.what;
        const auto has = [&w](const char* s) { return w.find(s) != std::string::npos; };
        const bool over = has("over"), n0 = has("n0");
        const void* kq = has("odd") ? reinterpret_cast<const void*>(static_cast<uintptr_t>(0x10008)) : a;
        KvCall d = KV_EXPORTS[r.id];
        d.pools(kq, a, a, has("notable") ? nullptr : a32, 4, 3, 12, has("P48") ? 48 : 64, 32).sizes(nb, nb + 1, nb + 2)
            .rows(a, a, n0 ? 0 : 5).lens(a32, a32, over ? 193 : n0 && r.id != KVX_KV8P_APPEND ? 0 : 40)
            .query(a, a, a, has("M17") ? 17 : 4, 2, 1, 0, 0).quant(has("w9") ? w9 : good, good, nullptr);
        if (r.id == KVX_KV8P_APPEND) d.counts = a32;
        else d.counts = nullptr;
        KvChecked c;
        int rc = 99;
        const bool go = kv_call_check(d, c, rc);
        bool ok = go == r.go && rc == r.code;
        if (go && r.id != KVX_KV8P_BYTES)      // what the launchers get: the int8 cache at the rows' logical capacity, and the page table
            ok = ok && c.cp.C == 192 && c.cp.D == 32 && c.cp.B == 4 && c.pages == &c.pg && c.pg.lg_p == 6 && c.pg.num_pages == 12 && c.pg.max_pages == 3 &&
                 c.c.kq == nullptr && (r.id != KVX_KV8P_DECODE || c.G == 2);
        if (!ok) {
            std::printf("new row %d (export %d, '%s'): code %d (launch %d), expected %d (launch %d)\n", n, (int)r.id, r.what, rc, (int)go, r.code,
                        (int)r.go);
            return -1;
        }
        ++n;
    }
    return n;
}

// the block_minifloat ids: contiguous, always ragged; the append reads the weight sides of the words, the decode all four
static int bm_rows() {
    const int32_t good[6] = {8, 4, 8, 8, 4, 8}, bfp[6] = {6, 8, 127, 6, 8, 127}, x_bad[6] = {12, 9, 0, 8, 4, 8}, m0[6] = {8, 4, 8, 5, 4, 8},
                  m8[6] = {8, 4, 8, 12, 3, 8}, bw9[6] = {8, 4, 8, 8, 4, 9};
    const void* a = reinterpret_cast<const void*>(static_cast<uintptr_t>(0x10000));
    const int32_t* a32 = static_cast<const int32_t*>(a);
    const int64_t odd_st[4] = {32, 32, 34, 32};
    const NewRow rows[] = {
        {KVX_BM_APPEND, "", 0, true},                                {KVX_BM_APPEND, "nolengths", MI355Q_E_BADARG, false},
        {KVX_BM_APPEND, "over", MI355Q_E_UNSUPPORTED, false},        {KVX_BM_APPEND, "n0", 0, false},
        {KVX_BM_APPEND, "n0 m0", 0, false},                          // (as for the bf16 cache: the early 0 comes before the quantiser words)
        {KVX_BM_APPEND, "bfp", MI355Q_E_UNSUPPORTED, false},         {KVX_BM_APPEND, "m0", MI355Q_E_UNSUPPORTED, false},
        {KVX_BM_APPEND, "m8", MI355Q_E_UNSUPPORTED, false},          {KVX_BM_APPEND, "bw9", MI355Q_E_UNSUPPORTED, false},
        {KVX_BM_APPEND, "xbad", 0, true},                            // the x sides are not the append's
        {KVX_BM_APPEND, "odd", MI355Q_E_ALIGN, false},               {KVX_BM_APPEND, "stride", MI355Q_E_ALIGN, false},
        {KVX_BM_APPEND, "D48", MI355Q_E_UNSUPPORTED, false},
        {KVX_BM_DECODE, "", 0, true},                                {KVX_BM_DECODE, "nolengths", MI355Q_E_BADARG, false},
        {KVX_BM_DECODE, "over", MI355Q_E_BADARG, false},             {KVX_BM_DECODE, "M17", MI355Q_E_UNSUPPORTED, false},
        {KVX_BM_DECODE, "bfp", MI355Q_E_UNSUPPORTED, false},         {KVX_BM_DECODE, "xbad", MI355Q_E_UNSUPPORTED, false},
        {KVX_BM_DECODE, "m0", MI355Q_E_UNSUPPORTED, false},          {KVX_BM_DECODE, "m8", MI355Q_E_UNSUPPORTED, false},
        {KVX_BM_DECODE, "bw9", MI355Q_E_UNSUPPORTED, false},         {KVX_BM_DECODE, "odd", MI355Q_E_ALIGN, false},
        {KVX_BM_DECODE, "stride", MI355Q_E_ALIGN, false},            {KVX_BM_DECODE, "Gneg", MI355Q_E_BADARG, false},
    };
    int n = 0;
    for (const NewRow& r : rows) {
        const std::string w = r.what;
        const auto has = [&w](const char* s) { return w.find(s) != std::string::npos; };
        const bool append = r.id == KVX_BM_APPEND, n0 = has("n0");
        const int32_t* words = has("bfp") ? bfp : has("xbad") ? x_bad : has("m0") ? m0 : has("m8") ? m8 : has("bw9") ? bw9 : good;
        const void* kq = has("odd") ? reinterpret_cast<const void*>(static_cast<uintptr_t>(0x10008)) : a;
        KvCall d = KV_EXPORTS[r.id];
        d.cache(kq, a, a, 4, 64, has("D48") ? 48 : 32).rows(a, a, n0 ? 0 : 5)
            .lens(has("nolengths") ? nullptr : a32, append ? a32 : nullptr, has("over") ? (append ? 60 : 65) : 40)
            .query(a, a, a, has("M17") ? 17 : 4, has("Gneg") ? -1 : 2, 1, 0, 0).quant(words, words, has("stride") ? odd_st : nullptr);
        KvChecked c;
        int rc = 99;
        const bool go = kv_call_check(d, c, rc);
        bool ok = go == r.go && rc == r.code;
        if (go)       // what the launchers get: the bf16 cache, no pages, and the block_minifloat quantisers' words
            ok = ok && c.c.C == 64 && c.c.D == 32 && c.c.B == 4 && c.pages == nullptr && c.cp.k == nullptr && c.ak.span == 15 && c.ak.bias_max == 255 &&
                 c.av.shift == 8.0f && c.av.mant_max == 7.0f && (append || (c.G == 2 && c.aq.span == 15 && c.ap.shift == 8.0f && c.causal == 1));
        if (!ok) {
            std::printf("block_minifloat row %d (export %d, '%s'): code %d (launch %d), expected %d (launch %d)\n", n, (int)r.id, r.what, rc, (int)go,
                        r.code, (int)r.go);
            return -1;
        }
        ++n;
    }
    return n;
}

int main() {
    long long id, code, a[27], given[3], vals[3][6];
    const int len[3] = {6, 6, 4};
    int rows = 0;
    while (std::scanf("%lld %lld", &id, &code) == 2) {
        for (long long& x : a)
            if (std::scanf("%lld", &x) != 1) return 2;
        for (int h = 0; h < 3; ++h) {
            if (std::scanf("%lld", &given[h]) != 1) return 2;
            for (int i = 0; i < len[h]; ++i)
                if (std::scanf("%lld", &vals[h][i]) != 1) return 2;
        }
        int32_t qk[6], pv[6];
        int64_t st[4];
        for (int i = 0; i < 6; ++i) { qk[i] = (int32_t)vals[0][i]; pv[i] = (int32_t)vals[1][i]; }
        for (int i = 0; i < 4; ++i) st[i] = vals[2][i];
        if (id < 0 || id >= KVX_COUNT) return 2;
        const auto p = [&a](int i) { return reinterpret_cast<const void*>(static_cast<uintptr_t>(a[i])); };
        const auto p32 = [&a](int i) { return reinterpret_cast<const int32_t*>(static_cast<uintptr_t>(a[i])); };
        const auto p64 = [&a](int i) { return reinterpret_cast<const int64_t*>(static_cast<uintptr_t>(a[i])); };
        KvCall d = KV_EXPORTS[id];
        d.cache(p(0), p(1), p(2), a[14], a[15], a[19]).pools(p(0), p(1), p(2), p32(10), a[14], a[16], a[17], a[18], a[19]).sizes(p64(11), p64(12), p64(13))
            .rows(p(3), p(4), a[22]).lens(p32(8), p32(9), a[21]).query(p(5), p(6), p(7), a[20], (int32_t)a[23], (int32_t)a[24], a[25], (int32_t)a[26])
            .quant(given[0] ? qk : nullptr, given[1] ? pv : nullptr, given[2] ? st : nullptr);
        KvChecked c;
        int rc = 99;
        if (kv_call_check(d, c, rc) || rc != code) {
            std::printf("row %d (export %lld): code %d, recorded %lld\n", rows, id, rc, code);
            return 1;
        }
        ++rows;
    }
    const int added = new_rows();
    const int added_bm = bm_rows();
    if (added < 0 || added_bm < 0) return 1;
    std::printf("kv_call_rows: %d rows, every code as recorded; %d rows of the paged int8-mantissa ids and %d of the block_minifloat ids, every code as written\n",
                rows, added, added_bm);
    return rows ? 0 : 2;
}
