// Stand-alone host program (its own main, no GPU, nothing loaded into Python): csrc/mi355q_kv_call.h's kv_call_check over rows of
// tests/golden/kv_api_codes.json / .npz, for a sanitizer build.  Reads the lines `python tools/record_kv_api_codes.py --dump N` writes:
//   export id, recorded code, the 27 flat arguments of mi355q_debug_kv_call, then for qk_params, pv_params and strides a 0 / 1 "given"
//   and their 6, 6 and 4 values
// and exits 1 at the first row whose code differs or that would launch.  Build and run: see the Makefile next to this file.
#include <cstdio>

#include "mi355q_kv_call.h"

using namespace mi355q;

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
    std::printf("kv_call_rows: %d rows, every code as recorded\n", rows);
    return rows ? 0 : 2;
}
