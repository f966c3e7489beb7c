// Stand-alone host program (its own main, no GPU, nothing loaded into Python): csrc/mi355q_kv_copy.h's kv_copy_check -- the argument
// check of mi355q_bfp_kv_paged_copy and, with int8 = true, of mi355q_bfp_kv8_paged_copy -- over the rows below, each under both, for a sanitizer build.  Pointers are made-up addresses: the check never
// dereferences one.  Exits 1 at the first row whose code differs from the one written next to it, or whose launch arguments are wrong.
// Build and run: see the Makefile next to this file (`make -C tools/kv_call_check check_copy`).
#include <cstdio>

#include "mi355q_kv_copy.h"

using namespace mi355q;

struct Row {
    long long kq, vq, src, dst, jobs, n_jobs, B, num_pages, P, D;
    int code;
    bool launch;
};

int main() {
    const long long a = 0x1000, b = 0x2000;
    const Row rows[] = {
        {a, a, a, b, a, 3, 4, 12, 32, 32, 0, true},
        {a, a, a, b, a, 65535, 65535, 0x7FFFFFFF, 1LL << 30, 128, 0, true},
        {0, 0, 0, 0, 0, 0, 4, 12, 32, 32, 0, false},                       // nothing to do: every pointer NULL
        {a, a, a, b, a, -1, 4, 12, 32, 32, MI355Q_E_BADARG, false},
        {a, a, a, b, a, 3, 0, 12, 32, 32, MI355Q_E_BADARG, false},
        {a, a, a, b, a, 3, 65536, 12, 32, 32, MI355Q_E_BADARG, false},
        {a, a, a, b, a, 3, 4, 0, 32, 32, MI355Q_E_BADARG, false},
        {a, a, a, b, a, 3, 4, 12, 16, 32, MI355Q_E_BADARG, false},
        {a, a, a, b, a, 3, 4, 12, 48, 32, MI355Q_E_BADARG, false},
        {a, a, a, b, a, 0, 4, 12, 96, 32, MI355Q_E_BADARG, false},         // the shape is checked before "nothing to do"
        {a, a, a, b, a, 3, 4, 12, 1LL << 31, 32, MI355Q_E_BADARG, false},
        {a, a, a, b, a, 3, 4, 12, 32, 0, MI355Q_E_BADARG, false},
        {a, a, a, b, a, 3, 4, 12, 32, 48, MI355Q_E_BADARG, false},
        {a, a, a, b, a, 3, 4, 12, 32, 160, MI355Q_E_BADARG, false},
        {0, a, a, b, a, 3, 4, 12, 32, 32, MI355Q_E_BADARG, false},
        {a, 0, a, b, a, 3, 4, 12, 32, 32, MI355Q_E_BADARG, false},
        {a, a, 0, b, a, 3, 4, 12, 32, 32, MI355Q_E_BADARG, false},
        {a, a, a, 0, a, 3, 4, 12, 32, 32, MI355Q_E_BADARG, false},
        {a, a, a, b, 0, 3, 4, 12, 32, 32, MI355Q_E_BADARG, false},
        {a, a, a, a, a, 3, 4, 12, 32, 32, MI355Q_E_BADARG, false},         // never in place
        {a, a, a, b, a, 65536, 4, 12, 32, 32, MI355Q_E_UNSUPPORTED, false},
        {a + 8, a, a, b, a, 3, 4, 12, 32, 32, MI355Q_E_ALIGN, false},
        {a, a, a, b + 4, a, 3, 4, 12, 32, 32, MI355Q_E_ALIGN, false},
        {a, a, a, b, a + 8, 3, 4, 12, 32, 32, MI355Q_E_ALIGN, false},
    };
    int n = 0;
    for (const bool int8 : {false, true})
        for (const Row& r : rows) {
            const auto p = [](long long x) { return reinterpret_cast<const void*>(static_cast<uintptr_t>(x)); };
            KvCopyArgs g;
            int rc = 99;
            const bool go = kv_copy_check(p(r.kq), p(r.vq), p(r.src), p(r.dst), p(r.jobs), r.n_jobs, r.B, r.num_pages, r.P, r.D, int8, g, rc);
            bool ok = go == r.launch && rc == r.code;
            if (go)     // what the kernel is given: a page of one pool in 16-byte units (bf16: 2 bytes a value; int8: 17 / 16), a row's stage,
                        // and a grid that covers both
                ok = ok && g.page_units * 16 == (int8 ? r.P * r.D * 17 / 16 : r.P * r.D * 2) && g.stage_units == 4 * r.D && g.n_jobs == r.n_jobs &&
                     g.B == r.B && g.num_pages == r.num_pages && kv_copy_blocks(g) * KV_COPY_THREADS >= 2 * g.page_units + g.stage_units &&
                     kv_copy_blocks(g) < (1LL << 31);
            if (!ok) {
                std::printf("row %d (int8 %d): code %d (launch %d), expected %d (launch %d)\n", n, (int)int8, rc, (int)go, r.code, (int)r.launch);
                return 1;
            }
            ++n;
        }
    {   // the page of P = D = 32 in 544-byte pieces: 68 units, no multiple of a wave's 64
        KvCopyArgs g;
        int rc = 99;
        const auto p = [](long long x) { return reinterpret_cast<const void*>(static_cast<uintptr_t>(x)); };
        if (!kv_copy_check(p(a), p(a), p(a), p(b), p(a), 1, 4, 12, 32, 32, true, g, rc) || g.page_units != 68 || kv_copy_blocks(g) != 2) {      // (2 x 68 + 128 stage units: two blocks of 256)
            std::printf("int8 page of P = D = 32: %lld units\n", g.page_units);
            return 1;
        }
    }
    std::printf("kv_copy_rows: %d rows, every code as written\n", n);
    return 0;
}
