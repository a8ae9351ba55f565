// Host-side check of csrc/philox.hpp and of dgpamd_philox_fill's refusals (DESIGN I.23), without a device.
//
// With a plain host compiler it is the block function alone (the unsigned __int128 branch of philox_mulhi):
//   c++ -O2 -std=c++17 tools/philox_check.cpp -o build/philox_check
//   build/philox_check KEY0 KEY1 C0 C1 C2 C3 [C0 C1 C2 C3 ...]
// prints one line per counter, the four words of its block in hexadecimal (numbers in any base strtoull reads);
// tests/test_philox_host.py holds these lines to numpy.random.Philox.  Without arguments it prints the block of the zero
// counter under the zero key and checks the two mappings to doubles at their ends.
//
// Compiled with hipcc together with the kernel's file it also makes every refused call of dgpamd_philox_fill, each of which
// returns before a launch, and may run under AddressSanitizer / UBSan on a CPU (from the repository root):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined tools/philox_check.cpp \
//         -x hip dgp_amd/csrc/philox.hip -o build/philox_check && build/philox_check
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#if defined(__HIPCC__)
#include "../dgp_amd/csrc/common.hpp"
#endif
#include "../dgp_amd/csrc/philox.hpp"

static int failures = 0;

static void expect(bool ok, const char *what) {
    if (!ok) printf("FAIL %s\n", what), ++failures;
}

#if defined(__HIPCC__)
static dgpamd_ctx *ctx;

struct Fill {
    dgpamd_ctx *ctx;
    int kind;
    uint64_t key0, key1, stream, c2_first;
    int64_t rounds, P, R;
    int D;
    void *out;
};

static void refused(const Fill &c, const char *what, const char *text) {
    char want[256];
    snprintf(want, sizeof want, "dgpamd_philox_fill: %s", text);
    ctx->err[0] = 0;
    const int rc = dgpamd_philox_fill(c.ctx, c.kind, c.key0, c.key1, c.stream, c.c2_first, c.rounds, c.P, c.R, c.D, c.out);
    if (rc != DGPAMD_BAD_ARG || (c.ctx && strcmp(ctx->err, want))) {
        printf("FAIL dgpamd_philox_fill with %s -> %d \"%s\", expected %d \"%s\"\n", what, rc, ctx->err, DGPAMD_BAD_ARG, want);
        ++failures;
    }
}
// a call that differs from an accepted one by `change`
#define REFUSED(change, text) \
    do {                      \
        Fill c = ok;          \
        change;               \
        refused(c, #change, text); \
    } while (0)

static void refusals() {
    ctx = new dgpamd_ctx();
    ctx->stream = nullptr;
    ctx->err[0] = 0;
    double d[4] = {0};                                          // stands for the device pointer: never dereferenced before a launch
    static_assert(DGPAMD_PHILOX_BITS == 0 && DGPAMD_PHILOX_UNIFORM == 1 && DGPAMD_PHILOX_LOG_UNIFORM == 2 &&
                      DGPAMD_PHILOX_NORMAL == 3 && DGPAMD_PHILOX_COUNT == 4,
                  "the numbers that ops.py restates");
    const Fill ok = {ctx, DGPAMD_PHILOX_NORMAL, 1, 2, 1, 0, 3, 2, 5, 7, d};
    REFUSED(c.ctx = nullptr, "");
    REFUSED(c.kind = -1, "kind must be one of DGPAMD_PHILOX_*");
    REFUSED(c.kind = DGPAMD_PHILOX_COUNT, "kind must be one of DGPAMD_PHILOX_*");
    const char *counts = "need rounds >= 1, P >= 1 and R >= 1";
    REFUSED(c.rounds = 0, counts);
    REFUSED(c.rounds = -4, counts);
    REFUSED(c.P = 0, counts);
    REFUSED(c.P = -1, counts);
    REFUSED(c.R = 0, counts);
    REFUSED(c.R = -1, counts);
    REFUSED(c.D = 0, "need 1 <= D <= DGPAMD_MAXD");
    REFUSED(c.D = -2, "need 1 <= D <= DGPAMD_MAXD");
    REFUSED(c.D = DGPAMD_MAXD + 1, "need 1 <= D <= DGPAMD_MAXD");
    const char *fields = "need P < 2^31 and R < 2^32";
    REFUSED(c.P = 1LL << 31, fields);
    REFUSED(c.P = 1LL << 62, fields);
    REFUSED(c.R = 1LL << 32, fields);
    REFUSED(c.R = 1LL << 62, fields);
    REFUSED((c.c2_first = ~0ULL, c.rounds = 1), "c2_first + rounds wraps");
    REFUSED((c.c2_first = ~0ULL - 2, c.rounds = 3), "c2_first + rounds wraps");
    REFUSED((c.c2_first = (1ULL << 63) + 1, c.rounds = INT64_MAX), "c2_first + rounds wraps");
    const char *size = "rounds P R must not pass 2^56";
    REFUSED((c.P = (1LL << 31) - 1, c.R = (1LL << 32) - 1), size);                 // (P R alone passes it)
    REFUSED((c.rounds = 1LL << 55, c.P = 1, c.R = 3), size);
    REFUSED((c.rounds = INT64_MAX, c.c2_first = 0), size);                          // (rounds P R would overflow)
    REFUSED(c.out = nullptr, "null pointer");
    delete ctx;
}
#endif

int main(int argc, char **argv) {
    if (argc > 1 && (argc < 7 || (argc - 3) % 4)) {
        fprintf(stderr, "usage: %s [KEY0 KEY1 C0 C1 C2 C3 [C0 C1 C2 C3 ...]]\n", argv[0]);
        return 2;
    }
    if (argc > 1) {
        const uint64_t k0 = strtoull(argv[1], nullptr, 0), k1 = strtoull(argv[2], nullptr, 0);
        for (int i = 3; i + 3 < argc; i += 4) {
            uint64_t c[4];
            for (int j = 0; j < 4; ++j) c[j] = strtoull(argv[i + j], nullptr, 0);
            philox4x64_10(c, k0, k1);
            printf("%016llx %016llx %016llx %016llx\n", (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)c[2],
                   (unsigned long long)c[3]);
        }
        return 0;
    }
    uint64_t c[4] = {0, 0, 0, 0};
    philox4x64_10(c, 0, 0);
    printf("%016llx %016llx %016llx %016llx\n", (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)c[2],
           (unsigned long long)c[3]);
    // the slot's counter: element e of slot (p, r) in round c2 of a stream is word e mod 4 of this block
    uint64_t w[4], v[4] = {1 + 3, (5ULL << 32) | 7, 9, 2};
    philox_slot_block(w, 11, 13, 2, 9, 5, 7, 3);
    philox4x64_10(v, 11, 13);
    expect(!memcmp(w, v, sizeof w), "philox_slot_block's counter words");
    expect(philox_uniform(0) == 0.0 && philox_uniform(~0ULL) == 1.0 - 1.0 / 9007199254740992.0 && philox_uniform(2047) == 0.0 &&
               philox_uniform(2048) == 1.0 / 9007199254740992.0,
           "philox_uniform's ends");
    expect(philox_uniform_open0(0) == 1.0 / 9007199254740992.0 && philox_uniform_open0(~0ULL) == 1.0, "philox_uniform_open0's ends");
#if defined(__HIPCC__)
    refusals();
#endif
    printf(failures ? "philox_check: %d FAILED\n" : "philox_check: ok\n", failures);
    return failures ? 1 : 0;
}
