// Philox4x64-10 (Salmon, Moraes, Dror and Shaw 2011), the block function of numpy.random.Philox, and the counter contract of
// dgpamd_philox_fill (DESIGN I.23).  Plain C++ for host and device: a host program checks the bits without a GPU
// (tools/philox_check.cpp).  The 64 x 64 -> 128 bit product is __umul64hi on the device and unsigned __int128 on the host.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PHILOX_HD __host__ __device__ inline
#else
#define PHILOX_HD inline
#endif

#define PHILOX_M0 0xD2E7470EE14C6C93ULL
#define PHILOX_M1 0xCA5A826395121157ULL
#define PHILOX_W0 0x9E3779B97F4A7C15ULL       // the key's increments, before rounds 2 .. 10
#define PHILOX_W1 0xBB67AE8584CAA73BULL
#define PHILOX_ROUNDS 10

PHILOX_HD uint64_t philox_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * (unsigned __int128)b) >> 64);
#endif
}

// c[0 .. 3] <- the block of counter c under key (k0, k1)
PHILOX_HD void philox4x64_10(uint64_t c[4], uint64_t k0, uint64_t k1) {
    for (int i = 0; i < PHILOX_ROUNDS; ++i) {
        if (i > 0) k0 += PHILOX_W0, k1 += PHILOX_W1;
        const uint64_t hi0 = philox_mulhi(PHILOX_M0, c[0]), lo0 = PHILOX_M0 * c[0];
        const uint64_t hi1 = philox_mulhi(PHILOX_M1, c[2]), lo1 = PHILOX_M1 * c[2];
        c[0] = hi1 ^ c[1] ^ k0, c[1] = lo1, c[2] = hi0 ^ c[3] ^ k1, c[3] = lo0;
    }
}

// The block that holds elements 4 j .. 4 j + 3 of slot (p, r) in round c2 of stream `stream`: the counter words are
// c0 = 1 + j, c1 = (p << 32) | r, c2, c3 = stream.  The 1 + makes element e the e-th output of
// numpy.random.Philox(counter=[0, c1, c2, c3], key=[k0, k1]).random_raw(): numpy increments before it generates.
PHILOX_HD void philox_slot_block(uint64_t w[4], uint64_t k0, uint64_t k1, uint64_t stream, uint64_t c2, uint64_t p, uint64_t r,
                                 uint64_t j) {
    w[0] = 1 + j, w[1] = (p << 32) | r, w[2] = c2, w[3] = stream;
    philox4x64_10(w, k0, k1);
}

// numpy's double of a word, in [0, 1): the top 53 bits
PHILOX_HD double philox_uniform(uint64_t w) { return (double)(w >> 11) * (1.0 / 9007199254740992.0); }
// the same moved up by one unit, in (0, 1]: the argument of Box and Muller's logarithm
PHILOX_HD double philox_uniform_open0(uint64_t w) { return (double)((w >> 11) + 1) * (1.0 / 9007199254740992.0); }
