// qpp_te4.h -- the AES round tables, the layout of their LDS image (two
// tables, or four in the close-from-LDS form of k_gcm) and the two ways a
// round combines a column from its four lookups.  Plain C++ apart from the
// places marked below, so that the CPU unit test (tests/te4_host.cc) builds
// the same code for the host.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define QPP_TE4_HD __host__ __device__ __forceinline__
#else
#define QPP_TE4_HD inline
#endif

namespace qpp {

// AES S-box and the little-endian round table Te0 (byte r of a word = row r):
// Te0[x] = 2S(x) | S(x)<<8 | S(x)<<16 | 3S(x)<<24.  Generated at compile time
// from GF(2^8) arithmetic (FIPS-197 sec. 5.1.1), so no table is transcribed.
struct AesTables {
    uint8_t sbox[256];
    uint32_t te0[256];
};

constexpr uint8_t gf8_mul(uint8_t a, uint8_t b)
{
    uint8_t r = 0;
    for (int i = 0; i < 8; ++i) {
        if (b & 1) r ^= a;
        a = (uint8_t)((a << 1) ^ ((a & 0x80) ? 0x1b : 0));
        b >>= 1;
    }
    return r;
}

constexpr AesTables make_aes_tables()
{
    AesTables t{};
    for (int x = 0; x < 256; ++x) {
        // inverse = x^254 in GF(2^8) (0 maps to 0)
        uint8_t inv = 1, base = (uint8_t)x;
        for (int e = 254; e; e >>= 1) {
            if (e & 1) inv = gf8_mul(inv, base);
            base = gf8_mul(base, base);
        }
        uint8_t s = inv;
        for (int i = 1; i <= 4; ++i) s ^= (uint8_t)((inv << i) | (inv >> (8 - i)));
        s ^= 0x63;
        t.sbox[x] = s;
        t.te0[x] = (uint32_t)gf8_mul(s, 2) | (uint32_t)s << 8 | (uint32_t)s << 16 |
                   (uint32_t)gf8_mul(s, 3) << 24;
    }
    return t;
}

constexpr AesTables kAesTables = make_aes_tables();

// The LDS image: entry x occupies one 256-byte row of 16 parts of 16 bytes,
//   [Te0[x] copy 0..31][Te1[x] copy 0..31]              the low 64 KiB
//   [Te2[x] copy 0..31][Te3[x] copy 0..31]              the high 64 KiB
// (the high half only in the four-table image), Te_r = Te0 rotated left by 8r.
constexpr int kTeBytes = 256 * 256;

QPP_TE4_HD uint32_t te_rotl(uint32_t x, int n)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(x, x, (32 - n) & 31);
#else
    n &= 31;
    return n ? (x << n) | (x >> (32 - n)) : x;
#endif
}
QPP_TE4_HD uint32_t te_xor3(uint32_t a, uint32_t b, uint32_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
#else
    return a ^ b ^ c;
#endif
}

// the word that fills part `part` (0..15) of row x in half `half` (0: low,
// 1: high), given te0 = Te0[x]
QPP_TE4_HD uint32_t te_image_word(uint32_t te0, int half, int part)
{
    return te_rotl(te0, 16 * half + (part < 8 ? 0 : 8));
}

// One column of a round from its four lookups.
// Two tables: rows 2 and 3 come from Te0 / Te1 (e2r, e3r: not yet rotated) and
// kr is the round key rotated right by 16 (KeySlot::rkr):
//   rotl16(e2r ^ e3r ^ kr) = Te2 ^ Te3 ^ k
QPP_TE4_HD uint32_t te_col2(uint32_t e0, uint32_t e1, uint32_t e2r, uint32_t e3r, uint32_t kr)
{
    return te_xor3(e0, e1, te_rotl(te_xor3(e2r, e3r, kr), 16));
}
// Four tables: every row from its own table, the plain round key, no rotate
QPP_TE4_HD uint32_t te_col4(uint32_t e0, uint32_t e1, uint32_t e2, uint32_t e3, uint32_t k)
{
    return te_xor3(te_xor3(e0, e1, e2), e3, k);
}

}  // namespace qpp
