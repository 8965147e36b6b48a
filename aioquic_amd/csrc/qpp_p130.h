// qpp_p130.h -- Poly1305 arithmetic mod 2^130 - 5 in radix 2^26 with lazy
// carries (RFC 8439 sec. 2.5), for the ChaCha20-Poly1305 kernels.  VALU only.
//
// Plain C++ so that the CPU unit test (tests/p130_host.cc) builds it for the
// host; the DPP forms (p130_from_lane, p130_quad_sum) stay in the engine.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include "qpp_device.h"
#define QPP_P130_FN __device__ __forceinline__
#else
#define QPP_P130_FN inline
namespace qpp {
struct u32x4 {
    uint32_t x, y, z, w;
};
}  // namespace qpp
#endif

namespace qpp {

struct P130 {
    uint32_t v[5];  // 26-bit limbs (slightly larger between reductions)
};

constexpr uint32_t kM26 = 0x3ffffff;

QPP_P130_FN P130 p130_zero() { return P130{{0, 0, 0, 0, 0}}; }

// 16-byte little-endian block plus 2^128 (every AEAD block is full, RFC 8439 sec. 2.8)
QPP_P130_FN P130 p130_block(u32x4 m)
{
    return P130{{m.x & kM26, ((m.x >> 26) | (m.y << 6)) & kM26, ((m.y >> 20) | (m.z << 12)) & kM26,
                 ((m.z >> 14) | (m.w << 18)) & kM26, (m.w >> 8) | (1u << 24)}};
}

QPP_P130_FN P130 p130_add(P130 a, P130 b)
{
    return P130{{a.v[0] + b.v[0], a.v[1] + b.v[1], a.v[2] + b.v[2], a.v[3] + b.v[3],
                 a.v[4] + b.v[4]}};
}

// h * r mod 2^130-5 with partial carry, for h limbs < 2^29 and r limbs
// < 2^26 + 2^11 (5 r fits 32 bits, a column sum stays below 2^60).  The
// result's limbs are < 2^26 but limb 1, which takes the fold's carry on top:
// < 2^26 + 2^8 (the fold adds at most 201 at those bounds).  Such a result
// serves as either operand again (tests/test_p130_host.py holds the bounds).
QPP_P130_FN P130 p130_mul(P130 h, P130 r)
{
    const uint32_t r0 = r.v[0], r1 = r.v[1], r2 = r.v[2], r3 = r.v[3], r4 = r.v[4];
    const uint32_t s1 = r1 * 5, s2 = r2 * 5, s3 = r3 * 5, s4 = r4 * 5;
    const uint64_t h0 = h.v[0], h1 = h.v[1], h2 = h.v[2], h3 = h.v[3], h4 = h.v[4];
    uint64_t d0 = h0 * r0 + h1 * s4 + h2 * s3 + h3 * s2 + h4 * s1;
    uint64_t d1 = h0 * r1 + h1 * r0 + h2 * s4 + h3 * s3 + h4 * s2;
    uint64_t d2 = h0 * r2 + h1 * r1 + h2 * r0 + h3 * s4 + h4 * s3;
    uint64_t d3 = h0 * r3 + h1 * r2 + h2 * r1 + h3 * r0 + h4 * s4;
    uint64_t d4 = h0 * r4 + h1 * r3 + h2 * r2 + h3 * r1 + h4 * r0;
    d1 += d0 >> 26;
    d2 += d1 >> 26;
    d3 += d2 >> 26;
    d4 += d3 >> 26;
    uint32_t o0 = (uint32_t)d0 & kM26, o1 = (uint32_t)d1 & kM26, o2 = (uint32_t)d2 & kM26;
    uint32_t o3 = (uint32_t)d3 & kM26, o4 = (uint32_t)d4 & kM26;
    uint64_t c = (d4 >> 26) * 5 + o0;
    o0 = (uint32_t)c & kM26;
    o1 += (uint32_t)(c >> 26);
    return P130{{o0, o1, o2, o3, o4}};
}

// d += h * r: the five 64-bit column sums of p130_mul without its carry.  A
// sum of four such products stays below 2^61 for h limbs <= 2^27 + 2^14 (a
// block plus a carried chain) and r limbs < 2^26 + 2^11 (each column < 2^57.8
// per product), so four blocks of a chunk can be multiplied by their own
// powers of r and carried once (p130_carry).
QPP_P130_FN void p130_mac(uint64_t (&d)[5], P130 h, P130 r)
{
    const uint32_t r0 = r.v[0], r1 = r.v[1], r2 = r.v[2], r3 = r.v[3], r4 = r.v[4];
    const uint32_t s1 = r1 * 5, s2 = r2 * 5, s3 = r3 * 5, s4 = r4 * 5;
    const uint64_t h0 = h.v[0], h1 = h.v[1], h2 = h.v[2], h3 = h.v[3], h4 = h.v[4];
    d[0] += h0 * r0 + h1 * s4 + h2 * s3 + h3 * s2 + h4 * s1;
    d[1] += h0 * r1 + h1 * r0 + h2 * s4 + h3 * s3 + h4 * s2;
    d[2] += h0 * r2 + h1 * r1 + h2 * r0 + h3 * s4 + h4 * s3;
    d[3] += h0 * r3 + h1 * r2 + h2 * r1 + h3 * r0 + h4 * s4;
    d[4] += h0 * r4 + h1 * r3 + h2 * r2 + h3 * r1 + h4 * r0;
}

// the partial carry of p130_mul on column sums below 2^61: limbs < 2^26 but
// limb 1 < 2^26 + 2^8
QPP_P130_FN P130 p130_carry(uint64_t d0, uint64_t d1, uint64_t d2, uint64_t d3, uint64_t d4)
{
    d1 += d0 >> 26;
    d2 += d1 >> 26;
    d3 += d2 >> 26;
    d4 += d3 >> 26;
    uint32_t o0 = (uint32_t)d0 & kM26, o1 = (uint32_t)d1 & kM26, o2 = (uint32_t)d2 & kM26;
    uint32_t o3 = (uint32_t)d3 & kM26, o4 = (uint32_t)d4 & kM26;
    uint64_t c = (d4 >> 26) * 5 + o0;
    o0 = (uint32_t)c & kM26;
    o1 += (uint32_t)(c >> 26);
    return P130{{o0, o1, o2, o3, o4}};
}

// clamp(r) from the first 16 bytes of the one-time key (RFC 8439 sec. 2.5)
QPP_P130_FN P130 p130_r(uint32_t k0, uint32_t k1, uint32_t k2, uint32_t k3)
{
    k0 &= 0x0fffffff; k1 &= 0x0ffffffc; k2 &= 0x0ffffffc; k3 &= 0x0ffffffc;
    return P130{{k0 & kM26, ((k0 >> 26) | (k1 << 6)) & kM26, ((k1 >> 20) | (k2 << 12)) & kM26,
                 ((k2 >> 14) | (k3 << 18)) & kM26, k3 >> 8}};
}

// Full reduction mod 2^130-5, then + s mod 2^128 -> tag words.  h is a
// limb-wise sum, not a carried value: chacha_packet adds two p130_mul results
// (every limb < 2^27 + 2^9), k_lone_chacha sums p130_mul results over up to
// ~50 lanes; any limbs <= 50 * 2^26 do (no sum below leaves 32 bits).
//
// Two full carry passes, each ending with the fold of limb 4's carry into
// limb 0 (2^130 = 5 mod p), then one carry out of limb 0.  Every limb is
// < 2^26 after that:
//   pass 1  carries are <= 50, so the fold adds <= 250 to h0 (< 2^32) and
//           leaves h1..h4 < 2^26;
//   pass 2  h0's carry c0 is <= 50, and h1 + c0 < 2^26 + 50, so every later
//           carry of the pass is 0 or 1.  If the last one (out of h4) is 1,
//           the chain rippled through h1..h4, which leaves h1 <= 49 and
//           h2 = h3 = h4 = 0; the fold then adds 5 to h0 < 2^26;
//   last    without a second fold h0 < 2^26 and nothing moves; with it
//           h0 < 2^26 + 5 carries at most 1 into h1 <= 49.  No further carry
//           can occur.
// (Stopping pass 2 at h2, as this function once did, left h2 = 2^26 when the
// h1 -> h2 carry met h2 = 2^26 - 1: the packing below then lost bit 46 and
// ORed bit 14 of w2 where it must add -- a wrong tag whenever h3 was odd.)
QPP_P130_FN u32x4 p130_finish(P130 h, uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3)
{
    uint32_t h0 = h.v[0], h1 = h.v[1], h2 = h.v[2], h3 = h.v[3], h4 = h.v[4], c;
    c = h1 >> 26; h1 &= kM26; h2 += c;
    c = h2 >> 26; h2 &= kM26; h3 += c;
    c = h3 >> 26; h3 &= kM26; h4 += c;
    c = h4 >> 26; h4 &= kM26; h0 += c * 5;
    c = h0 >> 26; h0 &= kM26; h1 += c;
    c = h1 >> 26; h1 &= kM26; h2 += c;
    c = h2 >> 26; h2 &= kM26; h3 += c;
    c = h3 >> 26; h3 &= kM26; h4 += c;
    c = h4 >> 26; h4 &= kM26; h0 += c * 5;
    c = h0 >> 26; h0 &= kM26; h1 += c;
    // g = h + 5 - 2^130; take g when it does not borrow
    uint32_t g0 = h0 + 5; c = g0 >> 26; g0 &= kM26;
    uint32_t g1 = h1 + c; c = g1 >> 26; g1 &= kM26;
    uint32_t g2 = h2 + c; c = g2 >> 26; g2 &= kM26;
    uint32_t g3 = h3 + c; c = g3 >> 26; g3 &= kM26;
    uint32_t g4 = h4 + c - (1u << 26);
    uint32_t keep_h = (uint32_t)((int32_t)g4 >> 31);  // all ones if g4 borrowed
    h0 = (h0 & keep_h) | (g0 & ~keep_h);
    h1 = (h1 & keep_h) | (g1 & ~keep_h);
    h2 = (h2 & keep_h) | (g2 & ~keep_h);
    h3 = (h3 & keep_h) | (g3 & ~keep_h);
    h4 = (h4 & keep_h) | (g4 & ~keep_h);
    uint32_t w0 = h0 | (h1 << 26), w1 = (h1 >> 6) | (h2 << 20), w2 = (h2 >> 12) | (h3 << 14),
             w3 = (h3 >> 18) | (h4 << 8);
    uint64_t f = (uint64_t)w0 + s0;
    w0 = (uint32_t)f;
    f = (uint64_t)w1 + s1 + (f >> 32);
    w1 = (uint32_t)f;
    f = (uint64_t)w2 + s2 + (f >> 32);
    w2 = (uint32_t)f;
    w3 = w3 + s3 + (uint32_t)(f >> 32);
    return u32x4{w0, w1, w2, w3};
}

}  // namespace qpp
