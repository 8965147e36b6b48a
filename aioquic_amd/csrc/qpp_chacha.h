// qpp_chacha.h -- ChaCha20 block function for the MI355X engine (RFC 8439
// sec. 2.3), VALU only; the kernels' Poly1305 limb arithmetic (sec. 2.5) is
// qpp_p130.h, included here.
#pragma once

#include "qpp_device.h"
#include "qpp_p130.h"

namespace qpp {

#define QPP_QR(a, b, c, d)                                      \
    a += b; d = rotl(d ^ a, 16);                                \
    c += d; b = rotl(b ^ c, 12);                                \
    a += b; d = rotl(d ^ a, 8);                                 \
    c += d; b = rotl(b ^ c, 7)

// 64-byte ChaCha20 block as 16 little-endian words.
__device__ __forceinline__ void chacha_block(const uint32_t *key, uint32_t ctr, uint32_t n0,
                                             uint32_t n1, uint32_t n2, uint32_t out[16])
{
    uint32_t x0 = 0x61707865, x1 = 0x3320646e, x2 = 0x79622d32, x3 = 0x6b206574;
    uint32_t x4 = key[0], x5 = key[1], x6 = key[2], x7 = key[3];
    uint32_t x8 = key[4], x9 = key[5], x10 = key[6], x11 = key[7];
    uint32_t x12 = ctr, x13 = n0, x14 = n1, x15 = n2;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        QPP_QR(x0, x4, x8, x12);
        QPP_QR(x1, x5, x9, x13);
        QPP_QR(x2, x6, x10, x14);
        QPP_QR(x3, x7, x11, x15);
        QPP_QR(x0, x5, x10, x15);
        QPP_QR(x1, x6, x11, x12);
        QPP_QR(x2, x7, x8, x13);
        QPP_QR(x3, x4, x9, x14);
    }
    out[0] = x0 + 0x61707865; out[1] = x1 + 0x3320646e;
    out[2] = x2 + 0x79622d32; out[3] = x3 + 0x6b206574;
    out[4] = x4 + key[0]; out[5] = x5 + key[1]; out[6] = x6 + key[2]; out[7] = x7 + key[3];
    out[8] = x8 + key[4]; out[9] = x9 + key[5]; out[10] = x10 + key[6]; out[11] = x11 + key[7];
    out[12] = x12 + ctr; out[13] = x13 + n0; out[14] = x14 + n1; out[15] = x15 + n2;
}

// chacha_block with side(i) called after double round i (i = 0..9), in the
// same straight-line code: independent work placed there (Poly1305 of the
// previous chunk) shares a basic block with the rounds, so the scheduler can
// interleave the two dependency chains.
template <class SIDE>
__device__ __forceinline__ void chacha_block_beside(const uint32_t *key, uint32_t ctr, uint32_t n0,
                                                    uint32_t n1, uint32_t n2, uint32_t out[16], SIDE side)
{
    uint32_t x0 = 0x61707865, x1 = 0x3320646e, x2 = 0x79622d32, x3 = 0x6b206574;
    uint32_t x4 = key[0], x5 = key[1], x6 = key[2], x7 = key[3];
    uint32_t x8 = key[4], x9 = key[5], x10 = key[6], x11 = key[7];
    uint32_t x12 = ctr, x13 = n0, x14 = n1, x15 = n2;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        QPP_QR(x0, x4, x8, x12);
        QPP_QR(x1, x5, x9, x13);
        QPP_QR(x2, x6, x10, x14);
        QPP_QR(x3, x7, x11, x15);
        QPP_QR(x0, x5, x10, x15);
        QPP_QR(x1, x6, x11, x12);
        QPP_QR(x2, x7, x8, x13);
        QPP_QR(x3, x4, x9, x14);
        side(i);
    }
    out[0] = x0 + 0x61707865; out[1] = x1 + 0x3320646e;
    out[2] = x2 + 0x79622d32; out[3] = x3 + 0x6b206574;
    out[4] = x4 + key[0]; out[5] = x5 + key[1]; out[6] = x6 + key[2]; out[7] = x7 + key[3];
    out[8] = x8 + key[4]; out[9] = x9 + key[5]; out[10] = x10 + key[6]; out[11] = x11 + key[7];
    out[12] = x12 + ctr; out[13] = x13 + n0; out[14] = x14 + n1; out[15] = x15 + n2;
}

// One ChaCha20 block computed by the 4 lanes of a quad together (all four
// hold the same inputs): lane j keeps column j (words j, 4+j, 8+j, 12+j), the
// column rounds are lane-local and the diagonal rounds rotate rows 1-3 by
// 1/2/3 lanes with DPP.  ~30 VALU per double round and 4 state registers, for
// the header-protection block every lane of the quad needs (sec. 5.4.4 of
// RFC 9001), instead of 96 VALU and 16 registers per lane for a private copy.
// Returns output words 0..3 (the first 16 keystream bytes) in every lane.
template <int CTRL>
__device__ __forceinline__ uint32_t qdpp(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xf, 0xf, false);
}

__device__ __forceinline__ u32x4 chacha_block_quad_row0(const uint32_t *key, uint32_t ctr,
                                                        uint32_t n0, uint32_t n1, uint32_t n2,
                                                        int sub)
{
    constexpr int kRot1 = 0x39, kRot2 = 0x4E, kRot3 = 0x93;  // lane j <- lane j+1 / j+2 / j+3
    const uint32_t sig = sub == 0 ? 0x61707865u : sub == 1 ? 0x3320646eu : sub == 2 ? 0x79622d32u : 0x6b206574u;
    const uint32_t kb = sub == 0 ? key[0] : sub == 1 ? key[1] : sub == 2 ? key[2] : key[3];
    const uint32_t kc = sub == 0 ? key[4] : sub == 1 ? key[5] : sub == 2 ? key[6] : key[7];
    const uint32_t kd = sub == 0 ? ctr : sub == 1 ? n0 : sub == 2 ? n1 : n2;
    uint32_t a = sig, b = kb, c = kc, d = kd;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        QPP_QR(a, b, c, d);
        b = qdpp<kRot1>(b); c = qdpp<kRot2>(c); d = qdpp<kRot3>(d);
        QPP_QR(a, b, c, d);
        b = qdpp<kRot3>(b); c = qdpp<kRot2>(c); d = qdpp<kRot1>(d);
    }
    a += sig;  // output word `sub` of row 0
    return u32x4{qdpp<0x00>(a), qdpp<0x55>(a), qdpp<0xAA>(a), qdpp<0xFF>(a)};
}
#undef QPP_QR

}  // namespace qpp
