// qpp_device.h -- device-side building blocks of the MI355X packet-protection
// engine: AES (T-table in LDS, one table replicated per LDS bank), GHASH by
// 4-bit windowed tables in LDS, ChaCha20 and Poly1305 in VALU, and the
// unaligned byte-stream helpers.  gfx950 only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/quic_pp.h"
#include "qpp_gh5.h"
#include "qpp_te4.h"

namespace qpp {

// ---------------------------------------------------------------- tables --

// AES S-box and round table Te0, generated at compile time (qpp_te4.h)
extern __constant__ AesTables c_aes;

// -------------------------------------------------------------- key slots --

// One expanded key slot (512 bytes).  Words are little-endian views of the
// byte strings, so packet bytes are used as loaded, with no byte swapping.
struct KeySlot {
    uint32_t suite;      // QPP_AES_128_GCM / QPP_AES_256_GCM / QPP_CHACHA20_POLY1305; 0xff = empty
    uint32_t key_phase;
    uint32_t nr;         // AES rounds (10 / 14)
    uint32_t rsv;
    uint32_t iv[4];      // iv[3] = 0
    uint32_t rk[60];     // AEAD: AES round keys, or the ChaCha20 key in rk[0..7]
    uint32_t hrk[60];    // header protection: AES round keys, or the ChaCha20 HP key
    uint32_t rkr[60];    // AEAD round keys rotated right by 16 (aes_rounds<.., true>)
    uint32_t pad[4];
};
static_assert(sizeof(KeySlot) == 768, "KeySlot layout");

// GHASH tables of one slot: [power p = H^(p+1)][window w][nibble v] -> 16 bytes.
// Window w = 2*byte + (0: low nibble, 1: high nibble).  32 KiB per slot.
constexpr int kGhashPowers = 4;
constexpr int kGhashPowBytes = 32 * 16 * 16;  // one power: 32 windows x 16 nibbles x 16 B

// H^4 once more, for the GCM step loop's LDS entries, in 5-bit windows
// (qpp_gh5.h: kGh5Windows, kGh5Hi, kGh5Bytes = 14 KiB per table)
constexpr int kGh5Off = kGhashPowers * kGhashPowBytes;  // offset of the 5-bit H^4 in a slot's tables
// H^1 .. H^kGhPowCount as plain 16-byte elements, for the lone-packet kernel
// (k_lone: GHASH as sum_i X_i H^(m-i) over a packet's m <= 189 blocks), in
// their own region after every slot's tables (gh_powers), so the slot stride
// of the quad kernels' tables stays 46 KiB (round 5).
constexpr int kGhPowCount = 192;
constexpr int kGhPowBytes = kGhPowCount * 16;
constexpr int kGhashTabBytes = kGh5Off + kGh5Bytes;  // 46 KiB per slot
// byte offset of slot's H^1.. in a table of `cap` slots (round 4 kept them
// inside each slot's tables at a 49 KiB stride: config 4 measured the same
// either way, same box interleaved, profiles/r5c_config4_powers_ab.txt)
__device__ __host__ __forceinline__ size_t gh_powers_off(uint32_t cap, uint32_t slot)
{
    return (size_t)cap * kGhashTabBytes + (size_t)slot * kGhPowBytes;
}
// one LDS table entry of the GCM kernel: H^4 in the step loop's layout
constexpr int kGhLdsEntry = kGh5Bytes;

// ---------------------------------------------------------------- helpers --

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c)
{
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}
__device__ __forceinline__ u32x4 xor3(u32x4 a, u32x4 b, u32x4 c)
{
    return u32x4{xor3(a.x, b.x, c.x), xor3(a.y, b.y, c.y), xor3(a.z, b.z, c.z),
                 xor3(a.w, b.w, c.w)};
}
__device__ __forceinline__ uint32_t rotl(uint32_t x, int n)
{
    return __builtin_amdgcn_alignbit(x, x, (32 - n) & 31);
}
__device__ __forceinline__ uint32_t bswap(uint32_t x) { return __builtin_bswap32(x); }

// Unaligned 16-byte global load/store (gfx950 runs with unaligned access on).
__device__ __forceinline__ u32x4 ld16(const uint8_t *p)
{
    u32x4 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}
__device__ __forceinline__ void st16(uint8_t *p, u32x4 v) { __builtin_memcpy(p, &v, 16); }

// First n (0..16) bytes of p, zero padded.  Only the tail block of a region
// takes the byte loop.
__device__ __forceinline__ u32x4 ld_part(const uint8_t *p, int n)
{
    if (n >= 16) return ld16(p);
    uint32_t w[4] = {0, 0, 0, 0};
    for (int i = 0; i < n; ++i) w[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
    return u32x4{w[0], w[1], w[2], w[3]};
}
// First n (0..16) bytes of v to p: at most 4 stores (8, 4, 2, 1 bytes by the
// bits of n), no byte loop.
__device__ __forceinline__ void st_part(uint8_t *p, u32x4 v, int n)
{
    if (n >= 16) { st16(p, v); return; }
    uint64_t a = (uint64_t)v.y << 32 | v.x;
    const uint64_t b = (uint64_t)v.w << 32 | v.z;
    if (n & 8) { __builtin_memcpy(p, &a, 8); p += 8; a = b; }
    if (n & 4) { const uint32_t w = (uint32_t)a; __builtin_memcpy(p, &w, 4); p += 4; a >>= 32; }
    if (n & 2) { const uint16_t h = (uint16_t)a; __builtin_memcpy(p, &h, 2); p += 2; a >>= 16; }
    if (n & 1) *p = (uint8_t)a;
}
// keep only the first n bytes (GHASH / Poly1305 zero padding)
__device__ __forceinline__ u32x4 keep_bytes(u32x4 v, int n)
{
    if (n >= 16) return v;
    uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int b = n - 4 * k;
        uint32_t m = b >= 4 ? 0xffffffffu : (b <= 0 ? 0u : ((1u << (8 * b)) - 1));
        w[k] &= m;
    }
    return u32x4{w[0], w[1], w[2], w[3]};
}
__device__ __forceinline__ uint32_t byte_of(u32x4 v, int i)
{
    uint32_t w = (i < 4) ? v.x : (i < 8) ? v.y : (i < 12) ? v.z : v.w;
    return (w >> (8 * (i & 3))) & 0xff;
}

// Lane id recomputed where it is used (2 VALU): volatile, so the compiler
// cannot hoist it and keep lane-derived addresses live (or spilled) across a
// register-tight loop.
__device__ __forceinline__ uint32_t lane_fresh()
{
    uint32_t l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

// A zero vector materialised where it is used (the compiler otherwise keeps
// one live across the packet loops, and spills it).
__device__ __forceinline__ u32x4 zero4()
{
    uint32_t z;
    asm volatile("v_mov_b32 %0, 0" : "=v"(z));
    return u32x4{z, z, z, z};
}

// Wave-wide minimum, returned wave-uniform.  DPP within each 16-lane row
// (quad swaps, half-row and row mirrors), then the four row minima by
// v_readlane: no lane-address registers, which the compiler would otherwise
// keep live (spilled) across the packet loops for the next reduction.
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_mov(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xf, 0xf, false);
}
constexpr int kDppQuadSwap1 = 0xB1, kDppQuadSwap2 = 0x4E, kDppHalfMirror = 0x141, kDppMirror = 0x140;

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v)
{
    v = min(v, dpp_mov<kDppQuadSwap1>(v));
    v = min(v, dpp_mov<kDppQuadSwap2>(v));
    v = min(v, dpp_mov<kDppHalfMirror>(v));
    v = min(v, dpp_mov<kDppMirror>(v));
    const uint32_t a = min((uint32_t)__builtin_amdgcn_readlane((int)v, 0),
                           (uint32_t)__builtin_amdgcn_readlane((int)v, 16));
    const uint32_t b = min((uint32_t)__builtin_amdgcn_readlane((int)v, 32),
                           (uint32_t)__builtin_amdgcn_readlane((int)v, 48));
    return min(a, b);
}

__device__ __forceinline__ uint64_t min_u64_dpp_step(uint64_t v, uint32_t lo2, uint32_t hi2)
{
    const uint64_t w = (uint64_t)hi2 << 32 | lo2;
    return w < v ? w : v;
}

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v)
{
#define QPP_MIN64_STEP(CTRL)                                                              \
    v = min_u64_dpp_step(v, dpp_mov<CTRL>((uint32_t)v), dpp_mov<CTRL>((uint32_t)(v >> 32)))
    QPP_MIN64_STEP(kDppQuadSwap1);
    QPP_MIN64_STEP(kDppQuadSwap2);
    QPP_MIN64_STEP(kDppHalfMirror);
    QPP_MIN64_STEP(kDppMirror);
#undef QPP_MIN64_STEP
    uint64_t m = ~0ull;
#pragma unroll
    for (int r = 0; r < 64; r += 16) {
        const uint64_t w = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), r) << 32 |
                           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, r);
        m = w < m ? w : m;
    }
    return m;
}

// DPP within a quad of lanes (the 4 lanes that share one packet).
template <int CTRL>
__device__ __forceinline__ uint32_t quad_perm(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xf, 0xf, false);
}
constexpr int kQuadSwap1 = 0xB1;  // [1,0,3,2]
constexpr int kQuadSwap2 = 0x4E;  // [2,3,0,1]
__device__ __forceinline__ u32x4 quad_xor_all(u32x4 v)
{
    v.x ^= quad_perm<kQuadSwap1>(v.x);
    v.y ^= quad_perm<kQuadSwap1>(v.y);
    v.z ^= quad_perm<kQuadSwap1>(v.z);
    v.w ^= quad_perm<kQuadSwap1>(v.w);
    v.x ^= quad_perm<kQuadSwap2>(v.x);
    v.y ^= quad_perm<kQuadSwap2>(v.y);
    v.z ^= quad_perm<kQuadSwap2>(v.z);
    v.w ^= quad_perm<kQuadSwap2>(v.w);
    return v;
}

// ------------------------------------------------------------------- AES --

// T-table lookups.  A lookup object provides, for byte r of a state word s,
//   t<r>(s) = Te_r[byte r of s]  (Te_r = Te0 rotated left by 8r)
// The LDS image holds Te0 and Te1, each replicated 32 times so lane l always
// reads bank (l & 31): entry x occupies one 256-byte row,
//   [Te0[x] copy 0..31][Te1[x] copy 0..31],
// so the address of byte r of s is (byte_r(s) << 8) | (lane&31)*4 -- a single
// v_perm -- with Te1 at immediate offset +128.  Te2 / Te3 are Te0 / Te1
// rotated by 16.  64 KiB of LDS (kTeBytes, qpp_te4.h).

struct LdsTe {
    static constexpr bool kFourTables = false;
    const uint8_t *te;  // LDS base of the 64 KiB image
    uint32_t lo;        // (lane & 31) * 4
    template <int R>
    __device__ __forceinline__ uint32_t addr(uint32_t s) const
    {
        // bytes {S0=s, S1=lo}: result byte0 = lo.byte0, byte1 = s.byte R, bytes 2,3 = 0
        // (round 4: byte 1 as (s & 0xff00) | lo, one v_and_or_b32 instead of
        // the v_perm, measured -0.3 % at the north star, -1.2 % config 2,
        // +0.6 % config 4 on one box, profiles/r4s_ab_addr_andor.txt: kept)
        return __builtin_amdgcn_perm(s, lo, 0x0c0c0000u | ((4u + R) << 8));
    }
    __device__ __forceinline__ uint32_t t0(uint32_t s) const
    {
        return *(const uint32_t *)(te + addr<0>(s));
    }
    __device__ __forceinline__ uint32_t t1(uint32_t s) const
    {
        return *(const uint32_t *)(te + 128 + addr<1>(s));
    }
    __device__ __forceinline__ uint32_t t2(uint32_t s) const
    {
        return rotl(*(const uint32_t *)(te + addr<2>(s)), 16);
    }
    __device__ __forceinline__ uint32_t t3(uint32_t s) const
    {
        return rotl(*(const uint32_t *)(te + 128 + addr<3>(s)), 16);
    }
    // t2 / t3 before their rotation by 16 (rotl16(t2r ^ t3r ^ k') = t2 ^ t3 ^ rotl16(k'))
    __device__ __forceinline__ uint32_t t2r(uint32_t s) const
    {
        return *(const uint32_t *)(te + addr<2>(s));
    }
    __device__ __forceinline__ uint32_t t3r(uint32_t s) const
    {
        return *(const uint32_t *)(te + 128 + addr<3>(s));
    }
    // final round: S(x) placed at byte r.  Te0 = (2S,S,S,3S), Te1 = (3S,2S,S,S)
    __device__ __forceinline__ uint32_t f0(uint32_t s) const
    {
        return (*(const uint32_t *)(te + addr<0>(s)) >> 8) & 0xffu;
    }
    __device__ __forceinline__ uint32_t f1(uint32_t s) const
    {
        return *(const uint32_t *)(te + addr<1>(s)) & 0xff00u;
    }
    __device__ __forceinline__ uint32_t f2(uint32_t s) const
    {
        return *(const uint32_t *)(te + 128 + addr<2>(s)) & 0xff0000u;
    }
    __device__ __forceinline__ uint32_t f3(uint32_t s) const
    {
        return *(const uint32_t *)(te + 128 + addr<3>(s)) & 0xff000000u;
    }
    // the same entries unmasked: S(x) is byte 1 of fr0 / fr1, byte 2 of fr2,
    // byte 3 of fr3 (fin_col merges them with two v_perm)
    __device__ __forceinline__ uint32_t fr0(uint32_t s) const { return *(const uint32_t *)(te + addr<0>(s)); }
    __device__ __forceinline__ uint32_t fr1(uint32_t s) const { return *(const uint32_t *)(te + addr<1>(s)); }
    __device__ __forceinline__ uint32_t fr2(uint32_t s) const { return *(const uint32_t *)(te + 128 + addr<2>(s)); }
    __device__ __forceinline__ uint32_t fr3(uint32_t s) const { return *(const uint32_t *)(te + 128 + addr<3>(s)); }
};

// The four-table image (128 KiB: the close-from-LDS form of k_gcm): Te2 | Te3
// in a second 64 KiB after Te0 | Te1, in the same row layout, so rows 2 and 3
// need no rotate.  The second half lies beyond the 16-bit ds_read immediate,
// so its bit 16 rides in the per-lane constant, and the one v_perm of the
// address takes result byte 2 from it for rows 2 and 3 and a zero for rows 0
// and 1 (and for the final round, which reads S(x) from the low half).
struct LdsTe4 {
    static constexpr bool kFourTables = true;
    const uint8_t *te;  // LDS base of the 128 KiB image
    uint32_t lo;        // (lane & 31) * 4 | 0x10000
    // HI: the high half
    template <int R, bool HI>
    __device__ __forceinline__ uint32_t addr(uint32_t s) const
    {
        // result byte0 = lo.byte0, byte1 = s.byte R, byte2 = lo.byte2 (= 1) or 0, byte3 = 0
        return __builtin_amdgcn_perm(s, lo, (HI ? 0x0c020000u : 0x0c0c0000u) | ((4u + R) << 8));
    }
    __device__ __forceinline__ uint32_t t0(uint32_t s) const { return *(const uint32_t *)(te + addr<0, false>(s)); }
    __device__ __forceinline__ uint32_t t1(uint32_t s) const { return *(const uint32_t *)(te + 128 + addr<1, false>(s)); }
    __device__ __forceinline__ uint32_t t2(uint32_t s) const { return *(const uint32_t *)(te + addr<2, true>(s)); }
    __device__ __forceinline__ uint32_t t3(uint32_t s) const { return *(const uint32_t *)(te + 128 + addr<3, true>(s)); }
    // final round, as LdsTe's
    __device__ __forceinline__ uint32_t f0(uint32_t s) const { return (fr0(s) >> 8) & 0xffu; }
    __device__ __forceinline__ uint32_t f1(uint32_t s) const { return fr1(s) & 0xff00u; }
    __device__ __forceinline__ uint32_t f2(uint32_t s) const { return fr2(s) & 0xff0000u; }
    __device__ __forceinline__ uint32_t f3(uint32_t s) const { return fr3(s) & 0xff000000u; }
    __device__ __forceinline__ uint32_t fr0(uint32_t s) const { return *(const uint32_t *)(te + addr<0, false>(s)); }
    __device__ __forceinline__ uint32_t fr1(uint32_t s) const { return *(const uint32_t *)(te + addr<1, false>(s)); }
    __device__ __forceinline__ uint32_t fr2(uint32_t s) const { return *(const uint32_t *)(te + 128 + addr<2, false>(s)); }
    __device__ __forceinline__ uint32_t fr3(uint32_t s) const { return *(const uint32_t *)(te + 128 + addr<3, false>(s)); }
};

// One output column of the final round from the raw lookups of LdsTe::fr0..3:
// bytes S(a0) S(a1) by one v_perm, S(a2) S(a3) by another, then (| , ^ k) in
// one v_bitop3 -- 3 VALU instead of 4 masks / shifts, 3 ors and an xor.
__device__ __forceinline__ uint32_t fin_col(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, uint32_t k)
{
    const uint32_t lo = __builtin_amdgcn_perm(r1, r0, 0x0c0c0501u);  // [r0.b1, r1.b1, 0, 0]
    const uint32_t hi = __builtin_amdgcn_perm(r3, r2, 0x07020c0cu);  // [0, 0, r2.b2, r3.b3]
    return __builtin_amdgcn_bitop3_b32(lo, hi, k, 0x56);            // (lo | hi) ^ k
}

// Constant-memory lookups (key setup and other cold paths).
struct ConstTe {
    __device__ __forceinline__ uint32_t t0(uint32_t s) const { return c_aes.te0[s & 255]; }
    __device__ __forceinline__ uint32_t t1(uint32_t s) const { return rotl(c_aes.te0[(s >> 8) & 255], 8); }
    __device__ __forceinline__ uint32_t t2(uint32_t s) const { return rotl(c_aes.te0[(s >> 16) & 255], 16); }
    __device__ __forceinline__ uint32_t t3(uint32_t s) const { return rotl(c_aes.te0[s >> 24], 24); }
    __device__ __forceinline__ uint32_t t2r(uint32_t s) const { return c_aes.te0[(s >> 16) & 255]; }
    __device__ __forceinline__ uint32_t t3r(uint32_t s) const { return rotl(c_aes.te0[s >> 24], 8); }
    __device__ __forceinline__ uint32_t f0(uint32_t s) const { return c_aes.sbox[s & 255]; }
    __device__ __forceinline__ uint32_t f1(uint32_t s) const { return (uint32_t)c_aes.sbox[(s >> 8) & 255] << 8; }
    __device__ __forceinline__ uint32_t f2(uint32_t s) const { return (uint32_t)c_aes.sbox[(s >> 16) & 255] << 16; }
    __device__ __forceinline__ uint32_t f3(uint32_t s) const { return (uint32_t)c_aes.sbox[s >> 24] << 24; }
};

// One AES encryption, state and round keys as little-endian column words.
// Round: column c takes row r from column c+r (ShiftRows) through Te_r
// (MixColumns coefficients); the final round substitutes only.
// Rounds R0..NR on a state that already holds round R0-1's output.  With
// KROT the keys of rounds R0..NR-1 are stored rotated right by 16 (KeySlot::
// rkr) and each column costs 3 VALU besides its lookups (te_col2):
//   xor3(T0(a), T1(b), rotl16(xor3(T0(c), T1(d), rotr16(k))))
// instead of xor3(xor3(T0(a), T1(b), rotl16 T0(c)), rotl16 T1(d), k).  A
// four-table lookup object (TE::kFourTables) takes plain keys and 2 VALU a
// column (te_col4); KROT then only selects the one-round-trip schedule.
template <int NR, int R0, bool KROT = false, class TE>
__device__ __forceinline__ u32x4 aes_rounds(u32x4 st, const uint32_t *rk, const TE &T)
{
    uint32_t s0 = st.x, s1 = st.y, s2 = st.z, s3 = st.w;
#pragma unroll
    for (int r = R0; r < NR; ++r) {
        const uint32_t *k = rk + 4 * r;
        uint32_t t0, t1, t2, t3;
        if constexpr (KROT) {
            // all 16 lookups of the round in flight before the first use: one
            // LDS round trip per round (the scheduler otherwise interleaves
            // waits after every few reads to save registers)
            if constexpr (TE::kFourTables) {
                // plain keys, every row from its own table: no rotate
                const uint32_t a0 = T.t0(s0), a1 = T.t1(s1), a2 = T.t2(s2), a3 = T.t3(s3);
                const uint32_t b0 = T.t0(s1), b1 = T.t1(s2), b2 = T.t2(s3), b3 = T.t3(s0);
                const uint32_t c0 = T.t0(s2), c1 = T.t1(s3), c2 = T.t2(s0), c3 = T.t3(s1);
                const uint32_t d0 = T.t0(s3), d1 = T.t1(s0), d2 = T.t2(s1), d3 = T.t3(s2);
                __builtin_amdgcn_sched_barrier(0);
                t0 = te_col4(a0, a1, a2, a3, k[0]);
                t1 = te_col4(b0, b1, b2, b3, k[1]);
                t2 = te_col4(c0, c1, c2, c3, k[2]);
                t3 = te_col4(d0, d1, d2, d3, k[3]);
            } else {
                const uint32_t a0 = T.t0(s0), a1 = T.t1(s1), a2 = T.t2r(s2), a3 = T.t3r(s3);
                const uint32_t b0 = T.t0(s1), b1 = T.t1(s2), b2 = T.t2r(s3), b3 = T.t3r(s0);
                const uint32_t c0 = T.t0(s2), c1 = T.t1(s3), c2 = T.t2r(s0), c3 = T.t3r(s1);
                const uint32_t d0 = T.t0(s3), d1 = T.t1(s0), d2 = T.t2r(s1), d3 = T.t3r(s2);
                __builtin_amdgcn_sched_barrier(0);
                t0 = te_col2(a0, a1, a2, a3, k[0]);
                t1 = te_col2(b0, b1, b2, b3, k[1]);
                t2 = te_col2(c0, c1, c2, c3, k[2]);
                t3 = te_col2(d0, d1, d2, d3, k[3]);
            }
        } else {
            t0 = xor3(xor3(T.t0(s0), T.t1(s1), T.t2(s2)), T.t3(s3), k[0]);
            t1 = xor3(xor3(T.t0(s1), T.t1(s2), T.t2(s3)), T.t3(s0), k[1]);
            t2 = xor3(xor3(T.t0(s2), T.t1(s3), T.t2(s0)), T.t3(s1), k[2]);
            t3 = xor3(xor3(T.t0(s3), T.t1(s0), T.t2(s1)), T.t3(s2), k[3]);
        }
        s0 = t0; s1 = t1; s2 = t2; s3 = t3;
    }
    const uint32_t *k = rk + 4 * NR;
    if constexpr (KROT) {
        const uint32_t a0 = T.fr0(s0), a1 = T.fr1(s1), a2 = T.fr2(s2), a3 = T.fr3(s3);
        const uint32_t b0 = T.fr0(s1), b1 = T.fr1(s2), b2 = T.fr2(s3), b3 = T.fr3(s0);
        const uint32_t c0 = T.fr0(s2), c1 = T.fr1(s3), c2 = T.fr2(s0), c3 = T.fr3(s1);
        const uint32_t d0 = T.fr0(s3), d1 = T.fr1(s0), d2 = T.fr2(s1), d3 = T.fr3(s2);
        __builtin_amdgcn_sched_barrier(0);
        return u32x4{fin_col(a0, a1, a2, a3, k[0]), fin_col(b0, b1, b2, b3, k[1]), fin_col(c0, c1, c2, c3, k[2]),
                     fin_col(d0, d1, d2, d3, k[3])};
    }
    return u32x4{(T.f0(s0) | T.f1(s1) | T.f2(s2) | T.f3(s3)) ^ k[0],
                 (T.f0(s1) | T.f1(s2) | T.f2(s3) | T.f3(s0)) ^ k[1],
                 (T.f0(s2) | T.f1(s3) | T.f2(s0) | T.f3(s1)) ^ k[2],
                 (T.f0(s3) | T.f1(s0) | T.f2(s1) | T.f3(s2)) ^ k[3]};
}

template <int NR, class TE>
__device__ __forceinline__ u32x4 aes_encrypt(u32x4 in, const uint32_t *rk, const TE &T)
{
    return aes_rounds<NR, 1>(u32x4{in.x ^ rk[0], in.y ^ rk[1], in.z ^ rk[2], in.w ^ rk[3]}, rk, T);
}

// One AES block held by every lane of a quad, computed by the quad jointly
// (HeaderProtection_mask of a packet, _crypto.c:278-287): lane j keeps state
// column j and takes the other three columns of each round from its quad
// neighbours by DPP, so a round costs 4 table lookups per lane instead of 16
// -- a quarter of the LDS instructions of four private copies.  rk: round
// keys in memory, column j read by lane j.  Every lane of the quad must be
// active.  Returns the block in every lane.
template <int NR, class TE>
__device__ __forceinline__ u32x4 aes_encrypt_quad(u32x4 in, const uint32_t *rk, const TE &T, int sub)
{
    constexpr int kNext1 = 0x39, kNext2 = 0x4E, kNext3 = 0x93;  // lane j <- lane j+1 / j+2 / j+3
    uint32_t k[NR + 1];
#pragma unroll
    for (int r = 0; r <= NR; ++r) k[r] = rk[4 * r + sub];
    uint32_t s = (sub == 0 ? in.x : sub == 1 ? in.y : sub == 2 ? in.z : in.w) ^ k[0];
#pragma unroll
    for (int r = 1; r < NR; ++r) {
        const uint32_t s1 = quad_perm<kNext1>(s), s2 = quad_perm<kNext2>(s), s3 = quad_perm<kNext3>(s);
        s = xor3(xor3(T.t0(s), T.t1(s1), T.t2(s2)), T.t3(s3), k[r]);
    }
    const uint32_t s1 = quad_perm<kNext1>(s), s2 = quad_perm<kNext2>(s), s3 = quad_perm<kNext3>(s);
    s = (T.f0(s) | T.f1(s1) | T.f2(s2) | T.f3(s3)) ^ k[NR];
    return u32x4{quad_perm<0x00>(s), quad_perm<0x55>(s), quad_perm<0xAA>(s), quad_perm<0xFF>(s)};
}

// Counter-mode caching.  Within a packet the GCM counter block is
// nonce || BE32(cb) with cb < 256 (at most 95 blocks + J0), so only byte 15
// changes: in round 1 it reaches one output word through one lookup, in
// round 2 that word reaches each output word through one lookup.  The other
// 12 + 12 lookups are per-packet constants (c0, d0..d3): a block costs
// 1 + 4 + 16 (NR - 2) lookups instead of 16 NR.
struct CtrCache {
    uint32_t c0, d0, d1, d2, d3;
};

template <class TE>
__device__ __forceinline__ CtrCache ctr_cache(u32x4 nonce, const uint32_t *rk, const TE &T)
{
    const uint32_t s0 = nonce.x ^ rk[0], s1 = nonce.y ^ rk[1], s2 = nonce.z ^ rk[2], s3 = rk[3];
    // round 1: word 0 lacks its T3(s3) term (byte 15); words 1..3 are complete
    const uint32_t c0 = xor3(T.t0(s0), T.t1(s1), T.t2(s2)) ^ rk[4];
    const uint32_t u1 = xor3(xor3(T.t0(s1), T.t1(s2), T.t2(s3)), T.t3(s0), rk[5]);
    const uint32_t u2 = xor3(xor3(T.t0(s2), T.t1(s3), T.t2(s0)), T.t3(s1), rk[6]);
    const uint32_t u3 = xor3(xor3(T.t0(s3), T.t1(s0), T.t2(s1)), T.t3(s2), rk[7]);
    // round 2: every word lacks the one term that reads round-1 word 0
    return CtrCache{c0, xor3(T.t1(u1), T.t2(u2), T.t3(u3)) ^ rk[8],
                    xor3(T.t0(u1), T.t1(u2), T.t2(u3)) ^ rk[9],
                    xor3(T.t0(u2), T.t1(u3), T.t3(u1)) ^ rk[10],
                    xor3(T.t0(u3), T.t2(u1), T.t3(u2)) ^ rk[11]};
}

// E_K(nonce || BE32(cb)), 1 <= cb < 256, from the packet's cache.  rk holds
// plain keys for rounds 0..2 and NR and rotated ones (rkr) for 3..NR-1
// (plain ones throughout for a four-table lookup object).
template <int NR, class TE>
__device__ __forceinline__ u32x4 aes_ctr(const CtrCache &c, uint32_t cb, const uint32_t *rk,
                                         const TE &T)
{
    const uint32_t u0 = c.c0 ^ T.t3(rk[3] ^ (cb << 24));
    const u32x4 v = {c.d0 ^ T.t0(u0), c.d1 ^ T.t3(u0), c.d2 ^ T.t2(u0), c.d3 ^ T.t1(u0)};
    return aes_rounds<NR, 3, true>(v, rk, T);
}

// Two counter blocks of one packet (cb0, cb1) as one chain of LDS phases:
// every phase issues both blocks' lookups (32 for a full round) before the
// first use, so a block pays half the LDS round trips of aes_ctr.
template <int NR, class TE>
__device__ __forceinline__ void aes_ctr2(const CtrCache &c, uint32_t cb0, uint32_t cb1,
                                         const uint32_t *rk, const TE &T, u32x4 &o0, u32x4 &o1)
{
    const uint32_t x0 = T.t3(rk[3] ^ (cb0 << 24)), x1 = T.t3(rk[3] ^ (cb1 << 24));
    __builtin_amdgcn_sched_barrier(0);
    const uint32_t u0 = c.c0 ^ x0, u1 = c.c0 ^ x1;
    const uint32_t v0 = T.t0(u0), v1 = T.t3(u0), v2 = T.t2(u0), v3 = T.t1(u0);
    const uint32_t w0 = T.t0(u1), w1 = T.t3(u1), w2 = T.t2(u1), w3 = T.t1(u1);
    __builtin_amdgcn_sched_barrier(0);
    uint32_t s[2][4] = {{c.d0 ^ v0, c.d1 ^ v1, c.d2 ^ v2, c.d3 ^ v3},
                        {c.d0 ^ w0, c.d1 ^ w1, c.d2 ^ w2, c.d3 ^ w3}};
#pragma unroll
    for (int r = 3; r < NR; ++r) {
        const uint32_t *k = rk + 4 * r;
        uint32_t e[2][16];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
#pragma unroll
            for (int col = 0; col < 4; ++col) {
                e[b][4 * col + 0] = T.t0(s[b][col]);
                e[b][4 * col + 1] = T.t1(s[b][(col + 1) & 3]);
                if constexpr (TE::kFourTables) {
                    e[b][4 * col + 2] = T.t2(s[b][(col + 2) & 3]);
                    e[b][4 * col + 3] = T.t3(s[b][(col + 3) & 3]);
                } else {
                    e[b][4 * col + 2] = T.t2r(s[b][(col + 2) & 3]);
                    e[b][4 * col + 3] = T.t3r(s[b][(col + 3) & 3]);
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int b = 0; b < 2; ++b) {
#pragma unroll
            for (int col = 0; col < 4; ++col) {
                if constexpr (TE::kFourTables)
                    s[b][col] = te_col4(e[b][4 * col], e[b][4 * col + 1], e[b][4 * col + 2], e[b][4 * col + 3], k[col]);
                else
                    s[b][col] = te_col2(e[b][4 * col], e[b][4 * col + 1], e[b][4 * col + 2], e[b][4 * col + 3], k[col]);
            }
        }
    }
    const uint32_t *k = rk + 4 * NR;
    uint32_t f[2][16];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
#pragma unroll
        for (int col = 0; col < 4; ++col) {
            f[b][4 * col + 0] = T.fr0(s[b][col]);
            f[b][4 * col + 1] = T.fr1(s[b][(col + 1) & 3]);
            f[b][4 * col + 2] = T.fr2(s[b][(col + 2) & 3]);
            f[b][4 * col + 3] = T.fr3(s[b][(col + 3) & 3]);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    uint32_t o[2][4];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
#pragma unroll
        for (int col = 0; col < 4; ++col)
            o[b][col] = fin_col(f[b][4 * col], f[b][4 * col + 1], f[b][4 * col + 2], f[b][4 * col + 3], k[col]);
    }
    o0 = u32x4{o[0][0], o[0][1], o[0][2], o[0][3]};
    o1 = u32x4{o[1][0], o[1][1], o[1][2], o[1][3]};
}

// --------------------------------------------------------------- GHASH ----

// x * H^p using the 32 windowed tables of power p at LDS byte offset `tab`.
// Entry address = tab + w*256 + v*16: a word's 8 window rows fold into the
// ds_read immediate; (word & 0xF0F0F0F0) already holds high-nibble*16 per byte.
// `tab` may differ by lane (the GCM close: lane j of a quad multiplies by
// H^(4-j), one code path for the four tables).  One input word (8 reads, 32
// VGPRs in flight) at a time, as ghash_mul_global and for its reason.
__device__ __forceinline__ u32x4 ghash_mul(u32x4 x, const uint8_t *lds, uint32_t tab)
{
    u32x4 acc = {0, 0, 0, 0};
    uint32_t xw[4] = {x.x, x.y, x.z, x.w};
#pragma unroll 1
    for (int d = 0; d < 4; ++d) {
        const uint32_t w = d == 0 ? xw[0] : d == 1 ? xw[1] : d == 2 ? xw[2] : xw[3];
        uint32_t hi = w & 0xF0F0F0F0u;
        uint32_t lo = (w << 4) & 0xF0F0F0F0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int wlo = 2 * (4 * d + b), whi = wlo + 1;
            // byte b of the pre-masked nibble words, zero-extended: one v_perm
            // each (ubfe gets rewritten into shift + mask, two ops)
            const uint32_t sel = 0x0c0c0c00u | (uint32_t)b;
            uint32_t alo = __builtin_amdgcn_perm(0u, lo, sel);
            uint32_t ahi = __builtin_amdgcn_perm(0u, hi, sel);
            u32x4 e0 = *(const u32x4 *)(lds + tab + wlo * 256 + alo);
            u32x4 e1 = *(const u32x4 *)(lds + tab + whi * 256 + ahi);
            acc = xor3(acc, e0, e1);
        }
    }
    return acc;
}

// x * H^4 from a 5-bit-window table (kGh5Bytes) at LDS `base` + tsel, in
// groups of windows.  A window's entry offset e * 8 + tsel is one v_bfe and
// one v_lshl_or; the window's row offset rides in the ds_read immediate.
// One group of windows [W0, W1): its reads (issue) and their sum (consume).
template <int W0, int W1>
struct Gh5Grp {
    u32x2 lo[W1 - W0], hi[W1 - W0];
    __device__ __forceinline__ void issue(const uint32_t (&xw)[4], const uint8_t *base, uint32_t tsel)
    {
#pragma unroll
        for (int i = 0; i < W1 - W0; ++i) {
            const int w = W0 + i, sb = 5 * w, d = sb >> 5, off = sb & 31;
            // e = the window's 5 bits: one v_bfe (the compiler's own choice,
            // shift + mask + or with tsel, is one VALU more per window)
            uint32_t e;
            if (off <= 27) asm("v_bfe_u32 %0, %1, %2, 5" : "=v"(e) : "v"(xw[d]), "i"(off));
            else if (d < 3) e = __builtin_amdgcn_alignbit(xw[d + 1], xw[d], off) & 31u;
            else e = xw[3] >> off;  // bits past 127 are zero
            const uint32_t a = (e << 3) | tsel;  // tsel: a multiple of 1 KiB
            lo[i] = *(const u32x2 *)(base + w * 256 + a);
            hi[i] = *(const u32x2 *)(base + kGh5Hi + w * 256 + a);
        }
    }
    // acc ^= the group's entries, pairwise: one xor3 per dword and pair
    __device__ __forceinline__ void consume(u32x4 &acc) const
    {
        constexpr int n = W1 - W0;
        static_assert(n % 2 == 0, "an odd window would cost four plain xors (kGh5Cut)");
#pragma unroll
        for (int i = 0; i < n; i += 2) {
            acc.x = xor3(acc.x, lo[i].x, lo[i + 1].x);
            acc.y = xor3(acc.y, lo[i].y, lo[i + 1].y);
            acc.z = xor3(acc.z, hi[i].x, hi[i + 1].x);
            acc.w = xor3(acc.w, hi[i].y, hi[i + 1].y);
        }
    }
};

// Six groups (kGh5Cut, qpp_gh5.h: an even number of windows each, so the sum
// is 13 xor3 per dword and nothing else) software-pipelined: group g + 1's
// reads are in flight while group g is summed, so a multiply pays about one
// LDS round trip instead of one per group; at most two groups' reads
// (24 + 16 = 40 VGPRs) are held.  The sum starts from `init`, which costs
// nothing: the result is init ^ x * H^4.  Grp: the group type (Gh5Grp,
// Gh5GrpC), `in`: what its issue() takes.
template <template <int, int> class Grp, class... In>
__device__ __forceinline__ u32x4 gh5_pipeline(u32x4 init, const In &...in)
{
    u32x4 acc = init;
#define QPP_SB() __builtin_amdgcn_sched_barrier(0)
    {
        Grp<kGh5Cut[0], kGh5Cut[1]> a;
        Grp<kGh5Cut[1], kGh5Cut[2]> b;
        Grp<kGh5Cut[2], kGh5Cut[3]> c;
        Grp<kGh5Cut[3], kGh5Cut[4]> d;
        Grp<kGh5Cut[4], kGh5Cut[5]> e;
        Grp<kGh5Cut[5], kGh5Cut[6]> f;
        a.issue(in...);
        b.issue(in...);
        QPP_SB();
        a.consume(acc);
        QPP_SB();
        c.issue(in...);
        QPP_SB();
        b.consume(acc);
        QPP_SB();
        d.issue(in...);
        QPP_SB();
        c.consume(acc);
        QPP_SB();
        e.issue(in...);
        QPP_SB();
        d.consume(acc);
        QPP_SB();
        f.issue(in...);
        QPP_SB();
        e.consume(acc);
        QPP_SB();
        f.consume(acc);
        QPP_SB();
    }
#undef QPP_SB
    return acc;
}
// init ^ x * H^4
__device__ __forceinline__ u32x4 ghash_mul_lds5(u32x4 x, const uint8_t *base, uint32_t tsel, u32x4 init = {0, 0, 0, 0})
{
    const uint32_t xw[4] = {x.x, x.y, x.z, x.w};
    return gh5_pipeline<Gh5Grp>(init, xw, base, tsel);
}

// x * H^4 with the workgroup's LDS table entry at tsel
__device__ __forceinline__ u32x4 ghash_mul_h4(u32x4 x, const uint8_t *base, uint32_t tsel)
{
    return ghash_mul_lds5(x, base, tsel);
}
// init ^ (a ^ b) * H^4: the step loop's form (this table's addresses take the
// windows of a ^ b itself, so that one xor stays)
__device__ __forceinline__ u32x4 ghash_mul_h4(u32x4 a, u32x4 b, const uint8_t *base, uint32_t tsel, u32x4 init)
{
    return ghash_mul_lds5(a ^ b, base, tsel, init);
}

// The same multiply where the table sits at a compile-time LDS address (the
// close-from-LDS form of k_gcm: one entry per workgroup, at `base`), so that
// nothing of the table's place is left in a window's address: it is only
// e * 8, one VALU for most windows (gh5_addr, qpp_gh5.h), 39 per multiply
// against 55.
template <int W0, int W1>
struct Gh5GrpC : Gh5Grp<W0, W1> {
    template <int i = 0>
    __device__ __forceinline__ void issue(const Gh5In &in, const uint8_t *base)
    {
        if constexpr (i < W1 - W0) {
            constexpr int w = W0 + i;
            const uint32_t a = gh5_addr<w>(in);
            this->lo[i] = *(const u32x2 *)(base + w * 256 + a);
            this->hi[i] = *(const u32x2 *)(base + kGh5Hi + w * 256 + a);
            issue<i + 1>(in, base);
        }
    }
};
__device__ __forceinline__ u32x4 ghash_mul_lds5c(u32x4 x, const uint8_t *base)
{
    const Gh5In in(x.x, x.y, x.z, x.w);
    return gh5_pipeline<Gh5GrpC>(u32x4{0, 0, 0, 0}, in, base);
}
// init ^ (a ^ b) * H^4: a ^ b is formed only inside the parity masks (Gh5In)
__device__ __forceinline__ u32x4 ghash_mul_lds5c(u32x4 a, u32x4 b, const uint8_t *base, u32x4 init)
{
    const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
    const Gh5In in(aw, bw);
    return gh5_pipeline<Gh5GrpC>(init, in, base);
}

// x * H^p from the slot's tables in global memory (tab = that power's 8 KiB):
// the few multiplies per packet outside the step loop (associated-data fold,
// the last step's H^(4-j)).  32 independent 16-byte loads, L1/L2 hits.
__device__ __forceinline__ u32x4 ghash_mul_global(u32x4 x, const uint8_t *tab)
{
    u32x4 acc = {0, 0, 0, 0};
    uint32_t xw[4] = {x.x, x.y, x.z, x.w};
    // one input word (8 loads, 32 VGPRs in flight) at a time: all 32 loads at
    // once would hold 128 VGPRs and spill in the 128-VGPR kernels
#pragma unroll 1
    for (int d = 0; d < 4; ++d) {
        const uint32_t w = d == 0 ? xw[0] : d == 1 ? xw[1] : d == 2 ? xw[2] : xw[3];
        uint32_t hi = w & 0xF0F0F0F0u;
        uint32_t lo = (w << 4) & 0xF0F0F0F0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int wlo = 2 * (4 * d + b), whi = wlo + 1;
            const uint32_t sel = 0x0c0c0c00u | (uint32_t)b;
            const uint32_t alo = __builtin_amdgcn_perm(0u, lo, sel);
            const uint32_t ahi = __builtin_amdgcn_perm(0u, hi, sel);
            u32x4 e0 = *(const u32x4 *)(tab + wlo * 256 + alo);
            u32x4 e1 = *(const u32x4 *)(tab + whi * 256 + ahi);
            acc = xor3(acc, e0, e1);
        }
    }
    return acc;
}

// Bit-serial GF(2^128) multiply (SP 800-38D Algorithm 1) on little-endian
// word views; key setup only.
__device__ inline u32x4 gf128_mul_slow(u32x4 x, u32x4 y)
{
    uint64_t xh = (uint64_t)bswap(x.x) << 32 | bswap(x.y), xl = (uint64_t)bswap(x.z) << 32 | bswap(x.w);
    uint64_t vh = (uint64_t)bswap(y.x) << 32 | bswap(y.y), vl = (uint64_t)bswap(y.z) << 32 | bswap(y.w);
    uint64_t zh = 0, zl = 0;
    for (int i = 0; i < 128; ++i) {
        uint64_t bit = i < 64 ? (xh >> (63 - i)) & 1 : (xl >> (127 - i)) & 1;
        if (bit) { zh ^= vh; zl ^= vl; }
        uint64_t lsb = vl & 1;
        vl = (vl >> 1) | (vh << 63);
        vh >>= 1;
        if (lsb) vh ^= 0xe100000000000000ull;
    }
    return u32x4{bswap((uint32_t)(zh >> 32)), bswap((uint32_t)zh), bswap((uint32_t)(zl >> 32)),
                 bswap((uint32_t)zl)};
}

}  // namespace qpp
