// Host build of aioquic_amd/csrc/qpp_p130.h for the CPU unit test
// (tests/test_p130_host.py): the Poly1305 limb primitives on arrays of n
// inputs, limbs as uint32 x 5, and a plain Horner loop over whole blocks.
#include <stdint.h>
#include <string.h>

#include "../aioquic_amd/csrc/qpp_p130.h"

using qpp::P130;

static P130 ld(const uint32_t *p)
{
    return P130{{p[0], p[1], p[2], p[3], p[4]}};
}

static void st(uint32_t *p, const P130 &x) { memcpy(p, x.v, 20); }

static qpp::u32x4 ld16(const uint8_t *p)
{
    uint32_t w[4];
    for (int i = 0; i < 4; ++i)
        w[i] = (uint32_t)p[4 * i] | (uint32_t)p[4 * i + 1] << 8 | (uint32_t)p[4 * i + 2] << 16 |
               (uint32_t)p[4 * i + 3] << 24;
    return qpp::u32x4{w[0], w[1], w[2], w[3]};
}

extern "C" {

void qpp_test_p130_mul(const uint32_t *h, const uint32_t *r, uint32_t *out, int n)
{
    for (int i = 0; i < n; ++i) st(out + 5 * i, qpp::p130_mul(ld(h + 5 * i), ld(r + 5 * i)));
}

void qpp_test_p130_add(const uint32_t *a, const uint32_t *b, uint32_t *out, int n)
{
    for (int i = 0; i < n; ++i) st(out + 5 * i, qpp::p130_add(ld(a + 5 * i), ld(b + 5 * i)));
}

// k products h[k*i + j] * r[k*i + j] into one set of column sums (cols: the
// five 64-bit sums as the kernel holds them), then one p130_carry
void qpp_test_p130_mac_carry(const uint32_t *h, const uint32_t *r, int k, uint64_t *cols, uint32_t *out, int n)
{
    for (int i = 0; i < n; ++i) {
        uint64_t d[5] = {0, 0, 0, 0, 0};
        for (int j = 0; j < k; ++j) qpp::p130_mac(d, ld(h + 5 * (k * i + j)), ld(r + 5 * (k * i + j)));
        memcpy(cols + 5 * i, d, 40);
        st(out + 5 * i, qpp::p130_carry(d[0], d[1], d[2], d[3], d[4]));
    }
}

void qpp_test_p130_block(const uint8_t *m, uint32_t *out, int n)
{
    for (int i = 0; i < n; ++i) st(out + 5 * i, qpp::p130_block(ld16(m + 16 * i)));
}

void qpp_test_p130_r(const uint8_t *k, uint32_t *out, int n)
{
    for (int i = 0; i < n; ++i) {
        const qpp::u32x4 w = ld16(k + 16 * i);
        st(out + 5 * i, qpp::p130_r(w.x, w.y, w.z, w.w));
    }
}

// s and the tag as four little-endian words each
void qpp_test_p130_finish(const uint32_t *h, const uint32_t *s, uint32_t *tag, int n)
{
    for (int i = 0; i < n; ++i) {
        const qpp::u32x4 t = qpp::p130_finish(ld(h + 5 * i), s[4 * i], s[4 * i + 1], s[4 * i + 2], s[4 * i + 3]);
        tag[4 * i] = t.x; tag[4 * i + 1] = t.y; tag[4 * i + 2] = t.z; tag[4 * i + 3] = t.w;
    }
}

// Poly1305 of nblk whole 16-byte blocks under the 32-byte one-time key:
// h = (h + block) r per block, then p130_finish
void qpp_test_p130_horner(const uint8_t *key, const uint8_t *msg, int nblk, uint8_t *tag)
{
    const qpp::u32x4 kr = ld16(key), ks = ld16(key + 16);
    const P130 r = qpp::p130_r(kr.x, kr.y, kr.z, kr.w);
    P130 h = qpp::p130_zero();
    for (int i = 0; i < nblk; ++i) h = qpp::p130_mul(qpp::p130_add(h, qpp::p130_block(ld16(msg + 16 * i))), r);
    const qpp::u32x4 t = qpp::p130_finish(h, ks.x, ks.y, ks.z, ks.w);
    const uint32_t w[4] = {t.x, t.y, t.z, t.w};
    for (int i = 0; i < 16; ++i) tag[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
}

}  // extern "C"
