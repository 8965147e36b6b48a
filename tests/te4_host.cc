// Host check of aioquic_amd/csrc/qpp_te4.h (tests/test_te4_host.py): the
// four-table AES image of the close-from-LDS form of k_gcm as load_te4 fills
// it (te_image_word), the lookup addresses of LdsTe4 (one byte permute: bit 16
// of the per-lane constant selects the high half for rows 2 and 3), and the
// two column combines -- te_col2 on the low half with the round key rotated
// right by 16 against te_col4 on both halves with the plain key.  Then whole
// AES-128 and AES-256 blocks through the four-table path against the C
// oracle's qo_aes_block.
// A program of its own, so that it also runs under the host sanitizers.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../aioquic_amd/csrc/qpp_te4.h"
#include "../oracle/qpp_oracle.h"

using namespace qpp;

static int g_fail = 0;
#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            if (g_fail++ < 10) printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
        }                                                              \
    } while (0)

// splitmix64
static uint64_t g_seed = 0x7e4a11ce5ull;
static uint64_t rnd64()
{
    uint64_t z = (g_seed += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static uint32_t rnd32() { return (uint32_t)rnd64(); }

// The image: 128 KiB as 32-bit words, filled as load_te4 fills it (16-byte
// part `part` of row x in each half holds four copies of te_image_word).
static std::vector<uint32_t> make_image()
{
    std::vector<uint32_t> im(2 * kTeBytes / 4);
    for (int i = 0; i < 256 * 16; ++i) {
        const int x = i >> 4, part = i & 15;
        for (int half = 0; half < 2; ++half)
            for (int c = 0; c < 4; ++c)
                im[(half * kTeBytes + x * 256 + part * 16) / 4 + c] = te_image_word(kAesTables.te0[x], half, part);
    }
    return im;
}

// v_perm_b32 D = perm({S0, S1}, sel): selector 0-3 byte of S1, 4-7 byte of S0, 0x0c zero
static uint32_t perm(uint32_t s0, uint32_t s1, uint32_t sel)
{
    uint32_t r = 0;
    for (int b = 0; b < 4; ++b) {
        const uint32_t k = (sel >> (8 * b)) & 0xff;
        uint32_t v = 0;
        if (k < 4) v = (s1 >> (8 * k)) & 0xff;
        else if (k < 8) v = (s0 >> (8 * (k - 4))) & 0xff;
        else CHECK(k == 0x0c);
        r |= v << (8 * b);
    }
    return r;
}

// The lookup objects of qpp_device.h, restated on the host image: `lo` is
// the per-lane constant, R the state byte
struct Te2 {  // LdsTe: the low half only
    const std::vector<uint32_t> &im;
    uint32_t lo;
    uint32_t at(uint32_t byte_addr) const
    {
        CHECK(byte_addr % 4 == 0 && byte_addr < (uint32_t)kTeBytes);
        return im[byte_addr / 4];
    }
    uint32_t addr(int R, uint32_t s) const { return perm(s, lo, 0x0c0c0000u | ((4u + R) << 8)); }
    uint32_t t0(uint32_t s) const { return at(addr(0, s)); }
    uint32_t t1(uint32_t s) const { return at(128 + addr(1, s)); }
    uint32_t t2r(uint32_t s) const { return at(addr(2, s)); }
    uint32_t t3r(uint32_t s) const { return at(128 + addr(3, s)); }
};
struct Te4 {  // LdsTe4
    const std::vector<uint32_t> &im;
    uint32_t lo;
    uint32_t at(uint32_t byte_addr) const
    {
        CHECK(byte_addr % 4 == 0 && byte_addr < 2u * kTeBytes);
        return im[byte_addr / 4];
    }
    uint32_t addr(int R, bool hi, uint32_t s) const
    {
        return perm(s, lo, (hi ? 0x0c020000u : 0x0c0c0000u) | ((4u + R) << 8));
    }
    uint32_t t0(uint32_t s) const { return at(addr(0, false, s)); }
    uint32_t t1(uint32_t s) const { return at(128 + addr(1, false, s)); }
    uint32_t t2(uint32_t s) const { return at(addr(2, true, s)); }
    uint32_t t3(uint32_t s) const { return at(128 + addr(3, true, s)); }
    uint32_t fr0(uint32_t s) const { return at(addr(0, false, s)); }
    uint32_t fr1(uint32_t s) const { return at(addr(1, false, s)); }
    uint32_t fr2(uint32_t s) const { return at(128 + addr(2, false, s)); }
    uint32_t fr3(uint32_t s) const { return at(128 + addr(3, false, s)); }
};
// fin_col of qpp_device.h: S(x) is byte 1 of fr0 / fr1, byte 2 of fr2, byte 3 of fr3
static uint32_t fin_col(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, uint32_t k)
{
    const uint32_t lo = perm(r1, r0, 0x0c0c0501u), hi = perm(r3, r2, 0x07020c0cu);
    return (lo | hi) ^ k;
}

static uint32_t rotr16(uint32_t x) { return (x >> 16) | (x << 16); }
static uint32_t bswap(uint32_t x) { return __builtin_bswap32(x); }

// One AES block through the four-table path: rk = 4 (nr + 1) little-endian
// column words (KeySlot::rk), state words as the kernels hold them
static void aes_te4(const Te4 &T, const uint32_t *rk, int nr, const uint32_t in[4], uint32_t out[4])
{
    uint32_t s[4] = {in[0] ^ rk[0], in[1] ^ rk[1], in[2] ^ rk[2], in[3] ^ rk[3]};
    for (int r = 1; r < nr; ++r) {
        uint32_t t[4];
        for (int c = 0; c < 4; ++c)
            t[c] = te_col4(T.t0(s[c]), T.t1(s[(c + 1) & 3]), T.t2(s[(c + 2) & 3]), T.t3(s[(c + 3) & 3]), rk[4 * r + c]);
        memcpy(s, t, sizeof s);
    }
    for (int c = 0; c < 4; ++c)
        out[c] = fin_col(T.fr0(s[c]), T.fr1(s[(c + 1) & 3]), T.fr2(s[(c + 2) & 3]), T.fr3(s[(c + 3) & 3]), rk[4 * nr + c]);
}

int main()
{
    const std::vector<uint32_t> im = make_image();

    // 1. the image: the low half is row x = [Te0[x] x 32 | Te1[x] x 32], the
    //    high half the same rows rotated left by 16
    for (int x = 0; x < 256; ++x) {
        const uint32_t te0 = kAesTables.te0[x];
        const uint32_t s = kAesTables.sbox[x];
        CHECK(te0 == ((uint32_t)gf8_mul((uint8_t)s, 2) | s << 8 | s << 16 | (uint32_t)gf8_mul((uint8_t)s, 3) << 24));
        for (int c = 0; c < 64; ++c) {
            const uint32_t want = c < 32 ? te0 : te_rotl(te0, 8);
            CHECK(im[(x * 256) / 4 + c] == want);
            CHECK(im[(kTeBytes + x * 256) / 4 + c] == te_rotl(want, 16));
        }
    }

    // 2. every (x, row) through every lane's constant: the four-table lookups
    //    are Te_row[x], the two-table ones Te0 / Te1 on the low half
    for (uint32_t lane = 0; lane < 64; ++lane) {
        const Te2 A{im, (lane & 31) * 4};
        const Te4 B{im, (lane & 31) * 4 | 0x10000u};
        for (uint32_t x = 0; x < 256; ++x) {
            const uint32_t te0 = kAesTables.te0[x], junk = rnd32();
            uint32_t s[4];
            for (int r = 0; r < 4; ++r) s[r] = (junk & ~(0xffu << (8 * r))) | x << (8 * r);
            CHECK(B.t0(s[0]) == te0 && B.t1(s[1]) == te_rotl(te0, 8));
            CHECK(B.t2(s[2]) == te_rotl(te0, 16) && B.t3(s[3]) == te_rotl(te0, 24));
            CHECK(A.t0(s[0]) == te0 && A.t1(s[1]) == te_rotl(te0, 8));
            CHECK(A.t2r(s[2]) == te0 && A.t3r(s[3]) == te_rotl(te0, 8));
            CHECK(B.fr0(s[0]) == te0 && B.fr1(s[1]) == te0);
            CHECK(B.fr2(s[2]) == te_rotl(te0, 8) && B.fr3(s[3]) == te_rotl(te0, 8));
            // the same column from both forms, x in each row in turn
            for (int r = 0; r < 4; ++r) {
                uint32_t st[4] = {rnd32(), rnd32(), rnd32(), rnd32()};
                st[r] = s[r];
                const uint32_t k = rnd32();
                const uint32_t two = te_col2(A.t0(st[0]), A.t1(st[1]), A.t2r(st[2]), A.t3r(st[3]), rotr16(k));
                const uint32_t four = te_col4(B.t0(st[0]), B.t1(st[1]), B.t2(st[2]), B.t3(st[3]), k);
                CHECK(two == four);
            }
        }
    }

    // 3. random states and keys
    for (int it = 0; it < 20000; ++it) {
        const uint32_t lane = rnd32() & 63;
        const Te2 A{im, (lane & 31) * 4};
        const Te4 B{im, (lane & 31) * 4 | 0x10000u};
        const uint32_t st[4] = {rnd32(), rnd32(), rnd32(), rnd32()}, k = rnd32();
        CHECK(te_col2(A.t0(st[0]), A.t1(st[1]), A.t2r(st[2]), A.t3r(st[3]), rotr16(k)) ==
              te_col4(B.t0(st[0]), B.t1(st[1]), B.t2(st[2]), B.t3(st[3]), k));
    }

    // 4. whole blocks against the oracle, AES-128 and AES-256
    for (int key_len = 16; key_len <= 32; key_len += 16) {
        for (int it = 0; it < 200; ++it) {
            uint8_t key[32], in[16], want[16];
            for (int i = 0; i < 32; ++i) key[i] = (uint8_t)rnd32();
            for (int i = 0; i < 16; ++i) in[i] = (uint8_t)rnd32();
            if (it == 0) {  // all-zero key and block
                memset(key, 0, sizeof key);
                memset(in, 0, sizeof in);
            }
            uint32_t rk_be[60], rk[60];
            const int nr = qo_aes_expand(key, key_len, rk_be);
            CHECK(nr == (key_len == 16 ? 10 : 14));
            qo_aes_block(rk_be, nr, in, want);
            for (int i = 0; i < 4 * (nr + 1); ++i) rk[i] = bswap(rk_be[i]);
            const Te4 B{im, (uint32_t)(it & 31) * 4 | 0x10000u};
            uint32_t iw[4], ow[4];
            memcpy(iw, in, 16);
            aes_te4(B, rk, nr, iw, ow);
            CHECK(memcmp(ow, want, 16) == 0);
        }
    }
    // FIPS-197 appendix C.1
    {
        uint8_t key[16], in[16];
        for (int i = 0; i < 16; ++i) {
            key[i] = (uint8_t)i;
            in[i] = (uint8_t)(0x11 * i);
        }
        static const uint8_t want[16] = {0x69, 0xc4, 0xe0, 0xd8, 0x6a, 0x7b, 0x04, 0x30,
                                         0xd8, 0xcd, 0xb7, 0x80, 0x70, 0xb4, 0xc5, 0x5a};
        uint32_t rk_be[60], rk[60], iw[4], ow[4];
        const int nr = qo_aes_expand(key, 16, rk_be);
        for (int i = 0; i < 4 * (nr + 1); ++i) rk[i] = bswap(rk_be[i]);
        memcpy(iw, in, 16);
        aes_te4(Te4{im, 0x10000u}, rk, nr, iw, ow);
        CHECK(memcmp(ow, want, 16) == 0);
    }

    if (g_fail) {
        printf("te4_host: %d checks failed\n", g_fail);
        return 1;
    }
    printf("te4_host: ok\n");
    return 0;
}
