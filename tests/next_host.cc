// Host build of aioquic_amd/csrc/qpp_next.h for tests/test_next_host.py: what
// every lane of k_derive_next computes, and the record check
// qpp_keytab_derive_next runs before it launches anything.  Plain g++, no HIP.
//
// Built as a shared object, the functions below are called through ctypes.
// Built as a program (with -fsanitize=address,undefined), main() runs the lane
// over heap buffers of exactly the records' sizes, so that a read or write
// past a record, a key material or the 64 secret bytes is the sanitizer's to
// report.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "../aioquic_amd/csrc/qpp_next.h"

using qpp_next::KeyMaterial;
using qpp_next::Rec;

extern "C" {

void nx_lane(const Rec *r, KeyMaterial *km, uint8_t *secret_out) { qpp_next::lane(*r, *km, secret_out); }

uint32_t nx_check(const Rec *r, uint32_t cap) { return qpp_next::check(*r, cap); }

}  // extern "C"

namespace {

int failures = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("FAILED line %d: %s\n", __LINE__, #c);          \
            ++failures;                                            \
        }                                                          \
    } while (0)

void unhex(const char *s, uint8_t *out)
{
    for (size_t i = 0; s[2 * i]; ++i) {
        unsigned v = 0;
        sscanf(s + 2 * i, "%2x", &v);
        out[i] = (uint8_t)v;
    }
}

struct Run {
    KeyMaterial km;
    uint8_t secret[64];
};

// the lane over heap copies of exactly sizeof(Rec), sizeof(KeyMaterial) and 64 bytes,
// the outputs filled with 0xa5 first: every byte of them must be written
Run lane_exact(const Rec &rec)
{
    Rec *r = (Rec *)malloc(sizeof(Rec));
    KeyMaterial *km = (KeyMaterial *)malloc(sizeof(KeyMaterial));
    uint8_t *sec = (uint8_t *)malloc(64);
    if (!r || !km || !sec) abort();
    memcpy(r, &rec, sizeof rec);
    memset(km, 0xa5, sizeof *km);
    memset(sec, 0xa5, 64);
    qpp_next::lane(*r, *km, sec);
    Run out;
    memcpy(&out.km, km, sizeof *km);
    memcpy(out.secret, sec, 64);
    free(r);
    free(km);
    free(sec);
    return out;
}

bool all_zero(const uint8_t *p, int n)
{
    for (int i = 0; i < n; ++i)
        if (p[i]) return false;
    return true;
}

}  // namespace

int main()
{
    // RFC 9001 A.5: the ChaCha20-Poly1305 secret and its "quic ku" output
    uint8_t a5[32], ku[32];
    unhex("9ac312a7f877468ebe69422748ad00a15443f18203a07d6060f688f30f21632b", a5);
    unhex("1223504755036d556342ee9361d253421a826c9ecdf3c7148684b36b714881f9", ku);
    for (uint8_t suite = 0; suite < 3; ++suite)
        for (uint8_t v2 = 0; v2 < 2; ++v2)
            for (int len : {1, 32, 48, 64})
                for (uint8_t fill : {(uint8_t)0x00, (uint8_t)0xff}) {
                    Rec r;
                    memset(&r, 0, sizeof r);
                    r.slot = suite == 1 ? qpp_next::kSlotNone : 7u + suite;
                    r.suite = suite;
                    r.key_phase = (uint8_t)(len & 1) ^ v2;
                    r.flags = v2;
                    r.secret_len = (uint8_t)len;
                    for (int j = 0; j < 64; ++j) r.secret[j] = (uint8_t)(j < 32 && len == 32 ? a5[j] : 0x11 * suite + 3 * j + len);
                    memset(r.hp, fill, 32);
                    CHECK(qpp_next::check(r, 16));
                    const Run a = lane_exact(r);
                    const int hl = qpp_next::hash_len(suite), kl = qpp_next::key_len(suite);
                    CHECK(a.km.slot == r.slot && a.km.suite == suite && a.km.key_phase == r.key_phase);
                    CHECK(a.km.rsv[0] == 0 && a.km.rsv[1] == 0);
                    CHECK(all_zero(a.km.key + kl, 32 - kl) && all_zero(a.km.hp + kl, 32 - kl));
                    CHECK(!all_zero(a.km.key, kl) && !all_zero(a.km.iv, 12));
                    for (int j = 0; j < kl; ++j) CHECK(a.km.hp[j] == fill);
                    CHECK(all_zero(a.secret + hl, 64 - hl) && !all_zero(a.secret, hl));
                    if (len == 32 && suite != 1) CHECK(memcmp(a.secret, ku, 32) == 0);
                    // bytes past secret_len and the hp bytes past the key length are not looked at
                    Rec q = r;
                    for (int j = len; j < 64; ++j) q.secret[j] ^= 0x5a;
                    for (int j = kl; j < 32; ++j) q.hp[j] ^= 0x5a;
                    const Run b = lane_exact(q);
                    CHECK(memcmp(&a, &b, sizeof a) == 0);
                    // the version changes key and iv, never the secret
                    q = r;
                    q.flags ^= 1;
                    const Run c = lane_exact(q);
                    CHECK(memcmp(a.secret, c.secret, 64) == 0);
                    CHECK(memcmp(a.km.key, c.km.key, 32) != 0 && memcmp(a.km.iv, c.km.iv, 12) != 0);
                }
    // the record check, each refusal alone
    {
        Rec g;
        memset(&g, 0, sizeof g);
        g.slot = 3;
        g.suite = 2;
        g.key_phase = 1;
        g.flags = 1;
        g.secret_len = 64;
        CHECK(qpp_next::check(g, 4));
        Rec b = g;
        b.slot = 4;
        CHECK(!qpp_next::check(b, 4));
        b.slot = qpp_next::kSlotNone - 1;
        CHECK(!qpp_next::check(b, 4));
        b.slot = qpp_next::kSlotNone;
        CHECK(qpp_next::check(b, 4));
        b = g, b.suite = 3;
        CHECK(!qpp_next::check(b, 4));
        b = g, b.secret_len = 0;
        CHECK(!qpp_next::check(b, 4));
        b = g, b.secret_len = 65;
        CHECK(!qpp_next::check(b, 4));
        b = g, b.secret_len = 1;
        CHECK(qpp_next::check(b, 4));
        b = g, b.key_phase = 2;
        CHECK(!qpp_next::check(b, 4));
        b = g, b.flags = 2;
        CHECK(!qpp_next::check(b, 4));
        b = g, b.flags = 0x81;
        CHECK(!qpp_next::check(b, 4));
    }
    if (failures) return 1;
    printf("next_host: ok\n");
    return 0;
}
