// qpp_next.h -- the next key phase of one traffic secret (quic_pp.h:
// qpp_keytab_derive_next), shared by k_derive_next and a plain g++ build
// (tests/next_host.cc): no HIP type appears here, and qpp_hkdf.h's qualifier
// vanishes outside hipcc.
//
// A key update (RFC 9001 sec. 6, quic/crypto.py:148-168) replaces the traffic
// secret, the AEAD key and the IV, and keeps the header-protection key:
//   secret' = HKDF-Expand-Label(secret, "quic ku", "", hl)     "quic ku" for v2 as well
//   key     = HKDF-Expand-Label(secret', "quic key" | "quicv2 key", "", klen)
//   iv      = HKDF-Expand-Label(secret', "quic iv"  | "quicv2 iv",  "", 12)
//   hp      = the record's, copied
// with hl = 48 for AES-256-GCM (SHA-384) and 32 otherwise (SHA-256), klen = 16
// for AES-128-GCM and 32 otherwise.  lane() is what one lane computes;
// check() is the host's test of a record before anything is launched.
#pragma once

#include <stdint.h>

#include "qpp_hkdf.h"

namespace qpp_next {

constexpr uint32_t kSlotNone = 0xffffffffu;  // QPP_SLOT_NONE: derive and return only
constexpr uint8_t kSuiteAes128 = 0;          // QPP_AES_128_GCM
constexpr uint8_t kSuiteAes256 = 1;          // QPP_AES_256_GCM
constexpr uint8_t kSuiteMax = 2;             // QPP_CHACHA20_POLY1305
constexpr uint8_t kV2 = 1;                   // QPP_DERIVE_V2
constexpr int kSecretMax = 64;

struct Rec {  // qpp_next_phase
    uint32_t slot;
    uint8_t suite, key_phase, flags, secret_len;
    uint8_t secret[64];
    uint8_t hp[32];
};
static_assert(sizeof(Rec) == 104, "ABI record");

struct KeyMaterial {  // qpp_key_material
    uint32_t slot;
    uint8_t suite, key_phase, rsv[2];
    uint8_t iv[12], key[32], hp[32];
};
static_assert(sizeof(KeyMaterial) == 84, "ABI record");

QPP_HD int hash_len(uint8_t suite) { return suite == kSuiteAes256 ? 48 : 32; }
QPP_HD int key_len(uint8_t suite) { return suite == kSuiteAes128 ? 16 : 32; }

// Whether qpp_keytab_derive_next takes the record for a table of `cap` slots.
QPP_HD bool check(const Rec &r, uint32_t cap)
{
    if (r.slot >= cap && r.slot != kSlotNone) return false;
    if (r.suite > kSuiteMax) return false;
    if (r.secret_len < 1 || r.secret_len > kSecretMax) return false;
    if (r.key_phase > 1) return false;
    return (r.flags & ~kV2) == 0;
}

// One record that check() passed.  km: the whole qpp_key_material, its key
// and hp zero past klen as everywhere the library writes one; secret_out:
// secret', zero past hl.  Reads secret[0, secret_len) and hp[0, klen) only.
QPP_HD void lane(const Rec &r, KeyMaterial &km, uint8_t secret_out[kSecretMax])
{
    const bool big = r.suite == kSuiteAes256;
    const int hl = hash_len(r.suite), klen = key_len(r.suite);
    uint8_t secret[kSecretMax];
    const int len = r.secret_len;
    for (int j = 0; j < kSecretMax; ++j) secret[j] = j < len ? r.secret[j] : 0;
    qpp_hkdf::Hmac m;
    qpp_hkdf::hmac_init(m, big, secret, len);
    uint8_t next[48];
    qpp_hkdf::expand_label(m, "quic ku", 7, hl, next);
    for (int j = 0; j < kSecretMax; ++j) secret_out[j] = j < hl ? next[j] : 0;
    qpp_hkdf::hmac_init(m, big, next, hl);
    km.slot = r.slot;
    km.suite = r.suite;
    km.key_phase = r.key_phase;
    km.rsv[0] = km.rsv[1] = 0;
    for (int j = 0; j < 32; ++j) km.key[j] = 0;
    if (r.flags & kV2) {
        qpp_hkdf::expand_label(m, "quicv2 key", 10, klen, km.key);
        qpp_hkdf::expand_label(m, "quicv2 iv", 9, 12, km.iv);
    } else {
        qpp_hkdf::expand_label(m, "quic key", 8, klen, km.key);
        qpp_hkdf::expand_label(m, "quic iv", 7, 12, km.iv);
    }
    for (int j = 0; j < 32; ++j) km.hp[j] = j < klen ? r.hp[j] : 0;
}

}  // namespace qpp_next
