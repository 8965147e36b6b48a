// Host build of the Initial-key part of aioquic_amd/csrc/qpp_hkdf.h for the
// CPU test (tests/test_hkdf_initial.py): the function the kernel
// k_derive_initial calls per lane, and the salts' HMAC pad states both ways.
#include "../aioquic_amd/csrc/qpp_hkdf.h"

static void put_be(uint8_t *p, const uint32_t *w, int n)
{
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < 4; ++j) p[4 * i + j] = (uint8_t)(w[i] >> (24 - 8 * j));
}

// out: secret (32) | key (16) | iv (12) | hp (16).  cid must be readable for 20 bytes.
extern "C" int qpp_test_derive_initial(const uint8_t *cid, int cid_len, int v2, int server,
                                       uint8_t *out)
{
    qpp_hkdf::InitialSalts salts;
    qpp_hkdf::initial_salt_pads(salts);
    qpp_hkdf::InitialKeys k;
    qpp_hkdf::derive_initial(salts, cid, cid_len, v2 != 0, server != 0, k);
    put_be(out, k.secret, 8);
    put_be(out + 32, k.key, 4);
    put_be(out + 48, k.iv, 3);
    put_be(out + 60, k.hp, 4);
    return 0;
}

// The precomputed pad states: per version, ist[8] then ost[8].
extern "C" void qpp_test_salt_pads(uint32_t out[32])
{
    qpp_hkdf::InitialSalts salts;
    qpp_hkdf::initial_salt_pads(salts);
    for (int v = 0; v < 2; ++v)
        for (int i = 0; i < 8; ++i) {
            out[16 * v + i] = salts.v[v].ist[i];
            out[16 * v + 8 + i] = salts.v[v].ost[i];
        }
}

// The same states from hmac_init (the byte-array code k_derive runs) on a salt's bytes.
extern "C" void qpp_test_hmac_init(const uint8_t *key, int key_len, uint32_t out[16])
{
    qpp_hkdf::Hmac m;
    qpp_hkdf::hmac_init(m, false, key, key_len);
    for (int i = 0; i < 8; ++i) {
        out[i] = m.ist32[i];
        out[8 + i] = m.ost32[i];
    }
}
