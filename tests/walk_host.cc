// Host build of aioquic_amd/csrc/qpp_walk.h for tests/test_walk_host.py: the
// header walk every lane of k_walk runs.  Plain g++, no HIP.
//
// Built as a shared object, the functions below are called through ctypes.
// Built as a program (with -fsanitize=address,undefined), main() runs the
// truncation and varint cases on heap buffers of exactly the datagram's size,
// so that a read at or past p[len] is the sanitizer's to report.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../aioquic_amd/csrc/qpp_walk.h"

using qpp_wk::Rec;

extern "C" {

// the walk of one datagram: records out[0 .. return value)
uint32_t wk_walk(const uint8_t *p, uint32_t len, uint32_t cid_len, Rec *out)
{
    return qpp_wk::walk(p, len, cid_len, [&](uint32_t k, const Rec &r) { out[k] = r; });
}

void wk_parse_one(const uint8_t *p, uint32_t len, uint32_t pos, uint32_t cid_len, Rec *out)
{
    qpp_wk::parse_one(p, len, pos, cid_len, *out);
}

uint32_t wk_keyset_of(uint32_t type, uint32_t version) { return qpp_wk::keyset_of((uint8_t)type, version); }
uint32_t wk_space_of(uint32_t type) { return qpp_wk::space_of((uint8_t)type); }

}  // extern "C"

namespace {

typedef std::vector<uint8_t> Bytes;

void put_varint(Bytes &b, uint64_t v, int form)  // form: log2 of the encoded size
{
    const int n = 1 << form;
    for (int k = n - 1; k >= 0; --k) {
        uint8_t x = (uint8_t)(v >> (8 * k));
        if (k == n - 1) x = (uint8_t)((x & 0x3f) | (form << 6));
        b.push_back(x);
    }
}

// flags(1) version(4) dcid scid [token] Length, then `body` bytes; Length as given
Bytes long_packet(uint8_t first, uint32_t version, int dcid, int scid, int token, int token_form, uint64_t length,
                  int length_form, size_t body)
{
    Bytes b;
    b.push_back(first);
    for (int k = 3; k >= 0; --k) b.push_back((uint8_t)(version >> (8 * k)));
    b.push_back((uint8_t)dcid);
    for (int k = 0; k < dcid; ++k) b.push_back((uint8_t)(0xD0 + k));
    b.push_back((uint8_t)scid);
    for (int k = 0; k < scid; ++k) b.push_back((uint8_t)(0x50 + k));
    if (token >= 0) {
        put_varint(b, (uint64_t)token, token_form);
        for (int k = 0; k < token; ++k) b.push_back((uint8_t)k);
    }
    put_varint(b, length, length_form);
    for (size_t k = 0; k < body; ++k) b.push_back((uint8_t)(0xA0 ^ k));
    return b;
}

// the walk over a heap copy of exactly `len` bytes
uint32_t walk_exact(const uint8_t *src, uint32_t len, uint32_t cid_len, Rec *out)
{
    uint8_t *p = (uint8_t *)malloc(len ? len : 1);
    if (!p) abort();
    if (len) memcpy(p, src, len);
    // with len == 0 the one allocated byte must not be read either; the
    // walk is handed a pointer past it
    const uint32_t n = wk_walk(len ? p : p + 1, len, cid_len, out);
    free(p);
    return n;
}

int failures = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("FAILED line %d: %s\n", __LINE__, #c);          \
            ++failures;                                            \
        }                                                          \
    } while (0)

}  // namespace

int main()
{
    Rec r[qpp_wk::kWalkMax];
    // Initial (8-byte token) + Handshake + 1-RTT, 1200 bytes, the 1-RTT packet the padding's bearer
    Bytes ini = long_packet(0xC1, 1, 8, 8, 8, 0, 300, 1, 300);
    Bytes hs = long_packet(0xE1, 1, 8, 8, -1, 0, 200, 1, 200);
    Bytes dg = ini;
    dg.insert(dg.end(), hs.begin(), hs.end());
    dg.push_back(0x41);
    while (dg.size() < 1200) dg.push_back((uint8_t)dg.size());
    uint32_t n = walk_exact(dg.data(), (uint32_t)dg.size(), 8, r);
    CHECK(n == 3 && r[0].status == 0 && r[1].status == 0 && r[2].status == 0);
    CHECK(r[0].type == 0 && r[0].len == ini.size() && r[0].token_len == 8 && r[0].pn_off == ini.size() - 300);
    CHECK(r[1].type == 2 && r[1].off == ini.size() && r[1].len == hs.size());
    CHECK(r[2].type == 5 && r[2].off == ini.size() + hs.size() && r[2].off + r[2].len == 1200 && r[2].pn_off == 9);
    for (uint32_t len = 0; len <= dg.size(); ++len) {
        n = walk_exact(dg.data(), len, 8, r);
        CHECK(n <= qpp_wk::kWalkMax && (len == 0) == (n == 0));
        for (uint32_t k = 0; k < n; ++k) {
            CHECK(r[k].off <= len && r[k].len <= len - r[k].off);
            CHECK(r[k].status == 0 || k == n - 1);
        }
        // a cut inside a long packet is a parse error where that packet starts
        if (len && len < ini.size()) CHECK(n == 1 && r[0].status == 1 && r[0].off == 0);
        if (len > ini.size() && len < ini.size() + hs.size()) CHECK(n == 2 && r[1].status == 1 && r[1].off == ini.size());
    }
    // token length and Length in all four varint forms, every truncation of each
    for (int tf = 0; tf < 4; ++tf)
        for (int lf = 0; lf < 4; ++lf) {
            Bytes p = long_packet(0xC0, 1, 5, 0, 33, tf, 40, lf, 40);
            n = walk_exact(p.data(), (uint32_t)p.size(), 8, r);
            CHECK(n == 1 && r[0].status == 0 && r[0].len == p.size() && r[0].token_len == 33);
            CHECK(r[0].pn_off == p.size() - 40);
            for (uint32_t len = 0; len < p.size(); ++len) {
                n = walk_exact(p.data(), len, 8, r);
                CHECK(len == 0 ? n == 0 : (n == 1 && r[0].status == 1 && r[0].len == 0));
            }
        }
    // Length = 2^62 - 1 and Length = remaining + 1, token length likewise
    {
        Bytes p = long_packet(0xE0, 1, 8, 8, -1, 0, (1ull << 62) - 1, 3, 64);
        n = walk_exact(p.data(), (uint32_t)p.size(), 8, r);
        CHECK(n == 1 && r[0].status == 1);
        p = long_packet(0xE0, 1, 8, 8, -1, 0, 65, 1, 64);
        n = walk_exact(p.data(), (uint32_t)p.size(), 8, r);
        CHECK(n == 1 && r[0].status == 1);
        p = long_packet(0xE0, 1, 8, 8, -1, 0, 64, 1, 64);
        n = walk_exact(p.data(), (uint32_t)p.size(), 8, r);
        CHECK(n == 1 && r[0].status == 0 && r[0].len == p.size());
        p = long_packet(0xC0, 1, 8, 8, 0, 0, 10, 0, 10);
        p[1 + 4 + 9 + 9] = 0xFF;  // the token length's first byte: an 8-byte form
        for (int k = 1; k < 8; ++k) p.insert(p.begin() + 23 + k, 0xFF);
        n = walk_exact(p.data(), (uint32_t)p.size(), 8, r);
        CHECK(n == 1 && r[0].status == 1);
    }
    if (failures) return 1;
    printf("walk_host: ok\n");
    return 0;
}
