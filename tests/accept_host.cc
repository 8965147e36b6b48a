// Host build of aioquic_amd/csrc/qpp_accept.h for tests/test_accept_host.py:
// the decision every lane of k_accept runs.  Plain g++, no HIP.
//
// Built as a shared object, the functions below are called through ctypes.
// Built as a program (with -fsanitize=address,undefined), main() runs the
// decision over heap buffers of exactly the datagram's size, for every
// truncation of an accepted datagram's first 6 + dcid_len bytes, so that a
// read at or past p[len] is the sanitizer's to report.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../aioquic_amd/csrc/qpp_accept.h"

using qpp_ac::Acc;
using qpp_ac::Desc;
using qpp_ac::Initial;
using qpp_wk::Rec;

extern "C" {

// the decision from a given walk count and packet 0's record
uint32_t ac_accept_rec(const uint8_t *p, uint32_t len, uint32_t i, uint64_t off, uint32_t route_conn,
                       uint32_t route_cls, uint32_t walk_n, const Rec *w0, uint32_t slot_client, uint32_t slot_server,
                       uint32_t accept_flags, uint32_t desc_flags, Initial *ini, Desc *d, Acc *acc)
{
    return qpp_ac::accept_one(i, route_conn, (uint8_t)route_cls, walk_n, *w0, off, len, p, slot_client, slot_server,
                              accept_flags, (uint16_t)desc_flags, *ini, *d, *acc);
}

// the walk of the datagram (qpp_walk.h), then the decision, as k_walk and k_accept run in a row
uint32_t ac_accept(const uint8_t *p, uint32_t len, uint32_t cid_len, uint32_t i, uint64_t off, uint32_t route_conn,
                   uint32_t route_cls, uint32_t slot_client, uint32_t slot_server, uint32_t accept_flags,
                   uint32_t desc_flags, Initial *ini, Desc *d, Acc *acc)
{
    Rec r[qpp_wk::kWalkMax];
    memset(r, 0, sizeof r);
    const uint32_t n = qpp_wk::walk(p, len, cid_len, [&](uint32_t k, const Rec &w) { r[k] = w; });
    return ac_accept_rec(p, len, i, off, route_conn, route_cls, n, &r[0], slot_client, slot_server, accept_flags,
                         desc_flags, ini, d, acc);
}

}  // extern "C"

namespace {

typedef std::vector<uint8_t> Bytes;

// a client Initial of `size` bytes: flags version dcid scid token-length(0) Length(2 bytes) body
Bytes initial(uint32_t version, int dcid, size_t size)
{
    Bytes b;
    b.push_back(version == qpp_wk::kVersion2 ? 0xD0 : 0xC0);
    for (int k = 3; k >= 0; --k) b.push_back((uint8_t)(version >> (8 * k)));
    b.push_back((uint8_t)dcid);
    for (int k = 0; k < dcid; ++k) b.push_back((uint8_t)(0xD0 + k));
    b.push_back(0);  // no SCID
    b.push_back(0);  // no token
    const size_t body = size - b.size() - 2;
    b.push_back((uint8_t)(0x40 | body >> 8));
    b.push_back((uint8_t)body);
    while (b.size() < size) b.push_back((uint8_t)(0xA0 ^ b.size()));
    return b;
}

int failures = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("FAILED line %d: %s\n", __LINE__, #c);          \
            ++failures;                                            \
        }                                                          \
    } while (0)

struct Out {
    Initial ini;
    Desc d;
    Acc acc;
};

// the decision over a heap copy of exactly `len` bytes, with the record given
// (w0 == NULL: walked from those bytes)
uint32_t accept_exact(const uint8_t *src, uint32_t len, uint32_t walk_n, const Rec *w0, Out &o)
{
    uint8_t *p = (uint8_t *)malloc(len ? len : 1);
    if (!p) abort();
    if (len) memcpy(p, src, len);
    memset(&o, 0x5A, sizeof o);
    const uint8_t *q = len ? p : p + 1;  // with len == 0 the one allocated byte must not be read either
    const uint32_t st = w0 ? ac_accept_rec(q, len, 7, 4096, qpp_ac::kConnNone, qpp_ac::kClsLong, walk_n, w0, 10, 11,
                                           0, 0, &o.ini, &o.d, &o.acc)
                           : ac_accept(q, len, 8, 7, 4096, qpp_ac::kConnNone, qpp_ac::kClsLong, 10, 11, 0, 0, &o.ini,
                                       &o.d, &o.acc);
    free(p);
    return st;
}

bool names_nothing(const Out &o)
{
    for (int k = 0; k < 20; ++k)
        if (o.ini.cid[k]) return false;
    return o.ini.slot_client == qpp_ac::kSlotNone && o.ini.slot_server == qpp_ac::kSlotNone && o.ini.cid_len == 0 &&
           o.ini.flags == 0 && o.acc.desc == qpp_wk::kDescNone && o.acc.version == 0;
}

}  // namespace

int main()
{
    for (int dcid : {1, 8, 20})
        for (uint32_t version : {qpp_wk::kVersion1, qpp_wk::kVersion2}) {
            const Bytes dg = initial(version, dcid, 1200);
            Rec full[qpp_wk::kWalkMax];
            const uint32_t n = qpp_wk::walk(dg.data(), 1200, 8, [&](uint32_t k, const Rec &w) { full[k] = w; });
            CHECK(n == 1 && full[0].status == 0 && full[0].type == 0 && full[0].len == 1200);
            Out o;
            // the whole datagram, in a buffer of exactly 1200 bytes: accepted
            CHECK(accept_exact(dg.data(), 1200, 0, NULL, o) == qpp_ac::kOk);
            CHECK(o.ini.slot_client == 10 && o.ini.slot_server == 11 && o.ini.cid_len == dcid);
            CHECK(o.ini.flags == (version == qpp_wk::kVersion2 ? 1 : 0) && o.acc.version == o.ini.flags);
            CHECK(memcmp(o.ini.cid, dg.data() + 6, dcid) == 0);
            for (int k = dcid; k < 20; ++k) CHECK(o.ini.cid[k] == 0);
            CHECK(o.d.in_off == 4096 && o.d.out_off == 4096 && o.d.len == 1200 && o.d.hdr_len == full[0].pn_off);
            CHECK(o.d.pn == 0 && o.d.slot == 10 && o.d.rsv == 0 && o.acc.desc == 7 && o.acc.status == 0);
            // one byte less: too small, from its own walk (a parse error) and
            // from the whole datagram's record alike
            CHECK(accept_exact(dg.data(), 1199, 0, NULL, o) == qpp_ac::kNotInitial && names_nothing(o));
            CHECK(accept_exact(dg.data(), 1199, n, &full[0], o) == qpp_ac::kSmall && names_nothing(o));
            // every truncation of the first 6 + dcid_len bytes: walked from
            // the bytes that are there, and with the whole datagram's record,
            // which claims a DCID the buffer no longer holds
            for (uint32_t cut = 0; cut <= 6u + dcid; ++cut) {
                const uint32_t st = accept_exact(dg.data(), cut, 0, NULL, o);
                CHECK(st == qpp_ac::kNotInitial && names_nothing(o) && o.acc.status == st);
                CHECK(accept_exact(dg.data(), cut, n, &full[0], o) == qpp_ac::kSmall && names_nothing(o));
            }
        }
    if (failures) return 1;
    printf("accept_host: ok\n");
    return 0;
}
