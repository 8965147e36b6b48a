// Host build of aioquic_amd/csrc/qpp_reply.h for tests/test_reply_host.py:
// the assembly every lane of k_reply runs.  Plain g++, no HIP.
//
// Built as a shared object, the functions below are called through ctypes.
// Built as a program (with -fsanitize=address,undefined), main() runs a lane
// over heap buffers of exactly the size it may touch -- a datagram that ends
// at 7 + dl + sl, every truncation of it, a walk record whose CID lengths
// disagree with the bytes, an address and random bytes of exactly their
// strides, a region of exactly 256 bytes -- so that a read or write past any
// of them is the sanitizer's to report.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../aioquic_amd/csrc/qpp_reply.h"

using qpp_ac::Desc;
using qpp_wk::Rec;
typedef qpp_rp::Rec Reply;

extern "C" {

// one candidate from its accept status and the three fields of packet 0's walk record the reply needs
void rp_reply(uint32_t a, uint32_t acc_status, uint32_t version, uint32_t dcid_len, uint32_t scid_len,
              const uint8_t *p, uint32_t len, const uint8_t *addr, const uint8_t *rnd, uint64_t token_ctr,
              const uint32_t *versions, uint32_t n_versions, uint32_t reply_flags, uint8_t *region, Desc *seal,
              Desc *tag, Reply *rec)
{
    Rec w0;
    memset(&w0, 0, sizeof w0);
    w0.version = version;
    w0.dcid_len = (uint8_t)dcid_len;
    w0.scid_len = (uint8_t)scid_len;
    qpp_rp::reply_one(a, (uint8_t)acc_status, w0, len, p, addr, rnd, token_ctr, versions, n_versions, reply_flags,
                      region, *seal, *tag, *rec);
}

// the generic pseudo-packet builder
uint32_t rp_pseudo(uint8_t *out, uint32_t version, uint32_t unused, const uint8_t *odcid, uint32_t odl,
                   const uint8_t *dcid, uint32_t dl, const uint8_t *scid, uint32_t sl, const uint8_t *token,
                   uint32_t token_len)
{
    return qpp_rp::retry_pseudo(out, version, unused, odcid, odl, dcid, dl, scid, sl, token, token_len);
}

}  // extern "C"

namespace {

typedef std::vector<uint8_t> Bytes;

// flags version dl DCID sl SCID, and nothing after them
Bytes header(uint32_t version, uint32_t dl, uint32_t sl)
{
    Bytes b;
    b.push_back(0xC0);
    for (int k = 3; k >= 0; --k) b.push_back((uint8_t)(version >> (8 * k)));
    b.push_back((uint8_t)dl);
    for (uint32_t k = 0; k < dl; ++k) b.push_back((uint8_t)(0xD0 + k));
    b.push_back((uint8_t)sl);
    for (uint32_t k = 0; k < sl; ++k) b.push_back((uint8_t)(0x50 + k));
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
    uint8_t region[qpp_rp::kStride];
    Desc seal, tag;
    Reply rec;
};

uint8_t *exact(const uint8_t *src, size_t n)
{
    uint8_t *p = (uint8_t *)malloc(n ? n : 1);
    if (!p) abort();
    if (n) memcpy(p, src, n);
    return p;
}

// a lane over heap copies of exactly the bytes it may touch; the walk
// record's lengths are given apart from the bytes
void reply_exact(uint32_t a, uint8_t status, uint32_t version, uint32_t dl, uint32_t sl, const uint8_t *src,
                 uint32_t len, uint32_t alen, Out &o)
{
    uint8_t addr_src[qpp_rp::kAddrStride] = {0}, rnd_src[qpp_rp::kRandStride];
    addr_src[0] = (uint8_t)alen;
    for (uint32_t k = 1; k < qpp_rp::kAddrStride; ++k) addr_src[k] = (uint8_t)(0x20 + k);
    for (uint32_t k = 0; k < qpp_rp::kRandStride; ++k) rnd_src[k] = (uint8_t)(0xE0 + k);
    const uint32_t versions_src[2] = {qpp_wk::kVersion1, qpp_wk::kVersion2};
    uint8_t *p = exact(src, len), *addr = exact(addr_src, sizeof addr_src), *rnd = exact(rnd_src, sizeof rnd_src);
    uint32_t *versions = (uint32_t *)exact((const uint8_t *)versions_src, sizeof versions_src);
    uint8_t *region = (uint8_t *)malloc(qpp_rp::kStride);
    if (!region) abort();
    memset(region, 0x5A, qpp_rp::kStride);
    memset(&o.seal, 0x5A, sizeof o.seal);
    memset(&o.tag, 0x5A, sizeof o.tag);
    memset(&o.rec, 0x5A, sizeof o.rec);
    Rec w0;
    memset(&w0, 0, sizeof w0);
    w0.version = version;
    w0.dcid_len = (uint8_t)dl;
    w0.scid_len = (uint8_t)sl;
    const uint8_t *q = len ? p : p + 1;  // with len == 0 the one allocated byte must not be read either
    qpp_rp::reply_one(a, status, w0, len, q, addr, rnd, 1000, versions, 2, qpp_rp::kVn | qpp_rp::kRetry, region,
                      o.seal, o.tag, o.rec);
    memcpy(o.region, region, qpp_rp::kStride);
    free(p), free(addr), free(rnd), free(versions), free(region);
}

bool says_nothing(const Out &o, uint32_t a, uint8_t status)
{
    for (uint32_t k = 0; k < qpp_rp::kStride; ++k)
        if (o.region[k]) return false;
    const uint64_t base = (uint64_t)a * qpp_rp::kStride;
    for (const Desc *d : {&o.seal, &o.tag})
        if (d->in_off != base || d->out_off != base || d->len || d->hdr_len || d->flags != qpp_rp::kNoHp || d->pn ||
            d->slot != qpp_ac::kSlotNone || d->rsv)
            return false;
    return o.rec.off == base && o.rec.len == 0 && o.rec.kind == qpp_rp::kKindNone && o.rec.status == status;
}

}  // namespace

int main()
{
    const uint32_t a = 3;
    const uint64_t base = (uint64_t)a * qpp_rp::kStride;
    for (uint32_t dl : {0u, 1u, 8u, 20u})
        for (uint32_t sl : {0u, 8u, 20u})
            for (uint32_t version : {qpp_wk::kVersion1, qpp_wk::kVersion2, 0x0a0a0a0au}) {
                const bool known = version != 0x0a0a0a0au;
                if (known && dl == 0) continue;  // QPP_ACC_NO_TOKEN is never said of an empty DCID
                const uint8_t status = known ? qpp_ac::kNoToken : qpp_ac::kVersion;
                const Bytes dg = header(version, dl, sl);
                const uint32_t full = 7 + dl + sl;
                CHECK(dg.size() == full);
                Out o;
                // the datagram ends where its CIDs end: answered
                for (uint32_t alen : {6u, 18u}) {
                    reply_exact(a, status, version, dl, sl, dg.data(), full, alen, o);
                    CHECK(o.rec.status == qpp_rp::kStOk);
                    if (known) {
                        const uint32_t tok = 1 + dl + 7 + sl + 8, plen = 1 + alen + 1 + dl + 1 + 8;
                        CHECK(o.rec.kind == qpp_rp::kKindRetry && o.rec.off == base + 1 + dl);
                        CHECK(o.rec.len == 7 + sl + 8 + (8 + plen + 16) + 16);
                        CHECK(o.seal.in_off == base + tok && o.seal.out_off == base + tok && o.seal.len == plen);
                        CHECK(o.seal.hdr_len == 8 && o.seal.pn == 1000 + a && o.seal.slot == qpp_rp::kSlotToken);
                        CHECK(o.tag.in_off == base && o.tag.out_off == base && o.tag.len == 0);
                        CHECK(o.tag.hdr_len == tok + 8 + plen + 16 && o.tag.hdr_len + 16u <= 145);
                        CHECK(o.tag.slot == (version == qpp_wk::kVersion2 ? qpp_rp::kSlotV2 : qpp_rp::kSlotV1));
                        CHECK(o.region[0] == dl && memcmp(o.region + 1, dg.data() + 6, dl) == 0);
                        CHECK(o.region[1 + dl] == (version == qpp_wk::kVersion2 ? 0xC0 : 0xF0));
                        for (uint32_t k = o.tag.hdr_len - 16; k < qpp_rp::kStride; ++k) CHECK(o.region[k] == 0);
                    } else {
                        CHECK(o.rec.kind == qpp_rp::kKindVn && o.rec.off == base && o.rec.len == 7 + sl + dl + 8);
                        CHECK(o.region[0] == (0x80 | (0xE8 & 0x7f)) && o.region[5] == sl && o.region[6 + sl] == dl);
                        CHECK(o.seal.slot == qpp_ac::kSlotNone && o.tag.slot == qpp_ac::kSlotNone);
                    }
                }
                // every truncation, with the whole datagram's record: the
                // record claims CIDs the buffer no longer holds
                for (uint32_t cut = 0; cut < full; ++cut) {
                    reply_exact(a, status, version, dl, sl, dg.data(), cut, 6, o);
                    CHECK(says_nothing(o, a, qpp_rp::kBounds));
                }
                // a record whose lengths disagree with the bytes, in a buffer
                // that ends where the bytes' own CIDs end
                for (uint32_t wd = 0; wd <= 21; ++wd)
                    for (uint32_t ws : {0u, 1u, 8u, 20u, 21u, 255u}) {
                        if (wd == dl && ws == sl) continue;
                        reply_exact(a, status, version, wd, ws, dg.data(), full, 18, o);
                        CHECK(says_nothing(o, a, qpp_rp::kBounds));
                    }
                // an address length that is neither 6 nor 18: nothing of the address is read
                if (known)
                    for (uint32_t alen : {0u, 5u, 7u, 17u, 19u, 255u}) {
                        reply_exact(a, status, version, dl, sl, dg.data(), full, alen, o);
                        CHECK(says_nothing(o, a, qpp_rp::kAddr));
                    }
                // a status that gets no reply reads nothing: not even a buffer of no bytes
                for (uint8_t st : {qpp_ac::kOk, qpp_ac::kRouted, qpp_ac::kNotInitial, qpp_ac::kSmall, qpp_ac::kCid}) {
                    reply_exact(a, st, version, dl, sl, dg.data(), 0, 6, o);
                    CHECK(says_nothing(o, a, qpp_rp::kStOk));
                }
            }
    if (failures) return 1;
    printf("reply_host: ok\n");
    return 0;
}
