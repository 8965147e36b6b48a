// qpp_reply.h -- the packet a server sends instead of accepting an unrouted
// Initial (quic_pp.h: qpp_route_reply), shared by the assembling kernel and a
// plain g++ build (tests/reply_host.cc): no HIP type appears here, and the
// qualifier of qpp_walk.h vanishes outside hipcc.
//
// reply_one restates what the reference's server sends before it drops such a
// datagram (asyncio/server.py:71-111): encode_quic_version_negotiation
// (quic/packet.py:317-334) for a version it does not speak, and in Retry mode
// encode_quic_retry (quic/packet.py:288-314) around a token whose plaintext is
// the buffer of QuicRetryTokenHandler.create_token (quic/retry.py:25-28).  No
// cipher runs here: the token's seal and the Retry integrity tag are two
// AEAD-only descriptors for qpp_protect, both in place in the reply buffer.
//
// Bounds: the datagram bytes read are p[5 .. 7 + dl + sl), and only after
// dl <= 20, sl <= 20 and 7 + dl + sl <= len were checked here against the
// caller's length, not taken on trust from the walk record.  Every write lands
// in the candidate's own kStride bytes: a Retry ends at 145 at the most.
#pragma once

#include <stdint.h>

#include "qpp_accept.h"

namespace qpp_rp {

constexpr uint32_t kStride = 256;                               // QPP_REPLY_STRIDE
constexpr uint32_t kVn = 1u, kRetry = 2u;                       // QPP_RP_VN, QPP_RP_RETRY
constexpr uint8_t kKindNone = 0, kKindVn = 1, kKindRetry = 2;   // QPP_RP_KIND_*
constexpr uint8_t kStOk = 0, kBounds = 0x40, kAddr = 0x41;      // QPP_RP_OK, QPP_RP_BOUNDS, QPP_RP_ADDR
constexpr uint32_t kMaxVersions = 16;                           // QPP_RP_MAX_VERSIONS
constexpr uint32_t kAddrStride = 20, kRandStride = 16;          // QPP_RP_ADDR_STRIDE, QPP_RP_RAND_STRIDE
constexpr uint32_t kScidLen = 8;                                // the Retry's source CID (server.py:98)
constexpr uint32_t kCtrLen = 8, kTagLen = 16;
constexpr uint32_t kSlotV1 = 0, kSlotV2 = 1, kSlotToken = 2;    // the reply key table's slots
constexpr uint16_t kNoHp = 1;                                   // QPP_F_NO_HP

struct Rec {  // qpp_reply_rec
    uint32_t off;
    uint16_t len;
    uint8_t kind, status;
};
static_assert(sizeof(Rec) == 8, "qpp_reply_rec layout");

// encode_long_header_first_byte for a Retry (packet.py:270-285): type code 3
// in version 1, 0 in version 2, `unused` in the low four bits.
QPP_HD inline uint8_t retry_first_byte(uint32_t version, uint32_t unused)
{
    return (uint8_t)(0xC0u | (version == qpp_wk::kVersion2 ? 0u : 0x30u) | (unused & 0xfu));
}

// The Retry pseudo-packet of RFC 9001 sec. 5.8 up to its token, at out[0]:
// [odl | ODCID | first byte | version | dl | DCID | sl | SCID].  The Retry
// packet itself starts at 1 + odl; returns where its token starts.
QPP_HD inline uint32_t retry_header(uint8_t *__restrict__ out, uint32_t version, uint32_t unused,
                                    const uint8_t *odcid, uint32_t odl, const uint8_t *dcid, uint32_t dl,
                                    const uint8_t *scid, uint32_t sl)
{
    uint32_t at = 0;
    out[at++] = (uint8_t)odl;
    for (uint32_t k = 0; k < odl; ++k) out[at++] = odcid[k];
    out[at++] = retry_first_byte(version, unused);
    out[at++] = (uint8_t)(version >> 24);
    out[at++] = (uint8_t)(version >> 16);
    out[at++] = (uint8_t)(version >> 8);
    out[at++] = (uint8_t)version;
    out[at++] = (uint8_t)dl;
    for (uint32_t k = 0; k < dl; ++k) out[at++] = dcid[k];
    out[at++] = (uint8_t)sl;
    for (uint32_t k = 0; k < sl; ++k) out[at++] = scid[k];
    return at;
}

// The whole pseudo-packet around a token the caller holds; returns its length
// (the AAD length of the integrity tag).  out needs 1 + odl + 7 + dl + sl +
// token_len bytes.
QPP_HD inline uint32_t retry_pseudo(uint8_t *__restrict__ out, uint32_t version, uint32_t unused,
                                    const uint8_t *odcid, uint32_t odl, const uint8_t *dcid, uint32_t dl,
                                    const uint8_t *scid, uint32_t sl, const uint8_t *token, uint32_t token_len)
{
    uint32_t at = retry_header(out, version, unused, odcid, odl, dcid, dl, scid, sl);
    for (uint32_t k = 0; k < token_len; ++k) out[at++] = token[k];
    return at;
}

QPP_HD inline void inert_desc(qpp_ac::Desc &d, uint64_t base)
{
    d.in_off = base;
    d.out_off = base;
    d.len = 0;
    d.hdr_len = 0;
    d.flags = kNoHp;
    d.pn = 0;
    d.slot = qpp_ac::kSlotNone;
    d.rsv = 0;
}

// Candidate a, whose accept status is acc_status and whose datagram is the
// len bytes at p with packet 0's walk record w0 (p is not touched unless a
// reply is due).  addr: the candidate's kAddrStride bytes [alen | packed IP |
// port, big-endian] or NULL; rnd: its kRandStride random bytes, [0, 8) the
// Retry's source CID, [8] the Version Negotiation's first byte.  region: its
// kStride bytes of the reply buffer, 8-byte aligned, which lie at a * kStride
// of the buffer the descriptors and the record index.  Everything is written
// whole: the region zero filled first, both descriptors, the record.
QPP_HD inline void reply_one(uint32_t a, uint8_t acc_status, const qpp_wk::Rec &w0, uint32_t len, const uint8_t *p,
                             const uint8_t *addr, const uint8_t *rnd, uint64_t token_ctr, const uint32_t *versions,
                             uint32_t n_versions, uint32_t reply_flags, uint8_t *__restrict__ region,
                             qpp_ac::Desc &seal, qpp_ac::Desc &tag, Rec &rec)
{
    const uint64_t base = (uint64_t)a * kStride;
    uint64_t *z = reinterpret_cast<uint64_t *>(region);
    for (uint32_t k = 0; k < kStride / 8; ++k) z[k] = 0;
    inert_desc(seal, base);
    inert_desc(tag, base);
    rec.off = (uint32_t)base;
    rec.len = 0;
    rec.kind = kKindNone;
    rec.status = kStOk;
    const bool vn = acc_status == qpp_ac::kVersion && (reply_flags & kVn);
    const bool retry = acc_status == qpp_ac::kNoToken && (reply_flags & kRetry);
    if (!vn && !retry) return;
    const uint32_t dl = w0.dcid_len, sl = w0.scid_len;
    // the record's lengths, held against the caller's length and then against the bytes themselves
    if (dl > qpp_wk::kCidMax || sl > qpp_wk::kCidMax || 7u + dl + sl > len || p[5] != dl || p[6 + dl] != sl) {
        rec.status = kBounds;
        return;
    }
    const uint8_t *c_dcid = p + 6, *c_scid = p + 7 + dl;
    if (vn) {
        // source_cid = the client's DCID, destination_cid = its SCID (server.py:77-81)
        uint32_t at = 0;
        region[at++] = (uint8_t)(0x80u | (rnd[8] & 0x7fu));
        at += 4;  // version 0
        region[at++] = (uint8_t)sl;
        for (uint32_t k = 0; k < sl; ++k) region[at++] = c_scid[k];
        region[at++] = (uint8_t)dl;
        for (uint32_t k = 0; k < dl; ++k) region[at++] = c_dcid[k];
        const uint32_t nv = n_versions < kMaxVersions ? n_versions : kMaxVersions;
        // (a constant trip count: the list stays where the kernel's arguments are)
        for (uint32_t k = 0; k < kMaxVersions; ++k)
            if (k < nv) {
                const uint32_t v = versions[k];
                region[at++] = (uint8_t)(v >> 24);
                region[at++] = (uint8_t)(v >> 16);
                region[at++] = (uint8_t)(v >> 8);
                region[at++] = (uint8_t)v;
            }
        rec.len = (uint16_t)at;
        rec.kind = kKindVn;
        return;
    }
    const uint32_t version = w0.version;
    if (dl < 1 || (version != qpp_wk::kVersion1 && version != qpp_wk::kVersion2)) {
        rec.status = kBounds;  // not what QPP_ACC_NO_TOKEN says of an Initial
        return;
    }
    const uint32_t alen = addr ? addr[0] : 0;
    if (alen != 6 && alen != 18) {
        rec.status = kAddr;
        return;
    }
    // source_cid = rnd[0, 8), destination_cid = the client's SCID, the original DCID = its DCID
    const uint32_t pkt = 1 + dl;
    const uint32_t tok = retry_header(region, version, 0, c_dcid, dl, c_scid, sl, rnd, kScidLen);
    const uint64_t ctr = token_ctr + a;
    uint32_t at = tok;
    for (uint32_t k = 0; k < kCtrLen; ++k) region[at++] = (uint8_t)(ctr >> (56 - 8 * k));
    // create_token's buffer (retry.py:25-28): three one-byte-length opaques
    region[at++] = (uint8_t)alen;
    for (uint32_t k = 0; k < alen; ++k) region[at++] = addr[1 + k];
    region[at++] = (uint8_t)dl;
    for (uint32_t k = 0; k < dl; ++k) region[at++] = c_dcid[k];
    region[at++] = (uint8_t)kScidLen;
    for (uint32_t k = 0; k < kScidLen; ++k) region[at++] = rnd[k];
    const uint32_t plen = at - tok - kCtrLen;
    const uint32_t end = at + kTagLen;  // of the token and of the pseudo-packet: <= 129
    seal.in_off = seal.out_off = base + tok;
    seal.len = plen;
    seal.hdr_len = (uint16_t)kCtrLen;
    seal.pn = ctr;
    seal.slot = kSlotToken;
    tag.hdr_len = (uint16_t)end;
    tag.slot = version == qpp_wk::kVersion2 ? kSlotV2 : kSlotV1;
    rec.off = (uint32_t)(base + pkt);
    rec.len = (uint16_t)(end - pkt + kTagLen);
    rec.kind = kKindRetry;
}

}  // namespace qpp_rp
