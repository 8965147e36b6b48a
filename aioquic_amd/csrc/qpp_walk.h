// qpp_walk.h -- the header walk of a long-header datagram (quic_pp.h:
// qpp_route_walk), shared by the walking kernel and a plain g++ build
// (tests/walk_host.cc): no HIP type appears here, and the qualifier below
// vanishes outside hipcc.
//
// parse_one restates pull_quic_header (aioquic_amd/packet.py:121-159, the
// reference's quic/packet.py:181-267) for the packet at `pos` of a datagram of
// `len` bytes; walk runs it over the coalesced packets of one datagram as
// QuicConnection.receive_datagram's loop does (connection.py:793-899).
//
// Bounds: every byte read is preceded by a check against `len`; nothing at or
// past p[len] is ever read.  A varint's value is compared with the bytes that
// remain before it is added to a position, so no position ever wraps or passes
// `len`, whatever the datagram holds.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define QPP_HD __host__ __device__
#else
#define QPP_HD
#endif

namespace qpp_wk {

constexpr uint32_t kWalkMax = 4;            // QPP_WALK_MAX
constexpr uint32_t kKeysets = 5;            // QPP_KEYSETS
constexpr uint32_t kSpaces = 3;             // QPP_SPACES
constexpr uint32_t kDescNone = 0xffffffffu; // QPP_DESC_NONE
constexpr uint32_t kMaxHdr = 1500;          // QPP_MAX_HDR
constexpr uint32_t kCidMax = 20;            // QPP_CID_MAX
constexpr uint32_t kRetryTag = 16;          // RETRY_INTEGRITY_TAG_SIZE
constexpr uint32_t kVersion1 = 0x00000001u, kVersion2 = 0x6B3343CFu;

// QPP_W_*
constexpr uint8_t kOk = 0, kParse = 1, kHost = 2;
// QuicPacketType values
constexpr uint8_t kInitial = 0, kZeroRtt = 1, kHandshake = 2, kRetry = 3, kVersionNegotiation = 4, kOneRtt = 5;
constexpr uint32_t kKeysetNone = 0xffffffffu;

struct Rec {  // qpp_walk_rec
    uint32_t off;
    uint32_t len;
    uint32_t version;
    uint32_t desc;
    uint16_t pn_off;
    uint16_t token_len;
    uint8_t type;
    uint8_t status;
    uint8_t dcid_len, scid_len;
};
static_assert(sizeof(Rec) == 24, "qpp_walk_rec layout");

// A variable-length integer (RFC 9000 sec. 16) at `pos`: all four forms.
// false, with nothing moved, when its bytes do not fit before `len`.
QPP_HD inline bool pull_varint(const uint8_t *p, uint32_t len, uint32_t &pos, uint64_t &v)
{
    if (pos >= len) return false;
    const uint8_t b0 = p[pos];
    const uint32_t n = 1u << (b0 >> 6);
    if (n > len - pos) return false;
    uint64_t x = b0 & 0x3fu;
    for (uint32_t k = 1; k < n; ++k) x = (x << 8) | p[pos + k];
    pos += n;
    v = x;
    return true;
}

// A CID length byte and the CID: false when the length is > 20 or the bytes
// do not fit.
QPP_HD inline bool pull_cid(const uint8_t *p, uint32_t len, uint32_t &pos, uint8_t &cid_len)
{
    if (pos >= len) return false;
    const uint32_t n = p[pos];
    if (n > kCidMax || n > len - (pos + 1)) return false;
    pos += 1 + n;
    cid_len = (uint8_t)n;
    return true;
}

// The long-header type of the two type bits: the v2 table for version 2, the
// v1 table for every other version, grease included (packet.py:144-146).
QPP_HD inline uint8_t long_type(uint32_t version, uint32_t bits)
{
    return (uint8_t)(version == kVersion2 ? (bits + 3u) & 3u : bits);
}

// The packet at `pos` (< len).  Fills every field of `r` but desc (kDescNone):
// status kOk with the header's fields, kHost for a header whose encrypted
// offset is past kMaxHdr, or kParse (header_parse_error: off = pos, type
// kOneRtt, everything else 0).  pn_off and token_len saturate at 0xffff; both
// only do so in a kHost record.
QPP_HD inline void parse_one(const uint8_t *p, uint32_t len, uint32_t pos, uint32_t cid_len, Rec &r)
{
    const uint32_t start = pos;
    r.off = start;
    r.len = 0;
    r.version = 0;
    r.desc = kDescNone;
    r.pn_off = 0;
    r.token_len = 0;
    r.type = kOneRtt;
    r.status = kParse;
    r.dcid_len = 0;
    r.scid_len = 0;
    if (pos >= len) return;
    const uint8_t first = p[pos++];
    if (!(first & 0x80)) {
        if (!(first & 0x40)) return;           // "Packet fixed bit is zero"
        if (cid_len > len - pos) return;       // the CID does not fit
        r.len = len - start;
        r.pn_off = (uint16_t)(1 + cid_len);
        r.dcid_len = (uint8_t)cid_len;
        r.status = kOk;
        return;
    }
    if (len - pos < 4) return;
    const uint32_t version =
        (uint32_t)p[pos] << 24 | (uint32_t)p[pos + 1] << 16 | (uint32_t)p[pos + 2] << 8 | (uint32_t)p[pos + 3];
    pos += 4;
    uint8_t dl, sl;
    if (!pull_cid(p, len, pos, dl) || !pull_cid(p, len, pos, sl)) return;
    if (version == 0) {
        // Version Negotiation: no fixed-bit check, runs to the datagram's end
        r.len = len - start;
        r.type = kVersionNegotiation;
        r.dcid_len = dl;
        r.scid_len = sl;
        r.status = kOk;
        return;
    }
    if (!(first & 0x40)) return;
    const uint8_t type = long_type(version, (first >> 4) & 3u);
    uint32_t plen, token_len = 0;
    if (type == kRetry) {
        if (len - pos < kRetryTag) return;     // no room for the integrity tag
        plen = len - start;
        pos = start;                           // pn_off 0: nothing is packet-protected
    } else {
        uint64_t v;
        if (type == kInitial) {
            if (!pull_varint(p, len, pos, v)) return;
            if (v > len - pos) return;         // the token does not fit
            token_len = (uint32_t)v;
            pos += token_len;
        }
        if (!pull_varint(p, len, pos, v)) return;
        if (v > len - pos) return;             // "Packet payload is truncated"
        plen = pos - start + (uint32_t)v;
    }
    const uint32_t pn_off = pos - start;
    r.len = plen;
    r.version = version;
    r.pn_off = (uint16_t)(pn_off > 0xffffu ? 0xffffu : pn_off);
    r.token_len = (uint16_t)(token_len > 0xffffu ? 0xffffu : token_len);
    r.type = type;
    r.dcid_len = dl;
    r.scid_len = sl;
    r.status = pn_off > kMaxHdr ? kHost : kOk;
}

// The packets of one datagram, in order: emit(k, rec) for packet k <
// kWalkMax; returns how many were emitted.  The walk ends at the datagram's
// end (a short header, Version Negotiation and Retry run to it), at a parse
// error (one kParse record where it happened) and at a kHost record: a header
// past kMaxHdr, or the fourth packet when a fifth follows it.
template <class Emit>
QPP_HD inline uint32_t walk(const uint8_t *p, uint32_t len, uint32_t cid_len, Emit &&emit)
{
    uint32_t pos = 0, n = 0;
    while (pos < len && n < kWalkMax) {
        Rec r;
        parse_one(p, len, pos, cid_len, r);
        const uint32_t next = r.off + r.len;  // <= len
        if (r.status == kOk && n == kWalkMax - 1 && next < len) r.status = kHost;
        emit(n++, r);
        if (r.status != kOk) break;
        pos = next;
    }
    return n;
}

// The connection's key-set of a packet (QPP_KEYSETS: Initial v1, Initial v2,
// 0-RTT, Handshake, 1-RTT), or kKeysetNone: not packet-protected, or an
// Initial of a version that is neither v1 nor v2.
QPP_HD inline uint32_t keyset_of(uint8_t type, uint32_t version)
{
    switch (type) {
    case kInitial: return version == kVersion1 ? 0u : version == kVersion2 ? 1u : kKeysetNone;
    case kZeroRtt: return 2u;
    case kHandshake: return 3u;
    case kOneRtt: return 4u;
    default: return kKeysetNone;
    }
}

QPP_HD inline bool protected_type(uint8_t type)
{
    return type == kInitial || type == kZeroRtt || type == kHandshake || type == kOneRtt;
}

// The packet number space (QPP_SPACES: Initial, Handshake, application) of a
// packet-protected type.
QPP_HD inline uint32_t space_of(uint8_t type)
{
    return type == kInitial ? 0u : type == kHandshake ? 1u : 2u;
}

}  // namespace qpp_wk
