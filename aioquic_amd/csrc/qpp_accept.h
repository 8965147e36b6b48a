// qpp_accept.h -- whether a server may answer an unrouted Initial, and the
// records that follow from it (quic_pp.h: qpp_route_accept), shared by the
// accepting kernel and a plain g++ build (tests/accept_host.cc): no HIP type
// appears here, and the qualifier below vanishes outside hipcc.
//
// decide restates the checks the reference's server runs on a datagram whose
// DCID it does not know, before it creates a connection
// (asyncio/server.py:60-152): a supported version (:71-84), a datagram of at
// least 1200 bytes (:91), and in Retry mode a token (:95-111).  The header
// itself was parsed by the walk (qpp_walk.h); nothing is parsed again here.
//
// Bounds: the only datagram bytes read are the DCID's, p[6 .. 6 + dcid_len),
// and only after 6 + dcid_len <= len was checked here against the caller's
// length, not taken from the walk record.
#pragma once

#include <stdint.h>

#include "qpp_walk.h"

namespace qpp_ac {

// QPP_ACC_*
constexpr uint8_t kOk = 0, kRouted = 1, kNotInitial = 2, kVersion = 3, kSmall = 4, kCid = 5, kNoToken = 6;
constexpr uint8_t kBadToken = 7;             // QPP_ACC_BAD_TOKEN: only from qpp_route_accept_tokens
constexpr uint32_t kNeedToken = 1u;          // QPP_A_NEED_TOKEN
constexpr uint32_t kMinDatagram = 1200;      // SMALLEST_MAX_DATAGRAM_SIZE (server.py:91)
constexpr uint32_t kSlotNone = 0xffffffffu;  // QPP_SLOT_NONE
constexpr uint32_t kConnNone = 0xffffffffu;  // QPP_CONN_NONE
constexpr uint8_t kClsLong = 1;              // QPP_R_LONG
constexpr uint8_t kDeriveV2 = 1;             // QPP_DERIVE_V2

struct Initial {  // qpp_initial
    uint32_t slot_client, slot_server;
    uint8_t cid_len, flags, rsv[2];
    uint8_t cid[20];
};
struct Desc {  // qpp_desc
    uint64_t in_off, out_off;
    uint32_t len;
    uint16_t hdr_len, flags;
    uint64_t pn;
    uint32_t slot, rsv;
};
struct Acc {  // qpp_accept_rec
    uint32_t desc;
    uint8_t status, version, rsv[2];
};
static_assert(sizeof(Initial) == 32 && sizeof(Desc) == 40 && sizeof(Acc) == 8, "ABI records");

// The verdict on one candidate: the first failing test names the status.
// route_conn / route_cls: the datagram's route record; walk_n and w0: its walk
// count and packet 0's record (w0 is not looked at when walk_n == 0); len: the
// datagram's length.  Reads no datagram byte.
QPP_HD inline uint8_t decide(uint32_t route_conn, uint8_t route_cls, uint32_t walk_n, const qpp_wk::Rec &w0,
                             uint32_t len, uint32_t accept_flags)
{
    if (route_conn != kConnNone || route_cls != kClsLong) return kRouted;
    if (walk_n < 1 || w0.status != qpp_wk::kOk || w0.type != qpp_wk::kInitial || w0.off != 0) return kNotInitial;
    if (w0.version != qpp_wk::kVersion1 && w0.version != qpp_wk::kVersion2) return kVersion;
    if (len < kMinDatagram) return kSmall;
    const uint32_t dl = w0.dcid_len;
    if (dl < 1 || dl > qpp_wk::kCidMax || 6u + dl > len) return kCid;
    if ((accept_flags & kNeedToken) && w0.token_len == 0) return kNoToken;
    return kOk;
}

// Candidate a of datagram i (at p, len bytes, d_off[i] = off) whose verdict is
// st: its qpp_initial and qpp_accept_rec, always, and its descriptor when st is
// kOk (d is left alone otherwise).  A rejected candidate's qpp_initial names
// no slot and no CID: derived, never installed.
QPP_HD inline uint8_t accept_fill(uint8_t st, uint32_t i, const qpp_wk::Rec &w0, uint64_t off, const uint8_t *p,
                                  uint32_t slot_client, uint32_t slot_server, uint16_t desc_flags, Initial &ini,
                                  Desc &d, Acc &acc)
{
    ini.slot_client = ini.slot_server = kSlotNone;
    ini.cid_len = ini.flags = ini.rsv[0] = ini.rsv[1] = 0;
    for (uint32_t k = 0; k < qpp_wk::kCidMax; ++k) ini.cid[k] = 0;
    acc.desc = qpp_wk::kDescNone;
    acc.status = st;
    acc.version = 0;
    acc.rsv[0] = acc.rsv[1] = 0;
    if (st != kOk) return st;
    const bool v2 = w0.version == qpp_wk::kVersion2;
    const uint32_t dl = w0.dcid_len;  // 1..20, 6 + dl <= len
    ini.slot_client = slot_client;
    ini.slot_server = slot_server;
    ini.cid_len = (uint8_t)dl;
    ini.flags = v2 ? kDeriveV2 : 0;
    // (a constant trip count: the record stays in registers in the kernel)
    for (uint32_t k = 0; k < qpp_wk::kCidMax; ++k) ini.cid[k] = k < dl ? p[6 + k] : 0;
    d.in_off = off;
    d.out_off = off;
    d.len = w0.len;
    d.hdr_len = w0.pn_off;
    d.flags = desc_flags;
    d.pn = 0;
    d.slot = slot_client;
    d.rsv = 0;
    acc.desc = i;
    acc.version = v2 ? 1 : 0;
    return st;
}

// decide, then accept_fill with its verdict.
QPP_HD inline uint8_t accept_one(uint32_t i, uint32_t route_conn, uint8_t route_cls, uint32_t walk_n,
                                 const qpp_wk::Rec &w0, uint64_t off, uint32_t len, const uint8_t *p,
                                 uint32_t slot_client, uint32_t slot_server, uint32_t accept_flags,
                                 uint16_t desc_flags, Initial &ini, Desc &d, Acc &acc)
{
    const uint8_t st = decide(route_conn, route_cls, walk_n, w0, len, accept_flags);
    return accept_fill(st, i, w0, off, p, slot_client, slot_server, desc_flags, ini, d, acc);
}

}  // namespace qpp_ac
