// qpp_send.h -- one 1-RTT packet's short header, packet number, sample padding
// and protect descriptor (quic_pp.h: qpp_send_fill), shared by k_send and a
// plain g++ build (tests/send_host.cc): no HIP type appears here, and the
// qualifier below vanishes outside hipcc.
//
// It restates what the reference's builder does for a 1-RTT packet
// (quic/packet_builder.py:19-20 the send sizes, :264-296 _end_packet's sample
// padding, :330-339 its short header):
//   header   0x40 | spin << 5 | key_phase << 2 | (pn_len - 1), the peer's CID,
//            the packet number's low 16 bits big-endian; pn_len is always 2
//   padding  max(0, 4 - pn_len - len) zero bytes (PADDING frames) behind the
//            payload, so that a 16-byte header-protection sample exists
//   an empty packet is cancelled, never sent
// The payload lies in the buffer already, at p_off; the header is written
// right-aligned against it, at [p_off - hdr_len, p_off), the padding at
// [p_off + len, p_off + len + pad).  decide() holds every check and reads no
// byte of the buffer; emit() holds every store, and stores nothing into the
// buffer unless decide() said kOk.  Neither reads the payload.
#pragma once

#include <stdint.h>

#include "qpp_route.h"  // QPP_HD

namespace qpp_sn {

constexpr uint32_t kPnLen = 2;                // QPP_SEND_PN_LEN: PACKET_NUMBER_SEND_SIZE
constexpr uint32_t kPnMax = 4;                // PACKET_NUMBER_MAX_SIZE
constexpr uint32_t kCidMax = 20;              // QPP_CID_MAX
constexpr uint32_t kTag = 16;                 // QPP_TAG_LEN
constexpr uint32_t kHead = 1 + kCidMax + kPnLen;    // QPP_SEND_HEAD: the longest header
constexpr uint32_t kPadMax = kPnMax - kPnLen - 1;   // the padding of a 1-byte payload, the shortest sent
constexpr uint32_t kTail = kPadMax + kTag;          // QPP_SEND_TAIL
constexpr uint32_t kSlotNone = 0xffffffffu;   // QPP_SLOT_NONE
constexpr uint32_t kSuiteMax = 2;             // QPP_CHACHA20_POLY1305: the last installed suite
constexpr uint32_t kSuiteEmpty = 0xffu;       // a slot that is empty, past the table, or "none"
constexpr uint64_t kPnLimit = 1ull << 62;     // packet numbers are 0 .. 2^62 - 1 (RFC 9000 sec. 12.3)

// QPP_SN_*: the first check that fails, in this order
constexpr uint8_t kOk = 0, kConn = 1, kCid = 2, kNoKey = 3, kEmpty = 4, kPn = 5, kRoom = 6;

struct Conn {  // qpp_send_conn
    uint64_t next_pn;
    uint32_t slot;
    uint8_t cid_len, spin;
    uint8_t cid[20];
    uint8_t rsv[6];
};
static_assert(sizeof(Conn) == 40, "ABI record");

struct Desc {  // qpp_desc
    uint64_t in_off, out_off;
    uint32_t len;
    uint16_t hdr_len, flags;
    uint64_t pn;
    uint32_t slot, rsv;
};
static_assert(sizeof(Desc) == 40, "ABI record");

struct Rec {  // qpp_send_rec
    uint64_t pn;
    uint16_t hdr_len;
    uint8_t status, rsv[5];
};
static_assert(sizeof(Rec) == 16, "ABI record");

// What a lane knows of its connection's send slot: its suite (kSuiteEmpty when
// the index is past the table, the slot was never installed, or there is
// none) and key phase.
struct Slot {
    uint32_t suite, key_phase;
};

// A lane's verdict and, with kOk, what emit() writes.
struct Plan {
    uint8_t status, b0;
    uint32_t hdr_len, pad;
    uint64_t pn;
};

// Every check, in the order of the statuses.  conn_ok: p_conn[i] < n_conn; c
// and s are looked at only then.  seq is the packet's ordinal among its
// connection's packets of the batch.
QPP_HD inline Plan decide(bool conn_ok, const Conn &c, const Slot &s, uint64_t p_off, uint32_t len, uint32_t seq,
                          uint64_t buf_len)
{
    Plan p = {kConn, 0, 0, 0, 0};
    if (!conn_ok) return p;
    p.status = kCid;
    if (c.cid_len > kCidMax) return p;
    p.status = kNoKey;
    if (s.suite > kSuiteMax) return p;
    p.status = kEmpty;
    if (len == 0) return p;
    p.status = kPn;
    const uint64_t pn = c.next_pn + seq;
    if (pn < c.next_pn || pn >= kPnLimit) return p;
    p.status = kRoom;
    const uint32_t hdr_len = 1 + (uint32_t)c.cid_len + kPnLen;
    const uint32_t pad = len < kPnMax - kPnLen ? kPnMax - kPnLen - len : 0;
    if (p_off < hdr_len || p_off > buf_len || (uint64_t)len + pad + kTag > buf_len - p_off) return p;
    p.status = kOk;
    p.b0 = (uint8_t)(0x40u | (c.spin ? 0x20u : 0u) | (s.key_phase & 1u) << 2 | (kPnLen - 1));
    p.hdr_len = hdr_len;
    p.pad = pad;
    p.pn = pn;
    return p;
}

// Every store of a lane: the descriptor and the record whole, whatever the
// verdict, and with kOk the header and the padding.  The CID is copied over a
// constant 20 with a guarded store per byte, and the padding likewise over
// kPadMax, so that no loop's trip count depends on the data.
QPP_HD inline void emit(const Plan &p, const Conn &c, uint64_t p_off, uint32_t len, uint8_t *buf, Desc *desc, Rec *rec)
{
    const bool ok = p.status == kOk;
    Desc d;
    d.in_off = d.out_off = ok ? p_off - p.hdr_len : p_off;
    d.len = ok ? len + p.pad : 0;
    d.hdr_len = (uint16_t)(ok ? p.hdr_len : 0);
    d.flags = 0;
    d.pn = ok ? p.pn : 0;
    d.slot = ok ? c.slot : kSlotNone;
    d.rsv = 0;
    *desc = d;
    Rec r;
    r.pn = ok ? p.pn : 0;
    r.hdr_len = (uint16_t)(ok ? p.hdr_len : 0);
    r.status = p.status;
    for (int k = 0; k < 5; ++k) r.rsv[k] = 0;
    *rec = r;
    if (!ok) return;
    uint8_t *h = buf + (p_off - p.hdr_len);
    h[0] = p.b0;
    for (uint32_t k = 0; k < kCidMax; ++k)
        if (k < c.cid_len) h[1 + k] = c.cid[k];
    h[1 + c.cid_len] = (uint8_t)(p.pn >> 8);
    h[2 + c.cid_len] = (uint8_t)p.pn;
    uint8_t *t = buf + p_off + len;
    for (uint32_t k = 0; k < kPadMax; ++k)
        if (k < p.pad) t[k] = 0;
}

// The region of the buffer a packet may touch, [p_off - kHead, p_off + len +
// kTail): the caller of the device form keeps these pairwise disjoint, the
// fused host form checks it.  False when the region does not fit [0, buf_len).
QPP_HD inline bool region(uint64_t p_off, uint32_t len, uint64_t buf_len, uint64_t *lo, uint64_t *hi)
{
    if (p_off < kHead || p_off > buf_len || (uint64_t)len + kTail > buf_len - p_off) return false;
    *lo = p_off - kHead;
    *hi = p_off + len + kTail;
    return true;
}

// The fused host form's test of the caller's arrays, before anything is
// launched (qpp_session_send_protect): offsets strictly increasing, every
// packet's region inside both buffers and behind its predecessor's, every
// connection index below n_conn, every slot inside the table or kSlotNone.
inline bool batch_ok(const Conn *conns, uint32_t n_conn, uint32_t cap, const uint64_t *off, const uint32_t *len,
                     const uint32_t *conn, uint32_t n, uint64_t in_len, uint64_t out_len)
{
    const uint64_t room = in_len < out_len ? in_len : out_len;
    uint64_t prev_hi = 0;
    for (uint32_t i = 0; i < n; ++i) {
        uint64_t lo, hi;
        if (!region(off[i], len[i], room, &lo, &hi)) return false;
        if (i && (off[i] <= off[i - 1] || lo < prev_hi)) return false;
        prev_hi = hi;
        if (conn[i] >= n_conn) return false;
    }
    for (uint32_t c = 0; c < n_conn; ++c)
        if (conns[c].slot >= cap && conns[c].slot != kSlotNone) return false;
    return true;
}

}  // namespace qpp_sn
