// qpp_phase.h -- whether a routed short-header packet belongs to its
// connection's next key phase (quic_pp.h: qpp_route_phase), shared by k_phase
// and a plain g++ build (tests/phase_host.cc): no HIP type appears here, and
// the qualifier below vanishes outside hipcc.
//
// A peer's key update keeps the header-protection key (quic/crypto.py:157-168,
// apply_key_phase: only the AEAD key, the phase and the secret change), so the
// mask of the current slot's HP key unmasks the first byte of a packet of
// either phase.  The decision is cut in two around that mask, which only the
// device computes: eligible() says, from the descriptor and the two slots
// alone, whether a lane looks at its packet at all; flips() says, from the
// first byte and mask byte 0, whether the packet's key-phase bit differs from
// the current slot's.  decide() is both.  A lane that is not eligible reads no
// packet byte; an eligible one reads byte 0 and the sixteen sample bytes at
// sample_off(), which eligible() has placed inside the packet.
#pragma once

#include <stdint.h>

#include "qpp_route.h"  // QPP_HD

namespace qpp_ph {

constexpr uint32_t kSlotNone = 0xffffffffu;  // QPP_SLOT_NONE
constexpr uint32_t kNoEntry = 0xffffffffu;   // next_entry: the lane consults no d_next entry
constexpr uint32_t kSuiteMax = 2;            // QPP_CHACHA20_POLY1305: the last installed suite
constexpr uint32_t kSuiteEmpty = 0xffu;      // a slot that is empty, past the table, or "none"
constexpr uint16_t kNoHp = 1;                // QPP_F_NO_HP
constexpr uint32_t kMaxHdr = 1500;           // QPP_MAX_HDR
constexpr uint8_t kClsShort = 0;             // QPP_R_SHORT

struct Desc {  // qpp_desc
    uint64_t in_off, out_off;
    uint32_t len;
    uint16_t hdr_len, flags;
    uint64_t pn;
    uint32_t slot, rsv;
};
static_assert(sizeof(Desc) == 40, "ABI record");

// What a lane knows of a key slot: its suite (kSuiteEmpty when the index is
// past the table, the slot was never installed, or there is none) and phase.
struct Slot {
    uint32_t suite, key_phase;
};

// The d_next entry descriptor i consults: its connection's with route
// records (short headers of a connection below n_next only), its own without.
QPP_HD inline uint32_t next_entry(bool routed, uint8_t cls, uint32_t conn, uint32_t n_next, uint32_t i)
{
    if (!routed) return i;
    return cls == kClsShort && conn < n_next ? conn : kNoEntry;
}

// Whether the lane acts: header protection is on, the header and the sample
// lie inside the packet by the bounds pkt_begin checks (so a packet that gets
// QPP_S_LENGTH from the packet kernels still gets it), the current slot is
// installed, and the next slot is installed with the same suite and the other
// phase.  Reads no packet byte.
QPP_HD inline bool eligible(const Desc &d, const Slot &s0, const Slot &s1)
{
    if (d.flags & kNoHp) return false;
    if (d.hdr_len < 1 || d.hdr_len > kMaxHdr - 4) return false;
    if ((uint64_t)d.hdr_len + 20 > d.len) return false;
    if (s0.suite > kSuiteMax || s1.suite > kSuiteMax) return false;
    return s1.suite == s0.suite && s1.key_phase != s0.key_phase;
}

// Offset of the sixteen sample bytes from the packet's start (_crypto.c:331).
QPP_HD inline uint32_t sample_off(const Desc &d) { return (uint32_t)d.hdr_len + 4; }

// The first byte as it is on the wire and mask byte 0: a short header (bit 7
// clear once unmasked) whose key-phase bit is not the current slot's.
QPP_HD inline bool flips(uint8_t b0_wire, uint8_t mask0, uint32_t s0_phase)
{
    const uint32_t b0 = (uint32_t)b0_wire ^ (mask0 & 0x1fu);
    return !(b0 & 0x80u) && ((b0 >> 2) & 1u) != s0_phase;
}

// Whether to point the descriptor at the next slot.
QPP_HD inline bool decide(const Desc &d, uint8_t b0_wire, uint8_t mask0, const Slot &s0, const Slot &s1)
{
    return eligible(d, s0, s1) && flips(b0_wire, mask0, s0.key_phase);
}

}  // namespace qpp_ph
