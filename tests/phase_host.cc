// Host build of aioquic_amd/csrc/qpp_phase.h for tests/test_phase_host.py:
// the decision every lane of k_phase runs.  Plain g++, no HIP.
//
// Built as a shared object, the functions below are called through ctypes.
// ph_lane is one lane of the kernel in its order -- the d_next entry, the two
// slots, eligible(), then byte 0 and the sample, the mask, flips() -- with the
// mask left to a callback (the test's is the C oracle's HeaderProtection
// mask).  Built as a program (with -fsanitize=address,undefined), main() runs
// ph_lane over heap buffers of exactly the packet's size, so that a read at or
// past p[len] is the sanitizer's to report.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../aioquic_amd/csrc/qpp_phase.h"

using qpp_ph::Desc;
using qpp_ph::Slot;

struct Route {  // qpp_route_rec
    uint32_t conn;
    uint8_t cls, rsv[3];
};

typedef void (*mask_fn)(uint32_t suite, uint32_t slot, const uint8_t *sample, uint8_t *mask);

extern "C" {

uint32_t ph_next_entry(uint32_t routed, uint32_t cls, uint32_t conn, uint32_t n_next, uint32_t i)
{
    return qpp_ph::next_entry(routed != 0, (uint8_t)cls, conn, n_next, i);
}

uint32_t ph_eligible(const Desc *d, uint32_t s0_suite, uint32_t s0_phase, uint32_t s1_suite, uint32_t s1_phase)
{
    return qpp_ph::eligible(*d, Slot{s0_suite, s0_phase}, Slot{s1_suite, s1_phase});
}

uint32_t ph_flips(uint32_t b0, uint32_t mask0, uint32_t s0_phase)
{
    return qpp_ph::flips((uint8_t)b0, (uint8_t)mask0, s0_phase);
}

uint32_t ph_decide(const Desc *d, uint32_t b0, uint32_t mask0, uint32_t s0_suite, uint32_t s0_phase, uint32_t s1_suite,
                   uint32_t s1_phase)
{
    return qpp_ph::decide(*d, (uint8_t)b0, (uint8_t)mask0, Slot{s0_suite, s0_phase}, Slot{s1_suite, s1_phase});
}

// Lane i of k_phase over host memory.  slots[cap]: suite (qpp_ph::kSuiteEmpty:
// never installed) and phase per key slot; route may be NULL.  Returns what the
// kernel writes to d_phase[i]; desc[i].slot is the only other thing written.
uint32_t ph_lane(const Slot *slots, uint32_t cap, const Route *route, const uint32_t *next, uint32_t n_next,
                 Desc *desc, uint32_t i, const uint8_t *in, mask_fn mask_of)
{
    const Desc d = desc[i];
    uint32_t e = i, s1i = qpp_ph::kSlotNone;
    if (route) e = qpp_ph::next_entry(true, route[i].cls, route[i].conn, n_next, i);
    if (e != qpp_ph::kNoEntry) s1i = next[e];
    Slot s0 = {qpp_ph::kSuiteEmpty, 0}, s1 = {qpp_ph::kSuiteEmpty, 0};
    if (d.slot < cap) s0 = slots[d.slot];
    if (s1i < cap) s1 = slots[s1i];
    if (!qpp_ph::eligible(d, s0, s1)) return 0;
    const uint8_t *src = in + d.in_off;
    const uint8_t b0 = src[0];
    uint8_t sample[16], mask[16];
    memcpy(sample, src + qpp_ph::sample_off(d), 16);
    mask_of(s0.suite, d.slot, sample, mask);
    if (!qpp_ph::flips(b0, mask[0], s0.key_phase)) return 0;
    desc[i].slot = s1i;
    return 1;
}

}  // extern "C"

namespace {

int failures = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("FAILED line %d: %s\n", __LINE__, #c);          \
            ++failures;                                            \
        }                                                          \
    } while (0)

// a stand-in mask that depends on every sample byte, so that all sixteen are read
void xor_mask(uint32_t suite, uint32_t slot, const uint8_t *sample, uint8_t *mask)
{
    uint8_t x = (uint8_t)(suite + slot);
    for (int k = 0; k < 16; ++k) x ^= sample[k];
    memset(mask, x, 16);
}

// slots 0 / 1: suite 0, phases 0 / 1; 2: suite 1, phase 1; 3: empty
const Slot kSlots[4] = {{0, 0}, {0, 1}, {1, 1}, {qpp_ph::kSuiteEmpty, 0}};

struct Run {
    uint32_t phase, slot;
    bool only_slot;  // nothing of the descriptor but its slot changed
};

// the lane over a heap copy of exactly `len` packet bytes at in_off = 0
Run lane_exact(const uint8_t *pkt, uint32_t len, uint16_t hdr_len, uint16_t flags, uint32_t slot, const Route *route,
               uint32_t next)
{
    uint8_t *p = (uint8_t *)malloc(len ? len : 1);
    if (!p) abort();
    if (len) memcpy(p, pkt, len);
    Desc d = {0, 7, len, hdr_len, flags, 99, slot, 0};
    const Desc before = d;
    const uint32_t nx[1] = {next};
    const uint8_t *q = len ? p : p + 1;  // with len == 0 the one allocated byte must not be read either
    const uint32_t ph = ph_lane(kSlots, 4, route, nx, 1, &d, 0, q, xor_mask);
    free(p);
    Desc same = d;
    same.slot = before.slot;
    return Run{ph, d.slot, memcmp(&same, &before, sizeof same) == 0};
}

}  // namespace

int main()
{
    uint8_t pkt[64];
    for (int k = 0; k < 64; ++k) pkt[k] = (uint8_t)(0x30 + 3 * k);
    for (uint16_t h : {(uint16_t)1, (uint16_t)9, (uint16_t)21}) {
        const uint32_t len = h + 20u;  // the sample's last byte is the packet's last
        // make byte 0 a short header whose phase bit, once unmasked, is 1 (flips slot 0) or 0
        uint8_t m[16];
        xor_mask(0, 0, pkt + h + 4, m);
        for (int bit = 0; bit < 2; ++bit) {
            pkt[0] = (uint8_t)((0x40 | bit << 2) ^ (m[0] & 0x1f));
            Run r = lane_exact(pkt, len, h, 0, 0, NULL, 1);
            CHECK(r.phase == (uint32_t)bit && r.slot == (bit ? 1u : 0u) && r.only_slot);
        }
        pkt[0] = (uint8_t)(0x44 ^ (m[0] & 0x1f));  // flips from here on
        const Route shortr = {0, 0, {0, 0, 0}}, longr = {0, 1, {0, 0, 0}}, past = {1, 0, {0, 0, 0}};
        CHECK(lane_exact(pkt, len, h, 0, 0, &shortr, 1).phase == 1);
        CHECK(lane_exact(pkt, len, h, 0, 0, &longr, 1).phase == 0);
        CHECK(lane_exact(pkt, len, h, 0, 0, &past, 1).phase == 0);
        // one byte short of a sample: nothing is read (the buffer holds len - 1 bytes)
        Run r = lane_exact(pkt, len - 1, h, 0, 0, NULL, 1);
        CHECK(r.phase == 0 && r.slot == 0 && r.only_slot);
        // every truncation, and an empty packet
        for (uint32_t cut = 0; cut < len; ++cut) CHECK(lane_exact(pkt, cut, h, 0, 0, NULL, 1).phase == 0);
        // each other condition failing alone
        CHECK(lane_exact(pkt, len, h, qpp_ph::kNoHp, 0, NULL, 1).phase == 0);
        CHECK(lane_exact(pkt, len, 0, 0, 0, NULL, 1).phase == 0);
        CHECK(lane_exact(pkt, len, h, 0, 0, NULL, qpp_ph::kSlotNone).phase == 0);
        CHECK(lane_exact(pkt, len, h, 0, 0, NULL, 4).phase == 0);  // past the table
        CHECK(lane_exact(pkt, len, h, 0, 0, NULL, 3).phase == 0);  // empty
        CHECK(lane_exact(pkt, len, h, 0, 0, NULL, 2).phase == 0);  // another suite
        CHECK(lane_exact(pkt, len, h, 0, 0, NULL, 0).phase == 0);  // the same phase
        CHECK(lane_exact(pkt, len, h, 0, 3, NULL, 1).phase == 0);  // current slot empty
        CHECK(lane_exact(pkt, len, h, 0, 9, NULL, 1).phase == 0);  // current slot past the table
        // a long header never flips, whatever bit 2 says
        pkt[0] |= 0x80;
        CHECK(lane_exact(pkt, len, h, 0, 0, NULL, 1).phase == 0);
    }
    // the header bound: QPP_MAX_HDR - 4 acts, one more does not
    {
        const uint32_t big = qpp_ph::kMaxHdr + 40;
        uint8_t *p = (uint8_t *)calloc(big, 1);
        if (!p) abort();
        uint8_t m[16];
        xor_mask(0, 0, p + (qpp_ph::kMaxHdr - 4) + 4, m);
        p[0] = (uint8_t)(0x44 ^ (m[0] & 0x1f));
        CHECK(lane_exact(p, qpp_ph::kMaxHdr - 4 + 20, (uint16_t)(qpp_ph::kMaxHdr - 4), 0, 0, NULL, 1).phase == 1);
        CHECK(lane_exact(p, qpp_ph::kMaxHdr - 3 + 20, (uint16_t)(qpp_ph::kMaxHdr - 3), 0, 0, NULL, 1).phase == 0);
        free(p);
    }
    if (failures) return 1;
    printf("phase_host: ok\n");
    return 0;
}
