// Host build of aioquic_amd/csrc/qpp_send.h for tests/test_send_host.py: what
// every lane of k_send runs.  Plain g++, no HIP.
//
// Built as a shared object, sn_lane is one lane of the kernel in its order --
// the connection's record, its slot's suite and phase, decide(), emit() -- over
// host memory, and sn_batch_ok the fused form's host check.  Built as a
// program (with -fsanitize=address,undefined), main() runs sn_lane over heap
// buffers of exactly the packet's region, so that a store before the header's
// first byte or behind the tag's room is the sanitizer's to report.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../aioquic_amd/csrc/qpp_send.h"

using qpp_sn::Conn;
using qpp_sn::Desc;
using qpp_sn::Rec;
using qpp_sn::Slot;

extern "C" {

// Lane i of k_send over host memory.  slots[cap]: suite (qpp_sn::kSuiteEmpty:
// never installed) and phase per key slot.  Returns the record's status.
uint32_t sn_lane(const Slot *slots, uint32_t cap, const Conn *conns, uint32_t n_conn, const uint64_t *off,
                 const uint32_t *len, const uint32_t *conn, const uint32_t *seq, uint32_t i, uint8_t *buf,
                 uint64_t buf_len, Desc *desc, Rec *rec)
{
    const uint32_t ci = conn[i];
    const bool conn_ok = ci < n_conn;
    Conn c;
    memset(&c, 0, sizeof c);
    Slot s = {qpp_sn::kSuiteEmpty, 0};
    if (conn_ok) {
        c = conns[ci];
        if (c.slot < cap) s = slots[c.slot];
    }
    const qpp_sn::Plan p = qpp_sn::decide(conn_ok, c, s, off[i], len[i], seq[i], buf_len);
    qpp_sn::emit(p, c, off[i], len[i], buf, desc + i, rec + i);
    return rec[i].status;
}

uint32_t sn_batch_ok(const Conn *conns, uint32_t n_conn, uint32_t cap, const uint64_t *off, const uint32_t *len,
                     const uint32_t *conn, uint32_t n, uint64_t in_len, uint64_t out_len)
{
    return qpp_sn::batch_ok(conns, n_conn, cap, off, len, conn, n, in_len, out_len);
}

uint32_t sn_const(uint32_t which)
{
    const uint32_t v[] = {qpp_sn::kPnLen, qpp_sn::kHead, qpp_sn::kTail, qpp_sn::kPadMax,
                          (uint32_t)sizeof(Conn), (uint32_t)sizeof(Rec)};
    return which < sizeof v / sizeof v[0] ? v[which] : 0xffffffffu;
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

// slots 0 / 1: suite 0, phases 0 / 1; 2: suite 2, phase 1; 3: empty
const Slot kSlots[4] = {{0, 0}, {0, 1}, {2, 1}, {qpp_sn::kSuiteEmpty, 0}};

Conn make_conn(uint64_t next_pn, uint32_t slot, uint8_t cid_len, uint8_t spin)
{
    Conn c;
    memset(&c, 0, sizeof c);
    c.next_pn = next_pn;
    c.slot = slot;
    c.cid_len = cid_len;
    c.spin = spin;
    for (int k = 0; k < 20; ++k) c.cid[k] = k < cid_len ? (uint8_t)(0xa0 + k) : 0;
    return c;
}

struct Run {
    uint32_t status;
    bool untouched;  // no byte of the buffer changed
    bool exact;      // header, payload, padding as expected; nothing else changed
    Desc d;
    Rec r;
};

// One lane over a heap buffer of exactly [head bytes | payload | tail bytes]:
// the payload lies at p_off = head, the buffer ends at p_off + len + tail.
Run lane_exact(const Conn &c, uint32_t conn_ix, uint32_t len, uint32_t seq, uint32_t head, uint32_t tail)
{
    const size_t size = (size_t)head + len + tail;
    uint8_t *p = (uint8_t *)malloc(size ? size : 1), *before = (uint8_t *)malloc(size ? size : 1);
    if (!p || !before) abort();
    for (size_t k = 0; k < size; ++k) p[k] = (uint8_t)(0x11 + 7 * k);
    memcpy(before, p, size);
    const uint64_t off[1] = {head};
    const uint32_t ln[1] = {len}, cn[1] = {conn_ix}, sq[1] = {seq};
    Run r;
    memset(&r.d, 0xab, sizeof r.d);
    memset(&r.r, 0xab, sizeof r.r);
    uint8_t *q = size ? p : p + 1;  // an empty buffer's one allocated byte must not be touched either
    r.status = sn_lane(kSlots, 4, &c, 1, off, ln, cn, sq, 0, q, size, &r.d, &r.r);
    r.untouched = memcmp(before, p, size) == 0;
    r.exact = false;
    if (r.status == qpp_sn::kOk) {
        const uint32_t hl = 1u + c.cid_len + 2u, pad = len < 2 ? 2 - len : 0;
        const uint64_t pn = c.next_pn + seq;
        uint8_t *want = before;
        uint8_t *h = want + head - hl;
        h[0] = (uint8_t)(0x40 | (c.spin ? 0x20 : 0) | (kSlots[c.slot].key_phase << 2) | 1);
        memcpy(h + 1, c.cid, c.cid_len);
        h[1 + c.cid_len] = (uint8_t)(pn >> 8);
        h[2 + c.cid_len] = (uint8_t)pn;
        memset(want + head + len, 0, pad);
        r.exact = memcmp(want, p, size) == 0 && r.d.in_off == head - hl && r.d.out_off == head - hl &&
                  r.d.len == len + pad && r.d.hdr_len == hl && r.d.flags == 0 && r.d.pn == pn && r.d.slot == c.slot &&
                  r.d.rsv == 0 && r.r.pn == pn && r.r.hdr_len == hl;
    } else {
        r.exact = r.untouched && r.d.in_off == head && r.d.out_off == head && r.d.len == 0 && r.d.hdr_len == 0 &&
                  r.d.flags == 0 && r.d.pn == 0 && r.d.slot == qpp_sn::kSlotNone && r.d.rsv == 0 && r.r.pn == 0 &&
                  r.r.hdr_len == 0;
    }
    for (int k = 0; k < 5; ++k) r.exact = r.exact && r.r.rsv[k] == 0;
    free(p);
    free(before);
    return r;
}

}  // namespace

int main()
{
    for (uint8_t cid_len : {(uint8_t)0, (uint8_t)1, (uint8_t)8, (uint8_t)20}) {
        const uint32_t hl = 1u + cid_len + 2u;
        for (uint32_t len : {1u, 2u, 3u, 40u, 1173u}) {
            const uint32_t pad = len < 2 ? 2 - len : 0, need = pad + 16;
            for (uint32_t slot = 0; slot < 3; ++slot) {
                const Conn c = make_conn(0xfffe, slot, cid_len, (uint8_t)(slot & 1));
                // a region of exactly the header, the payload, the padding and the tag's room
                for (uint32_t seq = 0; seq < 4; ++seq) {
                    Run r = lane_exact(c, 0, len, seq, hl, need);
                    CHECK(r.status == qpp_sn::kOk && r.exact);
                }
                // every truncation of the room in front: nothing is written
                for (uint32_t head = 0; head < hl; ++head) {
                    Run r = lane_exact(c, 0, len, 0, head, need);
                    CHECK(r.status == qpp_sn::kRoom && r.exact);
                }
                // and of the room behind
                for (uint32_t tail = 0; tail < need; ++tail) {
                    Run r = lane_exact(c, 0, len, 0, hl, tail);
                    CHECK(r.status == qpp_sn::kRoom && r.exact);
                }
                // more room than needed changes nothing
                Run r = lane_exact(c, 0, len, 1, qpp_sn::kHead, qpp_sn::kTail);
                CHECK(r.status == qpp_sn::kOk && r.exact);
            }
        }
    }
    // each other condition failing alone, over a region that would do
    {
        const uint32_t head = qpp_sn::kHead, tail = qpp_sn::kTail;
        CHECK(lane_exact(make_conn(5, 0, 8, 0), 0, 30, 0, head, tail).status == qpp_sn::kOk);
        Run r = lane_exact(make_conn(5, 0, 8, 0), 1, 30, 0, head, tail);  // conn >= n_conn
        CHECK(r.status == qpp_sn::kConn && r.exact);
        r = lane_exact(make_conn(5, 0, 8, 0), 0xffffffffu, 30, 0, head, tail);
        CHECK(r.status == qpp_sn::kConn && r.exact);
        CHECK(lane_exact(make_conn(5, 0, 20, 0), 0, 30, 0, head, tail).status == qpp_sn::kOk);
        r = lane_exact(make_conn(5, 0, 21, 0), 0, 30, 0, head + 1, tail);
        CHECK(r.status == qpp_sn::kCid && r.exact);
        r = lane_exact(make_conn(5, 0, 255, 0), 0, 30, 0, head, tail);
        CHECK(r.status == qpp_sn::kCid && r.exact);
        for (uint32_t slot : {3u, 4u, 1000u, qpp_sn::kSlotNone}) {  // empty, past the table, none
            r = lane_exact(make_conn(5, slot, 8, 0), 0, 30, 0, head, tail);
            CHECK(r.status == qpp_sn::kNoKey && r.exact);
        }
        r = lane_exact(make_conn(5, 0, 8, 0), 0, 0, 0, head, tail);
        CHECK(r.status == qpp_sn::kEmpty && r.exact);
        CHECK(lane_exact(make_conn(qpp_sn::kPnLimit - 1, 0, 8, 0), 0, 30, 0, head, tail).status == qpp_sn::kOk);
        CHECK(lane_exact(make_conn(qpp_sn::kPnLimit - 2, 0, 8, 0), 0, 30, 1, head, tail).status == qpp_sn::kOk);
        r = lane_exact(make_conn(qpp_sn::kPnLimit, 0, 8, 0), 0, 30, 0, head, tail);
        CHECK(r.status == qpp_sn::kPn && r.exact);
        r = lane_exact(make_conn(qpp_sn::kPnLimit - 1, 0, 8, 0), 0, 30, 1, head, tail);
        CHECK(r.status == qpp_sn::kPn && r.exact);
        r = lane_exact(make_conn(~0ull, 0, 8, 0), 0, 30, 1, head, tail);  // the sum wraps to 0
        CHECK(r.status == qpp_sn::kPn && r.exact);
        r = lane_exact(make_conn(~0ull - 5, 0, 8, 0), 0, 30, 0xffffffffu, head, tail);
        CHECK(r.status == qpp_sn::kPn && r.exact);
        // the first failing check names the status
        r = lane_exact(make_conn(~0ull, 3, 21, 0), 0, 0, 1, 0, 0);
        CHECK(r.status == qpp_sn::kCid && r.exact);
        r = lane_exact(make_conn(~0ull, 3, 20, 0), 0, 0, 1, 0, 0);
        CHECK(r.status == qpp_sn::kNoKey && r.exact);
        r = lane_exact(make_conn(~0ull, 0, 20, 0), 0, 0, 1, 0, 0);
        CHECK(r.status == qpp_sn::kEmpty && r.exact);
        r = lane_exact(make_conn(~0ull, 0, 20, 0), 0, 1, 1, 0, 0);
        CHECK(r.status == qpp_sn::kPn && r.exact);
    }
    // offsets and lengths at the ends of their types never reach the buffer
    {
        const Conn c = make_conn(5, 0, 8, 0);
        uint8_t one[1] = {0x5a};
        Desc d;
        Rec rc;
        for (uint64_t off : {~0ull, ~0ull - 10, 1ull << 63, 2ull}) {
            for (uint32_t len : {1u, 0xffffffffu, 0xfffffff0u}) {
                const uint64_t o[1] = {off};
                const uint32_t l[1] = {len}, z[1] = {0};
                CHECK(sn_lane(kSlots, 4, &c, 1, o, l, z, z, 0, one, 1, &d, &rc) == qpp_sn::kRoom && one[0] == 0x5a);
            }
        }
    }
    if (failures) return 1;
    printf("send_host: ok\n");
    return 0;
}
