/* The in-order receive rule of the binding's walks, once: CryptoPair.decrypt_packet's
 * sequential semantics (quic/crypto.py:184-192) with the expected-number update of
 * connection.py:984-985 and the reserved-bit close of :949-960, over the results of a
 * launch that decoded every packet against the state the batch began with.
 * results_walk (unprotect_walk, walk_results) and short_walk (receive_short and the
 * receive_routed forms) in _crypto_ext.c fetch one packet's facts from their arrays,
 * call rxwalk_step, and turn its verdict into Python objects.
 * Plain C11, no Python and no HIP: tests/rxwalk_host.c runs it as a program. */
#pragma once

#include <stdint.h>

#include "quic_pp.h"

/* Host-side outcomes of the receive walks (never produced by a kernel):
 * a packet that authenticated with a reserved bit set (connection.py:949-960),
 * a packet of a connection the walk has closed (:756-757). */
#define WALK_S_RESERVED 0x101
#define WALK_S_CLOSED 0x102
#define WALK_NO_CONN 0xffffffffu
#define RXWALK_NO_PHASE (-1)

/* decode_packet_number (quic/packet.py:118-132) of the truncated number as
 * HeaderProtection.remove hands it over: a signed C int (_crypto.c:349), so a
 * 4-byte value >= 2^31 enters negative, exactly as the Python walk sees it.
 * Returns -1 where Python would produce a negative number. */
static int64_t decode_pn_signed(uint64_t pn, int pn_len, uint64_t expected)
{
    const int bits = 8 * pn_len;
    int64_t trunc = (int64_t)(pn & ((1ull << bits) - 1));
    if (pn_len == 4 && trunc >= ((int64_t)1 << 31)) trunc -= (int64_t)1 << 32;
    const int64_t window = (int64_t)1 << bits, half = window / 2, exp = (int64_t)expected;
    const int64_t cand = (exp & ~(window - 1)) | trunc;
    int64_t r;
    if (cand <= exp - half && cand < ((int64_t)1 << 62) - window) r = cand + window;
    else if (cand > exp + half && cand >= window) r = cand - window;
    else r = cand;
    return r < 0 ? -1 : r;
}

/* What a walk has changed so far.  A deferred packet blocks what it might still
 * change: whatever follows it there waits for the caller's general path too. */
typedef struct {
    uint64_t *sx;     /* expected packet number per space */
    uint8_t *closed;  /* per connection */
    uint8_t *blocked_pair, *blocked_space, *blocked_conn;
    uint8_t *rolled;  /* per pair: a packet of the batch has rolled its keys; NULL: phases are not resolved */
} RxWalkState;

/* One packet's facts, in batch order. */
typedef struct {
    uint32_t pair, space;
    uint32_t conn;     /* WALK_NO_CONN: none */
    int launched;      /* 0: nothing ran for it (closed on entry, or no receive key); what follows is unused then */
    uint16_t status;   /* QPP_S_* of its result */
    uint16_t hdr_len;  /* of its result */
    uint64_t pn;       /* of its result */
    uint32_t pn_off;   /* the offset the launch was given */
    uint64_t exp;      /* the expected number the launch decoded against */
    uint8_t rsv_mask;  /* reserved bits of the first byte; 0: no check */
    uint8_t first;     /* first output byte of a success (0 when it has no header byte) */
    uint8_t track;     /* a success advances its space */
    int phase;         /* the device's verdict: 1 ran on the next phase's slot, 0 on the current one's; or
                          RXWALK_NO_PHASE */
} RxWalkPacket;

typedef enum {
    RXW_DEFERRED,  /* the caller's general path takes it, in order, from the state left here */
    RXW_CLOSED,    /* its connection is closed (connection.py:756-757) */
    RXW_NO_KEY,    /* no receive key (crypto.py:78-79) */
    RXW_RESERVED,  /* authenticated with a reserved bit set: closes its connection, advances nothing */
    RXW_OK,
    RXW_FAILED,    /* with the packet's status */
} RxWalkVerdict;

static RxWalkVerdict rxwalk_step(RxWalkState *s, const RxWalkPacket *k)
{
    const uint32_t p = k->pair, sp = k->space, c = k->conn;
    const int has_conn = c != WALK_NO_CONN, phased = s->rolled && k->phase != RXWALK_NO_PHASE;
    /* a deferred packet of the connection may close it: wait for it */
    int defer = has_conn && s->blocked_conn[c];
    if (k->launched && (s->blocked_pair[p] || s->blocked_space[sp])) defer = 1;
    /* a closed connection's packets are dropped whatever their keys or numbers say */
    if (!defer && has_conn && s->closed[c]) return RXW_CLOSED;
    const uint64_t now = s->sx[sp];
    if (!defer && k->launched) {
        if (k->status == QPP_S_KEY_PHASE) {
            defer = 1; /* a key roll follows */
        } else if (phased && s->rolled[p] && !k->phase) {
            /* the pair has rolled and this packet ran on the slot of the phase before: the general
               path's, as a flip is (it tries the phase after next and fails, crypto.py:91-96) */
            defer = 1;
        } else if (now != k->exp && (k->status == QPP_S_OK || k->status == QPP_S_DECRYPT)) {
            /* its truncated number decodes differently under the expected number by now */
            const int pn_len = (int)k->hdr_len - (int)k->pn_off;
            if (pn_len < 1 || pn_len > 4 || decode_pn_signed(k->pn, pn_len, now) != (int64_t)k->pn) defer = 1;
        }
    }
    if (defer) {
        if (has_conn) s->blocked_conn[c] = 1;
        if (k->launched) s->blocked_pair[p] = s->blocked_space[sp] = 1;
        return RXW_DEFERRED;
    }
    if (!k->launched || k->status == QPP_S_NO_KEY) return RXW_NO_KEY;
    /* a packet of the next phase that authenticates updates the keys inside decrypt_packet
       (crypto.py:184-192), before the reserved bits are looked at (connection.py:949-960) */
    if (phased && k->phase && k->status == QPP_S_OK) s->rolled[p] = 1;
    if (k->status != QPP_S_OK) return RXW_FAILED;
    if (k->first & k->rsv_mask) {
        /* connection.py:949-960: close, end, no expected-number update */
        if (has_conn) s->closed[c] = 1;
        return RXW_RESERVED;
    }
    if (k->track && k->pn > now) s->sx[sp] = k->pn + 1; /* connection.py:984-985 */
    return RXW_OK;
}
