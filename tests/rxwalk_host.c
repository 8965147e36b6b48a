/* The in-order receive rule of aioquic_amd/csrc/qpp_rxwalk.h, run as a program:
 *   gcc -std=c11 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover -I include -I aioquic_amd/csrc
 *       -o rxwalk_host tests/rxwalk_host.c && ./rxwalk_host
 * A table of named scenarios, one per rule of the header, each a handful of packets whose
 * verdicts and final state are written out by hand from the rule's text; then, over seeded
 * inputs both of the binding's walks can express (every packet launched and of a connection,
 * every success tracked, mask 0x18, no phases), the way results_walk states a packet's facts
 * and the way short_walk does must give the same verdicts and the same final state.
 * Every array is a heap block of exactly its size, so a stray index is an error here. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qpp_rxwalk.h"

#define NP 4 /* pairs, spaces and connections of a scenario */
#define MAXPK 8
#define OK QPP_S_OK
#define DEC QPP_S_DECRYPT
#define LEN QPP_S_LENGTH
#define KPH QPP_S_KEY_PHASE
#define NOKEY QPP_S_NO_KEY
#define NONE WALK_NO_CONN
#define NOPH RXWALK_NO_PHASE

typedef struct {
    RxWalkPacket k;
    RxWalkVerdict want;
} Step;

typedef struct {
    const char *name;
    uint64_t sx0;           /* every space's expected number on entry */
    uint8_t closed0[NP];
    int phased;             /* the state has a rolled array */
    int n;
    Step s[MAXPK];
    uint64_t sx[NP];        /* the state afterwards */
    uint8_t closed[NP], bpair[NP], bspace[NP], bconn[NP], rolled[NP];
} Scenario;

/* a launched packet: pair, space, conn, status, pn, hdr_len, pn_off, exp, mask, first byte, track, phase */
#define L(p, sp, c, st, num, hl, po, ex, mk, fb, tr, ph) \
    {.pair = p, .space = sp, .conn = c, .launched = 1, .status = st, .pn = num, .hdr_len = hl, .pn_off = po, .exp = ex, \
     .rsv_mask = mk, .first = fb, .track = tr, .phase = ph}
/* a record nothing was launched for: only short_walk has them */
#define U(p, sp, c) {.pair = p, .space = sp, .conn = c, .launched = 0, .rsv_mask = 0x18, .track = 1, .phase = NOPH}
/* the usual short-header packet of pair = space = conn = x: a 1-byte number after 5 header bytes */
#define S1(x, st, num, ex) L(x, x, x, st, num, 6, 5, ex, 0x18, 0x40, 1, NOPH)

static const Scenario kScenarios[] = {
    {"a success above the expected number advances its space; one equal to it does not",
     10, {0}, 0, 3,
     {{S1(0, OK, 11, 10), RXW_OK},    /* 11 > 10: expected becomes 12 */
      {S1(0, OK, 12, 10), RXW_OK},    /* now 12 != exp 10, but 12 decodes to 12 under 12; 12 > 12 is false */
      {S1(1, OK, 10, 10), RXW_OK}},   /* pn == now: no advance */
     {12, 10, 10, 10}, {0}, {0}, {0}, {0}, {0}},
    {"an untracked success advances nothing",
     10, {0}, 0, 2,
     {{L(0, 0, 0, OK, 50, 6, 5, 10, 0x18, 0x40, 0, NOPH), RXW_OK},
      {L(0, 0, NONE, OK, 60, 6, 5, 10, 0x18, 0x40, 1, NOPH), RXW_OK}}, /* no connection: still advances */
     {61, 10, 10, 10}, {0}, {0}, {0}, {0}, {0}},
    {"a key-phase flip is deferred and blocks its pair, space and connection",
     10, {0}, 0, 6,
     {{S1(0, KPH, 11, 10), RXW_DEFERRED},
      {L(0, 1, 1, OK, 11, 6, 5, 10, 0x18, 0x40, 1, NOPH), RXW_DEFERRED},    /* its pair; blocks space 1, conn 1 */
      {L(1, 0, 2, OK, 11, 6, 5, 10, 0x18, 0x40, 1, NOPH), RXW_DEFERRED},    /* its space; blocks pair 1, conn 2 */
      {L(2, 2, 0, OK, 11, 6, 5, 10, 0x18, 0x40, 1, NOPH), RXW_DEFERRED},    /* its connection; blocks pair 2, space 2 */
      {S1(3, OK, 11, 10), RXW_OK},
      {L(3, 1, NONE, OK, 13, 6, 5, 10, 0x18, 0x40, 1, NOPH), RXW_DEFERRED}}, /* space 1, no connection; blocks pair 3 */
     {10, 10, 10, 12}, {0}, {1, 1, 1, 1}, {1, 1, 1, 0}, {1, 1, 1, 0}, {0}},
    {"a number that decodes differently by now is deferred, for OK and DECRYPT alone",
     10, {0}, 0, 6,
     {{L(0, 0, 0, OK, 300, 7, 5, 10, 0x18, 0x40, 1, NOPH), RXW_OK},  /* 2 bytes: expected becomes 301 */
      {S1(0, LEN, 20, 10), RXW_FAILED},    /* not a status whose number is looked at */
      {S1(0, OK, 20, 10), RXW_DEFERRED},   /* 1 byte 0x14 under 301 is 276, not 20 */
      {L(1, 1, 1, OK, 300, 7, 5, 10, 0x18, 0x40, 1, NOPH), RXW_OK},
      {S1(1, DEC, 20, 10), RXW_DEFERRED},
      {S1(2, DEC, 20, 10), RXW_FAILED}},   /* now == exp: nothing to decode again */
     {301, 301, 10, 10}, {0}, {1, 1, 0, 0}, {1, 1, 0, 0}, {1, 1, 0, 0}, {0}},
    {"a number length outside 1..4 cannot be decoded again: deferred",
     10, {0}, 0, 3,
     {{S1(0, OK, 40, 10), RXW_OK},
      {L(0, 0, 0, OK, 40, 10, 5, 10, 0x18, 0x40, 1, NOPH), RXW_DEFERRED},   /* 5 bytes */
      {L(1, 1, 1, OK, 40, 5, 5, 10, 0x18, 0x40, 1, NOPH), RXW_OK}},         /* 0 bytes, but now == exp */
     {41, 41, 10, 10}, {0}, {1, 0, 0, 0}, {1, 0, 0, 0}, {1, 0, 0, 0}, {0}},
    {"closed on entry: dropped whatever its status, unless something of it is blocked",
     10, {1, 0, 0, 0}, 0, 5,
     {{L(0, 0, 0, KPH, 11, 6, 5, 10, 0x18, 0x40, 1, NOPH), RXW_CLOSED},  /* closed suppresses the flip's deferral */
      {L(0, 0, 0, OK, 11, 6, 5, 9, 0x18, 0x58, 1, NOPH), RXW_CLOSED},    /* and the re-decode, and the reserved bits */
      {S1(1, KPH, 11, 10), RXW_DEFERRED},
      {L(1, 2, 0, OK, 11, 6, 5, 10, 0x18, 0x40, 1, NOPH), RXW_DEFERRED}, /* closed, but its pair is blocked: blocked first */
      {L(3, 3, 0, OK, 11, 6, 5, 10, 0x18, 0x40, 1, NOPH), RXW_DEFERRED}},/* and now its connection is */
     {10, 10, 10, 10}, {1, 0, 0, 0}, {0, 1, 0, 1}, {0, 1, 1, 1}, {1, 1, 0, 0}, {0}},
    {"blocked, then a close that cannot be seen: the connection's later packets wait",
     10, {0}, 0, 3,
     {{L(0, 0, 0, KPH, 11, 6, 5, 10, 0x18, 0x40, 1, NOPH), RXW_DEFERRED},
      {L(1, 1, 0, OK, 11, 6, 5, 10, 0x18, 0x58, 1, NOPH), RXW_DEFERRED},  /* reserved bits set, but deferred: no close */
      {L(2, 2, 0, OK, 11, 6, 5, 10, 0x18, 0x40, 1, NOPH), RXW_DEFERRED}},
     {10, 10, 10, 10}, {0}, {1, 1, 1, 0}, {1, 1, 1, 0}, {1, 0, 0, 0}, {0}},
    {"reserved bits close the connection and advance nothing; the mask is the packet's",
     10, {0}, 0, 6,
     {{L(0, 0, 0, OK, 11, 6, 5, 10, 0x18, 0x48, 1, NOPH), RXW_RESERVED},
      {S1(0, OK, 11, 10), RXW_CLOSED},
      {L(1, 1, 1, OK, 11, 6, 5, 10, 0, 0x58, 1, NOPH), RXW_OK},              /* mask 0: no check */
      {L(2, 2, NONE, OK, 11, 6, 5, 10, 0x18, 0x50, 1, NOPH), RXW_RESERVED},  /* nothing to close */
      {L(2, 2, 2, OK, 11, 9, 5, 10, 0x0c, 0xc4, 1, NOPH), RXW_RESERVED},     /* a long header's mask */
      {L(3, 3, 3, DEC, 11, 6, 5, 10, 0x18, 0x58, 1, NOPH), RXW_FAILED}},     /* only a success is looked at */
     {10, 12, 10, 10}, {1, 0, 1, 0}, {0}, {0}, {0}, {0}},
    {"a launched packet without a key: deferred by, and blocking, pair, space and connection",
     10, {0}, 0, 4,
     {{S1(0, NOKEY, 0, 10), RXW_NO_KEY},
      {S1(1, KPH, 11, 10), RXW_DEFERRED},
      {L(1, 2, 2, NOKEY, 0, 6, 5, 10, 0x18, 0, 1, NOPH), RXW_DEFERRED}, /* its pair is blocked */
      {L(3, 3, 2, OK, 11, 6, 5, 10, 0x18, 0x40, 1, NOPH), RXW_DEFERRED}},/* so connection 2 is now */
     {10, 10, 10, 10}, {0}, {0, 1, 0, 1}, {0, 1, 1, 1}, {0, 1, 1, 0}, {0}},
    {"a record nothing was launched for waits for its connection alone, and blocks it alone",
     10, {0, 0, 0, 1}, 0, 6,
     {{S1(0, KPH, 11, 10), RXW_DEFERRED},
      {U(0, 0, 1), RXW_NO_KEY},     /* pair 0 and space 0 are blocked: no matter */
      {U(1, 1, 0), RXW_DEFERRED},   /* connection 0 is; pair 1 and space 1 stay free */
      {S1(1, OK, 11, 10), RXW_OK},
      {U(2, 2, 3), RXW_CLOSED},     /* closed on entry */
      {U(2, 2, 2), RXW_NO_KEY}},
     {10, 12, 10, 10}, {0, 0, 0, 1}, {1, 0, 0, 0}, {1, 0, 0, 0}, {1, 0, 0, 0}, {0}},
    {"a next-phase packet that authenticates rolls its pair; the old slot's packets then wait",
     10, {0}, 1, 5,
     {{L(0, 0, 0, OK, 11, 6, 5, 10, 0x18, 0x40, 1, 0), RXW_OK},        /* before the roll: the current slot is right */
      {L(1, 1, 1, DEC, 11, 6, 5, 10, 0x18, 0x40, 1, 1), RXW_FAILED},   /* failed its tag: rolls nothing */
      {L(1, 1, 1, OK, 11, 6, 5, 10, 0x18, 0x40, 1, 0), RXW_OK},
      {L(0, 0, 0, OK, 13, 6, 5, 10, 0x18, 0x44, 1, 1), RXW_OK},        /* rolls pair 0; expected becomes 14 */
      {L(0, 0, 0, OK, 14, 6, 5, 10, 0x18, 0x40, 1, 0), RXW_DEFERRED}}, /* ran on the phase before */
     {14, 12, 10, 10}, {0}, {1, 0, 0, 0}, {1, 0, 0, 0}, {1, 0, 0, 0}, {1, 0, 0, 0}},
    {"the roll comes before the reserved bits; a closed connection's old-slot packet is dropped, not deferred",
     10, {0}, 1, 3,
     {{L(0, 0, 0, OK, 11, 6, 5, 10, 0x18, 0x4c, 1, 1), RXW_RESERVED},  /* rolled, then closed */
      {L(0, 0, 0, OK, 12, 6, 5, 10, 0x18, 0x40, 1, 0), RXW_CLOSED},
      {L(0, 1, 1, OK, 12, 6, 5, 10, 0x18, 0x40, 1, 0), RXW_DEFERRED}}, /* the pair's other connection: open, so it waits */
     {10, 10, 10, 10}, {1, 0, 0, 0}, {1, 0, 0, 0}, {0, 1, 0, 0}, {0, 1, 0, 0}, {1, 0, 0, 0}},
    {"without the device's verdicts nothing rolls and nothing waits for a roll",
     10, {0}, 1, 2,
     {{L(0, 0, 0, OK, 11, 6, 5, 10, 0x18, 0x40, 1, NOPH), RXW_OK},
      {L(0, 0, 0, OK, 13, 6, 5, 10, 0x18, 0x40, 1, NOPH), RXW_OK}},
     {14, 10, 10, 10}, {0}, {0}, {0}, {0}, {0}},
    {"a 4-byte number at or above 2^31 enters the decode as a negative int",
     0x180000020ull, {0}, 0, 4,
     {{S1(0, OK, 0x180000025ull, 0x180000020ull), RXW_OK},  /* expected becomes 0x180000026 */
      /* 0x80000010 handed over signed is -0x7ffffff0: the candidate is negative, a window is added: 0x80000010 again */
      {L(0, 0, 0, OK, 0x80000010ull, 9, 5, 0x180000020ull, 0x18, 0x40, 1, NOPH), RXW_OK},
      /* the unsigned decode's 0x180000010 is not what Python computes by now */
      {L(1, 1, 1, OK, 0x180000021ull, 6, 5, 0x180000020ull, 0x18, 0x40, 1, NOPH), RXW_OK},
      {L(1, 1, 1, OK, 0x180000010ull, 9, 5, 0x180000020ull, 0x18, 0x40, 1, NOPH), RXW_DEFERRED}},
     {0x180000026ull, 0x180000022ull, 0x180000020ull, 0x180000020ull}, {0}, {0, 1, 0, 0}, {0, 1, 0, 0}, {0, 1, 0, 0}, {0}},
};

static const char *const kVerdict[] = {"deferred", "closed", "no key", "reserved", "ok", "failed"};

static void *dup_bytes(const void *src, size_t n)
{
    void *p = malloc(n);
    if (!p) abort();
    if (src) memcpy(p, src, n);
    else memset(p, 0, n);
    return p;
}

static RxWalkState state_new(size_t n_pairs, size_t n_spaces, size_t n_conns, uint64_t sx0, const uint8_t *closed,
                             int phased)
{
    RxWalkState st = {dup_bytes(NULL, n_spaces * sizeof(uint64_t)), dup_bytes(closed, n_conns),
                      dup_bytes(NULL, n_pairs), dup_bytes(NULL, n_spaces), dup_bytes(NULL, n_conns),
                      phased ? dup_bytes(NULL, n_pairs) : NULL};
    for (size_t s = 0; s < n_spaces; ++s) st.sx[s] = sx0;
    return st;
}

static void state_free(RxWalkState *st)
{
    free(st->sx), free(st->closed), free(st->blocked_pair), free(st->blocked_space), free(st->blocked_conn);
    free(st->rolled);
}

static int same(const char *name, const char *what, const uint8_t *got, const uint8_t *want, size_t n)
{
    if (!memcmp(got, want, n)) return 0;
    printf("FAIL %s: %s is", name, what);
    for (size_t i = 0; i < n; ++i) printf(" %u", got[i]);
    printf("\n");
    return 1;
}

static int run_scenario(const Scenario *sc)
{
    int bad = 0;
    RxWalkState st = state_new(NP, NP, NP, sc->sx0, sc->closed0, sc->phased);
    for (int i = 0; i < sc->n; ++i) {
        const RxWalkVerdict v = rxwalk_step(&st, &sc->s[i].k);
        if (v != sc->s[i].want) {
            printf("FAIL %s: packet %d is %s, not %s\n", sc->name, i, kVerdict[v], kVerdict[sc->s[i].want]);
            bad = 1;
        }
    }
    for (int s = 0; s < NP; ++s)
        if (st.sx[s] != sc->sx[s]) {
            printf("FAIL %s: space %d expects %llu\n", sc->name, s, (unsigned long long)st.sx[s]);
            bad = 1;
        }
    bad |= same(sc->name, "closed", st.closed, sc->closed, NP);
    bad |= same(sc->name, "blocked_pair", st.blocked_pair, sc->bpair, NP);
    bad |= same(sc->name, "blocked_space", st.blocked_space, sc->bspace, NP);
    bad |= same(sc->name, "blocked_conn", st.blocked_conn, sc->bconn, NP);
    if (sc->phased) bad |= same(sc->name, "rolled", st.rolled, sc->rolled, NP);
    state_free(&st);
    return bad;
}

/* ---- the common domain, stated the way each of the binding's walks states it ---- */

static uint64_t rng_state;
static uint32_t rnd(uint32_t n)
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((rng_state >> 33) % n);
}

enum { CN = 48, CC = 5 }; /* packets and connections (= pairs = spaces) of a seeded case */

typedef struct {
    uint32_t conn[CN], off[CN];
    uint64_t exp[CN], pn[CN];
    uint16_t status[CN], hdr_len[CN];
    uint8_t first[CN], closed0[CC];
} Common;

static void common_case(Common *c, uint64_t seed)
{
    static const uint16_t kStatus[10] = {OK, OK, OK, OK, OK, OK, OK, DEC, KPH, NOKEY};
    static const uint64_t kStep[8] = {0, 1, 1, 1, 2, 2, 200, 40000};
    rng_state = seed;
    uint64_t at[CC];
    for (int k = 0; k < CC; ++k) at[k] = 1000, c->closed0[k] = rnd(12) == 0;
    for (int i = 0; i < CN; ++i) {
        const uint32_t k = c->conn[i] = rnd(CC);
        const int pn_len = 1 + (int)rnd(4);
        at[k] += kStep[rnd(8)];
        c->off[i] = 1 + rnd(20);
        c->hdr_len[i] = (uint16_t)(c->off[i] + (uint32_t)pn_len);
        c->exp[i] = 1000;
        c->pn[i] = (uint64_t)decode_pn_signed(at[k], pn_len, 1000); /* what the launch reports */
        c->status[i] = kStatus[rnd(10)];
        c->first[i] = (uint8_t)(0x40 | (rnd(25) == 0 ? 0x08 : 0) | rnd(8));
    }
}

/* results_walk: per-packet pair, space, conn, track and mask arrays; a keyless packet is a launched NO_KEY one */
static void walk_results_way(const Common *c, RxWalkState *st, RxWalkVerdict *v)
{
    uint32_t *pair = dup_bytes(c->conn, sizeof c->conn), *space = dup_bytes(c->conn, sizeof c->conn);
    uint8_t *track = dup_bytes(NULL, CN), *rsv = dup_bytes(NULL, CN);
    memset(track, 1, CN), memset(rsv, 0x18, CN);
    for (int i = 0; i < CN; ++i) {
        RxWalkPacket k = {.pair = pair[i], .space = space[i], .conn = c->conn[i], .launched = 1,
                          .status = c->status[i], .hdr_len = c->hdr_len[i], .pn = c->pn[i], .pn_off = c->off[i],
                          .exp = c->exp[i], .rsv_mask = rsv[i], .track = track[i], .phase = RXWALK_NO_PHASE};
        if (k.status == QPP_S_OK && k.hdr_len) k.first = c->first[i];
        v[i] = rxwalk_step(st, &k);
    }
    free(pair), free(space), free(track), free(rsv);
}

/* short_walk: pair and space through the connection, offset and expected number from the descriptor */
static void walk_short_way(const Common *c, RxWalkState *st, RxWalkVerdict *v)
{
    uint32_t *cpair = dup_bytes(NULL, CC * sizeof(uint32_t)), *cspace = dup_bytes(NULL, CC * sizeof(uint32_t));
    for (uint32_t k = 0; k < CC; ++k) cpair[k] = cspace[k] = k;
    for (int i = 0; i < CN; ++i) {
        const uint32_t cn = c->conn[i];
        RxWalkPacket k = {.pair = cpair[cn], .space = cspace[cn], .conn = cn, .launched = 1, .rsv_mask = 0x18,
                          .track = 1, .phase = RXWALK_NO_PHASE};
        k.status = c->status[i], k.hdr_len = c->hdr_len[i], k.pn = c->pn[i];
        k.pn_off = (uint16_t)c->off[i], k.exp = c->exp[i];
        if (k.status == QPP_S_OK) k.first = c->first[i];
        v[i] = rxwalk_step(st, &k);
    }
    free(cpair), free(cspace);
}

static int run_common(uint64_t seed, unsigned *seen)
{
    Common *c = dup_bytes(NULL, sizeof *c);
    common_case(c, seed);
    RxWalkState a = state_new(CC, CC, CC, 1000, c->closed0, 0), b = state_new(CC, CC, CC, 1000, c->closed0, 0);
    RxWalkVerdict *va = dup_bytes(NULL, CN * sizeof *va), *vb = dup_bytes(NULL, CN * sizeof *vb);
    walk_results_way(c, &a, va);
    walk_short_way(c, &b, vb);
    int bad = memcmp(va, vb, CN * sizeof *va) != 0 || memcmp(a.sx, b.sx, CC * sizeof(uint64_t)) != 0 ||
              memcmp(a.closed, b.closed, CC) != 0 || memcmp(a.blocked_pair, b.blocked_pair, CC) != 0 ||
              memcmp(a.blocked_space, b.blocked_space, CC) != 0 || memcmp(a.blocked_conn, b.blocked_conn, CC) != 0;
    if (bad) printf("FAIL common domain, seed %llu: the two ways differ\n", (unsigned long long)seed);
    for (int i = 0; i < CN; ++i) seen[va[i]]++;
    free(va), free(vb), free(c);
    state_free(&a), state_free(&b);
    return bad;
}

int main(void)
{
    int bad = 0;
    const int ns = (int)(sizeof kScenarios / sizeof kScenarios[0]);
    for (int i = 0; i < ns; ++i) bad |= run_scenario(&kScenarios[i]);
    unsigned seen[6] = {0};
    for (uint64_t seed = 1; seed <= 400; ++seed) bad |= run_common(seed, seen);
    for (int v = 0; v < 6; ++v)
        if (!seen[v]) {
            printf("FAIL common domain: no packet was %s\n", kVerdict[v]);
            bad = 1;
        }
    printf("%s: %d scenarios, 400 seeded cases (deferred %u closed %u no-key %u reserved %u ok %u failed %u)\n",
           bad ? "FAILED" : "ok", ns, seen[0], seen[1], seen[2], seen[3], seen[4], seen[5]);
    return bad;
}
