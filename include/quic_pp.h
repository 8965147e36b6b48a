/*
 * quic_pp.h -- C ABI of the MI355X QUIC packet-protection engine (libquicpp.so).
 *
 * This is the drop-in boundary for aioquic's per-packet protection path.  The
 * reference binds that path as a CPython extension, aioquic._crypto
 * (src/aioquic/_crypto.c, API stub src/aioquic/_crypto.pyi:1-15), called from
 * src/aioquic/quic/crypto.py:4.  Each entry point below names the reference
 * function(s) it replaces.  Plain pointers and sizes only: no HIP, torch or
 * Python types cross this boundary (streams are passed as void*, i.e. a
 * hipStream_t; NULL = the null stream).
 *
 * Threading: a qpp_keytab may be shared between threads for launches; setting
 * keys and launching on the same slots concurrently is the caller's race (as
 * with the reference's per-object scratch, _crypto.c:39-42).  A qpp_session and
 * a qpp_plan are single-threaded: use one per thread (the CPython binding
 * keeps one session per OS thread).
 *
 * Buffers: the device-pointer launches (qpp_protect, qpp_unprotect and the
 * planned forms) cannot see buffer sizes, so every descriptor's input and
 * output extents must lie inside the caller's allocations; the buffers
 * themselves may be of any size.  A packet's input extent is hdr_len + len
 * bytes at in_off for protect and len bytes for unprotect; its output extent
 * is hdr_len + len + QPP_TAG_LEN bytes at out_off for protect and
 * len - QPP_TAG_LEN bytes for unprotect.  The kernels that run 16 packets per
 * wavefront (an "item": 16 consecutive descriptors, or up to 16 consecutive
 * in a plan's bucket order) address an item through 32-bit views based at its
 * lowest offsets, so for every packet of an item
 *     (offset - lowest offset in the item) + extent <= QPP_ITEM_SPAN_MAX,
 * separately for input and output.  A packet beyond that gets QPP_S_LENGTH
 * and nothing of it is written; the item's other packets are not affected.
 * Launches that run one packet per wavefront (small unplanned launches) have
 * no such limit.  The session forms check every descriptor against in_len /
 * out_len and report QPP_S_LENGTH for one that does not fit, without touching
 * memory for it.
 *
 * Authentication failures: unprotect decrypts as it authenticates, so the
 * plaintext of a packet whose tag does not verify is produced before the
 * verdict.  The kernels then overwrite that packet's payload region at
 * out_off + hdr_len with zeros (out_len = 0), so no unauthenticated plaintext
 * is left in the output.  An in-place unprotect (in == out) of a forged
 * packet therefore also destroys its ciphertext, as the reference's copy-out
 * semantics never do (_crypto.c:145-154 returns an error, not bytes).
 */
#ifndef QUIC_PP_H
#define QUIC_PP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QPP_ABI_VERSION 3

/* cipher suites (quic/crypto.py:12-16 CIPHER_SUITES) */
#define QPP_AES_128_GCM 0        /* aes-128-gcm + aes-128-ecb header protection */
#define QPP_AES_256_GCM 1        /* aes-256-gcm + aes-256-ecb header protection */
#define QPP_CHACHA20_POLY1305 2  /* chacha20-poly1305 + chacha20 header protection */

#define QPP_PACKET_MAX 1500      /* _crypto.c:13 PACKET_LENGTH_MAX */
#define QPP_TAG_LEN 16           /* _crypto.c:11 AEAD_TAG_LENGTH */
#define QPP_MAX_HDR 1500         /* longest header / associated data the kernels accept */
#define QPP_ITEM_SPAN_MAX 0xffffff00u /* bytes one 16-packet item may span (see Buffers above) */

/* return codes of the API calls */
#define QPP_OK 0
#define QPP_E_ARG (-1)           /* bad argument (NULL, n too large, bad slot) */
#define QPP_E_HIP (-2)           /* a HIP runtime call failed */
#define QPP_E_NODEV (-3)         /* no usable gfx950 device */
#define QPP_E_NOMEM (-4)

/* per-packet status codes (qpp_result.status) */
#define QPP_S_OK 0
#define QPP_S_LENGTH 1      /* "Invalid payload length" (_crypto.c:126-129,168-171) or sample out of range */
#define QPP_S_DECRYPT 2     /* "Payload decryption failed" (_crypto.c:148-152) */
#define QPP_S_KEY_PHASE 3   /* short header whose key-phase bit differs from the slot's
                               (quic/crypto.py:91-96): caller retries with the next-phase key,
                               unless qpp_route_phase pointed the descriptor at it beforehand */
#define QPP_S_NO_KEY 4      /* slot never installed: KeyUnavailableError (quic/crypto.py:78-79) */
#define QPP_S_INTERNAL 5    /* the engine gave up on the packet: a bounded wait inside a kernel
                               (a GHASH table entry, a two-wave hand-over) ran out.  Nothing at
                               out_off is valid (unprotect: no plaintext is left there), and the
                               call raises CryptoError, as a failed reference call does
                               (_crypto.c:17-29).  Never expected; counted by qpp_watchdog_count */

/* descriptor flags */
#define QPP_F_NO_HP 1u      /* AEAD only (AEAD.encrypt/.decrypt): no header protection, no
                               packet-number decode, no key-phase check; hdr_len = AAD length */
#define QPP_F_RFC_PN 2u     /* decode a 4-byte truncated packet number as unsigned (RFC 9000
                               App. A.3).  Default: bit-exact with the reference, which hands
                               the truncated number to Python as a signed int (_crypto.c:349),
                               so values >= 2^31 decode differently once pn >= 2^32. */

/* One packet of a batch.  Offsets are byte offsets into the caller's device
 * buffers; no alignment is required. */
typedef struct qpp_desc {
    uint64_t in_off;   /* protect: header then payload; unprotect: the protected packet */
    uint64_t out_off;  /* protect: header||ciphertext||tag; unprotect: header||plaintext */
    uint32_t len;      /* protect: payload length; unprotect: packet length (>= pn_off + 20) */
    uint16_t hdr_len;  /* protect: header (= AAD) length; unprotect: packet-number offset
                          ("encrypted_offset"), or the AAD length with QPP_F_NO_HP */
    uint16_t flags;    /* QPP_F_* */
    uint64_t pn;       /* protect: packet number; unprotect: expected packet number,
                          or the exact packet number with QPP_F_NO_HP */
    uint32_t slot;     /* key-table slot */
    uint32_t rsv;
} qpp_desc;            /* 40 bytes */

typedef struct qpp_result {
    uint64_t pn;       /* unprotect: decoded packet number; protect: pn used */
    uint16_t status;   /* QPP_S_* */
    uint16_t hdr_len;  /* plain header length (pn_off + pn_len for unprotect) */
    uint32_t out_len;  /* bytes written at out_off */
} qpp_result;          /* 16 bytes */

/* Raw key material for one slot, as produced by derive_key_iv_hp
 * (quic/crypto.py:34-56).  key/hp use 16 bytes for AES-128, 32 otherwise. */
typedef struct qpp_key_material {
    uint32_t slot;
    uint8_t suite;      /* QPP_AES_128_GCM / QPP_AES_256_GCM / QPP_CHACHA20_POLY1305 */
    uint8_t key_phase;  /* 0/1, compared with bit 2 of a short header */
    uint8_t rsv[2];
    uint8_t iv[12];
    uint8_t key[32];
    uint8_t hp[32];
} qpp_key_material;     /* 84 bytes */

/* One connection's traffic secret for the batched key schedule (qpp_keytab_derive). */
#define QPP_DERIVE_V2 1u    /* QUIC v2 labels "quicv2 key/iv/hp" (quic/crypto.py:52-56) */

typedef struct qpp_secret {
    uint32_t slot;
    uint8_t suite;       /* QPP_AES_128_GCM (SHA-256) / QPP_AES_256_GCM (SHA-384) /
                            QPP_CHACHA20_POLY1305 (SHA-256), tls.py:1108-1112 */
    uint8_t key_phase;
    uint8_t flags;       /* QPP_DERIVE_* */
    uint8_t secret_len;  /* bytes of secret[] used: 1..64 */
    uint32_t updates;    /* key updates applied first: secret = HKDF-Expand-Label(secret,
                            "quic ku", "", hash_len) per step (next_key_phase,
                            quic/crypto.py:157-168; the label is "quic ku" for v2 too) */
    uint32_t rsv;
    uint8_t secret[64];
} qpp_secret;            /* 80 bytes */

/* One connection's Initial keys for the batched CryptoPair.setup_initial
 * (qpp_keytab_derive_initial): the destination connection ID the keys come
 * from and the slots of the two directions. */
#define QPP_SLOT_NONE 0xffffffffu   /* derive_initial: do not install this direction */
#define QPP_CID_MAX 20              /* RFC 9000 sec. 17.2 */

typedef struct qpp_initial {
    uint32_t slot_client;  /* slot for the "client in" keys (a client sends with them, a
                              server receives with them), or QPP_SLOT_NONE */
    uint32_t slot_server;  /* slot for the "server in" keys, or QPP_SLOT_NONE */
    uint8_t cid_len;       /* 0..QPP_CID_MAX */
    uint8_t flags;         /* QPP_DERIVE_V2: the v2 salt and the "quicv2 key/iv/hp" labels */
    uint8_t rsv[2];
    uint8_t cid[20];
} qpp_initial;             /* 32 bytes */

/* One context's current traffic secret for the batched next_key_phase
 * (qpp_keytab_derive_next): what a key update derives from, the
 * header-protection key it keeps, and where the next phase goes. */
typedef struct qpp_next_phase {
    uint32_t slot;        /* slot to install the next phase in, or QPP_SLOT_NONE: derive and return only */
    uint8_t  suite;
    uint8_t  key_phase;   /* the NEXT phase's bit (the caller flips it) */
    uint8_t  flags;       /* QPP_DERIVE_V2 */
    uint8_t  secret_len;  /* 1..64, as qpp_secret */
    uint8_t  secret[64];  /* the CURRENT phase's traffic secret */
    uint8_t  hp[32];      /* the current header-protection key, kept */
} qpp_next_phase;         /* 104 bytes */

typedef struct qpp_keytab qpp_keytab;   /* device-resident expanded keys */
typedef struct qpp_session qpp_session; /* pinned staging + device buffers + stream */

/* library / device */
int qpp_abi_version(void);
/* 16 hex digits: the hash of the native sources the library was built from
 * (aioquic_amd/_srchash.py); a binding checks it against its own at load. */
const char *qpp_source_hash(void);
/* Watchdog events on the current device since the library loaded: a launch
 * whose kernel waited ~1 s for a GHASH table entry (that key slot's packets),
 * or a two-wave packet whose hand-over timed out, reported QPP_S_INTERNAL
 * for the packets concerned.  Never expected
 * (it would be a bug); tests check it stays 0.  A synchronous read. */
uint32_t qpp_watchdog_count(void);
/* Single-key AES-GCM launches (process-wide, since the library loaded) that
 * found all of their key table's launch-pool slots held by launches still in
 * flight and so ran without the launch-wide item pool (static shares only;
 * the same bytes, a possibly longer tail).  Diagnostic. */
uint64_t qpp_pool_fallbacks(void);
/* AES-GCM launches (process-wide, since the library loaded) that ran the
 * kernel form whose closing GHASH multiplies read an LDS copy of the key's
 * tables: unplanned 1024-thread launches with one key of the suite in the
 * table.  The same bytes as the other form.  Diagnostic. */
uint64_t qpp_close_lds_launches(void);
const char *qpp_strerror(int rc);
int qpp_device_check(void);             /* QPP_OK if the current device is gfx950 */

/* Key tables.  qpp_keytab_set replaces AEAD_init (_crypto.c:68-102) and
 * HeaderProtection_init (_crypto.c:232-266): one device launch expands AES
 * round keys, H = E_K(0^128) and the GHASH tables for every slot in km. */
int qpp_keytab_create(uint32_t capacity, qpp_keytab **out);
/* Every launch that uses the table must have completed (its stream
 * synchronized) before the table is destroyed. */
void qpp_keytab_destroy(qpp_keytab *kt);
uint32_t qpp_keytab_capacity(const qpp_keytab *kt);
int qpp_keytab_set(qpp_keytab *kt, const qpp_key_material *km, uint32_t n, void *stream);
int qpp_keytab_clear(qpp_keytab *kt, const uint32_t *slots, uint32_t n, void *stream);
/* Batched CryptoContext.setup (quic/crypto.py:121-136) for n connections at once:
 * derive_key_iv_hp (quic/crypto.py:34-56 = HKDF-Expand-Label, tls.py:164-185)
 * on the device, one lane per secret, after `updates` key updates, then the same
 * slot expansion as qpp_keytab_set.  km_out (host memory, may be NULL) receives
 * the derived key material, e.g. for the host-side AEAD objects. */
int qpp_keytab_derive(qpp_keytab *kt, const qpp_secret *sec, uint32_t n,
                      qpp_key_material *km_out, void *stream);
/* Batched CryptoPair.setup_initial (quic/crypto.py:201-227) for n connections
 * at once, e.g. every new connection of a receive batch, once per supported
 * version as the reference's loop does (quic/connection.py:1509-1515).  Per
 * record, on the device, two lanes per connection:
 *     root     = HMAC-SHA256(salt, cid)            salt = INITIAL_SALT_VERSION_1, or
 *                                                  _2 with QPP_DERIVE_V2
 *     secret_x = HKDF-Expand-Label(root, "client in" | "server in", "", 32)
 *     key(16) / iv(12) / hp(16) of secret_x with the "quic " labels, or the
 *                                                  "quicv2 " ones with QPP_DERIVE_V2
 * always as QPP_AES_128_GCM with key_phase 0.  Each direction whose slot is
 * not QPP_SLOT_NONE is then installed with the same slot expansion as
 * qpp_keytab_set.  km_out (host memory, may be NULL) receives 2n records:
 * [2i] the client direction of record i, [2i + 1] its server direction; a
 * direction given QPP_SLOT_NONE is derived and returned all the same, with
 * slot = QPP_SLOT_NONE, only not installed.  secrets_out (host memory, may be
 * NULL) receives the 2n x 32 bytes of the "client in" / "server in" secrets in
 * the same order (CryptoContext.secret).  km_out feeds qpp_multi_set_keys
 * unchanged.
 * QPP_E_ARG, with nothing installed: NULL kt, NULL ini with n > 0, n > 2^24, a
 * slot that is neither < capacity nor QPP_SLOT_NONE, cid_len > QPP_CID_MAX, a
 * flag bit other than QPP_DERIVE_V2, or slot_client == slot_server (unless
 * both are QPP_SLOT_NONE).  The same slot named by two different records is
 * the caller's race, as with qpp_keytab_set.  n == 0 returns QPP_OK.
 * Synchronous, like qpp_keytab_derive: the records are caller memory. */
int qpp_keytab_derive_initial(qpp_keytab *kt, const qpp_initial *ini, uint32_t n,
                              qpp_key_material *km_out, uint8_t *secrets_out, void *stream);
/* qpp_keytab_derive_initial over n records that already lie in device memory
 * (d_ini, e.g. written by qpp_route_accept earlier on the same stream).
 * Asynchronous on `stream`: no allocation and no synchronisation inside.  It
 * launches the same two kernels as qpp_keytab_derive_initial, the derivation
 * and then the slot expansion, with the same grids.  d_km (2n
 * qpp_key_material) and d_secrets (2n x 32 bytes) are caller-owned device
 * buffers that receive what km_out / secrets_out receive there, in the same
 * order; both are required.
 * The host cannot know which records the device will install, so h_slots[2n]
 * (host memory) lists the slots the records may name, QPP_SLOT_NONE entries
 * skipped.  Every listed slot is noted as QPP_AES_128_GCM in the table's host
 * bookkeeping before the launch.  Listing a slot that no record installs (an
 * over-count) only makes a later launch choose the general AES-GCM kernel
 * form over the single-key forms; the general form is correct for any number
 * of keys.  Not listing a slot that a record installs (an under-count) is not
 * safe.  The caller clears the listed slots that were not installed with
 * qpp_keytab_clear afterwards, which also takes them out of the bookkeeping.
 * QPP_E_ARG, with nothing launched or noted: NULL kt, a NULL array with n > 0,
 * n > 2^24, a listed slot >= capacity that is not QPP_SLOT_NONE, the same
 * slot listed twice.  n == 0 returns QPP_OK.  The records' own fields are the
 * device's: a slot >= capacity in one is skipped by the slot expansion, a
 * cid_len > QPP_CID_MAX is the caller's to rule out (qpp_route_accept never
 * writes one).  The timing of qpp_keytab_derive_trace does not cover this
 * call. */
int qpp_keytab_derive_initial_device(qpp_keytab *kt, const qpp_initial *d_ini, uint32_t n,
                                     const uint32_t *h_slots, qpp_key_material *d_km, uint8_t *d_secrets,
                                     void *stream);
/* Batched next_key_phase (quic/crypto.py:148-168) for n contexts at once: the
 * keys a key update moves to, derived from the current traffic secrets on the
 * device, one lane per record, in one launch:
 *     secret' = HKDF-Expand-Label(secret, "quic ku", "", hl)   hl = 48 for QPP_AES_256_GCM
 *                                                              (SHA-384), else 32 (SHA-256);
 *                                                              "quic ku" with QPP_DERIVE_V2 too
 *     key(klen) / iv(12) of secret' with the "quic " labels, or the "quicv2 " ones
 *                                                              with QPP_DERIVE_V2
 *     hp      = the record's first klen bytes: a key update keeps the
 *               header-protection key (deriving "quic hp" from secret', as
 *               qpp_keytab_derive with updates = 1 does, gives the wrong key)
 * Each record whose slot is not QPP_SLOT_NONE is then installed with the same
 * slot expansion as qpp_keytab_set, under the record's key_phase.  km_out
 * (host memory, may be NULL) receives n records, key and hp zero past klen; a
 * record given QPP_SLOT_NONE is derived and returned all the same, with slot =
 * QPP_SLOT_NONE, only not installed (the send direction of a key update).
 * secrets_out (host memory, may be NULL) receives n x 64 bytes: secret', zero
 * past hl (CryptoContext.secret of the next phase).
 * QPP_E_ARG, with nothing launched, noted or installed: NULL kt, NULL rec with
 * n > 0, n > 2^24, a slot that is neither < capacity nor QPP_SLOT_NONE, a
 * suite above QPP_CHACHA20_POLY1305, secret_len outside 1..64, key_phase > 1,
 * a flag bit other than QPP_DERIVE_V2.  The same slot named by two records is
 * the caller's race, as with qpp_keytab_set.  n == 0 returns QPP_OK.
 * Synchronous, like qpp_keytab_derive: the records are caller memory. */
int qpp_keytab_derive_next(qpp_keytab *kt, const qpp_next_phase *rec, uint32_t n,
                           qpp_key_material *km_out, uint8_t *secrets_out, void *stream);
/* Where the device time of a qpp_keytab_derive_initial or
 * qpp_keytab_derive_next call goes (diagnostic, for
 * tools/bench_initial_keys.py and tools/bench_next_keys.py): enable != 0 makes
 * the table's following calls put timing events around their two kernels (0
 * off, -1 unchanged); derive_ms and setup_ms (may be NULL) receive the last
 * timed call's durations of the derivation kernel and of the slot expansion
 * (0 before any). */
int qpp_keytab_derive_trace(qpp_keytab *kt, int enable, float *derive_ms, float *setup_ms);

/* Batched packet protection on device buffers (asynchronous on `stream`).
 * qpp_protect replaces AEAD_encrypt (_crypto.c:157-194) + HeaderProtection_apply
 * (_crypto.c:289-319), i.e. CryptoContext.encrypt_packet (quic/crypto.py:105-116).
 * qpp_unprotect replaces HeaderProtection_remove (_crypto.c:321-350) +
 * decode_packet_number (quic/packet.py:118-132) + AEAD_decrypt (_crypto.c:115-155),
 * i.e. CryptoContext.decrypt_packet (quic/crypto.py:75-103).
 * Packets with the same slot should be contiguous for speed (any order is correct). */
int qpp_protect(const qpp_keytab *kt, const qpp_desc *d_desc, uint32_t n, const uint8_t *d_in,
                uint8_t *d_out, qpp_result *d_res, void *stream);
int qpp_unprotect(const qpp_keytab *kt, const qpp_desc *d_desc, uint32_t n,
                  const uint8_t *d_in, uint8_t *d_out, qpp_result *d_res, void *stream);

/* Bucketing by (suite, key slot).  A server's batch interleaves many
 * connections (src/aioquic/asyncio/server.py:60-152 demultiplexes them per
 * datagram), but a kernel wants each workgroup on one key and one suite.
 * qpp_plan_build sorts the batch's packet indices on the device by
 * (suite, slot) and counts the packets of each suite; the order of the
 * packets within one (suite, slot) run is unspecified (results are mapped
 * back to the caller's order, so it is not observable).  A *_planned launch gathers its descriptors into that order, runs
 * each suite's kernel over its own bucket only, and writes every result at
 * the packet's position in the CALLER's descriptor order.  A plan is built
 * once per batch and serves every launch over descriptors with the same
 * slots in the same positions (e.g. protect, then unprotect of the same
 * packets).  Asynchronous on `stream`; a plan serves one stream at a time.
 * Empty or unknown slots are reported QPP_S_NO_KEY, as by qpp_protect. */
typedef struct qpp_plan qpp_plan;
int qpp_plan_create(uint32_t max_packets, qpp_plan **out);
void qpp_plan_destroy(qpp_plan *p);
int qpp_plan_build(qpp_plan *p, const qpp_keytab *kt, const qpp_desc *d_desc, uint32_t n,
                   void *stream);
int qpp_protect_planned(const qpp_keytab *kt, const qpp_plan *p, const qpp_desc *d_desc,
                        uint32_t n, const uint8_t *d_in, uint8_t *d_out, qpp_result *d_res,
                        void *stream);
int qpp_unprotect_planned(const qpp_keytab *kt, const qpp_plan *p, const qpp_desc *d_desc,
                          uint32_t n, const uint8_t *d_in, uint8_t *d_out, qpp_result *d_res,
                          void *stream);

/* Routing received datagrams to connections by connection ID, on the device.
 * Replaces the per-datagram routing of the reference's server
 * (src/aioquic/asyncio/server.py:60-152: pull_quic_header,
 * quic/packet.py:181-267, in Python, then
 * self._protocols.get(header.destination_cid)) and its CID bookkeeping
 * (server.py:154-170: _connection_id_issued / _connection_id_retired).
 *
 * A qpp_cidmap maps connection IDs of 1..QPP_CID_MAX bytes to the caller's
 * connection indices.  It is an open-addressing table of 32-byte buckets
 * (conn, cid_len, cid[20] zero-padded) with linear probing from
 * hash(cid_len, cid) & (buckets - 1), buckets = the power of two >= 2 x
 * capacity, at least 16.  The host keeps the authoritative mirror and alone
 * decides where an entry lives; put and remove change the mirror and then
 * scatter only the buckets they changed to the device copy (never the whole
 * table).  The device only reads the table, in qpp_route: no device-side
 * inserts, no atomics, no races.  A lookup stops at an empty bucket and is
 * bounded by `buckets` probes whatever the table holds.
 *
 * put = _connection_id_issued, remove = _connection_id_retired; a batched put
 * serves a burst of new connections.  Both are synchronous, like
 * qpp_keytab_derive: on return the device table is current for every later
 * launch (a launch still in flight on another stream is the caller's race).
 * Put of a CID already present replaces its conn; the last duplicate inside
 * one call wins.  Removing an absent CID is ignored; remove ignores conn.
 * Removal is by backward shift (no tombstones, never a rebuild): the entries
 * of the cluster behind the removed one move up, so after any sequence of
 * puts and removes every remaining CID is found.  One removal rewrites the
 * buckets of its own cluster only, an expected 1.5 at the table's maximum load
 * of 1/2, so a full table's worth of churn (capacity removes and capacity
 * puts) costs about 2.5 x capacity bucket writes on the host and as many
 * 32-byte stores on the device, spread over the calls that made them.
 * QPP_E_ARG with nothing changed, checked before the first change: NULL
 * arguments with n > 0, a cid_len of 0 or > QPP_CID_MAX, a put that would take
 * count past capacity (capacity itself: 1..2^22).  n == 0 returns QPP_OK.
 * A map is single-threaded for put / remove; launches only read it. */
#define QPP_CONN_NONE 0xffffffffu
typedef struct qpp_cid_entry {
    uint32_t conn;       /* caller's connection index */
    uint8_t cid_len;     /* 1..QPP_CID_MAX */
    uint8_t rsv[3];
    uint8_t cid[20];     /* bytes past cid_len are ignored */
    uint32_t rsv2;
} qpp_cid_entry;         /* 32 bytes */
typedef struct qpp_cidmap qpp_cidmap;
int qpp_cidmap_create(uint32_t capacity, qpp_cidmap **out);
/* Every launch that uses the map must have completed before it is destroyed. */
void qpp_cidmap_destroy(qpp_cidmap *m);
uint32_t qpp_cidmap_count(const qpp_cidmap *m);
int qpp_cidmap_put(qpp_cidmap *m, const qpp_cid_entry *e, uint32_t n, void *stream);
int qpp_cidmap_remove(qpp_cidmap *m, const qpp_cid_entry *e, uint32_t n, void *stream);
/* The host mirror's answer: the CID's conn, or QPP_CONN_NONE. */
uint32_t qpp_cidmap_find(const qpp_cidmap *m, const uint8_t *cid, uint32_t cid_len);
/* The CID's home bucket (diagnostic / test hook; QPP_CONN_NONE for a bad length). */
uint32_t qpp_cidmap_home(const qpp_cidmap *m, const uint8_t *cid, uint32_t cid_len);
uint32_t qpp_cidmap_buckets(const qpp_cidmap *m);

/* qpp_route: n raw datagrams (d_len[i] bytes at d_in + d_off[i], no alignment)
 * to qpp_unprotect-ready descriptors, one lane per datagram (asynchronous on
 * `stream`).  cid_len is the server's fixed host CID length
 * (configuration.connection_id_length), 1..QPP_CID_MAX, else QPP_E_ARG.  A lane
 * reads bytes [0, 1 + cid_len) of a short-header datagram and
 * [0, 6 + DCID length) of a long-header one, never a byte past its d_len[i].
 * Everything that changes per batch lives in two caller-owned device arrays
 * indexed by conn: d_conn_slot (the receive key slot or QPP_SLOT_NONE) and
 * d_conn_expected (the packet number space's expected packet number); the map
 * changes only when CIDs are issued or retired.
 *
 * d_route[i] = (conn, cls).  For QPP_R_SHORT, d_desc[i] = {in_off = out_off =
 * d_off[i], len = d_len[i], hdr_len = 1 + cid_len, flags = desc_flags, pn =
 * d_conn_expected[conn], slot = d_conn_slot[conn], rsv = 0}; a short packet
 * too short to unprotect is still routed and gets QPP_S_LENGTH from
 * qpp_unprotect as ever.  For every other class d_desc[i] = {in_off = out_off
 * = d_off[i], len = 0, hdr_len = 0, flags = desc_flags, pn = 0, slot =
 * QPP_SLOT_NONE, rsv = 0}: qpp_unprotect reports QPP_S_NO_KEY for it and
 * touches nothing, and its offsets keep its item's 32-bit views where its
 * neighbours are (Buffers, above).  d_desc may be NULL: only d_route is
 * written.  The descriptors feed qpp_plan_build + qpp_unprotect_planned, or
 * qpp_unprotect, unchanged. */
#define QPP_R_SHORT 0        /* short header, CID known: the descriptor is ready for qpp_unprotect */
#define QPP_R_LONG 1         /* long header (bit 7): conn = its DCID's connection or QPP_CONN_NONE;
                                the packets of the datagram are qpp_route_walk's, or the host walk's */
#define QPP_R_UNKNOWN_CID 2  /* short header, CID not in the map */
#define QPP_R_MALFORMED 3    /* empty; (b0 & 0xC0) == 0; short and len < 1 + cid_len; long and
                                len < 6, DCID length > 20 or len < 6 + DCID length */
#define QPP_R_BAD_CONN 4     /* the entry's conn >= n_conn (either header form): nothing of the
                                conn arrays was read; conn is the entry's */
typedef struct qpp_route_rec {
    uint32_t conn;           /* connection index, or QPP_CONN_NONE */
    uint8_t cls;             /* QPP_R_* */
    uint8_t rsv[3];
} qpp_route_rec;             /* 8 bytes */
int qpp_route(const qpp_cidmap *m, uint32_t cid_len, const uint64_t *d_off, const uint32_t *d_len,
              uint32_t n, const uint8_t *d_in, const uint32_t *d_conn_slot,
              const uint64_t *d_conn_expected, uint32_t n_conn, uint16_t desc_flags,
              qpp_desc *d_desc /* may be NULL */, qpp_route_rec *d_route, void *stream);

/* qpp_route_walk: the header walk of the long-header datagrams of a routed
 * batch on the device, in place of the host's per-datagram pull_quic_header
 * loop (quic/packet.py:181-267, connection.py:793-899).  Asynchronous on
 * `stream`; runs after qpp_route on the same stream, over the same datagram
 * arrays and the d_route (read only here) and d_desc that qpp_route wrote.
 * d_long_idx[n_long] names the datagrams to walk, strictly increasing and
 * < n (the caller's to guarantee for this device form; an index >= n is
 * skipped: no packets, zeroed records, inert extra descriptors).  One lane per listed datagram: lane r walks datagram i =
 * d_long_idx[r] and writes d_walk_n[r] = its packets found, at most
 * QPP_WALK_MAX, and one record d_walk[r * QPP_WALK_MAX + k] per packet k
 * (records past d_walk_n[r] are written as zeros).  A lane reads header bytes of its
 * datagram only, each after a check against d_len[i]: never a byte at or past
 * d_len[i], whatever the header's length fields claim.
 *
 * The walk of a datagram ends at its end (a short header, which is parsed at
 * any position but the first, Version Negotiation and Retry run to it), at a
 * header that does not parse (one QPP_W_PARSE record at that packet's offset,
 * the host walk's "header_parse_error") and at a QPP_W_HOST record: a header
 * whose pn_off is above QPP_MAX_HDR, or the fourth packet of a datagram that
 * holds a fifth.  QPP_W_HOST means "leave this datagram to the host walk".
 * A Version Negotiation packet is QPP_W_OK whatever follows its CIDs: its list
 * of versions is the host's to validate (pull_quic_header reads it in 4-byte
 * units and fails on a remainder; receive_routed records that as
 * header_parse_error, as the host walk does).
 *
 * Descriptors.  A datagram that qpp_route classed QPP_R_LONG with a
 * connection gets, for each QPP_W_OK packet of type Initial, 0-RTT, Handshake
 * or 1-RTT, {in_off = out_off = d_off[i] + off, len = the packet's length,
 * hdr_len = pn_off, flags = desc_flags, pn = d_conn_expected[conn *
 * QPP_SPACES + space], slot = d_conn_slot[conn * QPP_KEYSETS + key-set], rsv
 * = 0}, with QPP_SLOT_NONE for an Initial of a version that is neither 1 nor
 * 2.  Packet 0's descriptor replaces d_desc[i]; packet k >= 1 goes to
 * d_desc[n + 3 r + k - 1]; the record's desc is that index.  Every extra
 * entry d_desc[n + 3 r .. n + 3 r + 2] with no packet is written inert, as
 * qpp_route's are: len 0, QPP_SLOT_NONE, offsets d_off[i].  The placement is
 * fixed by (n, r, k) alone: no atomics, nothing to read back before the
 * unprotect launch over all n + 3 n_long descriptors (d_desc and the
 * results are the caller's to size for as many).  The extras of distant
 * datagrams share 16-packet items, so the QPP_ITEM_SPAN_MAX rule (Buffers,
 * above) applies to them: past it a packet reports QPP_S_LENGTH, harmlessly.
 * Version Negotiation and Retry packets, and every packet of a datagram with
 * no connection (QPP_CONN_NONE) or classed QPP_R_BAD_CONN, get records with
 * desc = QPP_DESC_NONE, and the conn arrays are not read for them.  A listed
 * datagram of any other class (not a long header) gets d_walk_n[r] = 0. */
#define QPP_WALK_MAX 4
#define QPP_KEYSETS 5   /* per connection: Initial v1, Initial v2, 0-RTT, Handshake, 1-RTT */
#define QPP_SPACES 3    /* Initial, Handshake, application (0-RTT and 1-RTT share it) */
#define QPP_DESC_NONE 0xffffffffu
#define QPP_W_OK 0      /* parsed; desc says whether a descriptor was written */
#define QPP_W_PARSE 1   /* header_parse_error here; the datagram ends */
#define QPP_W_HOST 2    /* more than QPP_WALK_MAX packets, or pn_off > QPP_MAX_HDR */
typedef struct qpp_walk_rec {
    uint32_t off;       /* packet start within the datagram */
    uint32_t len;       /* packet_length */
    uint32_t version;   /* 0: short header or Version Negotiation */
    uint32_t desc;      /* index into d_desc / d_res, or QPP_DESC_NONE */
    uint16_t pn_off;    /* encrypted offset from the packet start; 0 for VN and Retry */
    uint16_t token_len; /* an Initial's token length */
    uint8_t type;       /* QuicPacketType value 0..5 */
    uint8_t status;     /* QPP_W_* */
    uint8_t dcid_len, scid_len;
} qpp_walk_rec;         /* 24 bytes */
int qpp_route_walk(uint32_t cid_len, const uint64_t *d_off, const uint32_t *d_len, uint32_t n,
                   const uint8_t *d_in, const qpp_route_rec *d_route, const uint32_t *d_long_idx,
                   uint32_t n_long, const uint32_t *d_conn_slot /* n_conn x QPP_KEYSETS */,
                   const uint64_t *d_conn_expected /* n_conn x QPP_SPACES */, uint32_t n_conn,
                   uint16_t desc_flags, qpp_desc *d_desc /* n + 3 n_long */, qpp_walk_rec *d_walk,
                   uint32_t *d_walk_n, void *stream);
/* qpp_route_walk launches of the walking kernel (process-wide, since the
 * library loaded).  Diagnostic: an all-short batch makes none. */
uint64_t qpp_route_walk_launches(void);

/* qpp_route_accept: the unrouted Initials of a routed and walked batch that a
 * server may answer (asyncio/server.py:60-152, the checks it runs before it
 * creates a connection), with the record their Initial keys are derived from
 * and the descriptor their first packet is unprotected with.  Asynchronous
 * on `stream`; runs after qpp_route and qpp_route_walk on the same stream,
 * over the same datagram arrays and the d_route, d_long_idx, d_walk and
 * d_walk_n of those calls (all read only here) and their d_desc.
 * d_acc_row[n_acc] names the candidates: strictly increasing rows r <
 * n_long of the walk's listing, so the datagram is i = d_long_idx[r] (the
 * caller's to guarantee for this device form; a row >= n_long, or an index
 * >= n, reads nothing of the batch and is QPP_ACC_NOT_INITIAL).
 * d_acc_slot[2 n_acc] gives two key slots per candidate: [2a] for the "client
 * in" keys (the server's receive direction) and [2a + 1] for the "server in"
 * keys, which may be QPP_SLOT_NONE.  One lane per candidate.  Lane a accepts
 * its datagram if and only if all of these hold; the first that fails gives
 * d_acc[a].status:
 *   1. d_route[i] is (QPP_CONN_NONE, QPP_R_LONG)              QPP_ACC_ROUTED
 *   2. d_walk_n[r] >= 1 and packet 0's record is QPP_W_OK, of type Initial,
 *      at offset 0 (so not a parse error, QPP_W_HOST, Version Negotiation,
 *      Retry, or Handshake / 0-RTT to an unknown DCID)        QPP_ACC_NOT_INITIAL
 *   3. the version is 1 or 2 (version negotiation is the host's,
 *      server.py:71-84)                                       QPP_ACC_VERSION
 *   4. d_len[i] >= 1200 (server.py:91)                        QPP_ACC_SMALL
 *   5. 1 <= DCID length <= QPP_CID_MAX and 6 + DCID length <= d_len[i],
 *      checked here against d_len (a zero-length DCID cannot enter a
 *      qpp_cidmap and stays the host's)                       QPP_ACC_CID
 *   6. with QPP_A_NEED_TOKEN in accept_flags, token length > 0 (the server's
 *      Retry mode, server.py:95-111: an Initial without a token is answered
 *      with a Retry and needs no keys)                        QPP_ACC_NO_TOKEN
 * Accepted (QPP_ACC_OK): d_ini[a] = {slot_client = d_acc_slot[2a], slot_server
 * = d_acc_slot[2a + 1], cid_len, QPP_DERIVE_V2 for version 2, the DCID's bytes
 * from the datagram at [6, 6 + DCID length), zero padded}; d_desc[i] = {in_off
 * = out_off = d_off[i], len = the record's packet length, hdr_len = pn_off,
 * flags = desc_flags, pn = 0, slot = d_acc_slot[2a], rsv = 0}; d_acc[a] =
 * {desc = i, status, version = 0 for version 1 and 1 for version 2}.  Any
 * other verdict: d_ini[a] names no slot (both QPP_SLOT_NONE) and no CID
 * (cid_len 0, zero bytes), so qpp_keytab_derive_initial_device derives it and
 * installs nothing; d_desc is not touched, so the inert descriptor qpp_route
 * wrote stays; d_acc[a] = {QPP_DESC_NONE, status, 0}.  d_ini and d_acc are
 * written whole for every candidate: the same input gives the same bytes.
 * Only packet 0 of a datagram gets a descriptor here; the later packets of an
 * accepted datagram keep QPP_DESC_NONE in their walk records.  A lane reads
 * its own walk and route records, d_len[i] and the DCID's bytes: nothing at or
 * past d_len[i].
 * QPP_E_ARG: a NULL array with n_acc > 0, or an accept_flags bit other than
 * QPP_A_NEED_TOKEN.  n_acc == 0 returns QPP_OK and launches nothing. */
#define QPP_ACC_OK 0
#define QPP_ACC_ROUTED 1
#define QPP_ACC_NOT_INITIAL 2
#define QPP_ACC_VERSION 3
#define QPP_ACC_SMALL 4
#define QPP_ACC_CID 5
#define QPP_ACC_NO_TOKEN 6
#define QPP_A_NEED_TOKEN 1u
typedef struct qpp_accept_rec {
    uint32_t desc;       /* the datagram's index (= its packet 0's descriptor), or QPP_DESC_NONE */
    uint8_t status;      /* QPP_ACC_* */
    uint8_t version;     /* accepted: 0 for QUIC version 1, 1 for version 2 */
    uint8_t rsv[2];
} qpp_accept_rec;        /* 8 bytes */
int qpp_route_accept(const uint64_t *d_off, const uint32_t *d_len, uint32_t n, const uint8_t *d_in,
                     const qpp_route_rec *d_route, const uint32_t *d_long_idx, uint32_t n_long,
                     const qpp_walk_rec *d_walk, const uint32_t *d_walk_n, const uint32_t *d_acc_row,
                     const uint32_t *d_acc_slot, uint32_t n_acc, uint32_t accept_flags, uint16_t desc_flags,
                     qpp_initial *d_ini, qpp_desc *d_desc, qpp_accept_rec *d_acc, void *stream);
/* qpp_route_accept launches of the accepting kernel (process-wide, since the
 * library loaded).  Diagnostic: a batch without candidates makes none. */
uint64_t qpp_route_accept_launches(void);

/* qpp_route_token and qpp_route_accept_tokens: the Retry token a client sends
 * back in its second Initial, validated on the device before anything is
 * derived, installed or unprotected for it -- what the reference's server does
 * per datagram with validate_token before it creates a connection
 * (asyncio/server.py:112-120).  The token format is this server's own
 * (aioquic_amd/retry.py): counter (8 bytes, big-endian) | AES-128-GCM(P, aad =
 * counter, pn = counter) under slot 2 of the reply key table (qpp_route_reply),
 * with P the buffer of QuicRetryTokenHandler.create_token (quic/retry.py:25-28):
 * three one-byte-length opaques, the encoded address, the original DCID and
 * the Retry's source CID.  Three steps on one stream, after qpp_route and
 * qpp_route_walk and over their arrays:
 *   1. qpp_route_token: one lane per candidate of d_acc_row[n_acc] (as
 *      qpp_route_accept names them).  A lane whose candidate passes tests 1-6
 *      of qpp_route_accept with QPP_A_NEED_TOKEN set looks for the token of
 *      packet 0: with dl / sl / T the record's DCID, SCID and token lengths,
 *      QPP_TOKEN_MIN <= T <= QPP_TOKEN_MAX (else QPP_TK_LENGTH), then dl, sl <=
 *      20, 7 + dl + sl <= d_len[i], bytes 5 and 6 + dl of the datagram are dl
 *      and sl, the varint at 7 + dl + sl (any of its encodings) fits, equals T,
 *      and the T bytes after it end at or before d_len[i] (else QPP_TK_BOUNDS);
 *      every bound is held against d_len, not the record.  Then d_tokdesc[a] =
 *      {in_off = d_off[i] + the token's offset, out_off = a * QPP_TOKEN_STRIDE,
 *      len = T, hdr_len = 8, QPP_F_NO_HP, pn = the token's first 8 bytes
 *      big-endian, slot 2, rsv 0} and d_tokrec[a] = {QPP_TK_OK, zeros}.  Any
 *      other candidate gets the inert descriptor {in_off = d_off[i] (0 without
 *      a datagram), out_off = a * QPP_TOKEN_STRIDE, len 0, hdr_len 0,
 *      QPP_F_NO_HP, pn 0, QPP_SLOT_NONE} and {QPP_TK_NONE (no token test is
 *      due), QPP_TK_LENGTH or QPP_TK_BOUNDS, zeros}: its token is never
 *      decrypted.  Both records are written whole for every candidate.
 *   2. qpp_unprotect(reply_kt, d_tokdesc, n_acc, d_in, d_tok, d_tokres): d_tok
 *      holds QPP_TOKEN_STRIDE bytes per candidate, zeroed by the caller; an
 *      opened token leaves [counter | P] at a * 128, 8 + |P| <= 112.  The
 *      datagram buffer is only read: a token is part of its Initial's AAD.
 *   3. qpp_route_accept_tokens: qpp_route_accept with three more inputs
 *      (d_addr[20 n_acc] as qpp_route_reply takes it, d_tok, d_tokres) and
 *      d_tokrec, read and rewritten.  Tests 1-6 run unchanged; a candidate that
 *      passes them with QPP_A_NEED_TOKEN set then gets the token's verdict: its
 *      preliminary status if that is not QPP_TK_OK (QPP_TK_NONE included: a
 *      token nobody examined is not accepted); QPP_TK_AUTH unless
 *      d_tokres[a].status is QPP_S_OK, and no opened byte is read then; the
 *      three opaques parsed as validate_token does, trailing bytes allowed, a
 *      field that runs past the end or a CID field of more than 20 bytes
 *      QPP_TK_FORM; field 0 against d_addr[20a] = [alen | packed IP | port],
 *      in length and bytes (an alen that is neither 6 nor 18 matches nothing),
 *      QPP_TK_ADDR.  QPP_TK_OK: d_tokrec[a] = {QPP_TK_OK,
 *      the two CIDs}, and the candidate is accepted as by qpp_route_accept.
 *      Otherwise d_tokrec[a] = {verdict, zeros} and d_acc[a].status =
 *      QPP_ACC_BAD_TOKEN, written as any rejection is: d_ini[a] names no slot
 *      and no CID, desc = QPP_DESC_NONE, d_desc is left alone, so no keys are
 *      installed and nothing is unprotected.  A candidate that does not reach
 *      the token test gets {QPP_TK_NONE, zeros}.
 * Two deliberate divergences from the host's validate_token, neither of a
 * token this server issues (its largest is 8 + 19 + 21 + 21 + 16 = 85 bytes): a
 * CID field of more than 20 bytes is QPP_TK_FORM where the host returns it, and
 * a token of more than QPP_TOKEN_MAX bytes is QPP_TK_LENGTH where the host
 * would open one sealed with trailing bytes.
 * QPP_E_ARG: a NULL array with n_acc > 0, an accept_flags bit other than
 * QPP_A_NEED_TOKEN, n_acc > 2^24.  n_acc == 0 returns QPP_OK and launches
 * nothing. */
#define QPP_TOKEN_STRIDE 128
#define QPP_TOKEN_MIN 27    /* 8 + 3 + 16: the bound validate_token has */
#define QPP_TOKEN_MAX 128
#define QPP_ACC_BAD_TOKEN 7 /* from qpp_route_accept_tokens only: dropped silently (server.py:119-120) */
#define QPP_TK_OK 0
#define QPP_TK_NONE 1       /* no token test was due for this candidate */
#define QPP_TK_LENGTH 2     /* a token shorter than QPP_TOKEN_MIN or longer than QPP_TOKEN_MAX */
#define QPP_TK_BOUNDS 3     /* the walk record's lengths do not fit the datagram's bytes */
#define QPP_TK_AUTH 4       /* the token does not open under the token key */
#define QPP_TK_FORM 5       /* a field runs past the plaintext's end, or a CID field of more than 20 bytes */
#define QPP_TK_ADDR 6       /* sealed for another address */
typedef struct qpp_token_rec {
    uint8_t status;      /* QPP_TK_* */
    uint8_t odcid_len;   /* with QPP_TK_OK: the original DCID (the first flight's) */
    uint8_t rscid_len;   /*                 and the Retry's source CID */
    uint8_t rsv;
    uint8_t odcid[20];
    uint8_t rscid[20];
    uint8_t rsv2[4];
} qpp_token_rec;         /* 48 bytes */
int qpp_route_token(const uint64_t *d_off, const uint32_t *d_len, uint32_t n, const uint8_t *d_in,
                    const qpp_route_rec *d_route, const uint32_t *d_long_idx, uint32_t n_long,
                    const qpp_walk_rec *d_walk, const uint32_t *d_walk_n, const uint32_t *d_acc_row, uint32_t n_acc,
                    uint32_t accept_flags, qpp_desc *d_tokdesc, qpp_token_rec *d_tokrec, void *stream);
/* qpp_route_token launches of the locating kernel (process-wide, since the
 * library loaded).  Diagnostic: a call without candidates makes none. */
uint64_t qpp_route_token_launches(void);
/* Counted by qpp_route_accept_launches, as the accepting kernel it is. */
int qpp_route_accept_tokens(const uint64_t *d_off, const uint32_t *d_len, uint32_t n, const uint8_t *d_in,
                            const qpp_route_rec *d_route, const uint32_t *d_long_idx, uint32_t n_long,
                            const qpp_walk_rec *d_walk, const uint32_t *d_walk_n, const uint32_t *d_acc_row,
                            const uint32_t *d_acc_slot, uint32_t n_acc, uint32_t accept_flags, uint16_t desc_flags,
                            const uint8_t *d_addr, const uint8_t *d_tok, const qpp_result *d_tokres,
                            qpp_initial *d_ini, qpp_desc *d_desc, qpp_accept_rec *d_acc, qpp_token_rec *d_tokrec,
                            void *stream);

/* qpp_route_reply: the packets a server sends instead of accepting, for the
 * two verdicts of qpp_route_accept after which the reference's server sends
 * something and drops the datagram (asyncio/server.py:71-111): a Version
 * Negotiation packet for QPP_ACC_VERSION (encode_quic_version_negotiation,
 * quic/packet.py:317-334) and, in Retry mode, a Retry for QPP_ACC_NO_TOKEN
 * (encode_quic_retry, quic/packet.py:288-314, around a token whose plaintext
 * is the buffer of QuicRetryTokenHandler.create_token, quic/retry.py:25-28).
 * Asynchronous on `stream`; runs after qpp_route_accept on the same stream,
 * over the same datagram arrays, d_long_idx, d_walk, d_acc_row and the d_acc
 * that call wrote (all read only here).  One lane per candidate; no cipher
 * runs here.  Candidate a owns the QPP_REPLY_STRIDE bytes at a * 256 of
 * d_reply (256-byte aligned memory), d_seal[a], d_tag[a] and d_rec[a]; all are
 * written whole for every candidate, the region zero filled first, so the same
 * input gives the same bytes.
 * With dl / sl the DCID / SCID lengths of packet 0's walk record, a lane that
 * owes a reply first checks dl <= 20, sl <= 20 and 7 + dl + sl <= d_len[i]
 * against d_len, then that bytes 5 and 6 + dl of the datagram are dl and sl;
 * a failure gives {kind none, QPP_RP_BOUNDS}.  It reads the datagram's bytes
 * [5, 7 + dl + sl) and nothing else of it.
 *   QPP_ACC_VERSION with QPP_RP_VN in reply_flags: the region holds [0x80 |
 *   (d_rand[16a + 8] & 0x7f), four zero bytes, sl, the client's SCID, dl, its
 *   DCID (dl may be 0), versions[0 .. n_versions) big-endian]; d_rec[a] =
 *   {256a, 7 + sl + dl + 4 n_versions, QPP_RP_KIND_VN, QPP_RP_OK}.
 *   QPP_ACC_NO_TOKEN with QPP_RP_RETRY: the region holds the pseudo-packet of
 *   RFC 9001 sec. 5.8 from offset 0: [dl, the client's DCID], then at pkt = 1 +
 *   dl the Retry packet [0xF0 (version 1) or 0xC0 (version 2), the version,
 *   sl, the client's SCID, 8, d_rand[16a .. 16a + 8) as the new source CID],
 *   then at tok = pkt + 7 + sl + 8 the token: ctr = token_ctr + a as 8
 *   big-endian bytes, the plaintext P = [alen, address, dl, DCID, 8, the new
 *   source CID] with alen = d_addr[20a] (6 or 18, else {none, QPP_RP_ADDR})
 *   and the address the alen bytes after it (the packed IP, then the port
 *   big-endian: encode_address), and 16 zero bytes for the seal's tag; T = 8 +
 *   |P| + 16.  d_seal[a] = {in_off = out_off = 256a + tok, len = |P|, hdr_len
 *   = 8, QPP_F_NO_HP, pn = ctr, slot 2}; d_tag[a] = {in_off = out_off = 256a,
 *   len = 0, hdr_len = tok + T, QPP_F_NO_HP, pn = 0, slot 0 for version 1 and
 *   1 for version 2}; d_rec[a] = {256a + pkt, 7 + sl + 8 + T + 16,
 *   QPP_RP_KIND_RETRY, QPP_RP_OK}.  tok + T <= 129, and the integrity tag ends
 *   at 145 at the most.
 *   Anything else: d_rec[a] = {256a, 0, QPP_RP_KIND_NONE, status}.
 * Every candidate without a Retry gets two inert descriptors, as qpp_route
 * writes them: len 0, QPP_SLOT_NONE, both offsets 256a.
 * The caller then runs qpp_protect(reply_kt, d_seal, n_acc, d_reply, d_reply,
 * ...) and, after it on the same stream, the same over d_tag: the first seals
 * every token in place, the second appends every Retry integrity tag
 * (get_retry_integrity_tag, quic/packet.py:135-159).  reply_kt is a key table
 * of its own by this convention, which nothing enforces: slot 0 the Retry key
 * and nonce of RFC 9001 sec. 5.8, slot 1 those of RFC 9369 sec. 3.3.3, slot 2
 * the server's own token key and IV, all QPP_AES_128_GCM.  No (key, nonce)
 * pair of slot 2 may repeat: the caller never hands out a counter twice.
 * versions[n_versions] is host memory, read before the call returns.
 * QPP_E_ARG: a NULL array with n_acc > 0 (d_addr may be NULL without
 * QPP_RP_RETRY), a reply_flags bit other than QPP_RP_VN | QPP_RP_RETRY,
 * n_versions outside 1..QPP_RP_MAX_VERSIONS, or NULL versions.  n_acc == 0
 * returns QPP_OK and launches nothing. */
#define QPP_REPLY_STRIDE 256
#define QPP_RP_MAX_VERSIONS 16
#define QPP_RP_ADDR_STRIDE 20
#define QPP_RP_RAND_STRIDE 16
#define QPP_RP_VN 1u
#define QPP_RP_RETRY 2u
#define QPP_RP_KIND_NONE 0
#define QPP_RP_KIND_VN 1
#define QPP_RP_KIND_RETRY 2
#define QPP_RP_OK 0
#define QPP_RP_BOUNDS 0x40  /* the walk record's CID lengths do not fit the datagram */
#define QPP_RP_ADDR 0x41    /* an address length that is neither 6 nor 18 */
typedef struct qpp_reply_rec {
    uint32_t off;        /* of the packet to send, in the reply buffer */
    uint16_t len;        /* its length, or 0 */
    uint8_t kind;        /* QPP_RP_KIND_* */
    uint8_t status;      /* QPP_RP_OK, QPP_RP_BOUNDS, QPP_RP_ADDR; from the session form also the
                            QPP_S_* of a Retry's failed seal or tag, its kind then QPP_RP_KIND_NONE */
} qpp_reply_rec;         /* 8 bytes */
int qpp_route_reply(const uint64_t *d_off, const uint32_t *d_len, uint32_t n, const uint8_t *d_in,
                    const uint32_t *d_long_idx, uint32_t n_long, const qpp_walk_rec *d_walk,
                    const uint32_t *d_acc_row, const qpp_accept_rec *d_acc, uint32_t n_acc, const uint8_t *d_addr,
                    const uint8_t *d_rand, uint64_t token_ctr, const uint32_t *versions, uint32_t n_versions,
                    uint32_t reply_flags, uint8_t *d_reply, qpp_desc *d_seal, qpp_desc *d_tag, qpp_reply_rec *d_rec,
                    void *stream);
/* qpp_route_reply launches of the assembling kernel (process-wide, since the
 * library loaded).  Diagnostic: a call without candidates makes none. */
uint64_t qpp_route_reply_launches(void);

/* qpp_route_phase: a peer's key update (quic/crypto.py:91-96, :184-192)
 * resolved on the device ahead of the unprotect.  Asynchronous on `stream`;
 * runs after qpp_route (and qpp_route_walk) on the same stream, over the
 * d_desc[0, n) and d_route they wrote, and before qpp_unprotect.  d_next names
 * a next-phase key slot, or QPP_SLOT_NONE, per connection: lane i consults
 * S1 = d_next[d_route[i].conn], or, with d_route NULL, S1 = d_next[i] (one
 * entry per descriptor; n_next is not looked at then).  One lane per
 * descriptor.  The lane acts only if all of these hold; otherwise d_desc[i]
 * is left untouched and d_phase[i] = 0:
 *   - with route records, d_route[i].cls == QPP_R_SHORT and conn < n_next;
 *   - QPP_F_NO_HP is not set in the descriptor's flags;
 *   - 1 <= hdr_len <= QPP_MAX_HDR - 4 and hdr_len + 20 <= len, the bounds the
 *     packet kernels check, so a packet that would get QPP_S_LENGTH still does;
 *   - S0 = d_desc[i].slot < capacity and is installed;
 *   - S1 < capacity, is installed, has S0's suite and the other key_phase.
 * It then computes mask = HP(S0's header-protection key, in[in_off + hdr_len +
 * 4 .. + 20)) and b0 = in[in_off] ^ (mask[0] & 0x1f).  If bit 7 of b0 is clear
 * and ((b0 >> 2) & 1) != S0's key_phase, d_desc[i].slot = S1 and d_phase[i] =
 * 1; otherwise d_phase[i] = 0.  Only the slot field of a descriptor ever
 * changes; d_phase is written whole, so the same input gives the same bytes.
 * A lane reads byte in_off and the 16 sample bytes of its packet, never a
 * byte at or past in_off + len.
 * The caller's contract: a next-phase slot holds the CURRENT slot's
 * header-protection key (a key update keeps it, quic/crypto.py:157-168), the
 * next phase's AEAD key and IV, and the opposite key_phase, so both slots give
 * the same header mask and the packet kernels meet a slot whose phase matches
 * the packet.  A next slot with another HP key only makes the re-pointed
 * packet fail its tag (QPP_S_DECRYPT), which is harmless.  What a re-pointed
 * packet's QPP_S_OK means for the connection's keys (CryptoPair._update_key) is
 * the caller's, from d_phase.
 * QPP_E_ARG: NULL kt, or a NULL d_next / d_desc / d_in / d_phase with n > 0.
 * n == 0 returns QPP_OK and launches nothing. */
int qpp_route_phase(const qpp_keytab *kt, const qpp_route_rec *d_route /* may be NULL */,
                    const uint32_t *d_next, uint32_t n_next, qpp_desc *d_desc, uint32_t n,
                    const uint8_t *d_in, uint8_t *d_phase, void *stream);
/* qpp_route_phase launches of the resolving kernel (process-wide, since the
 * library loaded).  Diagnostic: a batch with no next-phase slot makes none. */
uint64_t qpp_route_phase_launches(void);

/* ---- routed send: 1-RTT headers and packet numbers built on the device ----
 * The mirror of routed receive.  The caller holds its connections' send state
 * in one device array, hands payloads and a connection index each, and a
 * kernel in front of qpp_protect writes what the reference's builder writes
 * per 1-RTT packet (quic/packet_builder.py:19-20 PACKET_NUMBER_SEND_SIZE,
 * :264-296 _end_packet's sample padding, :330-339 its short header): the
 * header, the packet number, the padding and an ordinary qpp_desc.  Long headers, datagram padding, frames and
 * congestion accounting stay with the caller's builder. */
#define QPP_SEND_PN_LEN 2                               /* packet_builder.py:20 PACKET_NUMBER_SEND_SIZE */
#define QPP_SEND_HEAD (1 + QPP_CID_MAX + QPP_SEND_PN_LEN) /* the longest header: first byte, CID, number */
#define QPP_SEND_TAIL (1 + QPP_TAG_LEN)                 /* the largest padding (a 1-byte payload's) + tag */
#define QPP_SN_OK 0
#define QPP_SN_CONN 1     /* p_conn[i] >= n_conn */
#define QPP_SN_CID 2      /* the connection's cid_len > QPP_CID_MAX */
#define QPP_SN_NO_KEY 3   /* the connection's slot is QPP_SLOT_NONE, past the table, or not installed */
#define QPP_SN_EMPTY 4    /* len == 0: the builder cancels an empty packet (packet_builder.py:266,361-363) */
#define QPP_SN_PN 5       /* next_pn + seq wraps or is >= 2^62 */
#define QPP_SN_ROOM 6     /* p_off < hdr_len, or p_off + len + pad + QPP_TAG_LEN > buf_len */
/* One connection's send state. */
typedef struct qpp_send_conn {
    uint64_t next_pn;  /* the packet number of the connection's first packet of the batch */
    uint32_t slot;     /* its 1-RTT send key slot; the header's key-phase bit is the slot's own */
    uint8_t cid_len;   /* the peer's connection ID, 0..QPP_CID_MAX bytes */
    uint8_t spin;      /* the spin bit (nonzero: set) */
    uint8_t cid[20];   /* zero padded */
    uint8_t rsv[6];
} qpp_send_conn;       /* 40 bytes */
typedef struct qpp_send_rec {
    uint64_t pn;       /* the packet's number; 0 unless status is QPP_SN_OK */
    uint16_t hdr_len;  /* 1 + cid_len + QPP_SEND_PN_LEN; 0 unless status is QPP_SN_OK */
    uint8_t status;    /* QPP_SN_*: the first failing check, in the order above */
    uint8_t rsv[5];
} qpp_send_rec;        /* 16 bytes */
/* qpp_send_fill: asynchronous on `stream`; runs before qpp_protect on the same
 * stream, over the same buffer.  Packet i's payload lies at d_buf[d_off[i],
 * d_off[i] + d_len[i]) already and belongs to connection C = d_sendconn[
 * d_conn[i]]; d_seq[i] is its ordinal among C's packets of this batch, counted
 * by the caller (the device ranks nothing and uses no atomics).  One lane per
 * packet.  With pn = C.next_pn + d_seq[i], hdr_len = 1 + C.cid_len +
 * QPP_SEND_PN_LEN and pad = max(0, 4 - QPP_SEND_PN_LEN - len), lane i writes
 *   d_buf[off - hdr_len]          0x40 | spin << 5 | key_phase << 2 | (QPP_SEND_PN_LEN - 1),
 *                                 key_phase the installed slot C.slot's own (a local key
 *                                 update is then only a new slot)
 *   d_buf[off - hdr_len + 1 ..]   C.cid[0, cid_len), then pn & 0xffff big-endian
 *   d_buf[off + len, + pad)       zeros: PADDING frames, so that the header-protection sample
 *                                 exists (the descriptor's len includes them)
 *   d_desc[i] = {in_off = out_off = off - hdr_len, len + pad, hdr_len, flags 0, pn, C.slot}
 *   d_rec[i]  = {pn, hdr_len, QPP_SN_OK}
 * A lane whose status is not QPP_SN_OK writes no byte of d_buf, the inert
 * descriptor {in_off = out_off = off, len 0, hdr_len 0, QPP_SLOT_NONE} (which
 * qpp_protect answers with QPP_S_NO_KEY, touching nothing) and a record with
 * pn 0.  Descriptors and records are written whole for every lane, so the same
 * input gives the same bytes.  A lane reads nothing of the payload.  Length
 * limits beyond the buffer's (QPP_PACKET_MAX) stay with qpp_protect, as
 * QPP_S_LENGTH.
 * The caller's contract for the device form: the regions [d_off[i] -
 * QPP_SEND_HEAD, d_off[i] + d_len[i] + QPP_SEND_TAIL) are pairwise disjoint;
 * the lanes' stores and the protect's then never meet.
 * QPP_E_ARG: NULL kt, or with n > 0 a NULL array or buffer, or a NULL
 * d_sendconn with n_conn > 0.  n == 0 returns QPP_OK and launches nothing. */
int qpp_send_fill(const qpp_keytab *kt, const qpp_send_conn *d_sendconn, uint32_t n_conn, const uint64_t *d_off,
                  const uint32_t *d_len, const uint32_t *d_conn, const uint32_t *d_seq, uint32_t n, uint8_t *d_buf,
                  uint64_t buf_len, qpp_desc *d_desc, qpp_send_rec *d_rec, void *stream);
/* qpp_send_fill launches (process-wide, since the library loaded).  Diagnostic. */
uint64_t qpp_send_launches(void);

/* Header-protection masks: replaces HeaderProtection_mask (_crypto.c:278-287).
 * d_samples: n x 16 bytes, d_masks: n x 16 bytes (first 5 used). */
int qpp_hp_mask(const qpp_keytab *kt, const uint32_t *d_slots, const uint8_t *d_samples,
                uint32_t n, uint8_t *d_masks, void *stream);

/* Synchronous host-buffer forms (pinned staging, H2D, kernel, D2H), used by the
 * per-packet object API and the batched send/receive callers.  A batch with at
 * least 64 MiB of output and out_off non-decreasing in descriptor order runs as
 * a chunked H2D / kernel / D2H pipeline on three streams (QPP_SESSION_SERIAL=1
 * in the environment forces the serial form); the bytes written are the same. */
int qpp_session_create(size_t max_bytes, uint32_t max_packets, qpp_session **out);
void qpp_session_destroy(qpp_session *s);
void *qpp_session_stream(qpp_session *s);
int qpp_session_protect(qpp_session *s, const qpp_keytab *kt, const qpp_desc *desc, uint32_t n,
                        const uint8_t *in, size_t in_len, uint8_t *out, size_t out_len,
                        qpp_result *res);
int qpp_session_unprotect(qpp_session *s, const qpp_keytab *kt, const qpp_desc *desc,
                          uint32_t n, const uint8_t *in, size_t in_len, uint8_t *out,
                          size_t out_len, qpp_result *res);
int qpp_session_hp_mask(qpp_session *s, const qpp_keytab *kt, const uint32_t *slots,
                        const uint8_t *samples, uint32_t n, uint8_t *masks);
/* qpp_route + qpp_unprotect on host buffers: one H2D of the datagram bytes
 * and the small arrays, the routing kernel, the unplanned unprotect over all
 * n descriptors, one D2H of output, descriptors (desc_out may be NULL), route
 * records and results.  Serial form only: there is no chunked pipeline for
 * this call, whatever the batch's size.  Works with the session's own pinned
 * staging (qpp_session_stage) as `in` / `out`, like the calls above.  The
 * host checks every off[i] + len[i] <= in_len and <= out_len before anything
 * is launched: a violation is QPP_E_ARG (the caller's own arrays are wrong)
 * and nothing is touched.  Output bytes no packet writes are zeros. */
int qpp_session_route_unprotect(qpp_session *s, const qpp_keytab *kt, const qpp_cidmap *m, uint32_t cid_len,
                                const uint64_t *off, const uint32_t *len, uint32_t n, const uint8_t *in,
                                size_t in_len, const uint32_t *conn_slot, const uint64_t *conn_expected,
                                uint32_t n_conn, uint16_t desc_flags, uint8_t *out, size_t out_len,
                                qpp_desc *desc_out, qpp_route_rec *route_out, qpp_result *res);
/* qpp_session_route_unprotect with the device walk of the long-header
 * datagrams long_idx[n_long] (qpp_route_walk) between the routing kernel and
 * the unprotect: one H2D, the routing kernel, the walking kernel when n_long >
 * 0, one unplanned unprotect over n + 3 n_long descriptors, one D2H that
 * also returns the walk records (walk_out[n_long * QPP_WALK_MAX],
 * walk_n_out[n_long]).  desc_out (may be NULL) and res hold n + 3 n_long
 * entries.  The per-connection arrays are the walk's: conn_slot[n_conn *
 * QPP_KEYSETS], conn_expected[n_conn * QPP_SPACES]; the routing kernel is
 * given each connection's 1-RTT slot and application-space number from them.
 * Checked on the host before anything is launched, besides the offsets as
 * above: long_idx strictly increasing, every index < n, n + 3 n_long <=
 * 2^31 - 1, walk_out / walk_n_out given when n_long > 0.  A violation is
 * QPP_E_ARG and nothing is touched.  With n_long == 0 the call does what
 * qpp_session_route_unprotect does: the same launches, the same bytes. */
int qpp_session_route_walk_unprotect(qpp_session *s, const qpp_keytab *kt, const qpp_cidmap *m, uint32_t cid_len,
                                     const uint64_t *off, const uint32_t *len, uint32_t n, const uint8_t *in,
                                     size_t in_len, const uint32_t *long_idx, uint32_t n_long,
                                     const uint32_t *conn_slot, const uint64_t *conn_expected, uint32_t n_conn,
                                     uint16_t desc_flags, uint8_t *out, size_t out_len, qpp_desc *desc_out,
                                     qpp_route_rec *route_out, qpp_result *res, qpp_walk_rec *walk_out,
                                     uint32_t *walk_n_out);
/* qpp_session_route_walk_unprotect with the peers' key updates resolved on
 * the device (qpp_route_phase) between the walk and the unprotect.
 * conn_next[n_conn] (may be NULL) names each connection's next-phase 1-RTT
 * slot or QPP_SLOT_NONE; phase_out[n] (required when conn_next is given)
 * receives d_phase.  The sequence is one H2D, the routing kernel, the walking
 * kernel when n_long > 0, the resolving kernel over descriptors [0, n) when
 * conn_next holds at least one slot, one unplanned unprotect over n + 3
 * n_long descriptors, one D2H; conn_next and phase_out ride in the same
 * scratch copy in each direction.  The walk's extra descriptors [n, n + 3
 * n_long) -- coalesced 1-RTT packets behind long headers, which exist only
 * during a handshake, when no key update is legal -- are not resolved: a
 * flipped one reports QPP_S_KEY_PHASE as ever.
 * Checked on the host before anything is launched, besides what the walk form
 * checks: every conn_next entry < capacity or QPP_SLOT_NONE, phase_out given
 * with conn_next.  A violation is QPP_E_ARG and nothing is touched.  With
 * conn_next NULL or all QPP_SLOT_NONE the call makes the same launches and
 * returns the same bytes as qpp_session_route_walk_unprotect, and phase_out
 * (if given) is zeros. */
int qpp_session_route_phase_unprotect(qpp_session *s, const qpp_keytab *kt, const qpp_cidmap *m, uint32_t cid_len,
                                      const uint64_t *off, const uint32_t *len, uint32_t n, const uint8_t *in,
                                      size_t in_len, const uint32_t *long_idx, uint32_t n_long,
                                      const uint32_t *conn_slot, const uint64_t *conn_expected, uint32_t n_conn,
                                      const uint32_t *conn_next, uint16_t desc_flags, uint8_t *out, size_t out_len,
                                      qpp_desc *desc_out, qpp_route_rec *route_out, qpp_result *res,
                                      qpp_walk_rec *walk_out, uint32_t *walk_n_out, uint8_t *phase_out);
/* qpp_session_route_walk_unprotect for a server that also takes on new
 * connections: between the walk and the unprotect, qpp_route_accept picks
 * the unrouted Initials among the candidates acc_row[n_acc] (rows of
 * long_idx) and qpp_keytab_derive_initial_device derives and installs their
 * keys in the slots acc_slot[2 n_acc], so the one unprotect launch decrypts
 * their first packets too.  The sequence is one H2D, the routing kernel, the
 * walking kernel, the accepting kernel, the derivation, the slot expansion,
 * one unplanned unprotect over n + 3 n_long descriptors, one D2H.  The new
 * arrays ride in the same scratch copy in each direction; the records, the key
 * material and the secrets are device scratch of the session.  acc_out[n_acc]
 * receives the qpp_accept_rec records, km_out[2 n_acc] and secrets_out[2 n_acc
 * x 32] what qpp_keytab_derive_initial returns ([2a] the client direction of
 * candidate a, [2a + 1] its server direction; a rejected candidate's carry
 * QPP_SLOT_NONE and keys nobody uses).  kt is not const: every acc_slot is
 * noted in its bookkeeping (qpp_keytab_derive_initial_device), and the caller
 * clears those of the candidates the device rejected.
 * Checked on the host before anything is launched or noted, besides what the
 * walk form checks: acc_row strictly increasing and < n_long, every
 * acc_slot[2a] < capacity, every acc_slot[2a + 1] < capacity or QPP_SLOT_NONE,
 * all given slots pairwise distinct, n_acc <= 2^24, no accept_flags bit other
 * than QPP_A_NEED_TOKEN, and acc_out / km_out / secrets_out given when n_acc >
 * 0.  A violation is QPP_E_ARG and nothing is touched.  With n_acc == 0 the
 * call makes the same launches and returns the same bytes as
 * qpp_session_route_walk_unprotect. */
int qpp_session_accept_unprotect(qpp_session *s, qpp_keytab *kt, const qpp_cidmap *m, uint32_t cid_len,
                                 const uint64_t *off, const uint32_t *len, uint32_t n, const uint8_t *in,
                                 size_t in_len, const uint32_t *long_idx, uint32_t n_long,
                                 const uint32_t *conn_slot, const uint64_t *conn_expected, uint32_t n_conn,
                                 uint16_t desc_flags, const uint32_t *acc_row, const uint32_t *acc_slot,
                                 uint32_t n_acc, uint32_t accept_flags, uint8_t *out, size_t out_len,
                                 qpp_desc *desc_out, qpp_route_rec *route_out, qpp_result *res,
                                 qpp_walk_rec *walk_out, uint32_t *walk_n_out, qpp_accept_rec *acc_out,
                                 qpp_key_material *km_out, uint8_t *secrets_out);
/* qpp_session_accept_unprotect for a server that also answers what it does
 * not accept (asyncio/server.py:71-111; quic/packet.py:288-334; quic/retry.py):
 * qpp_route_reply runs after the accepting kernel, and after the batch's
 * unprotect two qpp_protect launches over the n_acc reply regions seal the
 * tokens and append the Retry integrity tags, both with reply_kt (the slot
 * convention of qpp_route_reply; capacity >= 3).  addr[20 n_acc] (may be NULL
 * without QPP_RP_RETRY), rnd[16 n_acc], token_ctr, versions[n_versions] and
 * reply_flags are qpp_route_reply's inputs, in host memory here.  The inputs
 * ride up in the existing scratch copy; the reply buffer, the records and the
 * two launches' results ride down in the existing one; the descriptors never
 * leave the device.  reply_out[256 n_acc] receives the reply buffer and
 * reply_rec_out[n_acc] the records: the packet to send for candidate a is
 * reply_out[rec.off .. rec.off + rec.len) when rec.kind is not
 * QPP_RP_KIND_NONE.  A Retry whose seal or tag result is not QPP_S_OK is
 * downgraded on the host to {len 0, QPP_RP_KIND_NONE, that status}: a reply
 * is never half built.
 * Checked on the host before anything is launched or noted, besides what the
 * accept form checks: with reply_flags != 0, reply_kt, rnd, reply_out and
 * reply_rec_out given, qpp_keytab_capacity(reply_kt) >= 3, no reply_flags bit
 * other than QPP_RP_VN | QPP_RP_RETRY, 1 <= n_versions <= QPP_RP_MAX_VERSIONS
 * with versions given, and with QPP_RP_RETRY addr given, every addr[20a] 6 or
 * 18 and token_ctr + n_acc not wrapping.  A violation is QPP_E_ARG and nothing
 * is touched.  With reply_flags == 0 (or n_acc == 0) the call is
 * qpp_session_accept_unprotect: the same launches, the same bytes, and the
 * reply arguments are not looked at. */
int qpp_session_accept_reply_unprotect(qpp_session *s, qpp_keytab *kt, const qpp_cidmap *m, uint32_t cid_len,
                                       const uint64_t *off, const uint32_t *len, uint32_t n, const uint8_t *in,
                                       size_t in_len, const uint32_t *long_idx, uint32_t n_long,
                                       const uint32_t *conn_slot, const uint64_t *conn_expected, uint32_t n_conn,
                                       uint16_t desc_flags, const uint32_t *acc_row, const uint32_t *acc_slot,
                                       uint32_t n_acc, uint32_t accept_flags, const qpp_keytab *reply_kt,
                                       const uint8_t *addr, const uint8_t *rnd, uint64_t token_ctr,
                                       const uint32_t *versions, uint32_t n_versions, uint32_t reply_flags,
                                       uint8_t *out, size_t out_len, qpp_desc *desc_out, qpp_route_rec *route_out,
                                       qpp_result *res, qpp_walk_rec *walk_out, uint32_t *walk_n_out,
                                       qpp_accept_rec *acc_out, qpp_key_material *km_out, uint8_t *secrets_out,
                                       uint8_t *reply_out, qpp_reply_rec *reply_rec_out);
/* qpp_session_accept_reply_unprotect for a server in Retry mode that also
 * validates the tokens that come back (asyncio/server.py:112-120;
 * quic/retry.py): the three steps of qpp_route_token run ahead of the
 * accepting kernel.  The sequence on the one stream is the routing kernel, the
 * walking kernel, a memset of the token scratch, the locating kernel,
 * qpp_unprotect(reply_kt, ...) over the n_acc token descriptors from the
 * datagram buffer (read only) into the token scratch, the accepting kernel
 * with the verdicts, the assembling kernel, the derivation, the batch's
 * unprotect and the two reply protects.  A QPP_ACC_BAD_TOKEN candidate gets
 * no keys, no slot, no unprotect and no reply.  tokrec_out[n_acc] receives the
 * qpp_token_rec records in the same download as the accept records; the token
 * descriptors, the opened tokens and their results never leave the device.
 * Checked on the host before anything is launched or noted, besides what the
 * reply form checks: QPP_A_NEED_TOKEN in accept_flags, QPP_RP_RETRY in
 * reply_flags, reply_kt given with capacity >= 3, and with n_acc > 0 addr and
 * tokrec_out given.  A violation is QPP_E_ARG and nothing is touched. */
int qpp_session_serve_unprotect(qpp_session *s, qpp_keytab *kt, const qpp_cidmap *m, uint32_t cid_len,
                                const uint64_t *off, const uint32_t *len, uint32_t n, const uint8_t *in,
                                size_t in_len, const uint32_t *long_idx, uint32_t n_long,
                                const uint32_t *conn_slot, const uint64_t *conn_expected, uint32_t n_conn,
                                uint16_t desc_flags, const uint32_t *acc_row, const uint32_t *acc_slot,
                                uint32_t n_acc, uint32_t accept_flags, const qpp_keytab *reply_kt,
                                const uint8_t *addr, const uint8_t *rnd, uint64_t token_ctr,
                                const uint32_t *versions, uint32_t n_versions, uint32_t reply_flags, uint8_t *out,
                                size_t out_len, qpp_desc *desc_out, qpp_route_rec *route_out, qpp_result *res,
                                qpp_walk_rec *walk_out, uint32_t *walk_n_out, qpp_accept_rec *acc_out,
                                qpp_key_material *km_out, uint8_t *secrets_out, uint8_t *reply_out,
                                qpp_reply_rec *reply_rec_out, qpp_token_rec *tokrec_out);
/* qpp_send_fill + qpp_protect on host buffers, the send side's counterpart of
 * qpp_session_route_unprotect: one H2D of the staged buffer `in` (the payloads
 * at off[i], room for a header before and padding and tag after each) and of
 * [off | len | conn | seq | sendconn], the filling kernel, one unplanned
 * qpp_protect over the n descriptors from the session's input buffer to its
 * output buffer at the same offsets, one D2H of the output and of [desc | rec |
 * results] (desc_out may be NULL).  Serial form only.  Works with the
 * session's own pinned staging (qpp_session_stage) as `in` / `out`.
 * Checked on the host before anything is launched; a violation is QPP_E_ARG
 * and nothing is touched:
 *   - off strictly increasing;
 *   - every region [off[i] - QPP_SEND_HEAD, off[i] + len[i] + QPP_SEND_TAIL)
 *     inside both buffers and behind its predecessor's;
 *   - every conn[i] < n_conn;
 *   - every sendconn[c].slot inside the table, or QPP_SLOT_NONE.
 * With n == 0 it returns QPP_OK and launches nothing.  Output bytes no packet
 * writes are zeros.  A packet qpp_send_fill refuses (rec_out[i].status) has
 * QPP_S_NO_KEY in res[i] and no byte written. */
int qpp_session_send_protect(qpp_session *s, const qpp_keytab *kt, const qpp_send_conn *sendconn, uint32_t n_conn,
                             const uint64_t *off, const uint32_t *len, const uint32_t *conn, const uint32_t *seq,
                             uint32_t n, const uint8_t *in, size_t in_len, uint8_t *out, size_t out_len,
                             qpp_desc *desc_out, qpp_send_rec *rec_out, qpp_result *res);
/* The session's own pinned staging buffers, sized for at least `bytes` of
 * input and of output and n packets; valid until the next call on the
 * session.  A caller that assembles its input straight into *h_in and passes
 * h_in / h_out as `in` / `out` to qpp_session_protect / _unprotect saves both
 * staging copies (the batched Python callers do). */
int qpp_session_stage(qpp_session *s, size_t bytes, uint32_t n, uint8_t **h_in, uint8_t **h_out);
int qpp_session_set_keys(qpp_session *s, qpp_keytab *kt, const qpp_key_material *km,
                         uint32_t n);

/* Phases of one pipelined host-buffer call (the chunked form of
 * qpp_session_protect / _unprotect), for a caller that wants to see where a
 * host batch's time goes: host copies into and out of pinned staging, both
 * PCIe directions and the kernels.  GPU phases come from timing events around
 * every chunk's H2D, kernels and D2H (sums of the chunks' durations; the
 * engines overlap, so they add up to more than the call). */
typedef struct qpp_trace {
    uint32_t pipelined;  /* 1 if the last call ran as the chunked pipeline (else the rest is 0) */
    uint32_t chunks;
    double total_ms;     /* the call, entry to return */
    double submit_ms;    /* the submission loop: staging copies in, enqueues, early hand-backs */
    double copy_in_ms;   /* caller -> pinned staging copies, wall time on the calling thread */
    double copy_out_ms;  /* pinned staging -> caller copies, summed over the copy threads' tasks */
    double wait_ms;      /* after the submission loop: the last chunks' D2H and copy-out */
    double h2d_ms;       /* sum of the chunks' H2D durations (descriptors and input) */
    double kernel_ms;    /* sum of the chunks' kernel durations */
    double d2h_ms;       /* sum of the chunks' D2H durations (output and results) */
    double gpu_span_ms;  /* first H2D start to last D2H end */
    double in_bytes, out_bytes;  /* bytes sent H2D / returned D2H */
} qpp_trace;
/* enable != 0 turns tracing on for the session's following calls (0 off, -1
 * unchanged); last (may be NULL) receives the previous traced call's phases. */
int qpp_session_trace(qpp_session *s, int enable, qpp_trace *last);


/* One host batch over several GPUs of the node (the
 * server socket of src/aioquic/asyncio/server.py:60-152 feeds all
 * connections, and that is the batch to split).  A qpp_multi holds a session
 * and a replica of the key table per device; *_protect / *_unprotect cut the
 * batch into contiguous descriptor ranges, one per device, run them at once
 * (one host thread each) and write every result at its packet's position in
 * the caller's arrays -- the same bytes and results as one session.  Ranges
 * need disjoint output extents (descriptors in output order); otherwise the
 * batch runs on the first device.  Up to 16 devices; a device may be listed
 * twice (two sessions on one GPU).  Like a session, single-threaded. */
typedef struct qpp_multi qpp_multi;
int qpp_multi_create(const int *devices, int n_devices, uint32_t key_capacity, qpp_multi **out);
void qpp_multi_destroy(qpp_multi *m);
int qpp_multi_devices(const qpp_multi *m);
int qpp_multi_set_keys(qpp_multi *m, const qpp_key_material *km, uint32_t n);
int qpp_multi_protect(qpp_multi *m, const qpp_desc *desc, uint32_t n, const uint8_t *in, size_t in_len,
                      uint8_t *out, size_t out_len, qpp_result *res);
int qpp_multi_unprotect(qpp_multi *m, const qpp_desc *desc, uint32_t n, const uint8_t *in, size_t in_len,
                        uint8_t *out, size_t out_len, qpp_result *res);
/* qpp_session_trace on every device's session; last[k] for device k (up to
 * max entries).  Returns the number of devices written, or a QPP_E_* code. */
int qpp_multi_trace(qpp_multi *m, int enable, qpp_trace *last, int max);

#ifdef __cplusplus
}
#endif
#endif
