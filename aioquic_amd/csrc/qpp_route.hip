// qpp_route.hip -- routing received datagrams to connections by connection ID
// on the device (quic_pp.h: qpp_cidmap_*, qpp_route, qpp_route_walk,
// qpp_route_accept, qpp_route_reply, qpp_session_route_unprotect,
// qpp_session_route_walk_unprotect, qpp_session_accept_unprotect,
// qpp_session_accept_reply_unprotect).
//
// Replaces the per-datagram routing of the reference's server
// (asyncio/server.py:60-152: pull_quic_header, then
// self._protocols.get(header.destination_cid)) and its CID bookkeeping
// (_connection_id_issued / _connection_id_retired, server.py:154-170).
//
// The host owns the map (qpp_route.h, HostMap): put and remove change the
// mirror and then scatter only the buckets they changed to the device copy.
// k_route only reads the table: no device-side inserts, no atomics.
#include <hip/hip_runtime.h>
#include <atomic>
#include <new>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include "quic_pp.h"
#include "qpp_internal.h"
#include "qpp_accept.h"
#include "qpp_reply.h"
#include "qpp_route.h"
#include "qpp_send.h"
#include "qpp_token.h"
#include "qpp_walk.h"

using qpp_rt::Bucket;
using qpp_rt::HostMap;

static_assert(sizeof(qpp_cid_entry) == 32 && sizeof(qpp_route_rec) == 8 && sizeof(qpp_desc) == 40, "ABI records");
static_assert(QPP_R_SHORT == qpp_rt::kShort && QPP_R_LONG == qpp_rt::kLong &&
              QPP_R_UNKNOWN_CID == qpp_rt::kUnknownCid && QPP_R_MALFORMED == qpp_rt::kMalformed &&
              QPP_R_BAD_CONN == qpp_rt::kBadConn && QPP_CONN_NONE == qpp_rt::kConnNone, "route classes");
static_assert(sizeof(qpp_walk_rec) == sizeof(qpp_wk::Rec) && QPP_WALK_MAX == qpp_wk::kWalkMax &&
              QPP_KEYSETS == qpp_wk::kKeysets && QPP_SPACES == qpp_wk::kSpaces &&
              QPP_DESC_NONE == qpp_wk::kDescNone && QPP_MAX_HDR == qpp_wk::kMaxHdr &&
              QPP_W_OK == qpp_wk::kOk && QPP_W_PARSE == qpp_wk::kParse && QPP_W_HOST == qpp_wk::kHost,
              "walk records");
static_assert(sizeof(qpp_accept_rec) == sizeof(qpp_ac::Acc) && sizeof(qpp_initial) == sizeof(qpp_ac::Initial) &&
              sizeof(qpp_desc) == sizeof(qpp_ac::Desc) && QPP_ACC_OK == qpp_ac::kOk &&
              QPP_ACC_ROUTED == qpp_ac::kRouted && QPP_ACC_NOT_INITIAL == qpp_ac::kNotInitial &&
              QPP_ACC_VERSION == qpp_ac::kVersion && QPP_ACC_SMALL == qpp_ac::kSmall &&
              QPP_ACC_CID == qpp_ac::kCid && QPP_ACC_NO_TOKEN == qpp_ac::kNoToken &&
              QPP_A_NEED_TOKEN == qpp_ac::kNeedToken && QPP_SLOT_NONE == qpp_ac::kSlotNone &&
              QPP_CONN_NONE == qpp_ac::kConnNone && QPP_R_LONG == qpp_ac::kClsLong &&
              QPP_DERIVE_V2 == qpp_ac::kDeriveV2 && QPP_CID_MAX == qpp_wk::kCidMax,
              "accept records");
static_assert(sizeof(qpp_reply_rec) == sizeof(qpp_rp::Rec) && QPP_REPLY_STRIDE == qpp_rp::kStride &&
              QPP_RP_MAX_VERSIONS == qpp_rp::kMaxVersions && QPP_RP_ADDR_STRIDE == qpp_rp::kAddrStride &&
              QPP_RP_RAND_STRIDE == qpp_rp::kRandStride && QPP_RP_VN == qpp_rp::kVn &&
              QPP_RP_RETRY == qpp_rp::kRetry && QPP_RP_KIND_NONE == qpp_rp::kKindNone &&
              QPP_RP_KIND_VN == qpp_rp::kKindVn && QPP_RP_KIND_RETRY == qpp_rp::kKindRetry &&
              QPP_RP_OK == qpp_rp::kStOk && QPP_RP_BOUNDS == qpp_rp::kBounds && QPP_RP_ADDR == qpp_rp::kAddr &&
              QPP_F_NO_HP == qpp_rp::kNoHp && QPP_TAG_LEN == qpp_rp::kTagLen,
              "reply records");
static_assert(sizeof(qpp_token_rec) == sizeof(qpp_tk::Rec) && sizeof(qpp_token_rec) == 48 &&
              offsetof(qpp_token_rec, odcid) == 4 && offsetof(qpp_token_rec, rscid) == 24 &&
              QPP_TOKEN_STRIDE == qpp_tk::kStride && QPP_TOKEN_MIN == qpp_tk::kTokenMin &&
              QPP_TOKEN_MAX == qpp_tk::kTokenMax && QPP_TK_OK == qpp_tk::kOk && QPP_TK_NONE == qpp_tk::kNone &&
              QPP_TK_LENGTH == qpp_tk::kLength && QPP_TK_BOUNDS == qpp_tk::kBounds && QPP_TK_AUTH == qpp_tk::kAuth &&
              QPP_TK_FORM == qpp_tk::kForm && QPP_TK_ADDR == qpp_tk::kAddr &&
              QPP_ACC_BAD_TOKEN == qpp_ac::kBadToken && QPP_ACC_BAD_TOKEN == QPP_ACC_NO_TOKEN + 1 &&
              QPP_S_OK == qpp_tk::kResOk && QPP_TOKEN_MAX <= QPP_TOKEN_STRIDE && sizeof(qpp_result) == 16,
              "token records");

struct qpp_cidmap {
    HostMap host;
    Bucket *d_tab;
    // staging of one scatter: bucket indices, then the buckets (grown on demand)
    uint32_t *d_idx;
    Bucket *d_val;
    uint32_t scatter_cap;
};

namespace {

constexpr int kRouteWG = 256;

// One lane per changed bucket: two 16-byte stores.  The host has removed
// duplicate indices, so no two lanes write the same bucket.
__global__ __launch_bounds__(kRouteWG) void k_cid_scatter(Bucket *tab, uint32_t buckets, const uint32_t *idx,
                                                          const Bucket *val, uint32_t n)
{
    const uint32_t i = blockIdx.x * kRouteWG + threadIdx.x;
    if (i >= n) return;
    const uint32_t b = idx[i];
    if (b >= buckets) return;
    const uint4 *s = reinterpret_cast<const uint4 *>(&val[i]);
    uint4 *d = reinterpret_cast<uint4 *>(&tab[b]);
    const uint4 lo = s[0], hi = s[1];
    d[0] = lo;
    d[1] = hi;
}

// The table lookup of qpp_route.h with the bucket read as two 16-byte loads:
// lo = conn, cid_len | rsv, cid words 0-1; hi = cid words 2-4, padding.
__device__ inline uint32_t route_lookup(const Bucket *tab, uint32_t buckets, uint32_t cid_len, const uint32_t w[5])
{
    uint32_t b = qpp_rt::hash_cid(cid_len, w) & (buckets - 1);
    for (uint32_t it = 0; it < buckets; ++it) {
        const uint4 *q = reinterpret_cast<const uint4 *>(&tab[b]);
        const uint4 lo = q[0];
        const uint32_t el = lo.y & 0xffu;
        if (el == 0) return QPP_CONN_NONE;
        if (el == cid_len && lo.z == w[0] && lo.w == w[1]) {
            const uint4 hi = q[1];
            if (hi.x == w[2] && hi.y == w[3] && hi.z == w[4]) return lo.x;
        }
        b = (b + 1) & (buckets - 1);
    }
    return QPP_CONN_NONE;
}

// One lane per datagram (k_route).
__global__ __launch_bounds__(kRouteWG) void k_route(const Bucket *tab, uint32_t buckets, uint32_t cid_len,
                                                    const uint64_t *off, const uint32_t *len, uint32_t n,
                                                    const uint8_t *in, const uint32_t *conn_slot,
                                                    const uint64_t *conn_expected, uint32_t n_conn, uint32_t flags,
                                                    qpp_desc *desc, qpp_route_rec *route)
{
    const uint32_t i = blockIdx.x * kRouteWG + threadIdx.x;
    if (i >= n) return;
    const uint64_t o = off[i];
    const uint32_t l = len[i];
    const uint8_t *p = in + o;
    uint32_t key_off, key_len;
    uint32_t cls = qpp_rt::classify(p, l, cid_len, &key_off, &key_len);
    uint32_t conn = QPP_CONN_NONE;
    if (cls != QPP_R_MALFORMED && key_len) {
        uint32_t w[5];
        qpp_rt::load_cid(p + key_off, key_len, w);
        conn = route_lookup(tab, buckets, key_len, w);
    }
    cls = qpp_rt::settle_class(cls, conn, n_conn);
    if (desc) {
        qpp_desc d;
        d.in_off = o;
        d.out_off = o;
        d.len = 0;
        d.hdr_len = 0;
        d.flags = (uint16_t)flags;
        d.pn = 0;
        d.slot = QPP_SLOT_NONE;
        d.rsv = 0;
        if (cls == QPP_R_SHORT) {
            d.len = l;
            d.hdr_len = (uint16_t)(1 + cid_len);
            d.pn = conn_expected[conn];
            d.slot = conn_slot[conn];
        }
        desc[i] = d;
    }
    qpp_route_rec r;
    r.conn = conn;
    r.cls = (uint8_t)cls;
    r.rsv[0] = r.rsv[1] = r.rsv[2] = 0;
    route[i] = r;
}

// One lane per listed long-header datagram (k_walk): the serial
// walk of qpp_walk.h over the lane's own datagram, byte loads only, each record
// and descriptor stored as it is found.  No LDS, no atomics: where everything
// goes is fixed by (n, r, k).
__global__ __launch_bounds__(kRouteWG) void k_walk(uint32_t cid_len, const uint64_t *off, const uint32_t *len,
                                                   uint32_t n, const uint8_t *in, const qpp_route_rec *route,
                                                   const uint32_t *long_idx, uint32_t n_long,
                                                   const uint32_t *conn_slot, const uint64_t *conn_expected,
                                                   uint32_t n_conn, uint32_t flags, qpp_desc *desc,
                                                   qpp_walk_rec *walk, uint32_t *walk_n)
{
    const uint32_t r = blockIdx.x * kRouteWG + threadIdx.x;
    if (r >= n_long) return;
    const uint32_t i = long_idx[r];
    const uint32_t extra = n + 3u * r;  // descriptors of packets 1..3
    qpp_walk_rec none;
    none.off = none.len = none.version = none.desc = 0;
    none.pn_off = none.token_len = 0;
    none.type = none.status = none.dcid_len = none.scid_len = 0;
    if (i >= n) {
        // not the caller's contract: nothing of the batch is this lane's, and
        // its extra descriptors are inert all the same
        qpp_desc d;
        d.in_off = 0;
        d.out_off = 0;
        d.len = 0;
        d.hdr_len = 0;
        d.flags = (uint16_t)flags;
        d.pn = 0;
        d.slot = QPP_SLOT_NONE;
        d.rsv = 0;
        for (uint32_t k = 0; k < QPP_WALK_MAX - 1; ++k) desc[extra + k] = d;
        for (uint32_t k = 0; k < QPP_WALK_MAX; ++k) walk[(size_t)r * QPP_WALK_MAX + k] = none;
        walk_n[r] = 0;
        return;
    }
    const uint64_t o = off[i];
    const uint32_t l = len[i];
    const uint8_t *p = in + o;
    const qpp_route_rec rr = route[i];
    // a class that passed classify()'s long-header checks: byte 0 is there
    const bool is_long = rr.cls == QPP_R_LONG || (rr.cls == QPP_R_BAD_CONN && l > 0 && (p[0] & 0x80));
    const bool keyed = rr.cls == QPP_R_LONG && rr.conn < n_conn;
    qpp_desc inert;
    inert.in_off = o;
    inert.out_off = o;
    inert.len = 0;
    inert.hdr_len = 0;
    inert.flags = (uint16_t)flags;
    inert.pn = 0;
    inert.slot = QPP_SLOT_NONE;
    inert.rsv = 0;
    uint32_t found = 0;
    if (is_long) {
        found = qpp_wk::walk(p, l, cid_len, [&](uint32_t k, qpp_wk::Rec &w) {
            const uint32_t at = k == 0 ? i : extra + k - 1;
            if (keyed && w.status == QPP_W_OK && qpp_wk::protected_type(w.type)) {
                const uint32_t ks = qpp_wk::keyset_of(w.type, w.version);
                qpp_desc d = inert;
                d.in_off = o + w.off;
                d.out_off = o + w.off;
                d.len = w.len;
                d.hdr_len = w.pn_off;
                d.pn = conn_expected[(size_t)rr.conn * QPP_SPACES + qpp_wk::space_of(w.type)];
                d.slot = ks == qpp_wk::kKeysetNone ? QPP_SLOT_NONE : conn_slot[(size_t)rr.conn * QPP_KEYSETS + ks];
                desc[at] = d;
                w.desc = at;
            } else if (k) {
                desc[at] = inert;
            }
            qpp_walk_rec q;
            q.off = w.off;
            q.len = w.len;
            q.version = w.version;
            q.desc = w.desc;
            q.pn_off = w.pn_off;
            q.token_len = w.token_len;
            q.type = w.type;
            q.status = w.status;
            q.dcid_len = w.dcid_len;
            q.scid_len = w.scid_len;
            walk[(size_t)r * QPP_WALK_MAX + k] = q;
        });
    }
    for (uint32_t k = found ? found : 1; k < QPP_WALK_MAX; ++k) desc[extra + k - 1] = inert;
    for (uint32_t k = found; k < QPP_WALK_MAX; ++k) walk[(size_t)r * QPP_WALK_MAX + k] = none;
    walk_n[r] = found;
}

// A candidate's datagram and the records the walk and the route left of it:
// what k_accept, k_token and k_reply start from.  A row or an index outside
// the batch (not the caller's contract) has no record, so it is "not an
// Initial", and nothing of the batch is read.
struct Cand {
    uint32_t i, conn, found, l;
    uint8_t cls;
    uint64_t o;
    qpp_wk::Rec w0;
};

__device__ inline Cand candidate(uint32_t a, const uint64_t *off, const uint32_t *len, uint32_t n,
                                 const qpp_route_rec *route, const uint32_t *long_idx, uint32_t n_long,
                                 const qpp_walk_rec *walk, const uint32_t *walk_n, const uint32_t *acc_row)
{
    Cand c;
    const uint32_t r = acc_row[a];
    c.i = r < n_long ? long_idx[r] : n;
    c.conn = QPP_CONN_NONE, c.found = 0, c.l = 0;
    c.cls = QPP_R_LONG;
    c.o = 0;
    c.w0.off = c.w0.len = c.w0.version = c.w0.desc = 0;
    c.w0.pn_off = c.w0.token_len = 0;
    c.w0.type = c.w0.status = c.w0.dcid_len = c.w0.scid_len = 0;
    if (c.i < n) {
        const qpp_route_rec rr = route[c.i];
        c.conn = rr.conn;
        c.cls = rr.cls;
        c.found = walk_n[r];
        c.o = off[c.i];
        c.l = len[c.i];
        if (c.found) {
            const qpp_walk_rec q = walk[(size_t)r * QPP_WALK_MAX];
            c.w0.off = q.off;
            c.w0.len = q.len;
            c.w0.version = q.version;
            c.w0.desc = q.desc;
            c.w0.pn_off = q.pn_off;
            c.w0.token_len = q.token_len;
            c.w0.type = q.type;
            c.w0.status = q.status;
            c.w0.dcid_len = q.dcid_len;
            c.w0.scid_len = q.scid_len;
        }
    }
    return c;
}

__device__ inline void store_desc(qpp_desc *dst, const qpp_ac::Desc &rd)
{
    qpp_desc d;
    d.in_off = rd.in_off;
    d.out_off = rd.out_off;
    d.len = rd.len;
    d.hdr_len = rd.hdr_len;
    d.flags = rd.flags;
    d.pn = rd.pn;
    d.slot = rd.slot;
    d.rsv = rd.rsv;
    *dst = d;
}

// What a lane of the accepting kernels does (k_accept): the
// decision of qpp_accept.h over the lane's own walk and route records, then
// its qpp_initial, its accept record and, when accepted, its datagram's
// descriptor.  TOKENS (k_accept_tokens): between the decision and the records,
// the verdict of qpp_token.h on the token k_token located and the launch after
// it opened; a candidate that fails it is QPP_ACC_BAD_TOKEN and is written as
// any other rejection is.  No LDS, no atomics: lane a writes ini[a], acc[a],
// tokrec[a] and desc[i] of its own datagram i, and the rows are distinct.
template <bool TOKENS>
__device__ __forceinline__ void accept_lane(uint32_t a, const uint64_t *off, const uint32_t *len, uint32_t n,
                                            const uint8_t *in, const qpp_route_rec *route, const uint32_t *long_idx,
                                            uint32_t n_long, const qpp_walk_rec *walk, const uint32_t *walk_n,
                                            const uint32_t *acc_row, const uint32_t *acc_slot, uint32_t accept_flags,
                                            uint32_t desc_flags, const uint8_t *addr, const uint8_t *tok,
                                            const qpp_result *tokres, qpp_initial *ini, qpp_desc *desc,
                                            qpp_accept_rec *acc, qpp_token_rec *tokrec)
{
    const Cand c = candidate(a, off, len, n, route, long_idx, n_long, walk, walk_n, acc_row);
    uint8_t st = qpp_ac::decide(c.conn, c.cls, c.found, c.w0, c.l, accept_flags);
    if (TOKENS) {
        // the preliminary status is k_token's; a candidate that reaches the
        // token test without one (kNone) was not examined and is not accepted
        qpp_tk::Rec tr;
        const bool tested = st == QPP_ACC_OK && (accept_flags & QPP_A_NEED_TOKEN);
        const uint8_t pre = tested ? tokrec[a].status : (uint8_t)QPP_TK_NONE;
        const uint8_t v = qpp_tk::check(pre, tested ? tokres[a].status : (uint16_t)QPP_S_OK, c.w0.token_len,
                                        tok + (size_t)a * QPP_TOKEN_STRIDE, addr + (size_t)a * QPP_RP_ADDR_STRIDE, tr);
        if (tested && v != QPP_TK_OK) st = QPP_ACC_BAD_TOKEN;
        qpp_token_rec qt;
        qt.status = tr.status;
        qt.odcid_len = tr.odcid_len;
        qt.rscid_len = tr.rscid_len;
        qt.rsv = 0;
        for (uint32_t k = 0; k < QPP_CID_MAX; ++k) qt.odcid[k] = tr.odcid[k], qt.rscid[k] = tr.rscid[k];
        for (uint32_t k = 0; k < 4; ++k) qt.rsv2[k] = 0;
        tokrec[a] = qt;
    }
    qpp_ac::Initial ri;
    qpp_ac::Desc rd;
    qpp_ac::Acc ra;
    qpp_ac::accept_fill(st, c.i, c.w0, c.o, in + c.o, acc_slot[2 * (size_t)a], acc_slot[2 * (size_t)a + 1],
                        (uint16_t)desc_flags, ri, rd, ra);
    qpp_initial qi;
    qi.slot_client = ri.slot_client;
    qi.slot_server = ri.slot_server;
    qi.cid_len = ri.cid_len;
    qi.flags = ri.flags;
    qi.rsv[0] = qi.rsv[1] = 0;
    for (uint32_t k = 0; k < QPP_CID_MAX; ++k) qi.cid[k] = ri.cid[k];
    ini[a] = qi;
    qpp_accept_rec qa;
    qa.desc = ra.desc;
    qa.status = ra.status;
    qa.version = ra.version;
    qa.rsv[0] = qa.rsv[1] = 0;
    acc[a] = qa;
    if (st == QPP_ACC_OK) store_desc(&desc[c.i], rd);  // i < n: an accepted candidate has a route record
}

__global__ __launch_bounds__(kRouteWG) void k_accept(const uint64_t *off, const uint32_t *len, uint32_t n,
                                                     const uint8_t *in, const qpp_route_rec *route,
                                                     const uint32_t *long_idx, uint32_t n_long,
                                                     const qpp_walk_rec *walk, const uint32_t *walk_n,
                                                     const uint32_t *acc_row, const uint32_t *acc_slot,
                                                     uint32_t n_acc, uint32_t accept_flags, uint32_t desc_flags,
                                                     qpp_initial *ini, qpp_desc *desc, qpp_accept_rec *acc)
{
    const uint32_t a = blockIdx.x * kRouteWG + threadIdx.x;
    if (a >= n_acc) return;
    accept_lane<false>(a, off, len, n, in, route, long_idx, n_long, walk, walk_n, acc_row, acc_slot, accept_flags,
                       desc_flags, NULL, NULL, NULL, ini, desc, acc, NULL);
}

__global__ __launch_bounds__(kRouteWG) void k_accept_tokens(
    const uint64_t *off, const uint32_t *len, uint32_t n, const uint8_t *in, const qpp_route_rec *route,
    const uint32_t *long_idx, uint32_t n_long, const qpp_walk_rec *walk, const uint32_t *walk_n,
    const uint32_t *acc_row, const uint32_t *acc_slot, uint32_t n_acc, uint32_t accept_flags, uint32_t desc_flags,
    const uint8_t *addr, const uint8_t *tok, const qpp_result *tokres, qpp_initial *ini, qpp_desc *desc,
    qpp_accept_rec *acc, qpp_token_rec *tokrec)
{
    const uint32_t a = blockIdx.x * kRouteWG + threadIdx.x;
    if (a >= n_acc) return;
    accept_lane<true>(a, off, len, n, in, route, long_idx, n_long, walk, walk_n, acc_row, acc_slot, accept_flags,
                      desc_flags, addr, tok, tokres, ini, desc, acc, tokrec);
}

// One lane per candidate (k_token): where the token of the
// lane's own Initial lies (qpp_token.h), as the AEAD-only descriptor that
// opens it from the datagram buffer into the lane's own 128 bytes of the token
// buffer, and the token's preliminary status.  Byte loads of the lane's own
// header only, each behind a check against the datagram's length; the datagram
// buffer is not written.  No LDS, no atomics: lane a writes tokdesc[a] and
// tokrec[a].
__global__ __launch_bounds__(kRouteWG) void k_token(const uint64_t *off, const uint32_t *len, uint32_t n,
                                                    const uint8_t *in, const qpp_route_rec *route,
                                                    const uint32_t *long_idx, uint32_t n_long,
                                                    const qpp_walk_rec *walk, const uint32_t *walk_n,
                                                    const uint32_t *acc_row, uint32_t n_acc, uint32_t accept_flags,
                                                    qpp_desc *tokdesc, qpp_token_rec *tokrec)
{
    const uint32_t a = blockIdx.x * kRouteWG + threadIdx.x;
    if (a >= n_acc) return;
    const Cand c = candidate(a, off, len, n, route, long_idx, n_long, walk, walk_n, acc_row);
    const uint8_t st = qpp_ac::decide(c.conn, c.cls, c.found, c.w0, c.l, accept_flags);
    qpp_ac::Desc rd;
    const uint8_t pre = qpp_tk::token_desc(a, st, accept_flags, c.w0, c.o, c.l, in + c.o, rd);
    store_desc(&tokdesc[a], rd);
    qpp_token_rec qt;
    qt.status = pre;
    qt.odcid_len = qt.rscid_len = qt.rsv = 0;
    for (uint32_t k = 0; k < QPP_CID_MAX; ++k) qt.odcid[k] = qt.rscid[k] = 0;
    for (uint32_t k = 0; k < 4; ++k) qt.rsv2[k] = 0;
    tokrec[a] = qt;
}

// The supported versions of a Version Negotiation reply, by value among the
// kernel's arguments.
struct ReplyVersions {
    uint32_t v[QPP_RP_MAX_VERSIONS];
};

// One lane per candidate (k_reply): the assembly of
// qpp_reply.h over the lane's own accept and walk records, into its own 256
// bytes of the reply buffer, its two descriptors and its record.  No LDS, no
// atomics: everything lane a writes is indexed by a.
__global__ __launch_bounds__(kRouteWG) void k_reply(const uint64_t *off, const uint32_t *len, uint32_t n,
                                                    const uint8_t *in, const uint32_t *long_idx, uint32_t n_long,
                                                    const qpp_walk_rec *walk, const uint32_t *acc_row,
                                                    const qpp_accept_rec *acc, uint32_t n_acc, const uint8_t *addr,
                                                    const uint8_t *rnd, uint64_t token_ctr, ReplyVersions vs,
                                                    uint32_t n_versions, uint32_t reply_flags, uint8_t *reply,
                                                    qpp_desc *seal, qpp_desc *tag, qpp_reply_rec *rec)
{
    const uint32_t a = blockIdx.x * kRouteWG + threadIdx.x;
    if (a >= n_acc) return;
    const uint32_t r = acc_row[a];
    const uint32_t i = r < n_long ? long_idx[r] : n;
    // a row or an index outside the batch (not the caller's contract): no
    // reply, and nothing of the batch is read
    uint8_t st = QPP_ACC_NOT_INITIAL;
    uint32_t l = 0;
    uint64_t o = 0;
    qpp_wk::Rec w0;
    w0.off = w0.len = w0.version = w0.desc = 0;
    w0.pn_off = w0.token_len = 0;
    w0.type = w0.status = w0.dcid_len = w0.scid_len = 0;
    if (i < n) {
        st = acc[a].status;
        o = off[i];
        l = len[i];
        const qpp_walk_rec q = walk[(size_t)r * QPP_WALK_MAX];
        w0.version = q.version;
        w0.dcid_len = q.dcid_len;
        w0.scid_len = q.scid_len;
    }
    qpp_ac::Desc rs, rt;
    qpp_rp::Rec rr;
    qpp_rp::reply_one(a, st, w0, l, in + o, addr ? addr + (size_t)a * QPP_RP_ADDR_STRIDE : NULL,
                      rnd + (size_t)a * QPP_RP_RAND_STRIDE, token_ctr, vs.v, n_versions, reply_flags,
                      reply + (size_t)a * QPP_REPLY_STRIDE, rs, rt, rr);
    qpp_desc d;
    d.in_off = rs.in_off;
    d.out_off = rs.out_off;
    d.len = rs.len;
    d.hdr_len = rs.hdr_len;
    d.flags = rs.flags;
    d.pn = rs.pn;
    d.slot = rs.slot;
    d.rsv = rs.rsv;
    seal[a] = d;
    d.in_off = rt.in_off;
    d.out_off = rt.out_off;
    d.len = rt.len;
    d.hdr_len = rt.hdr_len;
    d.flags = rt.flags;
    d.pn = rt.pn;
    d.slot = rt.slot;
    d.rsv = rt.rsv;
    tag[a] = d;
    qpp_reply_rec q;
    q.off = rr.off;
    q.len = rr.len;
    q.kind = rr.kind;
    q.status = rr.status;
    rec[a] = q;
}

std::atomic<uint64_t> g_walk_launches{0};
std::atomic<uint64_t> g_accept_launches{0};
std::atomic<uint64_t> g_reply_launches{0};
std::atomic<uint64_t> g_token_launches{0};

void map_entries(const qpp_cid_entry *e, uint32_t n, std::vector<HostMap::Entry> &v)
{
    v.resize(n);
    for (uint32_t i = 0; i < n; ++i) v[i] = HostMap::Entry{e[i].conn, e[i].cid_len, e[i].cid};
}

// Bring the device copy up to date with the buckets the mirror changed.
int map_flush(qpp_cidmap *m, hipStream_t s)
{
    std::vector<uint32_t> &dirty = m->host.dirty;
    std::sort(dirty.begin(), dirty.end());
    dirty.erase(std::unique(dirty.begin(), dirty.end()), dirty.end());
    const uint32_t nd = (uint32_t)dirty.size();
    if (nd == 0) return QPP_OK;
    if (nd > m->scatter_cap) {
        if (m->d_idx) (void)hipFree(m->d_idx);
        if (m->d_val) (void)hipFree(m->d_val);
        m->d_idx = NULL;
        m->d_val = NULL;
        m->scatter_cap = 0;
        HIPCHK(hipMalloc(&m->d_idx, (size_t)nd * sizeof(uint32_t)));
        HIPCHK(hipMalloc(&m->d_val, (size_t)nd * sizeof(Bucket)));
        m->scatter_cap = nd;
    }
    std::vector<Bucket> val(nd);
    for (uint32_t k = 0; k < nd; ++k) val[k] = m->host.tab[dirty[k]];
    int rc = QPP_OK;
    if (hipMemcpyAsync(m->d_idx, dirty.data(), (size_t)nd * sizeof(uint32_t), hipMemcpyHostToDevice, s) !=
            hipSuccess ||
        hipMemcpyAsync(m->d_val, val.data(), (size_t)nd * sizeof(Bucket), hipMemcpyHostToDevice, s) != hipSuccess) {
        rc = QPP_E_HIP;
    } else {
        hipLaunchKernelGGL(k_cid_scatter, dim3((nd + kRouteWG - 1) / kRouteWG), dim3(kRouteWG), 0, s, m->d_tab,
                           m->host.buckets, m->d_idx, m->d_val, nd);
        if (hipGetLastError() != hipSuccess) rc = QPP_E_HIP;
    }
    // the staged values are host memory of this call: finish before returning
    if (hipStreamSynchronize(s) != hipSuccess && rc == QPP_OK) rc = QPP_E_HIP;
    (void)hipGetLastError();
    if (rc == QPP_OK) dirty.clear();  // on failure the next call sends them again
    return rc;
}

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

int qpp_cidmap_create(uint32_t capacity, qpp_cidmap **out)
{
    if (!out) return QPP_E_ARG;
    *out = NULL;
    if (capacity == 0 || capacity > qpp_rt::kMaxCapacity) return QPP_E_ARG;
    const int rc = qpp_device_check();
    if (rc != QPP_OK) return rc;
    qpp_cidmap *m = new (std::nothrow) qpp_cidmap();
    if (!m) return QPP_E_NOMEM;
    m->d_tab = NULL;
    m->d_idx = NULL;
    m->d_val = NULL;
    m->scatter_cap = 0;
    try {
        m->host.init(capacity);
    } catch (...) {
        delete m;
        return QPP_E_NOMEM;
    }
    const size_t bytes = (size_t)m->host.buckets * sizeof(Bucket);
    if (hipMalloc(&m->d_tab, bytes) != hipSuccess || hipMemset(m->d_tab, 0, bytes) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {
        (void)hipGetLastError();
        qpp_cidmap_destroy(m);
        return QPP_E_NOMEM;
    }
    *out = m;
    return QPP_OK;
}

void qpp_cidmap_destroy(qpp_cidmap *m)
{
    if (!m) return;
    if (m->d_tab) (void)hipFree(m->d_tab);
    if (m->d_idx) (void)hipFree(m->d_idx);
    if (m->d_val) (void)hipFree(m->d_val);
    delete m;
}

uint32_t qpp_cidmap_count(const qpp_cidmap *m) { return m ? m->host.count : 0; }
uint32_t qpp_cidmap_buckets(const qpp_cidmap *m) { return m ? m->host.buckets : 0; }

uint32_t qpp_cidmap_find(const qpp_cidmap *m, const uint8_t *cid, uint32_t cid_len)
{
    if (!m || !cid || cid_len == 0 || cid_len > QPP_CID_MAX) return QPP_CONN_NONE;
    return m->host.find(cid, cid_len);
}

uint32_t qpp_cidmap_home(const qpp_cidmap *m, const uint8_t *cid, uint32_t cid_len)
{
    if (!m || !cid || cid_len == 0 || cid_len > QPP_CID_MAX) return QPP_CONN_NONE;
    return m->host.home(cid, cid_len);
}

int qpp_cidmap_put(qpp_cidmap *m, const qpp_cid_entry *e, uint32_t n, void *stream)
{
    if (!m || (!e && n)) return QPP_E_ARG;
    if (n == 0) return QPP_OK;
    try {
        std::vector<HostMap::Entry> v;
        map_entries(e, n, v);
        if (!m->host.put(v.data(), n)) return QPP_E_ARG;
    } catch (...) {
        return QPP_E_NOMEM;
    }
    return map_flush(m, (hipStream_t)stream);
}

int qpp_cidmap_remove(qpp_cidmap *m, const qpp_cid_entry *e, uint32_t n, void *stream)
{
    if (!m || (!e && n)) return QPP_E_ARG;
    if (n == 0) return QPP_OK;
    try {
        std::vector<HostMap::Entry> v;
        map_entries(e, n, v);
        if (!m->host.remove(v.data(), n)) return QPP_E_ARG;
    } catch (...) {
        return QPP_E_NOMEM;
    }
    return map_flush(m, (hipStream_t)stream);
}

int qpp_route(const qpp_cidmap *m, uint32_t cid_len, const uint64_t *d_off, const uint32_t *d_len, uint32_t n,
              const uint8_t *d_in, const uint32_t *d_conn_slot, const uint64_t *d_conn_expected, uint32_t n_conn,
              uint16_t desc_flags, qpp_desc *d_desc, qpp_route_rec *d_route, void *stream)
{
    if (!m || cid_len < 1 || cid_len > QPP_CID_MAX) return QPP_E_ARG;
    if (n == 0) return QPP_OK;
    if (!d_off || !d_len || !d_in || !d_route || (n_conn && d_desc && (!d_conn_slot || !d_conn_expected)))
        return QPP_E_ARG;
    hipLaunchKernelGGL(k_route, dim3((n + kRouteWG - 1) / kRouteWG), dim3(kRouteWG), 0, (hipStream_t)stream,
                       m->d_tab, m->host.buckets, cid_len, d_off, d_len, n, d_in, d_conn_slot, d_conn_expected,
                       n_conn, (uint32_t)desc_flags, d_desc, d_route);
    HIPCHK(hipGetLastError());
    return QPP_OK;
}

int qpp_route_walk(uint32_t cid_len, const uint64_t *d_off, const uint32_t *d_len, uint32_t n, const uint8_t *d_in,
                   const qpp_route_rec *d_route, const uint32_t *d_long_idx, uint32_t n_long,
                   const uint32_t *d_conn_slot, const uint64_t *d_conn_expected, uint32_t n_conn,
                   uint16_t desc_flags, qpp_desc *d_desc, qpp_walk_rec *d_walk, uint32_t *d_walk_n, void *stream)
{
    if (cid_len < 1 || cid_len > QPP_CID_MAX) return QPP_E_ARG;
    if (n_long == 0) return QPP_OK;
    if (n == 0 || n_long > n || (uint64_t)n + 3ull * n_long > 0x7fffffffull) return QPP_E_ARG;
    if (!d_off || !d_len || !d_in || !d_route || !d_long_idx || !d_desc || !d_walk || !d_walk_n ||
        (n_conn && (!d_conn_slot || !d_conn_expected)))
        return QPP_E_ARG;
    hipLaunchKernelGGL(k_walk, dim3((n_long + kRouteWG - 1) / kRouteWG), dim3(kRouteWG), 0, (hipStream_t)stream,
                       cid_len, d_off, d_len, n, d_in, d_route, d_long_idx, n_long, d_conn_slot, d_conn_expected,
                       n_conn, (uint32_t)desc_flags, d_desc, d_walk, d_walk_n);
    HIPCHK(hipGetLastError());
    g_walk_launches.fetch_add(1, std::memory_order_relaxed);
    return QPP_OK;
}

uint64_t qpp_route_walk_launches(void) { return g_walk_launches.load(std::memory_order_relaxed); }

int qpp_route_accept(const uint64_t *d_off, const uint32_t *d_len, uint32_t n, const uint8_t *d_in,
                     const qpp_route_rec *d_route, const uint32_t *d_long_idx, uint32_t n_long,
                     const qpp_walk_rec *d_walk, const uint32_t *d_walk_n, const uint32_t *d_acc_row,
                     const uint32_t *d_acc_slot, uint32_t n_acc, uint32_t accept_flags, uint16_t desc_flags,
                     qpp_initial *d_ini, qpp_desc *d_desc, qpp_accept_rec *d_acc, void *stream)
{
    if (accept_flags & ~QPP_A_NEED_TOKEN) return QPP_E_ARG;
    if (n_acc == 0) return QPP_OK;
    if (!d_off || !d_len || !d_in || !d_route || !d_long_idx || !d_walk || !d_walk_n || !d_acc_row || !d_acc_slot ||
        !d_ini || !d_desc || !d_acc)
        return QPP_E_ARG;
    hipLaunchKernelGGL(k_accept, dim3((n_acc + kRouteWG - 1) / kRouteWG), dim3(kRouteWG), 0, (hipStream_t)stream,
                       d_off, d_len, n, d_in, d_route, d_long_idx, n_long, d_walk, d_walk_n, d_acc_row, d_acc_slot,
                       n_acc, accept_flags, (uint32_t)desc_flags, d_ini, d_desc, d_acc);
    HIPCHK(hipGetLastError());
    g_accept_launches.fetch_add(1, std::memory_order_relaxed);
    return QPP_OK;
}

uint64_t qpp_route_accept_launches(void) { return g_accept_launches.load(std::memory_order_relaxed); }

int qpp_route_token(const uint64_t *d_off, const uint32_t *d_len, uint32_t n, const uint8_t *d_in,
                    const qpp_route_rec *d_route, const uint32_t *d_long_idx, uint32_t n_long,
                    const qpp_walk_rec *d_walk, const uint32_t *d_walk_n, const uint32_t *d_acc_row, uint32_t n_acc,
                    uint32_t accept_flags, qpp_desc *d_tokdesc, qpp_token_rec *d_tokrec, void *stream)
{
    if (accept_flags & ~QPP_A_NEED_TOKEN) return QPP_E_ARG;
    if (n_acc == 0) return QPP_OK;
    if (n_acc > (1u << 24)) return QPP_E_ARG;
    if (!d_off || !d_len || !d_in || !d_route || !d_long_idx || !d_walk || !d_walk_n || !d_acc_row || !d_tokdesc ||
        !d_tokrec)
        return QPP_E_ARG;
    hipLaunchKernelGGL(k_token, dim3((n_acc + kRouteWG - 1) / kRouteWG), dim3(kRouteWG), 0, (hipStream_t)stream,
                       d_off, d_len, n, d_in, d_route, d_long_idx, n_long, d_walk, d_walk_n, d_acc_row, n_acc,
                       accept_flags, d_tokdesc, d_tokrec);
    HIPCHK(hipGetLastError());
    g_token_launches.fetch_add(1, std::memory_order_relaxed);
    return QPP_OK;
}

uint64_t qpp_route_token_launches(void) { return g_token_launches.load(std::memory_order_relaxed); }

int qpp_route_accept_tokens(const uint64_t *d_off, const uint32_t *d_len, uint32_t n, const uint8_t *d_in,
                            const qpp_route_rec *d_route, const uint32_t *d_long_idx, uint32_t n_long,
                            const qpp_walk_rec *d_walk, const uint32_t *d_walk_n, const uint32_t *d_acc_row,
                            const uint32_t *d_acc_slot, uint32_t n_acc, uint32_t accept_flags, uint16_t desc_flags,
                            const uint8_t *d_addr, const uint8_t *d_tok, const qpp_result *d_tokres,
                            qpp_initial *d_ini, qpp_desc *d_desc, qpp_accept_rec *d_acc, qpp_token_rec *d_tokrec,
                            void *stream)
{
    if (accept_flags & ~QPP_A_NEED_TOKEN) return QPP_E_ARG;
    if (n_acc == 0) return QPP_OK;
    if (!d_off || !d_len || !d_in || !d_route || !d_long_idx || !d_walk || !d_walk_n || !d_acc_row || !d_acc_slot ||
        !d_addr || !d_tok || !d_tokres || !d_ini || !d_desc || !d_acc || !d_tokrec)
        return QPP_E_ARG;
    hipLaunchKernelGGL(k_accept_tokens, dim3((n_acc + kRouteWG - 1) / kRouteWG), dim3(kRouteWG), 0,
                       (hipStream_t)stream, d_off, d_len, n, d_in, d_route, d_long_idx, n_long, d_walk, d_walk_n,
                       d_acc_row, d_acc_slot, n_acc, accept_flags, (uint32_t)desc_flags, d_addr, d_tok, d_tokres,
                       d_ini, d_desc, d_acc, d_tokrec);
    HIPCHK(hipGetLastError());
    g_accept_launches.fetch_add(1, std::memory_order_relaxed);
    return QPP_OK;
}

int qpp_route_reply(const uint64_t *d_off, const uint32_t *d_len, uint32_t n, const uint8_t *d_in,
                    const uint32_t *d_long_idx, uint32_t n_long, const qpp_walk_rec *d_walk,
                    const uint32_t *d_acc_row, const qpp_accept_rec *d_acc, uint32_t n_acc, const uint8_t *d_addr,
                    const uint8_t *d_rand, uint64_t token_ctr, const uint32_t *versions, uint32_t n_versions,
                    uint32_t reply_flags, uint8_t *d_reply, qpp_desc *d_seal, qpp_desc *d_tag, qpp_reply_rec *d_rec,
                    void *stream)
{
    if (reply_flags & ~(QPP_RP_VN | QPP_RP_RETRY)) return QPP_E_ARG;
    if (!versions || n_versions < 1 || n_versions > QPP_RP_MAX_VERSIONS) return QPP_E_ARG;
    if (n_acc == 0) return QPP_OK;
    if (!d_off || !d_len || !d_in || !d_long_idx || !d_walk || !d_acc_row || !d_acc || !d_rand || !d_reply ||
        !d_seal || !d_tag || !d_rec || ((reply_flags & QPP_RP_RETRY) && !d_addr))
        return QPP_E_ARG;
    ReplyVersions vs;
    for (uint32_t k = 0; k < QPP_RP_MAX_VERSIONS; ++k) vs.v[k] = k < n_versions ? versions[k] : 0;
    hipLaunchKernelGGL(k_reply, dim3((n_acc + kRouteWG - 1) / kRouteWG), dim3(kRouteWG), 0, (hipStream_t)stream,
                       d_off, d_len, n, d_in, d_long_idx, n_long, d_walk, d_acc_row, d_acc, n_acc, d_addr, d_rand,
                       token_ctr, vs, n_versions, reply_flags, d_reply, d_seal, d_tag, d_rec);
    HIPCHK(hipGetLastError());
    g_reply_launches.fetch_add(1, std::memory_order_relaxed);
    return QPP_OK;
}

uint64_t qpp_route_reply_launches(void) { return g_reply_launches.load(std::memory_order_relaxed); }

// The new-connection step of qpp_session_accept_unprotect.
struct AcceptArgs {
    qpp_keytab *kt;
    const uint32_t *row, *slot;
    uint32_t n, flags;
    qpp_accept_rec *acc_out;
    qpp_key_material *km_out;
    uint8_t *secrets_out;
};

// The answering step of qpp_session_accept_reply_unprotect, beside AcceptArgs.
struct ReplyArgs {
    const qpp_keytab *reply_kt;
    const uint8_t *addr, *rnd;
    uint64_t token_ctr;
    const uint32_t *versions;
    uint32_t n_versions, reply_flags;
    uint8_t *reply_out;
    qpp_reply_rec *reply_rec_out;
};

// The token step of qpp_session_serve_unprotect, beside AcceptArgs and ReplyArgs.
struct TokenArgs {
    qpp_token_rec *tokrec_out;
};

// The session forms.  walk_form: conn_slot / conn_expected are the walk's
// per-key-set and per-space arrays, and the routing kernel's per-connection
// ones (the 1-RTT slot, the application space's number) are taken from them.
// ac (walk form only; NULL or no candidates: nothing of it happens): the
// accepting kernel and the key derivation between the walk and the unprotect.
// rp (with ac's candidates only; NULL or no flag: nothing of it happens): the
// assembling kernel after the accepting one, the two reply protects after the
// batch's unprotect.
// tk (with ac and rp, Retry mode only): the locating kernel and the tokens'
// unprotect ahead of the accepting kernel, which then runs with their verdicts.
static int route_unprotect(qpp_session *s, const qpp_keytab *kt, const qpp_cidmap *m, uint32_t cid_len,
                           const uint64_t *off, const uint32_t *len, uint32_t n, const uint8_t *in, size_t in_len,
                           bool walk_form, const uint32_t *long_idx, uint32_t n_long, const uint32_t *conn_slot,
                           const uint64_t *conn_expected, uint32_t n_conn, uint16_t desc_flags, uint8_t *out,
                           size_t out_len, qpp_desc *desc_out, qpp_route_rec *route_out, qpp_result *res,
                           qpp_walk_rec *walk_out, uint32_t *walk_n_out, const AcceptArgs *ac = NULL,
                           const uint32_t *conn_next = NULL, uint8_t *phase_out = NULL, const ReplyArgs *rp = NULL,
                           const TokenArgs *tk = NULL)
{
    if (!s || !kt || !m || cid_len < 1 || cid_len > QPP_CID_MAX) return QPP_E_ARG;
    const uint32_t n_acc = ac ? ac->n : 0;
    if (ac && (ac->flags & ~QPP_A_NEED_TOKEN)) return QPP_E_ARG;
    // the tokens are a Retry-mode server's: both flags, the table with the token key, the addresses
    if (tk && (!ac || !rp || !(ac->flags & QPP_A_NEED_TOKEN) || !(rp->reply_flags & QPP_RP_RETRY) || !rp->reply_kt ||
               qpp_keytab_capacity(rp->reply_kt) < 3 || (n_acc && (!rp->addr || !tk->tokrec_out))))
        return QPP_E_ARG;
    if (n == 0) return n_long || n_acc ? QPP_E_ARG : QPP_OK;
    if (!off || !len || !route_out || !res || (in_len && !in) || (out_len && !out) ||
        (n_conn && (!conn_slot || !conn_expected)))
        return QPP_E_ARG;
    if (n_long && (!long_idx || !walk_out || !walk_n_out || n_long > n || (uint64_t)n + 3ull * n_long > 0x7fffffffull))
        return QPP_E_ARG;
    // the caller's own arrays: every datagram inside both buffers, or nothing runs
    for (uint32_t i = 0; i < n; ++i)
        if (off[i] > in_len || len[i] > in_len - off[i] || off[i] > out_len || len[i] > out_len - off[i])
            return QPP_E_ARG;
    for (uint32_t r = 0; r < n_long; ++r)
        if (long_idx[r] >= n || (r && long_idx[r] <= long_idx[r - 1])) return QPP_E_ARG;
    // next-phase slots: inside the table or none; the resolving kernel runs only when one is named
    bool any_next = false;
    if (conn_next) {
        if (!phase_out) return QPP_E_ARG;
        const uint32_t cap = qpp_keytab_capacity(kt);
        for (uint32_t c = 0; c < n_conn; ++c) {
            if (conn_next[c] >= cap && conn_next[c] != QPP_SLOT_NONE) return QPP_E_ARG;
            any_next = any_next || conn_next[c] != QPP_SLOT_NONE;
        }
    }
    if (n_acc) {
        if (!ac->row || !ac->slot || !ac->acc_out || !ac->km_out || !ac->secrets_out || n_acc > (1u << 24))
            return QPP_E_ARG;
        const uint32_t cap = qpp_keytab_capacity(kt);
        for (uint32_t a = 0; a < n_acc; ++a)
            if (ac->row[a] >= n_long || (a && ac->row[a] <= ac->row[a - 1]) || ac->slot[2 * (size_t)a] >= cap ||
                (ac->slot[2 * (size_t)a + 1] >= cap && ac->slot[2 * (size_t)a + 1] != QPP_SLOT_NONE))
                return QPP_E_ARG;
        // pairwise distinct, checked here too: a refusal by
        // qpp_keytab_derive_initial_device would come after the first kernels
        try {
            std::vector<uint32_t> named;
            named.reserve(2 * (size_t)n_acc);
            for (size_t k = 0; k < 2 * (size_t)n_acc; ++k)
                if (ac->slot[k] != QPP_SLOT_NONE) named.push_back(ac->slot[k]);
            std::sort(named.begin(), named.end());
            if (std::adjacent_find(named.begin(), named.end()) != named.end()) return QPP_E_ARG;
        } catch (...) {
            return QPP_E_NOMEM;
        }
    }
    const bool replies = rp && n_acc && rp->reply_flags;
    const bool tokens = tk && n_acc;  // then replies too: QPP_RP_RETRY is set
    if (replies) {
        const bool retry = rp->reply_flags & QPP_RP_RETRY;
        if ((rp->reply_flags & ~(QPP_RP_VN | QPP_RP_RETRY)) || !rp->reply_kt || !rp->rnd || !rp->reply_out ||
            !rp->reply_rec_out || qpp_keytab_capacity(rp->reply_kt) < 3 || !rp->versions || rp->n_versions < 1 ||
            rp->n_versions > QPP_RP_MAX_VERSIONS)
            return QPP_E_ARG;
        if (retry) {
            if (!rp->addr || rp->token_ctr + n_acc < rp->token_ctr) return QPP_E_ARG;
            for (uint32_t a = 0; a < n_acc; ++a) {
                const uint8_t al = rp->addr[(size_t)a * QPP_RP_ADDR_STRIDE];
                if (al != 6 && al != 18) return QPP_E_ARG;
            }
        }
    }
    const uint32_t nd = n + 3u * n_long;  // descriptors and results
    // scratch: [off | len | conn_slot | conn_expected | long_idx | key-set slots | space numbers]
    // go up in one copy, [desc | route | results | walk records | walk counts] come back in one
    const size_t o_len = al256((size_t)n * 8), o_slot = o_len + al256((size_t)n * 4),
                 o_exp = o_slot + al256((size_t)n_conn * 4), o_long = o_exp + al256((size_t)n_conn * 8),
                 o_kslot = o_long + (n_long ? al256((size_t)n_long * 4) : 0),
                 o_kexp = o_kslot + (n_long ? al256((size_t)n_conn * QPP_KEYSETS * 4) : 0),
                 o_arow = o_kexp + (n_long ? al256((size_t)n_conn * QPP_SPACES * 8) : 0),
                 o_aslot = o_arow + (n_acc ? al256((size_t)n_acc * 4) : 0),
                 o_next = o_aslot + (n_acc ? al256((size_t)n_acc * 8) : 0),
                 o_addr = o_next + (any_next ? al256((size_t)n_conn * 4) : 0),
                 o_rand = o_addr + (replies ? al256((size_t)n_acc * QPP_RP_ADDR_STRIDE) : 0),
                 up = o_rand + (replies ? al256((size_t)n_acc * QPP_RP_RAND_STRIDE) : 0);
    const size_t o_route = al256((size_t)nd * sizeof(qpp_desc)),
                 o_res = o_route + al256((size_t)n * sizeof(qpp_route_rec)),
                 o_walk = o_res + al256((size_t)nd * sizeof(qpp_result)),
                 o_walkn = o_walk + (n_long ? al256((size_t)n_long * QPP_WALK_MAX * sizeof(qpp_walk_rec)) : 0),
                 o_acc = o_walkn + (n_long ? al256((size_t)n_long * 4) : 0),
                 o_km = o_acc + (n_acc ? al256((size_t)n_acc * sizeof(qpp_accept_rec)) : 0),
                 o_sec = o_km + (n_acc ? al256((size_t)n_acc * 2 * sizeof(qpp_key_material)) : 0),
                 o_phase = o_sec + (n_acc ? al256((size_t)n_acc * 64) : 0),
                 o_reply = o_phase + (any_next ? al256((size_t)n) : 0),
                 o_rrec = o_reply + (replies ? (size_t)n_acc * QPP_REPLY_STRIDE : 0),
                 o_rres = o_rrec + (replies ? al256((size_t)n_acc * sizeof(qpp_reply_rec)) : 0),
                 o_trec = o_rres + (replies ? al256((size_t)n_acc * 2 * sizeof(qpp_result)) : 0),
                 down = o_trec + (tokens ? al256((size_t)n_acc * sizeof(qpp_token_rec)) : 0);
    // the candidates' qpp_initial records and the reply descriptors (the seals,
    // then the tags) never leave the device: scratch past both copies
    const size_t ini_bytes = n_acc ? al256((size_t)n_acc * sizeof(qpp_initial)) : 0;
    const size_t rdesc_bytes = replies ? al256((size_t)n_acc * 2 * sizeof(qpp_desc)) : 0;
    // nor do the tokens' descriptors, their opened bytes and the results of the launch that opens them
    const size_t tdesc_bytes = tokens ? al256((size_t)n_acc * sizeof(qpp_desc)) : 0;
    const size_t tok_bytes = tokens ? al256((size_t)n_acc * QPP_TOKEN_STRIDE) : 0;
    const size_t tres_bytes = tokens ? al256((size_t)n_acc * sizeof(qpp_result)) : 0;
    qpp_session_bufs b;
    const size_t need = in_len > out_len ? in_len : out_len;
    const size_t device_only = ini_bytes + rdesc_bytes + tdesc_bytes + tok_bytes + tres_bytes;
    int rc = qpp_internal_session_bufs(s, need, nd, up + down + device_only, &b);
    if (rc != QPP_OK) return rc;
    uint8_t *hu = b.h_scratch, *du = b.d_scratch, *hd = b.h_scratch + up, *dd = b.d_scratch + up;
    memcpy(hu, off, (size_t)n * 8);
    memcpy(hu + o_len, len, (size_t)n * 4);
    if (n_conn && !walk_form) {
        memcpy(hu + o_slot, conn_slot, (size_t)n_conn * 4);
        memcpy(hu + o_exp, conn_expected, (size_t)n_conn * 8);
    } else if (n_conn) {
        uint32_t *sl = (uint32_t *)(hu + o_slot);
        uint64_t *ex = (uint64_t *)(hu + o_exp);
        for (uint32_t c = 0; c < n_conn; ++c) {
            sl[c] = conn_slot[(size_t)c * QPP_KEYSETS + QPP_KEYSETS - 1];
            ex[c] = conn_expected[(size_t)c * QPP_SPACES + QPP_SPACES - 1];
        }
    }
    if (n_long) {
        memcpy(hu + o_long, long_idx, (size_t)n_long * 4);
        if (n_conn) {
            memcpy(hu + o_kslot, conn_slot, (size_t)n_conn * QPP_KEYSETS * 4);
            memcpy(hu + o_kexp, conn_expected, (size_t)n_conn * QPP_SPACES * 8);
        }
    }
    if (n_acc) {
        memcpy(hu + o_arow, ac->row, (size_t)n_acc * 4);
        memcpy(hu + o_aslot, ac->slot, (size_t)n_acc * 8);
    }
    if (any_next) memcpy(hu + o_next, conn_next, (size_t)n_conn * 4);
    if (replies) {
        if (rp->addr) memcpy(hu + o_addr, rp->addr, (size_t)n_acc * QPP_RP_ADDR_STRIDE);
        else memset(hu + o_addr, 0, (size_t)n_acc * QPP_RP_ADDR_STRIDE);
        memcpy(hu + o_rand, rp->rnd, (size_t)n_acc * QPP_RP_RAND_STRIDE);
    }
    if (in_len && in != b.h_in) memcpy(b.h_in, in, in_len);  // staged by the caller already?
    HIPCHK(hipMemcpyAsync(du, hu, up, hipMemcpyHostToDevice, b.stream));
    if (in_len) HIPCHK(hipMemcpyAsync(b.d_in, b.h_in, in_len, hipMemcpyHostToDevice, b.stream));
    // bytes the kernels do not write (unrouted datagrams, failed packets) come back as zeros
    if (out_len) HIPCHK(hipMemsetAsync(b.d_out, 0, out_len, b.stream));
    qpp_desc *d_desc = (qpp_desc *)dd;
    qpp_route_rec *d_route = (qpp_route_rec *)(dd + o_route);
    qpp_result *d_res = (qpp_result *)(dd + o_res);
    rc = qpp_route(m, cid_len, (const uint64_t *)du, (const uint32_t *)(du + o_len), n, b.d_in,
                   (const uint32_t *)(du + o_slot), (const uint64_t *)(du + o_exp), n_conn, desc_flags, d_desc,
                   d_route, b.stream);
    if (rc != QPP_OK) return rc;
    if (n_long) {
        rc = qpp_route_walk(cid_len, (const uint64_t *)du, (const uint32_t *)(du + o_len), n, b.d_in, d_route,
                            (const uint32_t *)(du + o_long), n_long, (const uint32_t *)(du + o_kslot),
                            (const uint64_t *)(du + o_kexp), n_conn, desc_flags, d_desc,
                            (qpp_walk_rec *)(dd + o_walk), (uint32_t *)(dd + o_walkn), b.stream);
        if (rc != QPP_OK) return rc;
    }
    if (n_acc) {
        qpp_initial *d_ini = (qpp_initial *)(dd + down);
        if (tokens) {
            // the datagram buffer is only read: a token is part of its Initial's AAD
            qpp_desc *d_tdesc = (qpp_desc *)(dd + down + ini_bytes + rdesc_bytes);
            uint8_t *d_tok = dd + down + ini_bytes + rdesc_bytes + tdesc_bytes;
            qpp_result *d_tres = (qpp_result *)(d_tok + tok_bytes);
            qpp_token_rec *d_trec = (qpp_token_rec *)(dd + o_trec);
            HIPCHK(hipMemsetAsync(d_tok, 0, tok_bytes + tres_bytes, b.stream));
            rc = qpp_route_token((const uint64_t *)du, (const uint32_t *)(du + o_len), n, b.d_in, d_route,
                                 (const uint32_t *)(du + o_long), n_long, (const qpp_walk_rec *)(dd + o_walk),
                                 (const uint32_t *)(dd + o_walkn), (const uint32_t *)(du + o_arow), n_acc, ac->flags,
                                 d_tdesc, d_trec, b.stream);
            if (rc != QPP_OK) return rc;
            rc = qpp_unprotect(rp->reply_kt, d_tdesc, n_acc, b.d_in, d_tok, d_tres, b.stream);
            if (rc != QPP_OK) return rc;
            rc = qpp_route_accept_tokens((const uint64_t *)du, (const uint32_t *)(du + o_len), n, b.d_in, d_route,
                                         (const uint32_t *)(du + o_long), n_long, (const qpp_walk_rec *)(dd + o_walk),
                                         (const uint32_t *)(dd + o_walkn), (const uint32_t *)(du + o_arow),
                                         (const uint32_t *)(du + o_aslot), n_acc, ac->flags, desc_flags, du + o_addr,
                                         d_tok, d_tres, d_ini, d_desc, (qpp_accept_rec *)(dd + o_acc), d_trec,
                                         b.stream);
        } else {
            rc = qpp_route_accept((const uint64_t *)du, (const uint32_t *)(du + o_len), n, b.d_in, d_route,
                                  (const uint32_t *)(du + o_long), n_long, (const qpp_walk_rec *)(dd + o_walk),
                                  (const uint32_t *)(dd + o_walkn), (const uint32_t *)(du + o_arow),
                                  (const uint32_t *)(du + o_aslot), n_acc, ac->flags, desc_flags, d_ini, d_desc,
                                  (qpp_accept_rec *)(dd + o_acc), b.stream);
        }
        if (rc != QPP_OK) return rc;
        if (replies) {
            qpp_desc *d_seal = (qpp_desc *)(dd + down + ini_bytes);
            rc = qpp_route_reply((const uint64_t *)du, (const uint32_t *)(du + o_len), n, b.d_in,
                                 (const uint32_t *)(du + o_long), n_long, (const qpp_walk_rec *)(dd + o_walk),
                                 (const uint32_t *)(du + o_arow), (const qpp_accept_rec *)(dd + o_acc), n_acc,
                                 du + o_addr, du + o_rand, rp->token_ctr, rp->versions, rp->n_versions,
                                 rp->reply_flags, dd + o_reply, d_seal, d_seal + n_acc,
                                 (qpp_reply_rec *)(dd + o_rrec), b.stream);
            if (rc != QPP_OK) return rc;
        }
        // notes every candidate's slots in the table's bookkeeping before the
        // unprotect launch below chooses its kernel form from it
        rc = qpp_keytab_derive_initial_device(ac->kt, d_ini, n_acc, ac->slot, (qpp_key_material *)(dd + o_km),
                                              dd + o_sec, b.stream);
        if (rc != QPP_OK) return rc;
    }
    if (any_next) {
        // the walk's extra descriptors [n, nd) keep the slot they have
        rc = qpp_route_phase(kt, d_route, (const uint32_t *)(du + o_next), n_conn, d_desc, n, b.d_in, dd + o_phase,
                             b.stream);
        if (rc != QPP_OK) return rc;
    }
    rc = qpp_unprotect(kt, d_desc, nd, b.d_in, b.d_out, d_res, b.stream);
    if (rc != QPP_OK) return rc;
    if (replies) {
        // in place in the reply buffer: every token sealed, then every Retry integrity tag
        const qpp_desc *d_seal = (const qpp_desc *)(dd + down + ini_bytes);
        qpp_result *d_rres = (qpp_result *)(dd + o_rres);
        rc = qpp_protect(rp->reply_kt, d_seal, n_acc, dd + o_reply, dd + o_reply, d_rres, b.stream);
        if (rc != QPP_OK) return rc;
        rc = qpp_protect(rp->reply_kt, d_seal + n_acc, n_acc, dd + o_reply, dd + o_reply, d_rres + n_acc, b.stream);
        if (rc != QPP_OK) return rc;
    }
    if (out_len) HIPCHK(hipMemcpyAsync(b.h_out, b.d_out, out_len, hipMemcpyDeviceToHost, b.stream));
    HIPCHK(hipMemcpyAsync(hd, dd, down, hipMemcpyDeviceToHost, b.stream));
    HIPCHK(hipStreamSynchronize(b.stream));
    if (out_len && out != b.h_out) memcpy(out, b.h_out, out_len);
    if (desc_out) memcpy(desc_out, hd, (size_t)nd * sizeof(qpp_desc));
    memcpy(route_out, hd + o_route, (size_t)n * sizeof(qpp_route_rec));
    memcpy(res, hd + o_res, (size_t)nd * sizeof(qpp_result));
    if (n_long) {
        memcpy(walk_out, hd + o_walk, (size_t)n_long * QPP_WALK_MAX * sizeof(qpp_walk_rec));
        memcpy(walk_n_out, hd + o_walkn, (size_t)n_long * 4);
    }
    if (any_next) memcpy(phase_out, hd + o_phase, (size_t)n);
    else if (phase_out) memset(phase_out, 0, (size_t)n);
    if (n_acc) {
        memcpy(ac->acc_out, hd + o_acc, (size_t)n_acc * sizeof(qpp_accept_rec));
        memcpy(ac->km_out, hd + o_km, (size_t)n_acc * 2 * sizeof(qpp_key_material));
        memcpy(ac->secrets_out, hd + o_sec, (size_t)n_acc * 64);
    }
    if (replies) {
        memcpy(rp->reply_out, hd + o_reply, (size_t)n_acc * QPP_REPLY_STRIDE);
        memcpy(rp->reply_rec_out, hd + o_rrec, (size_t)n_acc * sizeof(qpp_reply_rec));
        if (tokens) memcpy(tk->tokrec_out, hd + o_trec, (size_t)n_acc * sizeof(qpp_token_rec));
        // a Retry is whole or it is not sent
        const qpp_result *rres = (const qpp_result *)(hd + o_rres);
        for (uint32_t a = 0; a < n_acc; ++a) {
            qpp_reply_rec &q = rp->reply_rec_out[a];
            if (q.kind != QPP_RP_KIND_RETRY) continue;
            const uint16_t st = rres[a].status != QPP_S_OK ? rres[a].status : rres[n_acc + a].status;
            if (st == QPP_S_OK) continue;
            q.len = 0;
            q.kind = QPP_RP_KIND_NONE;
            q.status = (uint8_t)st;
        }
    }
    return QPP_OK;
}

// no copy into the staging may still be in flight when it is reused
static int settle(qpp_session *s, int rc)
{
    if (rc != QPP_OK && rc != QPP_E_ARG && s) {
        (void)hipStreamSynchronize((hipStream_t)qpp_session_stream(s));
        (void)hipGetLastError();
    }
    return rc;
}

int qpp_session_route_unprotect(qpp_session *s, const qpp_keytab *kt, const qpp_cidmap *m, uint32_t cid_len,
                                const uint64_t *off, const uint32_t *len, uint32_t n, const uint8_t *in,
                                size_t in_len, const uint32_t *conn_slot, const uint64_t *conn_expected,
                                uint32_t n_conn, uint16_t desc_flags, uint8_t *out, size_t out_len,
                                qpp_desc *desc_out, qpp_route_rec *route_out, qpp_result *res)
{
    return settle(s, route_unprotect(s, kt, m, cid_len, off, len, n, in, in_len, false, NULL, 0, conn_slot,
                                     conn_expected, n_conn, desc_flags, out, out_len, desc_out, route_out, res, NULL,
                                     NULL));
}

int qpp_session_route_walk_unprotect(qpp_session *s, const qpp_keytab *kt, const qpp_cidmap *m, uint32_t cid_len,
                                     const uint64_t *off, const uint32_t *len, uint32_t n, const uint8_t *in,
                                     size_t in_len, const uint32_t *long_idx, uint32_t n_long,
                                     const uint32_t *conn_slot, const uint64_t *conn_expected, uint32_t n_conn,
                                     uint16_t desc_flags, uint8_t *out, size_t out_len, qpp_desc *desc_out,
                                     qpp_route_rec *route_out, qpp_result *res, qpp_walk_rec *walk_out,
                                     uint32_t *walk_n_out)
{
    return settle(s, route_unprotect(s, kt, m, cid_len, off, len, n, in, in_len, true, long_idx, n_long, conn_slot,
                                     conn_expected, n_conn, desc_flags, out, out_len, desc_out, route_out, res,
                                     walk_out, walk_n_out));
}

int qpp_session_route_phase_unprotect(qpp_session *s, const qpp_keytab *kt, const qpp_cidmap *m, uint32_t cid_len,
                                      const uint64_t *off, const uint32_t *len, uint32_t n, const uint8_t *in,
                                      size_t in_len, const uint32_t *long_idx, uint32_t n_long,
                                      const uint32_t *conn_slot, const uint64_t *conn_expected, uint32_t n_conn,
                                      const uint32_t *conn_next, uint16_t desc_flags, uint8_t *out, size_t out_len,
                                      qpp_desc *desc_out, qpp_route_rec *route_out, qpp_result *res,
                                      qpp_walk_rec *walk_out, uint32_t *walk_n_out, uint8_t *phase_out)
{
    return settle(s, route_unprotect(s, kt, m, cid_len, off, len, n, in, in_len, true, long_idx, n_long, conn_slot,
                                     conn_expected, n_conn, desc_flags, out, out_len, desc_out, route_out, res,
                                     walk_out, walk_n_out, NULL, conn_next, phase_out));
}

int qpp_session_accept_unprotect(qpp_session *s, qpp_keytab *kt, const qpp_cidmap *m, uint32_t cid_len,
                                 const uint64_t *off, const uint32_t *len, uint32_t n, const uint8_t *in,
                                 size_t in_len, const uint32_t *long_idx, uint32_t n_long,
                                 const uint32_t *conn_slot, const uint64_t *conn_expected, uint32_t n_conn,
                                 uint16_t desc_flags, const uint32_t *acc_row, const uint32_t *acc_slot,
                                 uint32_t n_acc, uint32_t accept_flags, uint8_t *out, size_t out_len,
                                 qpp_desc *desc_out, qpp_route_rec *route_out, qpp_result *res,
                                 qpp_walk_rec *walk_out, uint32_t *walk_n_out, qpp_accept_rec *acc_out,
                                 qpp_key_material *km_out, uint8_t *secrets_out)
{
    const AcceptArgs ac = {kt, acc_row, acc_slot, n_acc, accept_flags, acc_out, km_out, secrets_out};
    return settle(s, route_unprotect(s, kt, m, cid_len, off, len, n, in, in_len, true, long_idx, n_long, conn_slot,
                                     conn_expected, n_conn, desc_flags, out, out_len, desc_out, route_out, res,
                                     walk_out, walk_n_out, &ac));
}

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
                                       uint8_t *reply_out, qpp_reply_rec *reply_rec_out)
{
    const AcceptArgs ac = {kt, acc_row, acc_slot, n_acc, accept_flags, acc_out, km_out, secrets_out};
    const ReplyArgs rp = {reply_kt, addr, rnd, token_ctr, versions, n_versions, reply_flags, reply_out, reply_rec_out};
    return settle(s, route_unprotect(s, kt, m, cid_len, off, len, n, in, in_len, true, long_idx, n_long, conn_slot,
                                     conn_expected, n_conn, desc_flags, out, out_len, desc_out, route_out, res,
                                     walk_out, walk_n_out, &ac, NULL, NULL, &rp));
}

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
                                qpp_reply_rec *reply_rec_out, qpp_token_rec *tokrec_out)
{
    const AcceptArgs ac = {kt, acc_row, acc_slot, n_acc, accept_flags, acc_out, km_out, secrets_out};
    const ReplyArgs rp = {reply_kt, addr, rnd, token_ctr, versions, n_versions, reply_flags, reply_out, reply_rec_out};
    const TokenArgs tk = {tokrec_out};
    return settle(s, route_unprotect(s, kt, m, cid_len, off, len, n, in, in_len, true, long_idx, n_long, conn_slot,
                                     conn_expected, n_conn, desc_flags, out, out_len, desc_out, route_out, res,
                                     walk_out, walk_n_out, &ac, NULL, NULL, &rp, &tk));
}

// qpp_send_fill + qpp_protect on host buffers: the payloads staged at their
// offsets go up with [off | len | conn | seq | sendconn] in the session's own
// scratch, k_send writes headers and padding into the device input, one
// unplanned protect runs from it to the device output at the same offsets, and
// the output comes back with [desc | rec | results].
static int send_protect(qpp_session *s, const qpp_keytab *kt, const qpp_send_conn *sendconn, uint32_t n_conn,
                        const uint64_t *off, const uint32_t *len, const uint32_t *conn, const uint32_t *seq,
                        uint32_t n, const uint8_t *in, size_t in_len, uint8_t *out, size_t out_len,
                        qpp_desc *desc_out, qpp_send_rec *rec_out, qpp_result *res)
{
    if (!s || !kt) return QPP_E_ARG;
    if (n == 0) return QPP_OK;
    if (!off || !len || !conn || !seq || !in || !out || !rec_out || !res || (n_conn && !sendconn)) return QPP_E_ARG;
    static_assert(sizeof(qpp_send_conn) == sizeof(qpp_sn::Conn), "ABI record");
    if (!qpp_sn::batch_ok(reinterpret_cast<const qpp_sn::Conn *>(sendconn), n_conn, qpp_keytab_capacity(kt), off, len,
                          conn, n, in_len, out_len))
        return QPP_E_ARG;
    const size_t o_len = al256((size_t)n * 8), o_conn = o_len + al256((size_t)n * 4),
                 o_seq = o_conn + al256((size_t)n * 4), o_sc = o_seq + al256((size_t)n * 4),
                 up = o_sc + al256((size_t)n_conn * sizeof(qpp_send_conn));
    const size_t o_rec = al256((size_t)n * sizeof(qpp_desc)), o_res = o_rec + al256((size_t)n * sizeof(qpp_send_rec)),
                 down = o_res + al256((size_t)n * sizeof(qpp_result));
    qpp_session_bufs b;
    int rc = qpp_internal_session_bufs(s, in_len > out_len ? in_len : out_len, n, up + down, &b);
    if (rc != QPP_OK) return rc;
    uint8_t *hu = b.h_scratch, *du = b.d_scratch, *hd = b.h_scratch + up, *dd = b.d_scratch + up;
    memcpy(hu, off, (size_t)n * 8);
    memcpy(hu + o_len, len, (size_t)n * 4);
    memcpy(hu + o_conn, conn, (size_t)n * 4);
    memcpy(hu + o_seq, seq, (size_t)n * 4);
    if (n_conn) memcpy(hu + o_sc, sendconn, (size_t)n_conn * sizeof(qpp_send_conn));
    if (in != b.h_in) memcpy(b.h_in, in, in_len);  // staged by the caller already?
    HIPCHK(hipMemcpyAsync(du, hu, up, hipMemcpyHostToDevice, b.stream));
    HIPCHK(hipMemcpyAsync(b.d_in, b.h_in, in_len, hipMemcpyHostToDevice, b.stream));
    // bytes no packet writes (the gaps between the regions) come back as zeros
    HIPCHK(hipMemsetAsync(b.d_out, 0, out_len, b.stream));
    qpp_desc *d_desc = (qpp_desc *)dd;
    qpp_send_rec *d_rec = (qpp_send_rec *)(dd + o_rec);
    qpp_result *d_res = (qpp_result *)(dd + o_res);
    rc = qpp_send_fill(kt, (const qpp_send_conn *)(du + o_sc), n_conn, (const uint64_t *)du,
                       (const uint32_t *)(du + o_len), (const uint32_t *)(du + o_conn),
                       (const uint32_t *)(du + o_seq), n, b.d_in, in_len, d_desc, d_rec, b.stream);
    if (rc != QPP_OK) return rc;
    rc = qpp_protect(kt, d_desc, n, b.d_in, b.d_out, d_res, b.stream);
    if (rc != QPP_OK) return rc;
    HIPCHK(hipMemcpyAsync(b.h_out, b.d_out, out_len, hipMemcpyDeviceToHost, b.stream));
    HIPCHK(hipMemcpyAsync(hd, dd, down, hipMemcpyDeviceToHost, b.stream));
    HIPCHK(hipStreamSynchronize(b.stream));
    if (out != b.h_out) memcpy(out, b.h_out, out_len);
    if (desc_out) memcpy(desc_out, hd, (size_t)n * sizeof(qpp_desc));
    memcpy(rec_out, hd + o_rec, (size_t)n * sizeof(qpp_send_rec));
    memcpy(res, hd + o_res, (size_t)n * sizeof(qpp_result));
    return QPP_OK;
}

int qpp_session_send_protect(qpp_session *s, const qpp_keytab *kt, const qpp_send_conn *sendconn, uint32_t n_conn,
                             const uint64_t *off, const uint32_t *len, const uint32_t *conn, const uint32_t *seq,
                             uint32_t n, const uint8_t *in, size_t in_len, uint8_t *out, size_t out_len,
                             qpp_desc *desc_out, qpp_send_rec *rec_out, qpp_result *res)
{
    return settle(s, send_protect(s, kt, sendconn, n_conn, off, len, conn, seq, n, in, in_len, out, out_len, desc_out,
                                  rec_out, res));
}

}  // extern "C"
