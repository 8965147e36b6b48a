// qpp_route.hip -- routing received datagrams to connections by connection ID
// on the device (quic_pp.h: qpp_cidmap_*, qpp_route, qpp_session_route_unprotect).
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
#include <new>
#include <stdlib.h>
#include <string.h>

#include "quic_pp.h"
#include "qpp_internal.h"
#include "qpp_route.h"

using qpp_rt::Bucket;
using qpp_rt::HostMap;

static_assert(sizeof(qpp_cid_entry) == 32 && sizeof(qpp_route_rec) == 8 && sizeof(qpp_desc) == 40, "ABI records");
static_assert(QPP_R_SHORT == qpp_rt::kShort && QPP_R_LONG == qpp_rt::kLong &&
              QPP_R_UNKNOWN_CID == qpp_rt::kUnknownCid && QPP_R_MALFORMED == qpp_rt::kMalformed &&
              QPP_R_BAD_CONN == qpp_rt::kBadConn && QPP_CONN_NONE == qpp_rt::kConnNone, "route classes");

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

static int route_unprotect(qpp_session *s, const qpp_keytab *kt, const qpp_cidmap *m, uint32_t cid_len,
                           const uint64_t *off, const uint32_t *len, uint32_t n, const uint8_t *in, size_t in_len,
                           const uint32_t *conn_slot, const uint64_t *conn_expected, uint32_t n_conn,
                           uint16_t desc_flags, uint8_t *out, size_t out_len, qpp_desc *desc_out,
                           qpp_route_rec *route_out, qpp_result *res)
{
    if (!s || !kt || !m || cid_len < 1 || cid_len > QPP_CID_MAX) return QPP_E_ARG;
    if (n == 0) return QPP_OK;
    if (!off || !len || !route_out || !res || (in_len && !in) || (out_len && !out) ||
        (n_conn && (!conn_slot || !conn_expected)))
        return QPP_E_ARG;
    // the caller's own arrays: every datagram inside both buffers, or nothing runs
    for (uint32_t i = 0; i < n; ++i)
        if (off[i] > in_len || len[i] > in_len - off[i] || off[i] > out_len || len[i] > out_len - off[i])
            return QPP_E_ARG;
    // scratch: [off | len | conn_slot | conn_expected] go up in one copy,
    // [desc | route | results] come back in one
    const size_t o_len = al256((size_t)n * 8), o_slot = o_len + al256((size_t)n * 4),
                 o_exp = o_slot + al256((size_t)n_conn * 4), up = o_exp + al256((size_t)n_conn * 8);
    const size_t o_route = al256((size_t)n * sizeof(qpp_desc)), o_res = o_route + al256((size_t)n * sizeof(qpp_route_rec)),
                 down = o_res + al256((size_t)n * sizeof(qpp_result));
    qpp_session_bufs b;
    const size_t need = in_len > out_len ? in_len : out_len;
    int rc = qpp_internal_session_bufs(s, need, n, up + down, &b);
    if (rc != QPP_OK) return rc;
    uint8_t *hu = b.h_scratch, *du = b.d_scratch, *hd = b.h_scratch + up, *dd = b.d_scratch + up;
    memcpy(hu, off, (size_t)n * 8);
    memcpy(hu + o_len, len, (size_t)n * 4);
    if (n_conn) {
        memcpy(hu + o_slot, conn_slot, (size_t)n_conn * 4);
        memcpy(hu + o_exp, conn_expected, (size_t)n_conn * 8);
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
    rc = qpp_unprotect(kt, d_desc, n, b.d_in, b.d_out, d_res, b.stream);
    if (rc != QPP_OK) return rc;
    if (out_len) HIPCHK(hipMemcpyAsync(b.h_out, b.d_out, out_len, hipMemcpyDeviceToHost, b.stream));
    HIPCHK(hipMemcpyAsync(hd, dd, down, hipMemcpyDeviceToHost, b.stream));
    HIPCHK(hipStreamSynchronize(b.stream));
    if (out_len && out != b.h_out) memcpy(out, b.h_out, out_len);
    if (desc_out) memcpy(desc_out, hd, (size_t)n * sizeof(qpp_desc));
    memcpy(route_out, hd + o_route, (size_t)n * sizeof(qpp_route_rec));
    memcpy(res, hd + o_res, (size_t)n * sizeof(qpp_result));
    return QPP_OK;
}

int qpp_session_route_unprotect(qpp_session *s, const qpp_keytab *kt, const qpp_cidmap *m, uint32_t cid_len,
                                const uint64_t *off, const uint32_t *len, uint32_t n, const uint8_t *in,
                                size_t in_len, const uint32_t *conn_slot, const uint64_t *conn_expected,
                                uint32_t n_conn, uint16_t desc_flags, uint8_t *out, size_t out_len,
                                qpp_desc *desc_out, qpp_route_rec *route_out, qpp_result *res)
{
    const int rc = route_unprotect(s, kt, m, cid_len, off, len, n, in, in_len, conn_slot, conn_expected, n_conn,
                                   desc_flags, out, out_len, desc_out, route_out, res);
    if (rc != QPP_OK && rc != QPP_E_ARG && s) {
        // no copy into the staging may still be in flight when it is reused
        (void)hipStreamSynchronize((hipStream_t)qpp_session_stream(s));
        (void)hipGetLastError();
    }
    return rc;
}

}  // extern "C"
