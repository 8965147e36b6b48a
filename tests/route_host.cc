// Host build of aioquic_amd/csrc/qpp_route.h for tests/test_route_host.py: the
// connection-ID map's host mirror (the code qpp_cidmap_* runs), the lookup
// the routing kernel runs over the same buckets, and the datagram
// classification.  Plain g++, no HIP.
#include <stdint.h>
#include <string.h>

#include "../aioquic_amd/csrc/qpp_route.h"

using qpp_rt::HostMap;

namespace {
// the layout of qpp_cid_entry (include/quic_pp.h)
struct CidEntry {
    uint32_t conn;
    uint8_t cid_len;
    uint8_t rsv[3];
    uint8_t cid[20];
    uint32_t rsv2;
};
static_assert(sizeof(CidEntry) == 32, "qpp_cid_entry");

std::vector<HostMap::Entry> entries(const CidEntry *e, uint32_t n)
{
    std::vector<HostMap::Entry> v(n);
    for (uint32_t i = 0; i < n; ++i) v[i] = HostMap::Entry{e[i].conn, e[i].cid_len, e[i].cid};
    return v;
}
}  // namespace

extern "C" {

void *rt_create(uint32_t capacity)
{
    HostMap *m = new HostMap();
    if (!m->init(capacity)) {
        delete m;
        return nullptr;
    }
    return m;
}

void rt_destroy(void *m) { delete (HostMap *)m; }
uint32_t rt_count(void *m) { return ((HostMap *)m)->count; }
uint32_t rt_buckets(void *m) { return ((HostMap *)m)->buckets; }

// 0, or -1 with nothing changed (QPP_E_ARG of qpp_cidmap_put / _remove)
int rt_put(void *m, const void *e, uint32_t n)
{
    if (!e && n) return -1;
    return ((HostMap *)m)->put(entries((const CidEntry *)e, n).data(), n) ? 0 : -1;
}

int rt_remove(void *m, const void *e, uint32_t n)
{
    if (!e && n) return -1;
    return ((HostMap *)m)->remove(entries((const CidEntry *)e, n).data(), n) ? 0 : -1;
}

uint32_t rt_find(void *m, const uint8_t *cid, uint32_t cid_len) { return ((HostMap *)m)->find(cid, cid_len); }
uint32_t rt_home(void *m, const uint8_t *cid, uint32_t cid_len) { return ((HostMap *)m)->home(cid, cid_len); }
// the bucket a CID sits in (0xffffffff: absent)
uint32_t rt_bucket_of(void *m, const uint8_t *cid, uint32_t cid_len)
{
    return ((HostMap *)m)->find_bucket(cid, cid_len);
}

// the table's bytes, 32 per bucket
void rt_dump(void *m, void *out)
{
    HostMap *h = (HostMap *)m;
    memcpy(out, h->tab.data(), (size_t)h->buckets * sizeof(qpp_rt::Bucket));
}

// buckets changed since the last call (the scatter list), then cleared
uint32_t rt_take_dirty(void *m, uint32_t *out, uint32_t max)
{
    HostMap *h = (HostMap *)m;
    uint32_t n = 0;
    for (uint32_t b : h->dirty)
        if (n < max) out[n++] = b;
    h->dirty.clear();
    return n;
}

// What a lane of k_route computes for one datagram over a table given as raw
// bytes (e.g. a copy kept up to date from rt_take_dirty alone): class, conn.
// conn_slot / conn_expected are not consulted here.
uint32_t rt_route_one(const void *tab, uint32_t buckets, uint32_t cid_len, const uint8_t *p, uint32_t len,
                      uint32_t n_conn, uint32_t *conn_out)
{
    uint32_t key_off, key_len;
    uint32_t cls = qpp_rt::classify(p, len, cid_len, &key_off, &key_len);
    uint32_t conn = qpp_rt::kConnNone;
    if (cls != qpp_rt::kMalformed && key_len) {
        uint32_t w[qpp_rt::kCidWords];
        qpp_rt::load_cid(p + key_off, key_len, w);
        const uint32_t b = qpp_rt::lookup((const qpp_rt::Bucket *)tab, buckets, key_len, w);
        if (b != qpp_rt::kConnNone) conn = ((const qpp_rt::Bucket *)tab)[b].conn;
    }
    *conn_out = conn;
    return qpp_rt::settle_class(cls, conn, n_conn);
}

// classify() alone: class, key offset and key length
uint32_t rt_classify(const uint8_t *p, uint32_t len, uint32_t cid_len, uint32_t *key_off, uint32_t *key_len)
{
    return qpp_rt::classify(p, len, cid_len, key_off, key_len);
}

}  // extern "C"
