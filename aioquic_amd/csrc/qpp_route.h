// qpp_route.h -- the connection-ID map and the datagram classification of
// qpp_route (quic_pp.h), shared by the host mirror, the routing kernel and a
// plain g++ build (tests/route_host.cc): no HIP type appears here, and the
// qualifiers below vanish outside hipcc.
//
// The map is an open-addressing table of 32-byte buckets with linear probing.
// Only the host ever decides where an entry lives (HostMap, the authoritative
// mirror); the device copy is read-only for the kernel, which runs the same
// lookup() as the host.  Deletion is by backward shift, so the table never
// holds tombstones and a probe sequence never crosses a hole: after any
// sequence of puts and removes every remaining CID is found, and a lookup
// stops at the first empty bucket.  The table is at most half full (buckets
// >= 2 x capacity), so an empty bucket always exists; the probe loop is
// bounded by `buckets` iterations all the same, whatever the memory holds.
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define QPP_HD __host__ __device__
#else
#define QPP_HD
#endif

#include <algorithm>
#include <array>
#include <vector>

namespace qpp_rt {

constexpr uint32_t kConnNone = 0xffffffffu;  // QPP_CONN_NONE
constexpr uint32_t kCidMax = 20;             // QPP_CID_MAX
constexpr uint32_t kCidWords = 5;
constexpr uint32_t kMinBuckets = 16;
constexpr uint32_t kMaxCapacity = 1u << 22;  // 2^23 buckets, 256 MiB

// classes of a datagram (QPP_R_* of quic_pp.h)
constexpr uint32_t kShort = 0, kLong = 1, kUnknownCid = 2, kMalformed = 3, kBadConn = 4;

struct alignas(32) Bucket {
    uint32_t conn;
    uint8_t cid_len;  // 0 = empty
    uint8_t rsv[3];
    uint8_t cid[kCidMax];  // zero-padded past cid_len
    uint32_t pad;
};
static_assert(sizeof(Bucket) == 32, "bucket layout");

// The power of two >= 2 x capacity, at least kMinBuckets.
QPP_HD inline uint32_t buckets_for(uint32_t capacity)
{
    uint32_t b = kMinBuckets;
    while (b < 2u * capacity) b <<= 1;
    return b;
}

// Hash over (cid_len, the five little-endian words of the zero-padded CID):
// a multiply / xor-shift round per word and a closing avalanche.  The CIDs
// are issued by the server itself, so flooding is not a concern.
QPP_HD inline uint32_t hash_cid(uint32_t cid_len, const uint32_t w[kCidWords])
{
    uint32_t h = (cid_len + 1u) * 0x9e3779b1u;
    for (uint32_t k = 0; k < kCidWords; ++k) {
        h ^= w[k];
        h *= 0x85ebca6bu;
        h ^= h >> 15;
    }
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

// The CID's words from bytes (no alignment assumed), zero-padded.  Reads
// exactly p[0 .. cid_len).
QPP_HD inline void load_cid(const uint8_t *p, uint32_t cid_len, uint32_t w[kCidWords])
{
    for (uint32_t k = 0; k < kCidWords; ++k) w[k] = 0;
    for (uint32_t k = 0; k < cid_len && k < kCidMax; ++k) w[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
}

QPP_HD inline void bucket_words(const Bucket &b, uint32_t w[kCidWords])
{
    load_cid(b.cid, kCidMax, w);
}

// Bucket index of (cid_len, w) or kConnNone.  Linear probing from the home
// bucket; a match needs the same length and the same five words; an empty
// bucket ends the search.
QPP_HD inline uint32_t lookup(const Bucket *tab, uint32_t buckets, uint32_t cid_len, const uint32_t w[kCidWords])
{
    if (cid_len == 0 || cid_len > kCidMax) return kConnNone;
    uint32_t b = hash_cid(cid_len, w) & (buckets - 1);
    for (uint32_t it = 0; it < buckets; ++it) {
        const Bucket &e = tab[b];
        if (e.cid_len == 0) return kConnNone;
        if (e.cid_len == cid_len) {
            uint32_t v[kCidWords];
            bucket_words(e, v);
            if (v[0] == w[0] && v[1] == w[1] && v[2] == w[2] && v[3] == w[3] && v[4] == w[4]) return b;
        }
        b = (b + 1) & (buckets - 1);
    }
    return kConnNone;
}

// What a datagram's first bytes say, a pure function of (bytes, len,
// cid_len): kShort (its CID is p[1 .. 1 + cid_len)), kLong (its DCID is
// p[6 .. 6 + *key_len), possibly empty) or kMalformed.  Reads p[0] of a
// non-empty datagram, p[5] of a long header of at least 6 bytes, nothing else.
QPP_HD inline uint32_t classify(const uint8_t *p, uint32_t len, uint32_t cid_len, uint32_t *key_off,
                                uint32_t *key_len)
{
    *key_off = 0;
    *key_len = 0;
    if (len == 0) return kMalformed;
    const uint8_t b0 = p[0];
    if ((b0 & 0xC0) == 0) return kMalformed;  // short header without the fixed bit
    if (!(b0 & 0x80)) {
        if (len < 1 + cid_len) return kMalformed;
        *key_off = 1;
        *key_len = cid_len;
        return kShort;
    }
    // flags(1) version(4) dcid_len(1) dcid (quic/packet.py:181-267)
    if (len < 6) return kMalformed;
    const uint32_t dl = p[5];
    if (dl > kCidMax || len < 6 + dl) return kMalformed;
    *key_off = 6;
    *key_len = dl;
    return kLong;
}

// The class of a datagram once its CID was looked up (conn, or kConnNone): an
// entry whose conn is past the caller's arrays is kBadConn, whatever the
// header form; a short header with no entry is kUnknownCid.
QPP_HD inline uint32_t settle_class(uint32_t cls, uint32_t conn, uint32_t n_conn)
{
    if (conn != kConnNone && conn >= n_conn) return kBadConn;
    if (cls == kShort && conn == kConnNone) return kUnknownCid;
    return cls;
}

// The authoritative host mirror (host code only).  put() and remove() note
// every bucket they change in `dirty` (duplicates possible), for the scatter
// to the device copy.
struct HostMap {
    std::vector<Bucket> tab;
    uint32_t capacity = 0, buckets = 0, count = 0;
    std::vector<uint32_t> dirty;

    struct Entry {  // the fields of a qpp_cid_entry this code needs
        uint32_t conn;
        uint32_t cid_len;
        const uint8_t *cid;
    };

    bool init(uint32_t cap)
    {
        if (cap == 0 || cap > kMaxCapacity) return false;
        capacity = cap;
        buckets = buckets_for(cap);
        tab.assign(buckets, Bucket{});
        count = 0;
        return true;
    }

    uint32_t home(const uint8_t *cid, uint32_t cid_len) const
    {
        uint32_t w[kCidWords];
        load_cid(cid, cid_len, w);
        return hash_cid(cid_len, w) & (buckets - 1);
    }

    uint32_t find_bucket(const uint8_t *cid, uint32_t cid_len) const
    {
        if (cid_len == 0 || cid_len > kCidMax) return kConnNone;
        uint32_t w[kCidWords];
        load_cid(cid, cid_len, w);
        return lookup(tab.data(), buckets, cid_len, w);
    }

    uint32_t find(const uint8_t *cid, uint32_t cid_len) const
    {
        const uint32_t b = find_bucket(cid, cid_len);
        return b == kConnNone ? kConnNone : tab[b].conn;
    }

    static bool lengths_ok(const Entry *e, uint32_t n)
    {
        for (uint32_t i = 0; i < n; ++i)
            if (e[i].cid_len == 0 || e[i].cid_len > kCidMax) return false;
        return true;
    }

    // false (nothing changed): a bad length, or more CIDs than `capacity`
    // after the call.  A CID already present has its conn replaced; the last
    // duplicate inside one call wins.
    bool put(const Entry *e, uint32_t n)
    {
        if (!lengths_ok(e, n)) return false;
        // distinct CIDs of the call that the table does not hold yet
        std::vector<std::array<uint8_t, kCidMax + 1>> fresh;
        for (uint32_t i = 0; i < n; ++i) {
            if (find_bucket(e[i].cid, e[i].cid_len) != kConnNone) continue;
            std::array<uint8_t, kCidMax + 1> k{};
            k[0] = (uint8_t)e[i].cid_len;
            memcpy(&k[1], e[i].cid, e[i].cid_len);
            fresh.push_back(k);
        }
        std::sort(fresh.begin(), fresh.end());
        const size_t add = (size_t)(std::unique(fresh.begin(), fresh.end()) - fresh.begin());
        if (add > (size_t)(capacity - count)) return false;
        for (uint32_t i = 0; i < n; ++i) {
            uint32_t b = find_bucket(e[i].cid, e[i].cid_len);
            if (b == kConnNone) {
                b = home(e[i].cid, e[i].cid_len);
                while (tab[b].cid_len != 0) b = (b + 1) & (buckets - 1);  // count < buckets / 2: ends
                Bucket nb{};
                nb.cid_len = (uint8_t)e[i].cid_len;
                memcpy(nb.cid, e[i].cid, e[i].cid_len);
                tab[b] = nb;
                ++count;
            }
            tab[b].conn = e[i].conn;
            dirty.push_back(b);
        }
        return true;
    }

    // false (nothing changed): a bad length.  An absent CID is ignored.
    // Backward-shift deletion: the entries of the cluster behind the hole move
    // up while that keeps them at or after their home bucket, so no probe
    // sequence ever crosses an empty bucket.  One removal rewrites at most the
    // buckets of its own cluster, an expected O(1) at load <= 1/2.
    bool remove(const Entry *e, uint32_t n)
    {
        if (!lengths_ok(e, n)) return false;
        const uint32_t mask = buckets - 1;
        for (uint32_t i = 0; i < n; ++i) {
            uint32_t hole = find_bucket(e[i].cid, e[i].cid_len);
            if (hole == kConnNone) continue;
            uint32_t j = hole;
            for (uint32_t it = 0; it < buckets; ++it) {
                j = (j + 1) & mask;
                if (tab[j].cid_len == 0) break;
                const uint32_t h = home(tab[j].cid, tab[j].cid_len);
                // movable when its home is not inside (hole, j], cyclically
                if (((j - h) & mask) >= ((j - hole) & mask)) {
                    tab[hole] = tab[j];
                    dirty.push_back(hole);
                    hole = j;
                }
            }
            tab[hole] = Bucket{};
            dirty.push_back(hole);
            --count;
        }
        return true;
    }
};
}  // namespace qpp_rt
