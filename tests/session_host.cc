// Host check of the host batch path's HIP-free parts (tests/test_session_host.py):
// aioquic_amd/csrc/qpp_hostcopy.h -- the non-temporal copy, the copy pool and
// its groups, par_memcpy -- and aioquic_amd/csrc/qpp_batch.h -- the bounds
// check, the pipeline's chunk count, tiling and input extents, and qpp_multi's
// range split.  A program of its own, so that it also runs under the host
// sanitizers (address + undefined behaviour, and thread).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/wait.h>
#include <unistd.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "../aioquic_amd/csrc/qpp_batch.h"
#include "../aioquic_amd/csrc/qpp_hostcopy.h"

using namespace qpp;

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            printf("session_host: %s:%d: %s\n", __FILE__, __LINE__, #x); \
            exit(1);                                                    \
        }                                                               \
    } while (0)

static uint64_t g_rng = 0x243f6a8885a308d3ull;
static uint64_t rnd()  // splitmix64
{
    uint64_t z = (g_rng += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// ---------------------------------------------------------------- copies --

constexpr size_t kMiB = (size_t)1 << 20;
constexpr size_t kGuard = 64;
static const size_t kSizes[] = {0, 1, 31, 32, 33, 65535, 65536, 65537, 65663, 8 * kMiB - 1, 8 * kMiB, 8 * kMiB + 65,
                                40 * kMiB + 3};
constexpr int kNumSizes = sizeof(kSizes) / sizeof(kSizes[0]);
constexpr size_t kMaxSize = 40 * kMiB + 3;

// A destination of n bytes at misalignment mis past a 64-byte boundary, with
// kGuard guard bytes on each side.
struct Dest {
    std::vector<uint8_t> mem;
    uint8_t *p = nullptr;
    size_t n = 0;
    void prepare(size_t bytes, size_t mis)
    {
        n = bytes;
        if (mem.size() < bytes + 2 * kGuard + 128) mem.resize(bytes + 2 * kGuard + 128);
        uint8_t *base = (uint8_t *)(((uintptr_t)mem.data() + 63) & ~(uintptr_t)63);
        p = base + kGuard + mis;
        memset(p - kGuard, 0xa5, kGuard);
        memset(p, 0, n);
        memset(p + n, 0xa5, kGuard);
    }
    void verify(const uint8_t *src) const
    {
        CHECK(memcmp(p, src, n) == 0);
        for (size_t i = 0; i < kGuard; ++i) CHECK(p[-(ptrdiff_t)kGuard + (ptrdiff_t)i] == 0xa5 && p[n + i] == 0xa5);
    }
};

static void test_copies()
{
    std::vector<uint8_t> srcmem(kMaxSize + 128);
    uint8_t *sbase = (uint8_t *)(((uintptr_t)srcmem.data() + 63) & ~(uintptr_t)63);
    for (size_t i = 0; i + 8 <= kMaxSize + 64; i += 8) {
        const uint64_t v = rnd();
        memcpy(sbase + i, &v, 8);
    }
    Dest d[4];
    // four outstanding copies per group, a pooled one (>= 8 MiB) in each
    static const int kBatches[4][4] = {{0, 1, 2, 9}, {3, 4, 5, 10}, {6, 7, 8, 11}, {12, 0, 4, 8}};
    for (size_t dmis : {(size_t)0, (size_t)1, (size_t)31})
        for (size_t smis : {(size_t)0, (size_t)7}) {
            const uint8_t *src = sbase + smis;
            for (int k = 0; k < kNumSizes; ++k) {
                d[0].prepare(kSizes[k], dmis);
                copy_bytes(d[0].p, src, kSizes[k]);
                d[0].verify(src);
                d[0].prepare(kSizes[k], dmis);
                par_memcpy(d[0].p, src, kSizes[k]);
                d[0].verify(src);
            }
            for (const auto &batch : kBatches) {
                CopyGroup g;
                for (int j = 0; j < 4; ++j) {
                    d[j].prepare(kSizes[batch[j]], dmis);
                    par_memcpy(d[j].p, src, d[j].n, &g);
                }
                g.wait();
                CHECK(g.busy_ns.load() > 0);
                for (int j = 0; j < 4; ++j) d[j].verify(src);
            }
        }
}

// ------------------------------------------------------- pool life cycle --

static bool pooled_copy_matches(uint8_t seed)
{
    const size_t n = 9 * kMiB;
    std::vector<uint8_t> a(n), b(n, 0);
    for (size_t i = 0; i < n; i += 8) {
        const uint64_t v = (i + seed) * 0x9e3779b97f4a7c15ull;
        memcpy(a.data() + i, &v, 8);
    }
    par_memcpy(b.data(), a.data(), n);
    return memcmp(a.data(), b.data(), n) == 0;
}

static void test_pool_life_cycle(bool with_fork)
{
    // a group on the stack that goes out of scope right after wait(): no
    // worker may touch it once wait() has seen pending == 0
    uint8_t src[3][64], dst[3][64];
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 64; ++i) src[j][i] = (uint8_t)(j * 64 + i);
    for (int round = 0; round < 20000; ++round) {
        CopyGroup g;
        for (int j = 0; j < 3; ++j) CopyPool::get().submit(dst[j], src[j], 64, &g);
        g.wait();
    }
    CHECK(memcmp(dst, src, sizeof src) == 0);
    // two callers on the pool at once
    bool ok[2] = {true, true};
    std::thread th[2];
    for (int t = 0; t < 2; ++t)
        th[t] = std::thread([&ok, t] {
            for (int k = 0; k < 20; ++k) ok[t] = ok[t] && pooled_copy_matches((uint8_t)(t * 20 + k));
        });
    for (auto &t : th) t.join();
    CHECK(ok[0] && ok[1]);
    // a forked child inherits the pool's pointer but not its threads
    if (with_fork) {
        CHECK(pooled_copy_matches(99));
        fflush(stdout);
        const pid_t pid = fork();
        CHECK(pid >= 0);
        if (pid == 0) _exit(pooled_copy_matches(7) ? 0 : 1);
        int status = 0;
        CHECK(waitpid(pid, &status, 0) == pid);
        CHECK(WIFEXITED(status) && WEXITSTATUS(status) == 0);
    }
}

// ---------------------------------------------------------------- bounds --

static qpp_desc make_desc(uint64_t in_off, uint64_t out_off, uint32_t len, uint16_t hdr_len, uint16_t flags = 0)
{
    qpp_desc d;
    memset(&d, 0, sizeof d);
    d.in_off = in_off;
    d.out_off = out_off;
    d.len = len;
    d.hdr_len = hdr_len;
    d.flags = flags;
    return d;
}

static bool rejected(bool enc, qpp_desc d, size_t in_len, size_t out_len)
{
    const uint16_t other = (uint16_t)(d.flags & ~kFlagReject);
    reject_out_of_bounds(enc, &d, 1, in_len, out_len);
    CHECK((uint16_t)(d.flags & ~kFlagReject) == other);  // every other flag bit survives
    return (d.flags & kFlagReject) != 0;
}

static void test_bounds()
{
    // an empty read at the very end of the input
    CHECK(!rejected(false, make_desc(100, 0, 0, 0), 100, 100));
    CHECK(rejected(false, make_desc(101, 0, 0, 0), 100, 100));
    for (bool enc : {true, false}) {
        const uint32_t tag = enc ? QPP_TAG_LEN : 0;
        // protect: rd = 10 + 50, wr = rd + 16; unprotect: rd = wr = 50
        const uint64_t rd = enc ? 60 : 50, wr = rd + tag;
        const uint64_t in_off = 40, out_off = 24;
        CHECK(desc_span(enc, make_desc(0, 0, 50, 10)).rd == rd && desc_span(enc, make_desc(0, 0, 50, 10)).wr == wr);
        CHECK(!rejected(enc, make_desc(in_off, out_off, 50, 10), in_off + rd, out_off + wr));
        CHECK(rejected(enc, make_desc(in_off, out_off, 50, 10), in_off + rd - 1, out_off + wr));
        CHECK(rejected(enc, make_desc(in_off, out_off, 50, 10), in_off + rd, out_off + wr - 1));
        // the tag counts on the write side only: the input holds no room for it
        CHECK(!rejected(enc, make_desc(in_off, out_off, 50, 10), in_off + rd, 1000));
        // no wrap-around
        CHECK(rejected(enc, make_desc(~0ull, 0, 1, 1), 1000, 1000));
        CHECK(rejected(enc, make_desc(0, ~0ull, 1, 1), 1000, 1000));
        CHECK(rejected(enc, make_desc(~0ull, ~0ull, 0, 0), SIZE_MAX, SIZE_MAX - 1));
        CHECK(rejected(enc, make_desc(8, 8, 0xffffffffu, 0xffffu), (size_t)1 << 32, (size_t)1 << 33));
        CHECK(rejected(enc, make_desc(8, 8, 0xffffffffu, 0xffffu), (size_t)1 << 33, (size_t)1 << 32));
        CHECK(!rejected(enc, make_desc(8, 8, 0xffffffffu, 0xffffu), (size_t)1 << 33, (size_t)1 << 33));
        // a stale reject flag is cleared when the descriptor fits; other bits stay
        qpp_desc d = make_desc(0, 0, 20, 4, (uint16_t)(kFlagReject | 0x7fffu));
        reject_out_of_bounds(enc, &d, 1, 100, 100);
        CHECK(d.flags == 0x7fffu);
        d = make_desc(0, 0, 200, 4, 0x1234u);
        reject_out_of_bounds(enc, &d, 1, 100, 100);
        CHECK(d.flags == (uint16_t)(0x1234u | kFlagReject));
    }
}

// ---------------------------------------------------------------- tiling --

// n protect descriptors with out_off non-decreasing: runs of equal offsets,
// gaps, the last few past out_len, and a middle block whose input does not fit.
static std::vector<qpp_desc> tiling_descs(uint32_t n, size_t &in_len, size_t &out_len)
{
    std::vector<qpp_desc> d(n);
    uint64_t in = 0, out = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t len = 20 + (uint32_t)(rnd() % 1200);
        const uint16_t hdr = (uint16_t)(5 + rnd() % 30);
        const unsigned kind = (unsigned)(rnd() % 8);
        if (kind == 0) out += rnd() % 5000;          // a gap
        d[i] = make_desc(in, out, len, hdr);
        in += hdr + len;
        if (kind != 1) out += hdr + len + QPP_TAG_LEN;  // else: the next packet at the same offset
    }
    in_len = (size_t)in;
    const uint32_t tail = n >= 8 ? n / 8 : 1;        // the last packets start past out_len
    out_len = d[n - tail].out_off ? (size_t)d[n - tail].out_off - 1 : 0;
    for (uint32_t i = n / 2; i < n / 2 + n / 8 + 1 && i < n; ++i) d[i].in_off = in_len + 5;
    return d;
}

static int g_all_rejected_chunks = 0, g_tapered = 0;

static void test_tiling_case(uint32_t n, int regular)
{
    size_t in_len, out_len;
    const std::vector<qpp_desc> desc = tiling_descs(n, in_len, out_len);
    PipeTiling t;
    pipe_tiling(desc.data(), n, out_len, regular, t);
    // the taper: exactly when there are >= 8 regular chunks
    const bool taper = regular >= 8;
    CHECK(t.chunks == (taper ? regular + 4 : regular) && t.chunks <= kPipeMaxChunks);
    g_tapered += taper;
    // brute force: the chunk's weights in quarters, summed
    std::vector<uint64_t> w((size_t)t.chunks, 4);
    if (taper) {
        w[0] = w[1] = w[(size_t)t.chunks - 1] = w[(size_t)t.chunks - 2] = 1;
        w[2] = w[(size_t)t.chunks - 3] = 2;
    }
    uint64_t total = 0;
    for (uint64_t x : w) total += x;
    CHECK(total == 4ull * (uint64_t)regular);
    uint64_t acc = 0;
    for (int c = 0; c <= t.chunks; ++c) {
        const uint32_t f = (uint32_t)((uint64_t)n * acc / total);
        CHECK(t.first[c] == f);
        size_t o = c == 0 ? 0 : c == t.chunks ? out_len : (size_t)std::min<uint64_t>(desc[f].out_off, out_len);
        CHECK(t.olo[c] == o);
        if (c < t.chunks) acc += w[(size_t)c];
    }
    CHECK(t.first[0] == 0 && t.first[t.chunks] == n && t.olo[0] == 0 && t.olo[t.chunks] == out_len);
    for (int c = 0; c < t.chunks; ++c)
        CHECK(t.first[c] <= t.first[c + 1] && t.olo[c] <= t.olo[c + 1] && t.olo[c + 1] <= out_len);
    std::vector<qpp_desc> hd = desc;
    reject_out_of_bounds(true, hd.data(), n, in_len, out_len);
    for (int c = 0; c < t.chunks; ++c) {
        const Extent x = pipe_chunk_input(hd.data(), t.first[c], t.first[c + 1], in_len);
        bool any = false;
        for (uint32_t i = t.first[c]; i < t.first[c + 1]; ++i) {
            if (hd[i].flags & kFlagReject) continue;
            any = true;
            CHECK(hd[i].out_off >= t.olo[c]);
            CHECK(x.lo <= hd[i].in_off && hd[i].in_off + desc_span(true, hd[i]).rd <= x.hi);
        }
        CHECK(any ? x.lo < x.hi && x.hi <= in_len : !(x.lo < x.hi));
        if (!any && t.first[c] < t.first[c + 1]) ++g_all_rejected_chunks;
    }
}

static void test_tiling()
{
    for (uint32_t n : {2u, 3u, 7u, 8u, 9u, 35u, 36u, 37u, 1000u})
        for (int chunks = 2; chunks <= (int)std::min<uint32_t>(n, 32); ++chunks) test_tiling_case(n, chunks);
    CHECK(g_all_rejected_chunks > 0 && g_tapered > 0);
    // the chunk count
    std::vector<qpp_desc> d(1000, make_desc(0, 0, 100, 10));
    for (uint32_t i = 0; i < 1000; ++i) d[i].out_off = (uint64_t)i * 126;
    CHECK(pipe_chunks(d.data(), 1000, 64 * kMiB - 1) == 0);
    CHECK(pipe_chunks(d.data(), 1000, 64 * kMiB) == 2);
    CHECK(pipe_chunks(d.data(), 1000, 33 * 32 * kMiB) == kPipeRegular);
    CHECK(pipe_chunks(d.data(), 3, 33 * 32 * kMiB) == 3);
    CHECK(pipe_chunks(d.data(), 1, 33 * 32 * kMiB) == 0);
    d[500].out_off = d[499].out_off;  // equal: still non-decreasing
    CHECK(pipe_chunks(d.data(), 1000, 64 * kMiB) == 2);
    d[500].out_off = d[499].out_off - 1;
    CHECK(pipe_chunks(d.data(), 1000, 64 * kMiB) == 0);
    CHECK(pipe_chunks(d.data(), 500, 64 * kMiB) == 2);  // the descending one is past this batch
}

// ----------------------------------------------------------- multi split --

// The invariants of a split of d (unchecked descriptors) over `devices`;
// returns the number of ranges.
static size_t check_split(bool enc, const std::vector<qpp_desc> &desc, int devices, size_t in_len, size_t out_len)
{
    const uint32_t n = (uint32_t)desc.size();
    std::vector<qpp_desc> d = desc;
    reject_out_of_bounds(enc, d.data(), n, in_len, out_len);
    const std::vector<MultiRange> r = multi_split(enc, d.data(), n, devices, in_len, out_len);
    if (r.size() == 1) {
        if (std::min<uint32_t>((uint32_t)devices, n) > 1)  // one device: the whole batch and buffers
            CHECK(r[0].b == 0 && r[0].e == n && r[0].ilo == 0 && r[0].ihi == in_len && r[0].olo == 0 &&
                  r[0].ohi == out_len);
        return 1;
    }
    CHECK(r.size() == std::min<size_t>((size_t)devices, n));
    CHECK(r.front().b == 0 && r.back().e == n);
    for (size_t k = 0; k + 1 < r.size(); ++k) CHECK(r[k].e == r[k + 1].b && r[k].b < r[k].e);
    // output extents pairwise disjoint
    for (size_t a = 0; a < r.size(); ++a)
        for (size_t b = a + 1; b < r.size(); ++b)
            if (r[a].ohi > r[a].olo && r[b].ohi > r[b].olo) CHECK(r[a].ohi <= r[b].olo || r[b].ohi <= r[a].olo);
    // rebased packets lie inside their range's extents
    std::vector<qpp_desc> rb = d;
    multi_rebase(rb.data(), r);
    for (const MultiRange &x : r) {
        CHECK(x.ihi <= in_len && x.ohi <= out_len);
        for (uint32_t i = x.b; i < x.e; ++i) {
            if (d[i].flags & kFlagReject) {
                CHECK(rb[i].in_off == ~0ull && rb[i].out_off == ~0ull);
                continue;
            }
            const DescSpan sp = desc_span(enc, d[i]);
            CHECK(rb[i].in_off == d[i].in_off - x.ilo && rb[i].out_off == d[i].out_off - x.olo);
            CHECK(rb[i].in_off + sp.rd <= x.ihi - x.ilo && rb[i].out_off + sp.wr <= x.ohi - x.olo);
        }
        // and the range's own session accepts exactly the same packets
        std::vector<qpp_desc> again(rb.begin() + x.b, rb.begin() + x.e);
        reject_out_of_bounds(enc, again.data(), x.e - x.b, x.ihi - x.ilo, x.ohi - x.olo);
        for (uint32_t i = x.b; i < x.e; ++i) CHECK(again[i - x.b].flags == d[i].flags);
    }
    // the zeroed gaps and the extents tile [0, out_len)
    std::vector<Extent> tiles = multi_gaps(r, out_len);
    for (const Extent &g : tiles) CHECK(g.lo < g.hi);
    for (const MultiRange &x : r)
        if (x.ohi > x.olo) tiles.push_back(Extent{x.olo, x.ohi});
    std::sort(tiles.begin(), tiles.end(), [](const Extent &a, const Extent &b) { return a.lo < b.lo; });
    size_t pos = 0;
    for (const Extent &e : tiles) {
        CHECK(e.lo == pos);
        pos = e.hi;
    }
    CHECK(pos == out_len);
    return r.size();
}

// n packets laid out one after another, the output `lead` bytes in and with
// a gap after every third packet
static std::vector<qpp_desc> socket_batch(bool enc, uint32_t n, size_t lead, size_t &in_len, size_t &out_len)
{
    std::vector<qpp_desc> d;
    uint64_t in = 0, out = lead;
    for (uint32_t i = 0; i < n; ++i) {
        d.push_back(make_desc(in, out, 60 + 7 * i, (uint16_t)(9 + i % 5)));
        const DescSpan sp = desc_span(enc, d.back());
        in += sp.rd;
        out += sp.wr + (i % 3 == 2 ? 40 : 0);
    }
    in_len = (size_t)in;
    out_len = (size_t)out + 11;
    return d;
}

static void test_multi_split()
{
    for (bool enc : {true, false}) {
        size_t in_len, out_len;
        // parts = min(devices, n)
        std::vector<qpp_desc> d = socket_batch(enc, 10, 7, in_len, out_len);
        CHECK(check_split(enc, d, 4, in_len, out_len) == 4);
        CHECK(check_split(enc, d, 10, in_len, out_len) == 10);
        CHECK(check_split(enc, d, 16, in_len, out_len) == 10);  // n < devices
        d = socket_batch(enc, 2, 0, in_len, out_len);
        CHECK(check_split(enc, d, 4, in_len, out_len) == 2);
        d = socket_batch(enc, 1, 3, in_len, out_len);
        CHECK(check_split(enc, d, 4, in_len, out_len) == 1);
        // overlapping output extents: one device
        d = socket_batch(enc, 9, 7, in_len, out_len);
        d[3].out_off = d[2].out_off + 1;  // range 1's first packet inside range 0's extent
        CHECK(check_split(enc, d, 3, in_len, out_len) == 1);
        // an all-rejected middle range compares with nothing
        d = socket_batch(enc, 9, 7, in_len, out_len);
        for (int i = 3; i < 6; ++i) d[i].in_off = in_len + 1;
        CHECK(check_split(enc, d, 3, in_len, out_len) == 3);
        d[4].in_off = ~0ull;
        d[5].out_off = ~0ull;
        CHECK(check_split(enc, d, 3, in_len, out_len) == 3);
        // every packet rejected: nothing overlaps, the gaps cover the output
        for (auto &x : d) x.in_off = in_len + 1;
        CHECK(check_split(enc, d, 3, in_len, out_len) == 3);
        // ranges out of output order: one device
        d = socket_batch(enc, 8, 0, in_len, out_len);
        for (int i = 0; i < 4; ++i) std::swap(d[i].out_off, d[i + 4].out_off);
        CHECK(check_split(enc, d, 2, in_len, out_len) == 1);
        // ... but out of order inside one range only is that range's business
        d = socket_batch(enc, 8, 0, in_len, out_len);
        std::swap(d[0].out_off, d[1].out_off);
        d[0].len = d[1].len = 60;
        CHECK(check_split(enc, d, 2, in_len, out_len + 64) == 2);
    }
}

int main()
{
    test_bounds();
    test_tiling();
    test_multi_split();
    test_copies();
#if defined(__SANITIZE_THREAD__)
    test_pool_life_cycle(false);  // (no thread starts after a multithreaded fork under ThreadSanitizer)
#else
    test_pool_life_cycle(true);
#endif
    printf("session_host: ok\n");
    return 0;
}
