// Host check of the seeded, evenly grouped window sum of the GCM step loop's
// H^4 multiply (tests/test_gh5_sum_host.py): the groups of
// aioquic_amd/csrc/qpp_gh5.h (kGh5Cut) summed pair by pair from an initial
// accumulator, as gh5_pipeline / Gh5Grp::consume (qpp_device.h) do, give
// init ^ (a ^ b) H^4; and the two-block Gh5In (the xor inside the parity
// masks) equals the one-block constructor on a ^ b.
// A program of its own, so that it also runs under the host sanitizers.
// The table restates k_key_setup (qpp_engine.hip); the reference multiply is
// gf128_mul of the oracle (oracle/qpp_oracle.c, reached through
// tests/gh5_sum_oracle.c).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../aioquic_amd/csrc/qpp_gh5.h"

extern "C" void gh5_sum_gf128(uint8_t x[16], const uint8_t y[16]);  // x *= y, the oracle's gf128_mul

using namespace qpp;

struct Blk {
    uint32_t w[4];  // the 16 bytes as little-endian words, as the kernels load them
};
static bool operator==(const Blk &a, const Blk &b) { return memcmp(a.w, b.w, 16) == 0; }
static Blk operator^(const Blk &a, const Blk &b)
{
    return Blk{{a.w[0] ^ b.w[0], a.w[1] ^ b.w[1], a.w[2] ^ b.w[2], a.w[3] ^ b.w[3]}};
}
static Blk from_hex(const char *s)
{
    uint8_t b[16];
    for (int i = 0; i < 16; ++i) {
        unsigned v;
        sscanf(s + 2 * i, "%2x", &v);
        b[i] = (uint8_t)v;
    }
    Blk r;
    memcpy(r.w, b, 16);
    return r;
}

static Blk gf_ref(const Blk &x, const Blk &y);  // below: through the oracle

// splitmix64
static uint64_t g_rng = 0x243f6a8885a308d3ull;
static uint64_t rnd()
{
    uint64_t z = (g_rng += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static Blk rnd_blk()
{
    const uint64_t a = rnd(), b = rnd();
    return Blk{{(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32)}};
}

static int g_fail = 0;
#define CHECK(c, ...)                  \
    do {                               \
        if (!(c)) {                    \
            if (g_fail++ < 20) {       \
                printf("FAIL: ");      \
                printf(__VA_ARGS__);   \
                printf("\n");          \
            }                          \
        }                              \
    } while (0)

// ---- the groups ------------------------------------------------------------

constexpr bool cuts_ok()
{
    if (kGh5Cut[0] != 0 || kGh5Cut[kGh5Groups] != kGh5Windows) return false;
    for (int g = 0; g < kGh5Groups; ++g) {
        const int n = kGh5Cut[g + 1] - kGh5Cut[g];
        if (n <= 0 || (n & 1)) return false;  // an odd window would take a plain xor of its own
    }
    // two groups' reads are in flight at once, 4 dwords per window: the
    // step loop has 40 VGPRs for them
    for (int g = 0; g + 1 < kGh5Groups; ++g)
        if (4 * (kGh5Cut[g + 2] - kGh5Cut[g]) > 40) return false;
    return true;
}
static_assert(cuts_ok(), "kGh5Cut: even groups that cover the 26 windows, at most 40 dwords in flight");

// ---- the table, as k_key_setup builds it ----------------------------------

typedef std::vector<uint32_t> Table;
static Table build_table(const Blk &power)
{
    Table t(kGh5Bytes / 4, 0xdeadbeefu);  // the rows no window owns stay poisoned
    for (int i = 0; i < kGh5Windows * 32; ++i) {
        const int w = i >> 5;
        const uint32_t e = (uint32_t)(i & 31);
        Blk el;
        gh5_element(w, e, el.w);
        const Blk v = gf_ref(el, power);
        uint32_t *lo = t.data() + gh5_word(w, e), *hi = lo + kGh5Hi / 4;
        lo[0] = v.w[0];
        lo[1] = v.w[1];
        hi[0] = v.w[2];
        hi[1] = v.w[3];
    }
    return t;
}
static Blk entry(const Table &t, int w, uint32_t a)
{
    // the two 8-byte reads of the kernel: row w at byte a, and kGh5Hi further
    const uint8_t *b = (const uint8_t *)t.data();
    Blk r;
    memcpy(&r.w[0], b + w * 256 + a, 8);
    memcpy(&r.w[2], b + kGh5Hi + w * 256 + a, 8);
    return r;
}

template <int w>
static void addrs(const Gh5In &in, uint32_t (&addr)[kGh5Windows])
{
    if constexpr (w < kGh5Windows) {
        addr[w] = gh5_addr<w>(in);
        addrs<w + 1>(in, addr);
    }
}

// The pipeline's sum: the accumulator starts from init; each group adds its
// entries two at a time (x ^ y ^ z per dword, the kernel's xor3), group after
// group.  `pairs` counts the three-input operations per dword.
static Blk sum_groups(const Table &t, const uint32_t (&addr)[kGh5Windows], const Blk &init, int *pairs)
{
    Blk acc = init;
    for (int g = 0; g < kGh5Groups; ++g)
        for (int w = kGh5Cut[g]; w < kGh5Cut[g + 1]; w += 2) {
            const Blk e0 = entry(t, w, addr[w]), e1 = entry(t, w + 1, addr[w + 1]);
            for (int d = 0; d < 4; ++d) acc.w[d] = acc.w[d] ^ e0.w[d] ^ e1.w[d];
            ++*pairs;
        }
    return acc;
}
// init ^ (a ^ b) H^4 as ghash_mul_lds5c(a, b, base, init) forms it
static Blk mul2_seeded(const Table &t, const Blk &a, const Blk &b, const Blk &init)
{
    const Gh5In in(a.w, b.w);
    uint32_t addr[kGh5Windows];
    addrs<0>(in, addr);
    int pairs = 0;
    const Blk r = sum_groups(t, addr, init, &pairs);
    CHECK(pairs == kGh5Windows / 2, "%d pairs per dword, want %d", pairs, kGh5Windows / 2);
    return r;
}
// ... and as ghash_mul_h4(a, b, base, tsel, init) does: windows of a ^ b
static Blk mul2_plain(const Table &t, const Blk &a, const Blk &b, const Blk &init)
{
    const Blk x = a ^ b;
    const unsigned __int128 v = (unsigned __int128)x.w[0] | (unsigned __int128)x.w[1] << 32 |
                                (unsigned __int128)x.w[2] << 64 | (unsigned __int128)x.w[3] << 96;
    uint32_t addr[kGh5Windows];
    for (int w = 0; w < kGh5Windows; ++w) addr[w] = ((uint32_t)(v >> (5 * w)) & 31u) << 3;
    int pairs = 0;
    return sum_groups(t, addr, init, &pairs);
}

static void check_in(const Blk &a, const Blk &b)
{
    const Blk x = a ^ b;
    const Gh5In one(x.w[0], x.w[1], x.w[2], x.w[3]), two(a.w, b.w);
    CHECK(memcmp(one.m, two.m, sizeof one.m) == 0, "Gh5In(a, b) differs from Gh5In(a ^ b): a %08x %08x %08x %08x",
          a.w[0], a.w[1], a.w[2], a.w[3]);
}

static Blk g_h4;
static void check_mul(const Table &t4, const Blk &a, const Blk &b, const Blk &init)
{
    check_in(a, b);
    const Blk want = init ^ gf_ref(a ^ b, g_h4);
    CHECK(mul2_seeded(t4, a, b, init) == want, "seeded sum, masks: a %08x %08x %08x %08x", a.w[0], a.w[1], a.w[2],
          a.w[3]);
    CHECK(mul2_plain(t4, a, b, init) == want, "seeded sum, plain windows: a %08x %08x %08x %08x", a.w[0], a.w[1],
          a.w[2], a.w[3]);
}

// the edge blocks: all zero, all ones, one bit on either side of each window
// boundary (bits 5w - 1 and 5w), each value of the 3-bit window 25
static std::vector<Blk> edge_blocks()
{
    std::vector<Blk> v;
    v.push_back(Blk{{0, 0, 0, 0}});
    v.push_back(Blk{{~0u, ~0u, ~0u, ~0u}});
    for (int w = 0; w < kGh5Windows; ++w)
        for (int bit = 5 * w - 1; bit <= 5 * w; ++bit) {
            if (bit < 0) continue;
            Blk x = {{0, 0, 0, 0}};
            x.w[bit >> 5] = 1u << (bit & 31);
            v.push_back(x);
            // both sides of the boundary at once
            if (bit == 5 * w - 1) {
                x.w[(bit + 1) >> 5] |= 1u << ((bit + 1) & 31);
                v.push_back(x);
            }
        }
    for (uint32_t e = 1; e < 8; ++e) {
        Blk x;
        gh5_element(kGh5Windows - 1, e, x.w);
        v.push_back(x);
        v.push_back(Blk{{~0u, ~0u, ~0u, ~x.w[3]}});
    }
    v.push_back(Blk{{0, 0, 0, 0x80000000u}});  // bit 127, the last of window 25
    return v;
}

// gf128 of the oracle on the blocks' bytes
static Blk gf_ref(const Blk &x, const Blk &y)
{
    uint8_t xb[16], yb[16];
    memcpy(xb, x.w, 16);
    memcpy(yb, y.w, 16);
    gh5_sum_gf128(xb, yb);
    Blk r;
    memcpy(r.w, xb, 16);
    return r;
}

int main()
{
    const std::vector<Blk> edges = edge_blocks();
    // H = E_K(0) of SP 800-38D's AES-GCM test cases 1, 3 and 13
    const char *hs[3] = {"66e94bd4ef8a2c3b884cfa59ca342b2e", "b83b533708bf535d0aa6e52980d53b78",
                         "dc95c078a2408989ad48a21492842087"};
    for (int k = 0; k < 3; ++k) {
        const Blk h = from_hex(hs[k]);
        const Blk h2 = gf_ref(h, h);
        g_h4 = gf_ref(h2, h2);
        const Table t4 = build_table(g_h4);
        for (int i = 0; i < 5000; ++i) check_mul(t4, rnd_blk(), rnd_blk(), rnd_blk());
        const Blk zero = {{0, 0, 0, 0}};
        for (const Blk &e : edges) {
            const Blk r = rnd_blk(), s = rnd_blk();
            check_mul(t4, e, zero, zero);  // the edge block itself
            check_mul(t4, e, zero, r);     // ... under a seed
            check_mul(t4, zero, e, r);     // ... as the addend
            check_mul(t4, r, r ^ e, s);    // ... as the xor of two random blocks
            check_mul(t4, r, s, e);        // ... as the seed
            for (const Blk &f : edges) check_in(e, f);
        }
        // a step's two multiplies, as inner2 chains them
        for (int i = 0; i < 1000; ++i) {
            const Blk acc = rnd_blk(), x0 = rnd_blk(), x1 = rnd_blk();
            const Blk got = mul2_seeded(t4, mul2_seeded(t4, acc, x0, x1), zero, zero);
            CHECK(got == gf_ref(gf_ref(acc ^ x0, g_h4) ^ x1, g_h4), "key %d: the step's chain, triple %d", k, i);
        }
    }
    if (g_fail) {
        printf("gh5_sum_host: %d checks failed\n", g_fail);
        return 1;
    }
    printf("gh5_sum_host: ok\n");
    return 0;
}
