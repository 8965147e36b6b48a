// Host check of aioquic_amd/csrc/qpp_gh5.h (tests/test_ghash5_host.py): the
// window addresses of the close-from-LDS GCM step loop, the 5-bit-window
// table as k_key_setup builds it (gh5_element, gh5_word) multiplied through
// those addresses, and the algebra of the round-12 study:
// an H^8 table built the same way, and a step's two multiplies as the two
// independent products (a ^ x0) H^8 ^ x1 H^4.
// A program of its own, so that it also runs under the host sanitizers.
// The powers restate k_key_setup (qpp_engine.hip); the reference multiply is
// SP 800-38D Algorithm 1, bit by bit.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../aioquic_amd/csrc/qpp_gh5.h"

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

// SP 800-38D sec. 6.3, Algorithm 1 on the blocks' bytes
static Blk gf_ref(const Blk &x, const Blk &y)
{
    uint8_t xb[16], v[16], z[16] = {0};
    memcpy(xb, x.w, 16);
    memcpy(v, y.w, 16);
    for (int i = 0; i < 128; ++i) {
        if ((xb[i >> 3] >> (7 - (i & 7))) & 1)
            for (int k = 0; k < 16; ++k) z[k] ^= v[k];
        const int lsb = v[15] & 1;
        for (int k = 15; k > 0; --k) v[k] = (uint8_t)((v[k] >> 1) | (v[k - 1] << 7));
        v[0] >>= 1;
        if (lsb) v[0] ^= 0xe1;
    }
    Blk r;
    memcpy(r.w, z, 16);
    return r;
}

// splitmix64
static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
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

// ---- 1. every window's address -------------------------------------------

template <int w>
static void check_windows(const Blk &x, uint32_t (&addr)[kGh5Windows])
{
    if constexpr (w < kGh5Windows) {
        const Gh5In in(x.w[0], x.w[1], x.w[2], x.w[3]);
        addr[w] = gh5_addr<w>(in);
        check_windows<w + 1>(x, addr);
    }
}
static void check_addr(const Blk &x)
{
    uint32_t addr[kGh5Windows];
    check_windows<0>(x, addr);
    const unsigned __int128 v = (unsigned __int128)x.w[0] | (unsigned __int128)x.w[1] << 32 |
                                (unsigned __int128)x.w[2] << 64 | (unsigned __int128)x.w[3] << 96;
    for (int w = 0; w < kGh5Windows; ++w) {
        const uint32_t want = ((uint32_t)(v >> (5 * w)) & 31u) << 3;
        CHECK(addr[w] == want, "window %d of %08x %08x %08x %08x: address %u, want %u", w, x.w[0], x.w[1], x.w[2],
              x.w[3], addr[w], want);
    }
}

// ---- 2. the tables, as k_key_setup builds them -----------------------------

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
// x times the table's power through the window addresses
static Blk mul_tab(const Table &t, const Blk &x)
{
    uint32_t addr[kGh5Windows];
    check_windows<0>(x, addr);
    Blk acc = {{0, 0, 0, 0}};
    for (int w = 0; w < kGh5Windows; ++w) acc = acc ^ entry(t, w, addr[w]);
    return acc;
}

int main()
{
    // 1. 10^5 random blocks and the patterns
    for (int i = 0; i < 100000; ++i) check_addr(rnd_blk());
    check_addr(Blk{{0, 0, 0, 0}});
    check_addr(Blk{{~0u, ~0u, ~0u, ~0u}});
    for (int bit = 0; bit < 128; ++bit) {
        Blk x = {{0, 0, 0, 0}};
        x.w[bit >> 5] = 1u << (bit & 31);
        check_addr(x);                                                        // one bit
        check_addr(Blk{{~x.w[0], ~x.w[1], ~x.w[2], ~x.w[3]}});                // all but one
    }
    for (int d = 0; d < 4; ++d) {
        // word boundaries: one word full, its neighbours' edge bits, alternating bits
        Blk x = {{0, 0, 0, 0}};
        x.w[d] = ~0u;
        check_addr(x);
        Blk y = {{0, 0, 0, 0}};
        y.w[d] = 0x80000001u;
        if (d < 3) y.w[d + 1] = 0x00000007u;
        check_addr(y);
        Blk z = {{0xaaaaaaaau, 0x55555555u, 0xaaaaaaaau, 0x55555555u}};
        z.w[d] = ~z.w[d];
        check_addr(z);
    }
    // each window alone full, and each alone empty
    for (int w = 0; w < kGh5Windows; ++w) {
        Blk x;
        gh5_element(w, 31, x.w);
        check_addr(x);
        check_addr(Blk{{~x.w[0], ~x.w[1], ~x.w[2], ~x.w[3]}});
    }

    // 2, 3. three keys: H = E_K(0) of SP 800-38D's AES-GCM test cases 1, 3 and 13
    const char *hs[3] = {"66e94bd4ef8a2c3b884cfa59ca342b2e", "b83b533708bf535d0aa6e52980d53b78",
                         "dc95c078a2408989ad48a21492842087"};
    for (int k = 0; k < 3; ++k) {
        // H^1..H^8 as k_key_setup: four by repeated multiply, then by doubling
        Blk hall[8];
        hall[0] = from_hex(hs[k]);
        for (int p = 1; p < 4; ++p) hall[p] = gf_ref(hall[p - 1], hall[0]);
        for (int t = 0; t < 4; ++t) hall[4 + t] = gf_ref(hall[t], hall[3]);
        const Blk h4 = hall[3], h8 = hall[7];
        CHECK(h8 == gf_ref(h4, h4), "key %d: H^8 is not H^4 squared", k);
        const Table t4 = build_table(h4), t8 = build_table(h8);
        for (int w = 0; w < kGh5Windows; ++w)
            for (uint32_t e = 0; e < 32; ++e) {
                if (w == kGh5Windows - 1 && e >= 8) continue;  // the last window is 3 bits wide
                const Blk want = gf_ref(entry(t4, w, e * 8), h4);
                CHECK(entry(t8, w, e * 8) == want, "key %d: H^8 entry (%d, %u)", k, w, e);
            }
        for (int i = 0; i < 10000; ++i) {
            const Blk a = rnd_blk(), x0 = rnd_blk(), x1 = rnd_blk();
            const Blk chained = mul_tab(t4, mul_tab(t4, a ^ x0) ^ x1);
            const Blk split = mul_tab(t8, a ^ x0) ^ mul_tab(t4, x1);
            CHECK(split == chained, "key %d triple %d: the two products differ from the chain", k, i);
            if (i < 100) CHECK(chained == gf_ref(gf_ref(a ^ x0, h4) ^ x1, h4), "key %d triple %d: table multiply", k, i);
        }
    }
    if (g_fail) {
        printf("ghash5_host: %d checks failed\n", g_fail);
        return 1;
    }
    printf("ghash5_host: ok\n");
    return 0;
}
