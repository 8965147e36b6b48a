// Host build of aioquic_amd/csrc/qpp_token.h for tests/test_token_host.py:
// what every lane of k_token and the token step of k_accept_tokens run.
// Plain g++, no HIP.
//
// Built as a shared object, the functions below are called through ctypes.
// Built as a program (with -fsanitize=address,undefined), main() runs a lane
// over heap buffers of exactly the size it may touch -- a datagram that ends
// where its token ends, every truncation of it, walk records whose lengths
// disagree with the bytes, an opened token of exactly 128 bytes, an address
// record of exactly 20 -- so that a read or write past any of them is the
// sanitizer's to report.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../aioquic_amd/csrc/qpp_token.h"

using qpp_ac::Desc;
typedef qpp_tk::Rec Token;

extern "C" {

// 1 and *start, or 0
int tk_locate(const uint8_t *p, uint32_t len, uint32_t dl, uint32_t sl, uint32_t token_len, uint32_t *start)
{
    return qpp_tk::locate(p, len, dl, sl, token_len, *start) ? 1 : 0;
}

// one candidate from its accept status and the three fields of packet 0's walk record the token needs
uint32_t tk_desc(uint32_t a, uint32_t acc_status, uint32_t accept_flags, uint32_t dcid_len, uint32_t scid_len,
                 uint32_t token_len, uint64_t off, const uint8_t *p, uint32_t len, Desc *d)
{
    qpp_wk::Rec w0;
    memset(&w0, 0, sizeof w0);
    w0.dcid_len = (uint8_t)dcid_len;
    w0.scid_len = (uint8_t)scid_len;
    w0.token_len = (uint16_t)token_len;
    return qpp_tk::token_desc(a, (uint8_t)acc_status, accept_flags, w0, off, len, p, *d);
}

uint32_t tk_check(uint32_t pre, uint32_t res_status, uint32_t token_len, const uint8_t *tok, const uint8_t *addr,
                  Token *rec)
{
    return qpp_tk::check((uint8_t)pre, (uint16_t)res_status, token_len, tok, addr, *rec);
}

}  // extern "C"

namespace {

typedef std::vector<uint8_t> Bytes;

int failures = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("FAILED line %d: %s\n", __LINE__, #c);          \
            ++failures;                                            \
        }                                                          \
    } while (0)

// flags version dl DCID sl SCID, the token's length in the varint form of
// 1 << form bytes, the token: nothing after it
Bytes header(uint32_t dl, uint32_t sl, uint32_t form, uint32_t tl)
{
    Bytes b;
    b.push_back(0xC0);
    for (int k = 3; k >= 0; --k) b.push_back((uint8_t)(qpp_wk::kVersion1 >> (8 * k)));
    b.push_back((uint8_t)dl);
    for (uint32_t k = 0; k < dl; ++k) b.push_back((uint8_t)(0xD0 + k));
    b.push_back((uint8_t)sl);
    for (uint32_t k = 0; k < sl; ++k) b.push_back((uint8_t)(0x50 + k));
    const uint32_t n = 1u << form;
    for (uint32_t k = 0; k < n; ++k)
        b.push_back((uint8_t)((tl >> (8 * (n - 1 - k))) & 0xff) | (k == 0 ? (uint8_t)(form << 6) : 0));
    for (uint32_t k = 0; k < tl; ++k) b.push_back((uint8_t)(0x80 + k));
    return b;
}

uint8_t *exact(const uint8_t *src, size_t n)
{
    uint8_t *p = (uint8_t *)malloc(n ? n : 1);
    if (!p) abort();
    if (n) memcpy(p, src, n);
    return p;
}

// a lane of k_token over a heap copy of exactly the datagram's bytes; the walk
// record's lengths are given apart from the bytes
uint8_t desc_exact(uint32_t a, uint8_t status, uint32_t flags, uint32_t dl, uint32_t sl, uint32_t tl,
                   const uint8_t *src, uint32_t len, uint64_t off, Desc &d)
{
    uint8_t *p = exact(src, len);
    memset(&d, 0x5A, sizeof d);
    qpp_wk::Rec w0;
    memset(&w0, 0, sizeof w0);
    w0.dcid_len = (uint8_t)dl;
    w0.scid_len = (uint8_t)sl;
    w0.token_len = (uint16_t)tl;
    const uint8_t *q = len ? p : p + 1;  // with len == 0 the one allocated byte must not be read either
    const uint8_t st = qpp_tk::token_desc(a, status, flags, w0, off, len, q, d);
    free(p);
    return st;
}

bool inert(const Desc &d, uint32_t a, uint64_t off)
{
    return d.in_off == off && d.out_off == (uint64_t)a * qpp_tk::kStride && d.len == 0 && d.hdr_len == 0 &&
           d.flags == qpp_rp::kNoHp && d.pn == 0 && d.slot == qpp_ac::kSlotNone && d.rsv == 0;
}

// the token step of k_accept_tokens over heap copies of exactly the opened
// token's 128 bytes and the address record's 20
uint8_t check_exact(uint8_t pre, uint16_t res, uint32_t tl, const Bytes &plain, const uint8_t *addr20, Token &rec)
{
    uint8_t tok_src[qpp_tk::kStride];
    memset(tok_src, 0, sizeof tok_src);
    for (size_t k = 0; k < plain.size() && 8 + k < sizeof tok_src; ++k) tok_src[8 + k] = plain[k];
    uint8_t *tok = exact(tok_src, sizeof tok_src), *addr = exact(addr20, qpp_rp::kAddrStride);
    memset(&rec, 0x5A, sizeof rec);
    const uint8_t st = qpp_tk::check(pre, res, tl, tok, addr, rec);
    free(tok), free(addr);
    return st;
}

bool bare(const Token &r, uint8_t status)
{
    const uint8_t *b = (const uint8_t *)&r;
    for (size_t k = 1; k < sizeof r; ++k)
        if (b[k]) return false;
    return r.status == status;
}

}  // namespace

int main()
{
    const uint32_t a = 5, need = qpp_ac::kNeedToken;
    const uint64_t off = 4097;
    Desc d;
    for (uint32_t dl : {1u, 8u, 20u})
        for (uint32_t sl : {0u, 8u, 20u})
            for (uint32_t form : {0u, 1u, 2u})
                for (uint32_t tl : {27u, 52u, 85u, 128u}) {
                    if (form == 0 && tl > 63) continue;
                    const Bytes dg = header(dl, sl, form, tl);
                    const uint32_t full = 7 + dl + sl + (1u << form) + tl;
                    CHECK(dg.size() == full);
                    // the datagram ends where its token ends: located
                    CHECK(desc_exact(a, qpp_ac::kOk, need, dl, sl, tl, dg.data(), full, off, d) == qpp_tk::kOk);
                    CHECK(d.in_off == off + full - tl && d.out_off == (uint64_t)a * qpp_tk::kStride && d.len == tl);
                    CHECK(d.hdr_len == 8 && d.flags == qpp_rp::kNoHp && d.slot == qpp_rp::kSlotToken && d.rsv == 0);
                    CHECK(d.pn == 0x8081828384858687ull);
                    // every truncation, with the whole datagram's record
                    for (uint32_t cut = 0; cut < full; ++cut) {
                        CHECK(desc_exact(a, qpp_ac::kOk, need, dl, sl, tl, dg.data(), cut, off, d) == qpp_tk::kBounds);
                        CHECK(inert(d, a, off));
                    }
                    // a record whose lengths disagree with the bytes
                    for (uint32_t wd = 0; wd <= 21; ++wd)
                        for (uint32_t ws : {0u, 1u, 8u, 20u, 21u, 255u}) {
                            if (wd == dl && ws == sl) continue;
                            CHECK(desc_exact(a, qpp_ac::kOk, need, wd, ws, tl, dg.data(), full, off, d) ==
                                  qpp_tk::kBounds);
                            CHECK(inert(d, a, off));
                        }
                    for (uint32_t wt : {27u, 28u, 127u, 128u}) {
                        if (wt == tl) continue;
                        CHECK(desc_exact(a, qpp_ac::kOk, need, dl, sl, wt, dg.data(), full, off, d) == qpp_tk::kBounds);
                    }
                    // a length outside [27, 128], a status or flags without a token test: nothing is read
                    for (uint32_t wt : {0u, 1u, 26u, 129u, 0xffffu}) {
                        CHECK(desc_exact(a, qpp_ac::kOk, need, dl, sl, wt, dg.data(), 0, off, d) == qpp_tk::kLength);
                        CHECK(inert(d, a, off));
                    }
                    for (uint8_t st : {qpp_ac::kRouted, qpp_ac::kNotInitial, qpp_ac::kVersion, qpp_ac::kSmall,
                                       qpp_ac::kCid, qpp_ac::kNoToken, qpp_ac::kBadToken}) {
                        CHECK(desc_exact(a, st, need, dl, sl, tl, dg.data(), 0, off, d) == qpp_tk::kNone);
                        CHECK(inert(d, a, off));
                    }
                    CHECK(desc_exact(a, qpp_ac::kOk, 0, dl, sl, tl, dg.data(), 0, off, d) == qpp_tk::kNone);
                }
    // the verdict over an opened token of exactly its stride
    uint8_t addr[qpp_rp::kAddrStride];
    memset(addr, 0, sizeof addr);
    for (uint32_t alen : {6u, 18u})
        for (uint32_t ol : {0u, 1u, 20u, 21u})
            for (uint32_t rl : {0u, 8u, 20u, 21u})
                for (uint32_t trail : {0u, 1u, 40u}) {
                    addr[0] = (uint8_t)alen;
                    for (uint32_t k = 1; k < qpp_rp::kAddrStride; ++k) addr[k] = (uint8_t)(0x20 + k);
                    Bytes plain;
                    plain.push_back((uint8_t)alen);
                    for (uint32_t k = 0; k < alen; ++k) plain.push_back(addr[1 + k]);
                    plain.push_back((uint8_t)ol);
                    for (uint32_t k = 0; k < ol; ++k) plain.push_back((uint8_t)(0xA0 + k));
                    plain.push_back((uint8_t)rl);
                    for (uint32_t k = 0; k < rl; ++k) plain.push_back((uint8_t)(0xC0 + k));
                    for (uint32_t k = 0; k < trail; ++k) plain.push_back(0xEE);
                    const uint32_t tl = 8 + (uint32_t)plain.size() + 16;
                    if (tl > qpp_tk::kTokenMax) continue;
                    Token rec;
                    const bool form = ol > 20 || rl > 20;
                    CHECK(check_exact(qpp_tk::kOk, 0, tl, plain, addr, rec) == (form ? qpp_tk::kForm : qpp_tk::kOk));
                    if (form) {
                        CHECK(bare(rec, qpp_tk::kForm));
                    } else {
                        CHECK(rec.status == qpp_tk::kOk && rec.odcid_len == ol && rec.rscid_len == rl);
                        CHECK(memcmp(rec.odcid, plain.data() + 2 + alen, ol) == 0);
                        CHECK(memcmp(rec.rscid, plain.data() + 3 + alen + ol, rl) == 0);
                        // every plaintext that ends early
                        for (uint32_t cut = 3; cut < 3 + alen + ol + rl; ++cut) {
                            const Bytes part(plain.begin(), plain.begin() + cut);
                            CHECK(check_exact(qpp_tk::kOk, 0, 8 + cut + 16, part, addr, rec) == qpp_tk::kForm);
                            CHECK(bare(rec, qpp_tk::kForm));
                        }
                        // another port, another length
                        addr[alen] ^= 1;
                        CHECK(check_exact(qpp_tk::kOk, 0, tl, plain, addr, rec) == qpp_tk::kAddr);
                        addr[alen] ^= 1;
                        addr[0] = (uint8_t)(24 - alen);
                        CHECK(check_exact(qpp_tk::kOk, 0, tl, plain, addr, rec) == qpp_tk::kAddr);
                        CHECK(bare(rec, qpp_tk::kAddr));
                        addr[0] = (uint8_t)alen;
                    }
                    // a launch that said no: no opened byte is read (there are none: a buffer of one byte)
                    for (uint16_t res : {1, 2, 3, 4, 5}) {
                        uint8_t *none = (uint8_t *)malloc(1), *ad = exact(addr, sizeof addr);
                        if (!none) abort();
                        CHECK(qpp_tk::check(qpp_tk::kOk, res, tl, none + 1, ad, rec) == qpp_tk::kAuth);
                        CHECK(bare(rec, qpp_tk::kAuth));
                        free(none), free(ad);
                    }
                    // a preliminary status that is not kOk stays, and nothing is read
                    for (uint8_t pre : {qpp_tk::kNone, qpp_tk::kLength, qpp_tk::kBounds}) {
                        uint8_t *none = (uint8_t *)malloc(1);
                        if (!none) abort();
                        CHECK(qpp_tk::check(pre, 0, tl, none + 1, none + 1, rec) == pre && bare(rec, pre));
                        free(none);
                    }
                }
    if (failures) return 1;
    printf("token_host: ok\n");
    return 0;
}
