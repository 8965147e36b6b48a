// qpp_batch.h -- the arithmetic of a host batch (qpp_session's bounds check
// and pipeline tiling, qpp_multi's range split; qpp_session.hip) as functions
// over plain arrays.  Plain C++17, nothing of HIP, so that
// tests/session_host.cc checks it on the CPU.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/quic_pp.h"

namespace qpp {

// Descriptor flag set by the host session for a descriptor whose extents do
// not fit the caller's buffers: the packet reports QPP_S_LENGTH and no byte
// of it is read or written.
constexpr uint32_t kFlagReject = 0x8000u;

// Host batches of at least 2 x kPipeChunkBytes of output go through the
// session as a three-stage pipeline of up to kPipeMaxChunks chunks (see
// session_run_pipelined): up to kPipeRegular chunks of about equal size, the
// first and last of them cut into quarter, quarter and half (kPipeTaper) so
// the pipeline fills and drains on small pieces.
constexpr size_t kPipeChunkBytes = (size_t)32 << 20;
constexpr int kPipeRegular = 32, kPipeTaper = 2;
constexpr int kPipeMaxChunks = kPipeRegular + 2 * kPipeTaper;
constexpr int kMultiMaxDevices = 16;  // qpp_multi: devices per host-batch engine

// Bytes a packet reads at in_off and writes at out_off: protect reads header
// + payload and writes header + ciphertext + tag; unprotect reads and writes
// at most the packet's length.
struct DescSpan {
    uint64_t rd, wr;
};
inline DescSpan desc_span(bool enc, const qpp_desc &d)
{
    const uint64_t rd = enc ? (uint64_t)d.hdr_len + d.len : (uint64_t)d.len;
    return DescSpan{rd, enc ? rd + QPP_TAG_LEN : rd};
}

// Descriptor extents against the caller's buffer sizes (quic_pp.h, Buffers):
// a descriptor that does not fit is flagged so the kernel reports
// QPP_S_LENGTH for it without touching memory.
inline void reject_out_of_bounds(bool enc, qpp_desc *d, uint32_t n, size_t in_len, size_t out_len)
{
    for (uint32_t i = 0; i < n; ++i) {
        const DescSpan sp = desc_span(enc, d[i]);
        const bool ok = d[i].in_off <= in_len && sp.rd <= in_len - d[i].in_off && d[i].out_off <= out_len &&
                        sp.wr <= out_len - d[i].out_off;
        d[i].flags = ok ? (uint16_t)(d[i].flags & ~kFlagReject) : (uint16_t)(d[i].flags | kFlagReject);
    }
}

// ------------------------------------------------------------- pipeline --

// Regular chunks of a batch's pipeline, or 0 for the serial path: one per
// kPipeChunkBytes of output, at most kPipeRegular and at most one per packet,
// at least two, and only with out_off non-decreasing in descriptor order (the
// chunks' output tiles then follow one another).
inline int pipe_chunks(const qpp_desc *desc, uint32_t n, size_t out_len)
{
    const size_t want = out_len / kPipeChunkBytes;
    int chunks = want > (size_t)kPipeRegular ? kPipeRegular : (int)want;
    if (chunks > (int)n) chunks = (int)n;
    if (chunks < 2) return 0;
    for (uint32_t i = 1; i < n; ++i)
        if (desc[i].out_off < desc[i - 1].out_off) return 0;
    return chunks;
}

// The pipeline's chunks: chunk c takes packets [first[c], first[c + 1]) and
// returns output bytes [olo[c], olo[c + 1]) -- from its first packet's
// out_off to the next chunk's, chunk 0 from 0 and the last to out_len, so the
// tiles cover the output, and bytes a packet writes past its tile belong to a
// later chunk's.
struct PipeTiling {
    int chunks;
    uint32_t first[kPipeMaxChunks + 1];
    size_t olo[kPipeMaxChunks + 1];
};
inline void pipe_tiling(const qpp_desc *desc, uint32_t n, size_t out_len, int regular, PipeTiling &t)
{
    // chunk weights in quarters of a regular chunk: 1, 1, 2 at the start and
    // 2, 1, 1 at the end when there are enough regular chunks to taper
    const bool taper = regular >= 8;
    const int chunks = t.chunks = taper ? regular + 2 * kPipeTaper : regular;
    auto weight = [&](int c) -> uint64_t {
        if (!taper) return 4;
        if (c < 3) return c < 2 ? 1 : 2;
        if (c >= chunks - 3) return c >= chunks - 2 ? 1 : 2;
        return 4;
    };
    const uint64_t wsum = 4ull * (uint64_t)regular;
    uint64_t wacc = 0;
    for (int c = 0; c <= chunks; ++c) {
        t.first[c] = (uint32_t)((uint64_t)n * wacc / wsum);
        if (c < chunks) wacc += weight(c);
        t.olo[c] = c == 0 ? 0 : c == chunks ? out_len : (size_t)desc[t.first[c]].out_off;
        if (t.olo[c] > out_len) t.olo[c] = out_len;
    }
}

// A byte range [lo, hi); empty when lo >= hi.
struct Extent {
    size_t lo, hi;
};

// Input bytes of a chunk's packets d[a, b) (bounds-checked descriptors): the
// span of those that fit, each to 16 bytes past its end, capped at in_len
// (over-copying bytes of a neighbour is harmless: same host bytes).
inline Extent pipe_chunk_input(const qpp_desc *d, uint32_t a, uint32_t b, size_t in_len)
{
    size_t lo = SIZE_MAX, hi = 0;
    for (uint32_t i = a; i < b; ++i) {
        if (d[i].flags & kFlagReject) continue;
        const size_t o = (size_t)d[i].in_off;
        const size_t e = o + (size_t)d[i].hdr_len + d[i].len + 16;
        if (o < lo) lo = o;
        if (e > hi) hi = e;
    }
    if (hi > in_len) hi = in_len;
    return Extent{lo, hi};
}

// ------------------------------------------------------ several devices --

// A device's share of a qpp_multi batch: packets [b, e) and the input and
// output extents of those that fit (all zero when none does).
struct MultiRange {
    uint32_t b, e;
    size_t ilo, ihi, olo, ohi;
};

// The batch's bounds-checked descriptors d[0, n) cut into contiguous ranges,
// one per device and at most one per packet.  Each range needs its own output
// extent: ranges in output order with disjoint extents -- every non-empty
// range starts at or after the end of all earlier non-empty ones (an empty
// range, every packet rejected, compares with nothing) -- or one range of the
// whole batch and buffers, for one device.
inline std::vector<MultiRange> multi_split(bool enc, const qpp_desc *d, uint32_t n, int devices, size_t in_len,
                                           size_t out_len)
{
    const int parts = devices < (int)n ? devices : (int)n;
    std::vector<MultiRange> r(parts);
    for (int k = 0; k < parts; ++k) {
        MultiRange &x = r[k];
        x.b = (uint32_t)((uint64_t)n * k / parts);
        x.e = (uint32_t)((uint64_t)n * (k + 1) / parts);
        x.ilo = x.olo = SIZE_MAX;
        x.ihi = x.ohi = 0;
        for (uint32_t i = x.b; i < x.e; ++i) {
            if (d[i].flags & kFlagReject) continue;
            const DescSpan sp = desc_span(enc, d[i]);
            if (d[i].in_off < x.ilo) x.ilo = (size_t)d[i].in_off;
            if (d[i].in_off + sp.rd > x.ihi) x.ihi = (size_t)(d[i].in_off + sp.rd);
            if (d[i].out_off < x.olo) x.olo = (size_t)d[i].out_off;
            if (d[i].out_off + sp.wr > x.ohi) x.ohi = (size_t)(d[i].out_off + sp.wr);
        }
        if (x.ilo == SIZE_MAX) x.ilo = x.ihi = x.olo = x.ohi = 0;
    }
    size_t seen_hi = 0;
    bool seen = false;
    for (int k = 0; k < parts; ++k) {
        if (r[k].ohi <= r[k].olo) continue;
        if (seen && seen_hi > r[k].olo) return {MultiRange{0, n, 0, in_len, 0, out_len}};
        if (r[k].ohi > seen_hi) seen_hi = r[k].ohi;
        seen = true;
    }
    return r;
}

// Each range's descriptors rebased onto its extents; a rejected one is put
// past every range buffer, so that the range's session rejects it again.
inline void multi_rebase(qpp_desc *d, const std::vector<MultiRange> &r)
{
    for (const MultiRange &x : r)
        for (uint32_t i = x.b; i < x.e; ++i) {
            if (d[i].flags & kFlagReject) {
                d[i].in_off = d[i].out_off = ~0ull;
                continue;
            }
            d[i].in_off -= x.ilo;
            d[i].out_off -= x.olo;
        }
}

// Output bytes outside every range's extent (zeros, as one session leaves them).
inline std::vector<Extent> multi_gaps(const std::vector<MultiRange> &r, size_t out_len)
{
    std::vector<Extent> gaps;
    size_t pos = 0;
    for (const MultiRange &x : r) {
        if (x.ohi <= x.olo) continue;
        if (x.olo > pos) gaps.push_back(Extent{pos, x.olo});
        pos = x.ohi;
    }
    if (out_len > pos) gaps.push_back(Extent{pos, out_len});
    return gaps;
}

}  // namespace qpp
