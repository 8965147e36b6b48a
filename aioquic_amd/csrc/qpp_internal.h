// qpp_internal.h -- library-internal interfaces between the translation units
// of libquicpp.so (not part of the C ABI).
#pragma once

#include <hip/hip_runtime.h>
#include <stdlib.h>

#include "qpp_batch.h"
#include "qpp_device.h"

#define HIPCHK(x)                          \
    do {                                   \
        if ((x) != hipSuccess) {           \
            (void)hipGetLastError();       \
            return QPP_E_HIP;              \
        }                                  \
    } while (0)

// The one way the library reads an environment switch: the variable's integer
// value, or dflt when it is unset or empty.  Every switch is a product or
// test switch that some test drives (tests/test_switches.py keeps the list).
static inline long qpp_env_long(const char *name, long dflt)
{
    const char *v = getenv(name);
    return (v && *v) ? atol(v) : dflt;
}

// A batch's bucketing (quic_pp.h, qpp_plan_*): device buffers for n <= cap.
struct qpp_plan {
    uint32_t cap;
    uint32_t n_built;            // packets of the last qpp_plan_build
    uint32_t *d_keys[2];         // sort keys (bucket << slot_bits | slot), in / out
    uint32_t *d_idx[2];          // packet indices, in / sorted
    qpp_desc *d_sorted;          // descriptors gathered into bucket order (rsv = caller index)
    uint32_t *d_count;           // [0, 4): packets per bucket; [8, 16): d_range; [16, 24): d_irange;
                                 // [24]: wave items in all
    uint32_t *d_range;           // [begin, end) per bucket: AES-128, AES-256, ChaCha20, no key
    // Wave items: runs of <= 16 sorted positions on one key slot, so that no
    // wave of a packet kernel (16 packets, 4 lanes each) straddles two slots.
    // item i = positions [d_items[i], d_items[i + 1]); d_items[total] = n.
    uint32_t *d_flags;           // 1 where a position starts an item
    uint32_t *d_pos;             // exclusive scan of d_flags: item index of a head
    uint32_t *d_items;           // item start positions (+ the sentinel n)
    uint32_t *d_irange;          // [begin, end) of each bucket's items
    void *d_tmp;                 // rocPRIM temporary storage
    size_t tmp_bytes;
    // Counting-sort path (tables of <= kPlanCountSlots slots): one bin per
    // sort key, 4 << slot_bits bins.
    uint32_t *d_bins;            // per-key counts, then the scatter cursors
    uint32_t *d_posoff;          // first sorted position of each key's run
    uint32_t *d_itmoff;          // first wave item of each key's run
};

// Tables up to this many slots bucket by a counting sort over (suite, slot)
// keys; larger ones by the rocPRIM radix sort.
constexpr uint32_t kPlanCountSlots = 4096;

int qpp_internal_plan_build(qpp_plan *p, const qpp::KeySlot *d_slots, uint32_t cap,
                            const qpp_desc *d_desc, uint32_t n, hipStream_t s);
int qpp_internal_plan_gather(const qpp_plan *p, const qpp_desc *d_desc, uint32_t n, hipStream_t s);
// wave items of a batch of n packets on a table of `cap` slots, at most
uint32_t qpp_internal_plan_max_items(uint32_t n, uint32_t cap);
int qpp_internal_plan_nokey(const qpp_plan *p, qpp_result *d_res, hipStream_t s);

// ---- qpp_engine.hip, for the sessions (qpp_session.hip; qpp_keytab stays
// opaque to them) ----

namespace qpp {

constexpr int kLoneWG = 1024;      // 16 packets per workgroup, one AES image

// A small host call handed to a lone kernel whole (qpp_session): the kernel
// copies the call's descriptors and input from the pinned staging (src, its
// device view) into the device staging (dst) itself, every thread 16 bytes
// in one bus round trip, instead of a copy-engine blit scheduled between
// stream operations.  bytes == 0: nothing staged (device-buffer launches).
// One workgroup (at most 16 packets); the workgroup barrier makes the copy
// visible to its waves (vector L1 writes through to L2).
struct LoneStage {
    const uint8_t *src;
    uint8_t *dst;
    uint32_t bytes;  // multiple of 16, <= kLoneStageMax
};
constexpr uint32_t kLoneStageMax = 2 * kLoneWG * 16;

}  // namespace qpp

// qpp_protect / qpp_unprotect (enc), over a plan's sorted descriptors when
// plan is given (qpp_*_planned), staged by the lone kernel when stage is
int qpp_internal_launch_packets(bool enc, const qpp_keytab *kt, const qpp_desc *d_desc, uint32_t n,
                                const uint8_t *d_in, uint8_t *d_out, qpp_result *d_res, void *stream,
                                const qpp_plan *plan = nullptr, const qpp::LoneStage *stage = nullptr);
// Up to how many packets an unplanned launch takes the lone kernels whatever
// the suite (0: never, QPP_LONE=0).
uint32_t qpp_internal_lone_limit();
// D2H of a session: up to two device ranges (s0, s1) into pinned host memory
// (device views d0, d1), by k_xfer.
int qpp_internal_launch_xfer(uint8_t *d0, const uint8_t *s0, size_t n0, uint8_t *d1, const uint8_t *s1,
                             size_t n1, hipStream_t st);

// ---- qpp_session.hip ----

// A session's buffers for a caller in another translation unit
// (qpp_session_route_unprotect): the staging reserved for `bytes` of input and
// of output and `packets` packets, as qpp_session_stage does, and `scratch`
// bytes of pinned (h_scratch) and device (d_scratch) memory of the session
// that no other call uses.  Valid until the next call on the session.
struct qpp_session_bufs {
    hipStream_t stream;
    uint8_t *h_in, *h_out, *d_in, *d_out;
    uint8_t *h_scratch, *d_scratch;
};
int qpp_internal_session_bufs(qpp_session *s, size_t bytes, uint32_t packets, size_t scratch,
                              qpp_session_bufs *out);
