// qpp_session.hip -- the host-buffer path of the C ABI: qpp_session (pinned
// staging, the small-call forms, the chunked pipeline) and qpp_multi (one
// host batch over several devices).  Host code only: it defines no kernel and
// reaches the key table and the kernels through quic_pp.h and qpp_internal.h
// (qpp_keytab is opaque here).  Its arithmetic -- bounds, tiling, the range
// split -- is qpp_batch.h and its host copies qpp_hostcopy.h, both checked on
// the CPU by tests/session_host.cc.
#include <hip/hip_runtime.h>

#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <thread>
#include <vector>

#include "qpp_hostcopy.h"
#include "qpp_internal.h"

using namespace qpp;

struct qpp_session {
    hipStream_t stream;             // kernels (and everything of the serial path)
    hipStream_t s_in, s_out;        // pipelined path: H2D and D2H copy streams
    hipEvent_t ev_in[kPipeMaxChunks], ev_k[kPipeMaxChunks], ev_out[kPipeMaxChunks];
    int device;
    size_t max_bytes;
    uint32_t max_packets;
    uint8_t *h_in, *h_out, *h_misc;  // pinned
    uint8_t *hd_in, *hd_out, *hd_misc;  // their device views (zero-copy small calls)
    uint8_t *d_in, *d_out, *d_misc;
    size_t misc_bytes;
    qpp_plan *plan;                  // bucketing of batches of >= kSessionPlanMin packets
    // qpp_session_trace: timing events around every chunk's H2D, kernels and
    // D2H (start / end), created on first enable; the last traced call
    bool trace;
    hipEvent_t tev[6][kPipeMaxChunks];
    qpp_trace last;
    // qpp_session_route_unprotect (qpp_route.hip): the small arrays of a routed
    // batch, apart from the staging above, which a caller may have filled
    uint8_t *h_scratch, *d_scratch;  // pinned / device
    size_t scratch_bytes;
};

// Host batches of at least this many packets are bucketed by (suite, slot)
// on the device before launch (qpp_plan); smaller ones launch as given.
constexpr uint32_t kSessionPlanMin = 128;

// Small host calls on the lone-packet kernels (and small header-protection
// mask calls) read and write the session's pinned staging from the kernel
// instead of through two copy-engine blits (~3.8 us each plus their
// scheduling, profiles/r4j_lone_latency); QPP_ZERO_COPY=0 keeps the copies
// (a study and test switch, read once per process).
static bool zero_copy_choice()
{
    static const bool b = qpp_env_long("QPP_ZERO_COPY", 1) != 0;
    return b;
}

// A small host call of one workgroup's packets staged by the lone kernel
// itself instead of a copy (QPP_LONE_STAGE=0: the copy; a study and test
// switch, read once per process).
static bool lone_stage_choice()
{
    static const bool b = qpp_env_long("QPP_LONE_STAGE", 1) != 0;
    return b;
}

static void session_free_buffers(qpp_session *s)
{
    if (s->h_in) (void)hipHostFree(s->h_in);
    if (s->h_out) (void)hipHostFree(s->h_out);
    if (s->h_misc) (void)hipHostFree(s->h_misc);
    if (s->d_in) (void)hipFree(s->d_in);
    if (s->d_out) (void)hipFree(s->d_out);
    if (s->d_misc) (void)hipFree(s->d_misc);
    s->h_in = s->h_out = s->h_misc = s->d_in = s->d_out = s->d_misc = NULL;
    s->hd_in = s->hd_out = s->hd_misc = NULL;
}

static size_t misc_bytes_for(uint32_t max_packets)
{
    // descriptors + results + slot ids + samples + masks
    return (size_t)max_packets * (sizeof(qpp_desc) + sizeof(qpp_result) + 4 + 16 + 16) + 256;
}

// A batch's descriptors and results in the misc buffers: max_packets
// descriptors, then the results; pinned (h), device (d), and the pinned
// results' device view (hrd).
struct SessionMisc {
    qpp_desc *hd, *dd;
    qpp_result *hr, *dr, *hrd;
};
static SessionMisc session_misc(const qpp_session *s)
{
    const size_t off = (size_t)s->max_packets * sizeof(qpp_desc);
    return SessionMisc{(qpp_desc *)s->h_misc, (qpp_desc *)s->d_misc, (qpp_result *)(s->h_misc + off),
                       (qpp_result *)(s->d_misc + off), (qpp_result *)(s->hd_misc + off)};
}

static int session_reserve(qpp_session *s, size_t bytes, uint32_t packets)
{
    if (bytes <= s->max_bytes && packets <= s->max_packets && s->h_in) return QPP_OK;
    size_t nb = bytes > s->max_bytes ? bytes : s->max_bytes;
    uint32_t np = packets > s->max_packets ? packets : s->max_packets;
    if (nb < 4096) nb = 4096;
    if (np < 64) np = 64;
    session_free_buffers(s);
    s->max_bytes = nb;
    s->max_packets = np;
    s->misc_bytes = misc_bytes_for(np);
    if (hipHostMalloc(&s->h_in, nb, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc(&s->h_out, nb, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc(&s->h_misc, s->misc_bytes, hipHostMallocDefault) != hipSuccess ||
        hipMalloc(&s->d_in, nb) != hipSuccess || hipMalloc(&s->d_out, nb) != hipSuccess ||
        hipMalloc(&s->d_misc, s->misc_bytes) != hipSuccess ||
        hipHostGetDevicePointer((void **)&s->hd_in, s->h_in, 0) != hipSuccess ||
        hipHostGetDevicePointer((void **)&s->hd_out, s->h_out, 0) != hipSuccess ||
        hipHostGetDevicePointer((void **)&s->hd_misc, s->h_misc, 0) != hipSuccess) {
        (void)hipGetLastError();
        session_free_buffers(s);
        s->max_bytes = 0;
        s->max_packets = 0;
        return QPP_E_NOMEM;
    }
    return QPP_OK;
}

int qpp_session_create(size_t max_bytes, uint32_t max_packets, qpp_session **out)
{
    if (!out) return QPP_E_ARG;
    *out = NULL;
    int rc = qpp_device_check();
    if (rc != QPP_OK) return rc;
    qpp_session *s = (qpp_session *)calloc(1, sizeof(qpp_session));
    if (!s) return QPP_E_NOMEM;
    (void)hipGetDevice(&s->device);
    if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) {
        free(s);
        return QPP_E_HIP;
    }
    bool ok = hipStreamCreateWithFlags(&s->s_in, hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(&s->s_out, hipStreamNonBlocking) == hipSuccess;
    for (int c = 0; ok && c < kPipeMaxChunks; ++c)
        ok = hipEventCreateWithFlags(&s->ev_in[c], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&s->ev_k[c], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&s->ev_out[c], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        qpp_session_destroy(s);
        return QPP_E_HIP;
    }
    rc = session_reserve(s, max_bytes, max_packets);
    if (rc != QPP_OK) {
        qpp_session_destroy(s);
        return rc;
    }
    *out = s;
    return QPP_OK;
}

void qpp_session_destroy(qpp_session *s)
{
    if (!s) return;
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    if (s->s_in) (void)hipStreamSynchronize(s->s_in);
    if (s->s_out) (void)hipStreamSynchronize(s->s_out);
    session_free_buffers(s);
    if (s->h_scratch) (void)hipHostFree(s->h_scratch);
    if (s->d_scratch) (void)hipFree(s->d_scratch);
    qpp_plan_destroy(s->plan);
    for (int c = 0; c < kPipeMaxChunks; ++c) {
        if (s->ev_in[c]) (void)hipEventDestroy(s->ev_in[c]);
        if (s->ev_k[c]) (void)hipEventDestroy(s->ev_k[c]);
        if (s->ev_out[c]) (void)hipEventDestroy(s->ev_out[c]);
        for (int k = 0; k < 6; ++k)
            if (s->tev[k][c]) (void)hipEventDestroy(s->tev[k][c]);
    }
    if (s->s_in) (void)hipStreamDestroy(s->s_in);
    if (s->s_out) (void)hipStreamDestroy(s->s_out);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    free(s);
}

void *qpp_session_stream(qpp_session *s) { return s ? (void *)s->stream : NULL; }

// One launch over n device descriptors of the session: bucketed by (suite,
// slot) through the session's plan when the batch is large enough.
static int session_launch(bool enc, qpp_session *s, const qpp_keytab *kt, const qpp_desc *dd,
                          uint32_t n, qpp_result *dr)
{
    if (n < kSessionPlanMin) return qpp_internal_launch_packets(enc, kt, dd, n, s->d_in, s->d_out, dr, s->stream);
    if (s->plan && s->plan->cap < n) {
        HIPCHK(hipStreamSynchronize(s->stream));  // the old plan may still be in use
        qpp_plan_destroy(s->plan);
        s->plan = NULL;
    }
    if (!s->plan) {
        const int rc = qpp_plan_create(n > s->max_packets ? n : s->max_packets, &s->plan);
        if (rc != QPP_OK) return rc;
    }
    int rc = qpp_plan_build(s->plan, kt, dd, n, s->stream);
    if (rc == QPP_OK)
        rc = enc ? qpp_protect_planned(kt, s->plan, dd, n, s->d_in, s->d_out, dr, s->stream)
                 : qpp_unprotect_planned(kt, s->plan, dd, n, s->d_in, s->d_out, dr, s->stream);
    return rc;
}

// Large host batches: chunk c of the packets (in descriptor order, tiled by
// pipe_tiling, qpp_batch.h) has its descriptors copied into pinned staging
// and bounds-checked by the host, its input extent copied into pinned staging
// by the copy pool, and both go H2D on s_in (the copy engines); the chunk's
// kernels run on the kernel stream once that lands; its output tile and
// results go D2H on s_out (k_xfer, which runs beside the packet kernels:
// profiles/r5g_d2h_engines.txt), and the pool copies them out while later
// chunks are in flight.  So host copies, both PCIe directions and the
// kernels of different chunks overlap, and no work on the whole batch
// precedes the first chunk's copies.  (Round 5 also built DMA straight from / to
// caller memory pinned by hipHostRegister: correct, but 9.6-10.7 GiB/s
// against 17-19 GiB/s for this staged pipeline on the same boxes whatever
// the flags and D2H form, so it was removed; profiles/r5e_host_path/.)
static int session_run_pipelined(bool enc, qpp_session *s, const qpp_keytab *kt,
                                 const qpp_desc *desc, uint32_t n, const uint8_t *in,
                                 size_t in_len, uint8_t *out, size_t out_len, qpp_result *res, int regular)
{
    const SessionMisc m = session_misc(s);
    const bool tr = s->trace;
    const auto clk = [] { return std::chrono::duration<double, std::milli>(
                              std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_start = clk();
    double t_copy_in = 0.0;
    double in_bytes = 0.0, out_bytes = 0.0;
    // the caller may have assembled its input / wants its output in the
    // session's own staging (qpp_session_stage): no host copy then
    const bool in_direct = in == s->h_in, out_direct = out == s->h_out;
    HIPCHK(hipMemsetAsync(s->d_out, 0, out_len, s->stream));
    PipeTiling t;
    pipe_tiling(desc, n, out_len, regular, t);
    const int chunks = t.chunks;
    const uint32_t *first = t.first;
    const size_t *olo = t.olo;
    // a chunk handed back to the caller: its output tile and results, copied
    // out by the pool while this thread goes on staging later chunks
    CopyGroup outg;
    struct WaitAll {
        CopyGroup &g;
        ~WaitAll() { g.wait(); }  // every return path: no pool copy outlives the call
    } wait_all{outg};
    auto hand_back = [&](int d) {
        if (olo[d + 1] > olo[d] && !out_direct)
            par_memcpy(out + olo[d], s->h_out + olo[d], olo[d + 1] - olo[d], &outg);
        memcpy(res + first[d], m.hr + first[d], (size_t)(first[d + 1] - first[d]) * sizeof(qpp_result));
    };
    int rc = QPP_OK;
    int next_out = 0;
    for (int c = 0; c < chunks; ++c) {
        const uint32_t a = first[c], b = first[c + 1];
        hipStream_t sin = s->s_in;
        memcpy(m.hd + a, desc + a, (size_t)(b - a) * sizeof(qpp_desc));
        reject_out_of_bounds(enc, m.hd + a, b - a, in_len, out_len);
        if (tr) HIPCHK(hipEventRecord(s->tev[0][c], sin));
        if (b > a)
            HIPCHK(hipMemcpyAsync(m.dd + a, m.hd + a, (size_t)(b - a) * sizeof(qpp_desc), hipMemcpyHostToDevice, sin));
        const Extent x = pipe_chunk_input(m.hd, a, b, in_len);
        if (x.lo < x.hi) {
            if (!in_direct) {
                const double t0 = tr ? clk() : 0.0;
                par_memcpy(s->h_in + x.lo, in + x.lo, x.hi - x.lo);
                if (tr) t_copy_in += clk() - t0;
            }
            HIPCHK(hipMemcpyAsync(s->d_in + x.lo, s->h_in + x.lo, x.hi - x.lo, hipMemcpyHostToDevice, sin));
            in_bytes += (double)(x.hi - x.lo);
        }
        in_bytes += (double)(b - a) * sizeof(qpp_desc);
        // each phase's closing trace event is recorded before the event the
        // next stream waits on: the waits this function makes (ev_out[c],
        // s_out) then cover every event the trace readout reads
        if (tr) HIPCHK(hipEventRecord(s->tev[1][c], sin));
        HIPCHK(hipEventRecord(s->ev_in[c], sin));
        HIPCHK(hipStreamWaitEvent(s->stream, s->ev_in[c], 0));
        if (tr) HIPCHK(hipEventRecord(s->tev[2][c], s->stream));
        if (b > a) {
            rc = session_launch(enc, s, kt, m.dd + a, b - a, m.dr + a);
            if (rc != QPP_OK) break;
        }
        if (tr) HIPCHK(hipEventRecord(s->tev[3][c], s->stream));
        HIPCHK(hipEventRecord(s->ev_k[c], s->stream));
        HIPCHK(hipStreamWaitEvent(s->s_out, s->ev_k[c], 0));
        if (tr) HIPCHK(hipEventRecord(s->tev[4][c], s->s_out));
        out_bytes += (double)(olo[c + 1] - olo[c]) + (double)(b - a) * sizeof(qpp_result);
        {
            const size_t tl = olo[c + 1] > olo[c] ? olo[c + 1] - olo[c] : 0;
            const size_t rl = (size_t)(b - a) * sizeof(qpp_result);
            rc = qpp_internal_launch_xfer(s->hd_out + olo[c], s->d_out + olo[c], tl, (uint8_t *)(m.hrd + a),
                                          (const uint8_t *)(m.dr + a), rl, s->s_out);
            if (rc != QPP_OK) break;
        }
        HIPCHK(hipEventRecord(s->ev_out[c], s->s_out));
        if (tr) HIPCHK(hipEventRecord(s->tev[5][c], s->s_out));
        // hand back chunks whose D2H has already landed while later ones fly
        while (next_out < c) {
            if (hipEventQuery(s->ev_out[next_out]) != hipSuccess) {
                (void)hipGetLastError();  // hipErrorNotReady must not reach a later HIPCHK
                break;
            }
            hand_back(next_out++);
        }
    }
    if (rc != QPP_OK) return rc;
    const double t_sub = clk();
    for (int c = next_out; c < chunks; ++c) {
        HIPCHK(hipEventSynchronize(s->ev_out[c]));
        hand_back(c);
    }
    HIPCHK(hipStreamSynchronize(s->s_out));
    outg.wait();
    const double t_end = clk();
    if (tr) {
        qpp_trace &T = s->last;
        T = qpp_trace{};
        T.pipelined = 1;
        T.chunks = (uint32_t)chunks;
        T.total_ms = t_end - t_start;
        T.submit_ms = t_sub - t_start;
        T.copy_in_ms = t_copy_in;
        T.copy_out_ms = (double)outg.busy_ns.load() * 1e-6;
        T.wait_ms = t_end - t_sub;
        T.in_bytes = in_bytes;
        T.out_bytes = out_bytes;
        float ms = 0.f;
        for (int c = 0; c < chunks; ++c) {
            HIPCHK(hipEventElapsedTime(&ms, s->tev[0][c], s->tev[1][c]));
            T.h2d_ms += ms;
            HIPCHK(hipEventElapsedTime(&ms, s->tev[2][c], s->tev[3][c]));
            T.kernel_ms += ms;
            HIPCHK(hipEventElapsedTime(&ms, s->tev[4][c], s->tev[5][c]));
            T.d2h_ms += ms;
        }
        HIPCHK(hipEventElapsedTime(&ms, s->tev[0][0], s->tev[5][chunks - 1]));
        T.gpu_span_ms = ms;
    }
    return QPP_OK;
}

constexpr uint32_t kSmallPackets = 64;
constexpr size_t kSmallBytes = (size_t)256 << 10;
static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

static int session_run(bool enc, qpp_session *s, const qpp_keytab *kt, const qpp_desc *desc,
                       uint32_t n, const uint8_t *in, size_t in_len, uint8_t *out, size_t out_len, qpp_result *res)
{
    if (!s || !kt || (n && (!desc || !res))) return QPP_E_ARG;
    if (n == 0) return QPP_OK;
    size_t need = in_len > out_len ? in_len : out_len;
    int rc = session_reserve(s, need, n);
    if (rc != QPP_OK) return rc;
    // QPP_SESSION_SERIAL=1 (an A/B and test switch, read at every call): the serial path
    if (out_len >= 2 * kPipeChunkBytes && qpp_env_long("QPP_SESSION_SERIAL", 0) != 1)
        if (const int chunks = pipe_chunks(desc, n, out_len))
            return session_run_pipelined(enc, s, kt, desc, n, in, in_len, out, out_len, res, chunks);
    // Small batches (the per-call object API: one packet per call): one H2D
    // copy of [descriptors | input | zeroed output] and one D2H copy of
    // [output | results] through the session's input staging, instead of
    // four copies and a device memset.
    const size_t sd = al256((size_t)n * sizeof(qpp_desc)), si = al256(in_len), so = al256(out_len);
    const size_t small = sd + si + so + (size_t)n * sizeof(qpp_result);
    if (n <= kSmallPackets && small <= kSmallBytes && in != s->h_in && out != s->h_out) {
        rc = session_reserve(s, small > need ? small : need, n);
        if (rc != QPP_OK) return rc;
        uint8_t *h = s->h_in, *d = s->d_in;
        memcpy(h, desc, (size_t)n * sizeof(qpp_desc));
        reject_out_of_bounds(enc, (qpp_desc *)h, n, in_len, out_len);
        if (in_len) memcpy(h + sd, in, in_len);
        memset(h + sd + si, 0, out_len);  // bytes the kernel does not write come back as zeros
        if (n <= qpp_internal_lone_limit() && zero_copy_choice()) {
            // one wave per packet; the output and results are written by
            // the kernel straight into the pinned staging (PCIe writes post;
            // reads there would put a bus round trip on each of the kernel's
            // dependent loads).  Descriptors and input: copied by the kernel
            // itself in one round trip when the call fits one workgroup,
            // else by one copy
            uint8_t *dh = s->hd_in;
            LoneStage st{dh, d, 0u};
            if (n <= (uint32_t)(kLoneWG / 64) && sd + si <= kLoneStageMax && lone_stage_choice())
                st.bytes = (uint32_t)(sd + si);  // 256-byte multiples
            else
                HIPCHK(hipMemcpyAsync(d, h, sd + si, hipMemcpyHostToDevice, s->stream));
            rc = qpp_internal_launch_packets(enc, kt, (const qpp_desc *)d, n, d + sd, dh + sd + si,
                                             (qpp_result *)(dh + sd + si + so), s->stream, nullptr, &st);
            if (rc != QPP_OK) return rc;
        } else {
            HIPCHK(hipMemcpyAsync(d, h, sd + si + out_len, hipMemcpyHostToDevice, s->stream));
            rc = qpp_internal_launch_packets(enc, kt, (const qpp_desc *)d, n, d + sd, d + sd + si,
                                             (qpp_result *)(d + sd + si + so), s->stream);
            if (rc != QPP_OK) return rc;
            HIPCHK(hipMemcpyAsync(h + sd + si, d + sd + si, so + (size_t)n * sizeof(qpp_result),
                                  hipMemcpyDeviceToHost, s->stream));
        }
        HIPCHK(hipStreamSynchronize(s->stream));
        if (out_len) memcpy(out, h + sd + si, out_len);
        memcpy(res, h + sd + si + so, (size_t)n * sizeof(qpp_result));
        return QPP_OK;
    }
    const SessionMisc m = session_misc(s);
    memcpy(m.hd, desc, (size_t)n * sizeof(qpp_desc));
    reject_out_of_bounds(enc, m.hd, n, in_len, out_len);
    if (in_len && in != s->h_in) memcpy(s->h_in, in, in_len);  // staged by the caller already?
    HIPCHK(hipMemcpyAsync(m.dd, m.hd, (size_t)n * sizeof(qpp_desc), hipMemcpyHostToDevice, s->stream));
    if (in_len) HIPCHK(hipMemcpyAsync(s->d_in, s->h_in, in_len, hipMemcpyHostToDevice, s->stream));
    // bytes the kernel does not write (gaps, failed packets) come back as zeros
    if (out_len) HIPCHK(hipMemsetAsync(s->d_out, 0, out_len, s->stream));
    rc = session_launch(enc, s, kt, m.dd, n, m.dr);
    if (rc != QPP_OK) return rc;
    rc = qpp_internal_launch_xfer(s->hd_out, s->d_out, out_len, (uint8_t *)m.hrd, (const uint8_t *)m.dr,
                                  (size_t)n * sizeof(qpp_result), s->stream);
    if (rc != QPP_OK) return rc;
    HIPCHK(hipStreamSynchronize(s->stream));
    if (out_len && out != s->h_out) memcpy(out, s->h_out, out_len);
    memcpy(res, m.hr, (size_t)n * sizeof(qpp_result));
    return QPP_OK;
}

// qpp_session_protect / _unprotect.  On a failure, drain the session's
// streams before returning, so no copy into its staging is still in flight
// when the staging is reused or freed.
static int session_call(bool enc, qpp_session *s, const qpp_keytab *kt, const qpp_desc *desc, uint32_t n,
                        const uint8_t *in, size_t in_len, uint8_t *out, size_t out_len, qpp_result *res)
{
    const int rc = session_run(enc, s, kt, desc, n, in, in_len, out, out_len, res);
    if (rc != QPP_OK && s) {
        if (s->s_in) (void)hipStreamSynchronize(s->s_in);
        (void)hipStreamSynchronize(s->stream);
        if (s->s_out) (void)hipStreamSynchronize(s->s_out);
        (void)hipGetLastError();
    }
    return rc;
}

int qpp_session_protect(qpp_session *s, const qpp_keytab *kt, const qpp_desc *desc, uint32_t n,
                        const uint8_t *in, size_t in_len, uint8_t *out, size_t out_len, qpp_result *res)
{
    return session_call(true, s, kt, desc, n, in, in_len, out, out_len, res);
}

int qpp_session_unprotect(qpp_session *s, const qpp_keytab *kt, const qpp_desc *desc,
                          uint32_t n, const uint8_t *in, size_t in_len, uint8_t *out, size_t out_len, qpp_result *res)
{
    return session_call(false, s, kt, desc, n, in, in_len, out, out_len, res);
}

// The trace's timing events, all or none.
static int session_create_trace_events(qpp_session *s)
{
    bool ok = true;
    for (auto &row : s->tev)
        for (hipEvent_t &e : row) ok = ok && hipEventCreate(&e) == hipSuccess;
    if (ok) return QPP_OK;
    (void)hipGetLastError();
    for (auto &row : s->tev)
        for (hipEvent_t &e : row) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
    return QPP_E_HIP;
}

int qpp_session_trace(qpp_session *s, int enable, qpp_trace *last)
{
    if (!s) return QPP_E_ARG;
    if (last) *last = s->last;
    if (enable > 0 && !s->tev[0][0]) {
        const int rc = session_create_trace_events(s);
        if (rc != QPP_OK) return rc;
    }
    if (enable >= 0) s->trace = enable > 0;
    if (s->trace) s->last = qpp_trace{};  // a call that does not pipeline reports pipelined = 0
    return QPP_OK;
}

int qpp_session_stage(qpp_session *s, size_t bytes, uint32_t n, uint8_t **h_in, uint8_t **h_out)
{
    if (!s || !h_in || !h_out) return QPP_E_ARG;
    const int rc = session_reserve(s, bytes, n);
    if (rc != QPP_OK) return rc;
    *h_in = s->h_in;
    *h_out = s->h_out;
    return QPP_OK;
}

// The session's staging, sized as by qpp_session_stage, and `scratch` bytes of
// pinned and device scratch beside it (qpp_internal.h).
int qpp_internal_session_bufs(qpp_session *s, size_t bytes, uint32_t packets, size_t scratch, qpp_session_bufs *out)
{
    if (!s || !out) return QPP_E_ARG;
    const int rc = session_reserve(s, bytes, packets);
    if (rc != QPP_OK) return rc;
    if (scratch > s->scratch_bytes) {
        HIPCHK(hipStreamSynchronize(s->stream));
        if (s->h_scratch) (void)hipHostFree(s->h_scratch);
        if (s->d_scratch) (void)hipFree(s->d_scratch);
        s->h_scratch = s->d_scratch = NULL;
        s->scratch_bytes = 0;
        if (hipHostMalloc(&s->h_scratch, scratch, hipHostMallocDefault) != hipSuccess ||
            hipMalloc(&s->d_scratch, scratch) != hipSuccess) {
            (void)hipGetLastError();
            if (s->h_scratch) (void)hipHostFree(s->h_scratch);
            s->h_scratch = NULL;
            return QPP_E_NOMEM;
        }
        s->scratch_bytes = scratch;
    }
    *out = qpp_session_bufs{s->stream, s->h_in, s->h_out, s->d_in, s->d_out, s->h_scratch, s->d_scratch};
    return QPP_OK;
}

int qpp_session_hp_mask(qpp_session *s, const qpp_keytab *kt, const uint32_t *slots,
                        const uint8_t *samples, uint32_t n, uint8_t *masks)
{
    if (!s || !kt || (n && (!slots || !samples || !masks))) return QPP_E_ARG;
    if (n == 0) return QPP_OK;
    int rc = session_reserve(s, (size_t)n * 32, n);
    if (rc != QPP_OK) return rc;
    uint8_t *hs = s->h_in, *hm = s->h_out;
    uint32_t *hidx = (uint32_t *)s->h_misc;
    memcpy(hidx, slots, (size_t)n * 4);
    memcpy(hs, samples, (size_t)n * 16);
    if (n <= kSmallPackets && zero_copy_choice()) {
        rc = qpp_hp_mask(kt, (const uint32_t *)s->hd_misc, s->hd_in, n, s->hd_out, s->stream);
        if (rc != QPP_OK) return rc;
    } else {
        HIPCHK(hipMemcpyAsync(s->d_misc, hidx, (size_t)n * 4, hipMemcpyHostToDevice, s->stream));
        HIPCHK(hipMemcpyAsync(s->d_in, hs, (size_t)n * 16, hipMemcpyHostToDevice, s->stream));
        rc = qpp_hp_mask(kt, (const uint32_t *)s->d_misc, s->d_in, n, s->d_out, s->stream);
        if (rc != QPP_OK) return rc;
        HIPCHK(hipMemcpyAsync(hm, s->d_out, (size_t)n * 16, hipMemcpyDeviceToHost, s->stream));
    }
    HIPCHK(hipStreamSynchronize(s->stream));
    memcpy(masks, hm, (size_t)n * 16);
    return QPP_OK;
}

int qpp_session_set_keys(qpp_session *s, qpp_keytab *kt, const qpp_key_material *km, uint32_t n)
{
    if (!s) return QPP_E_ARG;
    return qpp_keytab_set(kt, km, n, s->stream);
}

// ------------------------------------------------------ several devices --
//
// One host batch over several GPUs of the node (packets
// are independent, so no collective): a session and a replica of the key
// table per device; the batch is cut into contiguous descriptor ranges, one
// per device (multi_split, qpp_batch.h), each range's input and output
// extents are staged and run by its own host thread on its own device, and
// every result lands at its packet's position in the caller's arrays.  Ranges
// whose output extents overlap (not the layout of a socket batch) run on the
// first device alone.  Output bytes outside every packet are zeros.

struct qpp_multi {
    int n;
    int device[kMultiMaxDevices];
    qpp_session *s[kMultiMaxDevices];
    qpp_keytab *kt[kMultiMaxDevices];
};

int qpp_multi_create(const int *devices, int n_devices, uint32_t key_capacity, qpp_multi **out)
{
    if (!out || !devices || n_devices < 1 || n_devices > kMultiMaxDevices) return QPP_E_ARG;
    *out = NULL;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) return QPP_E_NODEV;
    for (int k = 0; k < n_devices; ++k)
        if (devices[k] < 0 || devices[k] >= count) return QPP_E_ARG;
    qpp_multi *m = (qpp_multi *)calloc(1, sizeof(qpp_multi));
    if (!m) return QPP_E_NOMEM;
    int prev = 0;
    (void)hipGetDevice(&prev);
    int rc = QPP_OK;
    for (int k = 0; k < n_devices && rc == QPP_OK; ++k) {
        m->device[k] = devices[k];
        if (hipSetDevice(devices[k]) != hipSuccess) rc = QPP_E_HIP;
        if (rc == QPP_OK) rc = qpp_session_create(1 << 16, 64, &m->s[k]);
        if (rc == QPP_OK) rc = qpp_keytab_create(key_capacity, &m->kt[k]);
        m->n = k + 1;
    }
    (void)hipSetDevice(prev);
    if (rc != QPP_OK) {
        qpp_multi_destroy(m);
        return rc;
    }
    *out = m;
    return QPP_OK;
}

void qpp_multi_destroy(qpp_multi *m)
{
    if (!m) return;
    int prev = 0;
    (void)hipGetDevice(&prev);
    for (int k = 0; k < m->n; ++k) {
        (void)hipSetDevice(m->device[k]);
        qpp_session_destroy(m->s[k]);
        qpp_keytab_destroy(m->kt[k]);
    }
    (void)hipSetDevice(prev);
    free(m);
}

int qpp_multi_devices(const qpp_multi *m) { return m ? m->n : 0; }

int qpp_multi_set_keys(qpp_multi *m, const qpp_key_material *km, uint32_t n)
{
    if (!m) return QPP_E_ARG;
    int prev = 0, rc = QPP_OK;
    (void)hipGetDevice(&prev);
    for (int k = 0; k < m->n && rc == QPP_OK; ++k) {
        if (hipSetDevice(m->device[k]) != hipSuccess) rc = QPP_E_HIP;
        if (rc == QPP_OK) rc = qpp_session_set_keys(m->s[k], m->kt[k], km, n);
        if (rc == QPP_OK) rc = hipStreamSynchronize((hipStream_t)qpp_session_stream(m->s[k])) == hipSuccess
                                   ? QPP_OK : QPP_E_HIP;
    }
    (void)hipSetDevice(prev);
    return rc;
}

// The whole batch on the first device's session (its bounds checks and
// staging), without the range split's copy and passes over the descriptors.
static int multi_run_first(bool enc, qpp_multi *m, const qpp_desc *desc, uint32_t n, const uint8_t *in,
                           size_t in_len, uint8_t *out, size_t out_len, qpp_result *res)
{
    int prev = 0;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(m->device[0]);
    const int rc = session_call(enc, m->s[0], m->kt[0], desc, n, in, in_len, out, out_len, res);
    (void)hipSetDevice(prev);
    return rc;
}

static int multi_run(bool enc, qpp_multi *m, const qpp_desc *desc, uint32_t n, const uint8_t *in,
                     size_t in_len, uint8_t *out, size_t out_len, qpp_result *res)
{
    if (!m || (n && (!desc || !res))) return QPP_E_ARG;
    if (n == 0) {
        if (out_len) memset(out, 0, out_len);
        return QPP_OK;
    }
    if (m->n == 1) return multi_run_first(enc, m, desc, n, in, in_len, out, out_len, res);
    // bounds first (as a session does), so that extents use only packets
    // that fit; rejected ones stay rejected in their range and touch nothing
    std::vector<qpp_desc> d(desc, desc + n);
    reject_out_of_bounds(enc, d.data(), n, in_len, out_len);
    const std::vector<MultiRange> r = multi_split(enc, d.data(), n, m->n, in_len, out_len);
    const int parts = (int)r.size();
    if (parts == 1) return multi_run_first(enc, m, desc, n, in, in_len, out, out_len, res);
    multi_rebase(d.data(), r);
    for (const Extent &g : multi_gaps(r, out_len)) memset(out + g.lo, 0, g.hi - g.lo);
    std::vector<int> rcs(parts, QPP_OK);
    std::vector<std::thread> th;
    for (int k = 0; k < parts; ++k)
        th.emplace_back([&, k] {
            const MultiRange &x = r[k];
            if (hipSetDevice(m->device[k]) != hipSuccess) {
                rcs[k] = QPP_E_HIP;
                return;
            }
            rcs[k] = session_call(enc, m->s[k], m->kt[k], d.data() + x.b, x.e - x.b, in + x.ilo, x.ihi - x.ilo,
                                  out + x.olo, x.ohi - x.olo, res + x.b);
        });
    for (auto &t : th) t.join();
    for (int k = 0; k < parts; ++k)
        if (rcs[k] != QPP_OK) return rcs[k];
    return QPP_OK;
}

int qpp_multi_protect(qpp_multi *m, const qpp_desc *desc, uint32_t n, const uint8_t *in, size_t in_len,
                      uint8_t *out, size_t out_len, qpp_result *res)
{
    return multi_run(true, m, desc, n, in, in_len, out, out_len, res);
}

int qpp_multi_unprotect(qpp_multi *m, const qpp_desc *desc, uint32_t n, const uint8_t *in, size_t in_len,
                        uint8_t *out, size_t out_len, qpp_result *res)
{
    return multi_run(false, m, desc, n, in, in_len, out, out_len, res);
}

int qpp_multi_trace(qpp_multi *m, int enable, qpp_trace *last, int max)
{
    if (!m || max < 0 || (max > 0 && !last)) return QPP_E_ARG;
    int prev = 0, rc = QPP_OK, k = 0;
    (void)hipGetDevice(&prev);
    for (; k < m->n && rc == QPP_OK; ++k) {
        if (hipSetDevice(m->device[k]) != hipSuccess) rc = QPP_E_HIP;
        if (rc == QPP_OK) rc = qpp_session_trace(m->s[k], enable, k < max ? last + k : nullptr);
    }
    (void)hipSetDevice(prev);
    return rc == QPP_OK ? (m->n < max ? m->n : max) : rc;
}
