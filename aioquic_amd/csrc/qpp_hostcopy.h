// qpp_hostcopy.h -- host copies between caller memory and pinned staging
// (qpp_session.hip).  Plain C++17, nothing of HIP: tests/session_host.cc runs
// it under the host sanitizers.  One thread streams ~10 GB/s, well under the
// PCIe rate, so large copies are split over a process-wide pool of copy
// threads (started on first use, never torn down: its threads sleep on a
// condition variable between copies; round 5: instead of a std::thread per
// part and copy), and a chunk's copy-out runs on it while the calling thread
// stages the next chunks.
#pragma once

#include <immintrin.h>
#include <pthread.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>

namespace qpp {

// Non-temporal stores: a plain memcpy below glibc's non-temporal threshold
// reads each destination line before writing it (write-allocate), so a copy
// moves three times its size through host memory instead of two.  (memcpy
// without AVX2.)
inline bool copy_nt_choice()
{
    static const bool b = __builtin_cpu_supports("avx2");
    return b;
}

__attribute__((target("avx2"))) inline void copy_nt_avx2(uint8_t *dst, const uint8_t *src, size_t n)
{
    size_t head = (size_t)((32u - ((uintptr_t)dst & 31u)) & 31u);
    if (head > n) head = n;
    memcpy(dst, src, head);
    dst += head;
    src += head;
    n -= head;
    size_t i = 0;
    for (; i + 128 <= n; i += 128) {
        const __m256i a = _mm256_loadu_si256((const __m256i *)(src + i));
        const __m256i b = _mm256_loadu_si256((const __m256i *)(src + i + 32));
        const __m256i c = _mm256_loadu_si256((const __m256i *)(src + i + 64));
        const __m256i d = _mm256_loadu_si256((const __m256i *)(src + i + 96));
        _mm256_stream_si256((__m256i *)(dst + i), a);
        _mm256_stream_si256((__m256i *)(dst + i + 32), b);
        _mm256_stream_si256((__m256i *)(dst + i + 64), c);
        _mm256_stream_si256((__m256i *)(dst + i + 96), d);
    }
    memcpy(dst + i, src + i, n - i);
    _mm_sfence();  // the streamed lines are visible before the copy is reported done
}

inline void copy_bytes(uint8_t *dst, const uint8_t *src, size_t n)
{
    if (n >= ((size_t)1 << 16) && copy_nt_choice()) copy_nt_avx2(dst, src, n);
    else memcpy(dst, src, n);
}

inline uint64_t ns_since(std::chrono::steady_clock::time_point t0)
{
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0)
        .count();
}

struct CopyGroup {
    std::mutex mu;
    std::condition_variable cv;
    int pending = 0;
    std::atomic<uint64_t> busy_ns{0};  // summed duration of the pool's tasks (qpp_trace)
    void wait()
    {
        std::unique_lock<std::mutex> l(mu);
        cv.wait(l, [&] { return pending == 0; });
    }
};

constexpr int kCopyThreads = 6;  // 2, 3, 4, 8 and 12 measured within the spread of 6
class CopyPool {
  public:
    static CopyPool &get()
    {
        // never destroyed (no join at exit); a forked child, which inherits
        // the pointer but not the threads, starts a pool of its own
        static std::once_flag once;
        std::call_once(once, [] { pthread_atfork(nullptr, nullptr, [] { g_pool.store(nullptr); }); });
        CopyPool *p = g_pool.load();
        if (!p) {
            std::lock_guard<std::mutex> l(g_pool_mu);
            p = g_pool.load();
            if (!p) {
                p = new CopyPool();
                g_pool.store(p);
            }
        }
        return *p;
    }
    int threads() const { return n_; }
    void submit(uint8_t *dst, const uint8_t *src, size_t len, CopyGroup *g)
    {
        {
            std::lock_guard<std::mutex> l(g->mu);
            ++g->pending;
        }
        {
            std::lock_guard<std::mutex> l(mu_);
            q_.push_back(Task{dst, src, len, g});
        }
        cv_.notify_one();
    }

  private:
    struct Task {
        uint8_t *dst;
        const uint8_t *src;
        size_t len;
        CopyGroup *g;
    };
    CopyPool()
    {
        // (round 5 also pinned the threads to the CPUs of the device's NUMA
        // node: 13.0-16.6 against 11.5-17.7 GiB/s unpinned on one two-socket
        // box, interleaved -- no difference through the run-to-run spread,
        // profiles/r5e_host_path/host_path_studies.txt; removed)
        for (int i = 0; i < n_; ++i) std::thread([this] { run(); }).detach();
    }
    void run()
    {
        for (;;) {
            Task t;
            {
                std::unique_lock<std::mutex> l(mu_);
                cv_.wait(l, [&] { return !q_.empty(); });
                t = q_.front();
                q_.pop_front();
            }
            const auto t0 = std::chrono::steady_clock::now();
            copy_bytes(t.dst, t.src, t.len);
            t.g->busy_ns.fetch_add(ns_since(t0), std::memory_order_relaxed);
            {
                // notify while holding the group's lock: the waiter cannot see
                // pending == 0 (and destroy the group, which lives on its
                // stack) until this worker has released the lock, after which
                // it never touches the group again
                std::lock_guard<std::mutex> l(t.g->mu);
                if (--t.g->pending == 0) t.g->cv.notify_all();
            }
        }
    }
    const int n_ = kCopyThreads;
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<Task> q_;
    inline static std::atomic<CopyPool *> g_pool{nullptr};
    inline static std::mutex g_pool_mu;
};

// dst <- src over the pool's threads in parts of >= 4 MiB; with g, return at
// once (g->wait() before the bytes are used), else when the copy is done.
inline void par_memcpy(uint8_t *dst, const uint8_t *src, size_t bytes, CopyGroup *g = nullptr)
{
    constexpr size_t kPart = (size_t)4 << 20;
    if (bytes < 2 * kPart) {
        const auto t0 = std::chrono::steady_clock::now();
        copy_bytes(dst, src, bytes);
        if (g) g->busy_ns.fetch_add(ns_since(t0), std::memory_order_relaxed);
        return;
    }
    CopyPool &pool = CopyPool::get();
    size_t parts = bytes / kPart;
    if (parts > (size_t)pool.threads()) parts = (size_t)pool.threads();
    const size_t step = (bytes / parts + 63) & ~(size_t)63;
    CopyGroup local;
    CopyGroup *grp = g ? g : &local;
    for (size_t lo = g ? 0 : step; lo < bytes; lo += step)
        pool.submit(dst + lo, src + lo, lo + step < bytes ? step : bytes - lo, grp);
    if (!g) {
        copy_bytes(dst, src, step < bytes ? step : bytes);  // the caller's own part
        local.wait();
    }
}

}  // namespace qpp
