// upload.h -- host symbols on their way to the device: the handle's ring of pinned memory and the narrowed upload.
#pragma once
#include "alphabet.h"
#include "handle.h"
#include <atomic>
#include <thread>

// ---- host symbols go up as 16-bit words ------------------------------------------------------------------------------
// east_hip_build hands over 4 bytes per symbol, and the link moves 56 GB/s: 245 MB for the 64 MiB bench document are 4.4 ms
// before the 1.7 ms build can start (tools/pcie_probe.py: pageable and pinned memory alike).  In the reference's encoding
// a text symbol is below U+0A00 and everything else a terminator whose number the build never reads, so half the bytes
// say it all: host threads narrow the symbols into the slots of the pinned ring (0xFFFF = "a terminator"), the slots go
// up one DMA each, and a kernel behind every DMA widens them again into the staging area the build reads -- the link
// carries 2 bytes per symbol, narrowing and widening hide under it.  (Tagged streams -- text above U+0A00 -- and small
// inputs take the plain copy; a handle's first call too, while the ring is pinned in the background.)
#define TP_RING_SLOTS 3                     // slots of TP_RING_SLOT bytes in a handle's pinned ring (common.h; textfront.h: tp_fill_stream)
#define SYM_NARROW_MIN ((u32)4 << 20)
#define SYM_TERMINATOR16 0xFFFFu
// The ring a background thread pinned becomes the handle's (or is given back when the handle pinned one itself in the
// meantime); wait: join the thread even if it is still at work (before an inline allocation, at destruction).
static void ring_adopt(east_hip_index *h, bool wait)
{
    if (h->ring_alloc.joinable() && (wait || h->ring_done.load())) h->ring_alloc.join();
    if (h->ring_alloc.joinable()) return;
    char *pending = h->ring_pending.exchange(nullptr);
    if (!pending) return;
    if (!h->ring) h->ring = pending;
    else if (pending != h->ring) (void)hipHostFree(pending);
}

// TP_RING_SLOTS slots of pinned memory; nullptr if they cannot be had.  (No handle: the background thread's allocation too.)
static char *ring_alloc_pinned()
{
    void *p = nullptr;
    if (hipHostMalloc(&p, TP_RING_SLOT * TP_RING_SLOTS, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return (char *)p;
}

// The handle's ring, pinned here and now if it has none (3-5 ms, once per handle), and the events of its slots (a ring
// that was pinned in the background comes without).  false: no pinned memory -- what then is the caller's business.
static bool ring_pin_now(east_hip_index *h)
{
    if (!h->ring) h->ring = ring_alloc_pinned();
    if (!h->ring) return false;
    while (h->ring_events.size() < TP_RING_SLOTS) {
        hipEvent_t e;
        HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        h->ring_events.push_back(e);
    }
    return true;
}

// a first call went without the ring (see prepare_texts_streamed): pin it now that the call is over, in the background
static void ring_pin_later(east_hip_index *h)
{
    ring_adopt(h, false);                  // (a thread that failed to pin is joined here, and the next call may try again)
    if (!h->ring_wanted || h->ring || h->ring_alloc.joinable() || h->ring_pending.load()) return;
    h->ring_wanted = false;
    h->ring_done.store(false);
    const int dev = h->device;
    std::atomic<char *> *slot = &h->ring_pending;
    std::atomic<bool> *done = &h->ring_done;
    h->ring_alloc = std::thread([dev, slot, done]() {
        if (hipSetDevice(dev) != hipSuccess) (void)hipGetLastError();
        else if (char *p = ring_alloc_pinned()) slot->store(p);
        done->store(true);
    });
}

__global__ __launch_bounds__(BLOCK) void widen_symbols_kernel(const uint16_t *__restrict__ in, u32 n, u32 *__restrict__ out)
{
    const u32 i = (blockIdx.x * BLOCK + threadIdx.x) * 8u;
    if (i + 8u <= n && ((uintptr_t)(in + i) & 15u) == 0 && ((uintptr_t)(out + i) & 15u) == 0) {
        const uint4 v = *reinterpret_cast<const uint4 *>(in + i);
        const u32 w[4] = {v.x, v.y, v.z, v.w};
        u32 o[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const u32 x = (w[k >> 1] >> ((k & 1) * 16)) & 0xFFFFu;
            o[k] = x == SYM_TERMINATOR16 ? TEXT_SYMBOLS : x;
        }
        reinterpret_cast<uint4 *>(out + i)[0] = uint4{o[0], o[1], o[2], o[3]};
        reinterpret_cast<uint4 *>(out + i)[1] = uint4{o[4], o[5], o[6], o[7]};
    } else {
        for (u32 j = i; j < i + 8u && j < n; j++) { const u32 x = in[j]; out[j] = x == SYM_TERMINATOR16 ? TEXT_SYMBOLS : x; }
    }
}

// (bytes: text code points below 0xFF as they are, 0xFF = a terminator)
__global__ __launch_bounds__(BLOCK) void widen_symbols8_kernel(const uint8_t *__restrict__ in, u32 n, u32 *__restrict__ out)
{
    const u32 i = (blockIdx.x * BLOCK + threadIdx.x) * 16u;
    if (i + 16u <= n && ((uintptr_t)(in + i) & 15u) == 0 && ((uintptr_t)(out + i) & 15u) == 0) {
        const uint4 v = *reinterpret_cast<const uint4 *>(in + i);
        const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int g = 0; g < 4; g++) {
            u32 o[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const u32 x = (w[g] >> (k * 8)) & 0xFFu;
                o[k] = x == 0xFFu ? TEXT_SYMBOLS : x;
            }
            reinterpret_cast<uint4 *>(out + i)[g] = uint4{o[0], o[1], o[2], o[3]};
        }
    } else {
        for (u32 j = i; j < i + 16u && j < n; j++) { const u32 x = in[j]; out[j] = x == 0xFFu ? TEXT_SYMBOLS : x; }
    }
}

// symbols [0, n) from the host into `staging` (device, n words) through the pinned ring; d_narrow: n + 8 halfwords of device scratch
// The narrowing of a stretch of host symbols into the pinned ring.  With AVX2 (looked for at run time): sixteen symbols a
// step -- unsigned compare by max, saturating pack, the lanes put back in order -- and STREAMING stores: the ring is
// written once and read by the copy engine, a store that first fetches the line it overwrites moves a third more bytes
// through the host's memory than the narrowing needs (4 B read + 2 B written per symbol).
#if !defined(__HIP_DEVICE_COMPILE__) && (defined(__x86_64__) || defined(__i386__))
#include <immintrin.h>
__attribute__((target("avx2"))) static void narrow_symbols_avx2(const u32 *src, uint16_t *dst, size_t n)
{
    size_t i = 0;
    for (; i < n && ((uintptr_t)(dst + i) & 31u); i++) dst[i] = src[i] < TEXT_SYMBOLS ? (uint16_t)src[i] : (uint16_t)SYM_TERMINATOR16;
    const __m256i first_term = _mm256_set1_epi32((int)TEXT_SYMBOLS), term = _mm256_set1_epi32((int)SYM_TERMINATOR16);
    for (; i + 16 <= n; i += 16) {
        __m256i a = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(src + i));
        __m256i b = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(src + i + 8));
        const __m256i ta = _mm256_cmpeq_epi32(_mm256_max_epu32(a, first_term), a);      // a >= TEXT_SYMBOLS (unsigned)
        const __m256i tb = _mm256_cmpeq_epi32(_mm256_max_epu32(b, first_term), b);
        a = _mm256_blendv_epi8(a, term, ta);
        b = _mm256_blendv_epi8(b, term, tb);
        const __m256i p = _mm256_permute4x64_epi64(_mm256_packus_epi32(a, b), 0xD8);    // (the pack works per 128-bit lane)
        _mm256_stream_si256(reinterpret_cast<__m256i *>(dst + i), p);
    }
    for (; i < n; i++) dst[i] = src[i] < TEXT_SYMBOLS ? (uint16_t)src[i] : (uint16_t)SYM_TERMINATOR16;
    _mm_sfence();
}
static const bool g_have_avx2 = __builtin_cpu_supports("avx2") && getenv("EAST_HIP_NO_AVX2") == nullptr;
#else
static void narrow_symbols_avx2(const u32 *, uint16_t *, size_t) {}
static const bool g_have_avx2 = false;
#endif
// ... and to BYTES, for text whose code points all lie below 0xFF (every BASELINE input: A-Z): half the bytes over the link
// again.  A text symbol the byte cannot hold (0xFF .. 0x9FF) is reported and the upload starts over with 16-bit words.
#if !defined(__HIP_DEVICE_COMPILE__) && (defined(__x86_64__) || defined(__i386__))
__attribute__((target("avx2"))) static bool narrow_symbols8_avx2(const u32 *src, uint8_t *dst, size_t n)
{
    size_t i = 0;
    bool bad = false;
    auto one = [&](size_t k) { const u32 c = src[k]; bad |= c >= 0xFFu && c < TEXT_SYMBOLS; dst[k] = c < 0xFFu ? (uint8_t)c : (uint8_t)0xFFu; };
    for (; i < n && ((uintptr_t)(dst + i) & 31u); i++) one(i);
    const __m256i first_term = _mm256_set1_epi32((int)TEXT_SYMBOLS), byte_max = _mm256_set1_epi32(0xFF);
    __m256i wrong = _mm256_setzero_si256();
    for (; i + 32 <= n; i += 32) {
        __m256i v[4];
#pragma GCC unroll 4
        for (int k = 0; k < 4; k++) {
            const __m256i a = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(src + i + 8 * k));
            const __m256i is_term = _mm256_cmpeq_epi32(_mm256_max_epu32(a, first_term), a);           // a >= TEXT_SYMBOLS (unsigned)
            const __m256i fits = _mm256_cmpeq_epi32(_mm256_min_epu32(a, byte_max), a);                  // a <= 0xFF
            // (0xFF itself does not fit either: it is the terminator's byte)
            wrong = _mm256_or_si256(wrong, _mm256_andnot_si256(is_term, _mm256_or_si256(_mm256_cmpeq_epi32(a, byte_max),
                                                                                         _mm256_xor_si256(fits, _mm256_set1_epi32(-1)))));
            v[k] = _mm256_blendv_epi8(a, byte_max, is_term);
        }
        // 32-bit -> 16-bit -> 8-bit, the 128-bit lanes put back in order at the end
        const __m256i p01 = _mm256_packus_epi32(v[0], v[1]), p23 = _mm256_packus_epi32(v[2], v[3]);
        const __m256i b = _mm256_packus_epi16(p01, p23);
        const __m256i r = _mm256_permutevar8x32_epi32(b, _mm256_setr_epi32(0, 4, 1, 5, 2, 6, 3, 7));
        _mm256_stream_si256(reinterpret_cast<__m256i *>(dst + i), r);
    }
    bad |= !_mm256_testz_si256(wrong, wrong);
    for (; i < n; i++) one(i);
    _mm_sfence();
    return !bad;
}
#else
static bool narrow_symbols8_avx2(const u32 *, uint8_t *, size_t) { return false; }
#endif
static bool narrow_symbols8(const u32 *src, uint8_t *dst, size_t n)
{
    if (g_have_avx2) return narrow_symbols8_avx2(src, dst, n);
    bool bad = false;
    for (size_t i = 0; i < n; i++) { const u32 c = src[i]; bad |= c >= 0xFFu && c < TEXT_SYMBOLS; dst[i] = c < 0xFFu ? (uint8_t)c : (uint8_t)0xFFu; }
    return !bad;
}
static void narrow_symbols(const u32 *src, uint16_t *dst, size_t n)
{
    if (g_have_avx2) { narrow_symbols_avx2(src, dst, n); return; }
    for (size_t i = 0; i < n; i++) dst[i] = src[i] < TEXT_SYMBOLS ? (uint16_t)src[i] : (uint16_t)SYM_TERMINATOR16;
}

// T = uint16_t: every symbol of the reference encoding fits (a terminator = 0xFFFF on the wire); T = uint8_t: text below
// 0xFF only -- returns false, with nothing left in flight, when a symbol did not fit (the caller starts over with 16 bits).
template <class T>
static bool upload_symbols_narrow(east_hip_index *h, const u32 *sym, u32 n, u32 *staging, T *d_narrow)
{
    constexpr bool BYTES = sizeof(T) == 1;
    static const size_t slot_env = getenv("EAST_HIP_SYMBOL_SLOT") ? (size_t)atoll(getenv("EAST_HIP_SYMBOL_SLOT")) : 0;     // (experiments)
    const size_t slot_bytes = slot_env >= 65536 && slot_env <= TP_RING_SLOT ? slot_env & ~(size_t)255 : TP_RING_SLOT;
    const size_t slot_syms = slot_bytes / sizeof(T);
    const u32 n_slots = ceil_div_u32(n, slot_syms);
    static const int threads_env = getenv("EAST_HIP_SYMBOL_THREADS") ? atoi(getenv("EAST_HIP_SYMBOL_THREADS")) : 0;     // (experiments)
    // (bytes: the link carries a quarter of the symbols' bytes, the narrowing threads read all of them -- eight, measured below)
    const int n_fill = threads_env > 0 ? std::min(threads_env, 64)
                                       : (int)std::min<u32>(BYTES ? 8u : 6u, std::max<u32>(2u, std::thread::hardware_concurrency() / 2u));
    // (measured on the 256-thread host of the MI355X box, 61 M symbols: 3 threads 5.8-6.4 ms per call, 4: 5.2-5.5, 6: 4.7-5.6,
    // 8-24: 4.9-5.9 -- against 6.1 ms with the plain 4-byte copy; the narrowing threads, not the link, set the pace)
    (void)ring_pin_now(h);                                   // (the caller has made sure of the ring: its events)
    // (the copy stream must not start before what is still queued on the handle's stream has left the arena alone)
    HIP_CHECK(hipEventRecord(h->ev0, h->stream));
    HIP_CHECK(hipStreamWaitEvent(h->copy_stream, h->ev0, 0));
    std::vector<std::atomic<int>> slot_parts(n_slots);
    for (auto &a : slot_parts) a.store(0, std::memory_order_relaxed);
    std::atomic<u32> slots_free{TP_RING_SLOTS};
    std::atomic<int> abort{0}, misfit{0};
    T *ring = (T *)h->ring;                                  // (slot k of the ring starts at k * TP_RING_SLOT whatever part of it is used)
    std::vector<std::thread> fillers;
    for (int j = 0; j < n_fill; j++)
        fillers.emplace_back([&, j]() {
            for (u32 sl = 0; sl < n_slots; sl++) {
                while (slots_free.load(std::memory_order_acquire) <= sl) {
                    if (abort.load(std::memory_order_acquire)) return;
                    std::this_thread::yield();
                }
                const size_t a = (size_t)sl * slot_syms, len = std::min<size_t>(slot_syms, (size_t)n - a);
                const size_t lo = len * (size_t)j / (size_t)n_fill, hi = len * (size_t)(j + 1) / (size_t)n_fill;
                const u32 *src = sym + a;
                T *dst = ring + (size_t)(sl % TP_RING_SLOTS) * (TP_RING_SLOT / sizeof(T));
                if constexpr (BYTES) { if (!narrow_symbols8(src + lo, (uint8_t *)dst + lo, hi - lo)) misfit.store(1, std::memory_order_release); }
                else narrow_symbols(src + lo, (uint16_t *)dst + lo, hi - lo);
                slot_parts[sl].fetch_add(1, std::memory_order_release);
            }
        });
    struct Joiner {
        std::vector<std::thread> &fill;
        std::atomic<int> &abort;
        hipStream_t copy;
        bool ok = false;
        ~Joiner()
        {
            if (!ok) abort.store(1, std::memory_order_release);
            for (auto &f : fill)
                if (f.joinable()) f.join();
            if (!ok) (void)hipStreamSynchronize(copy);
        }
    } joiner{fillers, abort, h->copy_stream};
    for (u32 sl = 0; sl < n_slots; sl++) {
        while (slot_parts[sl].load(std::memory_order_acquire) < n_fill) std::this_thread::yield();
        if (misfit.load(std::memory_order_acquire)) return false;      // (the joiner stops the fill threads and drains the copy stream)
        const size_t a = (size_t)sl * slot_syms, len = std::min<size_t>(slot_syms, (size_t)n - a);
        HIP_CHECK(hipMemcpyAsync(d_narrow + a, ring + (size_t)(sl % TP_RING_SLOTS) * (TP_RING_SLOT / sizeof(T)), len * sizeof(T), hipMemcpyHostToDevice, h->copy_stream));
        HIP_CHECK(hipEventRecord(h->ring_events[sl % TP_RING_SLOTS], h->copy_stream));
        if constexpr (BYTES)
            hipLaunchKernelGGL(widen_symbols8_kernel, dim3(ceil_div_u32(len, BLOCK * 16)), dim3(BLOCK), 0, h->copy_stream, (const uint8_t *)(d_narrow + a),
                               (u32)len, staging + a);
        else
            hipLaunchKernelGGL(widen_symbols_kernel, dim3(ceil_div_u32(len, BLOCK * 8)), dim3(BLOCK), 0, h->copy_stream, (const uint16_t *)(d_narrow + a),
                               (u32)len, staging + a);
        HIP_CHECK(hipGetLastError());
        if (sl >= 1) {                                   // the slot before is on the device: back to the fill threads
            HIP_CHECK(hipEventSynchronize(h->ring_events[(sl - 1) % TP_RING_SLOTS]));
            slots_free.store(sl + TP_RING_SLOTS, std::memory_order_release);
        }
    }
    joiner.ok = true;
    HIP_CHECK(hipEventRecord(h->ev1, h->copy_stream));   // (ev0 / ev1 are recorded anew by the build behind this)
    HIP_CHECK(hipStreamWaitEvent(h->stream, h->ev1, 0));
    return true;
}
