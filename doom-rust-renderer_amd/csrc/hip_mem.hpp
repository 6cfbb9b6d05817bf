// hip_mem.hpp — owners of device and pinned host memory, of streams and events, one timed interval on a stream, and host tables
// packed into one device allocation.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <type_traits>
#include <vector>

#include "slab_layout.h"

namespace dg {

// Move-only owners of device memory (hipMalloc) and pinned host memory (hipHostMalloc), and below of streams and events.  Whoever
// destroys one has made the owning ctx's device current and synchronised the streams that may still use the memory, and the stream
// itself or the one the event was recorded on (~dg_ctx, dg_upload_scene).  Destroying an empty owner does nothing.
struct DevMem {
    static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    void operator()(void *p) const { (void)hipFree(p); }
};
struct PinnedMem {
    static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    void operator()(void *p) const { (void)hipHostFree(p); }
};
template <class T> using DevPtr = std::unique_ptr<T, DevMem>;
template <class T> using PinnedPtr = std::unique_ptr<T, PinnedMem>;
// (Re)allocate: what p held is freed first, and p stays empty when the allocation fails.
template <class T, class Mem> hipError_t hip_alloc(std::unique_ptr<T, Mem> &p, size_t bytes) {
    p.reset();
    void *q = nullptr;
    const hipError_t e = Mem::alloc(&q, bytes);
    if (e == hipSuccess) p.reset(static_cast<T *>(q));
    return e;
}

// Streams and events: both handles are plain pointers.  The launch functions take the raw handle (get()).
struct StreamEnd { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };
struct EventEnd { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
using Stream = std::unique_ptr<std::remove_pointer_t<hipStream_t>, StreamEnd>;
using Event = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, EventEnd>;
// (std::vector<Slot> relies on both: a slot is moved, never copied, and moving one cannot fail half way)
static_assert(!std::is_copy_constructible_v<Stream> && !std::is_copy_constructible_v<Event>, "stream and event owners are not copyable");
static_assert(std::is_nothrow_move_constructible_v<Stream> && std::is_nothrow_move_constructible_v<Event>, "stream and event owners move without throwing");
// A non-blocking stream, with `priority` when one is given; an event, without timing when it only orders streams.  As hip_alloc:
// what the owner held is destroyed first, and it stays empty when the creation fails.
inline hipError_t stream_create(Stream &s, const int *priority = nullptr) {
    s.reset();
    hipStream_t q = nullptr;
    const hipError_t e = priority ? hipStreamCreateWithPriority(&q, hipStreamNonBlocking, *priority) : hipStreamCreateWithFlags(&q, hipStreamNonBlocking);
    if (e == hipSuccess) s.reset(q);
    return e;
}
inline hipError_t event_create(Event &ev, bool timing = true) {
    ev.reset();
    hipEvent_t q = nullptr;
    const hipError_t e = timing ? hipEventCreate(&q) : hipEventCreateWithFlags(&q, hipEventDisableTiming);
    if (e == hipSuccess) ev.reset(q);
    return e;
}
// Everything queued on the stream has run (an empty owner has nothing queued): what a destructor calls before its members go.
inline void drain(const Stream &s) { if (s) (void)hipStreamSynchronize(s.get()); }

// One timed interval on a stream of the ctx's own: the events around the kernel of the last call that used it, and whether that
// call completed.  begin() before the work is queued (the events are created by the first), end() once it has run; elapsed() reads
// the time of an interval that is `measured`.
struct TimedInterval {
    Event t0, t1;
    bool measured = false;
    hipError_t begin() {
        measured = false;
        hipError_t e = t0 ? hipSuccess : event_create(t0);
        if (e == hipSuccess && !t1) e = event_create(t1);
        return e;
    }
    void end() { measured = true; }
    hipError_t elapsed(float *ms) const { return hipEventElapsedTime(ms, t0.get(), t1.get()); }
};

// Host tables packed into one device allocation: each starts on a 256-byte boundary and takes at least 16 bytes (an empty table
// still has an address of its own).  add() the tables, upload() them (one hipMalloc, one copy), then at<T>() what add() returned.
struct TablePack {
    std::vector<uint8_t> staged;
    SlabCursor cur;
    const uint8_t *base = nullptr;
    template <class T> size_t add(const std::vector<T> &v) {
        const size_t at = cur.take(std::max<size_t>(v.size() * sizeof(T), 16));
        staged.resize(cur.next);
        if (!v.empty()) std::memcpy(staged.data() + at, v.data(), v.size() * sizeof(T));
        return at;
    }
    hipError_t upload(DevPtr<uint8_t> &mem) {
        const hipError_t e = hip_alloc(mem, staged.size());
        base = mem.get();
        return e != hipSuccess ? e : hipMemcpy(mem.get(), staged.data(), staged.size(), hipMemcpyHostToDevice);
    }
    template <class T> const T *at(size_t off) const { return reinterpret_cast<const T *>(base + off); }
};

}  // namespace dg
