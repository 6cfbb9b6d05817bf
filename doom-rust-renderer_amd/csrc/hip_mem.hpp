// hip_mem.hpp — owners of device and pinned host memory, and host tables packed into one device allocation.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "slab_layout.h"

namespace dg {

// Move-only owners of device memory (hipMalloc) and pinned host memory (hipHostMalloc).  Whoever destroys one has made the owning
// ctx's device current and synchronised the streams that may still use the memory (free_ctx, dg_upload_scene).
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
