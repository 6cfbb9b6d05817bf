// stream_read.hip — the rate of a plain streaming read of one buffer on one GPU: the yardstick of kernels that read much and write almost
// nothing (tools/explored_bench.py holds dg_seen_lines against it).
//     hipcc --offload-arch=gfx950 -O3 -o tools/microbench/stream_read tools/microbench/stream_read.hip
//     tools/microbench/stream_read [BYTES = 3072000000] [REPS = 10]
// 256 lanes per workgroup, four independent 16-byte loads per lane and step (the piece dg_seen_lines holds in flight), one workgroup per
// 16 KB x 4 steps; the loaded words are XORed and stored only if they hit a value the buffer cannot give, so nothing is written.
// Prints one JSON line with the median, minimum and maximum time of REPS launches (events on the dispatch) after two warm-up launches.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define HIP_OK(expr)                                                                                         \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess) { std::printf("{\"error\": \"%s: %s\"}\n", #expr, hipGetErrorString(e_)); return 1; } \
    } while (0)

constexpr int kThreads = 256, kLoads = 4, kSteps = 4;

__global__ void __launch_bounds__(kThreads) stream_read(const uint4 *__restrict__ src, size_t n16, unsigned *__restrict__ sink) {
    const size_t base = (size_t)blockIdx.x * kThreads * kLoads * kSteps;
    unsigned acc = 0u;
    for (int s = 0; s < kSteps; s++) {
        uint4 v[kLoads];
#pragma unroll
        for (int i = 0; i < kLoads; i++) {
            const size_t j = base + ((size_t)s * kLoads + i) * kThreads + threadIdx.x;
            v[i] = j < n16 ? src[j] : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int i = 0; i < kLoads; i++) acc ^= v[i].x ^ v[i].y ^ v[i].z ^ v[i].w;
    }
    if (acc == 0x12345678u) sink[0] = acc;                 // (the buffer holds one byte value everywhere: never)
}

int main(int argc, char **argv) {
    const size_t bytes = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 3072000000ull;
    const int reps = argc > 2 ? std::atoi(argv[2]) : 10;
    const size_t n16 = bytes / 16;
    if (n16 == 0 || reps < 1) { std::printf("{\"error\": \"bad arguments\"}\n"); return 2; }
    uint4 *src = nullptr;
    unsigned *sink = nullptr;
    HIP_OK(hipMalloc(&src, n16 * 16));
    HIP_OK(hipMalloc(&sink, 256));
    HIP_OK(hipMemset(src, 0x5a, n16 * 16));
    HIP_OK(hipMemset(sink, 0, 256));
    hipEvent_t e0, e1;
    HIP_OK(hipEventCreate(&e0));
    HIP_OK(hipEventCreate(&e1));
    const size_t per_block = (size_t)kThreads * kLoads * kSteps;
    const unsigned blocks = (unsigned)((n16 + per_block - 1) / per_block);
    std::vector<float> ms;
    for (int r = 0; r < reps + 2; r++) {
        hipExtLaunchKernelGGL(stream_read, dim3(blocks), dim3(kThreads), 0, nullptr, e0, e1, 0, (const uint4 *)src, n16, sink);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        float t = 0.0f;
        HIP_OK(hipEventElapsedTime(&t, e0, e1));
        if (r >= 2) ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    const double med = ms[ms.size() / 2];
    std::printf("{\"bytes\": %zu, \"reps\": %d, \"ms_median\": %.4f, \"ms_min\": %.4f, \"ms_max\": %.4f, \"tb_per_s\": %.3f}\n", n16 * 16, reps, med, ms.front(),
                ms.back(), (double)(n16 * 16) / (med * 1e-3) / 1e12);
    (void)hipFree(src);
    (void)hipFree(sink);
    return 0;
}
