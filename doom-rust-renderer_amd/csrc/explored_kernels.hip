// explored_kernels.hip — explored-map frames: which linedefs a session has had on screen, from its label planes,
// and the 2-D map drawn through that set.  The rules are explored_core.h's; everything is integer.
//
// dg_seen_lines   one workgroup per (frame, band of SEEN_BAND_PX consecutive pixels).  It reads 3 bytes per pixel and writes almost nothing:
//                 a bitset of the scene's segs in LDS (at most 8 KB), a lane ORs into it only when the wall seg differs from the last one
//                 it ORed (walls are long horizontal runs), and at the band's end every set bit goes through the seg -> linedef table into
//                 the frame's row in global memory with one vector atomic OR.  A line reached from several bands or segs is ORed more than
//                 once; the order cannot show.  <true>: 16 pixels per lane and step as one 16-byte load of cls and two of id (planes on
//                 16-byte boundaries, W * H a multiple of 16); <false>: any 2-byte aligned id, any cls, any size, a pixel per lane and step.
// dg_seen_accumulate   one lane per (run, word) walks its run's frames in order: the loads do not depend on each other.
// dg_seen_counts       one lane per frame: popcounts of its row and of what it adds to the row before it.
// dg_map_explored      replaces dg_map_copy for these frames: the frame's mask row staged in LDS, per pixel explored_pick over the cover
//                      (L2 / Infinity Cache resident: 4 MB at 1280x800) and non-temporal stores in the widest form that keeps every frame
//                      start aligned: <16, 2> 16 pixels = four 16-byte cover loads and three 16-byte stores per item, <4, 4> 4 pixels = three
//                      dword stores (3 W H a multiple of 4), <1, 4> bytes.  Every item is bounds-checked against the frame.
// The arrow on top is map_kernels.hip's dg_map_arrow (launch_map_arrow).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>

#include "explored_kernels.hpp"
#include "map_kernels.hpp"

namespace dg {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr uint32_t SEEN_BAND_PX = 16384u;                 // pixels of one band: 4 steps of 256 lanes x 16 pixels
constexpr uint32_t SEEN_STEPS = SEEN_BAND_PX / (16u * kThreads);
constexpr uint32_t SEEN_ACC_DEPTH = 16u;                  // frames a lane of dg_seen_accumulate loads before it ORs and stores them
constexpr int kMaxY = 65535;                              // frames per launch: the grid's y extent

template <bool WIDE>
__global__ void __launch_bounds__(kThreads) dg_seen_lines(const uint16_t *__restrict__ id, const uint8_t *__restrict__ cls, uint32_t px,
                                                          const uint32_t *__restrict__ seg_line, uint32_t n_segs, uint32_t *__restrict__ seen,
                                                          uint32_t words) {
    __shared__ uint32_t bits[SEEN_MAX_SEG_WORDS];
    const uint32_t tid = threadIdx.x, f = blockIdx.y;
    const uint32_t seg_words = (n_segs + 31u) / 32u;      // <= SEEN_MAX_SEG_WORDS (the launcher checks)
    for (uint32_t w = tid; w < seg_words; w += kThreads) bits[w] = 0u;
    __syncthreads();
    const uint32_t p0 = blockIdx.x * SEEN_BAND_PX, p1 = min(px, p0 + SEEN_BAND_PX);
    const uint16_t *const fid = id + (size_t)f * px;
    const uint8_t *const fcls = cls + (size_t)f * px;
    uint32_t last = 0xffffffffu;                          // the seg this lane ORed last
    auto note = [&](uint32_t c, uint32_t s) {
        if (seen_pixel(c, s, n_segs) && s != last) {
            atomicOr(&bits[s >> 5], 1u << (s & 31u));
            last = s;
        }
    };
    if (WIDE) {
        uint4 c[SEEN_STEPS], a[SEEN_STEPS], b[SEEN_STEPS];
#pragma unroll
        for (uint32_t i = 0; i < SEEN_STEPS; i++) {       // px and the band are multiples of 16: a piece that starts inside the band ends inside it
            const uint32_t q = p0 + 16u * (i * kThreads + tid);
            c[i] = make_uint4(0u, 0u, 0u, 0u); a[i] = c[i]; b[i] = c[i];
            if (q < p1) {
                c[i] = *reinterpret_cast<const uint4 *>(fcls + q);
                a[i] = *reinterpret_cast<const uint4 *>(fid + q);
                b[i] = *reinterpret_cast<const uint4 *>(fid + q + 8);
            }
        }
#pragma unroll
        for (uint32_t i = 0; i < SEEN_STEPS; i++) {
            const uint32_t cw[4] = {c[i].x, c[i].y, c[i].z, c[i].w};
            const uint32_t iw[8] = {a[i].x, a[i].y, a[i].z, a[i].w, b[i].x, b[i].y, b[i].z, b[i].w};
#pragma unroll
            for (uint32_t j = 0; j < 16u; j++) note((cw[j >> 2] >> (8u * (j & 3u))) & 255u, (iw[j >> 1] >> (16u * (j & 1u))) & 0xffffu);
        }
    } else {
        for (uint32_t q = p0 + tid; q < p1; q += kThreads) note(fcls[q], fid[q]);
    }
    __syncthreads();
    uint32_t *const row = seen + (size_t)f * words;
    for (uint32_t w = tid; w < seg_words; w += kThreads) {
        uint32_t v = bits[w];
        while (v) {
            const uint32_t seg = 32u * w + (uint32_t)(__ffs((int)v) - 1);     // < n_segs: only such bits were set
            v &= v - 1u;
            const uint32_t line = seg_line[seg];
            if ((line >> 5) < words) atomicOr(&row[line >> 5], 1u << (line & 31u));
        }
    }
}

__global__ void __launch_bounds__(kThreads) dg_seen_accumulate(const uint32_t *__restrict__ seen, uint32_t words, uint32_t runs, uint32_t run_len,
                                                               const uint32_t *__restrict__ carry_in, uint32_t *__restrict__ upto,
                                                               uint32_t *__restrict__ carry_out) {
    const size_t idx = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= (size_t)runs * words) return;
    const size_t run = idx / words, w = idx % words;
    uint32_t acc = carry_in ? carry_in[idx] : 0u;
    size_t at = run * run_len * words + w;
    uint32_t f = 0;
    for (; f + SEEN_ACC_DEPTH <= run_len; f += SEEN_ACC_DEPTH) {   // the loads of a piece are in flight together: a lane's walk is latency, not bytes
        uint32_t v[SEEN_ACC_DEPTH];
#pragma unroll
        for (uint32_t i = 0; i < SEEN_ACC_DEPTH; i++) v[i] = seen[at + (size_t)i * words];
#pragma unroll
        for (uint32_t i = 0; i < SEEN_ACC_DEPTH; i++, at += words) {
            acc |= v[i];
            upto[at] = acc;
        }
    }
    for (; f < run_len; f++, at += words) {
        acc |= seen[at];
        upto[at] = acc;
    }
    if (carry_out) carry_out[idx] = acc;
}

__global__ void __launch_bounds__(kThreads) dg_seen_counts(const uint32_t *__restrict__ upto, uint32_t words, uint32_t n_frames, uint32_t run_len,
                                                           const uint32_t *__restrict__ carry_in, uint32_t *__restrict__ total,
                                                           uint32_t *__restrict__ fresh) {
    const uint32_t f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= n_frames) return;
    const uint32_t *const row = upto + (size_t)f * words;
    const uint32_t *const prev = f % run_len ? row - words : carry_in ? carry_in + (size_t)(f / run_len) * words : nullptr;
    uint32_t t = 0u, n = 0u;
    for (uint32_t w = 0; w < words; w++) {
        const uint32_t v = row[w];
        t += __popc(v);
        n += __popc(v & ~(prev ? prev[w] : 0u));
    }
    if (total) total[f] = t;
    if (fresh) fresh[f] = n;
}

// PX pixels per item, ITEMS items per lane, frame blockIdx.y.  A lane's cover loads are issued first, so that they are in flight while the
// mask row is staged: a workgroup is one chain of latencies (mask row, barrier, cover, stores), not a stream.
template <int PX, int ITEMS>
__global__ void __launch_bounds__(kThreads) dg_map_explored(const uint32_t *__restrict__ cover, const uint32_t *__restrict__ chains,
                                                            const uint32_t *__restrict__ masks, uint32_t words, uint8_t *__restrict__ fb, uint32_t px) {
    __shared__ uint32_t mask[EXPLORED_MAX_WORDS];
    constexpr int Q = PX == 1 ? 1 : PX / 4;                // PX > 1: groups of 4 pixels = 16 bytes of cover = 12 bytes of frame
    const uint32_t n_items = px / PX;                      // PX divides px (the launcher picks PX so)
    const uint32_t j0 = blockIdx.x * (uint32_t)(kThreads * ITEMS) + threadIdx.x;
    uint4 v[ITEMS][Q];
#pragma unroll
    for (int i = 0; i < ITEMS; i++) {
        const uint32_t j = j0 + (uint32_t)(i * kThreads);
#pragma unroll
        for (int g = 0; g < Q; g++) {
            v[i][g] = make_uint4(0u, 0u, 0u, 0u);
            if (j < n_items) {
                if constexpr (PX == 1) v[i][g].x = cover[j];
                else v[i][g] = reinterpret_cast<const uint4 *>(cover)[(size_t)j * Q + g];
            }
        }
    }
    const uint32_t *const row = masks + (size_t)blockIdx.y * words;
    for (uint32_t w = threadIdx.x; w < words; w += kThreads) mask[w] = row[w];      // words <= EXPLORED_MAX_WORDS (the launcher checks)
    __syncthreads();
    uint8_t *const frame = fb + (size_t)blockIdx.y * 3u * (size_t)px;
#pragma unroll
    for (int i = 0; i < ITEMS; i++) {
        const uint32_t j = j0 + (uint32_t)(i * kThreads);
        if (j >= n_items) continue;
        if constexpr (PX == 1) {
            const uint32_t rgb = explored_pick(v[i][0].x, chains, mask);
            uint8_t *const o = frame + 3u * (size_t)j;
            o[0] = (uint8_t)rgb; o[1] = (uint8_t)(rgb >> 8); o[2] = (uint8_t)(rgb >> 16);
        } else {
            uint32_t o[3 * Q];
#pragma unroll
            for (int g = 0; g < Q; g++) {
                const uint32_t c0 = explored_pick(v[i][g].x, chains, mask), c1 = explored_pick(v[i][g].y, chains, mask);
                const uint32_t c2 = explored_pick(v[i][g].z, chains, mask), c3 = explored_pick(v[i][g].w, chains, mask);
                o[3 * g + 0] = c0 | (c1 << 24);
                o[3 * g + 1] = (c1 >> 8) | (c2 << 16);
                o[3 * g + 2] = (c2 >> 16) | (c3 << 8);
            }
            if constexpr (PX == 16) {
                u32x4 *const dst = reinterpret_cast<u32x4 *>(frame) + (size_t)j * 3u;
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    u32x4 t;
                    t.x = o[4 * k + 0]; t.y = o[4 * k + 1]; t.z = o[4 * k + 2]; t.w = o[4 * k + 3];
                    __builtin_nontemporal_store(t, dst + k);
                }
            } else {
                uint32_t *const dst = reinterpret_cast<uint32_t *>(frame) + (size_t)j * 3u;
#pragma unroll
                for (int k = 0; k < 3; k++) __builtin_nontemporal_store(o[k], dst + k);
            }
        }
    }
}

unsigned blocks_for(size_t items, size_t cap) {
    return (unsigned)std::max<size_t>(1, std::min<size_t>((items + kThreads - 1) / kThreads, cap));
}

}  // namespace

hipError_t launch_seen_lines(const uint16_t *id, const uint8_t *cls, int W, int H, int n_frames, const uint32_t *seg_line, uint32_t n_segs,
                             uint32_t *seen, uint32_t words, hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
    if (n_frames <= 0) return hipSuccess;
    if (n_segs > 32u * SEEN_MAX_SEG_WORDS || reinterpret_cast<uintptr_t>(id) % 2u) return hipErrorInvalidValue;
    const uint32_t px = (uint32_t)W * (uint32_t)H;
    const bool wide = px % 16u == 0u && reinterpret_cast<uintptr_t>(id) % 16u == 0u && reinterpret_cast<uintptr_t>(cls) % 16u == 0u;
    const unsigned bands = (px + SEEN_BAND_PX - 1u) / SEEN_BAND_PX;
    for (int f0 = 0; f0 < n_frames; f0 += kMaxY) {
        const int nf = std::min(kMaxY, n_frames - f0);
        const dim3 grid(bands, (unsigned)nf);
        hipEvent_t ev0 = f0 == 0 ? start : nullptr, ev1 = f0 + nf == n_frames ? stop : nullptr;
        const uint16_t *const i0 = id + (size_t)f0 * px;
        const uint8_t *const c0 = cls + (size_t)f0 * px;
        uint32_t *const s0 = seen + (size_t)f0 * words;
        if (wide) hipExtLaunchKernelGGL(dg_seen_lines<true>, grid, dim3(kThreads), 0, stream, ev0, ev1, 0, i0, c0, px, seg_line, n_segs, s0, words);
        else hipExtLaunchKernelGGL(dg_seen_lines<false>, grid, dim3(kThreads), 0, stream, ev0, ev1, 0, i0, c0, px, seg_line, n_segs, s0, words);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_seen_accumulate(const uint32_t *seen, uint32_t words, int n_frames, int run_len, const uint32_t *carry_in, uint32_t *upto,
                                  uint32_t *total, uint32_t *fresh, uint32_t *carry_out, hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
    if (n_frames <= 0) return hipSuccess;
    if (run_len < 1 || n_frames % run_len || !upto || words == 0u) return hipErrorInvalidValue;
    const uint32_t runs = (uint32_t)(n_frames / run_len);
    const bool counts = total || fresh;
    hipExtLaunchKernelGGL(dg_seen_accumulate, dim3(blocks_for((size_t)runs * words, 1u << 30)), dim3(kThreads), 0, stream, start, counts ? nullptr : stop, 0,
                          seen, words, runs, (uint32_t)run_len, carry_in, upto, carry_out);
    if (counts)
        hipExtLaunchKernelGGL(dg_seen_counts, dim3(blocks_for((size_t)n_frames, 1u << 30)), dim3(kThreads), 0, stream, nullptr, stop, 0,
                              (const uint32_t *)upto, words, (uint32_t)n_frames, (uint32_t)run_len, carry_in, total, fresh);
    return hipGetLastError();
}

hipError_t launch_explored_frames(const uint32_t *cover, const uint32_t *chains, const uint32_t *masks, uint32_t words, const MapSeg *arrow,
                                  int n_frames, uint8_t *fb, int W, int H, hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
    if (n_frames <= 0) return hipSuccess;
    if (words == 0u || words > EXPLORED_MAX_WORDS) return hipErrorInvalidValue;
    const uint32_t px = (uint32_t)W * (uint32_t)H;
    const size_t fsz = (size_t)3 * px;
    for (int f0 = 0; f0 < n_frames; f0 += kMaxY) {         // more frames than the grid's y extent take several launches, as in launch_seen_lines
        const int nf = std::min(kMaxY, n_frames - f0);
        hipEvent_t ev0 = f0 == 0 ? start : nullptr, ev1 = f0 + nf == n_frames ? stop : nullptr;
        const uint32_t *const m0 = masks + (size_t)f0 * words;
        uint8_t *const fb0 = fb + (size_t)f0 * fsz;
        // 2 x 16 pixels per lane (4 x 4, 4 x 1 in the narrower forms): enough workgroups per frame to fill the chip at any batch size
        auto blocks = [&](uint32_t n_items, int items) { return dim3((n_items + (uint32_t)(kThreads * items) - 1u) / (uint32_t)(kThreads * items), (unsigned)nf); };
        if (fsz % 16 == 0)
            hipExtLaunchKernelGGL((dg_map_explored<16, 2>), blocks(px / 16u, 2), dim3(kThreads), 0, stream, ev0, nullptr, 0, cover, chains, m0, words, fb0, px);
        else if (fsz % 4 == 0)
            hipExtLaunchKernelGGL((dg_map_explored<4, 4>), blocks(px / 4u, 4), dim3(kThreads), 0, stream, ev0, nullptr, 0, cover, chains, m0, words, fb0, px);
        else
            hipExtLaunchKernelGGL((dg_map_explored<1, 4>), blocks(px, 4), dim3(kThreads), 0, stream, ev0, nullptr, 0, cover, chains, m0, words, fb0, px);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = launch_map_arrow(arrow + (size_t)3 * f0, nf, fb0, W, H, stream, nullptr, ev1);   // (this chunk's lines into this chunk's frames)
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace dg
