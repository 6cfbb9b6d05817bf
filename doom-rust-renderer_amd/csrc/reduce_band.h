// reduce_band.h — phase 1 of the band kernels, stated once for the kernels that write reduced frames and planes (reduce_kernels.hip,
// plane_reduce_kernels.hip) and the ones that write observation tensors (observe_kernels.hip): a workgroup's lanes read a band of
// ny <= 16 source rows of one run and leave one value per source byte / column of the run in LDS.  Device code only; the caller's
// barrier follows.
#pragma once
#include <hip/hip_runtime.h>

#include "plane_reduce_kernels.hpp"
#include "reduce_kernels.hpp"

namespace dg {

// RGB24: sums[off0 + (b - b0)] = the sum over the band's rows of byte b of a row, for b in [b0, b1); returns off0.
//   PIECES: one 16-byte piece per lane and row, the pieces of a row consecutive and 16-byte aligned (row_bytes % 16 == 0, aligned
//   rows), so the run starts up to 15 bytes in front of b0; otherwise the lanes of a wave read 64 consecutive bytes per load, 16 loads
//   per row, and off0 = 0.
template <bool PIECES>
__device__ __forceinline__ uint32_t reduce_band_sums(uint16_t *sums, const uint8_t *rows, uint32_t row_bytes, uint32_t ny, uint32_t b0, uint32_t b1,
                                                     uint32_t tid) {
    uint32_t off0 = 0;                                                         // sums[off0] is byte b0
    if (PIECES) {
        const uint32_t a = b0 & ~15u;
        off0 = b0 - a;
        const uint32_t pos = a + 16u * tid;                                    // pos + 16 <= row_bytes: both are multiples of 16
        if (pos < b1) {
            // bytes 0 and 2 of each dword in ev, 1 and 3 in od: two 16-bit sums per register
            uint32_t ev[4] = {0u, 0u, 0u, 0u}, od[4] = {0u, 0u, 0u, 0u};
            for (uint32_t r = 0; r < ny; r += 4u) {
                uint4 v[4];
#pragma unroll
                for (uint32_t i = 0; i < 4u; i++) {
                    v[i] = make_uint4(0u, 0u, 0u, 0u);
                    if (r + i < ny) v[i] = *reinterpret_cast<const uint4 *>(rows + (size_t)(r + i) * row_bytes + pos);
                }
#pragma unroll
                for (uint32_t i = 0; i < 4u; i++) {
                    ev[0] += v[i].x & 0x00FF00FFu; od[0] += (v[i].x >> 8) & 0x00FF00FFu;
                    ev[1] += v[i].y & 0x00FF00FFu; od[1] += (v[i].y >> 8) & 0x00FF00FFu;
                    ev[2] += v[i].z & 0x00FF00FFu; od[2] += (v[i].z >> 8) & 0x00FF00FFu;
                    ev[3] += v[i].w & 0x00FF00FFu; od[3] += (v[i].w >> 8) & 0x00FF00FFu;
                }
            }
            uint32_t w[8];
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) {
                w[2 * k] = (ev[k] & 0xFFFFu) | (od[k] << 16);
                w[2 * k + 1] = (ev[k] >> 16) | (od[k] & 0xFFFF0000u);
            }
            uint4 *const o = reinterpret_cast<uint4 *>(sums + 16u * tid);
            o[0] = make_uint4(w[0], w[1], w[2], w[3]);
            o[1] = make_uint4(w[4], w[5], w[6], w[7]);
        }
    } else {
        uint32_t acc[16];
#pragma unroll
        for (uint32_t i = 0; i < 16u; i++) acc[i] = 0u;
        for (uint32_t r = 0; r < ny; r++) {
            const uint8_t *const row = rows + (size_t)r * row_bytes;
#pragma unroll
            for (uint32_t i = 0; i < 16u; i++) {
                const uint32_t pos = b0 + tid + REDUCE_LANES * i;
                if (pos < b1) acc[i] += row[pos];
            }
        }
#pragma unroll
        for (uint32_t i = 0; i < 16u; i++)
            if (b0 + tid + REDUCE_LANES * i < b1) sums[tid + REDUCE_LANES * i] = (uint16_t)acc[i];
    }
    return off0;
}

// int16 distances: cols[off0 + (c - c0)] = the minimum over the band's rows of plane_col_key(distance, row) of column c, for c in
// [c0, c1); returns off0.  PIECES: one 16-byte piece of 8 distances per lane and row (W % 8 == 0, 16-byte aligned rows), so the run
// starts up to 7 columns in front of c0; otherwise the lanes of a wave read 64 consecutive distances per load, 8 loads per row.
template <bool PIECES>
__device__ __forceinline__ uint32_t plane_band_keys(uint32_t *cols, const int16_t *rows, uint32_t W, uint32_t ny, uint32_t c0, uint32_t c1, uint32_t tid) {
    const uint32_t a = PIECES ? c0 & ~7u : c0;
    const uint32_t off0 = c0 - a;                                              // cols[off0] is column c0
    const uint32_t pos = a + 8u * tid;                                         // PIECES: pos + 8 <= W, both are multiples of 8
    uint32_t k[8];
#pragma unroll
    for (uint32_t i = 0; i < 8u; i++) k[i] = PLANE_KEY_NONE;
    if (PIECES) {
        if (pos < c1) {
            for (uint32_t r = 0; r < ny; r += 4u) {
                uint4 v[4];
#pragma unroll
                for (uint32_t i = 0; i < 4u; i++) {
                    v[i] = make_uint4(0u, 0u, 0u, 0u);
                    if (r + i < ny) v[i] = *reinterpret_cast<const uint4 *>(rows + (size_t)(r + i) * W + pos);
                }
#pragma unroll
                for (uint32_t i = 0; i < 4u; i++) {
                    if (r + i < ny) {
                        const uint32_t ry = r + i;
                        k[0] = min(k[0], plane_col_key(v[i].x, ry)); k[1] = min(k[1], plane_col_key(v[i].x >> 16, ry));
                        k[2] = min(k[2], plane_col_key(v[i].y, ry)); k[3] = min(k[3], plane_col_key(v[i].y >> 16, ry));
                        k[4] = min(k[4], plane_col_key(v[i].z, ry)); k[5] = min(k[5], plane_col_key(v[i].z >> 16, ry));
                        k[6] = min(k[6], plane_col_key(v[i].w, ry)); k[7] = min(k[7], plane_col_key(v[i].w >> 16, ry));
                    }
                }
            }
            uint4 *const o = reinterpret_cast<uint4 *>(cols + 8u * tid);
            o[0] = make_uint4(k[0], k[1], k[2], k[3]);
            o[1] = make_uint4(k[4], k[5], k[6], k[7]);
        }
    } else {
        const uint16_t *const urows = reinterpret_cast<const uint16_t *>(rows);
        for (uint32_t r = 0; r < ny; r++) {
            const uint16_t *const row = urows + (size_t)r * W;
#pragma unroll
            for (uint32_t i = 0; i < 8u; i++) {
                const uint32_t col = c0 + tid + PLANE_REDUCE_LANES * i;
                if (col < c1) k[i] = min(k[i], plane_col_key(row[col], r));
            }
        }
#pragma unroll
        for (uint32_t i = 0; i < 8u; i++)
            if (c0 + tid + PLANE_REDUCE_LANES * i < c1) cols[tid + PLANE_REDUCE_LANES * i] = k[i];
    }
    return off0;
}

}  // namespace dg
