// tests/observe/observe_host_main.cpp — the host side of the observation tensors as a stand-alone program, for a sanitizer build
// (tests/test_observe_host.py builds it with -fsanitize=address,undefined together with the library's host sources and runs it).
// Through the C-ABI: dg_observe_host at the boundary sizes, every source, rule and dtype, into contiguous NCHW, channels-last and the
// padded slice layout, each in a buffer of exactly the size the layout needs (a read or write past either end is a report) whose
// unaddressed elements are guard bytes; the integer value is taken from dg_reduce_host / dg_reduce_planes_host, float32 and uint8
// elements are checked exactly, the 16-bit ones by widening them back (their exact bits are the Python tier's).  And, from
// observe_core.h, the store phase's lane-to-element map of the colour kernel, lane after lane at the run boundaries.
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../doom-rust-renderer_amd/csrc/observe_core.h"
#include "../../include/doomgpu.h"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("observe_host_main: line %d: %s fails (%s)\n", __LINE__, #cond, dg_last_error()); return 1; } \
    } while (0)

static uint32_t rng_state = 1993;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static float widen_bf16(uint16_t b) {
    const uint32_t u = (uint32_t)b << 16;
    float f;
    std::memcpy(&f, &u, sizeof f);
    return f;
}
static float widen_f16(uint16_t h) {
    const int e = (h >> 10) & 31, m = h & 1023;
    const float mag = e == 0 ? std::ldexp((float)m, -24) : e == 31 ? (m ? NAN : INFINITY) : std::ldexp((float)(m | 1024), e - 25);
    return (h & 0x8000) ? -mag : mag;
}

struct Layout { size_t total, base; int64_t st[4]; };
static Layout layout(int kind, int n, int C, int oH, int oW) {
    const int64_t N = n, c = C, h = oH, w = oW;
    if (kind == 0) return {(size_t)(N * c * h * w), 0, {c * h * w, h * w, w, 1}};
    if (kind == 1) return {(size_t)(N * c * h * w), 0, {h * w * c, 1, w * c, c}};
    const int64_t plane = (h + 1) * (w + 3), frame = (c + 2) * plane + c * h * w;
    return {(size_t)(N * frame), (size_t)plane, {frame, plane, w + 3, 1}};
}

static int run(int W, int H, int fx, int fy, uint32_t source, uint32_t rule, uint32_t dtype, int lay, int n, uint64_t &elements) {
    const bool dist = source == DG_OBS_DISTANCE;
    dg_obs_desc d{(uint32_t)fx, (uint32_t)fy, source, rule, dtype, dist ? -100 : 3, dist ? 2048 : 250, 1.0f, 0.0f, 0u};
    if (dtype != DG_OBS_U8) { d.scale = dist ? 1.0f / 2048.0f : 2.0f / 255.0f; d.bias = dist ? 0.0f : -1.0f; }
    else if (dist) d.lo = 0, d.hi = 255;
    int C = 0, oH = 0, oW = 0, eb = 0;
    CHECK(dg_observed_size(W, H, &d, &C, &oH, &oW, &eb) == DG_OK);
    CHECK(C == (source == DG_OBS_RGB ? 3 : 1) && oW == (W + fx - 1) / fx && oH == (H + fy - 1) / fy && eb == (dtype == DG_OBS_U8 ? 1 : dtype == DG_OBS_F32 ? 4 : 2));
    const size_t px = (size_t)W * (size_t)H, opx = (size_t)oW * (size_t)oH;
    std::vector<uint8_t> rgb(dist ? 0 : (size_t)n * px * 3u), rgb_small(dist ? 0 : (size_t)n * opx * (size_t)C);
    std::vector<int16_t> dp(dist ? (size_t)n * px : 0), dp_small(dist ? (size_t)n * opx : 0);
    for (uint8_t &b : rgb) b = (uint8_t)rng();
    for (int16_t &v : dp) v = (int16_t)(uint16_t)rng();
    if (dist) {
        const dg_plane_reduce_desc pd{(uint32_t)fx, (uint32_t)fy, rule, 0u};
        CHECK(dg_reduce_planes_host(W, H, n, &pd, dp.data(), nullptr, nullptr, nullptr, dp_small.data(), nullptr, nullptr, nullptr) == DG_OK);
    } else {
        const dg_reduce_desc rd{(uint32_t)fx, (uint32_t)fy, source == DG_OBS_GRAY ? (uint32_t)DG_REDUCE_GRAY8 : (uint32_t)DG_REDUCE_RGB24, 0u};
        CHECK(dg_reduce_host(rgb.data(), W, H, n, &rd, rgb_small.data()) == DG_OK);
    }
    const Layout L = layout(lay, n, C, oH, oW);
    std::vector<uint8_t> buf(L.total * (size_t)eb, 0xA5);
    std::vector<uint8_t> written(L.total, 0);
    CHECK(dg_observe_host(dist ? (const void *)dp.data() : (const void *)rgb.data(), W, H, n, &d, buf.data() + L.base * (size_t)eb, L.st) == DG_OK);
    for (int f = 0; f < n; f++)
        for (int c = 0; c < C; c++)
            for (int oy = 0; oy < oH; oy++)
                for (int ox = 0; ox < oW; ox++) {
                    const size_t i = (size_t)f * opx + (size_t)oy * (size_t)oW + (size_t)ox;
                    int v = dist ? (int)dp_small[i] : (int)rgb_small[i * (size_t)C + (size_t)c];
                    v = v < d.lo ? d.lo : v > d.hi ? d.hi : v;
                    const size_t at = L.base + (size_t)(f * L.st[0] + c * L.st[1] + oy * L.st[2] + ox * L.st[3]);
                    CHECK(at < L.total && !written[at]);
                    written[at] = 1;
                    volatile float prod = (float)v * d.scale;
                    const float o = prod + d.bias;
                    if (dtype == DG_OBS_U8) CHECK(buf[at] == (uint8_t)v);
                    else if (dtype == DG_OBS_F32) CHECK(std::memcmp(&buf[at * 4u], &o, 4) == 0);
                    else {
                        uint16_t h;
                        std::memcpy(&h, &buf[at * 2u], 2);
                        const float back = dtype == DG_OBS_F16 ? widen_f16(h) : widen_bf16(h);
                        // |o| <= 1 here; half an ulp of binary16 is <= 2^-12 |o| above its subnormals (2^-25 below), of bfloat16 2^-9 |o|
                        CHECK(std::fabs(back - o) <= (dtype == DG_OBS_F16 ? std::fmax(std::ldexp(std::fabs(o), -11), std::ldexp(1.0f, -25)) : std::ldexp(std::fabs(o), -8)));
                    }
                    elements++;
                }
    for (size_t at = 0; at < L.total; at++)
        if (!written[at])
            for (int b = 0; b < eb; b++) CHECK(buf[at * (size_t)eb + (size_t)b] == 0xA5);       // the gaps are left as they were
    return 0;
}

// Items j = lane, lane + 256, ... of a run of np pixels: every (pixel, channel) once, and a wave's 64 lanes on consecutive addresses
// inside one channel (planar: strides (np, 1)) or across the pixels' channels (channels-last: strides (1, 3)).
static int item_map(uint32_t np) {
    for (int planar = 0; planar < 2; planar++) {
        std::vector<uint8_t> seen(3u * np, 0);
        uint32_t prev_addr = 0;
        for (uint32_t j = 0; j < 3u * np; j++) {
            uint32_t p = ~0u, c = ~0u;
            dg::obs_item(j, np, planar != 0, p, c);
            CHECK(p < np && c < 3u && !seen[3u * p + c]);
            seen[3u * p + c] = 1;
            const uint32_t addr = planar ? c * np + p : 3u * p + c;
            CHECK(addr == j);                               // item j is element j of the run in its layout's own order
            CHECK(j == 0 || addr == prev_addr + 1u);
            prev_addr = addr;
        }
    }
    return 0;
}

int main() {
    const int sizes[][2] = {{64, 40}, {131, 67}, {5, 9}, {1, 1}, {16, 16}, {17, 33}};
    const int factors[][2] = {{1, 1}, {3, 3}, {7, 3}, {16, 16}};
    const uint32_t kinds[][2] = {{DG_OBS_RGB, 0}, {DG_OBS_GRAY, 0}, {DG_OBS_DISTANCE, DG_PLANE_POINT}, {DG_OBS_DISTANCE, DG_PLANE_NEAREST}};
    uint64_t elements = 0;
    for (auto &s : sizes)
        for (auto &f : factors)
            for (auto &k : kinds)
                for (uint32_t dtype = 0; dtype < 4; dtype++)
                    for (int lay = 0; lay < 3; lay++)
                        if (run(s[0], s[1], f[0], f[1], k[0], k[1], dtype, lay, lay == 2 ? 3 : 2, elements)) return 1;
    for (uint32_t np : {1u, 2u, 63u, 64u, 65u, 85u, 86u, 255u, 256u, 257u, 1360u})
        if (item_map(np)) return 1;
    // the error returns: nothing is read or written (every pointer below is one element)
    alignas(4) uint8_t s1[4] = {0, 0, 0, 0};
    alignas(4) uint8_t d1[4] = {0x5a, 0x5a, 0x5a, 0x5a};
    const int64_t st[4] = {1, 1, 1, 1};
    const dg_obs_desc good{1, 1, DG_OBS_GRAY, 0, DG_OBS_F32, -32768, 32767, 1.0f, 0.0f, 0};
    CHECK(dg_observe_host(s1, 1, 1, 0, &good, d1, st) == DG_OK && d1[0] == 0x5a);
    CHECK(dg_observe_host(nullptr, 1, 1, 1, &good, d1, st) == DG_ERR_INVALID);
    CHECK(dg_observe_host(s1, 1, 1, 1, &good, nullptr, st) == DG_ERR_INVALID);
    CHECK(dg_observe_host(s1, 1, 1, 1, &good, d1, nullptr) == DG_ERR_INVALID);
    CHECK(dg_observe_host(s1, 1, 1, 1, nullptr, d1, st) == DG_ERR_INVALID);
    CHECK(dg_observe_host(s1, 1, 1, -1, &good, d1, st) == DG_ERR_INVALID);
    CHECK(dg_observe_host(s1, 1, 1, 1, &good, d1 + 1, st) == DG_ERR_INVALID);
    const int64_t zero[4] = {1, 1, 0, 1};
    CHECK(dg_observe_host(s1, 1, 1, 1, &good, d1, zero) == DG_ERR_INVALID);
    dg_obs_desc bad = good;
    bad.scale = INFINITY;
    CHECK(dg_observe_host(s1, 1, 1, 1, &bad, d1, st) == DG_ERR_INVALID);
    CHECK(d1[0] == 0x5a && d1[3] == 0x5a);
    std::printf("observe_host_main: ok (%llu elements)\n", (unsigned long long)elements);
    return 0;
}
