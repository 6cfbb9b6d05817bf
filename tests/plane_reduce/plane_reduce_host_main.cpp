// tests/plane_reduce/plane_reduce_host_main.cpp — the host side of the reduced depth and label planes as a stand-alone program, for a
// sanitizer build (tests/test_plane_reduce_host.py builds it with -fsanitize=address,undefined together with the library's host sources
// and runs it).  Through the C-ABI alone: dg_reduce_planes_host over the grid of sizes and box sizes of the Python tiers, both rules, 1 and
// 3 frames, pairs left out, buffers of exactly the size the contract names (so that a read or write past either end is a report), and
// the error returns.  It checks what it gets against the rule restated here as plain loops.
#include <cstdio>
#include <cstdint>
#include <vector>

#include "../../include/doomgpu.h"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("plane_reduce_host_main: line %d: %s fails (%s)\n", __LINE__, #cond, dg_last_error()); return 1; } \
    } while (0)

static uint32_t rng_state = 1993;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// The representative of box (ox, oy) by the contract's text.
static void representative(const int16_t *d, int W, int H, int fx, int fy, uint32_t rule, int ox, int oy, int &x, int &y) {
    if (rule == DG_PLANE_POINT) {
        x = ox * fx + fx / 2; if (x > W - 1) x = W - 1;
        y = oy * fy + fy / 2; if (y > H - 1) y = H - 1;
        return;
    }
    bool have = false;
    int best = 0;
    for (int yy = oy * fy; yy < oy * fy + fy && yy < H; yy++)
        for (int xx = ox * fx; xx < ox * fx + fx && xx < W; xx++)
            if (!have || d[yy * W + xx] < best) { have = true; best = d[yy * W + xx]; x = xx; y = yy; }
}

static int run(int W, int H, int fx, int fy, uint32_t rule, int n, int content, unsigned leave_out, uint64_t &pixels) {
    const size_t px = (size_t)W * (size_t)H;
    const dg_plane_reduce_desc desc{(uint32_t)fx, (uint32_t)fy, rule, 0u};
    int oW = 0, oH = 0;
    CHECK(dg_plane_reduced_size(W, H, &desc, &oW, &oH) == DG_OK);
    CHECK(oW == (W + fx - 1) / fx && oH == (H + fy - 1) / fy);
    const size_t opx = (size_t)oW * (size_t)oH;
    std::vector<int16_t> d((size_t)n * px), od((size_t)n * opx, 0x5a5a);
    std::vector<uint8_t> k((size_t)n * px), c((size_t)n * px), ok((size_t)n * opx, 0x5a), oc((size_t)n * opx, 0x5a);
    std::vector<uint16_t> id((size_t)n * px), oid((size_t)n * opx, 0x5a5a);
    for (size_t i = 0; i < (size_t)n * px; i++) {
        const size_t p = i % px;
        d[i] = content == 0 ? (int16_t)(uint16_t)rng() : content == 1 ? (int16_t)-5 : (int16_t)(rng() % 3u == 0u ? 32767 : (int)(rng() % 7u) - 3);
        id[i] = (uint16_t)(p & 0xFFFFu);
        c[i] = (uint8_t)(id[i] & 7u);
        k[i] = (uint8_t)((id[i] >> 3) & 3u);
    }
    const bool no_d = leave_out & 1u, no_k = leave_out & 2u, no_i = leave_out & 4u, no_c = leave_out & 8u;
    const int rc = dg_reduce_planes_host(W, H, n, &desc, no_d ? nullptr : d.data(), no_k ? nullptr : k.data(), no_i ? nullptr : id.data(), no_c ? nullptr : c.data(),
                                         no_d ? nullptr : od.data(), no_k ? nullptr : ok.data(), no_i ? nullptr : oid.data(), no_c ? nullptr : oc.data());
    if (rule == DG_PLANE_NEAREST && no_d) {
        CHECK(rc == DG_ERR_INVALID);
        for (size_t i = 0; i < (size_t)n * opx; i++) CHECK(ok[i] == 0x5a && oid[i] == 0x5a5a && oc[i] == 0x5a);
        return 0;
    }
    CHECK(rc == DG_OK);
    for (int f = 0; f < n; f++)
        for (int oy = 0; oy < oH; oy++)
            for (int ox = 0; ox < oW; ox++) {
                int x = -1, y = -1;
                representative(d.data() + (size_t)f * px, W, H, fx, fy, rule, ox, oy, x, y);
                const size_t s = (size_t)f * px + (size_t)y * (size_t)W + (size_t)x, o = (size_t)f * opx + (size_t)oy * (size_t)oW + (size_t)ox;
                CHECK(od[o] == (no_d ? (int16_t)0x5a5a : d[s]));
                CHECK(ok[o] == (no_k ? (uint8_t)0x5a : k[s]));
                CHECK(oid[o] == (no_i ? (uint16_t)0x5a5a : id[s]));
                CHECK(oc[o] == (no_c ? (uint8_t)0x5a : c[s]));
                pixels++;
            }
    return 0;
}

int main() {
    const int sizes[][2] = {{64, 40}, {80, 50}, {131, 67}, {5, 9}, {1, 1}, {320, 200}};
    const int factors[][2] = {{1, 1}, {2, 2}, {3, 3}, {4, 5}, {7, 3}, {16, 16}, {16, 1}, {1, 16}};
    uint64_t pixels = 0;
    for (auto &s : sizes)
        for (auto &f : factors)
            for (uint32_t rule : {(uint32_t)DG_PLANE_POINT, (uint32_t)DG_PLANE_NEAREST})
                for (int content = 0; content < 3; content++)
                    for (int n : {1, 3})
                        if (run(s[0], s[1], f[0], f[1], rule, n, content, 0u, pixels)) return 1;
    for (unsigned leave_out = 1; leave_out < 15; leave_out++)
        for (uint32_t rule : {(uint32_t)DG_PLANE_POINT, (uint32_t)DG_PLANE_NEAREST})
            if (run(131, 67, 7, 3, rule, 2, 0, leave_out, pixels)) return 1;
    // the error returns: nothing is read or written (every plane pointer below is one element)
    int16_t d1 = 0, od1 = 0;
    const dg_plane_reduce_desc good{2, 2, DG_PLANE_NEAREST, 0};
    const dg_plane_reduce_desc bad[] = {{0, 2, 0, 0}, {2, 17, 0, 0}, {2, 2, 2, 0}, {2, 2, 1, 9}};
    for (const dg_plane_reduce_desc &b : bad) {
        CHECK(dg_plane_reduced_size(8, 8, &b, nullptr, nullptr) == DG_ERR_INVALID);
        CHECK(dg_reduce_planes_host(8, 8, 1, &b, &d1, nullptr, nullptr, nullptr, &od1, nullptr, nullptr, nullptr) == DG_ERR_INVALID);
    }
    CHECK(dg_reduce_planes_host(8, 8, 1, nullptr, &d1, nullptr, nullptr, nullptr, &od1, nullptr, nullptr, nullptr) == DG_ERR_INVALID);
    CHECK(dg_reduce_planes_host(0, 8, 1, &good, &d1, nullptr, nullptr, nullptr, &od1, nullptr, nullptr, nullptr) == DG_ERR_INVALID);
    CHECK(dg_reduce_planes_host(8, 16385, 1, &good, &d1, nullptr, nullptr, nullptr, &od1, nullptr, nullptr, nullptr) == DG_ERR_INVALID);
    CHECK(dg_reduce_planes_host(8, 8, -1, &good, &d1, nullptr, nullptr, nullptr, &od1, nullptr, nullptr, nullptr) == DG_ERR_INVALID);
    CHECK(dg_reduce_planes_host(8, 8, 1, &good, &d1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == DG_ERR_INVALID);
    CHECK(dg_reduce_planes_host(8, 8, 1, &good, nullptr, nullptr, nullptr, nullptr, &od1, nullptr, nullptr, nullptr) == DG_ERR_INVALID);
    CHECK(dg_reduce_planes_host(1, 1, 1, &good, &d1, nullptr, nullptr, nullptr, &od1, nullptr, nullptr, nullptr) == DG_OK);
    CHECK(dg_reduce_planes_host(8, 8, 0, &good, &d1, nullptr, nullptr, nullptr, &od1, nullptr, nullptr, nullptr) == DG_OK);
    std::printf("plane_reduce_host_main: ok (%llu output pixels)\n", (unsigned long long)pixels);
    return 0;
}
