// CPU check of the slab layouts (doom-rust-renderer_amd/csrc/slab_layout.h) over a grid of frame widths, batch sizes, scene sizes and
// effect switches.  For every layout: each piece starts on a 256-byte boundary, pieces follow each other in declaration order without
// overlapping (their sizes are restated here from the record types), every offset is monotone in every count, and a full batch with
// every count at its cap fits the capacity dg_create allocates — restated here as the term-by-term sum it always was.
// Prints "ok <configurations> <checks>" or the first failure.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../doom-rust-renderer_amd/csrc/slab_layout.h"

using namespace dg;

static long long g_checks = 0;
static char g_where[256];

#define CHECK(cond)                                                                  \
    do {                                                                             \
        g_checks++;                                                                  \
        if (!(cond)) { std::printf("FAIL %s: %s (line %d)\n", g_where, #cond, __LINE__); std::exit(1); } \
    } while (0)

struct Piece { size_t at, bytes; };

// aligned, in order, not overlapping, and the slab ends where its last piece ends
static void check_pieces(const std::vector<Piece> &p, size_t total) {
    CHECK(!p.empty() && p[0].at == 0);
    for (size_t i = 0; i < p.size(); i++) {
        CHECK(p[i].at % 256 == 0);
        if (i + 1 < p.size()) { CHECK(p[i].at <= p[i + 1].at); CHECK(p[i].at + p[i].bytes <= p[i + 1].at); CHECK(p[i + 1].at - (p[i].at + p[i].bytes) < 256); }
    }
    CHECK(total == p.back().at + p.back().bytes);
}

static size_t up(size_t v) { return (v + 255) / 256 * 256; }

static std::vector<Piece> list_pieces(const ListLayout &L, size_t n, size_t W, size_t walls, size_t planes, size_t spans) {
    return {{L.frames, n * sizeof(DevFrame)}, {L.col_off, n * (W + 1) * 4}, {L.walls, walls * sizeof(DevWallRec)}, {L.planes, planes * sizeof(DevPlaneRec)},
            {L.spans, spans * sizeof(DevSpan)}};
}
static std::vector<size_t> offsets(const ListLayout &L) { return {L.frames, L.col_off, L.walls, L.planes, L.spans, L.total}; }

static std::vector<Piece> fe_pieces(const FeLayout &L, size_t n, size_t W, const size_t c[6]) {
    const size_t nb1 = (W + 63) / 64 + 1;
    return {{L.frames, n * sizeof(DevFrame)}, {L.fframes, n * sizeof(FeFrame)}, {L.parts, c[0] * sizeof(FePart)}, {L.sprites, c[1] * sizeof(FeSprite)},
            {L.behind, c[2] * 4}, {L.sky, c[3] * 4}, {L.bin_off, n * nb1 * 4}, {L.sbin_off, n * nb1 * 4}, {L.bins, c[4] * 2}, {L.sbins, c[5] * 2},
            {L.order, n * ((W + 255) / 256) * 4}};
}
static std::vector<size_t> offsets(const FeLayout &L) {
    return {L.frames, L.fframes, L.parts, L.sprites, L.behind, L.sky, L.bin_off, L.sbin_off, L.bins, L.sbins, L.order, L.total};
}
static FeLayout fe_at(size_t n, size_t W, const size_t c[6]) { return fe_layout(n, W, c[0], c[1], c[2], c[3], c[4], c[5]); }

static std::vector<size_t> offsets(const FsLayout &L) {
    return {L.frames, L.views, L.lights, L.mstate, L.lmask, L.mmask, L.lrows, L.mrows, L.fframes, L.parts, L.sprites, L.behind, L.sky, L.bin_off, L.sbin_off,
            L.bins, L.sbins, L.upload, L.total};
}

template <class V> static void check_monotone(const V &lo, const V &hi) {
    CHECK(lo.size() == hi.size());
    for (size_t i = 0; i < lo.size(); i++) CHECK(lo[i] <= hi[i]);
}

static void check_cursor() {
    std::snprintf(g_where, sizeof g_where, "cursor");
    SlabCursor c;
    CHECK(c.take(1) == 0 && c.end() == 1);
    CHECK(c.take(0) == 256 && c.end() == 256);                 // (a zero-size piece shares its offset with the next one)
    CHECK(c.take(256) == 256 && c.end() == 512);
    CHECK(c.take(257) == 512 && c.end() == 769);
    CHECK(c.take(5) == 1024 && c.end() == 1029);
}

static void check_list(size_t W, size_t F) {
    // dg_create: caps and capacity
    const size_t wall_cap = F * 4096, plane_cap = F * 4096, span_cap = F * W * 24;
    const size_t capacity = up(F * sizeof(DevFrame)) + up(F * (W + 1) * 4) + up(wall_cap * sizeof(DevWallRec)) + up(plane_cap * sizeof(DevPlaneRec)) +
                            span_cap * sizeof(DevSpan) + 1024;
    CHECK(list_layout(F, W, wall_cap, plane_cap, span_cap).total + 1024 == capacity);
    for (size_t n : {(size_t)1, (F + 1) / 2, F})
        for (size_t fill = 0; fill <= 4; fill++) {             // counts at 0, 1/4 .. 4/4 of the caps, one below and at the cap included
            const size_t walls = wall_cap * fill / 4, planes = plane_cap * fill / 4, spans = span_cap * fill / 4;
            const ListLayout L = list_layout(n, W, walls, planes, spans);
            check_pieces(list_pieces(L, n, W, walls, planes, spans), L.total);
            CHECK(L.total <= capacity - 1024);
            check_monotone(offsets(L), offsets(list_layout(n + 1, W, walls, planes, spans)));
            check_monotone(offsets(L), offsets(list_layout(n, W + 1, walls, planes, spans)));
            check_monotone(offsets(L), offsets(list_layout(n, W, walls + 1, planes, spans)));
            check_monotone(offsets(L), offsets(list_layout(n, W, walls, planes + 1, spans)));
            check_monotone(offsets(L), offsets(list_layout(n, W, walls, planes, spans + 1)));
        }
    // the single frame redo_frame_host packs
    const ListLayout R = list_layout(1, W, 37, 11, 4 * W);
    CHECK(R.frames == 0 && R.col_off == up(sizeof(DevFrame)) && R.walls == up(R.col_off + (W + 1) * 4));
    CHECK(R.total <= capacity);
}

static void check_fe(size_t W, size_t F) {
    const size_t caps[6] = {F * 2048, F * 256, F * 256 * 32, F * FE_MAX_SKY_SLOTS, F * 16384, F * 2048};    // dg_create (parts: the default records per frame)
    const size_t capacity = up(F * sizeof(DevFrame)) + up(F * sizeof(FeFrame)) + up(caps[0] * sizeof(FePart)) + up(caps[1] * sizeof(FeSprite)) + up(caps[2] * 4) +
                            up(caps[3] * 4) + 2 * up(F * ((W + FE_BIN_W - 1) / FE_BIN_W + 1) * 4) + up(caps[4] * 2) + up(caps[5] * 2) + F * ((W + 255) / 256) * 4 + 1024;
    CHECK(fe_at(F, W, caps).total + 1024 == capacity);
    for (size_t n : {(size_t)1, (F + 1) / 2, F})
        for (size_t fill = 0; fill <= 4; fill++) {
            size_t c[6];
            for (int k = 0; k < 6; k++) c[k] = caps[k] * fill / 4;
            const FeLayout L = fe_at(n, W, c);
            check_pieces(fe_pieces(L, n, W, c), L.total);
            CHECK(L.total <= capacity - 1024);
            check_monotone(offsets(L), offsets(fe_at(n + 1, W, c)));
            check_monotone(offsets(L), offsets(fe_at(n, W + 1, c)));
            for (int k = 0; k < 6; k++) {
                size_t m[6];
                for (int j = 0; j < 6; j++) m[j] = c[j] + (j == k ? 1 : 0);
                check_monotone(offsets(L), offsets(fe_at(n, W, m)));
            }
        }
}

static void check_fs(size_t W, size_t F, size_t n_sectors, size_t n_mobjs, bool pvs, bool lfx, bool mfx) {
    const uint32_t ss = fs_sprite_stride((uint32_t)n_mobjs), bs = fs_sbin_stride(ss, W);
    CHECK(ss % 32 == 0 && ss >= 32 && ss <= FS_SPRITE_CAP && (ss >= n_mobjs || ss == FS_SPRITE_CAP));
    CHECK(bs <= FS_SBIN_CAP && (bs == FS_SBIN_CAP || bs == ss * ((W + 63) / 64)));
    CHECK(fs_sprite_stride((uint32_t)n_mobjs + 1) >= ss && fs_sbin_stride(ss, W + 1) >= bs);
    for (size_t n : {(size_t)1, (F + 1) / 2, F}) {
        const FsLayout L = fs_layout(n, W, n_sectors, n_mobjs, pvs, lfx, mfx, ss, bs);
        const size_t sf = pvs ? n : 1, nb1 = (W + 63) / 64 + 1;
        check_pieces({{L.frames, n * sizeof(DevFrame)}, {L.views, n * sizeof(dg_view)}, {L.lights, sf * n_sectors * 2}, {L.mstate, sf * n_mobjs * 4},
                      {L.lmask, lfx && pvs ? n * ((n_sectors + 31) / 32) * 4 : 0}, {L.mmask, mfx && pvs ? n * ((n_mobjs + 31) / 32) * 4 : 0},
                      {L.lrows, lfx && !pvs ? n * n_sectors * 2 : 0}, {L.mrows, mfx && !pvs ? n * n_mobjs * 4 : 0}, {L.fframes, n * sizeof(FeFrame)},
                      {L.parts, n * FS_PART_CAP * sizeof(FePart)}, {L.sprites, n * ss * sizeof(FeSprite)}, {L.behind, n * ss * FS_BEHIND_WORDS * 4},
                      {L.sky, n * FS_SKY_CAP * 4}, {L.bin_off, n * nb1 * 4}, {L.sbin_off, n * nb1 * 4}, {L.bins, n * FS_BIN_CAP * 2}, {L.sbins, n * bs * 2}},
                     L.total);
        CHECK(L.upload <= L.total && L.upload % 256 == 0 && L.upload == L.lrows);       // the H2D part ends where the device-written part starts
        CHECK(L.mmask <= L.upload && L.upload <= L.fframes);
        if (!(lfx && pvs)) CHECK(L.lmask == L.mmask);                                   // zero-size pieces take no room
        if (!(mfx && pvs)) CHECK(L.mmask == L.lrows);
        if (!(lfx && !pvs)) CHECK(L.lrows == L.mrows);
        if (!(mfx && !pvs)) CHECK(L.mrows == L.fframes);
        check_monotone(offsets(L), offsets(fs_layout(n + 1, W, n_sectors, n_mobjs, pvs, lfx, mfx, ss, bs)));
        check_monotone(offsets(L), offsets(fs_layout(n, W + 1, n_sectors, n_mobjs, pvs, lfx, mfx, ss, bs)));
        check_monotone(offsets(L), offsets(fs_layout(n, W, n_sectors + 1, n_mobjs, pvs, lfx, mfx, ss, bs)));
        check_monotone(offsets(L), offsets(fs_layout(n, W, n_sectors, n_mobjs + 1, pvs, lfx, mfx, ss, bs)));
        check_monotone(offsets(L), offsets(fs_layout(n, W, n_sectors, n_mobjs, pvs, lfx, mfx, ss + 32, bs)));
        check_monotone(offsets(L), offsets(fs_layout(n, W, n_sectors, n_mobjs, pvs, lfx, mfx, ss, bs + 1)));
    }
}

static void check_scratch(size_t F, uint32_t n_segs, bool want_rows) {
    const FsScratchLayout L = fs_scratch_layout(F, n_segs);
    const uint32_t cap = fs_cl_row_cap(n_segs);
    CHECK(cap % 32 == 0 && cap >= n_segs * FS_CALLS && cap < n_segs * FS_CALLS + 32);
    CHECK((cap > FS_CL_CAP) == want_rows);
    CHECK(L.cl_row_cap == (want_rows ? cap : 0u));
    CHECK(L.zero_bytes == F * (size_t)fs_occ_words(n_segs) * 4);
    check_pieces({{L.occ, L.zero_bytes}, {L.lite, F * (size_t)n_segs * FS_CALLS * 8}, {L.cl_rows, want_rows ? F * (size_t)cap * 4 : 0},
                  {L.keep_rows, want_rows ? F * (size_t)(cap / 32) * 4 : 0}},
                 L.total);
    if (!want_rows) CHECK(L.cl_rows == L.keep_rows && L.keep_rows == L.total);
    const FsScratchLayout M = fs_scratch_layout(F + 1, n_segs), N = fs_scratch_layout(F, n_segs + 1);
    for (const FsScratchLayout *o : {&M, &N})
        CHECK(o->occ >= L.occ && o->lite >= L.lite && o->cl_rows >= L.cl_rows && o->keep_rows >= L.keep_rows && o->total >= L.total && o->zero_bytes >= L.zero_bytes);
}

int main() {
    long long configs = 0;
    check_cursor();
    const uint32_t segs_small = FS_CL_CAP / FS_CALLS / 2, segs_edge = FS_CL_CAP / FS_CALLS, segs_large = 4 * FS_CL_CAP;
    for (size_t W : {(size_t)320, (size_t)1280, (size_t)2560})
        for (size_t F : {(size_t)1, (size_t)64, (size_t)1000}) {
            std::snprintf(g_where, sizeof g_where, "W=%zu max_batch=%zu", W, F);
            check_list(W, F);
            check_fe(W, F);
            configs++;
            for (int bits = 0; bits < 8; bits++)
                for (size_t scene : {(size_t)0, (size_t)1, (size_t)2}) {
                    const size_t n_sectors = scene == 0 ? 1 : scene == 1 ? 187 : 4000, n_mobjs = scene == 0 ? 0 : scene == 1 ? 138 : 3000;
                    std::snprintf(g_where, sizeof g_where, "W=%zu max_batch=%zu per_view_state=%d lfx=%d mfx=%d sectors=%zu mobjs=%zu", W, F, bits & 1, (bits >> 1) & 1,
                                  (bits >> 2) & 1, n_sectors, n_mobjs);
                    check_fs(W, F, n_sectors, n_mobjs, bits & 1, (bits >> 1) & 1, (bits >> 2) & 1);
                    configs++;
                }
            const struct { uint32_t n_segs; bool rows; } scenes[] = {{1u, false}, {segs_small, false}, {segs_edge, false}, {segs_edge + 1u, true}, {segs_large, true}};
            for (const auto &sc : scenes) {             // candidate rows in global memory: only past FS_CL_CAP
                std::snprintf(g_where, sizeof g_where, "max_batch=%zu n_segs=%u", F, sc.n_segs);
                check_scratch(F, sc.n_segs, sc.rows);
                configs++;
            }
        }
    // both sides of FS_CL_CAP were met
    CHECK(fs_cl_row_cap(segs_small) < FS_CL_CAP && fs_cl_row_cap(segs_edge) <= FS_CL_CAP && fs_cl_row_cap(segs_edge + 1u) > FS_CL_CAP && fs_cl_row_cap(segs_large) > FS_CL_CAP);
    std::printf("ok %lld %lld\n", configs, g_checks);
    return 0;
}
