// tests/fe_auto/fe_auto_main.cpp — DG_FE_AUTO's policy (csrc/fe_auto.hpp) on the CPU: the decision per batch, the probe cadences of 32
// and 256 batches, and the running means with their dropped first samples.  Stand-alone (tests/test_fe_auto_host.py builds it with the
// address and undefined-behaviour sanitizers); prints "ok <checks>" or the first failure.
#include "../../doom-rust-renderer_amd/csrc/fe_auto.hpp"

#include <cstdio>

using dg::FeAuto;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                                              \
    do {                                                                                         \
        g_checks++;                                                                              \
        if (!(cond) && !g_failed++) std::printf("FAILED line %d: %s\n", __LINE__, #cond);        \
    } while (0)

// `cycles` times: `run` batches decided as `first`, then one decided the other way
static void expect_cadence(FeAuto &a, bool first, int run, int cycles) {
    for (int c = 0; c < cycles; c++) {
        for (int i = 0; i < run; i++) CHECK(a.seg_walk_next(true) == first);
        CHECK(a.seg_walk_next(true) == !first);
    }
}

int main() {
    {   // nothing in flight: the GPU takes it every time and neither counter moves, whatever has been measured
        FeAuto a;
        for (int i = 0; i < 300; i++) CHECK(a.seg_walk_next(false));
        a.ema_host = 0.3; a.ema_gpu_fs = 0.4;                     // (in a filled pipeline the host would keep it)
        a.since_probe = 5; a.since_fs_probe = 7;
        for (int i = 0; i < 300; i++) CHECK(a.seg_walk_next(false));
        CHECK(a.since_probe == 5 && a.since_fs_probe == 7);
    }
    {   // in flight, host mean 1.0, no seg-walk mean yet: 31 seg-walk batches, then one host batch, repeating
        FeAuto a;
        a.ema_host = 1.0;
        expect_cadence(a, true, 31, 3);
    }
    {   // host mean 1.0 far behind a seg-walk mean of 0.4: 255 seg-walk batches, then one host batch
        FeAuto a;
        a.ema_host = 1.0; a.ema_gpu_fs = 0.4;
        expect_cadence(a, true, 255, 2);
        a.ema_host = 0.8;                                         // exactly twice is not "far behind": every 32 again
        expect_cadence(a, true, 31, 2);
    }
    {   // host mean 0.3 ahead of a seg-walk mean of 0.4: 31 host batches, then one seg-walk batch, repeating
        FeAuto a;
        a.ema_host = 0.3; a.ema_gpu_fs = 0.4;
        expect_cadence(a, false, 31, 3);
        a.ema_host = 0.4;                                         // a tie stays with the host
        expect_cadence(a, false, 31, 1);
    }
    {   // host samples without calibration: v1 is ignored, v2 becomes the mean, v3 blends
        FeAuto a;
        a.host_batch(640.0, 64);                                  // v1 = 10
        CHECK(a.ema_host == -1.0 && a.host_samples == 1);
        a.host_batch(128.0, 64);                                  // v2 = 2
        CHECK(a.ema_host == 2.0 && a.host_samples == 2);
        a.host_batch(600.0, 100);                                 // v3 = 6
        CHECK(a.ema_host == 0.75 * 2.0 + 0.25 * 6.0 && a.host_samples == 3);
    }
    {   // after a calibration the first whole batch already blends
        FeAuto a;
        a.calibrated(16.0, 8, 4);                                 // 16 ms / 8 views / 4 threads x 1.25
        CHECK(a.ema_host == 0.625 && a.host_samples == 2);
        a.host_batch(128.0, 64);
        CHECK(a.ema_host == 0.75 * 0.625 + 0.25 * 2.0 && a.host_samples == 3);
        a.calibrated(8.0, 8, 0);                                  // (a pool of no threads counts as one; the sample count never goes back)
        CHECK(a.ema_host == 1.25 && a.host_samples == 3);
        FeAuto b;
        b.host_batch(640.0, 64);                                  // one dropped batch, then a calibration: the next batch blends as well
        b.calibrated(16.0, 8, 4);
        CHECK(b.host_samples == 2);
        b.host_batch(128.0, 64);
        CHECK(b.ema_host == 0.75 * 0.625 + 0.25 * 2.0);
    }
    {   // GPU samples: the first of each mode is ignored, the modes are counted separately, then the mean is set, then blended
        FeAuto a;
        a.gpu_batch(true, 640.0, 64);
        CHECK(a.ema_gpu_fs == -1.0 && a.ema_gpu_dev == -1.0 && a.gpu_samples[1] == 1 && a.gpu_samples[0] == 0);
        a.gpu_batch(true, 128.0, 64);
        CHECK(a.ema_gpu_fs == 2.0 && a.ema_gpu_dev == -1.0);
        a.gpu_batch(false, 640.0, 64);                            // the other mode's first: dropped although the seg walk has a mean
        CHECK(a.ema_gpu_dev == -1.0 && a.gpu_samples[0] == 1);
        a.gpu_batch(false, 256.0, 64);
        CHECK(a.ema_gpu_dev == 4.0 && a.ema_gpu_fs == 2.0);
        a.gpu_batch(true, 600.0, 100);
        a.gpu_batch(false, 800.0, 100);
        CHECK(a.ema_gpu_fs == 0.75 * 2.0 + 0.25 * 6.0 && a.ema_gpu_dev == 0.75 * 4.0 + 0.25 * 8.0);
        CHECK(a.gpu_samples[0] == 3 && a.gpu_samples[1] == 3 && a.ema_host == -1.0);
    }
    if (g_failed) return 1;
    std::printf("ok %d\n", g_checks);
    return 0;
}
