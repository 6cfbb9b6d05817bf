// fe_auto.hpp — DG_FE_AUTO's policy: what it has measured (running means over batches of >= 64 frames, ms per frame; < 0: not yet) and
// how it decides, per batch, who does the per-seg half.  Plain arithmetic, no HIP and no dg_ctx: context.cpp measures and asks,
// tests/fe_auto checks the rule on the CPU.  The host does the per-seg half for free as long as it is done before the GPU has finished
// the batches queued ahead (its time hides under theirs); the GPU pays for it (dg_fs_*: ~0.1 ms per 1 000 frames) but needs no host time.
// So: when nothing is in flight the host's time would be exposed in full — the GPU does it; in a filled pipeline the GPU does it when the
// host has been measured to be the slower of the two (few host threads, small frames), and until a seg-walk batch has been timed at all
// (a batch on a host that turns out to be the slower side costs the pipeline a millisecond).  The other side is timed again now and then:
// the host's speed depends on who else uses the CPUs, the first seg-walk samples may have been taken on a cold GPU; the host rarely when
// it was far behind.  The first sample of each kind is dropped: cold caches, arena growth, code not yet resident, clocks down — a seg
// walk judged by it alone was never tried again.
#pragma once
#include <algorithm>

namespace dg {

struct FeAuto {
    double ema_host = -1.0, ema_gpu_dev = -1.0, ema_gpu_fs = -1.0;   // the host's per-seg half; a batch's GPU work without / with the seg walk in it
    int host_samples = 0;               // batches the host walker was timed on
    int since_probe = 0;                // seg-walk batches since the host walker was last timed (again every 32 batches, or 256)
    int since_fs_probe = 0;             // host-walker batches since the seg walk was last timed (every 32)
    int gpu_samples[2] = {0, 0};        // finished batches seen per mode (host per-seg half / seg walk)

    // First guess of the host walker's speed: `timed` views took `ms` on one thread of a pool of `threads` (which does not scale perfectly).
    void calibrated(double ms, int timed, int threads) {
        ema_host = ms / timed / std::max(1, threads) * 1.25;
        host_samples = std::max(host_samples, 2);
    }
    // A whole batch of n frames went through the host walker in host_ms.
    void host_batch(double host_ms, int n) {
        if (host_samples++ == 0) return;
        ema_host = host_samples == 2 ? host_ms / n : 0.75 * ema_host + 0.25 * (host_ms / n);
    }
    // A column-walk batch of n frames has finished on the GPU: its kernels took ms.
    void gpu_batch(bool seg_walk, double ms, int n) {
        if (gpu_samples[seg_walk ? 1 : 0]++ == 0) return;
        double &ema = seg_walk ? ema_gpu_fs : ema_gpu_dev;
        ema = ema < 0.0 ? ms / n : 0.75 * ema + 0.25 * (ms / n);
    }
    // Should the next batch's per-seg half run on the GPU (the seg walk)?
    bool seg_walk_next(bool in_flight) {
        if (!in_flight) return true;
        bool fs = ema_gpu_fs < 0.0 ? true : ema_host > ema_gpu_fs;
        if (fs && ++since_probe >= (ema_gpu_fs > 0.0 && ema_host > 2.0 * ema_gpu_fs ? 256 : 32)) fs = false;
        else if (!fs && ++since_fs_probe >= 32) fs = true;
        if (!fs) since_probe = 0; else since_fs_probe = 0;
        return fs;
    }
};

}  // namespace dg
