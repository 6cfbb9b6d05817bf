// plan_check — the constants behind the band kernels' runs, printed from the project's own headers, for tests/test_extents_host.py to hold
// against the Python restatement (tests/extent_cases.py): one line "spans <REDUCE_SPAN> <PLANE_REDUCE_SPAN> <REDUCE_LANES>
// <PLANE_REDUCE_LANES> <REDUCE_MAX_FACTOR>", then per fx in 1..16 "<fx> <reduce_px_per_wg(fx)> <plane_reduce_px_per_wg(fx)>".
#include <cstdint>
#include <cstdio>

#include "../../doom-rust-renderer_amd/csrc/plane_reduce_kernels.hpp"
#include "../../doom-rust-renderer_amd/csrc/reduce_kernels.hpp"

int main() {
    std::printf("spans %u %u %u %u %u\n", dg::REDUCE_SPAN, dg::PLANE_REDUCE_SPAN, dg::REDUCE_LANES, dg::PLANE_REDUCE_LANES, (unsigned)dg::REDUCE_MAX_FACTOR);
    for (uint32_t fx = 1; fx <= 16; fx++) std::printf("%u %u %u\n", fx, dg::reduce_px_per_wg(fx), dg::plane_reduce_px_per_wg(fx));
    return 0;
}
