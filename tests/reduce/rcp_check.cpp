// rcp_check — the rounded divide of csrc/reduce_core.h against hardware division, exhaustively: for every box size n in 1..256 and
// every x in [0, 2*255*n + n] the high word of x * reduce_rcp(n) is x / 2n, and reduce_round(s, n, ..) is (2 s + n) / 2n for every
// sum s of n bytes.  Prints "ok <cases>" or the first mismatch.
#include <cstdint>
#include <cstdio>

#include "../../doom-rust-renderer_amd/csrc/reduce_core.h"

int main() {
    uint64_t cases = 0;
    for (uint32_t n = 1; n <= 256; n++) {
        const uint32_t rcp = dg::reduce_rcp(n);
        if ((uint64_t)rcp * 2u * n < (1ull << 32) || (uint64_t)(rcp - 1u) * 2u * n >= (1ull << 32)) { std::printf("rcp(%u) = %u is not ceil(2^32 / 2n)\n", n, rcp); return 1; }
        const uint32_t top = 2u * 255u * n + n;
        for (uint32_t x = 0; x <= top; x++, cases++) {
            const uint32_t hi = (uint32_t)(((uint64_t)x * rcp) >> 32);
            if (hi != x / (2u * n)) { std::printf("n %u x %u: %u != %u\n", n, x, hi, x / (2u * n)); return 1; }
        }
        for (uint32_t s = 0; s <= 255u * n; s++)
            if (dg::reduce_round(s, n, rcp) != (2u * s + n) / (2u * n)) { std::printf("n %u s %u\n", n, s); return 1; }
        if (dg::reduce_round(255u * n, n, rcp) != 255u || dg::reduce_round(0u, n, rcp) != 0u) { std::printf("n %u: ends\n", n); return 1; }
    }
    std::printf("ok %llu\n", (unsigned long long)cases);
    return 0;
}
