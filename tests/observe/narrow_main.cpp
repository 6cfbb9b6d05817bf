// tests/observe/narrow_main.cpp IN OUT — the two narrowings of observe_core.h over a file of float32 bit patterns, for
// tests/test_observe_host.py: IN holds n uint32; OUT receives n uint16 of obs_f16_bits, then n uint16 of obs_bf16_bits.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../doom-rust-renderer_amd/csrc/observe_core.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    std::FILE *in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<uint32_t> u;
    uint32_t buf[4096];
    for (size_t k; (k = std::fread(buf, sizeof(uint32_t), 4096, in)) > 0;) u.insert(u.end(), buf, buf + k);
    std::fclose(in);
    std::vector<uint16_t> out(2 * u.size());
    for (size_t i = 0; i < u.size(); i++) {
        float f;
        std::memcpy(&f, &u[i], sizeof f);
        out[i] = dg::obs_f16_bits(f);
        out[u.size() + i] = dg::obs_bf16_bits(f);
    }
    std::FILE *o = std::fopen(argv[2], "wb");
    if (!o || std::fwrite(out.data(), sizeof(uint16_t), out.size(), o) != out.size()) return 2;
    std::fclose(o);
    std::printf("narrow_main: ok (%zu patterns)\n", u.size());
    return 0;
}
