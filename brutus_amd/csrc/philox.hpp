// philox.hpp -- the counter-based generator of brutus_amd/rng.py on the device: Philox4x32-7,
// key = the 64-bit seed, counter = (index lo, index hi, c2, stream), and numpy's 53-bit uniform.
// Any deviate is a pure function of (seed, index).  Included by post_kernels.hpp (the lnpost
// streams) and los_walk_kernels.hpp (the walk stream); each includes it before its own code.
#pragma once

#include <stdint.h>

namespace {

struct Philox4 {
    uint32_t w[4];
};

__device__ __forceinline__ Philox4 philox4x32_7(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 7; ++r) {
        if (r > 0) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;   // v_mad_u64_u32
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0;
        c1 = lo1;
        c2 = n2;
        c3 = lo0;
    }
    Philox4 o;
    o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
    return o;
}

__device__ __forceinline__ double u53(uint32_t a, uint32_t b) {
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) / 9007199254740992.0;
}

// the streams of rng.py (counter word 3)
constexpr uint32_t STREAM_NORMAL = 0u, STREAM_UNIFORM = 1u, STREAM_RETRY = 2u, STREAM_TAIL = 3u, STREAM_WALK = 4u;

__device__ __forceinline__ Philox4 philox_at(uint64_t seed, uint64_t idx, uint32_t c2, uint32_t stream) {
    return philox4x32_7((uint32_t)idx, (uint32_t)(idx >> 32), c2, stream, (uint32_t)seed,
                        (uint32_t)(seed >> 32));
}

}  // namespace
