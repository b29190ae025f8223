// align16.cuh - 16 bytes that start at any byte phase, out of two ALIGNED 16-byte words (gfx950).  Shared by the loaders that
// read a byte stream whose start the format decides (raw_unpack_kernel, the stored blocks of lz4_decode_kernel).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fa {

// x = the aligned 16 bytes the run starts in, y = the 16 behind them (any value when sh == 0), sh = the run's phase 0 .. 15:
// -> bytes sh .. sh + 15 of x|y.  sh is meant to be wave-uniform: the dword index is static in every arm, one arm is taken.
__device__ __forceinline__ uint4 bytes16_at_phase(const uint4 x, const uint4 y, uint32_t sh) {
    const uint32_t dw[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
    uint4 o = x;
#pragma unroll
    for (uint32_t q = 0; q < 4; q++)
        if (q == (sh >> 2)) {
            o.x = __builtin_amdgcn_alignbyte(dw[q + 1], dw[q], sh & 3), o.y = __builtin_amdgcn_alignbyte(dw[q + 2], dw[q + 1], sh & 3);
            o.z = __builtin_amdgcn_alignbyte(dw[q + 3], dw[q + 2], sh & 3), o.w = __builtin_amdgcn_alignbyte(dw[q + 4], dw[q + 3], sh & 3);
        }
    return o;
}

}  // namespace fa
