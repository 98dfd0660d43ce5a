// window_fetch.h -- the gather kernel of the batch decoders' window fetch (batch_api.cpp, batch_index.cpp): every frame's
// marker segments are parsed on the host from small windows of the device-resident streams.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace jls {

// One window of every listed stream -> a contiguous staging buffer (then ONE device-to-host copy instead of one small,
// synchronously staged copy per frame: 4096 of those were 60 ms per round of the batch decoder).
struct WindowSpec
{
    uint64_t offset; // from the first slot
    uint32_t bytes;
    uint32_t pad;
};
static __global__ void gather_windows(const uint8_t* __restrict__ slots, const WindowSpec* __restrict__ specs, uint8_t* __restrict__ out,
                               uint32_t window)
{
    const WindowSpec w = specs[blockIdx.x];
    const uint8_t* src = slots + w.offset;
    uint8_t* dst = out + (size_t)blockIdx.x * window;
    for (uint32_t b = threadIdx.x; b < w.bytes; b += blockDim.x)
        dst[b] = src[b];
}

} // namespace jls
