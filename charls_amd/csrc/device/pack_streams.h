// pack_streams.h -- the segmented unaligned copy of the packed-stream calls (pack_streams.hip; host/batch_packed.cpp).
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#include <hip/hip_runtime_api.h>
#endif

namespace jls {

// One copy: `bytes` from source base + src_offset to destination base + dst_offset, then `pad_bytes` zeros behind them.
// Neither offset has any alignment.  The destination extents of the jobs of a launch must not overlap.
struct PackJob
{
    uint64_t src_offset;
    uint64_t dst_offset;
    uint64_t bytes;
    uint32_t pad_bytes;
    uint32_t reserved;
};

#ifdef __HIPCC__
namespace dev {
// `longest_bytes`: the largest bytes + pad_bytes of the jobs (HOST value: it shapes the grid).  d_jobs is a DEVICE pointer.
void launch_pack_streams(const uint8_t* d_src, uint8_t* d_dst, const PackJob* d_jobs, uint32_t count, uint64_t longest_bytes,
                         hipStream_t stream);
} // namespace dev
#endif

} // namespace jls
