// restart_intervals_encode.hip -- the encode half of restart_intervals.h (an extension: the reference's encoder cannot emit
// restart markers): intervals coded into private buffers are joined with FF D0+m between them.
#pragma once
#include <hip/hip_runtime.h>

#include "restart_intervals.h"
#include "scan_model.h"

namespace jls {
namespace interval {

// grid (intervals, scans), one thread.  `buffers` holds scans * intervals private streams of `capacity` bytes;
// `scratch` (may be null) scans * intervals line windows of `scratch_samples` samples for the global-memory kernels.
__global__ void build_encode_intervals(const ScanDesc* __restrict__ parents, uint32_t intervals, uint8_t* __restrict__ buffers,
                                       uint64_t capacity, uint16_t* __restrict__ scratch, uint64_t scratch_samples,
                                       ScanDesc* __restrict__ subs)
{
    const uint32_t j = blockIdx.x, s = blockIdx.y;
    ScanDesc d = parents[s];
    const uint32_t lines = d.restart_interval;
    const size_t at = (size_t)s * intervals + j;
    d.pixels += (uint64_t)j * lines * d.pixel_stride;
    // rows of this interval.  A parent with height 0 is a frame that failed earlier (container_kernels.hip:
    // place_scan_header empties its descriptor): all its intervals are empty scans with no room, which fail fast without
    // touching pixels or work areas -- the geometry of the launch (`intervals`) comes from the other frames.
    const uint64_t before = (uint64_t)j * lines;
    const bool dead = d.height == 0 || d.stream_capacity == 0;
    d.height = !dead && d.height > before ? (uint32_t)(d.height - before < lines ? d.height - before : lines) : 0u;
    d.stream = buffers + at * capacity;
    d.stream_capacity = dead ? 0 : capacity;
    d.restart_interval = 0;
    if (scratch != nullptr)
        d.line_scratch = scratch + at * scratch_samples;
    subs[at] = d;
}

// One thread per scan: where every interval goes in the scan's own stream; the scan's result.
// flags bit kIntervalRetry: an interval did not fit ITS private buffer (the caller repeats with worst-case buffers).
__global__ void plan_join(const ScanDesc* __restrict__ parents, uint32_t intervals, const ScanResult* __restrict__ sub_results,
                          uint64_t* __restrict__ offsets, ScanResult* __restrict__ results, uint32_t scans)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= scans)
        return;
    const ScanDesc d = parents[s];
    const ScanResult* sr = sub_results + (size_t)s * intervals;
    uint64_t* off = offsets + (size_t)s * intervals;
    if (d.height == 0 || d.stream_capacity == 0)
    { // a frame that failed before this scan: nothing to join, and no reason to repeat its group with larger buffers
        for (uint32_t j = 0; j < intervals; ++j)
            off[j] = 0;
        results[s] = ScanResult{kDestinationTooSmall, 0, 0};
        return;
    }
    ScanResult r{kOk, 0, 0};
    uint64_t at = 0;
    for (uint32_t j = 0; j < intervals; ++j)
    {
        if (sr[j].errc == kDestinationTooSmall)
            r.flags |= kIntervalRetry;
        else if (sr[j].errc != kOk && r.errc == kOk)
            r.errc = sr[j].errc;
        off[j] = at;
        at += sr[j].bytes + (j + 1 < intervals ? 2 : 0);
    }
    if (r.errc == kOk && r.flags == 0 && at > d.stream_capacity)
        r.errc = kDestinationTooSmall;
    r.bytes = r.errc == kOk && r.flags == 0 ? at : 0;
    results[s] = r;
}

// grid (intervals, scans) x 256 threads: copy + marker.
__global__ void __launch_bounds__(256) join_intervals(const ScanDesc* __restrict__ parents, const ScanDesc* __restrict__ subs,
                                                      uint32_t intervals, const ScanResult* __restrict__ sub_results,
                                                      const uint64_t* __restrict__ offsets, const ScanResult* __restrict__ results)
{
    const uint32_t j = blockIdx.x, s = blockIdx.y;
    const ScanResult r = results[s];
    if (r.errc != kOk || r.flags != 0)
        return;
    const size_t at = (size_t)s * intervals + j;
    const uint8_t* src = subs[at].stream;
    uint8_t* dst = parents[s].stream + offsets[at];
    const uint64_t n = sub_results[at].bytes;
    for (uint64_t i = threadIdx.x; i < n; i += 256)
        dst[i] = src[i];
    if (threadIdx.x == 0 && j + 1 < intervals)
    {
        dst[n] = 0xFF;
        dst[n + 1] = (uint8_t)(0xD0u + (j & 7u));
    }
}

} // namespace interval
} // namespace jls
