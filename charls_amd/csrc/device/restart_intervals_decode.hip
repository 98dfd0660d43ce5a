// restart_intervals_decode.hip -- the decode half of restart_intervals.h: marker search, one descriptor per interval, the check
// of the intervals' results.
#pragma once
#include <hip/hip_runtime.h>

#include "restart_intervals.h"
#include "scan_model.h"

namespace jls {
namespace interval {

// The walk reads kWalkChunks chunks of 1 KB per trip -- lane l holds bytes [16 l, 16 l + 16) of each -- and has the next trip's
// loads in flight while it looks at this trip's bytes.
constexpr int kWalkChunks = 4;
constexpr uint64_t kWalkBatch = 1024u * kWalkChunks;

// 0x80 in every byte of w that is 0xFF and is followed by a byte >= 0x80 (the next byte of w; the low byte of `after` behind
// the last): the bytes that can only be the first of a marker.
JLS_DEV uint32_t marker_bytes(uint32_t w, uint32_t after)
{
    const uint32_t v = ~w;
    const uint32_t is_ff = ~(((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v | 0x7F7F7F7Fu);
    return is_ff & ((w >> 8) | (after << 24));
}

// One trip's bytes: the 16 of this lane in every chunk (zeros from the first granule on that holds no source byte) and the
// byte behind the trip (0: none).  The loads are unconditional, so that they issue back to back and the waits count down: a
// lane beyond the source loads the granule of the last source byte again (`last`) and drops it.  u_end > u_begin.
typedef uint32_t WalkWords4 __attribute__((vector_size(16))); // (a granule as one load, through a pointer into global memory)
struct WalkBatch
{
    uint4 raw[kWalkChunks];
    uint32_t behind;
};
JLS_DEV void load_walk_batch(WalkBatch& b, const JLS_GLOBAL_AS uint8_t* gbase, uint64_t u0, uint64_t u_end, int lane)
{
    const uint64_t last = (u_end - 1) & ~(uint64_t)15;
#pragma unroll
    for (int c = 0; c < kWalkChunks; ++c)
    {
        const uint64_t mine = u0 + (uint64_t)c * 1024 + (uint64_t)lane * 16;
        const WalkWords4 v = *reinterpret_cast<const JLS_GLOBAL_AS WalkWords4*>(gbase + (mine < u_end ? mine : last));
        const uint32_t keep = 0u - (uint32_t)(mine < u_end); // (a mask, not a choice: a load that is chosen is moved behind a branch)
        b.raw[c] = make_uint4(v[0] & keep, v[1] & keep, v[2] & keep, v[3] & keep);
    }
    const uint64_t behind = u0 + kWalkBatch;
    const uint32_t byte = gbase[behind < u_end ? behind : u_end - 1];
    b.behind = byte & (0u - (uint32_t)(behind < u_end));
}

// The markers of one chunk, listed in order behind the `found` there are: this lane's 16 bytes at `mine`, `next_first` the
// byte behind them.  True when the chunk holds a marker that is no RSTm: the entropy-coded segment ends there.
JLS_DEV bool list_chunk_markers(const uint4 raw, uint32_t next_first, uint64_t mine, uint64_t u_begin, uint64_t u_end, int lane,
                                JLS_GLOBAL_AS uint32_t* out, uint32_t max_marks, uint32_t& found, bool& overflow)
{
    const uint32_t words[4] = {raw.x, raw.y, raw.z, raw.w};
    uint32_t rst_mask = 0, other_mask = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j)
    {
        const uint32_t b = (words[j >> 2] >> ((j & 3) * 8)) & 0xFFu;
        const uint32_t nb = j < 15 ? ((words[(j + 1) >> 2] >> (((j + 1) & 3) * 8)) & 0xFFu) : next_first;
        const uint64_t u = mine + (uint64_t)j;
        const bool inside = u >= u_begin && u + 1 < u_end;
        const bool is_marker = inside && b == 0xFFu && nb >= 0x80u;
        const bool is_rst = is_marker && (nb & 0xF8u) == 0xD0u;
        rst_mask |= (uint32_t)is_rst << j;
        other_mask |= (uint32_t)(is_marker && !is_rst) << j;
    }
    // the first non-RST marker ends the entropy-coded segment
    const unsigned long long lanes_other = __ballot(other_mask != 0);
    int stop_lane = 64, stop_bit = 16;
    if (lanes_other)
    {
        stop_lane = __ffsll(lanes_other) - 1;
        stop_bit = __ffs((int)__shfl((int)other_mask, stop_lane)) - 1;
    }
    if (lane > stop_lane)
        rst_mask = 0;
    else if (lane == stop_lane)
        rst_mask &= (1u << stop_bit) - 1u;
    // ordered append
    const int mine_count = __popc(rst_mask);
    int inc = mine_count;
    for (int delta = 1; delta < 64; delta <<= 1)
    {
        const int up = __shfl_up(inc, delta);
        if (lane >= delta)
            inc += up;
    }
    uint32_t at = found + (uint32_t)(inc - mine_count);
    uint32_t m = rst_mask;
    while (m)
    {
        const int j = __ffs((int)m) - 1;
        m &= m - 1;
        if (at < max_marks)
            out[at] = (uint32_t)(mine + (uint64_t)j - u_begin);
        ++at;
    }
    found += (uint32_t)__shfl(inc, 63);
    if (found > max_marks)
        overflow = true;
    return lanes_other != 0;
}

// One wavefront per scan.  marks[scan * max_marks + j] = offset (from desc.stream) of the 0xFF of the j-th RSTm marker;
// counts[scan] = number of RSTm markers before the first other marker (kTooManyMarkers when more than max_marks).
//
// A trip is 4 KB.  Its loads were issued a trip ahead, back to back.  The byte behind a lane's 16 comes from the next lane's
// first byte by a shuffle -- for lane 63 from lane 0 of the next chunk, behind the last chunk from the trip's one byte load --,
// and a trip without a byte that can start a marker (all but a few: inside the entropy-coded bytes no 0xFF is followed by a
// byte >= 0x80) costs one test per word and one ballot.  A trip with such a byte lists its chunks one after the other, so the
// marks stay in order and the walk stops at the first marker that is no RSTm whatever arrived with it.
__global__ void __launch_bounds__(64) find_restart_markers(const ScanDesc* __restrict__ descs, uint32_t* __restrict__ marks,
                                                           uint32_t max_marks, uint32_t* __restrict__ counts)
{
    const ScanDesc d = descs[blockIdx.x];
    const int lane = threadIdx.x;
    const uint64_t mis = (uint64_t)(reinterpret_cast<uintptr_t>(d.stream) & 15u);
    const JLS_GLOBAL_AS uint8_t* gbase = global_ptr(d.stream) - mis; // 16-byte aligned
    const uint64_t u_begin = mis, u_end = mis + d.stream_capacity;
    JLS_GLOBAL_AS uint32_t* out = global_ptr(marks) + (size_t)blockIdx.x * max_marks;
    uint32_t found = 0;
    bool overflow = false;
    WalkBatch cur{};
    if (u_end > u_begin) // (a scan without a byte has no marker, and nothing to read)
        load_walk_batch(cur, gbase, 0, u_end, lane);
    for (uint64_t u0 = 0; u0 < u_end && u_end > u_begin; u0 += kWalkBatch)
    {
        WalkBatch next;
        load_walk_batch(next, gbase, u0 + kWalkBatch, u_end, lane); // (nothing beyond the granule of the last source byte is read)
        uint32_t next_first[kWalkChunks];
        uint32_t suspects = 0;
#pragma unroll
        for (int c = 0; c < kWalkChunks; ++c)
        {
            const int after = c + 1 < kWalkChunks ? c + 1 : c; // (the chunk whose lane 0 holds the byte behind this chunk)
            const uint32_t behind_chunk = c + 1 < kWalkChunks ? (uint32_t)__shfl((int)(cur.raw[after].x & 0xFFu), 0) : cur.behind;
            const uint32_t neighbour = (uint32_t)__shfl_down((int)(cur.raw[c].x & 0xFFu), 1);
            next_first[c] = lane == 63 ? behind_chunk : neighbour;
            suspects |= marker_bytes(cur.raw[c].x, cur.raw[c].y) | marker_bytes(cur.raw[c].y, cur.raw[c].z) |
                        marker_bytes(cur.raw[c].z, cur.raw[c].w) | marker_bytes(cur.raw[c].w, next_first[c]);
        }
        bool ended = false;
        if (__ballot(suspects != 0))
        { // (bytes outside [u_begin, u_end) of the first and the last granule may be among the suspects: `inside` decides)
#pragma unroll
            for (int c = 0; c < kWalkChunks; ++c)
                if (!ended)
                    ended = list_chunk_markers(cur.raw[c], next_first[c], u0 + (uint64_t)c * 1024 + (uint64_t)lane * 16, u_begin, u_end, lane, out,
                                               max_marks, found, overflow);
        }
        if (ended)
            break;
        cur = next;
    }
    if (lane == 0)
        global_ptr(counts)[blockIdx.x] = overflow ? kTooManyMarkers : found;
}

// grid (intervals, scans), one thread: the interval as a scan of its own.
__global__ void build_decode_intervals(const ScanDesc* __restrict__ parents, const uint32_t* __restrict__ marks,
                                       uint32_t intervals, ScanDesc* __restrict__ subs)
{
    const uint32_t j = blockIdx.x, s = blockIdx.y;
    ScanDesc d = parents[s];
    const uint32_t* mk = marks + (size_t)s * (intervals - 1);
    const uint32_t lines = d.restart_interval;
    const uint64_t start = j == 0 ? 0 : (uint64_t)mk[j - 1] + 2;
    const uint64_t end = j + 1 < intervals ? (uint64_t)mk[j] + 2 : d.stream_capacity; // its own RSTm terminates an interval
    d.pixels += (uint64_t)j * lines * d.pixel_stride;
    // rows of this interval; a parent without rows (a frame that already failed) has only empty intervals
    const uint64_t before = (uint64_t)j * lines;
    d.height = d.height > before ? (uint32_t)(d.height - before < lines ? d.height - before : lines) : 0u;
    d.stream += start;
    d.stream_capacity = end > start ? end - start : 0;
    d.restart_interval = 0;
    subs[(size_t)s * intervals + j] = d;
}

// One thread per scan.
__global__ void check_intervals(const ScanDesc* __restrict__ parents, const uint32_t* __restrict__ marks, uint32_t intervals,
                                const ScanResult* __restrict__ sub_results, ScanResult* __restrict__ results, uint32_t scans)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= scans)
        return;
    const ScanDesc d = parents[s];
    const uint32_t* mk = marks + (size_t)s * (intervals - 1);
    const ScanResult* sr = sub_results + (size_t)s * intervals;
    bool ok = true;
    uint64_t start = 0;
    for (uint32_t j = 0; j < intervals; ++j)
    {
        ok = ok && sr[j].errc == kOk && (sr[j].flags & kUndecided) == 0;
        if (j + 1 < intervals)
        { // consumed exactly up to its marker, and the marker is the expected one
            ok = ok && sr[j].bytes == (uint64_t)mk[j] - start && d.stream[(uint64_t)mk[j] + 1] == 0xD0u + (j & 7u);
            start = (uint64_t)mk[j] + 2;
        }
    }
    ScanResult r{kOk, 0, 0};
    if (ok)
        r.bytes = start + sr[intervals - 1].bytes;
    else
        r.flags = kIntervalRetry;
    results[s] = r;
}

} // namespace interval
} // namespace jls
