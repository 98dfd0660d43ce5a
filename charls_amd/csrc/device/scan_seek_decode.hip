// scan_seek_decode.hip -- the exact decoder (decode_scans_wave) that saves its state every K lines, and the one that
// starts from such a state.
//
//  * decode_scans_wave_emit decodes a scan exactly as decode_scans_wave does and, at every line boundary y = i * K
//    (0 < y < height), writes seek point i (layout: seek_decode.h).
//  * decode_scans_wave_resume decodes rows [first_row, end_row) of a scan from the initial state (first_row = 0) or from a
//    seek point, stores the rows asked for, and then compares its end state with the next seek point, ends the scan
//    (end_scan, bytes consumed), or just stops (a band of rows).  In prefix mode (salvage through the index, charls_amd.h
//    part 2h) it ends the scan as well, and where it stops on an error it reports the rows it completed instead.
// Both run the line loop of scan_wave_decode.hip unchanged; what is new is the state going out to and coming in from
// global memory.  Positions are stored relative to the scan's first entropy-coded byte: the device copy of a stream has a
// different 16-byte misalignment from one call to the next, and the LDS ring is only a cache of the bytes.
// Scans with restart intervals are not taken (the host checks: seek_decode_eligible).
#pragma once
#include <hip/hip_runtime.h>

#include "scan_wave_decode.hip"
#include "seek_decode.h"

namespace jls {
namespace seek {

// The wavefront's state at a line boundary -> point p (all lanes).  The LDS it reads is settled: decode_line ends with a
// barrier.
template <typename S>
JLS_DEV void save_point(uint8_t* p, const uint8_t* smem, const S* line, uint32_t line_samples, const int* run_index,
                        const int* corner, const wave::RingReader& br, size_t reader_at, int lane)
{
    const uint32_t* ctx = reinterpret_cast<const uint32_t*>(smem);
    uint32_t* q = reinterpret_cast<uint32_t*>(p);
    for (uint32_t i = lane; i < kRunOff / 4; i += wave::kLanes)
        q[i] = ctx[i];
    const uint32_t* run = reinterpret_cast<const uint32_t*>(smem + wave::kCtxBytes);
    if (lane < 8)
        q[kRunOff / 4 + lane] = run[lane];
    S* ql = reinterpret_cast<S*>(p + kLineOff);
    for (uint32_t i = lane; i < line_samples; i += wave::kLanes)
        ql[i] = line[i];
    if (lane == 0)
    {
        int32_t* ri = reinterpret_cast<int32_t*>(p + kRunIndexOff);
        int32_t* co = reinterpret_cast<int32_t*>(p + kCornerOff);
        for (int j = 0; j < 4; ++j)
        {
            ri[j] = run_index[j];
            co[j] = corner[j];
        }
        uint32_t* rc = reinterpret_cast<uint32_t*>(p + kRestartOff);
        rc[0] = br.restart_counter;
        rc[1] = 0;
        uint64_t* rd = reinterpret_cast<uint64_t*>(p + reader_at);
        rd[0] = br.u_pos - br.u_begin;
        rd[1] = br.cache;
        rd[2] = (uint64_t)(uint32_t)br.valid;
    }
}

// Point p -> the wavefront's state (all lanes; a barrier follows in the caller).  The reader's ring is primed from 16
// bytes before the position, aligned down to 16 (the refill loads whole 16-byte groups; consumed_bytes looks back).
template <typename S>
JLS_DEV void load_point(const uint8_t* p, uint8_t* smem, S* line, uint32_t line_samples, int* run_index, int* corner,
                        wave::RingReader& br, const ScanDesc& d, uint8_t* ring, size_t reader_at, int lane)
{
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
    uint32_t* ctx = reinterpret_cast<uint32_t*>(smem);
    for (uint32_t i = lane; i < kRunOff / 4; i += wave::kLanes)
        ctx[i] = q[i];
    uint32_t* run = reinterpret_cast<uint32_t*>(smem + wave::kCtxBytes);
    if (lane < 8)
        run[lane] = q[kRunOff / 4 + lane];
    const S* ql = reinterpret_cast<const S*>(p + kLineOff);
    for (uint32_t i = lane; i < line_samples; i += wave::kLanes)
        line[i] = ql[i];
    const int32_t* ri = reinterpret_cast<const int32_t*>(p + kRunIndexOff);
    const int32_t* co = reinterpret_cast<const int32_t*>(p + kCornerOff);
    for (int j = 0; j < 4; ++j)
    { // (range-checked by the host; RUNindex is an index into J[] and is held to it here as well)
        const int r = ri[j];
        run_index[j] = r < 0 ? 0 : (r > 31 ? 31 : r);
        corner[j] = co[j];
    }
    const uint64_t* rd = reinterpret_cast<const uint64_t*>(p + reader_at);
    const uint64_t mis = (uint64_t)(reinterpret_cast<uintptr_t>(d.stream) & 15u);
    br.gbase = d.stream - mis;
    br.ring = ring;
    br.lane = lane;
    br.u_begin = mis;
    br.u_end = mis + d.stream_capacity;
    br.u_pos = mis + rd[0];
    br.u_loaded = br.u_pos >= 16 ? ((br.u_pos - 16) & ~(uint64_t)15) : 0;
    br.cache = rd[1];
    br.valid = (int)(uint32_t)rd[2];
    br.restart_counter = reinterpret_cast<const uint32_t*>(p + kRestartOff)[0];
    br.err = kOk;
}

// Does the wavefront's state equal point p?  Wave-uniform answer.
template <typename S>
JLS_DEV bool same_as_point(const uint8_t* p, const uint8_t* smem, const S* line, uint32_t line_samples, const int* run_index,
                           const int* corner, const wave::RingReader& br, size_t reader_at, int lane)
{
    bool differ = false;
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
    const uint32_t* ctx = reinterpret_cast<const uint32_t*>(smem);
    for (uint32_t i = lane; i < kRunOff / 4; i += wave::kLanes)
        differ = differ || q[i] != ctx[i];
    const uint32_t* run = reinterpret_cast<const uint32_t*>(smem + wave::kCtxBytes);
    if (lane < 8)
        differ = differ || q[kRunOff / 4 + lane] != run[lane];
    const S* ql = reinterpret_cast<const S*>(p + kLineOff);
    for (uint32_t i = lane; i < line_samples; i += wave::kLanes)
        differ = differ || ql[i] != line[i];
    if (lane == 0)
    {
        const int32_t* ri = reinterpret_cast<const int32_t*>(p + kRunIndexOff);
        const int32_t* co = reinterpret_cast<const int32_t*>(p + kCornerOff);
        for (int j = 0; j < 4; ++j)
            differ = differ || ri[j] != run_index[j] || co[j] != corner[j];
        differ = differ || reinterpret_cast<const uint32_t*>(p + kRestartOff)[0] != br.restart_counter;
        const uint64_t* rd = reinterpret_cast<const uint64_t*>(p + reader_at);
        differ = differ || rd[0] != br.u_pos - br.u_begin || rd[1] != br.cache || rd[2] != (uint64_t)(uint32_t)br.valid;
    }
    return !__any(differ);
}

} // namespace seek

// Dynamic LDS as decode_scans_wave.  Seek points of block b go to points + b * scan_stride + (i - 1) * point_bytes.
template <typename S, int NC>
__global__ void __launch_bounds__(64) decode_scans_wave_emit(const ScanDesc* __restrict__ descs, ScanResult* __restrict__ results,
                                                             uint8_t* __restrict__ points, uint64_t scan_stride, uint32_t lines)
{
    using namespace wave;
    JLS_DYNAMIC_LDS(smem);
    const int lane = threadIdx.x;
    const ScanDesc d = descs[blockIdx.x];
    const Traits t = make_traits(d);
    const WaveModel m{reinterpret_cast<PackedCtx*>(smem), reinterpret_cast<RunCtx*>(smem + kCtxBytes)};
    uint8_t* ring = smem + kCtxBytes + kRunBytes;
    S* line = reinterpret_cast<S*>(smem + kFixedLds);
    const uint32_t ps = d.width + 2;
    const int planes = d.interleave_mode == 0 ? 1 : d.components;
    const bool wide = sizeof(S) == 2;
    const size_t point_bytes = seek::point_bytes(d.width, planes, wide);
    const size_t reader_at = seek::reader_off(d.width, planes, wide);
    uint8_t* my_points = points + (size_t)blockIdx.x * scan_stride;

    init_model(t, m, lane);
    for (uint32_t i = lane; i < (uint32_t)planes * ps; i += kLanes)
        line[i] = 0;
    __syncthreads();

    RingReader br;
    br.init(d.stream, d.stream_capacity, ring, lane);
    int corner[4] = {0, 0, 0, 0};
    int run_index[4] = {0, 0, 0, 0};
    uint32_t left_in_interval = lines;

    for (uint32_t y = 0; y < d.height && br.err == kOk; ++y)
    {
        if (NC > 1)
            decode_line<S, NC>(t, m, br, line, ps, d.width, corner, run_index[0], lane);
        else
            for (int j = 0; j < planes; ++j)
                decode_line<S, 1>(t, m, br, line + j * ps, ps, d.width, corner + j, run_index[j], lane);
        if (br.err != kOk)
            break;
        if (d.pixels != nullptr) // (wave-uniform; an index-only build has nowhere to put rows: a seek point is the LDS line)
            line_to_row<S>(d, line, ps, d.pixels + (size_t)y * d.pixel_stride, lane);
        JLS_LOCKSTEP();
        if (--left_in_interval == 0 && y + 1 < d.height)
        {
            left_in_interval = lines;
            const uint32_t i = (y + 1) / lines;
            seek::save_point<S>(my_points + (size_t)(i - 1) * point_bytes, smem, line, (uint32_t)planes * ps, run_index, corner,
                                br, reader_at, lane);
            __syncthreads(); // (the next line's first store must not overtake a lane that is still copying)
        }
    }
    if (br.err == kOk)
        br.end_scan();
    if (lane == 0)
    {
        ScanResult r;
        r.errc = br.err;
        r.flags = 1;
        r.bytes = br.err == kOk ? br.consumed_bytes() : 0;
        results[blockIdx.x] = r;
    }
}

// Dynamic LDS as decode_scans_wave.  One work item (seek_decode.h: SeekWork) per block.
template <typename S, int NC>
__global__ void __launch_bounds__(64) decode_scans_wave_resume(const ScanDesc* __restrict__ descs, const seek::SeekWork* __restrict__ work,
                                                               ScanResult* __restrict__ results, const uint8_t* __restrict__ points)
{
    using namespace wave;
    JLS_DYNAMIC_LDS(smem);
    const int lane = threadIdx.x;
    const seek::SeekWork w = work[blockIdx.x];
    const ScanDesc d = descs[w.scan];
    const Traits t = make_traits(d);
    const WaveModel m{reinterpret_cast<PackedCtx*>(smem), reinterpret_cast<RunCtx*>(smem + kCtxBytes)};
    uint8_t* ring = smem + kCtxBytes + kRunBytes;
    S* line = reinterpret_cast<S*>(smem + kFixedLds);
    const uint32_t ps = d.width + 2;
    const int planes = d.interleave_mode == 0 ? 1 : d.components;
    const bool wide = sizeof(S) == 2;
    const size_t reader_at = seek::reader_off(d.width, planes, wide);

    RingReader br;
    int corner[4] = {0, 0, 0, 0};
    int run_index[4] = {0, 0, 0, 0};
    if (w.first_row == 0)
    {
        init_model(t, m, lane);
        for (uint32_t i = lane; i < (uint32_t)planes * ps; i += kLanes)
            line[i] = 0;
        __syncthreads();
        br.init(d.stream, d.stream_capacity, ring, lane);
    }
    else
    {
        seek::load_point<S>(points + w.from_point, smem, line, (uint32_t)planes * ps, run_index, corner, br, d, ring, reader_at, lane);
        __syncthreads();
    }

    uint32_t y = w.first_row; // (behind the loop: the rows that were completed, first_row + their count)
    for (; y < w.end_row && br.err == kOk; ++y)
    {
        if (NC > 1)
            decode_line<S, NC>(t, m, br, line, ps, d.width, corner, run_index[0], lane);
        else
            for (int j = 0; j < planes; ++j)
                decode_line<S, 1>(t, m, br, line + j * ps, ps, d.width, corner + j, run_index[j], lane);
        if (br.err != kOk)
            break;
        if (y >= w.store_from)
            line_to_row<S>(d, line, ps, d.pixels + (size_t)(y - w.row_base) * d.pixel_stride, lane);
        JLS_LOCKSTEP();
    }
    uint32_t flags = 1;
    const bool ends_scan = w.mode == seek::kResumeEnd || w.mode == seek::kResumePrefix;
    if (br.err == kOk && ends_scan)
        br.end_scan();
    else if (br.err == kOk && w.mode == seek::kResumeCompare)
    {
        __syncthreads();
        flags |= seek::kSeekChecked;
        if (!seek::same_as_point<S>(points + w.to_point, smem, line, (uint32_t)planes * ps, run_index, corner, br, reader_at, lane))
            flags |= seek::kSeekMismatch;
    }
    if (lane == 0)
    {
        ScanResult r;
        r.errc = br.err;
        r.flags = flags;
        r.bytes = br.err == kOk && ends_scan ? br.consumed_bytes() : 0;
        if (br.err != kOk && w.mode == seek::kResumePrefix)
            r.bytes = y; // the rows before the error are whole, and stored where the item stores rows
        results[blockIdx.x] = r;
    }
}

} // namespace jls
