// seek_decode.h -- seek points of the exact scan decoder (scan_seek_decode.hip): layout and launches, shared by the host
// facade (host/decoder_index.cpp) and the kernels.
//
// A seek point is the complete state of decode_scans_wave at a line boundary, in the kernel's own packed forms, so that a
// later decode can start a wavefront there.  Layout of one point (little-endian, offsets in bytes):
//     0  365 packed regular contexts {A : 32 | -B : 8 | C : 8 | N : 16}       2920
//  2920  2 run-interruption contexts {RItype, A, N, Nn} as int32               32
//  2952  RUNindex[4] (int32)                                                   16
//  2968  corner[4] (int32): prev[0] of every plane                             16
//  2984  restart counter (uint32), 4 bytes of zero                              8
//  2992  the line buffer: planes x (width + 2) samples of S, padded to 8
//   end  reader: position relative to the scan's first entropy-coded byte (uint64), cache (uint64), valid bits (int32), 0
#pragma once
#include <cstddef>
#include <cstdint>

#include "scan_types.h"

#ifdef __HIPCC__
#include <hip/hip_runtime_api.h>
#endif

namespace jls::seek {

constexpr uint32_t kCtxCount = 365;
constexpr uint32_t kCtxOff = 0;
constexpr uint32_t kRunOff = kCtxCount * 8;  // 2920: the compared context bytes, without the LDS table's pad
constexpr uint32_t kRunIndexOff = kRunOff + 32;
constexpr uint32_t kCornerOff = kRunIndexOff + 16;
constexpr uint32_t kRestartOff = kCornerOff + 16;
constexpr uint32_t kLineOff = kRestartOff + 8;
constexpr uint32_t kReaderBytes = 24;

constexpr size_t line_bytes(uint32_t width, int32_t planes, bool wide)
{
    const size_t raw = static_cast<size_t>(planes) * (static_cast<size_t>(width) + 2) * (wide ? 2 : 1);
    return (raw + 7) & ~size_t{7};
}
constexpr size_t point_bytes(uint32_t width, int32_t planes, bool wide)
{
    return kLineOff + line_bytes(width, planes, wide) + kReaderBytes;
}
constexpr size_t reader_off(uint32_t width, int32_t planes, bool wide)
{
    return kLineOff + line_bytes(width, planes, wide);
}

// Seek points of a scan that decodes `lines` lines per interval: one at every line y = i * lines, 0 < y < height.
constexpr uint32_t points_per_scan(uint32_t height, uint32_t lines)
{
    return lines == 0 || height == 0 ? 0u : (height - 1) / lines;
}

// What a wavefront of decode_scans_wave_resume does.
enum : uint32_t
{
    kResumeBand = 0,    // decode, store the rows asked for, stop
    kResumeCompare = 1, // ... then compare the end state with the point at `to_point`
    kResumeEnd = 2,     // ... then end the scan (end_scan) and report the bytes consumed, as decode_scans_wave does
    kResumePrefix = 3,  // as kResumeEnd; an item that stops on an error reports in ScanResult.bytes the row behind the
                        // last one it completed (first_row where there is none): rows [first_row, bytes) are whole
};
// ScanResult.flags of a resumed interval: bit 0 as decode_scans_wave sets it, and the outcome of a comparison.
enum : uint32_t
{
    kSeekMismatch = 2u, // the end state differs from the next seek point
    kSeekChecked = 4u,  // a comparison took place (and the interval decoded without error)
};

struct SeekWork
{
    uint32_t scan;       // index into the launch's ScanDesc array
    uint32_t first_row;  // 0: start from the initial state; else from the point at `from_point`
    uint32_t end_row;    // rows [first_row, end_row) are decoded
    uint32_t store_from; // rows [store_from, end_row) are stored, row r at pixels + (r - row_base) * pixel_stride
    uint32_t mode;       // kResume*
    uint32_t row_base;
    uint64_t from_point; // byte offsets into the launch's seek-point buffer
    uint64_t to_point;
};

// One job of segment_hash_kernel (segment_hash.hip): the bytes [offset, offset + bytes) of a batch's stream slots.
struct HashJob
{
    uint64_t offset; // from the first slot; no alignment
    uint64_t bytes;  // 0 included
};

} // namespace jls::seek

#ifdef __HIPCC__
namespace jls::dev {

// decode_scans_wave's conditions (decode_launch.hip: wave_decode_eligible) and no restart intervals.
bool seek_decode_eligible(const ScanDesc& d) noexcept;
// One scan per wavefront, as decode_scans_wave, writing the seek points of scan s from d_points + s * scan_stride.
void launch_seek_emit(const ScanDesc& proto, const ScanDesc* d_descs, ScanResult* d_results, uint32_t count, uint8_t* d_points,
                      uint64_t scan_stride, uint32_t lines, hipStream_t stream);
// One interval (or band) per wavefront; all work items share proto's geometry and coding mode.
void launch_seek_resume(const ScanDesc& proto, const ScanDesc* d_descs, const seek::SeekWork* d_work, ScanResult* d_results,
                        uint32_t count, const uint8_t* d_points, hipStream_t stream);
// d_out[j] = jls::segment_hash of job j's bytes (seek_index.h), one wavefront per job.
void launch_segment_hash(const uint8_t* d_slots, const seek::HashJob* d_jobs, uint64_t* d_out, uint32_t count, hipStream_t stream);

} // namespace jls::dev
#endif
