// group_launch.h -- launches of the lanes-per-scan kernels that live in translation units of their own (their template
// instantiations are most of the device code: compiling them next to the launch units instead of inside them keeps the build
// parallel).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernel_dispatch.h"
#include "runtime.h"
#include "scan_types.h"

namespace jls::dev {

constexpr size_t kGroupDecodeLds = 160 * 1024; // a workgroup of the group kernels may take the whole LDS of a CU
constexpr uint32_t kPixelWaves = 512; // wavefronts a launch of the pixel kernels (scan_group_pixels.hip, scan_group_encode.hip) aims at: two per CU

// scan_group_pixels.hip (launch_pixels.hip)
size_t pixel_group_lds_bytes(const ScanDesc& d, uint32_t scans_per_wave);
void launch_decode_pixels(const ScanDesc& proto, int lanes, const ScanDesc* d_descs, ScanResult* d_results, uint32_t count,
                          hipStream_t stream);

// scan_group_encode.hip (launch_group_encode.hip)
size_t group_encode_lds_bytes(const ScanDesc& d, uint32_t scans_per_wave);
void launch_encode_group(const ScanDesc& proto, int lanes, const ScanDesc* d_descs, ScanResult* d_results, uint32_t count,
                         hipStream_t stream);
// its measuring form (launch_group_measure_u8/_u16.hip): ScanResult::bytes is the length of the segment launch_encode_group writes for
// the same descriptors; stream, stream_capacity and line_scratch of the descriptors are not looked at.  The LDS is
// group_encode_lds_bytes.
void launch_measure_group(const ScanDesc& proto, int lanes, const ScanDesc* d_descs, ScanResult* d_results, uint32_t count,
                          hipStream_t stream);

} // namespace jls::dev
