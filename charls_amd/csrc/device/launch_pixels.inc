// launch_pixels.inc -- launches of decode_pixels_group (scan_group_pixels.hip); see group_launch.h.  Compiled for gfx950 only.
#include <hip/hip_runtime.h>

#include "group_launch.h"
#include "scan_group_pixels.hip"

// Included by launch_pixels_u8.hip and launch_pixels_u16.hip: one translation unit per sample width (JLS_UNIT_WIDE).
namespace jls::dev {

namespace {
using LaunchSample = std::conditional_t<JLS_UNIT_WIDE != 0, uint16_t, uint8_t>;
} // namespace

template <typename S>
void launch_decode_pixels_as(const ScanDesc& proto, int pixel_lanes, const ScanDesc* d_descs, ScanResult* d_results, uint32_t count,
                             hipStream_t stream);
// (each of the two units defines one of these)
template <>
void launch_decode_pixels_as<uint8_t>(const ScanDesc&, int, const ScanDesc*, ScanResult*, uint32_t, hipStream_t);
template <>
void launch_decode_pixels_as<uint16_t>(const ScanDesc&, int, const ScanDesc*, ScanResult*, uint32_t, hipStream_t);

#if JLS_UNIT_WIDE == 0
size_t pixel_group_lds_bytes(const ScanDesc& d, uint32_t scans_per_wave)
{
    const uint32_t nc = d.interleave_mode == 2 ? static_cast<uint32_t>(d.components) : 1u;
    const uint32_t nl = d.interleave_mode == 1 ? static_cast<uint32_t>(d.components) : 1u;
    return d.bits_per_sample > 8 ? grp::pixel_workgroup_lds_bytes<uint16_t>(d.width, nc, scans_per_wave, nl)
                                 : grp::pixel_workgroup_lds_bytes<uint8_t>(d.width, nc, scans_per_wave, nl);
}

void launch_decode_pixels(const ScanDesc& proto, int pixel_lanes, const ScanDesc* d_descs, ScanResult* d_results, uint32_t count,
                          hipStream_t stream)
{
    dispatch_sample(proto.bits_per_sample, [&](auto s) {
        launch_decode_pixels_as<typename decltype(s)::type>(proto, pixel_lanes, d_descs, d_results, count, stream);
    });
}
#endif

template <>
void launch_decode_pixels_as<LaunchSample>(const ScanDesc& proto, int pixel_lanes, const ScanDesc* d_descs, ScanResult* d_results,
                                           uint32_t count, hipStream_t stream)
{
    using S = LaunchSample;
    const int nc = proto.interleave_mode == 2 ? proto.components : 1;
    const uint32_t per_wave = 64u / static_cast<uint32_t>(pixel_lanes);
    const dim3 grid((count + per_wave - 1) / per_wave);
    const size_t lds = pixel_group_lds_bytes(proto, per_wave);
    // one line of NC co-sited components (sample interleave, single component), or NL lines of one component (line interleave)
    dispatch_int<8, 16, 32>(pixel_lanes, [&](auto g) {
        constexpr int G = decltype(g)::value;
        if (proto.interleave_mode == 1)
            dispatch_int<2, 3, 4>(proto.components, [&](auto nl) {
                launch_kernel(decode_pixels_group<S, G, 1, decltype(nl)::value>, grid, dim3(64), lds, stream, d_descs, d_results, count);
            });
        else
            dispatch_int<1, 2, 3, 4>(nc, [&](auto n) {
                launch_kernel(decode_pixels_group<S, G, decltype(n)::value>, grid, dim3(64), lds, stream, d_descs, d_results, count);
            });
    });
}

} // namespace jls::dev
