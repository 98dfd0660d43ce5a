// launch_group_encode.inc -- launches of encode_pixels_group (scan_group_encode.hip) in its encoding form, or, with
// JLS_UNIT_MEASURE, in its measuring form (kMeasure); see group_launch.h.  Compiled for gfx950 only.
#include <hip/hip_runtime.h>

#include "group_launch.h"
#include "scan_group_encode.hip"

// Included by launch_group_encode_u8/_u16.hip and launch_group_measure_u8/_u16.hip: one translation unit per sample width
// and form (JLS_UNIT_WIDE, JLS_UNIT_MEASURE).
namespace jls::dev {

namespace {
using LaunchSample = std::conditional_t<JLS_UNIT_WIDE != 0, uint16_t, uint8_t>;
constexpr bool kLaunchMeasure = JLS_UNIT_MEASURE != 0;
} // namespace

template <typename S, bool kMeasure>
void launch_encode_group_as(const ScanDesc& proto, int lanes, const ScanDesc* d_descs, ScanResult* d_results, uint32_t count,
                            hipStream_t stream);
// (each of the four units defines one of these)
template <>
void launch_encode_group_as<uint8_t, false>(const ScanDesc&, int, const ScanDesc*, ScanResult*, uint32_t, hipStream_t);
template <>
void launch_encode_group_as<uint16_t, false>(const ScanDesc&, int, const ScanDesc*, ScanResult*, uint32_t, hipStream_t);
template <>
void launch_encode_group_as<uint8_t, true>(const ScanDesc&, int, const ScanDesc*, ScanResult*, uint32_t, hipStream_t);
template <>
void launch_encode_group_as<uint16_t, true>(const ScanDesc&, int, const ScanDesc*, ScanResult*, uint32_t, hipStream_t);

#if JLS_UNIT_WIDE == 0 && JLS_UNIT_MEASURE == 0
size_t group_encode_lds_bytes(const ScanDesc& d, uint32_t scans_per_wave)
{
    const uint32_t nc = d.interleave_mode == 2 ? static_cast<uint32_t>(d.components) : 1u;
    const uint32_t nl = d.interleave_mode == 1 ? static_cast<uint32_t>(d.components) : 1u;
    return d.bits_per_sample > 8 ? grp::encode_workgroup_lds_bytes<uint16_t>(d.width, nc, scans_per_wave, nl)
                                 : grp::encode_workgroup_lds_bytes<uint8_t>(d.width, nc, scans_per_wave, nl);
}

void launch_encode_group(const ScanDesc& proto, int lanes, const ScanDesc* d_descs, ScanResult* d_results, uint32_t count,
                         hipStream_t stream)
{
    dispatch_sample(proto.bits_per_sample, [&](auto s) {
        launch_encode_group_as<typename decltype(s)::type, false>(proto, lanes, d_descs, d_results, count, stream);
    });
}

void launch_measure_group(const ScanDesc& proto, int lanes, const ScanDesc* d_descs, ScanResult* d_results, uint32_t count,
                          hipStream_t stream)
{
    dispatch_sample(proto.bits_per_sample, [&](auto s) {
        launch_encode_group_as<typename decltype(s)::type, true>(proto, lanes, d_descs, d_results, count, stream);
    });
}
#endif

// (the regions in LDS are those of the encoding form: one layout for both)
template <>
void launch_encode_group_as<LaunchSample, kLaunchMeasure>(const ScanDesc& proto, int lanes, const ScanDesc* d_descs,
                                                          ScanResult* d_results, uint32_t count, hipStream_t stream)
{
    using S = LaunchSample;
    const uint32_t per_wave = 64u / static_cast<uint32_t>(lanes);
    const dim3 grid((count + per_wave - 1) / per_wave);
    const size_t lds = group_encode_lds_bytes(proto, per_wave);
    const int nc = proto.interleave_mode == 2 ? proto.components : 1;
    // one line of NC co-sited components (sample interleave, single component), or NL lines of one component (line interleave)
    dispatch_int<8, 16, 32, 64>(lanes, [&](auto g) {
        constexpr int G = decltype(g)::value;
        if (proto.interleave_mode == 1)
            dispatch_int<2, 3, 4>(proto.components, [&](auto nl) {
                launch_kernel(encode_pixels_group<S, G, 1, decltype(nl)::value, kLaunchMeasure>, grid, dim3(64), lds, stream, d_descs,
                              d_results, count);
            });
        else
            dispatch_int<1, 2, 3, 4>(nc, [&](auto n) {
                launch_kernel(encode_pixels_group<S, G, decltype(n)::value, 1, kLaunchMeasure>, grid, dim3(64), lds, stream, d_descs,
                              d_results, count);
            });
    });
}

} // namespace jls::dev
