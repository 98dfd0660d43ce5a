// seek_launch.hip -- launches of the seek-point kernels (scan_seek_decode.hip; see seek_decode.h).  Compiled for gfx950 only.
#include <hip/hip_runtime.h>

#include "kernel_dispatch.h"
#include "runtime.h"
#include "scan_seek_decode.hip"
#include "seek_decode.h"

namespace jls::dev {

namespace {
size_t seek_lds(const ScanDesc& d)
{
    const size_t planes = d.interleave_mode == 0 ? 1 : static_cast<size_t>(d.components);
    return wave::kFixedLds + planes * (static_cast<size_t>(d.width) + 2) * (d.bits_per_sample > 8 ? 2 : 1);
}

} // namespace

void launch_seek_emit(const ScanDesc& proto, const ScanDesc* d_descs, ScanResult* d_results, uint32_t count, uint8_t* d_points,
                      uint64_t scan_stride, uint32_t lines, hipStream_t stream)
{
    if (count == 0)
        return;
    if (!seek_decode_eligible(proto) || lines == 0)
        raise(CHARLS_JPEGLS_ERRC_INVALID_OPERATION); // (the host asks only for scans the wave decoder takes)
    const int nc = proto.interleave_mode == 2 ? proto.components : 1;
    dispatch_sample(proto.bits_per_sample, [&](auto s) {
        dispatch_int<1, 2, 3, 4>(nc, [&](auto n) {
            launch_kernel(decode_scans_wave_emit<typename decltype(s)::type, decltype(n)::value>, dim3(count), dim3(64), seek_lds(proto),
                          stream, d_descs, d_results, d_points, scan_stride, lines);
        });
    });
}

void launch_seek_resume(const ScanDesc& proto, const ScanDesc* d_descs, const seek::SeekWork* d_work, ScanResult* d_results,
                        uint32_t count, const uint8_t* d_points, hipStream_t stream)
{
    if (count == 0)
        return;
    if (!seek_decode_eligible(proto))
        raise(CHARLS_JPEGLS_ERRC_INVALID_OPERATION);
    const int nc = proto.interleave_mode == 2 ? proto.components : 1;
    dispatch_sample(proto.bits_per_sample, [&](auto s) {
        dispatch_int<1, 2, 3, 4>(nc, [&](auto n) {
            launch_kernel(decode_scans_wave_resume<typename decltype(s)::type, decltype(n)::value>, dim3(count), dim3(64),
                          seek_lds(proto), stream, d_descs, d_work, d_results, d_points);
        });
    });
}

} // namespace jls::dev
