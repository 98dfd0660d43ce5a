// seek_launch.hip -- launches of the seek-point kernels (scan_seek_decode.hip; see seek_decode.h).  Compiled for gfx950 only.
#include <hip/hip_runtime.h>

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

template <typename S>
void emit(int nc, const ScanDesc* d_descs, ScanResult* d_results, uint32_t count, uint8_t* d_points, uint64_t scan_stride,
          uint32_t lines, size_t lds, hipStream_t stream)
{
    switch (nc)
    {
    case 1:
        hipLaunchKernelGGL((decode_scans_wave_emit<S, 1>), dim3(count), dim3(64), lds, stream, d_descs, d_results, d_points, scan_stride, lines);
        break;
    case 2:
        hipLaunchKernelGGL((decode_scans_wave_emit<S, 2>), dim3(count), dim3(64), lds, stream, d_descs, d_results, d_points, scan_stride, lines);
        break;
    case 3:
        hipLaunchKernelGGL((decode_scans_wave_emit<S, 3>), dim3(count), dim3(64), lds, stream, d_descs, d_results, d_points, scan_stride, lines);
        break;
    default:
        hipLaunchKernelGGL((decode_scans_wave_emit<S, 4>), dim3(count), dim3(64), lds, stream, d_descs, d_results, d_points, scan_stride, lines);
        break;
    }
}

template <typename S>
void resume(int nc, const ScanDesc* d_descs, const seek::SeekWork* d_work, ScanResult* d_results, uint32_t count,
            const uint8_t* d_points, size_t lds, hipStream_t stream)
{
    switch (nc)
    {
    case 1:
        hipLaunchKernelGGL((decode_scans_wave_resume<S, 1>), dim3(count), dim3(64), lds, stream, d_descs, d_work, d_results, d_points);
        break;
    case 2:
        hipLaunchKernelGGL((decode_scans_wave_resume<S, 2>), dim3(count), dim3(64), lds, stream, d_descs, d_work, d_results, d_points);
        break;
    case 3:
        hipLaunchKernelGGL((decode_scans_wave_resume<S, 3>), dim3(count), dim3(64), lds, stream, d_descs, d_work, d_results, d_points);
        break;
    default:
        hipLaunchKernelGGL((decode_scans_wave_resume<S, 4>), dim3(count), dim3(64), lds, stream, d_descs, d_work, d_results, d_points);
        break;
    }
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
    if (proto.bits_per_sample > 8)
        emit<uint16_t>(nc, d_descs, d_results, count, d_points, scan_stride, lines, seek_lds(proto), stream);
    else
        emit<uint8_t>(nc, d_descs, d_results, count, d_points, scan_stride, lines, seek_lds(proto), stream);
    hip_check(hipGetLastError());
}

void launch_seek_resume(const ScanDesc& proto, const ScanDesc* d_descs, const seek::SeekWork* d_work, ScanResult* d_results,
                        uint32_t count, const uint8_t* d_points, hipStream_t stream)
{
    if (count == 0)
        return;
    if (!seek_decode_eligible(proto))
        raise(CHARLS_JPEGLS_ERRC_INVALID_OPERATION);
    const int nc = proto.interleave_mode == 2 ? proto.components : 1;
    if (proto.bits_per_sample > 8)
        resume<uint16_t>(nc, d_descs, d_work, d_results, count, d_points, seek_lds(proto), stream);
    else
        resume<uint8_t>(nc, d_descs, d_work, d_results, count, d_points, seek_lds(proto), stream);
    hip_check(hipGetLastError());
}

} // namespace jls::dev
