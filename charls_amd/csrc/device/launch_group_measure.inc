// launch_group_measure.inc -- launches of the measuring form of encode_pixels_group (scan_group_encode.hip, kMeasure); see
// group_launch.h.  Compiled for gfx950 only.
#include <hip/hip_runtime.h>

#if JLS_LAUNCH_WIDE
#define JLS_LAUNCH_SAMPLE uint16_t
#define JLS_LAUNCH_NAME launch_measure_group_wide
#else
#define JLS_LAUNCH_SAMPLE uint8_t
#define JLS_LAUNCH_NAME launch_measure_group_narrow
#endif

#include "group_launch.h"
#include "scan_group_encode.hip"

// Included by launch_group_measure_u8.hip and launch_group_measure_u16.hip: one translation unit per sample width.
namespace jls::dev {

void launch_measure_group_narrow(const ScanDesc& proto, int lanes, const ScanDesc* d_descs, ScanResult* d_results, uint32_t count,
                                 hipStream_t stream);
void launch_measure_group_wide(const ScanDesc& proto, int lanes, const ScanDesc* d_descs, ScanResult* d_results, uint32_t count,
                               hipStream_t stream);

#if JLS_LAUNCH_WIDE == 0
void launch_measure_group(const ScanDesc& proto, int lanes, const ScanDesc* d_descs, ScanResult* d_results, uint32_t count,
                          hipStream_t stream)
{
    if (proto.bits_per_sample > 8)
        launch_measure_group_wide(proto, lanes, d_descs, d_results, count, stream);
    else
        launch_measure_group_narrow(proto, lanes, d_descs, d_results, count, stream);
}
#endif

void JLS_LAUNCH_NAME(const ScanDesc& proto, int lanes, const ScanDesc* d_descs, ScanResult* d_results, uint32_t count,
                     hipStream_t stream)
{
    const uint32_t per_wave = 64u / static_cast<uint32_t>(lanes);
    const dim3 grid((count + per_wave - 1) / per_wave);
    const size_t lds = group_encode_lds_bytes(proto, per_wave); // (the regions of the encoding form: one layout for both)
    const int nc = proto.interleave_mode == 2 ? proto.components : 1;
#define JLS_LAUNCH_MEASURE(S, G, N, NLINES)                                                                              \
    do                                                                                                                   \
    {                                                                                                                    \
        if (lds > kMaxDynamicLds)                                                                                        \
            hip_check(hipFuncSetAttribute(reinterpret_cast<const void*>(&encode_pixels_group<S, G, N, NLINES, true>),    \
                                          hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));           \
        hipLaunchKernelGGL((encode_pixels_group<S, G, N, NLINES, true>), grid, dim3(64), lds, stream, d_descs, d_results, count); \
    } while (0)
#define JLS_LAUNCH_MEASURE_N(S, G)                                                                                       \
    do                                                                                                                   \
    {                                                                                                                    \
        if (proto.interleave_mode == 1)                                                                                  \
        {                                                                                                                \
            if (proto.components == 2) JLS_LAUNCH_MEASURE(S, G, 1, 2);                                                   \
            else if (proto.components == 3) JLS_LAUNCH_MEASURE(S, G, 1, 3);                                              \
            else JLS_LAUNCH_MEASURE(S, G, 1, 4);                                                                         \
        }                                                                                                                \
        else if (nc == 1) JLS_LAUNCH_MEASURE(S, G, 1, 1);                                                                \
        else if (nc == 2) JLS_LAUNCH_MEASURE(S, G, 2, 1);                                                                \
        else if (nc == 3) JLS_LAUNCH_MEASURE(S, G, 3, 1);                                                                \
        else JLS_LAUNCH_MEASURE(S, G, 4, 1);                                                                             \
    } while (0)
    if (lanes == 8)
    {
        JLS_LAUNCH_MEASURE_N(JLS_LAUNCH_SAMPLE, 8);
    }
    else if (lanes == 16)
    {
        JLS_LAUNCH_MEASURE_N(JLS_LAUNCH_SAMPLE, 16);
    }
    else if (lanes == 32)
    {
        JLS_LAUNCH_MEASURE_N(JLS_LAUNCH_SAMPLE, 32);
    }
    else
    {
        JLS_LAUNCH_MEASURE_N(JLS_LAUNCH_SAMPLE, 64);
    }
#undef JLS_LAUNCH_MEASURE_N
#undef JLS_LAUNCH_MEASURE
    hip_check(hipGetLastError());
}

} // namespace jls::dev
