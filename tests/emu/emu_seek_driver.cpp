// TEST-ONLY driver of the seek-point kernels (scan_seek_decode.hip compiled for the host), a library of its own
// (tests/test_emu_seek_index.py).
#include "emu_launch.h"

namespace emu {
BlockState* g_block = nullptr;
thread_local dim3 t_threadIdx, t_blockIdx, t_blockDim, t_gridDim;
} // namespace emu

#include "../../charls_amd/csrc/device/scan_seek_decode.hip"

namespace {
size_t lds_of(const jls::ScanDesc& d)
{
    const int planes = d.interleave_mode == 0 ? 1 : d.components;
    return jls::wave::kFixedLds + (size_t)planes * (d.width + 2) * (d.bits_per_sample > 8 ? 2 : 1);
}
} // namespace

#define EMU_DISPATCH(KERNEL, ...)                                                                                              \
    do                                                                                                                         \
    {                                                                                                                          \
        const int nc = d.interleave_mode == 2 ? d.components : 1;                                                              \
        if (d.bits_per_sample <= 8)                                                                                            \
        {                                                                                                                      \
            if (nc == 1) emu::launch(jls::KERNEL<uint8_t, 1>, __VA_ARGS__);                                                    \
            else if (nc == 2) emu::launch(jls::KERNEL<uint8_t, 2>, __VA_ARGS__);                                               \
            else if (nc == 3) emu::launch(jls::KERNEL<uint8_t, 3>, __VA_ARGS__);                                               \
            else emu::launch(jls::KERNEL<uint8_t, 4>, __VA_ARGS__);                                                            \
        }                                                                                                                      \
        else                                                                                                                   \
        {                                                                                                                      \
            if (nc == 1) emu::launch(jls::KERNEL<uint16_t, 1>, __VA_ARGS__);                                                   \
            else if (nc == 2) emu::launch(jls::KERNEL<uint16_t, 2>, __VA_ARGS__);                                              \
            else if (nc == 3) emu::launch(jls::KERNEL<uint16_t, 3>, __VA_ARGS__);                                              \
            else emu::launch(jls::KERNEL<uint16_t, 4>, __VA_ARGS__);                                                           \
        }                                                                                                                      \
    } while (0)

extern "C" {

size_t emu_sizeof_scan_desc() { return sizeof(jls::ScanDesc); }
size_t emu_sizeof_seek_work() { return sizeof(jls::seek::SeekWork); }
size_t emu_seek_point_bytes(uint32_t width, int planes, int wide) { return jls::seek::point_bytes(width, planes, wide != 0); }

void emu_decode_scans_wave(const jls::ScanDesc* descs, jls::ScanResult* results)
{
    const jls::ScanDesc& d = descs[0];
    EMU_DISPATCH(decode_scans_wave, dim3(1), dim3(64), lds_of(d), descs, results);
}

void emu_seek_emit(const jls::ScanDesc* descs, jls::ScanResult* results, uint8_t* points, uint32_t lines)
{
    const jls::ScanDesc& d = descs[0];
    EMU_DISPATCH(decode_scans_wave_emit, dim3(1), dim3(64), lds_of(d), descs, results, points, (uint64_t)0, lines);
}

void emu_seek_resume(const jls::ScanDesc* descs, const jls::seek::SeekWork* work, jls::ScanResult* results, int count,
                     const uint8_t* points)
{
    const jls::ScanDesc& d = descs[0];
    EMU_DISPATCH(decode_scans_wave_resume, dim3(count), dim3(64), lds_of(d), descs, work, results, points);
}

} // extern "C"
