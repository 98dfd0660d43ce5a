// TEST-ONLY driver of the two kernels behind the salvage decode through the seek-point index (charls_amd.h part 2h):
// decode_scans_wave_emit / decode_scans_wave_resume (scan_seek_decode.hip) and judge_and_fill (salvage_intervals.hip),
// compiled for the host in ONE library (tests/test_emu_salvage_index.py), so that a test can take a damaged stream from
// the seek points of its sound self through the resumed intervals to the verdicts and the fill, as the host does.
#include "emu_launch.h"

namespace emu {
BlockState* g_block = nullptr;
thread_local dim3 t_threadIdx, t_blockIdx, t_blockDim, t_gridDim;
} // namespace emu

#include "../../charls_amd/csrc/device/salvage_intervals.hip"
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
size_t emu_sizeof_scan_result() { return sizeof(jls::ScanResult); }
size_t emu_sizeof_seek_work() { return sizeof(jls::seek::SeekWork); }
size_t emu_seek_point_bytes(uint32_t width, int planes, int wide) { return jls::seek::point_bytes(width, planes, wide != 0); }
size_t emu_seek_reader_off(uint32_t width, int planes, int wide) { return jls::seek::reader_off(width, planes, wide != 0); }
uint32_t emu_mode_prefix() { return jls::seek::kResumePrefix; }
uint32_t emu_rule_by_index() { return jls::salvage::kByIndex; }
uint32_t emu_rule_by_prefix() { return jls::salvage::kByPrefix; }
uint64_t emu_ends_in_next_point() { return jls::salvage::kEndsInNextPoint; }

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

void emu_salvage_judge(const jls::ScanDesc* parents, uint32_t intervals, uint32_t scans, const jls::ScanResult* sub_results,
                       const uint64_t* expect, uint8_t* status, uint32_t fill, uint32_t wide, uint64_t row_bytes)
{
    emu::launch(jls::salvage::judge_and_fill, dim3(intervals, scans), dim3(jls::salvage::kFillThreads), 0, parents, intervals,
                sub_results, expect, status, fill, wide, row_bytes);
}

} // extern "C"
