// TEST-ONLY driver of the measuring form of the group encoder (scan_group_encode.hip compiled for the host with kMeasure), a
// library of its own (tests/test_emu_group_measure.py).  The test compares ScanResult::bytes with the encoding form and with
// the oracle's entropy-coded segments.
#include "emu_launch.h"

namespace emu {
BlockState* g_block = nullptr;
thread_local dim3 t_threadIdx, t_blockIdx, t_blockDim, t_gridDim;
} // namespace emu

#include "../../charls_amd/csrc/device/scan_group_encode.hip"

extern "C" {

size_t emu_sizeof_scan_desc() { return sizeof(jls::ScanDesc); }

// Sample width, NC / NL and LDS chosen as dev::launch_measure_group does (launch_group_encode.inc); `group` lanes per scan.
int emu_measure_pixels_group(const jls::ScanDesc* descs, jls::ScanResult* results, int count, int group)
{
    const jls::ScanDesc& d = descs[0];
    const bool wide = d.bits_per_sample > 8;
    const int per_wave = 64 / group;
    const int nc = d.interleave_mode == 2 ? d.components : 1;
    const int nl = d.interleave_mode == 1 ? d.components : 1;
    const size_t lds = wide ? jls::grp::encode_workgroup_lds_bytes<uint16_t>(d.width, nc, per_wave, nl)
                            : jls::grp::encode_workgroup_lds_bytes<uint8_t>(d.width, nc, per_wave, nl);
    const dim3 grid((count + per_wave - 1) / per_wave);
#define EMU_MEASURE(S, G, N, NLINES) \
    emu::launch(jls::encode_pixels_group<S, G, N, NLINES, true>, grid, dim3(64), lds, descs, results, (uint32_t)count)
// (the shapes the test uses: lanes 8, 16 and 64; one component, three sample-interleaved, three line-interleaved)
#define EMU_MEASURE_G(S, N, NLINES)                          \
    do                                                       \
    {                                                        \
        if (group == 8) EMU_MEASURE(S, 8, N, NLINES);        \
        else if (group == 16) EMU_MEASURE(S, 16, N, NLINES); \
        else if (group == 64) EMU_MEASURE(S, 64, N, NLINES); \
        else return -1;                                      \
    } while (0)
#define EMU_MEASURE_S(S)                                     \
    do                                                       \
    {                                                        \
        if (nl == 3) EMU_MEASURE_G(S, 1, 3);                 \
        else if (nl == 1 && nc == 1) EMU_MEASURE_G(S, 1, 1); \
        else if (nl == 1 && nc == 3) EMU_MEASURE_G(S, 3, 1); \
        else return -1;                                      \
    } while (0)
    if (wide)
        EMU_MEASURE_S(uint16_t);
    else
        EMU_MEASURE_S(uint8_t);
#undef EMU_MEASURE_S
#undef EMU_MEASURE_G
#undef EMU_MEASURE
    return 0;
}

} // extern "C"
