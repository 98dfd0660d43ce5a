// TEST-ONLY driver of the segmented copy kernel (pack_streams.hip compiled for the host), a library of its own
// (tests/test_emu_pack_streams.py).  The test compares the kernel with numpy slicing.
#include "emu_launch.h"

namespace emu {
BlockState* g_block = nullptr;
thread_local dim3 t_threadIdx, t_blockIdx, t_blockDim, t_gridDim;
} // namespace emu

#include "../../charls_amd/csrc/device/pack_streams.hip"
#include "../../charls_amd/csrc/device/scan_types.h"

extern "C" {

size_t emu_sizeof_scan_desc() { return sizeof(jls::ScanDesc); }
size_t emu_sizeof_pack_job() { return sizeof(jls::PackJob); }
uint64_t emu_pack_trip_bytes() { return jls::pack::kTripBytes; }

// grid (shares, rows) as dev::launch_pack_streams shapes it; the test chooses both to reach the grid-stride loops.
void emu_pack_streams(const uint8_t* src, uint8_t* dst, const jls::PackJob* jobs, uint32_t count, uint32_t shares, uint32_t rows)
{
    emu::launch(jls::pack_streams_kernel, dim3(shares, rows), dim3(jls::pack::kThreads), 0, src, dst, jobs, count);
}

} // extern "C"
