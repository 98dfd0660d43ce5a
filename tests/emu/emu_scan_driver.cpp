// TEST-ONLY driver of block_exclusive_scan_pair (tile_pipeline.hip compiled for the host): one workgroup scans two series of
// `count` values (tests/test_emu_tile_tables.py).
#include "emu_launch.h"

namespace emu {
BlockState* g_block = nullptr;
thread_local dim3 t_threadIdx, t_blockIdx, t_blockDim, t_gridDim;
} // namespace emu

#include "../../charls_amd/csrc/device/tile_pipeline.hip"

namespace {

__global__ void scan_pair_kernel(const uint32_t* in_a, const uint32_t* in_b, uint32_t count, uint32_t* out_a, uint32_t* out_b)
{
    __shared__ uint32_t s_tmp[16];
    uint32_t a[2] = {0, 0}, b[2] = {0, 0};
    for (int half = 0; half < 2; ++half)
    {
        const uint32_t i = threadIdx.x + (uint32_t)half * blockDim.x;
        if (i < count)
        {
            a[half] = in_a[i];
            b[half] = in_b[i];
        }
    }
    jls::tile::block_exclusive_scan_pair(a, b, count, s_tmp);
    for (int half = 0; half < 2; ++half)
    {
        const uint32_t i = threadIdx.x + (uint32_t)half * blockDim.x;
        if (i < count)
        {
            out_a[i] = a[half];
            out_b[i] = b[half];
        }
    }
}

} // namespace

extern "C" {

void emu_scan_pair(const uint32_t* in_a, const uint32_t* in_b, uint32_t count, uint32_t threads, uint32_t* out_a, uint32_t* out_b)
{
    emu::launch(scan_pair_kernel, dim3(1), dim3(threads), 0, in_a, in_b, count, out_a, out_b);
}

size_t emu_sizeof_scan_desc() { return sizeof(jls::ScanDesc); }
}
