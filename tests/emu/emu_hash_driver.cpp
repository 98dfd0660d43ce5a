// TEST-ONLY driver of the segment-hash kernel (segment_hash.hip compiled for the host), a library of its own
// (tests/test_emu_segment_hash.py).  The host function it is compared with is the library's own (host/segment_hash.h).
#include "emu_launch.h"

namespace emu {
BlockState* g_block = nullptr;
thread_local dim3 t_threadIdx, t_blockIdx, t_blockDim, t_gridDim;
} // namespace emu

#include "../../charls_amd/csrc/device/segment_hash.hip"
#include "../../charls_amd/csrc/host/segment_hash.h"

extern "C" {

size_t emu_sizeof_scan_desc() { return sizeof(jls::ScanDesc); }
size_t emu_sizeof_hash_job() { return sizeof(jls::seek::HashJob); }

void emu_segment_hash(const uint8_t* slots, const jls::seek::HashJob* jobs, uint64_t* out, int count)
{
    emu::launch(jls::segment_hash_kernel, dim3(count), dim3(64), 0, slots, jobs, out);
}

uint64_t emu_host_segment_hash(const uint8_t* p, size_t n) { return jls::segment_hash_bytes(p, n); }

} // extern "C"
