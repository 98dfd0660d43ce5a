// pack_streams.hip -- the segmented unaligned copy behind the packed-stream calls (charls_amd.h part 2d; host/batch_packed.cpp):
// every job moves `bytes` from anywhere in a source allocation to anywhere in a destination allocation and writes
// `pad_bytes` zeros behind them.  Compiled for gfx950 only; tests/emu/emu_pack_driver.cpp runs the kernel on the host.
//
// Pure bandwidth work, driven from the DESTINATION: a workgroup of four wavefronts walks the 16-byte aligned granules of
// its job's destination extent, grid-stride over blockIdx.x; blockIdx.y strides over the jobs, so that a 40-byte stream
// beside a 7 MB one costs no tail.
//  * A granule that lies wholly inside the job's extent is ONE 16-byte store of a lane.  Its bytes come from the two aligned
//    16-byte source granules that straddle it, joined by the job's byte shift (wave-uniform: the same for every granule of a
//    job).  kUnroll granules per lane are loaded before the first of them is used.
//  * The granules at either end of the extent may be SHARED with other jobs -- with an offset alignment below 16 the last
//    granule of stream f is the first of stream f + 1, and three tiny streams fit in one granule -- and another workgroup
//    writes them at the same time.  They are never read and written back: head and tail are byte stores of exactly the
//    job's own bytes.
//
// Memory rule: source bytes of interior granules are read in whole 16-byte granules at 16-byte aligned addresses, and only
// granules that hold at least one byte of the job (up to 15 bytes before and behind the job's bytes are touched: the
// 16-byte readability rule of charls_amd_decode_batch_device).  Head, tail and the one granule where the copy ends and the
// padding begins read their bytes one by one.  Nothing is written outside [dst_offset, dst_offset + bytes + pad_bytes).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pack_streams.h"

namespace jls {
namespace pack {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kUnroll = 4;                               // granules of a lane in flight
constexpr uint64_t kTripGranules = uint64_t{kThreads} * kUnroll; // what one workgroup trip moves: 16 KiB
constexpr uint64_t kTripBytes = 16 * kTripGranules;

struct alignas(16) Granule
{
    uint64_t lo, hi;
};

// Bytes [shift, shift + 16) of the 32 bytes a | b (shift 1..15; wave-uniform).
__device__ __forceinline__ Granule joined(const Granule& a, const Granule& b, uint32_t shift)
{
    const bool high = shift >= 8;
    const uint64_t w0 = high ? a.hi : a.lo, w1 = high ? b.lo : a.hi, w2 = high ? b.hi : b.lo;
    const int s = (int)(shift & 7u) * 8;
    Granule r;
    r.lo = s ? (w0 >> s) | (w1 << (64 - s)) : w0;
    r.hi = s ? (w1 >> s) | (w2 << (64 - s)) : w1;
    return r;
}

// Destination granules [0, count) at `dst` (16-byte aligned) from the source bytes at `src`; every one of them is wholly
// source bytes.  kShifted: src is not 16-byte aligned -- granule g is joined from the aligned source granules g and g + 1,
// both of which hold bytes of the job.
template <bool kShifted>
__device__ __forceinline__ void copy_granules(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint64_t count)
{
    const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 15u);
    const uint8_t* granule0 = src - shift;
    const uint64_t last = count - 1;
    for (uint64_t base = (uint64_t)blockIdx.x * kTripGranules; base < count; base += (uint64_t)gridDim.x * kTripGranules)
    {
        Granule a[kUnroll], b[kUnroll];
        // (the loads are unconditional -- an index behind the last granule reads the last one again -- so that all of them
        // are issued before the first wait)
#pragma unroll
        for (uint32_t u = 0; u < kUnroll; ++u)
        {
            const uint64_t g = base + u * kThreads + threadIdx.x;
            const uint64_t at = 16 * (g < last ? g : last);
            a[u] = *reinterpret_cast<const Granule*>(granule0 + at);
            if (kShifted)
                b[u] = *reinterpret_cast<const Granule*>(granule0 + at + 16);
        }
#pragma unroll
        for (uint32_t u = 0; u < kUnroll; ++u)
        {
            const uint64_t g = base + u * kThreads + threadIdx.x;
            if (g < count)
                *reinterpret_cast<Granule*>(dst + 16 * g) = kShifted ? joined(a[u], b[u], shift) : a[u];
        }
    }
}

} // namespace pack

// grid (x: shares of a job's granules, y: jobs) x 256.
__global__ void __launch_bounds__(256) pack_streams_kernel(const uint8_t* __restrict__ src_base, uint8_t* __restrict__ dst_base,
                                                           const PackJob* __restrict__ jobs, uint32_t count)
{
    using namespace pack;
    for (uint32_t j = blockIdx.y; j < count; j += gridDim.y)
    {
        const PackJob job = jobs[j];
        const uint64_t total = job.bytes + job.pad_bytes;
        if (total == 0)
            continue;
        const uint8_t* src = src_base + job.src_offset;
        uint8_t* dst = dst_base + job.dst_offset;
        const uintptr_t d0 = reinterpret_cast<uintptr_t>(dst), d1 = d0 + total;
        // [in0, in1): the granules that lie wholly inside the extent (in0 >= d1: there is none, the head is everything)
        const uintptr_t in0 = (d0 + 15) & ~uintptr_t{15}, in1 = d1 & ~uintptr_t{15};
        const uintptr_t head_end = in0 < d1 ? in0 : d1;
        if (blockIdx.x == 0 && threadIdx.x < 32)
        { // head [d0, head_end) and tail [tail_begin, d1): at most 15 bytes each, one byte store per lane
            const uintptr_t tail_begin = in1 > head_end ? in1 : head_end;
            const bool head = threadIdx.x < 16;
            const uintptr_t at = head ? d0 + threadIdx.x : tail_begin + (threadIdx.x - 16);
            if (at < (head ? head_end : d1))
            {
                const uint64_t k = at - d0;
                dst[k] = k < job.bytes ? src[k] : (uint8_t)0;
            }
        }
        if (in0 >= in1)
            continue;
        const uint64_t granules = (in1 - in0) / 16;
        const uint64_t k0 = in0 - d0; // the job's byte at the first interior granule
        uint64_t whole = job.bytes >= k0 + 16 ? (job.bytes - k0) / 16 : 0; // granules that are wholly source bytes
        whole = whole < granules ? whole : granules;
        uint8_t* interior = dst + k0; // (16-byte aligned)
        if (whole != 0)
        {
            if ((reinterpret_cast<uintptr_t>(src + k0) & 15u) != 0)
                copy_granules<true>(interior, src + k0, whole);
            else
                copy_granules<false>(interior, src + k0, whole);
        }
        if (blockIdx.x == 0)
        { // the granule where the source bytes end (its bytes are read one by one) and the granules of padding behind it
            for (uint64_t g = whole + threadIdx.x; g < granules; g += kThreads)
            {
                const uint64_t k = k0 + 16 * g;
                const uint32_t have = job.bytes > k ? (uint32_t)(job.bytes - k) : 0u; // < 16
                Granule v{0, 0};
                for (uint32_t q = 0; q < have; ++q)
                {
                    const uint64_t byte = src[k + q];
                    if (q < 8)
                        v.lo |= byte << (8 * q);
                    else
                        v.hi |= byte << (8 * (q - 8));
                }
                *reinterpret_cast<Granule*>(interior + 16 * g) = v;
            }
        }
    }
}

} // namespace jls

#ifndef JLS_EMULATED
#include "runtime.h"

namespace jls::dev {

// Blocks: at most 1024 rows of jobs (the kernel strides over the rest) and, in x, as many shares as the longest job has
// trips, while the grid stays within 4096 workgroups (256 CUs x 8 resident workgroups, twice over: the jobs differ in
// length); the kernel grid-strides over what is left.
void launch_pack_streams(const uint8_t* d_src, uint8_t* d_dst, const PackJob* d_jobs, uint32_t count, uint64_t longest_bytes,
                         hipStream_t stream)
{
    if (count == 0)
        return;
    const uint32_t rows = count < 1024u ? count : 1024u;
    const uint64_t trips = (longest_bytes + pack::kTripBytes - 1) / pack::kTripBytes;
    const uint64_t room = 4096u / rows;
    const uint32_t shares = static_cast<uint32_t>(trips < 1 ? 1 : (trips < room ? trips : room));
    hipLaunchKernelGGL(pack_streams_kernel, dim3(shares, rows), dim3(pack::kThreads), 0, stream, d_src, d_dst, d_jobs, count);
    hip_check(hipGetLastError());
}

} // namespace jls::dev
#endif
