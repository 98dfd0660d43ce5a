// segment_hash.hip -- jls::segment_hash (host/decoder_index.cpp) for segments that live in device memory: the batch calls
// of the seek-point index (host/batch_index.cpp) check and produce the hash of every entropy-coded segment where the
// streams are, in HBM.  Compiled for gfx950 only; tests/emu/emu_hash_driver.cpp runs the kernel on the host.
//
// The function: h0 = seed ^ n * k1; per 8 bytes w: h = rotl(h ^ rotl(w * k2, 31) * k1, 27) * k1 + c; the zero-padded tail
// word t: h ^= t * k2; murmur3's finaliser.
//  * w' = rotl(w * k2, 31) * k1 depends on the word alone: every lane prepares two words per trip from 16-byte loads.
//  * the fold over w' is one serial chain per segment: it is kept in wave-uniform values (the lanes' words are read
//    lane by lane), so it runs on the scalar unit while the vector unit loads and prepares the next trip.
// One wavefront per segment; many segments in flight are what hides the chain.
//
// Memory rule: a job's bytes are read in whole 16-byte granules at 16-byte aligned addresses, and only granules that hold
// at least one byte of the segment (the rule of charls_amd_decode_batch_device: nothing is read past the 16-byte boundary
// behind a slot's end).  A job of length 0 reads nothing.
#include <hip/hip_runtime.h>

#include "seek_decode.h"

namespace jls {
namespace hash {

constexpr uint64_t kK1 = 0x9E3779B185EBCA87ull, kK2 = 0xC2B2AE3D27D4EB4Full;
constexpr uint64_t kSeed = 0x27D4EB2F165667C5ull, kAdd = 0x85EBCA77C2B2AE63ull;
constexpr uint32_t kLanes = 64;
constexpr uint32_t kTripWords = 2 * kLanes; // 16 bytes per lane

struct Quad
{
    uint64_t lo, hi;
};

__device__ __forceinline__ uint64_t rotl64(uint64_t v, int s)
{
    return (v << s) | (v >> (64 - s));
}
__device__ __forceinline__ uint64_t prepared(uint64_t w)
{
    return rotl64(w * kK2, 31) * kK1;
}
__device__ __forceinline__ uint64_t folded(uint64_t h, uint64_t prepared_word)
{
    return rotl64(h ^ prepared_word, 27) * kK1 + kAdd;
}
// Lane `lane`'s value for the whole wavefront (lane: wave-uniform).
__device__ __forceinline__ uint64_t from_lane(uint64_t v, int lane)
{
#ifdef JLS_EMULATED
    return __shfl(v, lane);
#else
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return ((uint64_t)hi << 32) | lo;
#endif
}

// The aligned granules `unit` and `unit + 1` from `granule0` as they lie in memory.  The loads are unconditional -- an index
// beyond the segment's last granule reads that last granule again -- so that nothing has to wait for them before the
// values are used, a trip later (words_of).  granules > 0.
struct Loaded
{
    Quad q0, q1;
};
__device__ __forceinline__ Loaded load_unit(const uint8_t* granule0, uint64_t unit, uint64_t granules)
{
    const uint64_t last = granules - 1;
    Loaded l;
    l.q0 = *reinterpret_cast<const Quad*>(granule0 + 16 * (unit < last ? unit : last));
    l.q1 = *reinterpret_cast<const Quad*>(granule0 + 16 * (unit + 1 < last ? unit + 1 : last));
    return l;
}
// The two words at segment bytes [16 * unit, 16 * unit + 16) (unit counts from the segment's first byte): granules unit
// and unit + 1, shifted by the segment's misalignment.  Granules beyond `granules` count as zero: they hold nothing of
// the segment.
__device__ __forceinline__ Quad words_of(const Loaded& l, uint64_t unit, uint64_t granules, uint32_t mis)
{
    const bool have0 = unit < granules, have1 = unit + 1 < granules;
    const uint64_t a0 = have0 ? l.q0.lo : 0, a1 = have0 ? l.q0.hi : 0, a2 = have1 ? l.q1.lo : 0, a3 = have1 ? l.q1.hi : 0;
    const bool high = mis >= 8;
    const uint64_t b0 = high ? a1 : a0, b1 = high ? a2 : a1, b2 = high ? a3 : a2;
    const int s = (int)(mis & 7u) * 8;
    Quad r;
    r.lo = s ? (b0 >> s) | (b1 << (64 - s)) : b0;
    r.hi = s ? (b1 >> s) | (b2 << (64 - s)) : b1;
    return r;
}

} // namespace hash

// grid (jobs) x 64: out[j] = segment_hash(slots + jobs[j].offset, jobs[j].bytes).
__global__ void __launch_bounds__(64) segment_hash_kernel(const uint8_t* __restrict__ slots, const seek::HashJob* __restrict__ jobs,
                                                          uint64_t* __restrict__ out)
{
    using namespace hash;
    const int lane = threadIdx.x;
    const seek::HashJob job = jobs[blockIdx.x];
    const uint8_t* p = slots + job.offset;
    const uint64_t n = job.bytes;
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u);
    const uint8_t* granule0 = p - mis;
    const uint64_t granules = n == 0 ? 0 : (mis + n + 15) / 16;
    const uint64_t full = n / 8;
    const uint32_t tail_bytes = (uint32_t)(n & 7u);
    const uint64_t words = full + (tail_bytes ? 1 : 0);
    const uint64_t trips = (words + kTripWords - 1) / kTripWords;

    uint64_t h = kSeed ^ (n * kK1);
    uint64_t tail = 0;
    Loaded next{};
    if (trips)
        next = load_unit(granule0, (uint64_t)lane, granules);
    for (uint64_t t = 0; t < trips; ++t)
    {
        const Quad raw = words_of(next, t * kLanes + lane, granules, mis);
        next = load_unit(granule0, (t + 1) * kLanes + lane, granules); // (in flight during this trip's fold)
        const uint64_t p0 = prepared(raw.lo), p1 = prepared(raw.hi);
        const uint64_t first = t * kTripWords;
        if (full >= first && full - first >= kTripWords)
        {
#pragma unroll 8
            for (int j = 0; j < (int)kLanes; ++j)
            {
                h = folded(h, from_lane(p0, j));
                h = folded(h, from_lane(p1, j));
            }
        }
        else
        { // the segment's last trip: `count` whole words, then the tail word where there is one
            const uint32_t count = full > first ? (uint32_t)(full - first) : 0u;
            for (uint32_t j = 0; j < count / 2; ++j)
            {
                h = folded(h, from_lane(p0, (int)j));
                h = folded(h, from_lane(p1, (int)j));
            }
            if (count & 1u)
                h = folded(h, from_lane(p0, (int)(count / 2)));
            if (tail_bytes)
            {
                const uint64_t word = from_lane((count & 1u) ? raw.hi : raw.lo, (int)(count / 2));
                tail = word & ((1ull << (8 * tail_bytes)) - 1);
            }
        }
    }
    h ^= tail * kK2;
    h ^= h >> 33;
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33;
    h *= 0xC4CEB9FE1A85EC53ull;
    h ^= h >> 33;
    if (lane == 0)
        out[blockIdx.x] = h;
}

} // namespace jls

#ifndef JLS_EMULATED
#include "runtime.h"

namespace jls::dev {

void launch_segment_hash(const uint8_t* d_slots, const seek::HashJob* d_jobs, uint64_t* d_out, uint32_t count, hipStream_t stream)
{
    if (count == 0)
        return;
    hipLaunchKernelGGL(segment_hash_kernel, dim3(count), dim3(64), 0, stream, d_slots, d_jobs, d_out);
    hip_check(hipGetLastError());
}

} // namespace jls::dev
#endif
