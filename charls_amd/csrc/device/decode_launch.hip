// decode_launch.hip -- the decoder dispatch (see runtime.h): which kernel a scan is eligible for, the launch plans and keys, the
// restart-interval and salvage drivers, and the exact decoder's one launch behind a speed path.  Compiled for gfx950 only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "knobs.h"
#include "runtime.h"
#include "work_areas.h"
#include "scan_wave_decode.hip"
#include "scan_fast_decode.hip"
#include "scan_group_decode.hip"
#include "group_launch.h"
#include "restart_intervals_decode.hip"
#include "salvage_intervals.hip"
#include "seek_decode.h"

namespace jls::dev {

namespace {
std::atomic<uint64_t> g_salvage_launches{0}; // launches of the kernels of salvage_intervals.hip
std::atomic<uint64_t> g_exact_retry_scans{0}; // scans a speed-path decoder handed to the exact decoder (it did not end cleanly there)
} // namespace
uint64_t exact_retry_scans() noexcept
{
    return g_exact_retry_scans.load();
}
uint64_t salvage_kernel_launches() noexcept
{
    return g_salvage_launches.load();
}

namespace {

size_t wave_decode_lds(const ScanDesc& d)
{
    const size_t planes = d.interleave_mode == 0 ? 1 : static_cast<size_t>(d.components);
    return wave::kFixedLds + planes * (static_cast<size_t>(d.width) + 2) * (d.bits_per_sample > 8 ? 2 : 1);
}

bool wave_decode_eligible(const ScanDesc& d)
{
    if (wave_decode_lds(d) > kMaxDynamicLds)
        return false; // line does not fit LDS
    if (d.reset == 0)
        return false; // RESET = 256*m is stored as 0 by the reference: N is never halved and outgrows the packed context
    if (d.bits_per_sample > 8 && d.interleave_mode == 0 &&
        ((reinterpret_cast<uintptr_t>(d.pixels) | d.pixel_stride) & 1u) != 0)
        return false; // odd row address for 16-bit samples
    return true;
}

// Scans whose restart intervals can be decoded as scans of their own (restart_intervals_decode.hip, salvage_intervals.hip).
bool intervals_decodable(const ScanDesc& d)
{
    return d.restart_interval != 0 && d.restart_interval < d.height && d.height <= 65535 && d.restart_interval <= 65535 &&
           wave_decode_eligible(d);
}

// ... and are, by the ordinary decode.
bool interval_decode_candidate(const ScanDesc& d)
{
    return intervals_decodable(d) && knobs::get_or(knobs::kSequentialIntervals, 0) == 0;
}

size_t fast_decode_lds(const ScanDesc& d)
{
    const size_t line_bytes = ((static_cast<size_t>(d.width) + 2) * (d.bits_per_sample > 8 ? 2 : 1) + 3) & ~size_t{3};
    return (d.bits_per_sample > 8 ? fast::fixed_lds<uint16_t>() : fast::fixed_lds<uint8_t>()) + line_bytes;
}

// Lines a scan of the group decoder keeps in LDS: one, or one per component of a line-interleaved scan.
uint32_t group_lines(const ScanDesc& d)
{
    return d.interleave_mode == 1 ? static_cast<uint32_t>(d.components) : 1u;
}

size_t group_lds_bytes(const ScanDesc& d, uint32_t scans_per_wave)
{
    return d.bits_per_sample > 8 ? grp::workgroup_lds_bytes<uint16_t>(d.width, scans_per_wave, group_lines(d))
                                 : grp::workgroup_lds_bytes<uint8_t>(d.width, scans_per_wave, group_lines(d));
}

// Lanes per scan (G) and wavefronts per workgroup (W) of the speed path (scan_group_decode.hip) for a launch of `count` scans;
// lanes 0 = the one-scan-per-wavefront kernel (scan_fast_decode.hip).
//
// What a sample costs: a wavefront stops for every event of every one of its scans (run mode, end of line, refill), so the
// fewer scans share a wavefront the less a step takes -- 206 ns with 2 scans per wavefront, 217 with 4, 232 with 8 -- as long
// as the wavefront has a SIMD TO ITSELF: two wavefronts of this kernel on one SIMD take a third longer each (4.8 s instead of
// 3.6 s for a frame's 16.8 M samples: profiles/r05_decode_wavefronts_per_workgroup.txt).  So the rule is one wavefront per
// SIMD, and the fewest scans per wavefront that allows:
//  * up to ONE wavefront per CU, one-wavefront workgroups (W = 1); with two per CU they still find a SIMD each, but a workgroup
//    of four is 4 % faster there too (1024 frames at 32 lanes: 2.91 s against 3.03 s, round 6), so W = 1 beyond one per CU is
//    left to the scans that have no W = 4 instantiation (several lines per pixel row);
//  * beyond two per CU the dispatcher doubles one-wavefront workgroups up on some SIMDs while others idle -- not in every launch:
//    1024 of them decoded 4096 frames in 3.67 s in one call and in 4.89 s in others, at an unchanged 2.39 GHz
//    (profiles/r05_pmc_decode_effective_clock.txt; rounds 3 and 4 took the slow launches for the chip clocking down and never
//    went beyond two wavefronts per CU).  A workgroup of FOUR wavefronts that takes the whole LDS of its CU is dealt out one
//    wavefront per SIMD by construction: 4096 frames at 16 lanes per scan in 3.76 s, every time (8 lanes, W = 1: 4.05 s).
// DECODE_GROUP / DECODE_WORKGROUP_WAVES override (0, 4, 8, 16, 32 lanes; 1, 4, 8 wavefronts) where that shape is built.
struct GroupPlan
{
    int lanes, waves;
};
// The instantiations of decode_scans_group<S, G, NL, W, kNear> the library is built with, for both sample widths: one-wavefront
// workgroups (W = 1) with 4, 8, 16 or 32 lanes per scan -- near-lossless: 8, 16 or 32 -- and up to four lines per pixel row;
// workgroups of 4 or 8 wavefronts -- near-lossless: 4 -- for single-line scans with 16 or 32 lanes.  The plan and the launch
// both ask here, so they cannot drift apart.
constexpr bool group_decode_built(int G, int NL, int W, bool near)
{
    if (!(G == 8 || G == 16 || G == 32 || (G == 4 && !near)) || NL < 1 || NL > 4)
        return false;
    if (W == 1)
        return true;
    return NL == 1 && G >= 16 && (W == 4 || (W == 8 && !near));
}
GroupPlan decode_group_plan(const ScanDesc& d, uint32_t count)
{
    if (d.bits_per_sample > 8 && d.t3 > grp::kMaxTableT3)
        return {0, 1};
    const int nl = static_cast<int>(std::min(group_lines(d), 4u)); // (as the launch counts them: its last listed value is the catch-all)
    const bool near = d.near_lossless != 0;
    const int forced = static_cast<int>(knobs::get_or(knobs::kDecodeGroup, -1));
    const int forced_waves = static_cast<int>(knobs::get_or(knobs::kDecodeWorkgroupWaves, -1));
    if (forced == 0)
        return {0, 1};
    // (a forced shape that is not built -- 4 lanes or 8 wavefronts for a near-lossless scan, say -- is not forced)
    if (group_decode_built(forced, nl, 1, near))
    {
        const uint32_t per_wave = 64u / static_cast<uint32_t>(forced);
        if (forced_waves > 1 && group_decode_built(forced, nl, forced_waves, near) &&
            group_lds_bytes(d, per_wave * static_cast<uint32_t>(forced_waves)) <= kGroupDecodeLds)
            return {forced, forced_waves};
        if (group_lds_bytes(d, per_wave) <= kGroupDecodeLds)
            return {forced, 1};
    }
    static const uint32_t cus = [] {
        hipDeviceProp_t prop;
        int device = 0;
        if (hipGetDevice(&device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess)
            return 256u;
        return static_cast<uint32_t>(prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256);
    }();
    const uint32_t waves_per_cu = static_cast<uint32_t>(std::clamp<long long>(knobs::get_or(knobs::kDecodeWavesPerCu, 2), 1, 16));
    int fallback = 0;
    for (int lanes = 32; lanes >= 8; lanes /= 2)
    {
        const uint32_t per_wave = 64u / static_cast<uint32_t>(lanes);
        if (group_lds_bytes(d, per_wave) > kGroupDecodeLds)
            break;
        fallback = lanes;
        const uint32_t waves = (count + per_wave - 1) / per_wave;
        if (waves <= cus)
            return {lanes, 1}; // a CU per wavefront
        // four wavefronts per CU as ONE workgroup (it must be the only one its CU can hold: more than half of the LDS): ahead of
        // two one-wavefront workgroups per CU since round 6 -- 1024 frames at 32 lanes: 2.91 s against 3.03 s
        // (profiles/r06_decode_launch_shapes.txt)
        const uint32_t per_group = 4 * per_wave;
        if (forced_waves != 1 && group_decode_built(lanes, nl, 4, near) && group_lds_bytes(d, per_group) <= kGroupDecodeLds && (count + per_group - 1) / per_group <= cus)
            return {lanes, 4};
        if (waves <= waves_per_cu * cus)
            return {lanes, 1};
    }
    return {fallback, 1};
}
int decode_group_lanes(const ScanDesc& d, uint32_t count)
{
    return decode_group_plan(d, count).lanes;
}

// Lanes per scan of the speed path of sample-interleaved scans, lossless or near-lossless, and of near-lossless
// single-component scans (scan_group_pixels.hip); 0 = the exact decoder.  Packing as in decode_group_lanes.
int pixel_group_lanes(const ScanDesc& d, uint32_t count)
{
    const bool by_sample = d.interleave_mode == 2 && d.components >= 2 && d.components <= 4;
    // (near-lossless single-component and line-interleaved scans have decode_scans_group<.., kNear> since round 6;
    // NEAR_DECODE_PIXELS=1 brings them back here: the A/B)
    const bool near_here = knobs::get_or(knobs::kNearDecodePixels, 0) != 0;
    const bool near_planar = d.interleave_mode == 0 && d.components == 1 && d.near_lossless != 0 && near_here;
    const bool near_by_line = d.interleave_mode == 1 && d.components >= 2 && d.components <= 4 && d.near_lossless != 0 && near_here;
    if ((!by_sample && !near_planar && !near_by_line) || !wave_decode_eligible(d))
        return 0;
    if (by_sample && d.bits_per_sample > 8 && ((reinterpret_cast<uintptr_t>(d.pixels) | d.pixel_stride) & 1u) != 0)
        return 0; // odd row address for 16-bit samples
    if ((d.bits_per_sample > 8 && d.t3 > grp::kMaxTableT3) || knobs::get_or(knobs::kExactDecoder, 0) != 0)
        return 0;
    const int forced = static_cast<int>(knobs::get_or(knobs::kDecodeGroup, -1));
    if (forced == 0)
        return 0;
    if ((forced == 8 || forced == 16 || forced == 32) && pixel_group_lds_bytes(d, 64u / forced) <= kGroupDecodeLds)
        return forced;
    int best = 0;
    for (int lanes = 32; lanes >= 8; lanes /= 2)
    {
        const uint32_t per_wave = 64u / static_cast<uint32_t>(lanes);
        if (pixel_group_lds_bytes(d, per_wave) > kGroupDecodeLds)
            break;
        best = lanes;
        if ((count + per_wave - 1) / per_wave <= kPixelWaves) // (two one-wavefront workgroups per CU find a SIMD each, see decode_group_plan)
            break;
    }
    return best;
}

// Lossless single-component scans take the speed path (scan_group_decode.hip / scan_fast_decode.hip); it defers to the
// exact kernels whenever the scan does not end cleanly.
bool fast_decode_eligible(const ScanDesc& d)
{
    const bool planar = d.interleave_mode == 0 && d.components == 1;
    const bool by_line = d.interleave_mode == 1 && d.components >= 2 && d.components <= 4; // group kernel only
    // (near-lossless scans: the group kernel only)
    const bool near_ok = d.near_lossless == 0 ||
                         (knobs::get_or(knobs::kNearDecodePixels, 0) == 0 && decode_group_lanes(d, 1) != 0);
    return wave_decode_eligible(d) && near_ok && (planar || by_line) &&
           ((planar && fast_decode_lds(d) <= kMaxDynamicLds) || decode_group_lanes(d, 1) != 0) &&
           knobs::get_or(knobs::kExactDecoder, 0) == 0;
}

// Scans the speed path handed back (ScanResult.flags & kFastRetry) are gathered so that ONE launch of the exact decoder
// takes all of them.
__global__ void gather_retries(const ScanDesc* __restrict__ descs, const ScanResult* __restrict__ results, uint32_t count,
                               ScanDesc* __restrict__ retry_descs, uint32_t* __restrict__ retry_index,
                               uint32_t* __restrict__ retry_count)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count && (results[i].flags & fast::kFastRetry) != 0)
    {
        const uint32_t slot = atomicAdd(retry_count, 1u);
        retry_index[slot] = i;
        retry_descs[slot] = descs[i];
    }
}

__global__ void scatter_retries(const ScanResult* __restrict__ retry_results, const uint32_t* __restrict__ retry_index,
                                uint32_t retries, ScanResult* __restrict__ results)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < retries)
        results[retry_index[s]] = retry_results[s];
}

// The exact decoder (scan_wave_decode.hip): NC co-sited components of a sample-interleaved scan, one otherwise.
void launch_wave_decode(const ScanDesc& proto, const ScanDesc* d_descs, ScanResult* d_results, uint32_t count, hipStream_t stream)
{
    const int nc = proto.interleave_mode == 2 ? proto.components : 1;
    dispatch_sample(proto.bits_per_sample, [&](auto s) {
        dispatch_int<1, 2, 3, 4>(nc, [&](auto n) {
            launch_kernel(decode_scans_wave<typename decltype(s)::type, decltype(n)::value>, dim3(count), dim3(64), wave_decode_lds(proto),
                          stream, d_descs, d_results);
        });
    });
}

// The group decoder (scan_group_decode.hip) in the shape of `plan`; a shape that is not built is an error, not another kernel.
void launch_group_decode(const ScanDesc& proto, GroupPlan plan, const ScanDesc* d_descs, ScanResult* d_results, uint32_t count,
                         hipStream_t stream)
{
    const uint32_t per_group = 64u / static_cast<uint32_t>(plan.lanes) * static_cast<uint32_t>(plan.waves);
    const dim3 grid((count + per_group - 1) / per_group);
    // (a workgroup of several wavefronts is to have its CU to itself -- one wavefront per SIMD: it asks for more than half
    // of the CU's LDS whatever its scans need)
    const size_t lds = plan.waves > 1 ? std::max<size_t>(group_lds_bytes(proto, per_group), kGroupDecodeLds / 2 + 1024)
                                      : group_lds_bytes(proto, per_group);
    dispatch_sample(proto.bits_per_sample, [&](auto s) {
        using S = typename decltype(s)::type;
        dispatch_bool(proto.near_lossless != 0, [&](auto k) {
            constexpr bool kNear = decltype(k)::value;
            dispatch_int<4, 8, 16, 32>(plan.lanes, [&](auto g) {
                constexpr int G = decltype(g)::value;
                dispatch_int<1, 2, 3, 4>(static_cast<int>(group_lines(proto)), [&](auto n) {
                    constexpr int NL = decltype(n)::value;
                    dispatch_int<4, 8, 1>(plan.waves, [&](auto w) {
                        constexpr int W = decltype(w)::value;
                        if constexpr (group_decode_built(G, NL, W, kNear))
                            launch_kernel(decode_scans_group<S, G, NL, W, kNear>, grid, dim3(64 * W), lds, stream, d_descs, d_results,
                                          count);
                        else
                            raise(CHARLS_JPEGLS_ERRC_INVALID_OPERATION);
                    });
                });
            });
        });
    });
}
} // namespace

bool seek_decode_eligible(const ScanDesc& d) noexcept
{
    return d.restart_interval == 0 && wave_decode_eligible(d);
}

namespace {
uint64_t interval_launch_key(const ScanDesc& d, uint64_t base) noexcept;
}

uint64_t decode_launch_key(const ScanDesc& d) noexcept
{
    // width | components | interleave | near-lossless | eligible | wide | exact-eligible : scans with equal keys can share a
    // launch.  The launch picks its kernel from its first scan: a near-lossless scan must not land behind a lossless one (a
    // 16-bit lossless scan with T3 beyond the group kernel's table takes decode_scans_fast, which has no near-lossless code)
    const uint64_t base = (static_cast<uint64_t>(d.width) << 16) | (static_cast<uint64_t>(d.components & 0xFF) << 8) |
                          (static_cast<uint64_t>(d.interleave_mode & 3) << 4) | (d.near_lossless != 0 ? 8u : 0u) |
                          (fast_decode_eligible(d) || pixel_group_lanes(d, 1) != 0 ? 4u : 0u) |
                          (d.bits_per_sample > 8 ? 2u : 0u) | (wave_decode_eligible(d) ? 1u : 0u);
    if (!interval_decode_candidate(d))
        return base;
    return interval_launch_key(d, base);
}

bool salvage_candidate(const ScanDesc& d) noexcept
{
    return intervals_decodable(d);
}

uint64_t salvage_launch_key(const ScanDesc& d) noexcept
{
    ScanDesc plain = d;
    plain.restart_interval = 0; // (the key of the interval scans' own launch, whatever SEQUENTIAL_INTERVALS says)
    return interval_launch_key(d, decode_launch_key(plain));
}

namespace {
uint64_t interval_launch_key(const ScanDesc& d, uint64_t base) noexcept
{
    // interval-parallel decode also needs equal height and restart interval (both < 2^16 here, as is the width)
    return (uint64_t{1} << 63) | (static_cast<uint64_t>(d.restart_interval) << 47) | (static_cast<uint64_t>(d.height) << 31) |
           (static_cast<uint64_t>(d.width & 0xFFFF) << 15) | (static_cast<uint64_t>(d.components & 7) << 12) |
           (static_cast<uint64_t>(d.interleave_mode & 3) << 10) | (base & 15u);
}
} // namespace

namespace {
void launch_decode_plain(const ScanDesc& proto, const ScanDesc* d_descs, ScanResult* d_results, uint32_t count,
                         hipStream_t stream);

// All `count` scans share proto's geometry and restart interval.
void launch_decode_intervals(const ScanDesc& proto, const ScanDesc* d_descs, ScanResult* d_results, uint32_t count,
                             hipStream_t stream)
{
    const uint32_t lines = proto.restart_interval;
    const uint32_t intervals = (proto.height + lines - 1) / lines;
    const uint32_t max_marks = intervals - 1;
    const size_t subs_n = static_cast<size_t>(count) * intervals;
    auto* d_marks = static_cast<uint32_t*>(work_buffer(WorkBuffer::marks).ensure(sizeof(uint32_t) * count * max_marks));
    auto* d_counts = static_cast<uint32_t*>(work_buffer(WorkBuffer::counts).ensure(sizeof(uint32_t) * count));
    auto* d_subs = static_cast<ScanDesc*>(work_buffer(WorkBuffer::interval_scans).ensure(sizeof(ScanDesc) * subs_n));
    auto* d_sub_results = static_cast<ScanResult*>(work_buffer(WorkBuffer::interval_results).ensure(sizeof(ScanResult) * subs_n));
    hipLaunchKernelGGL(interval::find_restart_markers, dim3(count), dim3(64), 0, stream, d_descs, d_marks, max_marks, d_counts);
    hip_check(hipGetLastError());
    std::vector<uint32_t> counts(count);
    hip_check(hipMemcpyAsync(counts.data(), d_counts, sizeof(uint32_t) * count, hipMemcpyDeviceToHost, stream));
    hip_check(hipStreamSynchronize(stream));
    bool regular = true;
    for (uint32_t c : counts)
        regular = regular && c == max_marks;
    if (!regular)
    { // a stream without the expected markers: the sequential decoder reports what the reference reports
        launch_decode_plain(proto, d_descs, d_results, count, stream);
        return;
    }
    hipLaunchKernelGGL(interval::build_decode_intervals, dim3(intervals, count), dim3(1), 0, stream, d_descs, d_marks, intervals,
                       d_subs);
    hip_check(hipGetLastError());
    ScanDesc sub_proto = proto;
    sub_proto.height = lines;
    sub_proto.restart_interval = 0;
    launch_decode_plain(sub_proto, d_subs, d_sub_results, static_cast<uint32_t>(subs_n), stream);
    hipLaunchKernelGGL(interval::check_intervals, dim3((count + 63) / 64), dim3(64), 0, stream, d_descs, d_marks, intervals,
                       d_sub_results, d_results, count);
    hip_check(hipGetLastError());
    std::vector<ScanResult> results(count);
    hip_check(hipMemcpyAsync(results.data(), d_results, sizeof(ScanResult) * count, hipMemcpyDeviceToHost, stream));
    hip_check(hipStreamSynchronize(stream));
    for (uint32_t i = 0; i < count; ++i)
        if ((results[i].flags & interval::kIntervalRetry) != 0)
            launch_decode_plain(proto, d_descs + i, d_results + i, 1, stream);
}
} // namespace

void launch_find_restart_markers(const ScanDesc* d_descs, uint32_t* d_marks, uint32_t max_marks, uint32_t* d_counts, uint32_t count,
                                 hipStream_t stream)
{
    if (count == 0)
        return;
    hipLaunchKernelGGL(interval::find_restart_markers, dim3(count), dim3(64), 0, stream, d_descs, d_marks, max_marks, d_counts);
    hip_check(hipGetLastError());
}

// All `count` scans share proto's geometry and restart interval (salvage_launch_key).  The intervals of every scan are found
// by their markers as far as these can be trusted, decoded as scans of their own by the ordinary decoders -- the exact decoder's
// one launch settles what the speed path leaves undecided -- and judged; the rows of the intervals that are not kept are filled.
void launch_decode_salvage(const ScanDesc& proto, const ScanDesc* d_descs, uint32_t count, const SalvageOutputs& outputs,
                           hipStream_t stream)
{
    if (count == 0)
        return;
    const uint32_t lines = proto.restart_interval;
    const uint32_t intervals = (proto.height + lines - 1) / lines;
    const uint32_t max_marks = intervals + 7;
    const size_t subs_n = static_cast<size_t>(count) * intervals;
    auto* d_marks = static_cast<uint32_t*>(work_buffer(WorkBuffer::salvage_marks).ensure(with_headroom(sizeof(uint32_t) * count * max_marks)));
    auto* d_segments = static_cast<salvage::Segment*>(work_buffer(WorkBuffer::salvage_segments).ensure(with_headroom(sizeof(salvage::Segment) * count)));
    auto* d_subs = static_cast<ScanDesc*>(work_buffer(WorkBuffer::salvage_scans).ensure(with_headroom(sizeof(ScanDesc) * subs_n)));
    auto* d_sub_results = static_cast<ScanResult*>(work_buffer(WorkBuffer::salvage_results).ensure(with_headroom(sizeof(ScanResult) * subs_n)));
    auto* d_expect = static_cast<uint64_t*>(work_buffer(WorkBuffer::salvage_lengths).ensure(with_headroom(sizeof(uint64_t) * subs_n)));
    auto* d_status = static_cast<uint8_t*>(work_buffer(WorkBuffer::salvage_status).ensure(with_headroom(subs_n)));
    auto* d_counts = static_cast<uint32_t*>(work_buffer(WorkBuffer::salvage_counts).ensure(with_headroom(sizeof(uint32_t) * 2 * count)));
    hipLaunchKernelGGL(salvage::find_salvage_markers, dim3(count), dim3(64), 0, stream, d_descs, d_marks, max_marks, d_segments);
    hip_check(hipGetLastError());
    hipLaunchKernelGGL(salvage::plan_salvage, dim3(count), dim3(64), 0, stream, d_descs, static_cast<const uint32_t*>(d_marks), max_marks,
                       static_cast<const salvage::Segment*>(d_segments), intervals, d_subs, d_expect, d_status, d_counts);
    hip_check(hipGetLastError());
    ScanDesc sub_proto = proto;
    sub_proto.height = lines;
    sub_proto.restart_interval = 0;
    launch_decode_plain(sub_proto, d_subs, d_sub_results, static_cast<uint32_t>(subs_n), stream);
    const uint64_t row_bytes = static_cast<uint64_t>(proto.width) * (proto.interleave_mode == 0 ? 1 : proto.components) *
                               (proto.bits_per_sample > 8 ? 2 : 1);
    for (uint32_t first = 0; first < count; first += 65535u) // (a grid has at most 65535 rows)
    {
        const size_t at = static_cast<size_t>(first) * intervals;
        hipLaunchKernelGGL(salvage::judge_and_fill, dim3(intervals, std::min(count - first, 65535u)), dim3(salvage::kFillThreads), 0, stream,
                           d_descs + first, intervals, static_cast<const ScanResult*>(d_sub_results + at),
                           static_cast<const uint64_t*>(d_expect + at), d_status + at, outputs.fill_value,
                           proto.bits_per_sample > 8 ? 1u : 0u, row_bytes);
        hip_check(hipGetLastError());
    }
    g_salvage_launches.fetch_add(3);
    std::vector<salvage::Segment> segments(count);
    hip_check(hipMemcpyAsync(outputs.status, d_status, subs_n, hipMemcpyDeviceToHost, stream));
    hip_check(hipMemcpyAsync(segments.data(), d_segments, sizeof(salvage::Segment) * count, hipMemcpyDeviceToHost, stream));
    hip_check(hipStreamSynchronize(stream));
    for (uint32_t i = 0; i < count; ++i)
        outputs.segment_ends[i] = segments[i].end;
}

static_assert(kSalvageByIndex == salvage::kByIndex && kSalvageByPrefix == salvage::kByPrefix &&
              kSalvageEndsInNextPoint == salvage::kEndsInNextPoint);

void launch_salvage_fill(const ScanDesc& proto, const ScanDesc* d_parents, uint32_t count, uint32_t intervals,
                         const ScanResult* d_results, const uint64_t* d_expect, uint8_t* d_status, uint32_t fill_value, uint32_t rule,
                         hipStream_t stream)
{
    if (count == 0 || intervals == 0)
        return;
    if ((rule != kSalvageByIndex && rule != kSalvageByPrefix) || intervals > 0x7FFFFFFFu)
        raise(CHARLS_JPEGLS_ERRC_INVALID_OPERATION);
    const uint64_t row_bytes = static_cast<uint64_t>(proto.width) * (proto.interleave_mode == 0 ? 1 : proto.components) *
                               (proto.bits_per_sample > 8 ? 2 : 1);
    for (uint32_t first = 0; first < count; first += 65535u) // (a grid has at most 65535 rows)
    {
        const size_t at = static_cast<size_t>(first) * intervals;
        hipLaunchKernelGGL(salvage::judge_and_fill, dim3(intervals, std::min(count - first, 65535u)), dim3(salvage::kFillThreads), 0, stream,
                           d_parents + first, intervals, d_results + at, d_expect + at, d_status + at, fill_value,
                           (proto.bits_per_sample > 8 ? salvage::kWideSamples : 0u) | rule, row_bytes);
        hip_check(hipGetLastError());
    }
}

void launch_decode(const ScanDesc& proto, const ScanDesc* d_descs, ScanResult* d_results, uint32_t count,
                   hipStream_t stream)
{
    if (count == 0)
        return;
    if (interval_decode_candidate(proto))
        launch_decode_intervals(proto, d_descs, d_results, count, stream);
    else
        launch_decode_plain(proto, d_descs, d_results, count, stream);
}

namespace {
void launch_decode_plain(const ScanDesc& proto, const ScanDesc* d_descs, ScanResult* d_results, uint32_t count,
                         hipStream_t stream)
{
    if (count == 0)
        return;
    if (!wave_decode_eligible(proto))
    {
        launch_decode_serial(d_descs, d_results, count, stream);
        return;
    }
    auto exact = [&](const ScanDesc* descs, ScanResult* results, uint32_t n) { launch_wave_decode(proto, descs, results, n, stream); };
    const int pixel_lanes = pixel_group_lanes(proto, count);
    if (pixel_lanes != 0)
    { // sample-interleaved scans, lossless or near-lossless
        launch_decode_pixels(proto, pixel_lanes, d_descs, d_results, count, stream);
    }
    else if (!fast_decode_eligible(proto))
    {
        exact(d_descs, d_results, count);
        return;
    }
    else
    {
        const GroupPlan plan = decode_group_plan(proto, count);
        if (plan.lanes == 0)
            dispatch_sample(proto.bits_per_sample, [&](auto s) {
                launch_kernel(decode_scans_fast<typename decltype(s)::type>, dim3(count), dim3(64), fast_decode_lds(proto), stream, d_descs,
                              d_results);
            });
        else
            launch_group_decode(proto, plan, d_descs, d_results, count, stream);
    }
    // scans that did not end cleanly are decided by the exact decoder (error codes and byte counts of the reference):
    // they are gathered on the device and decoded by one launch
    auto* d_retry_count = static_cast<uint32_t*>(work_buffer(WorkBuffer::retry_count).ensure(sizeof(uint32_t)));
    hip_check(hipMemsetAsync(d_retry_count, 0, sizeof(uint32_t), stream));
    auto* d_retry_index = static_cast<uint32_t*>(work_buffer(WorkBuffer::retry_index).ensure(with_headroom(sizeof(uint32_t) * count)));
    auto* d_retry_descs = static_cast<ScanDesc*>(work_buffer(WorkBuffer::retry_descs).ensure(with_headroom(sizeof(ScanDesc) * count)));
    hipLaunchKernelGGL(gather_retries, dim3((count + 255) / 256), dim3(256), 0, stream, d_descs,
                       static_cast<const ScanResult*>(d_results), count, d_retry_descs, d_retry_index, d_retry_count);
    hip_check(hipGetLastError());
    uint32_t retries = 0;
    hip_check(hipMemcpyAsync(&retries, d_retry_count, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    hip_check(hipStreamSynchronize(stream));
    if (retries == 0)
        return;
    g_exact_retry_scans.fetch_add(retries); // (charls_amd_engine_counters [9]: a valid stream that lands here is a lost speed path)
    auto* d_retry_results = static_cast<ScanResult*>(work_buffer(WorkBuffer::retry_results).ensure(with_headroom(sizeof(ScanResult) * retries)));
    exact(d_retry_descs, d_retry_results, retries);
    hipLaunchKernelGGL(scatter_retries, dim3((retries + 255) / 256), dim3(256), 0, stream,
                       static_cast<const ScanResult*>(d_retry_results), static_cast<const uint32_t*>(d_retry_index), retries,
                       d_results);
    hip_check(hipGetLastError());
}
} // namespace

} // namespace jls::dev
