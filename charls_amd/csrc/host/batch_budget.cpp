// batch_budget.cpp -- the batch API to a BYTE BUDGET (charls_amd.h part 2f): JPEG-LS has no rate control, so the size of a
// frame at some NEAR is only known once its chain has been walked.  Here the chains of all candidates of all frames are
// walked in ONE launch of the measuring form of the group encoder (device/scan_group_encode.hip, kMeasure), which writes no
// stream: frames x scans x candidates results of 16 bytes instead of that many stream slots.
//
//  * charls_amd_measure_batch_device reports the size of every frame's .jls at every candidate.
//  * charls_amd_encode_batch_device_budget picks every frame's first candidate within its budget and codes the chosen
//    (frame, NEAR) pairs with charls_amd_encode_batch_device_ragged, which groups the frames that chose the same NEAR and
//    packs in the caller's order.
//  * Scans the group encoder does not take are sized by coding them for real with the slot encoder into staging.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "../device/runtime.h"
#include "batch_streams.h"
#include "common.h"

using namespace jls;
using dev::hip_check;

namespace {

constexpr uint32_t kMaxCandidates = 64;
constexpr uint64_t kNoSize = ~uint64_t{0}; // a (frame, candidate) that was not sized, or whose coding failed

std::atomic<uint64_t> g_measured_scans{0}, g_measure_launches{0}, g_coded_scans{0};

// The distinct candidates in the order of their first appearance, each with what the encoder derives for it.
struct Candidates
{
    std::vector<int32_t> nears;       // distinct
    std::vector<EncodePlan> plans;    // of nears[u]
    std::vector<uint32_t> which;      // candidate c of the caller is nears[which[c]]
};

// The whole-call checks of both entry points that need no device; raises the first refused candidate's code.
Candidates check_candidates(const charls_amd_codec_params& params, size_t frame_pitch_bytes, uint32_t stride,
                            const int32_t* near_candidates, uint32_t candidate_count)
{
    check_pointer(near_candidates);
    check_argument(candidate_count >= 1 && candidate_count <= kMaxCandidates);
    Candidates c;
    for (uint32_t k = 0; k < candidate_count; ++k)
    {
        const auto seen = std::find(c.nears.begin(), c.nears.end(), near_candidates[k]);
        c.which.push_back(static_cast<uint32_t>(seen - c.nears.begin()));
        if (seen != c.nears.end())
            continue;
        charls_amd_codec_params p = params;
        p.near_lossless = near_candidates[k];
        c.plans.push_back(plan_encode(p, frame_pitch_bytes, stride));
        c.nears.push_back(near_candidates[k]);
    }
    return c;
}

uint64_t file_bytes(const charls_amd_codec_params& params, uint64_t container_and_segments)
{
    const uint64_t padded = container_and_segments + ((params.encoding_options & 1u) != 0 ? container_and_segments & 1u : 0u);
    return padded + 2; // EOI
}

// sized[f * U + u] = the bytes of frame f's complete .jls at c.nears[u] (U = c.nears.size()), kNoSize where coding the frame
// fails.  With `budgets` (the budget call) the fallback stops at every frame's first candidate -- in the caller's order --
// that fits, and leaves kNoSize behind it.
void size_frames(const charls_amd_codec_params& params, uint32_t frame_count, const uint8_t* frames, size_t frame_pitch_bytes,
                 uint32_t stride, const Candidates& c, const std::vector<uint32_t>& order, const uint64_t* budgets,
                 std::vector<uint64_t>& sized, void* hip_stream)
{
    auto stream = static_cast<hipStream_t>(hip_stream);
    const uint32_t distinct = static_cast<uint32_t>(c.nears.size());
    const uint32_t scans = c.plans[0].scans;
    const uint64_t total = static_cast<uint64_t>(frame_count) * scans * distinct;
    sized.assign(static_cast<size_t>(frame_count) * distinct, kNoSize);
    std::vector<uint8_t> measured(sized.size(), 0);

    // ---- the measuring kernel: candidate-major, so that the scans of a wavefront share NEAR except at the seams
    if (total <= UINT32_MAX)
    {
        std::vector<ScanDesc> descs(total);
        size_t at = 0;
        for (uint32_t u = 0; u < distinct; ++u)
            for (uint32_t f = 0; f < frame_count; ++f)
                for (uint32_t r = 0; r < scans; ++r)
                {
                    ScanDesc d = c.plans[u].scan;
                    d.pixels = const_cast<uint8_t*>(frames) + static_cast<size_t>(f) * frame_pitch_bytes +
                               static_cast<size_t>(r) * c.plans[u].stride * d.height;
                    descs[at++] = d;
                }
        dev::DeviceBuffer d_descs, d_results;
        d_descs.ensure(sizeof(ScanDesc) * descs.size());
        d_results.ensure(sizeof(ScanResult) * descs.size());
        hip_check(hipMemcpyAsync(d_descs.as<ScanDesc>(), descs.data(), sizeof(ScanDesc) * descs.size(), hipMemcpyHostToDevice, stream));
        if (dev::launch_measure(descs[0], d_descs.as<ScanDesc>(), d_results.as<ScanResult>(), static_cast<uint32_t>(total), stream))
        {
            std::vector<ScanResult> results(descs.size());
            hip_check(hipMemcpyAsync(results.data(), d_results.as<ScanResult>(), sizeof(ScanResult) * results.size(),
                                     hipMemcpyDeviceToHost, stream));
            hip_check(hipStreamSynchronize(stream));
            g_measured_scans += total;
            ++g_measure_launches;
            at = 0;
            for (uint32_t u = 0; u < distinct; ++u)
                for (uint32_t f = 0; f < frame_count; ++f)
                {
                    uint64_t bytes = c.plans[u].container_bytes;
                    bool ok = true;
                    for (uint32_t r = 0; r < scans; ++r, ++at)
                    {
                        ok = ok && results[at].errc == kOk;
                        bytes += results[at].bytes;
                    }
                    // (a chain the kernel gave up on -- a code no stream can hold -- is coded below for its verdict)
                    measured[static_cast<size_t>(f) * distinct + u] = ok;
                    if (ok)
                        sized[static_cast<size_t>(f) * distinct + u] = file_bytes(params, bytes);
                }
        }
        else
            hip_check(hipStreamSynchronize(stream)); // (descs goes away)
    }

    // ---- what is left: coded for real by the slot encoder into staging, candidate by candidate in the caller's order
    std::vector<uint8_t> settled(frame_count, 0); // budget call: the frame has its first fitting candidate
    std::vector<uint32_t> todo;
    std::vector<const uint8_t*> pixels;
    std::vector<uint64_t> sizes;
    std::vector<charls_jpegls_errc> errcs;
    for (const uint32_t u : order)
    {
        todo.clear();
        for (uint32_t f = 0; f < frame_count; ++f)
        {
            const size_t k = static_cast<size_t>(f) * distinct + u;
            if (!settled[f] && !measured[k])
                todo.push_back(f);
            else if (budgets != nullptr && !settled[f] && sized[k] != kNoSize && sized[k] <= budgets[f])
                settled[f] = 1;
        }
        if (todo.empty())
            continue;
        charls_amd_codec_params p = params;
        p.near_lossless = c.nears[u];
        const size_t slot = estimated_stream_bytes(p);
        const size_t budget = dev::work_area_budget();
        if (dev::workspace_limit() != 0 && budget < slot)
            raise(CHARLS_JPEGLS_ERRC_NOT_ENOUGH_MEMORY);
        uint32_t pass = static_cast<uint32_t>(std::min<size_t>(todo.size(), std::max<size_t>(1, budget / 4 / slot)));
        uint8_t* staging = nullptr;
        while ((staging = static_cast<uint8_t*>(dev::try_ensure(dev::pack_arena(), checked_mul(slot, pass) + 16))) == nullptr && pass > 1)
            pass = (pass + 1) / 2;
        if (staging == nullptr)
            raise(CHARLS_JPEGLS_ERRC_NOT_ENOUGH_MEMORY);
        for (size_t first = 0; first < todo.size(); first += pass)
        {
            const uint32_t n = static_cast<uint32_t>(std::min<size_t>(pass, todo.size() - first));
            pixels.resize(n);
            sizes.assign(n, 0);
            errcs.assign(n, CHARLS_JPEGLS_ERRC_SUCCESS);
            for (uint32_t i = 0; i < n; ++i)
                pixels[i] = frames + static_cast<size_t>(todo[first + i]) * frame_pitch_bytes;
            encode_batch_frames(p, n, pixels.data(), frame_pitch_bytes, stride, staging, slot, sizes.data(), errcs.data(), hip_stream);
            g_coded_scans += static_cast<uint64_t>(n) * scans;
            for (uint32_t i = 0; i < n; ++i)
            {
                const uint32_t f = todo[first + i];
                if (errcs[i] != CHARLS_JPEGLS_ERRC_SUCCESS)
                    continue;
                sized[static_cast<size_t>(f) * distinct + u] = sizes[i];
                if (budgets != nullptr && sizes[i] <= budgets[f])
                    settled[f] = 1;
            }
        }
    }
}

// The distinct candidates in the caller's order of preference.
std::vector<uint32_t> preference(const Candidates& c)
{
    std::vector<uint32_t> order;
    for (const uint32_t u : c.which)
        if (std::find(order.begin(), order.end(), u) == order.end())
            order.push_back(u);
    return order;
}

} // namespace

extern "C" charls_jpegls_errc charls_amd_measure_batch_device(const charls_amd_codec_params* params, uint32_t frame_count,
                                                              const void* d_frames, size_t frame_pitch_bytes, uint32_t stride,
                                                              const int32_t* near_candidates, uint32_t candidate_count,
                                                              uint64_t* sizes_out, void* hip_stream)
try
{
    check_pointer(params);
    check_pointer(sizes_out);
    const Candidates c = check_candidates(*params, frame_count == 0 ? SIZE_MAX : frame_pitch_bytes, stride, near_candidates, candidate_count);
    if (frame_count == 0)
        return CHARLS_JPEGLS_ERRC_SUCCESS;
    check_pointer(d_frames);
    dev::require_device();
    std::vector<uint64_t> sized;
    size_frames(*params, frame_count, static_cast<const uint8_t*>(d_frames), frame_pitch_bytes, stride, c, preference(c), nullptr, sized,
                hip_stream);
    const size_t distinct = c.nears.size();
    for (uint32_t f = 0; f < frame_count; ++f)
        for (uint32_t k = 0; k < candidate_count; ++k)
        {
            const uint64_t v = sized[f * distinct + c.which[k]];
            sizes_out[static_cast<size_t>(f) * candidate_count + k] = v == kNoSize ? 0 : v;
        }
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}

extern "C" charls_jpegls_errc charls_amd_encode_batch_device_budget(const charls_amd_codec_params* params, uint32_t frame_count,
                                                                    const void* d_frames, size_t frame_pitch_bytes, uint32_t stride,
                                                                    const uint64_t* budgets, const int32_t* near_candidates,
                                                                    uint32_t candidate_count, void* d_packed,
                                                                    size_t packed_capacity_bytes, uint32_t offset_alignment,
                                                                    uint64_t* offsets, uint64_t* sizes, int32_t* near_out,
                                                                    charls_jpegls_errc* errcs, void* hip_stream)
try
{
    check_pointer(params);
    check_pointer(budgets);
    check_pointer(offsets);
    check_pointer(sizes);
    check_pointer(near_out);
    check_pointer(errcs);
    check_offset_alignment(offset_alignment);
    const Candidates c = check_candidates(*params, frame_count == 0 ? SIZE_MAX : frame_pitch_bytes, stride, near_candidates, candidate_count);
    if (frame_count == 0)
    {
        offsets[0] = 0;
        return CHARLS_JPEGLS_ERRC_SUCCESS;
    }
    check_pointer(d_frames);
    check_pointer(d_packed);
    dev::require_device();
    const auto* frames = static_cast<const uint8_t*>(d_frames);
    const std::vector<uint32_t> order = preference(c);
    const size_t distinct = c.nears.size();

    std::vector<uint64_t> sized;
    size_frames(*params, frame_count, frames, frame_pitch_bytes, stride, c, order, budgets, sized, hip_stream);

    // ---- every frame's first candidate within its budget; the largest stream of every NEAR sizes that NEAR's staging slots
    constexpr uint32_t kNone = ~0u;
    std::vector<uint32_t> chosen(frame_count, kNone);
    std::vector<uint64_t> largest(distinct, 0);
    uint32_t coded = 0;
    for (uint32_t f = 0; f < frame_count; ++f)
        for (const uint32_t u : order)
            if (sized[f * distinct + u] != kNoSize && sized[f * distinct + u] <= budgets[f])
            {
                chosen[f] = u;
                largest[u] = std::max(largest[u], sized[f * distinct + u]);
                ++coded;
                break;
            }

    // ---- the chosen (frame, NEAR) pairs as a ragged batch: frames of one NEAR are one group there, and the pack is in the
    // caller's order.  The slots hold the largest stream and what the writer's flush rule wants spare behind it (it asks for
    // four free bytes whenever it flushes; the planar path codes a frame again whose scan ends within four bytes of its slot).
    std::vector<charls_amd_frame_source> sources;
    sources.reserve(coded);
    for (uint32_t f = 0; f < frame_count; ++f)
    {
        if (chosen[f] == kNone)
            continue;
        charls_amd_frame_source s{};
        s.params = *params;
        s.params.near_lossless = c.nears[chosen[f]];
        s.d_pixels = frames + static_cast<size_t>(f) * frame_pitch_bytes;
        s.stride = stride;
        s.max_stream_bytes = (largest[chosen[f]] + 64 + 255) & ~uint64_t{255};
        sources.push_back(s);
    }
    std::vector<uint64_t> coded_offsets(static_cast<size_t>(coded) + 1, 0), coded_sizes(coded, 0);
    std::vector<charls_jpegls_errc> coded_errcs(coded, CHARLS_JPEGLS_ERRC_SUCCESS);
    if (coded != 0)
    {
        const charls_jpegls_errc rc = charls_amd_encode_batch_device_ragged(coded, sources.data(), d_packed, packed_capacity_bytes,
                                                                            offset_alignment, coded_offsets.data(), coded_sizes.data(),
                                                                            coded_errcs.data(), hip_stream);
        if (rc != CHARLS_JPEGLS_ERRC_SUCCESS)
            return rc;
    }
    // ---- back to the caller's frames: a frame without a candidate takes no room at the offset of the frame after it
    for (uint32_t f = 0, k = 0; f < frame_count; ++f)
    {
        offsets[f] = coded_offsets[k];
        if (chosen[f] == kNone)
        {
            sizes[f] = 0;
            near_out[f] = -1;
            errcs[f] = CHARLS_JPEGLS_ERRC_DESTINATION_TOO_SMALL;
            continue;
        }
        sizes[f] = coded_sizes[k];
        errcs[f] = coded_errcs[k];
        near_out[f] = coded_errcs[k] == CHARLS_JPEGLS_ERRC_SUCCESS ? c.nears[chosen[f]] : -1;
        ++k;
    }
    offsets[frame_count] = coded_offsets[coded];
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}

extern "C" int32_t charls_amd_measure_counters(uint64_t* out, int32_t capacity)
{
    const uint64_t v[3] = {g_measured_scans.load(), g_measure_launches.load(), g_coded_scans.load()};
    int32_t n = 0;
    for (; out != nullptr && n < capacity && n < 3; ++n)
        out[n] = v[n];
    return n;
}
