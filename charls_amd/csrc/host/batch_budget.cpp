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
//  * Part 2k: the same on RAGGED frames (charls_amd_measure_batch_device_ragged, charls_amd_encode_batch_device_ragged_budget)
//    and as the encode step of a re-coding window (transcode_encode_budget; batch_transcode.cpp, batch_host.cpp).  The frames
//    of a call with equal params -- NEAR aside -- and stride are a GROUP, sized by what one uniform call over them does.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../device/runtime.h"
#include "batch_streams.h"
#include "common.h"
#include "event_timer.h"

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

void check_candidate_list(const int32_t* near_candidates, uint32_t candidate_count)
{
    check_pointer(near_candidates);
    check_argument(candidate_count >= 1 && candidate_count <= kMaxCandidates);
}

// The whole-call checks of the uniform entry points that need no device -- a group's own checks in the ragged ones --;
// raises the first refused candidate's code.
Candidates check_candidates(const charls_amd_codec_params& params, size_t frame_pitch_bytes, uint32_t stride,
                            const int32_t* near_candidates, uint32_t candidate_count)
{
    check_candidate_list(near_candidates, candidate_count);
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
// that fits, and leaves kNoSize behind it.  frames[f] is frame f's first row (HOST array of DEVICE pointers, as
// encode_batch_frames takes it), `frame_bytes` what every frame offers from there on.  Adds the GPU time of the sizing to
// ms[0] and that of its dominant kernels to ms[1].
void size_frames(const charls_amd_codec_params& params, uint32_t frame_count, const uint8_t* const* frames, size_t frame_bytes,
                 uint32_t stride, const Candidates& c, const std::vector<uint32_t>& order, const uint64_t* budgets,
                 std::vector<uint64_t>& sized, double ms[2], void* hip_stream)
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
                    d.pixels = const_cast<uint8_t*>(frames[f]) + static_cast<size_t>(r) * c.plans[u].stride * d.height;
                    descs[at++] = d;
                }
        dev::DeviceBuffer d_descs, d_results;
        d_descs.ensure(sizeof(ScanDesc) * descs.size());
        d_results.ensure(sizeof(ScanResult) * descs.size());
        hip_check(hipMemcpyAsync(d_descs.as<ScanDesc>(), descs.data(), sizeof(ScanDesc) * descs.size(), hipMemcpyHostToDevice, stream));
        EventTimer timer(stream, true);
        timer.start();
        if (dev::launch_measure(descs[0], d_descs.as<ScanDesc>(), d_results.as<ScanResult>(), static_cast<uint32_t>(total), stream))
        {
            timer.stop();
            std::vector<ScanResult> results(descs.size());
            hip_check(hipMemcpyAsync(results.data(), d_results.as<ScanResult>(), sizeof(ScanResult) * results.size(),
                                     hipMemcpyDeviceToHost, stream));
            hip_check(hipStreamSynchronize(stream));
            const double launch_ms = timer.ms();
            ms[0] += launch_ms;
            ms[1] += launch_ms;
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
                pixels[i] = frames[todo[first + i]];
            encode_batch_frames(p, n, pixels.data(), frame_bytes, stride, staging, slot, sizes.data(), errcs.data(), hip_stream);
            const dev::Timings& t = dev::last_timings();
            ms[0] += t.count > 0 ? t.values[0] : 0;
            ms[1] += t.count > 1 ? t.values[1] : 0;
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

// ---- ragged frames (part 2k): the frames of a call that the uniform calls would take as ONE batch -- equal params, NEAR
// aside, and equal stride -- in any positions of the caller's order
struct SizedGroup
{
    charls_amd_codec_params params; // near_lossless is 0 here: the candidates decide it
    uint32_t stride;
    std::vector<uint32_t> frames;   // in the caller's order
    charls_jpegls_errc errc;        // what the uniform calls return for these parameters with these candidates, device aside
    Candidates c;
    std::vector<uint32_t> order;    // preference(c)
    std::vector<uint64_t> sized;    // [place in `frames` * c.nears.size() + u], as size_frames leaves it
};

bool in_group(const SizedGroup& g, const charls_amd_frame_source& s)
{
    charls_amd_codec_params p = s.params;
    p.near_lossless = 0;
    return std::memcmp(&g.params, &p, sizeof p) == 0 && g.stride == s.stride; // (no padding: batch_ragged.cpp asserts it)
}

// Walks the frames once and sizes every group by what one uniform call over its frames does: one measuring launch for all
// its frames and candidates, the fallback of size_frames for the rest.  group_of[f] / place_of[f]: where frame f went.
// budgets: as size_frames, per frame of the call.  ms[0] / ms[1]: the GPU time of the sizing and of its dominant kernels.
std::vector<SizedGroup> size_groups(uint32_t frame_count, const charls_amd_frame_source* sources, const uint64_t* budgets,
                                    const int32_t* near_candidates, uint32_t candidate_count, std::vector<uint32_t>& group_of,
                                    std::vector<uint32_t>& place_of, double ms[2], void* hip_stream)
{
    std::vector<SizedGroup> groups;
    group_of.resize(frame_count);
    place_of.resize(frame_count);
    // (params with NEAR zeroed, then stride) -> group: a call with many geometries -- a tile grid, an archive -- stays one walk
    std::unordered_map<std::string, uint32_t> by_key;
    for (uint32_t f = 0; f < frame_count; ++f)
    {
        // (the frame before it first: a uniform batch, and runs of equal frames, cost one comparison each)
        size_t g = groups.size();
        if (f != 0 && in_group(groups[group_of[f - 1]], sources[f]))
            g = group_of[f - 1];
        else
        {
            charls_amd_codec_params p = sources[f].params;
            p.near_lossless = 0;
            std::string key(reinterpret_cast<const char*>(&p), sizeof p);
            key.append(reinterpret_cast<const char*>(&sources[f].stride), sizeof sources[f].stride);
            g = by_key.emplace(std::move(key), static_cast<uint32_t>(groups.size())).first->second;
        }
        if (g == groups.size())
        {
            groups.push_back(SizedGroup{sources[f].params, sources[f].stride, {}, CHARLS_JPEGLS_ERRC_SUCCESS, {}, {}, {}});
            groups[g].params.near_lossless = 0;
        }
        group_of[f] = static_cast<uint32_t>(g);
        place_of[f] = static_cast<uint32_t>(groups[g].frames.size());
        groups[g].frames.push_back(f);
    }
    ms[0] = ms[1] = 0;
    std::vector<const uint8_t*> pixels;
    std::vector<uint64_t> group_budgets;
    for (SizedGroup& g : groups)
    {
        try
        {
            g.c = check_candidates(g.params, SIZE_MAX, g.stride, near_candidates, candidate_count);
        }
        catch (const error& e)
        { // (the uniform call refuses these frames as a whole call: their errc, and no other frame's business)
            g.errc = e.code;
            continue;
        }
        g.order = preference(g.c);
        pixels.clear();
        group_budgets.clear();
        for (const uint32_t f : g.frames)
        {
            pixels.push_back(static_cast<const uint8_t*>(sources[f].d_pixels));
            if (budgets != nullptr)
                group_budgets.push_back(budgets[f]);
        }
        size_frames(g.params, static_cast<uint32_t>(g.frames.size()), pixels.data(), SIZE_MAX, g.stride, g.c, g.order,
                    budgets != nullptr ? group_budgets.data() : nullptr, g.sized, ms, hip_stream);
    }
    return groups;
}

// The whole-call checks on the frame table of the ragged calls.  max_stream_bytes: the budget is the limit.
void check_budget_sources(uint32_t frame_count, const charls_amd_frame_source* sources)
{
    check_pointer(sources);
    for (uint32_t f = 0; f < frame_count; ++f)
    {
        check_argument(sources[f].reserved == 0 && sources[f].max_stream_bytes == 0);
        check_pointer(sources[f].d_pixels);
    }
}

} // namespace

uint32_t jls::encode_ragged_budget_frames(uint32_t frame_count, const charls_amd_frame_source* sources, const uint64_t* budgets,
                                          const int32_t* near_candidates, uint32_t candidate_count, void* d_packed,
                                          size_t packed_capacity_bytes, uint32_t offset_alignment, uint64_t* offsets, uint64_t* sizes,
                                          int32_t* near_out, charls_jpegls_errc* errcs, void* hip_stream)
{
    std::vector<uint32_t> group_of, place_of;
    double ms[2];
    const std::vector<SizedGroup> groups =
        size_groups(frame_count, sources, budgets, near_candidates, candidate_count, group_of, place_of, ms, hip_stream);

    // ---- every frame's first candidate within its budget; the largest stream of every group and NEAR sizes the staging slots
    // of the frames of that group that chose that NEAR, which are one group of the ragged encoder then
    constexpr uint32_t kNone = ~0u;
    std::vector<uint32_t> chosen(frame_count, kNone);
    std::vector<std::vector<uint64_t>> largest(groups.size());
    for (size_t g = 0; g < groups.size(); ++g)
        largest[g].assign(groups[g].c.nears.size(), 0);
    uint32_t coded = 0;
    for (uint32_t f = 0; f < frame_count; ++f)
    {
        const SizedGroup& g = groups[group_of[f]];
        if (g.errc != CHARLS_JPEGLS_ERRC_SUCCESS)
            continue;
        const size_t distinct = g.c.nears.size();
        for (const uint32_t u : g.order)
        {
            const uint64_t bytes = g.sized[place_of[f] * distinct + u];
            if (bytes != kNoSize && bytes <= budgets[f])
            {
                chosen[f] = u;
                largest[group_of[f]][u] = std::max(largest[group_of[f]][u], bytes);
                ++coded;
                break;
            }
        }
    }

    // ---- the chosen (frame, NEAR) pairs as a ragged batch, packed in the caller's order.  The slots hold the largest stream
    // and what the writer's flush rule wants spare behind it (it asks for four free bytes whenever it flushes; the planar
    // path codes a frame again whose scan ends within four bytes of its slot).
    std::vector<charls_amd_frame_source> picked;
    picked.reserve(coded);
    for (uint32_t f = 0; f < frame_count; ++f)
    {
        if (chosen[f] == kNone)
            continue;
        charls_amd_frame_source s = sources[f];
        s.params.near_lossless = groups[group_of[f]].c.nears[chosen[f]];
        s.max_stream_bytes = (largest[group_of[f]][chosen[f]] + 64 + 255) & ~uint64_t{255};
        picked.push_back(s);
    }
    std::vector<uint64_t> coded_offsets(static_cast<size_t>(coded) + 1, 0), coded_sizes(coded, 0);
    std::vector<charls_jpegls_errc> coded_errcs(coded, CHARLS_JPEGLS_ERRC_SUCCESS);
    uint32_t beyond = coded;
    if (coded != 0)
    {
        beyond = encode_ragged_frames(coded, picked.data(), d_packed, packed_capacity_bytes, offset_alignment, coded_offsets.data(),
                                      coded_sizes.data(), coded_errcs.data(), hip_stream);
        const dev::Timings& t = dev::last_timings();
        ms[0] += t.count > 0 ? t.values[0] : 0;
        ms[1] += t.count > 1 ? t.values[1] : 0;
    }
    // ---- back to the caller's frames: a frame that was not coded takes no room at the offset of the frame after it
    uint32_t first_beyond = frame_count;
    for (uint32_t f = 0, k = 0; f < frame_count; ++f)
    {
        offsets[f] = coded_offsets[k];
        if (chosen[f] == kNone)
        {
            const SizedGroup& g = groups[group_of[f]];
            sizes[f] = 0;
            near_out[f] = -1;
            // (behind the frame that met the capacity every frame is destination_too_small, as in encode_ragged_frames)
            errcs[f] = g.errc != CHARLS_JPEGLS_ERRC_SUCCESS && first_beyond == frame_count ? g.errc : CHARLS_JPEGLS_ERRC_DESTINATION_TOO_SMALL;
            continue;
        }
        if (k == beyond)
            first_beyond = f;
        sizes[f] = coded_sizes[k];
        errcs[f] = coded_errcs[k];
        near_out[f] = coded_errcs[k] == CHARLS_JPEGLS_ERRC_SUCCESS ? picked[k].params.near_lossless : -1;
        ++k;
    }
    offsets[frame_count] = coded_offsets[coded];
    dev::Timings& t = dev::last_timings(); // charls_amd_last_timings: sizing and coding, [0] all launches, [1] their dominant kernels
    t.values[0] = ms[0];
    t.values[1] = ms[1];
    t.count = 2;
    return first_beyond;
}

TranscodeEncode jls::transcode_encode_budget(const uint64_t* budgets, const int32_t* near_candidates, uint32_t candidate_count,
                                             int32_t* near_out)
{
    return [=](uint32_t count, charls_amd_frame_source* sources, const uint32_t* sent, void* d_packed, size_t packed_capacity_bytes,
               uint32_t offset_alignment, uint64_t* offsets, uint64_t* sizes, charls_jpegls_errc* errcs, void* hip_stream) {
        std::vector<uint64_t> sent_budgets(count);
        std::vector<int32_t> nears(count, -1);
        for (uint32_t k = 0; k < count; ++k)
            sent_budgets[k] = budgets[sent[k]];
        const uint32_t beyond =
            encode_ragged_budget_frames(count, sources, sent_budgets.data(), near_candidates, candidate_count, d_packed, packed_capacity_bytes,
                                        offset_alignment, offsets, sizes, nears.data(), errcs, hip_stream);
        for (uint32_t k = 0; k < count; ++k)
        {
            near_out[sent[k]] = nears[k];
            if (nears[k] >= 0)
                sources[k].params.near_lossless = nears[k]; // (what the frame was coded with: params_out)
        }
        return beyond;
    };
}

void jls::check_budget_tables(const uint64_t* budgets, const int32_t* near_candidates, uint32_t candidate_count, const int32_t* near_out)
{
    check_pointer(budgets);
    check_pointer(near_out);
    check_candidate_list(near_candidates, candidate_count);
}

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
    std::vector<const uint8_t*> frames(frame_count);
    for (uint32_t f = 0; f < frame_count; ++f)
        frames[f] = static_cast<const uint8_t*>(d_frames) + static_cast<size_t>(f) * frame_pitch_bytes;
    std::vector<uint64_t> sized;
    double ms[2] = {0, 0};
    size_frames(*params, frame_count, frames.data(), frame_pitch_bytes, stride, c, preference(c), nullptr, sized, ms, hip_stream);
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
    (void)check_candidates(*params, frame_count == 0 ? SIZE_MAX : frame_pitch_bytes, stride, near_candidates, candidate_count);
    if (frame_count == 0)
    {
        offsets[0] = 0;
        return CHARLS_JPEGLS_ERRC_SUCCESS;
    }
    check_pointer(d_frames);
    check_pointer(d_packed);
    dev::require_device();
    // ---- the uniform batch as a ragged one of ONE group: sized by one size_frames, coded and packed by the body of part 2k
    std::vector<charls_amd_frame_source> sources(frame_count);
    for (uint32_t f = 0; f < frame_count; ++f)
    {
        sources[f] = charls_amd_frame_source{};
        sources[f].params = *params;
        sources[f].d_pixels = static_cast<const uint8_t*>(d_frames) + static_cast<size_t>(f) * frame_pitch_bytes;
        sources[f].stride = stride;
    }
    encode_ragged_budget_frames(frame_count, sources.data(), budgets, near_candidates, candidate_count, d_packed, packed_capacity_bytes,
                                offset_alignment, offsets, sizes, near_out, errcs, hip_stream);
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}

extern "C" charls_jpegls_errc charls_amd_measure_batch_device_ragged(uint32_t frame_count, const charls_amd_frame_source* sources,
                                                                     const int32_t* near_candidates, uint32_t candidate_count,
                                                                     uint64_t* sizes_out, charls_jpegls_errc* errcs, void* hip_stream)
try
{
    check_pointer(sizes_out);
    check_pointer(errcs);
    check_candidate_list(near_candidates, candidate_count);
    check_budget_sources(frame_count, sources);
    if (frame_count == 0)
        return CHARLS_JPEGLS_ERRC_SUCCESS;
    dev::require_device();
    std::vector<uint32_t> group_of, place_of;
    double ms[2];
    const std::vector<SizedGroup> groups =
        size_groups(frame_count, sources, nullptr, near_candidates, candidate_count, group_of, place_of, ms, hip_stream);
    for (uint32_t f = 0; f < frame_count; ++f)
    {
        const SizedGroup& g = groups[group_of[f]];
        errcs[f] = g.errc;
        const size_t distinct = g.c.nears.size();
        for (uint32_t k = 0; k < candidate_count; ++k)
        {
            const uint64_t v = g.errc == CHARLS_JPEGLS_ERRC_SUCCESS ? g.sized[place_of[f] * distinct + g.c.which[k]] : kNoSize;
            sizes_out[static_cast<size_t>(f) * candidate_count + k] = v == kNoSize ? 0 : v;
        }
    }
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}

extern "C" charls_jpegls_errc charls_amd_encode_batch_device_ragged_budget(
    uint32_t frame_count, const charls_amd_frame_source* sources, const uint64_t* budgets, const int32_t* near_candidates,
    uint32_t candidate_count, void* d_packed, size_t packed_capacity_bytes, uint32_t offset_alignment, uint64_t* offsets,
    uint64_t* sizes, int32_t* near_out, charls_jpegls_errc* errcs, void* hip_stream)
try
{
    check_pointer(offsets);
    check_pointer(sizes);
    check_pointer(errcs);
    check_budget_tables(budgets, near_candidates, candidate_count, near_out);
    check_offset_alignment(offset_alignment);
    check_budget_sources(frame_count, sources);
    if (frame_count == 0)
    {
        offsets[0] = 0;
        return CHARLS_JPEGLS_ERRC_SUCCESS;
    }
    check_pointer(d_packed);
    dev::require_device();
    encode_ragged_budget_frames(frame_count, sources, budgets, near_candidates, candidate_count, d_packed, packed_capacity_bytes,
                                offset_alignment, offsets, sizes, near_out, errcs, hip_stream);
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
