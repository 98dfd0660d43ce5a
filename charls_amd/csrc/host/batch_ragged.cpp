// batch_ragged.cpp -- the batch API on RAGGED frames (charls_amd.h part 2e): every frame of a call brings its own geometry,
// coding parameters and pointer; streams are in the packed form of part 2d.
//
//  * charls_amd_probe_batch_device_packed and charls_amd_decode_batch_device_ragged are the batch decoder (batch_api.cpp:
//    decode_batch_streams) without destinations -- it stops behind the headers -- and with the caller's table of them.
//  * charls_amd_encode_batch_device_ragged walks the frames in the caller's order in windows; the frames of a window that
//    share everything the encoder looks at are a group, coded by the slot encoder (batch_api.cpp: encode_batch_frames) into
//    a stretch of dev::pack_arena, and the window is packed by ONE launch in frame order.  No kernel knows the difference.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../device/knobs.h"
#include "../device/pack_streams.h"
#include "../device/runtime.h"
#include "batch_streams.h"
#include "common.h"

using namespace jls;
using dev::hip_check;

namespace {

// Frames are one group when the slot encoder is given the same arguments for them: params, stride, slot size.
bool same_group(const charls_amd_frame_source& a, const charls_amd_frame_source& b)
{
    static_assert(sizeof(charls_amd_codec_params) == 16 + 3 * 4 + 20 + 2 * 4, "charls_amd_codec_params has no padding: memcmp compares it");
    return std::memcmp(&a.params, &b.params, sizeof a.params) == 0 && a.stride == b.stride && a.max_stream_bytes == b.max_stream_bytes;
}

constexpr size_t kStretchAlignment = 256; // every group's stretch of the staging starts on one

struct Group
{
    uint32_t first;             // the frame the group's parameters are read from
    std::vector<uint32_t> frames; // in the caller's order
    size_t slot;
    size_t stretch;             // offset of the group's slots in the staging
};

} // namespace

extern "C" charls_jpegls_errc charls_amd_probe_batch_device_packed(uint32_t frame_count, const void* d_packed, const uint64_t* offsets,
                                                                   const uint64_t* sizes, charls_amd_codec_params* params_out,
                                                                   uint64_t* frame_bytes_out, charls_jpegls_errc* errcs, void* hip_stream)
try
{
    check_pointer(offsets);
    check_pointer(sizes);
    check_pointer(params_out);
    check_pointer(frame_bytes_out);
    check_pointer(errcs);
    if (frame_count == 0)
        return CHARLS_JPEGLS_ERRC_SUCCESS;
    check_pointer(d_packed);
    for (uint32_t f = 0; f < frame_count; ++f)
    {
        uint64_t end;
        if (__builtin_add_overflow(offsets[f], sizes[f], &end))
            raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_SIZE);
    }
    decode_batch_streams(frame_count, d_packed, offsets, sizes, BatchDests{nullptr, true, frame_bytes_out}, params_out, errcs, hip_stream);
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}

extern "C" charls_jpegls_errc charls_amd_decode_batch_device_ragged(uint32_t frame_count, const void* d_packed, const uint64_t* offsets,
                                                                    const uint64_t* sizes, const charls_amd_frame_dest* dests,
                                                                    charls_amd_codec_params* params_out, charls_jpegls_errc* errcs,
                                                                    void* hip_stream)
try
{
    check_pointer(offsets);
    check_pointer(sizes);
    check_pointer(dests);
    check_pointer(errcs);
    for (uint32_t f = 0; f < frame_count; ++f)
    {
        check_argument(dests[f].reserved == 0);
        check_buffer(dests[f].d_pixels, dests[f].capacity_bytes);
    }
    if (frame_count == 0)
        return CHARLS_JPEGLS_ERRC_SUCCESS;
    check_pointer(d_packed);
    for (uint32_t f = 0; f < frame_count; ++f)
    {
        uint64_t end;
        if (__builtin_add_overflow(offsets[f], sizes[f], &end))
            raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_SIZE);
    }
    dev::require_device();
    if (params_out != nullptr)
        std::fill(params_out, params_out + frame_count, charls_amd_codec_params{});
    decode_batch_streams(frame_count, d_packed, offsets, sizes, BatchDests{dests, true, nullptr}, params_out, errcs, hip_stream);
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}

extern "C" charls_jpegls_errc charls_amd_encode_batch_device_ragged(uint32_t frame_count, const charls_amd_frame_source* sources,
                                                                    void* d_packed, size_t packed_capacity_bytes,
                                                                    uint32_t offset_alignment, uint64_t* offsets, uint64_t* sizes,
                                                                    charls_jpegls_errc* errcs, void* hip_stream)
try
{
    check_pointer(sources);
    check_pointer(offsets);
    check_pointer(sizes);
    check_pointer(errcs);
    check_offset_alignment(offset_alignment);
    for (uint32_t f = 0; f < frame_count; ++f)
    {
        check_argument(sources[f].reserved == 0);
        check_pointer(sources[f].d_pixels);
    }
    if (frame_count == 0)
    {
        offsets[0] = 0;
        return CHARLS_JPEGLS_ERRC_SUCCESS;
    }
    check_pointer(d_packed);
    dev::require_device();
    encode_ragged_frames(frame_count, sources, d_packed, packed_capacity_bytes, offset_alignment, offsets, sizes, errcs, hip_stream);
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}

uint32_t jls::encode_ragged_frames(uint32_t frame_count, const charls_amd_frame_source* sources, void* d_packed, size_t packed_capacity_bytes,
                                   uint32_t offset_alignment, uint64_t* offsets, uint64_t* sizes, charls_jpegls_errc* errcs, void* hip_stream)
{
    auto stream = static_cast<hipStream_t>(hip_stream);

    // ---- every frame's own verdict and slot size.  A frame the encoder refuses is not coded: the verdict is its errc.
    std::vector<size_t> slot_of(frame_count, 0);
    size_t largest_slot = 0;
    for (uint32_t f = 0; f < frame_count; ++f)
    {
        const charls_amd_frame_source& s = sources[f];
        sizes[f] = 0;
        errcs[f] = CHARLS_JPEGLS_ERRC_SUCCESS;
        if (f != 0 && same_group(s, sources[f - 1])) // (a uniform batch is checked once)
        {
            errcs[f] = errcs[f - 1];
            slot_of[f] = slot_of[f - 1];
            continue;
        }
        try
        {
            check_encode_params(s.params, SIZE_MAX, s.stride);
            slot_of[f] = s.max_stream_bytes != 0 ? static_cast<size_t>(s.max_stream_bytes) : estimated_stream_bytes(s.params);
            largest_slot = std::max(largest_slot, slot_of[f]);
        }
        catch (const error& e)
        {
            errcs[f] = e.code;
        }
    }

    // ---- the windows: as many frames in the caller's order as the staging holds -- a work area of the calling thread, a
    // quarter of what its work areas may grow to (batch_packed.cpp) --, or PACK_PASS_FRAMES frames.  A group's stretch starts
    // on a multiple of kStretchAlignment, which the estimate below leaves room for with every frame.
    const size_t budget = dev::work_area_budget();
    if (dev::workspace_limit() != 0 && budget < largest_slot)
        raise(CHARLS_JPEGLS_ERRC_NOT_ENOUGH_MEMORY);
    const long long forced = knobs::get_or(knobs::kPackPassFrames, 0);
    size_t room = forced >= 1 ? SIZE_MAX : std::max<size_t>(budget / 4, 1); // (the knob forces the window length, as it forces the pass length)
    uint32_t most = forced >= 1 ? static_cast<uint32_t>(std::min<long long>(forced, frame_count)) : frame_count;
    std::vector<uint32_t> window_end; // one past the last frame of every window
    uint8_t* staging = nullptr;
    for (;;)
    {
        window_end.clear();
        size_t filled = 0, largest = 0;
        uint32_t held = 0;
        for (uint32_t f = 0; f < frame_count; ++f)
        {
            const size_t want = slot_of[f] == 0 ? 0 : checked_mul(slot_of[f] / kStretchAlignment + 2, kStretchAlignment);
            if (held != 0 && (held == most || want > room - std::min(filled, room)))
            {
                window_end.push_back(f);
                largest = std::max(largest, filled);
                filled = 0;
                held = 0;
            }
            filled += want;
            ++held;
        }
        window_end.push_back(frame_count);
        largest = std::max(largest, filled);
        // (+ 16: the pack kernel reads whole aligned 16-byte granules, up to 15 bytes behind the last slot)
        staging = static_cast<uint8_t*>(dev::try_ensure(dev::pack_arena(), largest + 16));
        if (staging != nullptr)
            break;
        if (window_end.size() == frame_count) // (windows of one frame each: nothing smaller to ask for)
            raise(CHARLS_JPEGLS_ERRC_NOT_ENOUGH_MEMORY);
        room = std::max<size_t>(room / 2, 1);
        most = (most + 1) / 2;
    }

    std::vector<PackJob> jobs(frame_count); // (every window fills a stretch of its own)
    dev::DeviceBuffer d_jobs;
    d_jobs.ensure(sizeof(PackJob) * frame_count);
    std::vector<Group> groups;
    std::vector<uint32_t> group_of(frame_count), place_in_group(frame_count);
    std::vector<const uint8_t*> pixels;
    std::vector<uint64_t> group_sizes;
    std::vector<charls_jpegls_errc> group_errcs;
    double total_ms = 0, scan_ms = 0;
    uint64_t at = 0;
    size_t job_count = 0;
    bool full = false; // a frame's end lay beyond the capacity: that frame and every frame after it get destination_too_small
    uint32_t first_beyond = frame_count;
    for (uint32_t w = 0, first = 0; w < window_end.size(); first = window_end[w++])
    {
        const uint32_t last = window_end[w];
        groups.clear();
        for (uint32_t f = first; f < last && !full; ++f)
        {
            if (errcs[f] != CHARLS_JPEGLS_ERRC_SUCCESS)
                continue;
            // (the frame before it first: the frames of a uniform batch, and runs of equal frames, cost one comparison each)
            size_t g = groups.size();
            if (f != first && errcs[f - 1] == CHARLS_JPEGLS_ERRC_SUCCESS && same_group(sources[f], sources[f - 1]))
                g = group_of[f - 1];
            else
                for (g = 0; g < groups.size() && !same_group(sources[f], sources[groups[g].first]); ++g)
                {
                }
            if (g == groups.size())
                groups.push_back(Group{f, {}, slot_of[f], 0});
            group_of[f] = static_cast<uint32_t>(g);
            place_in_group[f] = static_cast<uint32_t>(groups[g].frames.size());
            groups[g].frames.push_back(f);
        }
        size_t stretch = 0;
        for (Group& g : groups)
        {
            g.stretch = stretch;
            stretch = (stretch + g.slot * g.frames.size() + kStretchAlignment - 1) & ~(kStretchAlignment - 1);
        }
        // ---- the groups one after another, each by the launches of the slot encoder (which synchronises: the sizes and
        // errcs of the group are here when it returns)
        for (const Group& g : groups)
        {
            const uint32_t n = static_cast<uint32_t>(g.frames.size());
            pixels.resize(n);
            group_sizes.assign(n, 0);
            group_errcs.assign(n, CHARLS_JPEGLS_ERRC_SUCCESS);
            for (uint32_t k = 0; k < n; ++k)
                pixels[k] = static_cast<const uint8_t*>(sources[g.frames[k]].d_pixels);
            const charls_amd_frame_source& s = sources[g.first];
            encode_batch_frames(s.params, n, pixels.data(), SIZE_MAX, s.stride, staging + g.stretch, g.slot, group_sizes.data(),
                                group_errcs.data(), hip_stream);
            for (uint32_t k = 0; k < n; ++k)
            {
                sizes[g.frames[k]] = group_sizes[k];
                errcs[g.frames[k]] = group_errcs[k];
            }
            const dev::Timings& t = dev::last_timings();
            total_ms += t.count > 0 ? t.values[0] : 0;
            scan_ms += t.count > 1 ? t.values[1] : 0;
        }
        // ---- one pack launch for the window, the jobs in the caller's frame order (batch_packed.cpp has the rule)
        const size_t window_jobs = job_count;
        uint64_t longest = 0;
        for (uint32_t f = first; f < last; ++f)
        {
            offsets[f] = at;
            const bool coded = !full && errcs[f] == CHARLS_JPEGLS_ERRC_SUCCESS && sizes[f] != 0;
            if (coded && sizes[f] > packed_capacity_bytes - std::min<uint64_t>(at, packed_capacity_bytes))
            {
                full = true;
                first_beyond = f;
            }
            if (full)
            {
                errcs[f] = CHARLS_JPEGLS_ERRC_DESTINATION_TOO_SMALL;
                sizes[f] = 0;
                continue;
            }
            if (!coded)
            {
                sizes[f] = 0;
                continue; // (a frame that failed takes no room)
            }
            const uint64_t end = at + sizes[f];
            const uint64_t next = round_up_to(end, offset_alignment);
            // (the gap behind the last frame that fits is zeroed as far as the buffer goes)
            const uint64_t pad = std::min<uint64_t>(next, packed_capacity_bytes) - end;
            const Group& g = groups[group_of[f]];
            jobs[job_count++] = PackJob{g.stretch + static_cast<uint64_t>(place_in_group[f]) * g.slot, at, sizes[f], static_cast<uint32_t>(pad), 0};
            longest = std::max(longest, sizes[f] + pad);
            at = next;
        }
        if (job_count != window_jobs)
        {
            hip_check(hipMemcpyAsync(d_jobs.as<PackJob>() + window_jobs, jobs.data() + window_jobs, sizeof(PackJob) * (job_count - window_jobs),
                                     hipMemcpyHostToDevice, stream));
            dev::launch_pack_streams(staging, static_cast<uint8_t*>(d_packed), d_jobs.as<PackJob>() + window_jobs,
                                     static_cast<uint32_t>(job_count - window_jobs), longest, stream);
            // (the next window codes into the same staging, partly on the encoder's side streams)
            hip_check(hipStreamSynchronize(stream));
        }
    }
    offsets[frame_count] = at;
    dev::Timings& t = dev::last_timings(); // charls_amd_last_timings: the groups' totals and dominant kernels, summed
    t.values[0] = total_ms;
    t.values[1] = scan_ms;
    t.count = 2;
    return first_beyond;
}
