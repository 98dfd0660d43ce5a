// batch_packed.cpp -- the batch API on PACKED streams (charls_amd.h part 2d): streams back to back in one device buffer with
// a host table of offsets, the form files, archives, DICOM multi-frame pixel data and charls_amd_gather hold them in.
//
//  * charls_amd_pack_streams_device turns the slot array of charls_amd_encode_batch_device into the packed form: one launch
//    of the segmented copy kernel (device/pack_streams.hip).
//  * charls_amd_encode_batch_device_packed needs no caller-provided slots: it codes passes of P frames with the slot encoder
//    into staging slots of its own (dev::pack_arena, a work area of the calling thread) and packs every pass with ONE launch;
//    the running offset carries from pass to pass.
//  * charls_amd_decode_batch_device_packed is the slot decoder (batch_api.cpp: decode_batch_streams) with frame f's stream at
//    d_packed + offsets[f]; no kernel knows the difference.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../device/knobs.h"
#include "../device/pack_streams.h"
#include "../device/runtime.h"
#include "batch_streams.h"
#include "common.h"
#include "event_timer.h"

using namespace jls;
using dev::hip_check;

// charls_jpegls_encoder_get_estimated_destination_size for the frames of `p` (encoder_api.cpp; reference
// src/charls_jpegls_encoder.cpp:103-114).  Parameters the encoder is going to refuse give 1: the call fails on them anyway.
size_t jls::estimated_stream_bytes(const charls_amd_codec_params& p)
{
    const charls_frame_info& f = p.frame_info;
    if (f.width == 0 || f.width > kMaxDimension || f.height == 0 || f.height > kMaxDimension || f.component_count < 1 ||
        f.component_count > kMaxComponents || f.bits_per_sample < kMinBits || f.bits_per_sample > kMaxBits)
        return 1;
    const size_t size = static_cast<size_t>(f.width) * f.height * static_cast<size_t>(f.component_count) * bytes_per_sample(f.bits_per_sample);
    size_t extra = size / 16 + 1024 + kSpiffHeaderSize;
    if (p.restart_interval != 0)
        extra += 6 + 2 * static_cast<size_t>((f.height + p.restart_interval - 1) / p.restart_interval) * static_cast<size_t>(f.component_count);
    return size + extra;
}

size_t jls::longest_stream_bytes(const charls_amd_codec_params& p)
{
    const charls_frame_info& f = p.frame_info;
    const size_t rest = estimated_stream_bytes(p); // (the container, the markers and padding of restart intervals: its `extra`)
    if (rest == 1)
        return 1;
    // A regular sample is a Golomb code of at most LIMIT = 2 * (bpp + max(8, bpp)) bits; a run costs at most a bit per sample,
    // and the sample that ends it 1 + J bits of run length and at most LIMIT - J - 1 of error.  After a 0xFF byte the next
    // holds seven bits: at most 8 / 7 of the bytes.
    const size_t bpp = static_cast<size_t>(std::max<int32_t>(f.bits_per_sample, 2));
    const size_t limit_bits = 2 * (bpp + std::max<size_t>(8, bpp));
    const size_t samples = static_cast<size_t>(f.width) * f.height * static_cast<size_t>(f.component_count);
    return checked_mul(samples, limit_bits) / 7 + rest;
}

extern "C" charls_jpegls_errc charls_amd_pack_streams_device(uint32_t frame_count, const void* d_streams, size_t stream_pitch_bytes,
                                                             const uint64_t* sizes, void* d_packed, size_t packed_capacity_bytes,
                                                             uint32_t offset_alignment, uint64_t* offsets, void* hip_stream)
try
{
    check_pointer(sizes);
    check_pointer(offsets);
    check_offset_alignment(offset_alignment);
    if (frame_count == 0)
    {
        offsets[0] = 0;
        return CHARLS_JPEGLS_ERRC_SUCCESS;
    }
    check_pointer(d_streams);
    check_pointer(d_packed);
    dev::require_device();
    auto stream = static_cast<hipStream_t>(hip_stream);

    // the whole table first: a call that cannot be honoured writes nothing
    std::vector<PackJob> jobs;
    jobs.reserve(frame_count);
    std::vector<uint64_t> table(static_cast<size_t>(frame_count) + 1);
    uint64_t at = 0, longest = 0;
    for (uint32_t f = 0; f < frame_count; ++f)
    {
        table[f] = at;
        if (sizes[f] > stream_pitch_bytes || sizes[f] > packed_capacity_bytes - std::min<uint64_t>(at, packed_capacity_bytes))
            raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_SIZE);
        if (sizes[f] == 0)
            continue; // (a frame that failed takes no room)
        const uint64_t end = at + sizes[f];
        const uint64_t next = round_up_to(end, offset_alignment);
        if (next > packed_capacity_bytes)
            raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_SIZE);
        jobs.push_back(PackJob{static_cast<uint64_t>(f) * stream_pitch_bytes, at, sizes[f], static_cast<uint32_t>(next - end), 0});
        longest = std::max(longest, next - at);
        at = next;
    }
    table[frame_count] = at;
    std::copy(table.begin(), table.end(), offsets);
    if (jobs.empty())
        return CHARLS_JPEGLS_ERRC_SUCCESS;

    dev::DeviceBuffer d_jobs;
    d_jobs.ensure(sizeof(PackJob) * jobs.size());
    hip_check(hipMemcpyAsync(d_jobs.as<PackJob>(), jobs.data(), sizeof(PackJob) * jobs.size(), hipMemcpyHostToDevice, stream));
    EventTimer timer(stream);
    timer.start();
    dev::launch_pack_streams(static_cast<const uint8_t*>(d_streams), static_cast<uint8_t*>(d_packed), d_jobs.as<PackJob>(),
                             static_cast<uint32_t>(jobs.size()), longest, stream);
    timer.stop();
    const double ms = timer.ms();          // (the call returns after the stream work has completed)
    dev::Timings& t = dev::last_timings();   // charls_amd_last_timings: [0] = [1] = the copy kernel
    t.values[0] = t.values[1] = ms;
    t.count = 2;
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}

extern "C" charls_jpegls_errc charls_amd_encode_batch_device_packed(const charls_amd_codec_params* params, uint32_t frame_count,
                                                                    const void* d_frames, size_t frame_pitch_bytes, uint32_t stride,
                                                                    void* d_packed, size_t packed_capacity_bytes,
                                                                    uint32_t offset_alignment, size_t max_stream_bytes,
                                                                    uint64_t* offsets, uint64_t* sizes, charls_jpegls_errc* errcs,
                                                                    void* hip_stream)
try
{
    check_pointer(params);
    check_pointer(offsets);
    check_pointer(sizes);
    check_pointer(errcs);
    check_offset_alignment(offset_alignment);
    if (frame_count == 0)
    {
        offsets[0] = 0;
        return CHARLS_JPEGLS_ERRC_SUCCESS;
    }
    check_pointer(d_frames);
    check_pointer(d_packed);
    dev::require_device();
    auto stream = static_cast<hipStream_t>(hip_stream);
    const size_t slot = max_stream_bytes != 0 ? max_stream_bytes : estimated_stream_bytes(*params);

    // ---- the staging slots: a work area of the calling thread, a quarter of what its work areas may grow to (the encoder's
    // own areas want the rest); a configured workspace limit that does not cover one slot is honoured.
    const size_t budget = dev::work_area_budget();
    if (dev::workspace_limit() != 0 && budget < slot)
        raise(CHARLS_JPEGLS_ERRC_NOT_ENOUGH_MEMORY);
    uint32_t pass = static_cast<uint32_t>(std::min<size_t>(frame_count, std::max<size_t>(1, budget / 4 / slot)));
    const long long forced = knobs::get_or(knobs::kPackPassFrames, 0);
    if (forced >= 1)
        pass = static_cast<uint32_t>(std::min<long long>(forced, frame_count));
    uint8_t* staging = nullptr;
    // (+ 16: the pack kernel reads whole aligned 16-byte granules, up to 15 bytes behind the last slot)
    while ((staging = static_cast<uint8_t*>(dev::try_ensure(dev::pack_arena(), checked_mul(slot, pass) + 16))) == nullptr && pass > 1)
        pass = (pass + 1) / 2;
    if (staging == nullptr)
        raise(CHARLS_JPEGLS_ERRC_NOT_ENOUGH_MEMORY);

    std::vector<PackJob> jobs(frame_count); // (every pass fills a stretch of its own)
    dev::DeviceBuffer d_jobs;
    d_jobs.ensure(sizeof(PackJob) * frame_count);
    const auto* frames = static_cast<const uint8_t*>(d_frames);
    uint64_t at = 0;
    size_t job_count = 0;
    bool full = false; // a frame's end lay beyond the capacity: that frame and every frame after it get destination_too_small
    for (uint32_t first = 0; first < frame_count; first += pass)
    {
        const uint32_t n = std::min(pass, frame_count - first);
        if (!full)
        {
            const charls_jpegls_errc rc = charls_amd_encode_batch_device(params, n, frames + static_cast<size_t>(first) * frame_pitch_bytes,
                                                                         frame_pitch_bytes, stride, staging, slot, sizes + first,
                                                                         errcs + first, hip_stream);
            if (rc != CHARLS_JPEGLS_ERRC_SUCCESS)
                return rc;
        }
        // (the encoder has synchronised: sizes and errcs of the pass are here)
        const size_t pass_jobs = job_count;
        uint64_t longest = 0;
        for (uint32_t i = 0; i < n; ++i)
        {
            const uint32_t f = first + i;
            offsets[f] = at;
            if (!full && errcs[f] == CHARLS_JPEGLS_ERRC_SUCCESS && sizes[f] > packed_capacity_bytes - std::min<uint64_t>(at, packed_capacity_bytes))
                full = true;
            if (full)
            {
                errcs[f] = CHARLS_JPEGLS_ERRC_DESTINATION_TOO_SMALL;
                sizes[f] = 0;
                continue;
            }
            if (errcs[f] != CHARLS_JPEGLS_ERRC_SUCCESS || sizes[f] == 0)
            {
                sizes[f] = 0;
                continue; // (a frame that failed takes no room)
            }
            const uint64_t end = at + sizes[f];
            const uint64_t next = round_up_to(end, offset_alignment);
            // (the gap behind the last frame that fits is zeroed as far as the buffer goes)
            const uint64_t pad = std::min<uint64_t>(next, packed_capacity_bytes) - end;
            jobs[job_count++] = PackJob{static_cast<uint64_t>(i) * slot, at, sizes[f], static_cast<uint32_t>(pad), 0};
            longest = std::max(longest, sizes[f] + pad);
            at = next;
        }
        if (job_count != pass_jobs)
        {
            hip_check(hipMemcpyAsync(d_jobs.as<PackJob>() + pass_jobs, jobs.data() + pass_jobs, sizeof(PackJob) * (job_count - pass_jobs),
                                     hipMemcpyHostToDevice, stream));
            dev::launch_pack_streams(staging, static_cast<uint8_t*>(d_packed), d_jobs.as<PackJob>() + pass_jobs,
                                     static_cast<uint32_t>(job_count - pass_jobs), longest, stream);
            // (the next pass codes into the same staging slots, partly on the encoder's side streams)
            hip_check(hipStreamSynchronize(stream));
        }
    }
    offsets[frame_count] = at;
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}

extern "C" charls_jpegls_errc charls_amd_decode_batch_device_packed(uint32_t frame_count, const void* d_packed, const uint64_t* offsets,
                                                                    const uint64_t* sizes, void* d_frames, size_t frame_pitch_bytes,
                                                                    uint32_t stride, charls_amd_codec_params* params_out,
                                                                    charls_jpegls_errc* errcs, void* hip_stream)
try
{
    check_pointer(offsets);
    check_pointer(sizes);
    check_pointer(errcs);
    if (frame_count == 0)
        return CHARLS_JPEGLS_ERRC_SUCCESS;
    check_pointer(d_packed);
    check_pointer(d_frames);
    for (uint32_t f = 0; f < frame_count; ++f)
    {
        uint64_t end;
        if (__builtin_add_overflow(offsets[f], sizes[f], &end))
            raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_SIZE);
    }
    decode_batch_streams(frame_count, d_packed, offsets, sizes, d_frames, frame_pitch_bytes, stride, params_out, errcs, hip_stream);
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}
