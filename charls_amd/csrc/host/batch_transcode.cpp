// batch_transcode.cpp -- re-coding the streams of a packed blob in one call (charls_amd.h part 2j): every stream is decoded
// and coded again with a few of its parameters replaced -- a restart interval added, NEAR raised -- without the caller owning
// the frames in between.
//
//  * The call is a composition and adds no kernel: the probe and the ragged decode (batch_api.cpp: decode_batch_streams) and
//    the ragged encode (batch_ragged.cpp: encode_ragged_frames), joined the way a caller would join them.
//  * The frames are walked in the caller's order in WINDOWS: as many as fit one more work area of the calling thread
//    (dev::transcode_arena), into which a window is decoded and from which it is coded.  A window's streams go to
//    d_packed_out + base, base being the end of the window before it -- a multiple of the alignment, so that bytes, gaps and
//    offsets are those of one encode over all frames.
//  * charls_amd_transcode_batch_host (batch_host.cpp) runs the same body on device windows of host blobs.
//  * The ENCODE STEP of a window is a parameter of the body (batch_streams.h: TranscodeEncode): the ragged encode here, the
//    budgeted one (batch_budget.cpp: NEAR picked per frame from a list of candidates) in charls_amd_transcode_batch_device_budget
//    and its host form (charls_amd.h part 2k).  Everything else -- probe, windows, decode, offsets, capacity tail -- is shared.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "../device/knobs.h"
#include "../device/runtime.h"
#include "batch_streams.h"
#include "common.h"

using namespace jls;

namespace {

constexpr uint32_t kSpecBits = CHARLS_AMD_TRANSCODE_NEAR | CHARLS_AMD_TRANSCODE_RESTART_INTERVAL | CHARLS_AMD_TRANSCODE_PRESET |
                               CHARLS_AMD_TRANSCODE_ENCODING_OPTIONS;
constexpr size_t kFrameAlignment = 256; // every frame of a window starts on one

// ---- charls_amd_transcode_counters
enum Counter
{
    kRecoded,
    kWindows,
    kRefusedForTable,
    kBehindCapacity,
    kCounters
};
std::atomic<uint64_t> g_counters[kCounters];

void count(Counter c, uint64_t n) noexcept
{
    g_counters[c].fetch_add(n, std::memory_order_relaxed);
}

} // namespace

TranscodeEncode jls::transcode_encode_plain()
{
    return [](uint32_t count, charls_amd_frame_source* sources, const uint32_t*, void* d_packed, size_t packed_capacity_bytes,
              uint32_t offset_alignment, uint64_t* offsets, uint64_t* sizes, charls_jpegls_errc* errcs, void* hip_stream) {
        return encode_ragged_frames(count, sources, d_packed, packed_capacity_bytes, offset_alignment, offsets, sizes, errcs, hip_stream);
    };
}

void jls::transcode_count_behind_capacity(uint64_t frames) noexcept
{
    count(kBehindCapacity, frames);
}

charls_amd_codec_params jls::transcode_params(charls_amd_codec_params p, const charls_amd_transcode_spec& spec) noexcept
{
    if (spec.set & CHARLS_AMD_TRANSCODE_NEAR)
        p.near_lossless = spec.near_lossless;
    if (spec.set & CHARLS_AMD_TRANSCODE_RESTART_INTERVAL)
        p.restart_interval = spec.restart_interval;
    if (spec.set & CHARLS_AMD_TRANSCODE_PRESET)
        p.preset_coding_parameters = spec.preset_coding_parameters;
    if (spec.set & CHARLS_AMD_TRANSCODE_ENCODING_OPTIONS)
        p.encoding_options = spec.encoding_options;
    return p;
}

void jls::check_transcode_call(uint32_t frame_count, const void* packed_in, const uint64_t* offsets_in, const uint64_t* sizes_in,
                               const charls_amd_transcode_spec* specs, uint32_t spec_count, const void* packed_out, uint32_t offset_alignment,
                               const uint64_t* offsets_out, const uint64_t* sizes_out, const charls_amd_codec_params* params_out,
                               const charls_jpegls_errc* errcs)
{
    check_pointer(offsets_in);
    check_pointer(sizes_in);
    check_pointer(specs);
    check_pointer(offsets_out);
    check_pointer(sizes_out);
    check_pointer(params_out);
    check_pointer(errcs);
    check_argument(spec_count == 1 || spec_count == frame_count);
    for (uint32_t k = 0; k < spec_count; ++k)
        check_argument((specs[k].set & ~kSpecBits) == 0 && specs[k].reserved == 0);
    check_offset_alignment(offset_alignment);
    if (frame_count == 0)
        return;
    check_pointer(packed_in);
    check_pointer(packed_out);
    for (uint32_t f = 0; f < frame_count; ++f)
    {
        uint64_t end;
        if (__builtin_add_overflow(offsets_in[f], sizes_in[f], &end))
            raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_SIZE);
    }
}

void jls::check_transcode_budget_call(uint32_t frame_count, const void* packed_in, const uint64_t* offsets_in, const uint64_t* sizes_in,
                                      const charls_amd_transcode_spec* specs, uint32_t spec_count, const uint64_t* budgets,
                                      const int32_t* near_candidates, uint32_t candidate_count, const void* packed_out,
                                      uint32_t offset_alignment, const uint64_t* offsets_out, const uint64_t* sizes_out,
                                      const int32_t* near_out, const charls_amd_codec_params* params_out, const charls_jpegls_errc* errcs)
{
    check_budget_tables(budgets, near_candidates, candidate_count, near_out);
    check_pointer(specs);
    check_argument(spec_count == 1 || spec_count == frame_count);
    for (uint32_t k = 0; k < spec_count; ++k) // (the candidates decide NEAR)
        check_argument((specs[k].set & CHARLS_AMD_TRANSCODE_NEAR) == 0);
    check_transcode_call(frame_count, packed_in, offsets_in, sizes_in, specs, spec_count, packed_out, offset_alignment, offsets_out, sizes_out,
                         params_out, errcs);
}

void jls::transcode_near_of_uncoded(uint32_t frame_count, const charls_jpegls_errc* errcs, int32_t* near_out) noexcept
{
    for (uint32_t f = 0; f < frame_count; ++f)
        if (errcs[f] != CHARLS_JPEGLS_ERRC_SUCCESS)
            near_out[f] = -1;
}

uint32_t jls::transcode_frames(uint32_t frame_count, const void* d_packed_in, const uint64_t* offsets_in, const uint64_t* sizes_in,
                               const charls_amd_transcode_spec* specs, uint32_t spec_count, void* d_packed_out, size_t packed_capacity_bytes,
                               uint32_t offset_alignment, uint64_t* offsets_out, uint64_t* sizes_out, charls_amd_codec_params* params_out,
                               charls_jpegls_errc* errcs, const TranscodeEncode& encode, void* hip_stream)
{
    auto spec_of = [&](uint32_t f) -> const charls_amd_transcode_spec& { return specs[spec_count == 1 ? 0 : f]; };

    // ---- one probe of the whole batch: what every frame takes in the area, and what it will be coded with
    std::vector<charls_amd_codec_params> probed(frame_count);
    std::vector<uint64_t> frame_bytes(frame_count);
    std::vector<charls_jpegls_errc> probe_errcs(frame_count);
    decode_batch_streams(frame_count, d_packed_in, offsets_in, sizes_in, BatchDests{nullptr, true, frame_bytes.data()}, probed.data(),
                         probe_errcs.data(), hip_stream);
    std::vector<size_t> want(frame_count, 0);
    size_t largest = 0;
    for (uint32_t f = 0; f < frame_count; ++f)
    {
        if (probe_errcs[f] != CHARLS_JPEGLS_ERRC_SUCCESS || frame_bytes[f] == 0)
            continue;
        want[f] = checked_mul(static_cast<size_t>(frame_bytes[f]) / kFrameAlignment + 1, kFrameAlignment);
        // (the encoder's staging slot of the frame is a little larger than the frame: the limit has to cover that as well)
        largest = std::max({largest, want[f], estimated_stream_bytes(transcode_params(probed[f], spec_of(f)))});
    }
    // What a frame that is not coded for itself reports: the stream's parameters with the spec, where its header was read.
    auto params_by_probe = [&](uint32_t f) {
        return probe_errcs[f] == CHARLS_JPEGLS_ERRC_SUCCESS && frame_bytes[f] != 0 ? transcode_params(probed[f], spec_of(f))
                                                                                   : charls_amd_codec_params{};
    };

    // ---- the windows: as many frames in the caller's order as the area holds -- a quarter of what the thread's work areas
    // may grow to, as the staging of part 2d --, or TRANSCODE_WINDOW_FRAMES frames
    const size_t budget = dev::work_area_budget();
    if (dev::workspace_limit() != 0 && budget < largest)
        raise(CHARLS_JPEGLS_ERRC_NOT_ENOUGH_MEMORY);
    const long long forced = knobs::get_or(knobs::kTranscodeWindowFrames, 0);
    size_t room = forced >= 1 ? SIZE_MAX : std::max<size_t>(budget / 4, 1);
    uint32_t most = forced >= 1 ? static_cast<uint32_t>(std::min<long long>(forced, frame_count)) : frame_count;
    std::vector<uint32_t> window_end; // one past the last frame of every window
    uint8_t* area = nullptr;
    for (;;)
    {
        window_end.clear();
        size_t filled = 0, most_filled = 0;
        uint32_t held = 0;
        for (uint32_t f = 0; f < frame_count; ++f)
        {
            if (held != 0 && (held == most || want[f] > room - std::min(filled, room)))
            {
                window_end.push_back(f);
                most_filled = std::max(most_filled, filled);
                filled = 0;
                held = 0;
            }
            filled += want[f];
            ++held;
        }
        window_end.push_back(frame_count);
        most_filled = std::max(most_filled, filled);
        area = static_cast<uint8_t*>(dev::try_ensure(dev::transcode_arena(), most_filled + kFrameAlignment));
        if (area != nullptr)
            break;
        if (window_end.size() == frame_count) // (windows of one frame each: nothing smaller to ask for)
            raise(CHARLS_JPEGLS_ERRC_NOT_ENOUGH_MEMORY);
        room = std::max<size_t>(room / 2, 1);
        most = (most + 1) / 2;
    }

    auto* out = static_cast<uint8_t*>(d_packed_out);
    std::vector<charls_amd_frame_dest> dests;
    std::vector<charls_amd_frame_source> sources;
    std::vector<charls_amd_codec_params> w_params;
    std::vector<charls_jpegls_errc> w_errcs, c_errcs;
    std::vector<uint8_t> names_table;
    std::vector<uint32_t> sent;
    std::vector<uint64_t> c_offsets, c_sizes;
    double decode_ms = 0, encode_ms = 0, scan_ms = 0;
    uint64_t base = 0;                  // the end of the window before this one: a multiple of the alignment
    uint32_t first_beyond = frame_count; // the frame whose end lay beyond the capacity
    for (uint32_t w = 0, first = 0; w < window_end.size() && first_beyond == frame_count; first = window_end[w++])
    {
        const uint32_t last = window_end[w], n = last - first;
        count(kWindows, 1);
        // ---- 1. the ragged decode of the window into the area, packed
        dests.resize(n);
        size_t at = 0;
        for (uint32_t k = 0; k < n; ++k)
        {
            dests[k] = charls_amd_frame_dest{area + at, frame_bytes[first + k], 0, 0};
            at += want[first + k];
        }
        w_params.assign(n, charls_amd_codec_params{});
        w_errcs.assign(n, CHARLS_JPEGLS_ERRC_SUCCESS);
        names_table.assign(n, 0);
        decode_batch_streams(n, d_packed_in, offsets_in + first, sizes_in + first, BatchDests{dests.data(), true, nullptr, names_table.data()},
                             w_params.data(), w_errcs.data(), hip_stream);
        const dev::Timings& t = dev::last_timings();
        decode_ms += t.count > 0 ? t.values[0] : 0;
        scan_ms += t.count > 1 ? t.values[1] : 0;

        // ---- 2. the encode step on the frames that decoded, behind the window before
        sent.clear();
        sources.clear();
        for (uint32_t k = 0; k < n; ++k)
        {
            const uint32_t f = first + k;
            errcs[f] = w_errcs[k];
            sizes_out[f] = 0;
            params_out[f] = charls_amd_codec_params{};
            if (w_errcs[k] != CHARLS_JPEGLS_ERRC_SUCCESS)
                continue;
            if (names_table[k] != 0)
            { // (the batch encoder cannot write the table, and without it the samples would mean something else)
                errcs[f] = CHARLS_JPEGLS_ERRC_INVALID_OPERATION;
                count(kRefusedForTable, 1);
                continue;
            }
            params_out[f] = transcode_params(w_params[k], spec_of(f));
            sent.push_back(f);
            sources.push_back(charls_amd_frame_source{params_out[f], dests[k].d_pixels, 0, 0, 0});
        }
        const uint32_t m = static_cast<uint32_t>(sent.size());
        c_offsets.assign(static_cast<size_t>(m) + 1, 0);
        uint32_t beyond = m;
        if (m != 0)
        {
            c_sizes.assign(m, 0);
            c_errcs.assign(m, CHARLS_JPEGLS_ERRC_SUCCESS);
            const uint64_t reach = std::min<uint64_t>(base, packed_capacity_bytes);
            beyond = encode(m, sources.data(), sent.data(), out + reach, packed_capacity_bytes - static_cast<size_t>(reach), offset_alignment,
                            c_offsets.data(), c_sizes.data(), c_errcs.data(), hip_stream);
            const dev::Timings& e = dev::last_timings();
            encode_ms += e.count > 0 ? e.values[0] : 0;
            scan_ms += e.count > 1 ? e.values[1] : 0;
        }
        // ---- 3. the window's offsets from the start of the blob; a frame that was not coded stands where the next one starts
        for (uint32_t k = 0, c = 0; k < n; ++k)
        {
            const uint32_t f = first + k;
            offsets_out[f] = base + c_offsets[c];
            if (c < m && sent[c] == f)
            {
                sizes_out[f] = c_sizes[c];
                errcs[f] = c_errcs[c];
                params_out[f] = sources[c].params; // (what the step coded it with: the candidate it picked, in the budgeted form)
                ++c;
            }
        }
        base += c_offsets[m];
        if (beyond != m)
            first_beyond = sent[beyond];
    }
    // ---- behind the capacity: every frame after the one that did not fit, decoded or not, in this window or a later one
    for (uint32_t f = first_beyond; f < frame_count; ++f)
    {
        if (f != first_beyond)
        {
            offsets_out[f] = base;
            params_out[f] = params_by_probe(f);
        }
        sizes_out[f] = 0;
        errcs[f] = CHARLS_JPEGLS_ERRC_DESTINATION_TOO_SMALL;
    }
    if (first_beyond != frame_count)
        count(kBehindCapacity, frame_count - first_beyond - 1);
    offsets_out[frame_count] = base;
    uint64_t recoded = 0;
    for (uint32_t f = 0; f < frame_count; ++f)
        recoded += errcs[f] == CHARLS_JPEGLS_ERRC_SUCCESS ? 1 : 0;
    count(kRecoded, recoded);
    dev::Timings& t = dev::last_timings(); // charls_amd_last_timings: [0] all launches, [1] the dominant kernels, [2] decoding, [3] the encode steps (sizing and encoding)
    t.values[0] = decode_ms + encode_ms;
    t.values[1] = scan_ms;
    t.values[2] = decode_ms;
    t.values[3] = encode_ms;
    t.count = 4;
    return first_beyond;
}

extern "C" charls_jpegls_errc charls_amd_transcode_batch_device(uint32_t frame_count, const void* d_packed_in, const uint64_t* offsets_in,
                                                                const uint64_t* sizes_in, const charls_amd_transcode_spec* specs,
                                                                uint32_t spec_count, void* d_packed_out, size_t packed_capacity_bytes,
                                                                uint32_t offset_alignment, uint64_t* offsets_out, uint64_t* sizes_out,
                                                                charls_amd_codec_params* params_out, charls_jpegls_errc* errcs, void* hip_stream)
try
{
    check_transcode_call(frame_count, d_packed_in, offsets_in, sizes_in, specs, spec_count, d_packed_out, offset_alignment, offsets_out,
                         sizes_out, params_out, errcs);
    if (frame_count == 0)
    {
        offsets_out[0] = 0;
        return CHARLS_JPEGLS_ERRC_SUCCESS;
    }
    dev::require_device();
    transcode_frames(frame_count, d_packed_in, offsets_in, sizes_in, specs, spec_count, d_packed_out, packed_capacity_bytes, offset_alignment,
                     offsets_out, sizes_out, params_out, errcs, transcode_encode_plain(), hip_stream);
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}

// Part 2k: the same body with the budgeted encode step.
extern "C" charls_jpegls_errc charls_amd_transcode_batch_device_budget(
    uint32_t frame_count, const void* d_packed_in, const uint64_t* offsets_in, const uint64_t* sizes_in,
    const charls_amd_transcode_spec* specs, uint32_t spec_count, const uint64_t* budgets, const int32_t* near_candidates,
    uint32_t candidate_count, void* d_packed_out, size_t packed_capacity_bytes, uint32_t offset_alignment, uint64_t* offsets_out,
    uint64_t* sizes_out, int32_t* near_out, charls_amd_codec_params* params_out, charls_jpegls_errc* errcs, void* hip_stream)
try
{
    check_transcode_budget_call(frame_count, d_packed_in, offsets_in, sizes_in, specs, spec_count, budgets, near_candidates, candidate_count,
                                d_packed_out, offset_alignment, offsets_out, sizes_out, near_out, params_out, errcs);
    if (frame_count == 0)
    {
        offsets_out[0] = 0;
        return CHARLS_JPEGLS_ERRC_SUCCESS;
    }
    dev::require_device();
    transcode_frames(frame_count, d_packed_in, offsets_in, sizes_in, specs, spec_count, d_packed_out, packed_capacity_bytes, offset_alignment,
                     offsets_out, sizes_out, params_out, errcs, transcode_encode_budget(budgets, near_candidates, candidate_count, near_out),
                     hip_stream);
    transcode_near_of_uncoded(frame_count, errcs, near_out);
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}

extern "C" int32_t charls_amd_transcode_counters(uint64_t* out, int32_t capacity)
{
    int32_t n = 0;
    for (; out != nullptr && n < capacity && n < kCounters; ++n)
        out[n] = g_counters[n].load(std::memory_order_relaxed);
    return n;
}
