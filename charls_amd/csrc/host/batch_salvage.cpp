// batch_salvage.cpp -- the salvage decode (charls_amd.h part 2g): the ragged batch decoder, and behind it a second round for
// the frames it failed on that have restart intervals -- their intact intervals are decoded, the rest is filled.
//
//  * Round 1 is decode_batch_streams (batch_api.cpp), untouched: return value, params_out, errcs and the pixels of the frames
//    that decode are its own.  A batch without failed frames ends there.
//  * Round 2 parses the headers of the failed frames again (StreamWindows), keeps those that got past their header and their
//    destination checks and whose first scan has intervals that decode on their own (dev::salvage_candidate), and runs
//    dev::launch_decode_salvage on the scans that share a launch key -- scan by scan for planar frames: scan c + 1 is looked
//    for where scan c's segment ends; a scan that is not reached goes through the same launch without a stream and is filled.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <vector>

#include "../device/runtime.h"
#include "batch_streams.h"
#include "common.h"
#include "scan_engine.h"
#include "seek_index.h"
#include "stream_windows.h"

using namespace jls;
using dev::hip_check;

namespace {

std::atomic<uint64_t> g_frames_salvaged{0}, g_intervals_kept{0}, g_intervals_lost{0};

constexpr uint32_t kNoRow = UINT32_MAX;

// A frame of round 2.
struct Salvaged
{
    uint32_t frame;       // in the caller's tables
    uint32_t scans;       // the component scans of a planar frame, else 1
    uint32_t intervals;   // N of every scan
    ScanDesc first;       // its first scan
    size_t plane_bytes;   // from one scan's rows to the next scan's
    bool reached{true};   // the scan of the current round was located
    std::vector<uint8_t> status; // scans x N
};

// The frame's current scan as the kernels take it: the reader stands behind the scan's header.
ScanDesc desc_at(const StreamWindows& win, uint32_t k, const BatchFrame& x, const charls_amd_frame_dest& dest)
{
    const auto [row, stride] = row_and_stride(x.reader, dest.stride);
    (void)row;
    ScanDesc d = desc_of(scan_spec_of(x.reader));
    d.pixels = static_cast<uint8_t*>(dest.d_pixels) + x.plane_offset;
    d.pixel_stride = stride;
    d.stream = win.stream_ptr(k, x.cursor);
    d.stream_capacity = win.sizes[k] - x.cursor;
    return d;
}

} // namespace

void jls::decode_batch_salvage(uint32_t frame_count, const void* d_packed, const uint64_t* offsets, const uint64_t* sizes,
                               const charls_amd_frame_dest* dests, uint32_t fill_value, charls_amd_codec_params* params_out,
                               charls_amd_salvage_report* reports, uint8_t* interval_status, size_t status_pitch_bytes,
                               charls_jpegls_errc* errcs, void* hip_stream)
{
    decode_batch_streams(frame_count, d_packed, offsets, sizes, BatchDests{dests, true, nullptr}, params_out, errcs, hip_stream);
    std::vector<uint32_t> failed;
    for (uint32_t f = 0; f < frame_count; ++f)
    {
        reports[f] = charls_amd_salvage_report{errcs[f] == CHARLS_JPEGLS_ERRC_SUCCESS ? 0u : 2u, 0, 0, 0, kNoRow, 0};
        if (errcs[f] != CHARLS_JPEGLS_ERRC_SUCCESS)
            failed.push_back(f);
    }
    if (failed.empty())
        return;
    // charls_amd_last_timings [2]: what round 2 took, by the host's clock (every launch of it ends in a synchronise)
    struct RoundClock
    {
        std::chrono::steady_clock::time_point begin = std::chrono::steady_clock::now();
        ~RoundClock()
        {
            dev::Timings& t = dev::last_timings();
            t.values[2] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - begin).count();
            t.count = 3;
        }
    } round_clock;

    // ---- which of the failed frames got past their header, and have intervals to salvage
    auto stream = static_cast<hipStream_t>(hip_stream);
    const uint32_t n = static_cast<uint32_t>(failed.size());
    std::vector<uint64_t> at(n), bytes(n);
    for (uint32_t k = 0; k < n; ++k)
    {
        at[k] = offsets[failed[k]];
        bytes[k] = sizes[failed[k]];
    }
    StreamWindows win(n, d_packed, at.data(), bytes.data(), stream);
    win.read_headers(true);
    std::vector<Salvaged> set;
    std::vector<uint32_t> window_of; // set[i] is win.fr[window_of[i]]
    uint32_t most_scans = 0;
    for (uint32_t k = 0; k < n; ++k)
    {
        const BatchFrame& x = win.fr[k];
        const charls_amd_frame_dest& dest = dests[failed[k]];
        if (x.done)
            continue; // the header does not parse
        try
        {
            const auto [row, stride] = row_and_stride(x.reader, dest.stride);
            const uint32_t scans = static_cast<uint32_t>(scans_of_frame(x.reader));
            const size_t rows = static_cast<size_t>(x.reader.frame_info().height) * scans;
            if (stride < row || dest.capacity_bytes < stride * rows - (stride - row))
                continue; // round 1 refused the destination: nothing of the frame is written
            const ScanDesc d = desc_at(win, k, x, dest);
            if (!dev::salvage_candidate(d))
                continue;
            if (fill_value > static_cast<uint32_t>(x.reader.validated_pc().maximum_sample_value))
            {
                errcs[failed[k]] = CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT;
                continue;
            }
            Salvaged s{failed[k], scans, (d.height + d.restart_interval - 1) / d.restart_interval, d, stride * d.height, true, {}};
            s.status.assign(static_cast<size_t>(s.scans) * s.intervals, 3);
            most_scans = std::max(most_scans, scans);
            set.push_back(std::move(s));
            window_of.push_back(k);
        }
        catch (const error&)
        { // (parameters the decoder refuses: round 1 said so)
        }
    }
    if (set.empty())
        return;

    // ---- scan by scan: every frame's scan c, located or not, in the launches of its key
    dev::DeviceBuffer d_descs, d_scratch;
    std::vector<ScanDesc> descs;
    std::vector<uint32_t> owner, order;
    std::vector<uint8_t> status;
    std::vector<uint64_t> ends;
    for (uint32_t c = 0; c < most_scans; ++c)
    {
        descs.clear();
        owner.clear();
        size_t scratch_total = 0;
        std::vector<size_t> scratch_at;
        for (uint32_t i = 0; i < set.size(); ++i)
        {
            Salvaged& s = set[i];
            if (c >= s.scans)
                continue;
            BatchFrame& x = win.fr[window_of[i]];
            ScanDesc d = s.first;
            d.pixels = s.first.pixels + c * s.plane_bytes;
            d.stream_capacity = 0; // not reached -- unless the reader stands behind a header of the same kind of scan
            if (s.reached && c != 0)
            {
                s.reached = false;
                try
                {
                    const ScanDesc next = desc_at(win, window_of[i], x, dests[s.frame]);
                    if (!x.done && x.reader.scan_interleave_mode() == 0 && x.reader.scan_component_count() == 1 &&
                        dev::salvage_candidate(next) && dev::salvage_launch_key(next) == dev::salvage_launch_key(s.first))
                    {
                        d = next;
                        s.reached = true;
                    }
                }
                catch (const error&)
                {
                }
            }
            else if (s.reached)
                d = s.first;
            scratch_at.push_back(scratch_total);
            scratch_total += dev::line_scratch_samples(d.width, d.interleave_mode, d.components) * sizeof(uint16_t);
            scratch_total = (scratch_total + 255) & ~size_t{255};
            descs.push_back(d);
            owner.push_back(i);
        }
        const uint32_t count = static_cast<uint32_t>(descs.size());
        if (count == 0)
            break;
        auto* scratch = static_cast<uint8_t*>(d_scratch.ensure(scratch_total));
        order.resize(count);
        for (uint32_t k = 0; k < count; ++k)
        {
            order[k] = k;
            descs[k].line_scratch = reinterpret_cast<uint16_t*>(scratch + scratch_at[k]);
        }
        std::stable_sort(order.begin(), order.end(),
                         [&](uint32_t a, uint32_t b) { return dev::salvage_launch_key(descs[a]) < dev::salvage_launch_key(descs[b]); });
        std::vector<ScanDesc> sorted(count);
        for (uint32_t k = 0; k < count; ++k)
            sorted[k] = descs[order[k]];
        d_descs.ensure(sizeof(ScanDesc) * count);
        hip_check(hipMemcpyAsync(d_descs.as<ScanDesc>(), sorted.data(), sizeof(ScanDesc) * count, hipMemcpyHostToDevice, stream));
        ends.assign(count, 0);
        for (uint32_t first = 0; first < count;)
        {
            uint32_t last = first + 1;
            while (last < count && dev::salvage_launch_key(sorted[last]) == dev::salvage_launch_key(sorted[first]))
                ++last;
            const uint32_t intervals = set[owner[order[first]]].intervals;
            status.assign(static_cast<size_t>(last - first) * intervals, 0);
            dev::launch_decode_salvage(sorted[first], d_descs.as<ScanDesc>() + first, last - first,
                                       dev::SalvageOutputs{fill_value, status.data(), ends.data() + first}, stream);
            for (uint32_t k = first; k < last; ++k)
            {
                Salvaged& s = set[owner[order[k]]];
                std::memcpy(s.status.data() + static_cast<size_t>(c) * intervals, status.data() + static_cast<size_t>(k - first) * intervals,
                            intervals);
            }
            first = last;
        }
        // ---- on to the next scan of the planar frames: its header is looked for where this scan's segment ends
        std::vector<uint32_t> which;
        std::vector<size_t> bases;
        for (uint32_t k = 0; k < count; ++k)
        {
            Salvaged& s = set[owner[order[k]]];
            if (!s.reached || c + 1 >= s.scans)
                continue;
            BatchFrame& x = win.fr[window_of[owner[order[k]]]];
            x.cursor += static_cast<size_t>(ends[k]);
            x.plane_offset += s.plane_bytes;
            which.push_back(window_of[owner[order[k]]]);
            bases.push_back(x.cursor);
        }
        win.parse_behind_scans(win.fr, which, bases, std::vector<uint8_t>(which.size(), 0));
    }

    // ---- reports, status bytes, counters
    for (const Salvaged& s : set)
    {
        charls_amd_salvage_report& r = reports[s.frame];
        r.state = 1;
        r.intervals = s.scans * s.intervals;
        for (uint32_t c = 0; c < s.scans; ++c)
            for (uint32_t j = 0; j < s.intervals; ++j)
            {
                if (s.status[static_cast<size_t>(c) * s.intervals + j] == 0)
                    continue;
                const uint32_t row = j * s.first.restart_interval;
                ++r.intervals_lost;
                r.rows_lost += std::min(s.first.restart_interval, s.first.height - row);
                r.first_lost_row = std::min(r.first_lost_row, row);
            }
        if (interval_status != nullptr)
        {
            if (status_pitch_bytes >= s.status.size())
                std::memcpy(interval_status + static_cast<size_t>(s.frame) * status_pitch_bytes, s.status.data(), s.status.size());
            else
                r.reserved = 1;
        }
        g_frames_salvaged.fetch_add(1);
        g_intervals_kept.fetch_add(r.intervals - r.intervals_lost);
        g_intervals_lost.fetch_add(r.intervals_lost);
    }
}

extern "C" charls_jpegls_errc charls_amd_decode_batch_device_salvage(uint32_t frame_count, const void* d_packed, const uint64_t* offsets,
                                                                     const uint64_t* sizes, const charls_amd_frame_dest* dests,
                                                                     uint32_t fill_value, charls_amd_codec_params* params_out,
                                                                     charls_amd_salvage_report* reports, uint8_t* interval_status,
                                                                     size_t status_pitch_bytes, charls_jpegls_errc* errcs, void* hip_stream)
try
{
    check_pointer(offsets);
    check_pointer(sizes);
    check_pointer(dests);
    check_pointer(errcs);
    check_pointer(reports);
    check_argument(interval_status == nullptr || status_pitch_bytes != 0);
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
    decode_batch_salvage(frame_count, d_packed, offsets, sizes, dests, fill_value, params_out, reports, interval_status, status_pitch_bytes,
                         errcs, hip_stream);
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}

extern "C" int32_t charls_amd_salvage_counters(uint64_t* out, int32_t capacity)
{
    const uint64_t v[4] = {g_frames_salvaged.load(), g_intervals_kept.load(), g_intervals_lost.load(), dev::salvage_kernel_launches()};
    int32_t n = 0;
    for (; out != nullptr && n < capacity && n < 4; ++n)
        out[n] = v[n];
    return n;
}
