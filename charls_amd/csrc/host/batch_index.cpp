// batch_index.cpp -- the seek-point index in the batch API (charls_amd.h part 2c): building the indexes of many
// device-resident streams in one call, decoding many frames through their indexes, decoding many row bands.
//
// Per frame the contract is part 1's (decoder_index.cpp), and the index is parsed, checked and written by the same
// functions (seek_index.h).  What is new is the shape of the work: all scans of a call that share the seek kernels'
// specialisation (sample width, components per pixel) are ONE launch over one ScanDesc array, one work list and one
// seek-point buffer, the resumed wavefronts store straight into the caller's frames or bands, and the segment hashes
// are computed where the streams are (device/segment_hash.hip).
//   build:  rounds per scan ordinal (scan c + 1 starts where scan c ended): one emit launch per group and round.
//   use:    the index names every segment's length, so the host walks to every SOS first; then one hash launch and
//           one resume launch per group for all scans of all frames.
//   bands:  as use, with the work items of decode_rows.
// A frame whose index does not hold, or that gets no seek points, is decoded in the same call by the ordinary launches
// (decode_batch_streams on every run of such frames).
//
// The three bodies (build_indexes, decode_through_indexes, decode_bands) take the streams as StreamWindows -- an offset per
// stream -- and a destination, capacity and stride per frame.  The slot calls of part 2c state i * pitch, the pitch and their
// one stride; the calls of part 2l hand over the caller's tables, and the index-only build hands over no destinations at all
// (index_packed_frames: pass A without pixels, pass B into scratch frames for the frames that get no seek points).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <functional>
#include <vector>

#include "../device/knobs.h"
#include "../device/runtime.h"
#include "../device/seek_decode.h"
#include "batch_streams.h"
#include "common.h"
#include "preset.h"
#include "seek_index.h"
#include "stream_reader.h"
#include "stream_windows.h"

using namespace jls;
using dev::hip_check;

namespace {

enum : int
{ // dev::seek_arena
    kArenaPoints = 0,
    kArenaWork = 1,
    kArenaDescs = 2,
    kArenaResults = 3,
    kArenaHash = 4,
    kArenaFrame = 5, // a whole frame of the bands' ordinary path
};

// GPU time of the seek launches and of the hash launches of the running call (charls_amd_last_timings [0] and [1]).
thread_local double t_seek_ms = 0, t_hash_ms = 0;
void timings_begin() noexcept
{
    t_seek_ms = t_hash_ms = 0;
}
void timings_end() noexcept
{
    dev::Timings& t = dev::last_timings();
    t.values[0] = t_seek_ms;
    t.values[1] = t_hash_ms;
    t.count = 2;
}

// The scan whose header x's reader has read, decoding to `dest` with the checks charls_amd_decode_batch_device makes
// (stride, extent).  No line scratch.  dest == nullptr (the index-only build): rows of minimal stride that go nowhere --
// decode_scans_wave_emit stores no row of a scan without pixels; no other kernel is handed such a scan.
ScanDesc frame_scan_desc(const StreamWindows& s, uint32_t i, const BatchFrame& x, const charls_amd_frame_dest* dest)
{
    const ScanSpec spec = scan_spec_of(x.reader);
    const auto [row, stride] = row_and_stride(x.reader, dest != nullptr ? dest->stride : 0);
    if (stride < row)
        raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_STRIDE);
    const size_t need = stride * spec.height - (stride - row); // (a scan of ILV_NONE is one component)
    if (dest != nullptr && dest->capacity_bytes < x.plane_offset + need)
        raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_SIZE);
    ScanDesc d = desc_of(spec);
    d.pixels = dest != nullptr ? static_cast<uint8_t*>(dest->d_pixels) + x.plane_offset : nullptr;
    d.pixel_stride = stride;
    d.stream = s.stream_ptr(i, x.cursor);
    d.stream_capacity = s.sizes[i] - x.cursor;
    d.line_scratch = nullptr; // (the seek kernels keep their lines in LDS)
    return d;
}

// The seek kernels store samples with the sample's width: 16-bit rows must start at even addresses (part 1's device rows
// are packed; here the base, the pitch and the stride are the caller's).
bool rows_aligned(const ScanDesc& d) noexcept
{
    return d.bits_per_sample <= 8 || ((reinterpret_cast<uintptr_t>(d.pixels) | d.pixel_stride) & 1u) == 0;
}

// Scans with the same key share a launch of the seek kernels; the dynamic LDS of a launch is its largest scan's.
uint32_t seek_group(const ScanDesc& d) noexcept
{
    return (d.bits_per_sample > 8 ? 8u : 0u) | static_cast<uint32_t>(d.interleave_mode == 2 ? d.components : 1);
}
size_t seek_line_bytes(const ScanDesc& d) noexcept
{
    return (d.interleave_mode == 0 ? 1u : static_cast<size_t>(d.components)) * (static_cast<size_t>(d.width) + 2) * (d.bits_per_sample > 8 ? 2 : 1);
}

// What one pass may keep in the device seek-point buffer: half of what the thread's work areas may still grow to.
size_t points_budget() noexcept
{
    return std::max<size_t>(dev::work_area_budget() / 2, size_t{64} << 20);
}

std::vector<uint32_t> sorted_by_group(const std::vector<ScanDesc>& descs)
{
    std::vector<uint32_t> order(descs.size());
    for (uint32_t k = 0; k < order.size(); ++k)
        order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return seek_group(descs[a]) < seek_group(descs[b]); });
    return order;
}

// decode_scans_wave_emit over descs[k], all k: results[k], and the seek points of scan k (point_totals[k] bytes) to
// points_out[k].  One launch per group and pass.
void run_emit(const std::vector<ScanDesc>& descs, const std::vector<size_t>& point_totals, const std::vector<uint8_t*>& points_out,
              uint32_t lines, std::vector<ScanResult>& results, hipStream_t stream)
{
    const uint32_t n = static_cast<uint32_t>(descs.size());
    results.assign(n, ScanResult{});
    const std::vector<uint32_t> order = sorted_by_group(descs);
    const size_t budget = points_budget();
    for (uint32_t first = 0; first < n;)
    {
        uint32_t last = first;
        size_t stride = 16;
        uint32_t proto = order[first];
        while (last < n && seek_group(descs[order[last]]) == seek_group(descs[order[first]]))
        {
            stride = std::max(stride, (point_totals[order[last]] + 15) & ~size_t{15});
            if (seek_line_bytes(descs[order[last]]) > seek_line_bytes(descs[proto]))
                proto = order[last];
            ++last;
        }
        const uint32_t per_pass = static_cast<uint32_t>(std::max<size_t>(1, std::min<size_t>(last - first, budget / stride)));
        for (uint32_t at = first; at < last; at += per_pass)
        {
            const uint32_t count = std::min(per_pass, last - at);
            std::vector<ScanDesc> pass(count);
            for (uint32_t k = 0; k < count; ++k)
                pass[k] = descs[order[at + k]];
            auto* d_points = static_cast<uint8_t*>(dev::seek_arena(kArenaPoints).ensure(stride * count));
            auto* d_descs = static_cast<ScanDesc*>(dev::seek_arena(kArenaDescs).ensure(dev::with_headroom(sizeof(ScanDesc) * count)));
            auto* d_results = static_cast<ScanResult*>(dev::seek_arena(kArenaResults).ensure(dev::with_headroom(sizeof(ScanResult) * count)));
            std::vector<ScanResult> got(count);
            hip_check(hipMemcpyAsync(d_descs, pass.data(), sizeof(ScanDesc) * count, hipMemcpyHostToDevice, stream));
            {
                EventTimer clock(stream, true);
                clock.start();
                dev::launch_seek_emit(descs[proto], d_descs, d_results, count, d_points, stride, lines, stream);
                clock.stop();
                add_index_counters(0, 0, 0, 1);
                hip_check(hipMemcpyAsync(got.data(), d_results, sizeof(ScanResult) * count, hipMemcpyDeviceToHost, stream));
                hip_check(hipStreamSynchronize(stream));
                t_seek_ms += clock.ms();
            }
            for (uint32_t k = 0; k < count; ++k)
            {
                const uint32_t scan = order[at + k];
                results[scan] = got[k];
                if (got[k].errc == kOk && point_totals[scan] != 0)
                    hip_check(hipMemcpyAsync(points_out[scan], d_points + stride * k, point_totals[scan], hipMemcpyDeviceToHost, stream));
            }
            hip_check(hipStreamSynchronize(stream));
        }
        first = last;
    }
}

// One scan of a resume launch: its seek points (host) and its work items, whose point offsets count from the scan's first
// point.
struct ResumeScan
{
    ScanDesc desc;
    const uint8_t* points{};
    size_t point_total{};
    std::vector<seek::SeekWork> work;
    std::vector<ScanResult> results; // beside work
};

// decode_scans_wave_resume over every work item of every scan.  One launch per group and pass.
void run_resume(std::vector<ResumeScan>& scans, hipStream_t stream)
{
    const uint32_t n = static_cast<uint32_t>(scans.size());
    std::vector<ScanDesc> descs(n);
    for (uint32_t k = 0; k < n; ++k)
        descs[k] = scans[k].desc;
    const std::vector<uint32_t> order = sorted_by_group(descs);
    const size_t budget = points_budget();
    for (uint32_t first = 0; first < n;)
    {
        // a pass: scans of one group whose points fit the budget (one scan always does)
        uint32_t last = first;
        size_t total = 0, items = 0;
        uint32_t proto = order[first];
        while (last < n && seek_group(descs[order[last]]) == seek_group(descs[order[first]]))
        {
            const size_t bytes = (scans[order[last]].point_total + 15) & ~size_t{15};
            if (last > first && total + bytes > budget)
                break;
            total += bytes;
            items += scans[order[last]].work.size();
            if (seek_line_bytes(descs[order[last]]) > seek_line_bytes(descs[proto]))
                proto = order[last];
            ++last;
        }
        const uint32_t count = last - first;
        auto* d_points = static_cast<uint8_t*>(dev::seek_arena(kArenaPoints).ensure(std::max<size_t>(total, 16)));
        auto* d_descs = static_cast<ScanDesc*>(dev::seek_arena(kArenaDescs).ensure(dev::with_headroom(sizeof(ScanDesc) * count)));
        auto* d_work = static_cast<seek::SeekWork*>(dev::seek_arena(kArenaWork).ensure(dev::with_headroom(sizeof(seek::SeekWork) * items)));
        auto* d_results = static_cast<ScanResult*>(dev::seek_arena(kArenaResults).ensure(dev::with_headroom(sizeof(ScanResult) * items)));
        std::vector<ScanDesc> pass(count);
        std::vector<seek::SeekWork> work;
        work.reserve(items);
        size_t at = 0;
        for (uint32_t k = 0; k < count; ++k)
        {
            const ResumeScan& s = scans[order[first + k]];
            pass[k] = s.desc;
            if (s.point_total != 0)
                hip_check(hipMemcpyAsync(d_points + at, s.points, s.point_total, hipMemcpyHostToDevice, stream));
            for (seek::SeekWork w : s.work)
            {
                w.scan = k;
                w.from_point += at;
                w.to_point += at;
                work.push_back(w);
            }
            at += (s.point_total + 15) & ~size_t{15};
        }
        std::vector<ScanResult> got(items);
        if (items != 0)
        {
            hip_check(hipMemcpyAsync(d_descs, pass.data(), sizeof(ScanDesc) * count, hipMemcpyHostToDevice, stream));
            hip_check(hipMemcpyAsync(d_work, work.data(), sizeof(seek::SeekWork) * items, hipMemcpyHostToDevice, stream));
            EventTimer clock(stream, true);
            clock.start();
            dev::launch_seek_resume(descs[proto], d_descs, d_work, d_results, static_cast<uint32_t>(items), d_points, stream);
            clock.stop();
            add_index_counters(0, items, 0, 1);
            hip_check(hipMemcpyAsync(got.data(), d_results, sizeof(ScanResult) * items, hipMemcpyDeviceToHost, stream));
            hip_check(hipStreamSynchronize(stream));
            t_seek_ms += clock.ms();
        }
        hip_check(hipStreamSynchronize(stream));
        size_t item = 0;
        for (uint32_t k = 0; k < count; ++k)
        {
            ResumeScan& s = scans[order[first + k]];
            s.results.assign(got.begin() + item, got.begin() + item + s.work.size());
            item += s.work.size();
        }
        first = last;
    }
}

// segment_hash of the bytes [offset, offset + bytes) of the slots, job by job, on the device.
std::vector<uint64_t> device_hashes(const StreamWindows& s, const std::vector<seek::HashJob>& jobs)
{
    const size_t n = jobs.size();
    std::vector<uint64_t> out(n);
    if (n == 0)
        return out;
    const size_t jobs_bytes = (sizeof(seek::HashJob) * n + 15) & ~size_t{15};
    auto* area = static_cast<uint8_t*>(dev::seek_arena(kArenaHash).ensure(dev::with_headroom(jobs_bytes + sizeof(uint64_t) * n)));
    hip_check(hipMemcpyAsync(area, jobs.data(), sizeof(seek::HashJob) * n, hipMemcpyHostToDevice, s.stream));
    EventTimer clock(s.stream, true);
    clock.start();
    dev::launch_segment_hash(s.slots, reinterpret_cast<const seek::HashJob*>(area), reinterpret_cast<uint64_t*>(area + jobs_bytes),
                             static_cast<uint32_t>(n), s.stream);
    clock.stop();
    hip_check(hipMemcpyAsync(out.data(), area + jobs_bytes, sizeof(uint64_t) * n, hipMemcpyDeviceToHost, s.stream));
    hip_check(hipStreamSynchronize(s.stream));
    t_hash_ms += clock.ms();
    return out;
}

// Every run of frames marked in `ordinary` through the batch decoder (batch_api.cpp: decode_batch_streams) with the streams'
// offsets and the frames' destinations as they are here.  params_out as charls_amd_decode_batch_device documents it
// (params_from: the lowest frame whose parameters it holds so far), or, `ragged`, as an array.
void decode_ordinary(const StreamWindows& s, const std::vector<uint8_t>& ordinary, const charls_amd_frame_dest* dests, bool ragged,
                     charls_amd_codec_params* params_out, uint32_t& params_from, charls_jpegls_errc* errcs)
{
    const uint32_t n = static_cast<uint32_t>(ordinary.size());
    for (uint32_t i = 0; i < n;)
    {
        if (!ordinary[i])
        {
            ++i;
            continue;
        }
        uint32_t last = i + 1;
        while (last < n && ordinary[last])
            ++last;
        charls_amd_codec_params got{};
        decode_batch_streams(last - i, s.slots, s.offsets() + i, s.sizes + i, BatchDests{dests + i, ragged, nullptr},
                             ragged ? (params_out != nullptr ? params_out + i : nullptr) : &got, errcs + i, s.stream);
        if (!ragged && params_out && got.frame_info.width != 0 && i < params_from)
        { // (the run's lowest frame that got as far as a scan is not known: no frame before the run's first can be it)
            *params_out = got;
            params_from = i;
        }
        i = last;
    }
}

// The frames of a slot call as a table of destinations: frame i at base + i * pitch, `pitch` bytes, one stride.
std::vector<charls_amd_frame_dest> slot_dests(uint32_t count, void* base, size_t pitch, uint32_t stride)
{
    std::vector<charls_amd_frame_dest> dests(count);
    for (uint32_t i = 0; i < count; ++i)
        dests[i] = charls_amd_frame_dest{static_cast<uint8_t*>(base) + i * pitch, pitch, stride, 0};
    return dests;
}

// set_index for every frame that has one: parsed[i] (empty scans: none), errors to the frame.
void parse_indexes(StreamWindows& s, const void* indexes, size_t index_pitch, const uint64_t* index_sizes, std::vector<SeekIndex>& parsed)
{
    const uint32_t n = static_cast<uint32_t>(s.fr.size());
    parsed.assign(n, SeekIndex{});
    for (uint32_t i = 0; i < n; ++i)
    {
        BatchFrame& x = s.fr[i];
        if (x.done || index_sizes[i] == 0)
            continue;
        try
        {
            check_argument(index_sizes[i] <= index_pitch, CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_SIZE);
            parsed[i] = parse_index(x.reader, static_cast<const uint8_t*>(indexes) + i * index_pitch, static_cast<size_t>(index_sizes[i]));
        }
        catch (const error& e)
        {
            x.errc = e.code;
            x.done = true;
        }
    }
}

// The walk over a frame's scans that an index allows: scan c starts at starts[c], its descriptor is descs[c].
struct Walk
{
    uint32_t frame{};
    std::vector<ScanDesc> descs;
    std::vector<ScanSpec> specs;
    std::vector<size_t> starts;
    bool ok{true};
    bool beyond{}; // a scan with seek points whose length, as the index has it, runs past the stream's end
};

} // namespace

// The whole-call checks the calls of part 2l share: the tables, the destinations where there are any, the offsets.  Raises;
// needs no device.  frame_count == 0 passes with any d_packed.
void jls::check_packed_index_call(uint32_t frame_count, const void* packed, const uint64_t* offsets, const uint64_t* sizes,
                                  const charls_amd_frame_dest* dests, const uint64_t* index_sizes, const charls_jpegls_errc* errcs)
{
    check_pointer(offsets);
    check_pointer(sizes);
    check_pointer(index_sizes);
    check_pointer(errcs);
    for (uint32_t f = 0; dests != nullptr && f < frame_count; ++f)
    {
        check_argument(dests[f].reserved == 0);
        check_buffer(dests[f].d_pixels, dests[f].capacity_bytes);
    }
    if (frame_count == 0)
        return;
    check_pointer(packed);
    for (uint32_t f = 0; f < frame_count; ++f)
    {
        uint64_t end;
        if (__builtin_add_overflow(offsets[f], sizes[f], &end))
            raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_SIZE);
    }
}

extern "C" charls_jpegls_errc charls_amd_index_size_bound(const charls_amd_codec_params* params, uint32_t lines_per_seek_point, size_t* bytes)
try
{
    check_pointer(params);
    check_pointer(bytes);
    check_argument(lines_per_seek_point > 0);
    const charls_frame_info& f = params->frame_info;
    check_argument(f.width >= 1 && f.height >= 1 && f.bits_per_sample >= kMinBits && f.bits_per_sample <= kMaxBits && f.component_count >= 1 &&
                   f.component_count <= kMaxComponents);
    check_argument(params->interleave_mode >= 0 && params->interleave_mode <= 2);
    check_argument(params->interleave_mode == 0 || f.component_count <= kMaxComponentsInScan);
    ScanSpec first{};
    first.width = f.width;
    first.height = f.height;
    first.components = params->interleave_mode == 0 ? 1 : f.component_count;
    first.interleave_mode = params->interleave_mode;
    first.bits_per_sample = f.bits_per_sample;
    first.near_lossless = params->near_lossless;
    first.color_transformation = params->color_transformation;
    first.restart_interval = params->restart_interval;
    if (!pc_validate(params->preset_coding_parameters, bit_max_value(f.bits_per_sample), params->near_lossless, &first.pc))
        raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT);
    const size_t scans = params->interleave_mode == 0 ? static_cast<size_t>(f.component_count) : 1u;
    *bytes = index_size_bound(first, scans, false, lines_per_seek_point);
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}

namespace {

// charls_amd_decode_batch_device_and_index behind its whole-call checks, on frames whose headers are read (s.read_headers).
// Frame i of `s` goes to dests[i]; what the call reports of it -- index, index size, errc, and params_out where `ragged` makes
// that an array -- goes to element slot_of[i] of the caller's arrays (slot_of == nullptr: element i).  `ragged`: the
// destinations are a table of the caller's own, checked against the whole frame before anything of it is decoded.
// dests == nullptr is the index-only build: every scan goes through the emit kernel without pixels.  A frame that gets no
// seek points there -- by its header, or for a scan it meets later -- is marked in `set_aside` and left to the caller, who
// gives it somewhere to decode to; what is reported of it here does not count.
void build_indexes(StreamWindows& s, const charls_amd_frame_dest* dests, bool ragged, uint32_t lines, const uint32_t* slot_of, void* indexes,
                   size_t index_pitch_bytes, uint64_t* index_sizes, charls_amd_codec_params* params_out, charls_jpegls_errc* errcs,
                   std::vector<uint8_t>* set_aside)
{
    const uint32_t frame_count = static_cast<uint32_t>(s.fr.size());
    const hipStream_t stream = s.stream;
    const auto out = [&](uint32_t i) { return slot_of != nullptr ? slot_of[i] : i; };
    const auto aside = [&](uint32_t i) {
        (*set_aside)[i] = 1;
        s.fr[i].done = true;
    };
    if (dests != nullptr && ragged)
        check_ragged_dests(s, BatchDests{dests, true, nullptr});

    struct Build
    {
        StreamReader header; // as read: write_index describes the frame by its first scan
        ScanSpec first{};
        SeekIndex index;
    };
    std::vector<Build> builds(frame_count);
    for (uint32_t i = 0; i < frame_count; ++i)
    {
        BatchFrame& x = s.fr[i];
        index_sizes[out(i)] = 0;
        if (x.done)
            continue;
        try
        { // (checked before decoding: nothing of a frame whose index cannot be kept is decoded)
            check_argument(index_pitch_bytes >= index_size_bound(x.reader, lines), CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_SIZE);
            builds[i].header = x.reader;
            builds[i].first = scan_spec_of(x.reader);
            builds[i].index.lines = lines;
            if (dests == nullptr && (x.reader.height_from_dnl() || !seek_spec_eligible(builds[i].first)))
                aside(i); // (by its header the frame gets no seek points: it needs somewhere to decode to)
        }
        catch (const error& e)
        {
            x.errc = e.code;
            x.done = true;
        }
    }

    // (the scans that get no seek points: the build call needs every scan's length, which charls_amd_decode_batch_device does
    // not report; the launcher's clock is not reported, so it must not fail the call)
    DecodeLauncher plain(stream, true);
    uint32_t params_from = UINT32_MAX;
    const auto stride_of = [&](uint32_t i) { return dests != nullptr ? dests[i].stride : 0u; };
    for (size_t scan_no = 0;; ++scan_no)
    {
        std::vector<uint32_t> emit_frames, plain_frames;
        std::vector<ScanDesc> emit_descs, plain_descs;
        std::vector<size_t> point_totals;
        std::vector<uint8_t*> points_out;
        for (uint32_t i = 0; i < frame_count; ++i)
        {
            BatchFrame& x = s.fr[i];
            if (x.done)
                continue;
            try
            {
                const ScanDesc d = frame_scan_desc(s, i, x, dests != nullptr ? dests + i : nullptr);
                if (params_out && ragged)
                    params_out[out(i)] = params_of(x.reader);
                else if (params_out && i < params_from)
                {
                    *params_out = params_of(x.reader);
                    params_from = i;
                }
                const ScanSpec spec = scan_spec_of(x.reader);
                Build& b = builds[i];
                b.index.scans.resize(scan_no + 1);
                IndexScan& rec = b.index.scans[scan_no];
                const bool eligible = !x.reader.height_from_dnl() && same_scan_parameters(spec, b.first) && seek_spec_eligible(spec) && rows_aligned(d);
                rec.points = eligible ? seek::points_per_scan(spec.height, lines) : 0u;
                if (dests == nullptr && !eligible)
                { // (an ordinary scan after all: the ordinary launch needs rows to store to)
                    aside(i);
                    continue;
                }
                rec.data.assign(static_cast<size_t>(rec.points) * seek_point_bytes(spec), 0);
                if (rec.points != 0 || dests == nullptr) // (without pixels a scan too short for a point goes this way too)
                {
                    emit_frames.push_back(i);
                    emit_descs.push_back(d);
                    point_totals.push_back(rec.data.size());
                    points_out.push_back(rec.data.data());
                }
                else
                {
                    plain_frames.push_back(i);
                    plain_descs.push_back(d);
                }
            }
            catch (const error& e)
            {
                x.errc = e.code;
                x.done = true;
            }
        }
        if (emit_frames.empty() && plain_frames.empty())
            break;
        std::vector<ScanResult> emit_results, plain_results;
        run_emit(emit_descs, point_totals, points_out, lines, emit_results, stream);
        plain.run(plain_descs, plain_results);

        // every scan's length and hash; then past it, to the next SOS or the end of the image
        std::vector<uint32_t> which;
        std::vector<size_t> bases;
        std::vector<uint8_t> last;
        std::vector<seek::HashJob> jobs;
        auto scan_done = [&](uint32_t i, const ScanResult& r) {
            BatchFrame& x = s.fr[i];
            if (r.errc != kOk)
            {
                x.errc = static_cast<charls_jpegls_errc>(r.errc);
                x.done = true;
                return;
            }
            if (r.bytes > s.sizes[i] - x.cursor)
            { // (cannot happen: a scan is decoded from the bytes of its stream; the hash kernel must not be handed more)
                x.errc = CHARLS_JPEGLS_ERRC_INVALID_DATA;
                x.done = true;
                return;
            }
            builds[i].index.scans[scan_no].segment_bytes = r.bytes;
            jobs.push_back(seek::HashJob{s.offset_of(i) + x.cursor, r.bytes});
            x.cursor += r.bytes;
            x.decoded_components += x.reader.scan_component_count();
            const bool end = x.decoded_components == x.reader.component_count();
            if (!end)
                x.plane_offset += row_and_stride(x.reader, stride_of(i)).stride * x.reader.frame_info().height;
            which.push_back(i);
            bases.push_back(x.cursor);
            last.push_back(end ? 1 : 0);
        };
        for (size_t k = 0; k < emit_frames.size(); ++k)
            scan_done(emit_frames[k], emit_results[k]);
        for (size_t k = 0; k < plain_frames.size(); ++k)
            scan_done(plain_frames[k], plain_results[k]);
        const std::vector<uint64_t> hashes = device_hashes(s, jobs);
        for (size_t k = 0; k < which.size(); ++k)
            builds[which[k]].index.scans[scan_no].hash = hashes[k];
        s.parse_behind_scans(s.fr, which, bases, last);
        for (size_t k = 0; k < which.size(); ++k)
        {
            BatchFrame& x = s.fr[which[k]];
            if (x.done || !last[k])
                continue;
            x.done = true; // the end of the image has been read: the index is the frame's
            try
            {
                index_sizes[out(which[k])] = write_index(builds[which[k]].header, builds[which[k]].index,
                                                         static_cast<uint8_t*>(indexes) + out(which[k]) * index_pitch_bytes, index_pitch_bytes);
            }
            catch (const error& e)
            {
                x.errc = e.code;
            }
        }
    }
    for (uint32_t i = 0; i < frame_count; ++i)
        errcs[out(i)] = s.fr[i].errc;
}

} // namespace

extern "C" charls_jpegls_errc charls_amd_decode_batch_device_and_index(uint32_t frame_count, const void* d_streams, size_t stream_pitch_bytes,
                                                                       const uint64_t* sizes, void* d_frames, size_t frame_pitch_bytes,
                                                                       uint32_t stride_arg, uint32_t lines, void* indexes,
                                                                       size_t index_pitch_bytes, uint64_t* index_sizes,
                                                                       charls_amd_codec_params* params_out, charls_jpegls_errc* errcs,
                                                                       void* hip_stream)
try
{
    check_pointer(sizes);
    check_pointer(errcs);
    check_pointer(index_sizes);
    check_argument(lines > 0);
    if (frame_count == 0)
        return CHARLS_JPEGLS_ERRC_SUCCESS;
    check_pointer(d_streams);
    check_pointer(d_frames);
    check_pointer(indexes);
    dev::require_device();
    auto stream = static_cast<hipStream_t>(hip_stream);
    const std::vector<uint64_t> stream_at = slot_offsets(frame_count, stream_pitch_bytes, sizes);
    const std::vector<charls_amd_frame_dest> dests = slot_dests(frame_count, d_frames, frame_pitch_bytes, stride_arg);
    StreamWindows s(frame_count, d_streams, stream_at.data(), sizes, stream);
    timings_begin();
    s.read_headers(true);
    build_indexes(s, dests.data(), false, lines, nullptr, indexes, index_pitch_bytes, index_sizes, params_out, errcs, nullptr);
    timings_end();
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}

namespace {

// The frames of `s` that have an index with seek points for every scan: the walk over their scans (every SOS parsed on a copy
// of the frame, `probe`).  A frame whose walk breaks off is left out (walks[k].ok = false).
void walk_indexed_frames(StreamWindows& s, const std::vector<SeekIndex>& parsed, std::vector<BatchFrame>& probe, std::vector<Walk>& walks,
                         const std::function<ScanDesc(uint32_t, const BatchFrame&, size_t)>& scan_desc, bool want_points)
{
    probe = s.fr;
    const uint32_t n = static_cast<uint32_t>(s.fr.size());
    for (uint32_t i = 0; i < n; ++i)
    {
        if (s.fr[i].done || parsed[i].scans.empty())
            continue;
        Walk w;
        w.frame = i;
        walks.push_back(std::move(w));
    }
    for (size_t c = 0;; ++c)
    {
        std::vector<uint32_t> which;
        std::vector<size_t> bases;
        std::vector<size_t> of_walk;
        for (size_t k = 0; k < walks.size(); ++k)
        {
            Walk& w = walks[k];
            const SeekIndex& index = parsed[w.frame];
            if (!w.ok || c >= index.scans.size() || w.descs.size() != c)
                continue;
            BatchFrame& y = probe[w.frame];
            try
            {
                const ScanSpec spec = scan_spec_of(y.reader);
                const IndexScan& rec = index.scans[c];
                if ((want_points && rec.points == 0) || rec.segment_bytes > s.sizes[w.frame] - y.cursor)
                {
                    w.beyond = rec.points != 0 && rec.segment_bytes > s.sizes[w.frame] - y.cursor;
                    w.ok = false;
                    continue;
                }
                w.descs.push_back(scan_desc(w.frame, y, c));
                w.specs.push_back(spec);
                w.starts.push_back(y.cursor);
                if (c + 1 < index.scans.size())
                {
                    y.plane_offset += w.descs.back().pixel_stride * spec.height;
                    which.push_back(w.frame);
                    bases.push_back(y.cursor + static_cast<size_t>(rec.segment_bytes));
                    of_walk.push_back(k);
                }
            }
            catch (const error&)
            {
                w.ok = false;
            }
        }
        if (which.empty())
            break;
        s.parse_behind_scans(probe, which, bases, std::vector<uint8_t>(which.size(), 0));
        for (size_t q = 0; q < which.size(); ++q)
            if (probe[which[q]].done)
                walks[of_walk[q]].ok = false;
    }
    for (Walk& w : walks)
        w.ok = w.ok && w.descs.size() == parsed[w.frame].scans.size();
}

} // namespace

namespace {

// charls_amd_decode_batch_device_indexed behind its whole-call checks, on frames whose headers are read: frame i of `s`
// through the index_sizes[i] bytes at indexes + i * index_pitch_bytes to dests[i].  `ragged`: the destinations are a table
// of the caller's own, checked against the whole frame up front, and params_out is an array.
void decode_through_indexes(StreamWindows& s, const void* indexes, size_t index_pitch_bytes, const uint64_t* index_sizes,
                            const charls_amd_frame_dest* dests, bool ragged, charls_amd_codec_params* params_out, charls_jpegls_errc* errcs)
{
    const uint32_t frame_count = static_cast<uint32_t>(s.fr.size());
    if (ragged)
        check_ragged_dests(s, BatchDests{dests, true, nullptr});
    std::vector<SeekIndex> parsed;
    parse_indexes(s, indexes, index_pitch_bytes, index_sizes, parsed);

    // ---- the frames that can go through their index: every scan has seek points and is one the seek kernels take
    std::vector<BatchFrame> probe;
    std::vector<Walk> walks;
    walk_indexed_frames(s, parsed, probe, walks,
                        [&](uint32_t i, const BatchFrame& y, size_t) { return frame_scan_desc(s, i, y, dests + i); }, true);
    std::vector<uint8_t> ordinary(frame_count, 0);
    std::vector<uint8_t> with_points(frame_count, 0); // the frame's index has seek points: decoding it from the top is a fallback
    for (uint32_t i = 0; i < frame_count; ++i)
    {
        ordinary[i] = !s.fr[i].done;
        for (const IndexScan& rec : parsed[i].scans)
            with_points[i] = with_points[i] || rec.points != 0;
    }
    std::vector<seek::HashJob> jobs;
    for (Walk& w : walks)
    {
        const BatchFrame& x = s.fr[w.frame];
        const ScanSpec first = scan_spec_of(x.reader);
        for (size_t c = 0; w.ok && c < w.descs.size(); ++c)
            w.ok = !x.reader.height_from_dnl() && same_scan_parameters(w.specs[c], first) && seek_spec_eligible(w.specs[c]) &&
                   rows_aligned(w.descs[c]);
        for (size_t c = 0; w.ok && c < w.descs.size(); ++c)
            jobs.push_back(seek::HashJob{s.offset_of(w.frame) + w.starts[c], parsed[w.frame].scans[c].segment_bytes});
    }
    {
        const std::vector<uint64_t> hashes = device_hashes(s, jobs);
        size_t job = 0;
        for (Walk& w : walks)
        {
            if (!w.ok)
                continue;
            for (size_t c = 0; c < w.descs.size(); ++c)
                if (hashes[job++] != parsed[w.frame].scans[c].hash)
                    w.ok = false;
        }
    }
    std::vector<ResumeScan> scans;
    std::vector<std::pair<uint32_t, uint32_t>> scan_of; // (walk, scan ordinal) of scans[k]
    for (uint32_t k = 0; k < walks.size(); ++k)
    {
        const Walk& w = walks[k];
        if (!w.ok)
            continue;
        const SeekIndex& index = parsed[w.frame];
        for (uint32_t c = 0; c < w.descs.size(); ++c)
        {
            ResumeScan r;
            r.desc = w.descs[c];
            r.points = index.scans[c].data.data();
            r.point_total = index.scans[c].data.size();
            const size_t point_bytes = seek_point_bytes(w.specs[c]);
            const uint32_t intervals = index.scans[c].points + 1;
            for (uint32_t i = 0; i < intervals; ++i)
            { // (ScanEngine::decode_scan_resumed's intervals)
                seek::SeekWork item{};
                item.first_row = i * index.lines;
                item.end_row = static_cast<uint32_t>(std::min<uint64_t>(w.specs[c].height, (static_cast<uint64_t>(i) + 1) * index.lines));
                item.store_from = item.first_row;
                item.row_base = 0;
                item.mode = i + 1 < intervals ? seek::kResumeCompare : seek::kResumeEnd;
                item.from_point = i == 0 ? 0 : (i - 1) * point_bytes;
                item.to_point = i + 1 < intervals ? i * point_bytes : 0;
                r.work.push_back(item);
            }
            scans.push_back(std::move(r));
            scan_of.emplace_back(k, c);
        }
    }
    run_resume(scans, s.stream);
    for (size_t k = 0; k < scans.size(); ++k)
    {
        Walk& w = walks[scan_of[k].first];
        const std::vector<ScanResult>& got = scans[k].results;
        for (size_t i = 0; i + 1 < got.size(); ++i)
            if (got[i].errc != kOk || (got[i].flags & seek::kSeekChecked) == 0 || (got[i].flags & seek::kSeekMismatch) != 0)
                w.ok = false;
        // (the last interval ends the scan where the index says the segment ends: the next SOS was read from there)
        if (got.back().errc != kOk || got.back().bytes != parsed[w.frame].scans[scan_of[k].second].segment_bytes)
            w.ok = false;
    }
    {
        std::vector<uint32_t> which;
        std::vector<size_t> bases;
        for (const Walk& w : walks)
        {
            if (!w.ok)
                continue;
            which.push_back(w.frame);
            bases.push_back(w.starts.back() + static_cast<size_t>(parsed[w.frame].scans.back().segment_bytes));
        }
        s.parse_behind_scans(probe, which, bases, std::vector<uint8_t>(which.size(), 1));
    }
    uint32_t params_from = UINT32_MAX;
    uint64_t from_points = 0, fallbacks = 0;
    for (const Walk& w : walks)
    {
        if (!w.ok || probe[w.frame].errc != CHARLS_JPEGLS_ERRC_SUCCESS)
            continue; // (decoded again below, which reports what part 1 reports)
        s.fr[w.frame].errc = CHARLS_JPEGLS_ERRC_SUCCESS;
        s.fr[w.frame].done = true;
        ordinary[w.frame] = 0;
        from_points += w.descs.size();
        if (params_out && ragged)
            params_out[w.frame] = params_of(s.fr[w.frame].reader);
        else if (params_out && w.frame < params_from)
        {
            *params_out = params_of(s.fr[w.frame].reader);
            params_from = w.frame;
        }
    }
    for (uint32_t i = 0; i < frame_count; ++i)
        fallbacks += ordinary[i] && with_points[i];
    add_index_counters(from_points, 0, fallbacks, 0);
    for (uint32_t i = 0; i < frame_count; ++i)
        errcs[i] = s.fr[i].errc;
    decode_ordinary(s, ordinary, dests, ragged, params_out, params_from, errcs);
}

} // namespace

extern "C" charls_jpegls_errc charls_amd_decode_batch_device_indexed(uint32_t frame_count, const void* d_streams, size_t stream_pitch_bytes,
                                                                     const uint64_t* sizes, const void* indexes, size_t index_pitch_bytes,
                                                                     const uint64_t* index_sizes, void* d_frames, size_t frame_pitch_bytes,
                                                                     uint32_t stride_arg, charls_amd_codec_params* params_out,
                                                                     charls_jpegls_errc* errcs, void* hip_stream)
try
{
    check_pointer(sizes);
    check_pointer(errcs);
    check_pointer(index_sizes);
    if (frame_count == 0)
        return CHARLS_JPEGLS_ERRC_SUCCESS;
    check_pointer(d_streams);
    check_pointer(d_frames);
    check_pointer(indexes);
    dev::require_device();
    auto stream = static_cast<hipStream_t>(hip_stream);
    const std::vector<uint64_t> stream_at = slot_offsets(frame_count, stream_pitch_bytes, sizes);
    const std::vector<charls_amd_frame_dest> dests = slot_dests(frame_count, d_frames, frame_pitch_bytes, stride_arg);
    StreamWindows s(frame_count, d_streams, stream_at.data(), sizes, stream);
    timings_begin();
    s.read_headers(true);
    decode_through_indexes(s, indexes, index_pitch_bytes, index_sizes, dests.data(), false, params_out, errcs);
    timings_end(); // (this call's seek and hash launches, not the ordinary launches of the frames that went that way)
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}

namespace {

// charls_amd_decode_rows_batch_device behind its whole-call checks, on frames whose headers are read: rows [first_rows[i],
// first_rows[i] + row_counts[i]) of frame i of `s` to bands[i], in decode_rows' layout at bands[i].stride.
void decode_bands(StreamWindows& s, const void* indexes, size_t index_pitch_bytes, const uint64_t* index_sizes, const uint32_t* first_rows,
                  const uint32_t* row_counts, const charls_amd_frame_dest* bands, charls_jpegls_errc* errcs)
{
    const uint32_t frame_count = static_cast<uint32_t>(s.fr.size());
    std::vector<SeekIndex> parsed;
    parse_indexes(s, indexes, index_pitch_bytes, index_sizes, parsed);

    // decode_rows' argument checks; the stride of every frame
    std::vector<size_t> strides(frame_count, 0);
    for (uint32_t i = 0; i < frame_count; ++i)
    {
        BatchFrame& x = s.fr[i];
        if (x.done)
            continue;
        try
        {
            const charls_frame_info& f = x.reader.frame_info();
            check_argument(row_counts[i] > 0 && first_rows[i] < f.height && row_counts[i] <= f.height - first_rows[i]);
            const ScanSpec first = scan_spec_of(x.reader);
            const size_t row_bytes = row_bytes_of(first);
            const size_t stride = bands[i].stride == 0 ? row_bytes : bands[i].stride;
            check_argument(stride >= row_bytes, CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_STRIDE);
            const size_t needed = checked_mul(checked_mul(stride, row_counts[i]), scans_of_frame(x.reader)) - (stride - row_bytes);
            check_argument(bands[i].capacity_bytes >= needed, CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_SIZE);
            strides[i] = stride;
        }
        catch (const error& e)
        {
            x.errc = e.code;
            x.done = true;
        }
    }
    auto band_desc = [&](uint32_t i, const BatchFrame& y, size_t c) {
        ScanDesc d = desc_of(scan_spec_of(y.reader));
        d.pixels = static_cast<uint8_t*>(bands[i].d_pixels) + strides[i] * row_counts[i] * c;
        d.pixel_stride = strides[i];
        d.stream = s.stream_ptr(i, y.cursor);
        d.stream_capacity = s.sizes[i] - y.cursor;
        d.line_scratch = nullptr;
        return d;
    };

    // ---- frames on the seek kernels: every scan is reached through the index (or the frame has one scan) and is one the
    // kernels take; the others are decoded whole on the ordinary path
    std::vector<BatchFrame> probe;
    std::vector<Walk> walks;
    walk_indexed_frames(s, parsed, probe, walks, band_desc, false);
    std::vector<uint8_t> whole(frame_count, 0), walked(frame_count, 0);
    for (const Walk& w : walks)
        walked[w.frame] = 1;
    for (uint32_t i = 0; i < frame_count; ++i)
    {
        const BatchFrame& x = s.fr[i];
        if (x.done || walked[i])
            continue;
        if (scans_of_frame(x.reader) == 1)
        { // no index: one scan from the top
            Walk w;
            w.frame = i;
            w.descs.push_back(band_desc(i, x, 0));
            w.specs.push_back(scan_spec_of(x.reader));
            w.starts.push_back(x.cursor);
            walks.push_back(std::move(w));
        }
        else
            whole[i] = 1;
    }
    std::vector<seek::HashJob> jobs;
    for (Walk& w : walks)
    {
        const BatchFrame& x = s.fr[w.frame];
        const SeekIndex& index = parsed[w.frame];
        for (size_t c = 0; w.ok && c < w.descs.size(); ++c)
            w.ok = !x.reader.height_from_dnl() && seek_spec_eligible(w.specs[c]) && rows_aligned(w.descs[c]);
        // (a planar frame is walked by the lengths the index names: every one of them must be the segment's, so every scan's
        // hash is checked, not only those of scans with seek points)
        for (size_t c = 0; w.ok && c < index.scans.size(); ++c)
            if (index.scans[c].points != 0 || index.scans.size() > 1)
                jobs.push_back(seek::HashJob{s.offset_of(w.frame) + w.starts[c], index.scans[c].segment_bytes});
        if (!w.ok)
            whole[w.frame] = 1;
    }
    {
        const std::vector<uint64_t> hashes = device_hashes(s, jobs);
        size_t job = 0;
        for (Walk& w : walks)
        {
            if (!w.ok)
                continue;
            const SeekIndex& index = parsed[w.frame];
            for (size_t c = 0; c < index.scans.size(); ++c)
                if ((index.scans[c].points != 0 || index.scans.size() > 1) && hashes[job++] != index.scans[c].hash && w.ok)
                { // a band cannot be checked by chaining: the index must belong to this very segment
                    w.ok = false;
                    s.fr[w.frame].errc = CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT;
                    s.fr[w.frame].done = true;
                }
        }
    }
    // (a walk that broke off on a frame with an index: the length of a segment beyond the stream is what decode_rows
    // refuses as invalid_argument; anything else is the whole-frame path's to report)
    for (Walk& w : walks)
    {
        if (w.ok || s.fr[w.frame].done)
            continue;
        if (w.beyond)
        {
            s.fr[w.frame].errc = CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT;
            s.fr[w.frame].done = true;
            whole[w.frame] = 0;
        }
        else
            whole[w.frame] = 1;
    }

    std::vector<ResumeScan> scans;
    std::vector<uint32_t> walk_of;
    uint64_t from_points = 0;
    for (uint32_t k = 0; k < walks.size(); ++k)
    {
        const Walk& w = walks[k];
        if (!w.ok || s.fr[w.frame].done)
            continue;
        const SeekIndex& index = parsed[w.frame];
        const ScanSpec first = scan_spec_of(s.fr[w.frame].reader);
        const uint32_t first_row = first_rows[w.frame], rows = row_counts[w.frame], end = first_row + rows;
        for (uint32_t c = 0; c < w.descs.size(); ++c)
        {
            ResumeScan r;
            r.desc = w.descs[c];
            const bool use = c < index.scans.size() && index.scans[c].points != 0 && same_scan_parameters(w.specs[c], first);
            const uint32_t lines = use ? index.lines : 0;
            const uint32_t count = use ? index.scans[c].points : 0u;
            if (use)
            {
                r.points = index.scans[c].data.data();
                r.point_total = index.scans[c].data.size();
                ++from_points;
            }
            const size_t point_bytes = seek_point_bytes(w.specs[c]);
            // (ScanEngine::decode_scan_band's work items: every interval the band touches is a wavefront of its own)
            const uint32_t from = count != 0 ? std::min(first_row / lines, count) : 0u;
            const uint32_t to = count != 0 ? std::min((end - 1) / lines, count) : 0u;
            for (uint32_t i = from; i <= to; ++i)
            {
                seek::SeekWork item{};
                item.first_row = i * lines;
                item.end_row = i == to ? end : std::min(end, (i + 1) * lines);
                item.store_from = std::max(first_row, item.first_row);
                item.row_base = first_row;
                item.mode = seek::kResumeBand;
                item.from_point = i == 0 ? 0 : (i - 1) * point_bytes;
                r.work.push_back(item);
            }
            scans.push_back(std::move(r));
            walk_of.push_back(k);
        }
    }
    run_resume(scans, s.stream);
    add_index_counters(from_points, 0, 0, 0);
    for (size_t k = 0; k < scans.size(); ++k)
    {
        BatchFrame& x = s.fr[walks[walk_of[k]].frame];
        for (const ScanResult& r : scans[k].results) // (the first error from the top of the band down, scan by scan)
            if (r.errc != kOk && x.errc == CHARLS_JPEGLS_ERRC_SUCCESS)
                x.errc = static_cast<charls_jpegls_errc>(r.errc);
        x.done = true;
    }
    for (uint32_t i = 0; i < frame_count; ++i)
        errcs[i] = s.fr[i].errc;

    // ---- the others: the whole frame on the ordinary path into a work area, the band copied out
    for (uint32_t i = 0; i < frame_count; ++i)
    {
        if (!whole[i] || s.fr[i].done)
            continue;
        const BatchFrame& x = s.fr[i];
        const charls_frame_info& f = x.reader.frame_info();
        const size_t row_bytes = row_and_stride(x.reader, 0).row;
        const size_t scans_n = scans_of_frame(x.reader);
        const size_t frame_bytes = checked_mul(checked_mul(row_bytes, f.height), scans_n);
        auto* area = static_cast<uint8_t*>(dev::seek_arena(kArenaFrame).ensure(frame_bytes));
        const charls_amd_frame_dest whole_frame{area, frame_bytes, 0, 0};
        decode_batch_streams(1, s.slots, s.offsets() + i, s.sizes + i, BatchDests{&whole_frame, false, nullptr}, nullptr, errcs + i, s.stream);
        if (errcs[i] != CHARLS_JPEGLS_ERRC_SUCCESS)
            continue;
        for (size_t c = 0; c < scans_n; ++c)
            hip_check(hipMemcpy2DAsync(static_cast<uint8_t*>(bands[i].d_pixels) + strides[i] * row_counts[i] * c, strides[i],
                                       area + row_bytes * f.height * c + row_bytes * first_rows[i], row_bytes, row_bytes, row_counts[i],
                                       hipMemcpyDeviceToDevice, s.stream));
        hip_check(hipStreamSynchronize(s.stream));
    }
}

} // namespace

// The body above for a caller in another unit (batch_bands.cpp: the frames its marker route leaves or gives back), with the
// timings of a call of its own.
void jls::decode_row_bands(StreamWindows& s, const void* indexes, size_t index_pitch_bytes, const uint64_t* index_sizes,
                           const uint32_t* first_rows, const uint32_t* row_counts, const charls_amd_frame_dest* bands,
                           charls_jpegls_errc* errcs)
{
    timings_begin();
    decode_bands(s, indexes, index_pitch_bytes, index_sizes, first_rows, row_counts, bands, errcs);
    timings_end();
}

extern "C" charls_jpegls_errc charls_amd_decode_rows_batch_device(uint32_t frame_count, const void* d_streams, size_t stream_pitch_bytes,
                                                                  const uint64_t* sizes, const void* indexes, size_t index_pitch_bytes,
                                                                  const uint64_t* index_sizes, const uint32_t* first_rows,
                                                                  const uint32_t* row_counts, void* d_bands, size_t band_pitch_bytes,
                                                                  uint32_t stride_arg, charls_jpegls_errc* errcs, void* hip_stream)
try
{
    check_pointer(sizes);
    check_pointer(errcs);
    check_pointer(index_sizes);
    check_pointer(first_rows);
    check_pointer(row_counts);
    if (frame_count == 0)
        return CHARLS_JPEGLS_ERRC_SUCCESS;
    check_pointer(d_streams);
    check_pointer(d_bands);
    dev::require_device();
    auto stream = static_cast<hipStream_t>(hip_stream);
    const std::vector<uint64_t> stream_at = slot_offsets(frame_count, stream_pitch_bytes, sizes);
    for (uint32_t i = 0; i < frame_count; ++i)
        if (index_sizes[i] != 0)
            check_pointer(indexes);
    const std::vector<charls_amd_frame_dest> bands = slot_dests(frame_count, d_bands, band_pitch_bytes, stride_arg);
    StreamWindows s(frame_count, d_streams, stream_at.data(), sizes, stream);
    timings_begin();
    s.read_headers(true);
    decode_bands(s, indexes, index_pitch_bytes, index_sizes, first_rows, row_counts, bands.data(), errcs);
    timings_end();
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}

// ---- part 2l: the same three bodies on a packed blob, with the caller's table of destinations or with none ------------------

// The index-only build behind its whole-call checks (frame_count >= 1, a device is there; timings are the caller's).
//   Pass A: every frame that by its header is all seek points, through the emit kernel without pixels.
//   Pass B: the frames pass A set aside -- no seek points by their header, or an ordinary scan met later --, through the same
//           body into scratch frames, window by window: dev::index_scratch_arena, a quarter of what the thread's work areas may
//           grow to (as the frame area of part 2j), or INDEX_WINDOW_FRAMES frames.  A frame that cannot be given a scratch
//           frame gets not_enough_memory.
void jls::index_packed_frames(uint32_t frame_count, const void* d_packed, const uint64_t* offsets, const uint64_t* sizes, uint32_t lines,
                              void* indexes, size_t index_pitch_bytes, uint64_t* index_sizes, charls_amd_codec_params* params_out,
                              charls_jpegls_errc* errcs, void* hip_stream)
{
    constexpr size_t kFrameAlignment = 256; // (a scratch frame starts on one: 16-bit rows are never at an odd address)
    auto stream = static_cast<hipStream_t>(hip_stream);
    if (params_out != nullptr)
        std::fill(params_out, params_out + frame_count, charls_amd_codec_params{});
    std::vector<uint8_t> aside(frame_count, 0);
    std::vector<uint32_t> later;  // the frames of pass B, in the caller's order
    std::vector<size_t> want;     // what each takes in the area
    std::vector<uint64_t> bytes;  // its frame, packed
    {
        StreamWindows s(frame_count, d_packed, offsets, sizes, stream);
        s.read_headers(true);
        build_indexes(s, nullptr, true, lines, nullptr, indexes, index_pitch_bytes, index_sizes, params_out, errcs, &aside);
        for (uint32_t f = 0; f < frame_count; ++f)
        {
            if (!aside[f])
                continue;
            index_sizes[f] = 0;
            try
            {
                const charls_frame_info& fi = s.fr[f].reader.frame_info();
                const size_t frame = checked_mul(checked_mul(checked_mul(static_cast<size_t>(fi.component_count), fi.height), fi.width),
                                                 bytes_per_sample(fi.bits_per_sample));
                later.push_back(f);
                bytes.push_back(frame);
                want.push_back(checked_mul(frame / kFrameAlignment + 1, kFrameAlignment));
            }
            catch (const error& e)
            {
                errcs[f] = e.code;
            }
        }
    }
    if (later.empty())
        return;

    // ---- the windows of pass B, planned as those of transcode_frames are
    const uint32_t n_later = static_cast<uint32_t>(later.size());
    const size_t budget = dev::work_area_budget();
    const long long forced = knobs::get_or(knobs::kIndexWindowFrames, 0);
    size_t room = forced >= 1 ? SIZE_MAX : std::max<size_t>(budget / 4, 1);
    uint32_t most = forced >= 1 ? static_cast<uint32_t>(std::min<long long>(forced, n_later)) : n_later;
    std::vector<uint32_t> window_end; // one past the last frame of every window (positions in `later`)
    uint8_t* area = nullptr;
    const bool limited = dev::workspace_limit() != 0 && budget < *std::max_element(want.begin(), want.end());
    while (!limited)
    {
        window_end.clear();
        size_t filled = 0, most_filled = 0;
        uint32_t held = 0;
        for (uint32_t k = 0; k < n_later; ++k)
        {
            if (held != 0 && (held == most || want[k] > room - std::min(filled, room)))
            {
                window_end.push_back(k);
                most_filled = std::max(most_filled, filled);
                filled = 0;
                held = 0;
            }
            filled += want[k];
            ++held;
        }
        window_end.push_back(n_later);
        most_filled = std::max(most_filled, filled);
        area = static_cast<uint8_t*>(dev::try_ensure(dev::index_scratch_arena(), most_filled + kFrameAlignment));
        if (area != nullptr || window_end.size() == n_later) // (windows of one frame each: nothing smaller to ask for)
            break;
        room = std::max<size_t>(room / 2, 1);
        most = (most + 1) / 2;
    }
    if (area == nullptr)
    {
        for (const uint32_t f : later)
            errcs[f] = CHARLS_JPEGLS_ERRC_NOT_ENOUGH_MEMORY;
        return;
    }
    std::vector<uint64_t> w_offsets, w_sizes;
    std::vector<charls_amd_frame_dest> w_dests;
    for (uint32_t w = 0, first = 0; w < window_end.size(); first = window_end[w++])
    {
        const uint32_t n = window_end[w] - first;
        w_offsets.resize(n);
        w_sizes.resize(n);
        w_dests.resize(n);
        size_t at = 0;
        for (uint32_t k = 0; k < n; ++k)
        {
            const uint32_t f = later[first + k];
            w_offsets[k] = offsets[f];
            w_sizes[k] = sizes[f];
            w_dests[k] = charls_amd_frame_dest{area + at, bytes[first + k], 0, 0};
            at += want[first + k];
        }
        StreamWindows s(n, d_packed, w_offsets.data(), w_sizes.data(), stream);
        s.read_headers(true);
        build_indexes(s, w_dests.data(), true, lines, later.data() + first, indexes, index_pitch_bytes, index_sizes, params_out, errcs, nullptr);
    }
}

extern "C" charls_jpegls_errc charls_amd_index_batch_device_packed(uint32_t frame_count, const void* d_packed, const uint64_t* offsets,
                                                                   const uint64_t* sizes, const charls_amd_frame_dest* dests, uint32_t lines,
                                                                   void* indexes, size_t index_pitch_bytes, uint64_t* index_sizes,
                                                                   charls_amd_codec_params* params_out, charls_jpegls_errc* errcs,
                                                                   void* hip_stream)
try
{
    check_packed_index_call(frame_count, d_packed, offsets, sizes, dests, index_sizes, errcs);
    check_argument(lines > 0);
    if (frame_count == 0)
        return CHARLS_JPEGLS_ERRC_SUCCESS;
    check_pointer(indexes);
    dev::require_device();
    timings_begin();
    if (dests == nullptr)
        index_packed_frames(frame_count, d_packed, offsets, sizes, lines, indexes, index_pitch_bytes, index_sizes, params_out, errcs, hip_stream);
    else
    {
        if (params_out != nullptr)
            std::fill(params_out, params_out + frame_count, charls_amd_codec_params{});
        StreamWindows s(frame_count, d_packed, offsets, sizes, static_cast<hipStream_t>(hip_stream));
        s.read_headers(true);
        build_indexes(s, dests, true, lines, nullptr, indexes, index_pitch_bytes, index_sizes, params_out, errcs, nullptr);
    }
    timings_end();
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}

extern "C" charls_jpegls_errc charls_amd_decode_batch_device_ragged_indexed(uint32_t frame_count, const void* d_packed, const uint64_t* offsets,
                                                                            const uint64_t* sizes, const void* indexes,
                                                                            size_t index_pitch_bytes, const uint64_t* index_sizes,
                                                                            const charls_amd_frame_dest* dests,
                                                                            charls_amd_codec_params* params_out, charls_jpegls_errc* errcs,
                                                                            void* hip_stream)
try
{
    check_pointer(dests);
    check_packed_index_call(frame_count, d_packed, offsets, sizes, dests, index_sizes, errcs);
    if (frame_count == 0)
        return CHARLS_JPEGLS_ERRC_SUCCESS;
    check_pointer(indexes);
    dev::require_device();
    if (params_out != nullptr)
        std::fill(params_out, params_out + frame_count, charls_amd_codec_params{});
    StreamWindows s(frame_count, d_packed, offsets, sizes, static_cast<hipStream_t>(hip_stream));
    timings_begin();
    s.read_headers(true);
    decode_through_indexes(s, indexes, index_pitch_bytes, index_sizes, dests, true, params_out, errcs);
    timings_end(); // (this call's seek and hash launches, not the ordinary launches of the frames that went that way)
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}

extern "C" charls_jpegls_errc charls_amd_decode_rows_batch_device_ragged(uint32_t frame_count, const void* d_packed, const uint64_t* offsets,
                                                                         const uint64_t* sizes, const void* indexes, size_t index_pitch_bytes,
                                                                         const uint64_t* index_sizes, const uint32_t* first_rows,
                                                                         const uint32_t* row_counts, const charls_amd_frame_dest* bands,
                                                                         charls_jpegls_errc* errcs, void* hip_stream)
try
{
    check_pointer(bands);
    check_pointer(first_rows);
    check_pointer(row_counts);
    check_packed_index_call(frame_count, d_packed, offsets, sizes, bands, index_sizes, errcs);
    if (frame_count == 0)
        return CHARLS_JPEGLS_ERRC_SUCCESS;
    for (uint32_t f = 0; f < frame_count; ++f)
        if (index_sizes[f] != 0)
            check_pointer(indexes);
    dev::require_device();
    StreamWindows s(frame_count, d_packed, offsets, sizes, static_cast<hipStream_t>(hip_stream));
    timings_begin();
    s.read_headers(true);
    decode_bands(s, indexes, index_pitch_bytes, index_sizes, first_rows, row_counts, bands, errcs);
    timings_end();
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}
