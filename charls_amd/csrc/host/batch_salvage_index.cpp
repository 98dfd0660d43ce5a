// batch_salvage_index.cpp -- salvage decode through the seek-point index (charls_amd.h part 2h): what the
// salvage call of part 2g (batch_salvage.cpp) leaves failed because the stream has no restart intervals.
//
//  * Rounds 1 and 2 of part 2g are decode_batch_salvage, untouched: a frame it decodes has state 0, a frame it salvages by its
//    restart intervals state 1, and their results are that call's.
//  * Index mode.  A frame left in state 2 that has a usable index is cut at the index's seek points: interval i of scan c
//    starts from the scan's initial state or from point i (decode_scans_wave_resume) and is kept when it ends in the state of
//    point i + 1 -- the last one: when it ends the scan with the bytes consumed that the index names.  The segment hash is
//    not asked: it cannot match.  Scan c + 1 of a planar frame starts where the index says scan c ends.
//  * Prefix mode (CHARLS_AMD_SALVAGE_PREFIX, no usable index).  The frame is decoded from the top, scan by scan, on the same
//    kernel (seek::kResumePrefix): the rows before the first error stay, the rest is filled.
//  The verdicts and the fill are judge_and_fill's (dev::launch_salvage_fill).  One launch of either kernel per group of scans
//  that share the seek kernels' specialisation, row length, height and interval length, and per pass over the seek-point
//  budget (batch_index.cpp's).  The buffers are the calling thread's seek arenas.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <tuple>
#include <vector>

#include "../device/runtime.h"
#include "../device/seek_decode.h"
#include "batch_streams.h"
#include "common.h"
#include "event_timer.h"
#include "seek_index.h"
#include "stream_windows.h"

using namespace jls;
using dev::hip_check;

namespace {

// charls_amd_salvage_index_counters
std::atomic<uint64_t> g_frames_by_index{0}, g_kept_proven{0}, g_kept_on_index{0}, g_lost{0}, g_frames_by_prefix{0}, g_launches{0};

constexpr uint32_t kNoRow = UINT32_MAX;
constexpr uint32_t kFlagPrefix = CHARLS_AMD_SALVAGE_PREFIX;

enum : int
{ // dev::seek_arena, in the roles batch_index.cpp gives them; the expected values and status bytes share the hash jobs' area
    kArenaPoints = 0,
    kArenaWork = 1,
    kArenaDescs = 2,
    kArenaResults = 3,
    kArenaVerdicts = 4,
};

enum : uint8_t
{ // status bytes (salvage_intervals.hip)
    kKept = 0,
    kLost = 2,
    kNotReached = 3,
    kOnTheIndex = 4,
    kPrefix = 5,
};

// One scan of a launch: N intervals of `lines` rows (prefix mode: one interval of all its rows).
struct Item
{
    ScanDesc desc;               // stream_capacity 0: not reached
    uint32_t lines{}, intervals{};
    const uint8_t* points{};     // HOST: the scan's seek points (index mode)
    size_t point_total{};
    std::vector<seek::SeekWork> work; // `intervals` of them; point offsets count from the scan's first point
    std::vector<uint64_t> expect;
    std::vector<uint8_t> status;      // in: 0 launched, 3 not; out: the verdicts
    std::vector<ScanResult> results;  // out
};

bool rows_aligned(const ScanDesc& d) noexcept
{ // (the seek kernels store samples with the sample's width)
    return d.bits_per_sample <= 8 || ((reinterpret_cast<uintptr_t>(d.pixels) | d.pixel_stride) & 1u) == 0;
}

// Scans with equal keys share a launch of both kernels: the resume kernel's specialisation and LDS, judge_and_fill's row
// length and interval count.
struct GroupKey
{
    uint32_t kind;
    uint32_t width, height, lines;
    bool operator<(const GroupKey& o) const noexcept
    {
        return std::tie(kind, width, height, lines) < std::tie(o.kind, o.width, o.height, o.lines);
    }
    bool operator==(const GroupKey& o) const noexcept { return !(*this < o) && !(o < *this); }
};
GroupKey key_of(const Item& it) noexcept
{
    const ScanDesc& d = it.desc;
    const uint32_t planes = d.interleave_mode == 0 ? 1u : static_cast<uint32_t>(d.components);
    return GroupKey{(d.bits_per_sample > 8 ? 64u : 0u) | (static_cast<uint32_t>(d.interleave_mode) << 4) | planes, d.width, d.height,
                    it.lines};
}

size_t points_budget() noexcept
{
    return std::max<size_t>(dev::work_area_budget() / 2, size_t{64} << 20);
}

// A no-op work item: an interval that is not launched still has its place in the result array.
seek::SeekWork idle_work() noexcept
{
    seek::SeekWork w{};
    w.mode = seek::kResumeBand; // rows [0, 0) from the initial state
    return w;
}

// decode_scans_wave_resume over every work item of every scan, then judge_and_fill over the results.  `device_ms`: the time
// of the launches by device events.
void run_items(std::vector<Item>& items, uint32_t fill_value, uint32_t rule, hipStream_t stream, double& device_ms)
{
    const uint32_t n = static_cast<uint32_t>(items.size());
    std::vector<uint32_t> order(n);
    for (uint32_t k = 0; k < n; ++k)
        order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key_of(items[a]) < key_of(items[b]); });
    const size_t budget = points_budget();
    for (uint32_t first = 0; first < n;)
    {
        // a pass: scans of one group whose points fit the budget (one scan always does)
        const GroupKey key = key_of(items[order[first]]);
        const uint32_t intervals = items[order[first]].intervals;
        uint32_t last = first;
        size_t total = 0;
        while (last < n && key_of(items[order[last]]) == key)
        {
            const size_t bytes = (items[order[last]].point_total + 15) & ~size_t{15};
            if (last > first && total + bytes > budget)
                break;
            total += bytes;
            ++last;
        }
        const uint32_t count = last - first;
        const size_t slots = static_cast<size_t>(count) * intervals;
        if (slots > 0x7FFFFFFFu)
            raise(CHARLS_JPEGLS_ERRC_NOT_ENOUGH_MEMORY);
        auto* d_points = static_cast<uint8_t*>(dev::seek_arena(kArenaPoints).ensure(std::max<size_t>(total, 16)));
        // the scans as the decoder takes them, and behind them the copies that carry the interval length for judge_and_fill
        auto* d_descs = static_cast<ScanDesc*>(dev::seek_arena(kArenaDescs).ensure(dev::with_headroom(sizeof(ScanDesc) * 2 * count)));
        auto* d_work = static_cast<seek::SeekWork*>(dev::seek_arena(kArenaWork).ensure(dev::with_headroom(sizeof(seek::SeekWork) * slots)));
        auto* d_results = static_cast<ScanResult*>(dev::seek_arena(kArenaResults).ensure(dev::with_headroom(sizeof(ScanResult) * slots)));
        auto* d_verdicts = static_cast<uint8_t*>(dev::seek_arena(kArenaVerdicts).ensure(dev::with_headroom(sizeof(uint64_t) * slots + slots)));
        auto* d_expect = reinterpret_cast<uint64_t*>(d_verdicts);
        uint8_t* d_status = d_verdicts + sizeof(uint64_t) * slots;

        std::vector<ScanDesc> descs(2 * static_cast<size_t>(count));
        std::vector<seek::SeekWork> work;
        std::vector<uint64_t> expect;
        std::vector<uint8_t> status;
        work.reserve(slots);
        expect.reserve(slots);
        status.reserve(slots);
        size_t at = 0;
        for (uint32_t k = 0; k < count; ++k)
        {
            const Item& it = items[order[first + k]];
            descs[k] = it.desc;
            descs[k].restart_interval = 0;
            descs[k].line_scratch = nullptr; // (the seek kernels keep their lines in LDS)
            descs[count + k] = it.desc;
            descs[count + k].restart_interval = it.lines;
            if (it.point_total != 0)
                hip_check(hipMemcpyAsync(d_points + at, it.points, it.point_total, hipMemcpyHostToDevice, stream));
            for (seek::SeekWork w : it.work)
            {
                w.scan = k;
                w.from_point += at;
                w.to_point += at;
                work.push_back(w);
            }
            expect.insert(expect.end(), it.expect.begin(), it.expect.end());
            status.insert(status.end(), it.status.begin(), it.status.end());
            at += (it.point_total + 15) & ~size_t{15};
        }
        hip_check(hipMemcpyAsync(d_descs, descs.data(), sizeof(ScanDesc) * descs.size(), hipMemcpyHostToDevice, stream));
        hip_check(hipMemcpyAsync(d_work, work.data(), sizeof(seek::SeekWork) * slots, hipMemcpyHostToDevice, stream));
        hip_check(hipMemcpyAsync(d_expect, expect.data(), sizeof(uint64_t) * slots, hipMemcpyHostToDevice, stream));
        hip_check(hipMemcpyAsync(d_status, status.data(), slots, hipMemcpyHostToDevice, stream));
        std::vector<ScanResult> got(slots);
        {
            EventTimer clock(stream, true);
            clock.start();
            dev::launch_seek_resume(descs[0], d_descs, d_work, d_results, static_cast<uint32_t>(slots), d_points, stream);
            dev::launch_salvage_fill(items[order[first]].desc, d_descs + count, count, intervals, d_results, d_expect, d_status, fill_value,
                                     rule, stream);
            clock.stop();
            g_launches.fetch_add(2);
            hip_check(hipMemcpyAsync(got.data(), d_results, sizeof(ScanResult) * slots, hipMemcpyDeviceToHost, stream));
            hip_check(hipMemcpyAsync(status.data(), d_status, slots, hipMemcpyDeviceToHost, stream));
            hip_check(hipStreamSynchronize(stream));
            device_ms += clock.ms();
        }
        for (uint32_t k = 0; k < count; ++k)
        {
            Item& it = items[order[first + k]];
            const size_t from = static_cast<size_t>(k) * intervals;
            it.results.assign(got.begin() + from, got.begin() + from + intervals);
            it.status.assign(status.begin() + from, status.begin() + from + intervals);
        }
        first = last;
    }
}

// A frame of this file's round.
struct Frame
{
    uint32_t frame{};  // in the caller's tables
    uint32_t window{}; // in the round's StreamWindows
    bool by_index{};
    uint32_t scans{}, lines{}, intervals{}; // per scan (prefix mode: lines = height, one interval)
    ScanSpec first{};
    ScanDesc desc{};    // its first scan
    size_t plane_bytes{};
    const SeekIndex* index{};
    bool reached{true}; // prefix mode: the scan of the current round was located
    std::vector<uint8_t> status; // scans x intervals
    std::vector<uint32_t> whole_rows; // prefix mode, per scan: the rows that stay
};

uint64_t reader_position(const uint8_t* point, const ScanSpec& spec) noexcept
{
    const size_t at = seek::reader_off(spec.width, spec.interleave_mode == 0 ? 1 : spec.components, spec.bits_per_sample > 8);
    uint64_t v = 0;
    for (int b = 7; b >= 0; --b)
        v = (v << 8) | point[at + b];
    return v;
}

// The work of scan `d` of an index-mode frame (stream_capacity 0: not reached).
Item index_item(const Frame& f, const ScanDesc& d, const IndexScan& rec)
{
    Item it;
    it.desc = d;
    it.lines = f.lines;
    it.intervals = f.intervals;
    it.points = rec.data.data();
    it.point_total = rec.data.size();
    const size_t point_bytes = seek_point_bytes(f.first);
    for (uint32_t i = 0; i < f.intervals; ++i)
    {
        seek::SeekWork w{};
        w.first_row = i * f.lines;
        w.end_row = static_cast<uint32_t>(std::min<uint64_t>(f.first.height, (static_cast<uint64_t>(i) + 1) * f.lines));
        w.store_from = w.first_row;
        w.mode = i + 1 < f.intervals ? seek::kResumeCompare : seek::kResumeEnd;
        w.from_point = i == 0 ? 0 : (i - 1) * point_bytes;
        w.to_point = i + 1 < f.intervals ? i * point_bytes : 0;
        // a point whose reader stands beyond the bytes that are left starts nothing
        const bool launched = d.stream_capacity != 0 && (i == 0 || reader_position(it.points + w.from_point, f.first) <= d.stream_capacity);
        it.work.push_back(launched ? w : idle_work());
        it.expect.push_back(i + 1 < f.intervals ? dev::kSalvageEndsInNextPoint : rec.segment_bytes);
        it.status.push_back(launched ? kKept : kNotReached);
    }
    return it;
}

Item prefix_item(const Frame& f, const ScanDesc& d)
{
    Item it;
    it.desc = d;
    it.lines = f.first.height;
    it.intervals = 1;
    seek::SeekWork w{};
    w.end_row = f.first.height;
    w.mode = seek::kResumePrefix;
    const bool launched = d.stream_capacity != 0;
    it.work.push_back(launched ? w : idle_work());
    it.expect.push_back(0);
    it.status.push_back(launched ? kKept : kNotReached);
    return it;
}

} // namespace

void jls::decode_batch_salvage_indexed(uint32_t frame_count, const void* d_packed, const uint64_t* offsets, const uint64_t* sizes,
                                       const SeekIndex* const* parsed_indexes, const void* indexes, size_t index_pitch_bytes,
                                       const uint64_t* index_sizes, const charls_amd_frame_dest* dests, uint32_t fill_value, uint32_t flags,
                                       charls_amd_codec_params* params_out, charls_amd_salvage_report* reports, uint8_t* interval_status,
                                       size_t status_pitch_bytes, charls_jpegls_errc* errcs, void* hip_stream)
{
    decode_batch_salvage(frame_count, d_packed, offsets, sizes, dests, fill_value, params_out, reports, interval_status, status_pitch_bytes,
                         errcs, hip_stream);
    std::vector<uint32_t> failed;
    for (uint32_t f = 0; f < frame_count; ++f)
        if (reports[f].state == 2)
            failed.push_back(f);
    if (failed.empty())
        return;
    // charls_amd_last_timings: [2] grows by what this round took by the host's clock, [3] is its launches by device events
    double device_ms = 0;
    struct RoundClock
    {
        const double& device_ms;
        std::chrono::steady_clock::time_point begin = std::chrono::steady_clock::now();
        ~RoundClock()
        {
            dev::Timings& t = dev::last_timings();
            t.values[2] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - begin).count();
            t.values[3] = device_ms;
            t.count = 4;
        }
    } round_clock{device_ms};

    // ---- which of the failed frames got past their header, and are frames the seek kernels take
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
    std::vector<SeekIndex> own(n); // the indexes parsed here
    std::vector<Frame> set;
    for (uint32_t k = 0; k < n; ++k)
    {
        const BatchFrame& x = win.fr[k];
        const uint32_t f = failed[k];
        const charls_amd_frame_dest& dest = dests[f];
        if (x.done)
            continue; // the header does not parse
        try
        {
            const auto [row, stride] = row_and_stride(x.reader, dest.stride);
            const uint32_t scans = static_cast<uint32_t>(scans_of_frame(x.reader));
            const size_t rows = static_cast<size_t>(x.reader.frame_info().height) * scans;
            if (stride < row || dest.capacity_bytes < stride * rows - (stride - row))
                continue; // round 1 refused the destination: nothing of the frame is written
            const ScanSpec spec = scan_spec_of(x.reader);
            if (x.reader.height_from_dnl() || !seek_spec_eligible(spec))
                continue;
            ScanDesc d = desc_of(spec);
            d.pixels = static_cast<uint8_t*>(dest.d_pixels) + x.plane_offset;
            d.pixel_stride = stride;
            d.stream = win.stream_ptr(k, x.cursor);
            d.stream_capacity = win.sizes[k] - x.cursor;
            d.line_scratch = nullptr;
            if (!rows_aligned(d) || d.stream_capacity == 0)
                continue;

            // the index: set_index's checks; one that is refused or has no points for every scan counts as absent
            const SeekIndex* index = parsed_indexes != nullptr ? parsed_indexes[f] : nullptr;
            bool offered = index != nullptr;
            if (index == nullptr && index_sizes != nullptr && index_sizes[f] != 0)
            {
                offered = true;
                try
                {
                    check_argument(indexes != nullptr && index_sizes[f] <= index_pitch_bytes, CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_SIZE);
                    own[k] = parse_index(x.reader, static_cast<const uint8_t*>(indexes) + static_cast<size_t>(f) * index_pitch_bytes,
                                         static_cast<size_t>(index_sizes[f]));
                    index = &own[k];
                }
                catch (const error&)
                {
                }
            }
            if (index != nullptr)
            {
                bool usable = index->lines != 0 && index->scans.size() == scans;
                for (size_t c = 0; usable && c < index->scans.size(); ++c)
                    usable = index->scans[c].points != 0 && index->scans[c].points == seek::points_per_scan(spec.height, index->lines) &&
                             index->scans[c].data.size() == static_cast<size_t>(index->scans[c].points) * seek_point_bytes(spec);
                if (!usable)
                    index = nullptr;
            }
            if (offered && index == nullptr)
                reports[f].reserved |= 2u;
            if (index == nullptr && (flags & kFlagPrefix) == 0)
                continue;
            if (fill_value > static_cast<uint32_t>(x.reader.validated_pc().maximum_sample_value))
            {
                errcs[f] = CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT;
                continue;
            }
            Frame fr;
            fr.frame = f;
            fr.window = k;
            fr.by_index = index != nullptr;
            fr.scans = scans;
            fr.lines = index != nullptr ? index->lines : spec.height;
            fr.intervals = index != nullptr ? index->scans[0].points + 1 : 1u;
            fr.first = spec;
            fr.desc = d;
            fr.plane_bytes = stride * spec.height;
            fr.index = index;
            fr.status.assign(static_cast<size_t>(scans) * fr.intervals, kNotReached);
            fr.whole_rows.assign(scans, 0);
            set.push_back(std::move(fr));
        }
        catch (const error&)
        { // (parameters the decoder refuses: round 1 said so)
        }
    }
    if (set.empty())
        return;

    // ---- index mode: every scan of every frame in the launches of its group.  Scan c + 1 is looked for where the index says
    // scan c ends; without a valid SOS of the same kind of scan there, it and the scans behind it are not reached.
    {
        std::vector<Item> items;
        std::vector<std::pair<uint32_t, uint32_t>> item_of; // (set index, scan)
        std::vector<uint8_t> reached(set.size(), 1);
        uint32_t most_scans = 0;
        for (const Frame& fr : set)
            most_scans = std::max(most_scans, fr.by_index ? fr.scans : 0u);
        for (uint32_t c = 0; c < most_scans; ++c)
        {
            for (uint32_t i = 0; i < set.size(); ++i)
            {
                Frame& fr = set[i];
                if (!fr.by_index || c >= fr.scans)
                    continue;
                const BatchFrame& x = win.fr[fr.window];
                ScanDesc d = fr.desc;
                d.pixels = fr.desc.pixels + c * fr.plane_bytes;
                d.stream_capacity = 0;
                if (reached[i] && c != 0)
                {
                    reached[i] = 0;
                    try
                    {
                        if (!x.done && x.reader.scan_interleave_mode() == 0 && x.reader.scan_component_count() == 1 &&
                            same_scan_parameters(scan_spec_of(x.reader), fr.first) && x.cursor < win.sizes[fr.window])
                            reached[i] = 1;
                    }
                    catch (const error&)
                    {
                    }
                }
                if (reached[i])
                {
                    d.stream = win.stream_ptr(fr.window, x.cursor);
                    d.stream_capacity = win.sizes[fr.window] - x.cursor;
                }
                items.push_back(index_item(fr, d, fr.index->scans[c]));
                item_of.emplace_back(i, c);
            }
            // on to scan c + 1
            std::vector<uint32_t> which;
            std::vector<size_t> bases;
            for (uint32_t i = 0; i < set.size(); ++i)
            {
                Frame& fr = set[i];
                if (!fr.by_index || !reached[i] || c + 1 >= fr.scans)
                    continue;
                BatchFrame& x = win.fr[fr.window];
                const uint64_t length = fr.index->scans[c].segment_bytes;
                if (length >= win.sizes[fr.window] - x.cursor)
                {
                    reached[i] = 0;
                    continue;
                }
                x.cursor += static_cast<size_t>(length);
                which.push_back(fr.window);
                bases.push_back(x.cursor);
            }
            win.parse_behind_scans(win.fr, which, bases, std::vector<uint8_t>(which.size(), 0));
        }
        if (!items.empty())
            run_items(items, fill_value, dev::kSalvageByIndex, stream, device_ms);
        for (size_t k = 0; k < items.size(); ++k)
        {
            Frame& fr = set[item_of[k].first];
            uint8_t* status = fr.status.data() + static_cast<size_t>(item_of[k].second) * fr.intervals;
            bool proven = true; // every interval above is kept: exact by induction from the true initial state
            for (uint32_t i = 0; i < fr.intervals; ++i)
            {
                const uint8_t v = items[k].status[i];
                status[i] = v == kKept && !proven ? static_cast<uint8_t>(kOnTheIndex) : v;
                proven = proven && v == kKept;
            }
        }
    }

    // ---- prefix mode: scan by scan from the top; the scan behind one that decoded is looked for where it ended
    {
        uint32_t most_scans = 0;
        for (const Frame& fr : set)
            most_scans = std::max(most_scans, fr.by_index ? 0u : fr.scans);
        for (uint32_t c = 0; c < most_scans; ++c)
        {
            std::vector<Item> items;
            std::vector<uint32_t> owner;
            for (uint32_t i = 0; i < set.size(); ++i)
            {
                Frame& fr = set[i];
                if (fr.by_index || c >= fr.scans)
                    continue;
                const BatchFrame& x = win.fr[fr.window];
                ScanDesc d = fr.desc;
                d.pixels = fr.desc.pixels + c * fr.plane_bytes;
                d.stream_capacity = 0;
                if (fr.reached && c != 0)
                {
                    fr.reached = false;
                    try
                    {
                        if (!x.done && x.reader.scan_interleave_mode() == 0 && x.reader.scan_component_count() == 1 &&
                            same_scan_parameters(scan_spec_of(x.reader), fr.first) && x.cursor < win.sizes[fr.window])
                            fr.reached = true;
                    }
                    catch (const error&)
                    {
                    }
                }
                if (fr.reached)
                {
                    d.stream = win.stream_ptr(fr.window, x.cursor);
                    d.stream_capacity = win.sizes[fr.window] - x.cursor;
                }
                items.push_back(prefix_item(fr, d));
                owner.push_back(i);
            }
            if (items.empty())
                break;
            run_items(items, fill_value, dev::kSalvageByPrefix, stream, device_ms);
            std::vector<uint32_t> which;
            std::vector<size_t> bases;
            for (size_t k = 0; k < items.size(); ++k)
            {
                Frame& fr = set[owner[k]];
                const uint8_t v = items[k].status[0];
                fr.status[c] = v;
                fr.whole_rows[c] = v == kKept ? fr.first.height
                                              : (v == kPrefix ? static_cast<uint32_t>(std::min<uint64_t>(items[k].results[0].bytes, fr.first.height)) : 0u);
                if (v != kKept)
                    fr.reached = false;
                if (!fr.reached || c + 1 >= fr.scans)
                    continue;
                BatchFrame& x = win.fr[fr.window];
                const uint64_t used = items[k].results[0].bytes;
                if (used >= win.sizes[fr.window] - x.cursor)
                {
                    fr.reached = false;
                    continue;
                }
                x.cursor += static_cast<size_t>(used);
                which.push_back(fr.window);
                bases.push_back(x.cursor);
            }
            win.parse_behind_scans(win.fr, which, bases, std::vector<uint8_t>(which.size(), 0));
        }
    }

    // ---- reports, status bytes, counters
    for (const Frame& fr : set)
    {
        charls_amd_salvage_report& r = reports[fr.frame];
        const uint32_t kept_bits = r.reserved;
        r = charls_amd_salvage_report{fr.by_index ? 1u : 3u, fr.scans * fr.intervals, 0, 0, kNoRow, kept_bits};
        uint64_t proven = 0, on_index = 0;
        for (uint32_t c = 0; c < fr.scans; ++c)
            for (uint32_t j = 0; j < fr.intervals; ++j)
            {
                const uint8_t v = fr.status[static_cast<size_t>(c) * fr.intervals + j];
                proven += v == kKept;
                on_index += v == kOnTheIndex;
                if (v == kKept || v == kOnTheIndex)
                    continue;
                const uint32_t row = fr.by_index ? j * fr.lines : fr.whole_rows[c];
                const uint32_t lost = fr.by_index ? std::min(fr.lines, fr.first.height - row) : fr.first.height - row;
                ++r.intervals_lost;
                r.rows_lost += lost;
                if (lost != 0)
                    r.first_lost_row = std::min(r.first_lost_row, row);
            }
        if (interval_status != nullptr)
        {
            if (status_pitch_bytes >= fr.status.size())
                std::memcpy(interval_status + static_cast<size_t>(fr.frame) * status_pitch_bytes, fr.status.data(), fr.status.size());
            else
                r.reserved |= 1u;
        }
        if (fr.by_index)
        {
            g_frames_by_index.fetch_add(1);
            g_kept_proven.fetch_add(proven);
            g_kept_on_index.fetch_add(on_index);
            g_lost.fetch_add(r.intervals_lost);
        }
        else
            g_frames_by_prefix.fetch_add(1);
    }
}

extern "C" charls_jpegls_errc charls_amd_decode_batch_device_salvage_indexed(
    uint32_t frame_count, const void* d_packed, const uint64_t* offsets, const uint64_t* sizes, const void* indexes, size_t index_pitch_bytes,
    const uint64_t* index_sizes, const charls_amd_frame_dest* dests, uint32_t fill_value, uint32_t flags, charls_amd_codec_params* params_out,
    charls_amd_salvage_report* reports, uint8_t* interval_status, size_t status_pitch_bytes, charls_jpegls_errc* errcs, void* hip_stream)
try
{
    check_pointer(offsets);
    check_pointer(sizes);
    check_pointer(index_sizes);
    check_pointer(dests);
    check_pointer(errcs);
    check_pointer(reports);
    check_argument((flags & ~kFlagPrefix) == 0);
    check_argument(interval_status == nullptr || status_pitch_bytes != 0);
    for (uint32_t f = 0; f < frame_count; ++f)
    {
        check_argument(dests[f].reserved == 0);
        check_buffer(dests[f].d_pixels, dests[f].capacity_bytes);
        if (index_sizes[f] != 0)
            check_pointer(indexes);
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
    decode_batch_salvage_indexed(frame_count, d_packed, offsets, sizes, nullptr, indexes, index_pitch_bytes, index_sizes, dests, fill_value,
                                 flags, params_out, reports, interval_status, status_pitch_bytes, errcs, hip_stream);
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}

extern "C" int32_t charls_amd_salvage_index_counters(uint64_t* out, int32_t capacity)
{
    const uint64_t v[6] = {g_frames_by_index.load(), g_kept_proven.load(), g_kept_on_index.load(),
                           g_lost.load(),            g_frames_by_prefix.load(), g_launches.load()};
    int32_t n = 0;
    for (; out != nullptr && n < capacity && n < 6; ++n)
        out[n] = v[n];
    return n;
}
