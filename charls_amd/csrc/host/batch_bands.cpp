// batch_bands.cpp -- row bands through restart markers (charls_amd.h part 2m).
//
// charls_amd_decode_rows_batch_device_ragged sends a frame with restart intervals down the whole-frame branch of decode_bands
// (batch_index.cpp): decoded whole into a work area, the band copied out, one frame at a time.  A band meets one or a few of
// the frame's intervals, and an interval is a scan of its own (restart_intervals.h).  So here:
//   markers      find_restart_markers over all such scans of the call, ONE launch per scan ordinal (a planar frame's scan c + 1
//                starts where find_scan_end puts the end of scan c; nothing of scan c is decoded for that); the counts, the
//                marks the bands need and the number bytes of the markers up to the band come to the host
//   descriptors  built on the host (band_plan.h): interval j with restart_interval 0, its rows, its stream window
//   destinations an interval inside the band decodes to its rows of the band; one that sticks out decodes into the thread's
//                edge area (dev::band_edges_arena) and its wanted rows are copied (hipMemcpy2DAsync, one synchronise for all)
//   decode       every band interval of every frame through the ordinary launcher: one launch per kernel specialisation
//   verdict      band_plan.h: piece_holds, for every band interval of the frame
// A frame that fails anything on the way goes through decode_bands in the same call, as does every frame that was never a
// candidate: that path decodes from the top and reports what the reference reports.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <set>
#include <vector>

#include "../device/restart_intervals.h"
#include "../device/runtime.h"
#include "band_plan.h"
#include "batch_streams.h"
#include "common.h"
#include "scan_engine.h"
#include "seek_index.h"
#include "stream_reader.h"
#include "stream_windows.h"

using namespace jls;
using dev::hip_check;

static_assert(band::kUndecidedFlags == interval::kUndecided, "the flags an interval's result may not keep");

namespace {

// charls_amd_band_marker_counters
std::atomic<uint64_t> g_route_frames{0}, g_route_intervals{0}, g_route_fallbacks{0}, g_route_launches{0};

enum : int
{ // dev::seek_arena: the route is over before decode_bands uses them
    kArenaMarks = 0,
    kArenaNumbers = 1,
    kArenaDescs = 2,
    kArenaCounts = 3,
    kArenaSearch = 4,
};
constexpr size_t kEdgeAlignment = 256; // (an edge starts on one: 16-bit rows are never at an odd address)

struct RouteFrame
{
    uint32_t frame{};
    uint32_t height{}, lines{}, intervals{};
    uint32_t first{}, rows{};
    band::Range met{};
    size_t stride{}, row_bytes{}, scans_n{};
    ScanSpec spec{};
    std::vector<ScanDesc> scans;              // scan c: its stream from its first byte, its pixels the band's rows of plane c
    std::vector<std::vector<uint32_t>> marks; // scan c: marks 0 .. min(j1, N - 2)
    size_t edge_at{};                         // of the frame's edges in the area
    bool ok{true};
};

size_t edge_bytes(const RouteFrame& r, const band::Piece& p)
{
    return (r.row_bytes * p.rows + kEdgeAlignment - 1) & ~(kEdgeAlignment - 1);
}

// The band's checks of decode_bands, without a verdict: a frame that fails one is reported by that body.
bool band_fits(const BatchFrame& x, uint32_t first, uint32_t rows, const charls_amd_frame_dest& to, RouteFrame& r)
{
    try
    {
        const charls_frame_info& f = x.reader.frame_info();
        if (!(rows > 0 && first < f.height && rows <= f.height - first))
            return false;
        r.spec = scan_spec_of(x.reader);
        r.row_bytes = row_bytes_of(r.spec);
        r.stride = to.stride == 0 ? r.row_bytes : to.stride;
        r.scans_n = scans_of_frame(x.reader);
        if (r.stride < r.row_bytes)
            return false;
        return to.capacity_bytes >= checked_mul(checked_mul(r.stride, rows), r.scans_n) - (r.stride - r.row_bytes);
    }
    catch (const error&)
    {
        return false;
    }
}

// Scan c of frame r as the reader of `y` stands behind its header: the band's rows of plane c.
ScanDesc route_scan_desc(const StreamWindows& s, const RouteFrame& r, const BatchFrame& y, const charls_amd_frame_dest& to, size_t c)
{
    ScanDesc d = desc_of(scan_spec_of(y.reader));
    d.pixels = static_cast<uint8_t*>(to.d_pixels) + r.stride * r.rows * c;
    d.pixel_stride = r.stride;
    d.stream = s.stream_ptr(r.frame, y.cursor);
    d.stream_capacity = s.sizes[r.frame] - y.cursor;
    d.line_scratch = nullptr;
    return d;
}

bool scan_on_route(const ScanSpec& spec, const ScanSpec& first, const ScanDesc& d) noexcept
{
    return same_scan_parameters(spec, first) && spec.restart_interval > 0 && spec.restart_interval < spec.height && dev::salvage_candidate(d);
}

// Steps 1 to 6 of the route.  Frames that end on it are done in `s`, with success; every other frame is left as it was.
// `started`: the frames that started the route -- no frame is done before the last statement that can raise, so a caller that
// catches what this raises finds every one of them as it was.
void bands_through_markers(StreamWindows& s, const void* indexes, size_t index_pitch_bytes, const uint64_t* index_sizes,
                           const uint32_t* first_rows, const uint32_t* row_counts, const charls_amd_frame_dest* bands, size_t& started)
{
    const uint32_t frame_count = static_cast<uint32_t>(s.fr.size());
    const hipStream_t stream = s.stream;

    // ---- which frames
    std::vector<RouteFrame> route;
    for (uint32_t i = 0; i < frame_count; ++i)
    {
        const BatchFrame& x = s.fr[i];
        RouteFrame r;
        r.frame = i;
        if (x.done || x.reader.height_from_dnl() || !band_fits(x, first_rows[i], row_counts[i], bands[i], r))
            continue;
        if (index_sizes[i] != 0)
        { // (an index that does not parse is decode_bands' to report)
            try
            {
                if (index_sizes[i] > index_pitch_bytes)
                    continue;
                const SeekIndex index =
                    parse_index(x.reader, static_cast<const uint8_t*>(indexes) + i * index_pitch_bytes, static_cast<size_t>(index_sizes[i]));
                bool points = false;
                for (const IndexScan& rec : index.scans)
                    points = points || rec.points != 0;
                if (points)
                    continue;
            }
            catch (const error&)
            {
                continue;
            }
        }
        r.first = first_rows[i];
        r.rows = row_counts[i];
        r.height = r.spec.height;
        r.lines = r.spec.restart_interval;
        const ScanDesc d = route_scan_desc(s, r, x, bands[i], 0);
        if (!scan_on_route(r.spec, r.spec, d))
            continue;
        r.intervals = band::interval_count(r.height, r.lines);
        r.met = band::intervals_met(r.first, r.rows, r.lines);
        r.scans.push_back(d);
        route.push_back(std::move(r));
    }
    if (route.empty())
        return;

    // ---- room for the edges: a quarter of what the thread's work areas may hold; frames beyond it go the existing way
    {
        const size_t room = std::max<size_t>(dev::work_area_budget() / 4, 1);
        size_t total = 0;
        std::vector<RouteFrame> kept;
        for (RouteFrame& r : route)
        {
            size_t want = 0;
            const band::Piece a = band::piece_rows(r.height, r.lines, r.first, r.rows, r.met.j0);
            const band::Piece b = band::piece_rows(r.height, r.lines, r.first, r.rows, r.met.j1);
            if (a.edge)
                want += edge_bytes(r, a);
            if (b.edge && r.met.j1 != r.met.j0)
                want += edge_bytes(r, b);
            want *= r.scans_n;
            if (want > room - std::min(total, room))
                continue;
            r.edge_at = total;
            total += want;
            kept.push_back(std::move(r));
        }
        if (total != 0 && dev::try_ensure(dev::band_edges_arena(), total) == nullptr)
        { // no edge area at all: the frames without edges still go the route
            std::vector<RouteFrame> inner;
            for (RouteFrame& r : kept)
            {
                const band::Piece a = band::piece_rows(r.height, r.lines, r.first, r.rows, r.met.j0);
                const band::Piece b = band::piece_rows(r.height, r.lines, r.first, r.rows, r.met.j1);
                if (!a.edge && !b.edge)
                    inner.push_back(std::move(r));
            }
            kept.swap(inner);
        }
        route.swap(kept);
    }
    if (route.empty())
        return;
    g_route_frames.fetch_add(route.size());
    started = route.size();

    // ---- markers, scan ordinal by scan ordinal
    std::vector<BatchFrame> probe; // readers and cursors of the frames with further scans
    uint64_t launches = 0;
    for (size_t c = 0;; ++c)
    {
        std::vector<uint32_t> active; // positions in `route`
        for (uint32_t k = 0; k < route.size(); ++k)
            if (route[k].ok && route[k].scans.size() == c + 1)
                active.push_back(k);
        if (active.empty())
            break;
        const uint32_t n = static_cast<uint32_t>(active.size());
        uint32_t max_marks = 1, most_needed = 1;
        std::vector<ScanDesc> descs(n);
        std::vector<uint32_t> needed(n);
        std::vector<MarkerSearch> searches;
        std::vector<uint32_t> searching; // positions in `active`
        for (uint32_t q = 0; q < n; ++q)
        {
            const RouteFrame& r = route[active[q]];
            descs[q] = r.scans[c];
            max_marks = std::max(max_marks, r.intervals - 1);
            needed[q] = std::min(r.met.j1, r.intervals - 2) + 1;
            most_needed = std::max(most_needed, needed[q]);
            if (c + 1 < r.scans_n)
            {
                const uint64_t at = s.offset_of(r.frame);
                searches.push_back(MarkerSearch{at + (s.sizes[r.frame] - r.scans[c].stream_capacity), at + s.sizes[r.frame]});
                searching.push_back(q);
            }
        }
        auto* d_descs = static_cast<ScanDesc*>(dev::seek_arena(kArenaDescs).ensure(dev::with_headroom(sizeof(ScanDesc) * n)));
        auto* d_marks = static_cast<uint32_t*>(dev::seek_arena(kArenaMarks).ensure(dev::with_headroom(sizeof(uint32_t) * n * max_marks)));
        auto* d_counts = static_cast<uint32_t*>(dev::seek_arena(kArenaCounts).ensure(dev::with_headroom(sizeof(uint32_t) * n)));
        std::vector<uint32_t> counts(n), marks(static_cast<size_t>(n) * most_needed);
        std::vector<unsigned long long> found(searches.size());
        hip_check(hipMemcpyAsync(d_descs, descs.data(), sizeof(ScanDesc) * n, hipMemcpyHostToDevice, stream));
        dev::launch_find_restart_markers(d_descs, d_marks, max_marks, d_counts, n, stream);
        ++launches;
        if (!searches.empty())
        {
            const size_t search_bytes = (sizeof(MarkerSearch) * searches.size() + 255) & ~size_t{255};
            auto* area = static_cast<uint8_t*>(
                dev::seek_arena(kArenaSearch).ensure(dev::with_headroom(search_bytes + sizeof(unsigned long long) * searches.size())));
            hip_check(hipMemcpyAsync(area, searches.data(), sizeof(MarkerSearch) * searches.size(), hipMemcpyHostToDevice, stream));
            dev::launch_find_scan_end(s.slots, reinterpret_cast<const MarkerSearch*>(area), reinterpret_cast<unsigned long long*>(area + search_bytes),
                                      static_cast<uint32_t>(searches.size()), stream);
            hip_check(hipMemcpyAsync(found.data(), area + search_bytes, sizeof(unsigned long long) * searches.size(), hipMemcpyDeviceToHost, stream));
        }
        hip_check(hipMemcpyAsync(counts.data(), d_counts, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, stream));
        hip_check(hipMemcpy2DAsync(marks.data(), sizeof(uint32_t) * most_needed, d_marks, sizeof(uint32_t) * max_marks,
                                   sizeof(uint32_t) * most_needed, n, hipMemcpyDeviceToHost, stream));
        hip_check(hipStreamSynchronize(stream));

        // the number bytes of markers 0 .. min(j1, N - 2) of every scan whose count is right: one gather
        std::vector<WindowSpec> specs;
        std::vector<uint32_t> numbers_at(n, 0);
        for (uint32_t q = 0; q < n; ++q)
        {
            RouteFrame& r = route[active[q]];
            if (counts[q] != r.intervals - 1)
            {
                r.ok = false;
                continue;
            }
            const uint32_t* mk = marks.data() + static_cast<size_t>(q) * most_needed;
            r.marks.emplace_back(mk, mk + needed[q]);
            numbers_at[q] = static_cast<uint32_t>(specs.size());
            const uint64_t scan_at = s.offset_of(r.frame) + (s.sizes[r.frame] - r.scans[c].stream_capacity);
            for (uint32_t k = 0; k < needed[q]; ++k) // (a mark has a byte behind it: find_restart_markers' u + 1 < u_end)
                specs.push_back(WindowSpec{scan_at + mk[k] + 1, 1, 0});
        }
        if (!specs.empty())
        {
            const size_t spec_bytes = (sizeof(WindowSpec) * specs.size() + 255) & ~size_t{255};
            auto* area = static_cast<uint8_t*>(dev::seek_arena(kArenaNumbers).ensure(dev::with_headroom(spec_bytes + specs.size())));
            std::vector<uint8_t> numbers(specs.size());
            hip_check(hipMemcpyAsync(area, specs.data(), sizeof(WindowSpec) * specs.size(), hipMemcpyHostToDevice, stream));
            hipLaunchKernelGGL(gather_windows, dim3(static_cast<uint32_t>(specs.size())), dim3(64), 0, stream, s.slots,
                               reinterpret_cast<const WindowSpec*>(area), area + spec_bytes, 1u);
            hip_check(hipGetLastError());
            hip_check(hipMemcpyAsync(numbers.data(), area + spec_bytes, specs.size(), hipMemcpyDeviceToHost, stream));
            hip_check(hipStreamSynchronize(stream));
            for (uint32_t q = 0; q < n; ++q)
            {
                RouteFrame& r = route[active[q]];
                if (r.ok && !band::numbers_cyclic(numbers.data() + numbers_at[q], needed[q]))
                    r.ok = false;
            }
        }

        // on to scan c + 1: the part-1 reader on what stands where the segment ended
        std::vector<uint32_t> which;
        std::vector<size_t> bases;
        std::vector<uint32_t> of_route;
        for (size_t w = 0; w < searching.size(); ++w)
        {
            RouteFrame& r = route[active[searching[w]]];
            if (!r.ok)
                continue;
            if (found[w] == kNoMarker)
            {
                r.ok = false;
                continue;
            }
            if (probe.empty())
                probe = s.fr;
            which.push_back(r.frame);
            bases.push_back(static_cast<size_t>(found[w] - s.offset_of(r.frame)));
            of_route.push_back(active[searching[w]]);
        }
        s.parse_behind_scans(probe, which, bases, std::vector<uint8_t>(which.size(), 0));
        for (size_t w = 0; w < which.size(); ++w)
        {
            RouteFrame& r = route[of_route[w]];
            const BatchFrame& y = probe[r.frame];
            try
            {
                if (y.done)
                    raise(CHARLS_JPEGLS_ERRC_INVALID_DATA);
                const ScanDesc d = route_scan_desc(s, r, y, bands[r.frame], c + 1);
                if (!scan_on_route(scan_spec_of(y.reader), r.spec, d))
                    raise(CHARLS_JPEGLS_ERRC_INVALID_DATA);
                r.scans.push_back(d);
            }
            catch (const error&)
            {
                r.ok = false;
            }
        }
    }

    // ---- descriptors and destinations
    struct Launched
    {
        uint32_t of_route;
        uint32_t scan;
        band::Piece piece;
        uint8_t* edge; // where an edge was decoded to
    };
    std::vector<ScanDesc> descs;
    std::vector<Launched> launched;
    auto* edges = dev::band_edges_arena().as<uint8_t>();
    for (uint32_t k = 0; k < route.size(); ++k)
    {
        RouteFrame& r = route[k];
        r.ok = r.ok && r.scans.size() == r.scans_n && r.marks.size() == r.scans_n;
        if (!r.ok)
            continue;
        size_t edge_at = r.edge_at;
        for (uint32_t c = 0; c < r.scans_n; ++c)
            for (uint32_t j = r.met.j0; j <= r.met.j1; ++j)
            {
                const band::Piece p = band::piece_of(r.height, r.lines, r.first, r.rows, j, r.marks[c].data(), r.scans[c].stream_capacity);
                ScanDesc d = r.scans[c];
                d.height = p.rows;
                d.restart_interval = 0;
                d.stream += p.start;
                d.stream_capacity = p.bytes;
                uint8_t* edge = nullptr;
                if (p.edge)
                {
                    edge = edges + edge_at;
                    edge_at += edge_bytes(r, p);
                    d.pixels = edge;
                    d.pixel_stride = r.row_bytes;
                }
                else
                    d.pixels += r.stride * p.band_row;
                descs.push_back(d);
                launched.push_back(Launched{k, c, p, edge});
            }
    }
    if (!descs.empty())
    {
        std::set<uint64_t> keys;
        for (const ScanDesc& d : descs)
            keys.insert(dev::decode_launch_key(d));
        // (descriptors, results and line scratch of the launch are the launcher's own, allocated for the call as the batch
        // decoder's are: no work areas.  Counted: the launches of the decoders themselves, one per specialisation; a launch of the
        // exact decoder behind a speed path, for intervals that did not end cleanly there, is not.)
        DecodeLauncher launcher(stream, true);
        std::vector<ScanResult> results;
        launcher.run(descs, results);
        launches += keys.size();
        g_route_intervals.fetch_add(descs.size());

        // ---- verdict, then the wanted rows of the edges of the frames that held
        for (size_t k = 0; k < launched.size(); ++k)
        {
            RouteFrame& r = route[launched[k].of_route];
            if (!band::piece_holds(launched[k].piece, r.intervals, results[k].errc, results[k].flags, results[k].bytes))
                r.ok = false;
        }
        for (const Launched& l : launched)
        {
            const RouteFrame& r = route[l.of_route];
            if (!r.ok || l.edge == nullptr)
                continue;
            hip_check(hipMemcpy2DAsync(static_cast<uint8_t*>(bands[r.frame].d_pixels) + r.stride * r.rows * l.scan + r.stride * l.piece.band_row,
                                       r.stride, l.edge + r.row_bytes * l.piece.skip, r.row_bytes, r.row_bytes, l.piece.copy_rows,
                                       hipMemcpyDeviceToDevice, stream));
        }
        hip_check(hipStreamSynchronize(stream));
    }
    uint64_t fallbacks = 0;
    for (const RouteFrame& r : route)
    {
        if (!r.ok)
        {
            ++fallbacks;
            continue;
        }
        s.fr[r.frame].errc = CHARLS_JPEGLS_ERRC_SUCCESS;
        s.fr[r.frame].done = true;
    }
    g_route_fallbacks.fetch_add(fallbacks);
    g_route_launches.fetch_add(launches);
}

} // namespace

extern "C" charls_jpegls_errc charls_amd_decode_rows_batch_device_ragged_markers(
    uint32_t frame_count, const void* d_packed, const uint64_t* offsets, const uint64_t* sizes, const void* indexes, size_t index_pitch_bytes,
    const uint64_t* index_sizes, const uint32_t* first_rows, const uint32_t* row_counts, const charls_amd_frame_dest* bands,
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
    s.read_headers(true);
    size_t started = 0;
    try
    {
        bands_through_markers(s, indexes, index_pitch_bytes, index_sizes, first_rows, row_counts, bands, started);
    }
    catch (const error& e)
    { // no memory for a buffer of the route: its frames go the existing way, as those without room for their edges do
        if (e.code != CHARLS_JPEGLS_ERRC_NOT_ENOUGH_MEMORY)
            throw;
        (void)hipGetLastError();
        g_route_fallbacks.fetch_add(started);
    }
    decode_row_bands(s, indexes, index_pitch_bytes, index_sizes, first_rows, row_counts, bands, errcs);
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}

extern "C" int32_t charls_amd_band_marker_counters(uint64_t* out, int32_t capacity)
{
    const uint64_t v[4] = {g_route_frames.load(), g_route_intervals.load(), g_route_fallbacks.load(), g_route_launches.load()};
    int32_t n = 0;
    for (; out != nullptr && n < capacity && n < 4; ++n)
        out[n] = v[n];
    return n;
}
