// encode_launch.hip -- the encoder dispatch (see runtime.h): the tile pipeline's driver, the restart-interval encoder, the group
// encoder's lane rule and the sizing dispatch.  Compiled for gfx950 only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "knobs.h"
#include "runtime.h"
#include "work_areas.h"
#include "pipeline_common.hip"
#include "block_stuffing.hip"
#include "speculative_stuffing.hip"
#include "tile_pipeline.hip"
#include "group_launch.h"
#include "restart_intervals_encode.hip"

namespace jls::dev {

namespace {
std::atomic<uint64_t> g_speculation[tile_counter_count]{};
std::atomic<uint64_t> g_serial_fallback_scans{0}; // scans the tile pipeline was eligible for that ran on the one-wavefront kernel: no work area
void note_pipeline_fallback(uint32_t scans) noexcept
{
    g_serial_fallback_scans.fetch_add(scans);
}
} // namespace
uint64_t pipeline_fallback_scans() noexcept
{
    return g_serial_fallback_scans.load();
}
void speculation_counters(uint64_t out[tile_counter_count]) noexcept
{
    for (int i = 0; i < tile_counter_count; ++i)
        out[i] = g_speculation[i].load();
}

// ---------------------------------------------------------------------------------------------------------------
// Lossless pipeline orchestration.
namespace {

struct StageTimer
{
    hipEvent_t ev[10]{};
    int n = 0;
    hipStream_t s;
    explicit StageTimer(hipStream_t stream) : s(stream) {}
    StageTimer(const StageTimer&) = delete;
    StageTimer& operator=(const StageTimer&) = delete;
    StageTimer(StageTimer&& o) noexcept : n(o.n), s(o.s)
    {
        for (int i = 0; i < n; ++i)
            ev[i] = o.ev[i];
        o.n = 0;
    }
    ~StageTimer()
    {
        for (int i = 0; i < n; ++i)
            (void)hipEventDestroy(ev[i]);
    }
    void mark() { mark_on(s); }
    void mark_on(hipStream_t stream)
    {
        hip_check(hipEventCreate(&ev[n]));
        hip_check(hipEventRecord(ev[n], stream));
        ++n;
    }
    double between(int a, int b)
    {
        float ms = 0;
        hip_check(hipEventSynchronize(ev[b]));
        hip_check(hipEventElapsedTime(&ms, ev[a], ev[b]));
        return ms;
    }
};

// Events of a call, destroyed with it (also when a HIP error is raised half-way through a pass).
struct EventList
{
    std::vector<hipEvent_t> events;
    explicit EventList(size_t n = 0) { grow(n); }
    EventList(const EventList&) = delete;
    EventList& operator=(const EventList&) = delete;
    ~EventList()
    {
        for (hipEvent_t e : events)
            (void)hipEventDestroy(e);
    }
    void grow(size_t n)
    {
        events.reserve(n);
        while (events.size() < n)
        {
            hipEvent_t e{};
            hip_check(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            events.push_back(e);
        }
    }
    hipEvent_t operator[](size_t i) const { return events[i]; }
};

size_t align_up(size_t v, size_t a)
{
    return (v + a - 1) / a * a;
}

// Stage E in its block-parallel form (block_stuffing.hip) unless CHARLS_AMD_BLOCK_STUFFING=0 asks for stuff_scan.
bool block_stuffing_enabled()
{
    return knobs::get_or(knobs::kBlockStuffing, 1) != 0;
}

// Stage E in its speculative form (speculative_stuffing.hip) unless CHARLS_AMD_SPEC_STUFFING=0: for the passes whose stuffing
// nothing hides (the last pass of a call) and for streams so long that one wavefront per scan takes longer than the next
// pass's first stages (stuff_scan: 4.2 ns per byte, 99 ms for the 23.5 MB of a 4096 x 4096 RGB frame).
bool spec_stuffing_enabled()
{
    return knobs::get_or(knobs::kSpecStuffing, 1) != 0;
}
constexpr size_t kSpecStuffingAlwaysBytes = size_t{32} << 20; // destination capacity from which every pass takes the speculative form

constexpr uint32_t kBlockStuffingScans = 8; // scans per pass up to which stage E runs in its block-parallel form (it is for latency: every chunk is
                                            // walked from 16 entry states, 2.7 GB of L2 misses per frame when 64 frames do it at once)

// ---------------------------------------------------------------------------------------------------------------
// Tile pipeline (tile_pipeline.hip, tile_pixel_mode.hip): every lossless scan the pipeline is eligible for.

// Work area of one scan: 8 B per sample of up to 8 bits (key / slot map 2, records 3, code words 3: 2-byte slots, of which the
// run starts -- at most every second sample -- take two), 10 B per wider sample (2 + 4 + 4), the (tiles + 1) x 367 piece table,
// the job states and the unstuffed stream.
struct TileLayout
{
    tile::TilePlan plan;
    size_t samples, lines, raw_bytes, max_jobs, max_run_jobs;
    uint32_t lines_per_tile, tiles, job_events, warm_events, run_job_events, run_warm_events, rare_warm_events;
    size_t off_keyinv, off_seg, off_total, off_base, off_jobfirst, off_planpart, off_rec, off_code, off_jobs, off_runjobs, off_bbase, off_raw,
        off_bits, off_status, off_stuff, bytes;
    TileLayout(const ScanDesc& d, size_t capacity_hint, uint32_t count)
    {
        plan = tile::plan_tiles(d);
        lines = plan.lines;
        samples = static_cast<size_t>(plan.samples);
        lines_per_tile = plan.lines_per_tile;
        tiles = plan.tiles;
        // Jobs: every job pays warm_events of warm-up, so long jobs are cheaper; but ONE frame needs thousands of lanes to
        // fill the chip.  Aim at a quarter of a million lanes per launch, between 1024 and 8192 events per job.
        const long long knob_job = knobs::get(knobs::kJobEvents), knob_warm = knobs::get(knobs::kWarmEvents);
        uint64_t job = 1024;
        while (job < 8192 && samples * count / (job * 2) >= (uint64_t{1} << 18))
            job *= 2;
        job_events = knob_job != knobs::kUnset ? static_cast<uint32_t>(std::max<long long>(32, knob_job) / 32 * 32) : static_cast<uint32_t>(job); // (whole rounds of the walkers: 32 two-byte slots)
        warm_events = knob_warm != knobs::kUnset ? static_cast<uint32_t>(std::max<long long>(0, knob_warm)) : 1024u;
        max_jobs = samples / job_events + pipe::kChains;
        // the run chain: jobs of 2048 run events with a warm-up of as many (a test frame has 55 000 run events); small batches
        // take smaller jobs -- ONE frame has the whole chip, and the walk of a job and its warm-up is what the frame waits for
        // (up to four 4096 x 4096 frames: 128 events behind a warm-up of 1024 -- 2.35 ms per frame where 256 / 2048 took 2.65;
        // 512 events of warm-up are enough for the test frame and 256 are not: every job walked again, 10.8 ms)
        const long long knob_run_job = knobs::get(knobs::kRunJobEvents), knob_run_warm = knobs::get(knobs::kRunWarmEvents);
        const uint64_t batch_samples = static_cast<uint64_t>(samples) * count;
        const uint32_t run_job_default = batch_samples <= (uint64_t{1} << 26) ? 128u : (batch_samples <= (uint64_t{1} << 29) ? 512u : 2048u);
        run_job_events = knob_run_job != knobs::kUnset ? static_cast<uint32_t>(std::max<long long>(32, knob_run_job) / 32 * 32) : run_job_default;
        run_warm_events = knob_run_warm != knobs::kUnset ? static_cast<uint32_t>(std::max<long long>(0, knob_run_warm)) : (run_job_default == 128u ? 1024u : 2048u);
        max_run_jobs = samples / run_job_events + 2; // (+ the entry of the totals)
        // the exact walk of the rarer run context: events of that type a lane walks before its segment of the list
        rare_warm_events = static_cast<uint32_t>(std::max<long long>(0, knobs::get_or(knobs::kRareWarmEvents, 512)));
        const size_t worst = worst_case_scan_bytes(plan.line_samples, static_cast<uint32_t>(lines), 1, d.bits_per_sample);
        raw_bytes = align_up((capacity_hint < worst ? capacity_hint : worst) + 64, 16);
        size_t o = 0;
        auto take = [&](size_t n) {
            const size_t at = o;
            o = align_up(o + n, 256);
            return at;
        };
        off_keyinv = take(samples * 2);
        off_seg = take(static_cast<size_t>(tiles + 1) * pipe::kChains * 4);
        off_total = take(pipe::kChains * 4);
        off_base = take(pipe::kChains * 4);
        off_jobfirst = take((pipe::kChains + 1) * 4);
        off_planpart = take(static_cast<size_t>(tile::kPlanGroups) * pipe::kChains * 4);
        // records and code words: 2-byte slots for samples of up to 8 bits (a run start takes two), 4-byte slots otherwise
        const uint32_t run_slots = d.bits_per_sample > 8 ? 1u : 2u;
        const size_t slot_bytes = d.bits_per_sample > 8 ? 4 : 2;
        const size_t slots = static_cast<size_t>(tile::slots_capacity(samples, run_slots, lines)) + tile::kSlack;
        off_rec = take(slots * slot_bytes);
        off_code = take(slots * slot_bytes);
        off_jobs = take(max_jobs * sizeof(tile::JobState));
        off_runjobs = take(max_run_jobs * sizeof(tile::RunJob));
        off_bbase = take(static_cast<size_t>(tiles) * 16); // look-back states and tile tails, 8 B each
        off_raw = take(raw_bytes);
        off_bits = take(16);
        off_status = take(8);
        off_stuff = take(std::max(block_stuffing_enabled() ? (raw_bytes / pipe::kStuffChunk + 1) * pipe::kStuffWords * 4 : 0,
                                  spec_stuffing_enabled() ? pipe::stuff_spec_table_words(raw_bytes, pipe::stuff_spec_geometry().chunk_bytes) * 4 : 0));
        bytes = o;
    }
};

// The tile kernels ask for more dynamic LDS than a kernel gets by default.  Function attributes are per DEVICE: they are set
// once for every device this process launches the kernels on.
void ensure_tile_attributes()
{
    static std::mutex guard;
    static uint64_t done[4] = {0, 0, 0, 0}; // bitmap of devices
    int device = 0;
    hip_check(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(guard);
    if (device >= 0 && device < 256 && (done[device >> 6] >> (device & 63) & 1u) != 0)
        return;
    const int lds = 160 * 1024;
    auto set = [&](const void* kernel) { hip_check(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds)); };
    set(reinterpret_cast<const void*>(tile::analyze_tiles<uint8_t, 0>));
    set(reinterpret_cast<const void*>(tile::analyze_tiles<uint16_t, 0>));
    set(reinterpret_cast<const void*>(tile::pack_tiles<uint8_t>));
    set(reinterpret_cast<const void*>(tile::pack_tiles<uint16_t>));
    set(reinterpret_cast<const void*>(tile::sort_tiles<uint8_t, 0>));
    set(reinterpret_cast<const void*>(tile::sort_tiles<uint16_t, 0>));
    set(reinterpret_cast<const void*>(tile::analyze_pixel_tiles<uint8_t>));
    set(reinterpret_cast<const void*>(tile::analyze_pixel_tiles<uint16_t>));
    set(reinterpret_cast<const void*>(tile::sort_pixel_tiles<uint8_t>));
    set(reinterpret_cast<const void*>(tile::sort_pixel_tiles<uint16_t>));
    if (device >= 0 && device < 256)
        done[device >> 6] |= uint64_t{1} << (device & 63);
}

constexpr size_t kCounterBytes = 256; // tile::kCounters words behind the work areas of a call

template <typename S>
void run_tile_pipeline(const ScanDesc& proto, ScanDesc* d_descs, ScanResult* d_results, uint32_t count, hipStream_t stream)
{
    // (the shared work areas of the host-pointer ABI stay allocated between calls, so they are kept moderate: more frames than
    // fit take more passes)
    const size_t budget = on_shared_areas() ? std::min(arena_budget(work_buffer(WorkBuffer::pipeline).capacity()), shared_areas_keep_bytes())
                                                    : arena_budget(work_buffer(WorkBuffer::pipeline).capacity());
    // the layout depends on the number of scans of a pass only through the job size: settle on it for a full pass
    TileLayout lay(proto, proto.stream_capacity, count);
    size_t per_scan = lay.bytes + 2 * (sizeof(tile::Work) + sizeof(pipe::Work));
    uint32_t resident = static_cast<uint32_t>(std::max<size_t>(1, std::min<size_t>(count, budget / per_scan)));
    if (resident < count)
    {
        lay = TileLayout(proto, proto.stream_capacity, resident);
        per_scan = lay.bytes + 2 * (sizeof(tile::Work) + sizeof(pipe::Work));
        resident = static_cast<uint32_t>(std::max<size_t>(1, std::min<size_t>(count, budget / per_scan)));
    }
    uint8_t* arena = nullptr;
    // a configured limit that does not even cover ONE work area is honoured: the one-wavefront-per-scan kernel needs none
    const bool over_limit = workspace_limit() != 0 && budget < per_scan;
    for (; !over_limit;)
    {
        // (the shared areas of the host-pointer ABI see batches of every size: they grow in powers of two, so that they stop
        // growing -- growing frees the old block, and hipFree waits for every kernel on the device)
        uint32_t room = resident;
        if (on_shared_areas())
        {
            room = 1;
            while (room < resident)
                room *= 2;
            room = static_cast<uint32_t>(std::max<size_t>(resident, std::min<size_t>(room, budget / per_scan)));
        }
        arena = static_cast<uint8_t*>(try_ensure(work_buffer(WorkBuffer::pipeline), per_scan * room + kCounterBytes));
        if (arena != nullptr || resident == 1)
            break;
        resident = (resident + 1) / 2;
    }
    if (arena == nullptr)
    { // no work area to be had: the one-wavefront kernel needs none (counted: charls_amd_engine_counters)
        note_pipeline_fallback(count);
        launch_encode_serial(d_descs, d_results, count, stream);
        last_timings().count = 2;
        return;
    }
    const uint32_t passes = (count + resident - 1) / resident;
    const uint32_t per_pass = (count + passes - 1) / passes; // passes of equal size (a short last pass fills the chip badly)
    // what the speculative stages did (tile::Counter), summed over the scans and passes of this call
    auto* d_counters = reinterpret_cast<uint32_t*>(arena + per_scan * resident);
    hip_check(hipMemsetAsync(d_counters, 0, kCounterBytes, stream));
    std::vector<std::vector<tile::Work>> works(passes);
    std::vector<std::vector<pipe::Work>> stuff_works(passes);
    std::vector<StageTimer> timers;
    timers.reserve(passes);
    // As in run_pipeline: the stuffing stage of a pass runs on a side stream under the next pass's stages A - C.
    const bool overlap_stuffing = passes > 1;
    hipStream_t stuff_stream = stream;
    EventList packed, stuffed;
    pipeline_lanes().ensure();
    if (overlap_stuffing)
    {
        stuff_stream = pipeline_lanes().streams[0];
        packed.grow(passes);
        stuffed.grow(passes);
    }
    hipStream_t runs_stream = pipeline_lanes().streams[1];
    EventList sorted(passes), runs_coded(passes);
    ensure_tile_attributes();

    for (uint32_t pass = 0; pass < passes; ++pass)
    {
        const uint32_t first = pass * per_pass;
        const uint32_t n = std::min(per_pass, count - first);
        hipStream_t s = stream;
        const size_t copy = pass & 1u;
        uint8_t* tables = arena + lay.bytes * per_pass;
        auto* d_works = reinterpret_cast<tile::Work*>(tables) + copy * per_pass;
        auto* d_stuff = reinterpret_cast<pipe::Work*>(tables + 2 * sizeof(tile::Work) * per_pass) + copy * per_pass;
        works[pass].resize(n);
        stuff_works[pass].resize(n);
        for (uint32_t i = 0; i < n; ++i)
        {
            uint8_t* base = arena + lay.bytes * i;
            tile::Work& w = works[pass][i];
            w.keyinv = reinterpret_cast<uint16_t*>(base + lay.off_keyinv);
            w.seg = reinterpret_cast<uint32_t*>(base + lay.off_seg);
            w.plan_part = reinterpret_cast<uint32_t*>(base + lay.off_planpart);
            w.chain_total = reinterpret_cast<uint32_t*>(base + lay.off_total);
            w.chain_base = reinterpret_cast<uint32_t*>(base + lay.off_base);
            w.job_first = reinterpret_cast<uint32_t*>(base + lay.off_jobfirst);
            w.rec = reinterpret_cast<uint32_t*>(base + lay.off_rec);
            w.code = reinterpret_cast<uint32_t*>(base + lay.off_code);
            w.jobs = reinterpret_cast<tile::JobState*>(base + lay.off_jobs);
            w.run_jobs = reinterpret_cast<tile::RunJob*>(base + lay.off_runjobs);
            w.run_job_events = lay.run_job_events;
            w.run_warm_events = lay.run_warm_events;
            w.rare_warm_events = lay.rare_warm_events;
            w.blockbase = reinterpret_cast<uint64_t*>(base + lay.off_bbase);
            w.tile_tail = reinterpret_cast<uint64_t*>(base + lay.off_bbase) + lay.tiles;
            w.raw = reinterpret_cast<uint32_t*>(base + lay.off_raw);
            w.raw_words = lay.raw_bytes / 4;
            w.total_bits = reinterpret_cast<uint64_t*>(base + lay.off_bits) + copy; // (zeroed by plan_chains)
            w.status = reinterpret_cast<uint32_t*>(base + lay.off_status) + copy;
            w.counters = d_counters;
            w.lines_per_tile = lay.lines_per_tile;
            w.tiles = lay.tiles;
            w.job_events = lay.job_events;
            w.warm_events = lay.warm_events;
            w.segs_per_line = lay.plan.segs_per_line;
            w.seg_pixels = lay.plan.seg_pixels;
            w.tile_capacity = lay.plan.tile_capacity;
            w.run_slots = tile::run_slots_of<S>();
            pipe::Work& sw = stuff_works[pass][i];
            std::memset(&sw, 0, sizeof sw);
            sw.raw = w.raw;
            sw.raw_words = w.raw_words;
            sw.total_bits = w.total_bits;
            sw.status = w.status;
            sw.stuff_tables = reinterpret_cast<uint32_t*>(base + lay.off_stuff);
        }
        hip_check(hipMemcpyAsync(d_works, works[pass].data(), sizeof(tile::Work) * n, hipMemcpyHostToDevice, s));
        hip_check(hipMemcpyAsync(d_stuff, stuff_works[pass].data(), sizeof(pipe::Work) * n, hipMemcpyHostToDevice, s));

        const ScanDesc* descs = d_descs + first;
        const uint32_t tiles_grid = 8 * ((lay.tiles + 7) / 8);
        const tile::TilePlan& plan = lay.plan;
        const bool pixel_mode = plan.mode == 2;
        const size_t lds_a = pixel_mode ? tile::analyze_pixel_lds_bytes(plan.lines_per_tile, plan.step, plan.max_pixels, plan.nc, sizeof(S), plan.tile_capacity)
                                        : tile::analyze_lds_bytes(proto.width, lay.lines_per_tile, sizeof(S), proto.interleave_mode);
        const size_t lds_b = pixel_mode ? tile::sort_pixel_lds_bytes(plan.lines_per_tile, plan.step, plan.max_pixels, plan.nc, sizeof(S), plan.tile_capacity)
                                        : tile::sort_lds_bytes(proto.width, lay.lines_per_tile, sizeof(S), proto.interleave_mode);
        timers.emplace_back(s);
        StageTimer& t = timers.back();
        t.mark();
        if (pixel_mode)
            hipLaunchKernelGGL((tile::analyze_pixel_tiles<S>), dim3(tiles_grid, n), dim3(tile::kThreads), lds_a, s, descs, d_works);
        else
            hipLaunchKernelGGL((tile::analyze_tiles<S, 0>), dim3(tiles_grid, n), dim3(tile::kThreads), lds_a, s, descs, d_works);
        t.mark();
        hipLaunchKernelGGL(tile::sum_chains, dim3(tile::kPlanGroups, n), dim3(tile::kPlanThreads), 0, s, descs, d_works);
        hipLaunchKernelGGL(tile::plan_chains, dim3(n), dim3(tile::kPlanThreads), 0, s, descs, d_works);
        hipLaunchKernelGGL(tile::apply_chains, dim3(tile::kPlanGroups, n), dim3(tile::kPlanThreads), 0, s, descs, d_works);
        if (pixel_mode)
            hipLaunchKernelGGL((tile::sort_pixel_tiles<S>), dim3(tiles_grid, n), dim3(tile::kThreads), lds_b, s, descs, d_works);
        else
            hipLaunchKernelGGL((tile::sort_tiles<S, 0>), dim3(tiles_grid, n), dim3(tile::kThreads), lds_b, s, descs, d_works);
        t.mark();
        // The run chain on a side stream under the walkers of the regular chains: it touches the run chain and the
        // interruption chain only, they every other chain.
        hip_check(hipEventRecord(sorted[pass], s));
        hip_check(hipStreamWaitEvent(runs_stream, sorted[pass], 0));
        {
            const uint32_t run_jobs = static_cast<uint32_t>(lay.max_run_jobs);
            const dim3 lanes((static_cast<uint64_t>(run_jobs) * n + 63) / 64);
            const dim3 count_grid(std::min<uint32_t>(run_jobs, std::max<uint32_t>(32, 4096 / n)), n);
            if (pixel_mode)
                hipLaunchKernelGGL((tile::count_runs<S, 1>), count_grid, dim3(64), 0, runs_stream, d_works, plan.nc);
            else
                hipLaunchKernelGGL((tile::count_runs<S, 0>), count_grid, dim3(64), 0, runs_stream, d_works, 1u);
            hipLaunchKernelGGL(tile::scan_runs, dim3(n), dim3(64), 0, runs_stream, d_works);
            if (proto.interleave_mode != 2)
            { // the context of the rarer interruption type, exactly (a sample-interleaved scan has one type only)
                if (pixel_mode)
                    hipLaunchKernelGGL((tile::compact_rare_runs<S, 1>), count_grid, dim3(64), 0, runs_stream, d_works);
                else
                    hipLaunchKernelGGL((tile::compact_rare_runs<S, 0>), count_grid, dim3(64), 0, runs_stream, d_works);
            }
            const uint32_t rare_blocks = proto.interleave_mode != 2 ? n : 0u; // (the walk of the rarer context rides with the warm-ups: a wavefront per scan)
#define JLS_RUN_CHAIN(ILV, FMT)                                                                                          \
    do                                                                                                                   \
    {                                                                                                                    \
        hipLaunchKernelGGL((tile::warm_run_jobs<S, ILV, FMT>), dim3(rare_blocks + lanes.x), dim3(64), 0, runs_stream, descs, d_works, n, rare_blocks); \
        hipLaunchKernelGGL((tile::walk_run_jobs<S, ILV, FMT>), lanes, dim3(64), 0, runs_stream, descs, d_works, n);      \
        hipLaunchKernelGGL((tile::settle_runs<S, ILV, FMT>), dim3(n), dim3(64), 0, runs_stream, descs, d_works, n);  \
    } while (0)
            if (!pixel_mode)
                JLS_RUN_CHAIN(0, 0);
            else if (proto.interleave_mode == 2)
                JLS_RUN_CHAIN(2, 1);
            else if (proto.interleave_mode == 1)
                JLS_RUN_CHAIN(1, 1);
            else
                JLS_RUN_CHAIN(0, 1);
#undef JLS_RUN_CHAIN
        }
        hip_check(hipEventRecord(runs_coded[pass], runs_stream));
        hipLaunchKernelGGL((tile::walk_jobs<S>), dim3(static_cast<uint32_t>((lay.max_jobs + 63) / 64), n), dim3(64), 0, s, descs, d_works);
        hipLaunchKernelGGL((tile::settle_chains<S>), dim3(pipe::kChains, n), dim3(64), 0, s, descs, d_works, n);
        hip_check(hipStreamWaitEvent(s, runs_coded[pass], 0));
        t.mark();
        if (overlap_stuffing && pass > 0)
            hip_check(hipStreamWaitEvent(s, stuffed[pass - 1], 0)); // the raw bits of the pass before have been read
        hipLaunchKernelGGL(tile::clear_pack_state, dim3(1, n), dim3(256), 0, s, d_works,
                           static_cast<uint32_t>(static_cast<size_t>(lay.tiles) * 16));
        hipLaunchKernelGGL((tile::pack_tiles<S>), dim3(lay.tiles, n), dim3(tile::pack_threads_for(lay.plan.tile_capacity)), tile::pack_lds_bytes(lay.plan.tile_capacity, proto.bits_per_sample), s,
                           descs, d_works);
        t.mark();
        if (overlap_stuffing)
        {
            hip_check(hipEventRecord(packed[pass], s));
            hip_check(hipStreamWaitEvent(stuff_stream, packed[pass], 0));
        }
        t.mark_on(stuff_stream);
        // Block-parallel stuffing is what ONE frame needs (a lane per KB of stream instead of a wavefront per frame); it
        // walks every chunk from 16 entry states, so with a wavefront's worth of frames per SIMD pair stuff_scan is cheaper.
        if (block_stuffing_enabled() && n <= kBlockStuffingScans)
        {
            const uint32_t chunk_waves = static_cast<uint32_t>((lay.raw_bytes / pipe::kStuffChunk + 1 + 63) / 64);
            const uint32_t survey_blocks = pipe::stuff_survey_blocks(lay.raw_bytes);
            hipLaunchKernelGGL(pipe::stuff_survey, dim3(survey_blocks, n), dim3(64), 0, stuff_stream, d_stuff);
            hipLaunchKernelGGL(pipe::stuff_resolve, dim3(n), dim3(pipe::kStuffResolveThreads), 0, stuff_stream, d_stuff);
            hipLaunchKernelGGL(pipe::stuff_emit, dim3(chunk_waves, n), dim3(64), 0, stuff_stream, descs, d_stuff, d_results + first);
        }
        else if (spec_stuffing_enabled() && (pass + 1 == passes || lay.raw_bytes >= kSpecStuffingAlwaysBytes))
        { // a wavefront per 64 KB of raw stream, from guessed entry states
            const pipe::SpecGeometry spec = pipe::stuff_spec_geometry();
            const uint32_t waves = static_cast<uint32_t>(lay.raw_bytes / spec.chunk_bytes + 1);
            hipLaunchKernelGGL(pipe::stuff_spec_survey, dim3(waves, n), dim3(64), 0, stuff_stream, d_stuff, spec.chunk_bytes, spec.warm_bytes);
            hipLaunchKernelGGL(pipe::stuff_spec_resolve, dim3(n), dim3(64), 0, stuff_stream, d_stuff, spec.chunk_bytes);
            hipLaunchKernelGGL(pipe::stuff_spec_emit, dim3(waves, n), dim3(64), 0, stuff_stream, descs, d_stuff, d_results + first, spec.chunk_bytes);
        }
        else
            hipLaunchKernelGGL(pipe::stuff_scan, dim3(n), dim3(64), 0, stuff_stream, descs, d_stuff, d_results + first);
        t.mark_on(stuff_stream);
        if (overlap_stuffing)
            hip_check(hipEventRecord(stuffed[pass], stuff_stream));
        hip_check(hipGetLastError());
    }
    if (overlap_stuffing)
        hip_check(hipStreamWaitEvent(stream, stuffed[passes - 1], 0));
    static_assert(tile::kCounters == tile_counter_count, "runtime.h: tile_counter_count");
    uint32_t counters[tile::kCounters] = {};
    hip_check(hipMemcpyAsync(counters, d_counters, sizeof counters, hipMemcpyDeviceToHost, stream));
    hip_check(hipStreamSynchronize(stream)); // the host copies of the work descriptors and the timers go out of scope
    for (uint32_t i = 0; i < tile::kCounters; ++i)
        g_speculation[i].fetch_add(counters[i]);
#ifdef JLS_PHASE_CLOCKS
    { // debug build (tools/phase_clocks.sh): the clocks the wavefronts of the tile kernels spent in each of their phases
        unsigned long long all[(kCounterBytes - 32) / 8] = {};
        hip_check(hipMemcpy(all, reinterpret_cast<const uint8_t*>(d_counters) + 32, sizeof all, hipMemcpyDeviceToHost));
        std::fprintf(stderr, "phase_clocks");
        for (unsigned long long v : all)
            std::fprintf(stderr, " %llu", v);
        std::fprintf(stderr, "\n");
    }
#endif
    Timings& tm = last_timings();
    double stage_ms[5] = {0, 0, 0, 0, 0};
    for (StageTimer& t : timers)
    {
        for (int i = 0; i < 4; ++i)
            stage_ms[i] += t.between(i, i + 1);
        stage_ms[4] += t.between(5, 6);
    }
    for (int i = 0; i < 5; ++i)
        tm.values[2 + i] = stage_ms[i];
    tm.count = 7;
}

} // namespace

bool pipeline_eligible(const ScanDesc& d) noexcept
{
    if (encode_engine() == EncodeEngine::serial)
        return false;
    if (d.near_lossless != 0)
        return false; // the template then holds reconstructed samples: nothing is known ahead of the chain
    const bool planar = d.interleave_mode == 0 && d.components == 1 && d.color_transformation == 0;
    const bool interleaved = d.interleave_mode != 0 && d.components >= 2 && d.components <= 4 &&
                             (d.color_transformation == 0 || d.components == 3);
    if (!planar && !interleaved)
        return false;
    const uint64_t samples = static_cast<uint64_t>(d.width) * d.height * static_cast<uint64_t>(d.components);
    if (samples >= (uint64_t{1} << 31))
        return false;
    if (d.reset == 0 && samples >= (uint64_t{1} << 23))
        return false; // N never halves (RESET = 256 m through the reference's uint8): it would outgrow the 24-bit multiplies of the chain stage
    if (d.bits_per_sample > 8 && ((reinterpret_cast<uintptr_t>(d.pixels) | d.pixel_stride) & 1u) != 0)
        return false;
    return true;
}

namespace {
// Restart-interval encode (extension): every interval is coded as a scan of its own into a private buffer, then the
// pieces are joined with RSTm markers (restart_intervals_encode.hip).  All `count` scans share proto's geometry and interval.
void launch_encode_intervals(const ScanDesc& proto, ScanDesc* d_descs, ScanResult* d_results, uint32_t count,
                             hipStream_t stream)
{
    const uint32_t lines = proto.restart_interval;
    const uint32_t intervals = (proto.height + lines - 1) / lines;
    ScanDesc sub_proto = proto;
    sub_proto.height = lines;
    sub_proto.restart_interval = 0;
    const size_t worst = worst_case_scan_bytes(proto.width, lines, proto.interleave_mode == 0 ? 1 : proto.components,
                                               proto.bits_per_sample);
    const bool needs_scratch = !pipeline_eligible(sub_proto);
    const size_t scratch_samples = needs_scratch ? line_scratch_samples(proto.width, proto.interleave_mode, proto.components) : 0;
    // First attempt: twice the interval's share of the destination (a destination sized by
    // charls_jpegls_encoder_get_estimated_destination_size leaves every interval more than it can use).  An interval
    // that does not fit its private buffer makes its group repeat with worst-case buffers, so the verdict
    // destination_too_small depends on the joined size only.
    const size_t first_capacity = std::min(worst, align_up(2 * (static_cast<size_t>(proto.stream_capacity) / intervals) + 4096, 256));
    constexpr size_t kBufferBudget = size_t{8} << 30; // private interval buffers in flight
    for (uint32_t first = 0; first < count;)
    {
        size_t capacity = first_capacity;
        uint32_t group = 0;
        for (int attempt = 0; attempt < 2; ++attempt)
        {
            group = static_cast<uint32_t>(std::max<size_t>(1, std::min<size_t>(count - first, kBufferBudget / (capacity * intervals))));
            const size_t subs_n = static_cast<size_t>(group) * intervals;
            auto* d_subs = static_cast<ScanDesc*>(work_buffer(WorkBuffer::interval_scans).ensure(sizeof(ScanDesc) * subs_n));
            auto* d_sub_results = static_cast<ScanResult*>(work_buffer(WorkBuffer::interval_results).ensure(sizeof(ScanResult) * subs_n));
            auto* d_offsets = static_cast<uint64_t*>(work_buffer(WorkBuffer::join_offsets).ensure(sizeof(uint64_t) * subs_n));
            auto* d_scratch = needs_scratch
                                  ? static_cast<uint16_t*>(work_buffer(WorkBuffer::interval_line_scratch).ensure(sizeof(uint16_t) * scratch_samples * subs_n))
                                  : nullptr;
            auto* d_buffers = static_cast<uint8_t*>(work_buffer(WorkBuffer::interval_buffers).ensure(capacity * subs_n));
            hipLaunchKernelGGL(interval::build_encode_intervals, dim3(intervals, group), dim3(1), 0, stream, d_descs + first,
                               intervals, d_buffers, static_cast<uint64_t>(capacity), d_scratch,
                               static_cast<uint64_t>(scratch_samples), d_subs);
            hip_check(hipGetLastError());
            sub_proto.stream_capacity = capacity;
            launch_encode(sub_proto, d_subs, d_sub_results, static_cast<uint32_t>(subs_n), stream);
            hipLaunchKernelGGL(interval::plan_join, dim3((group + 63) / 64), dim3(64), 0, stream, d_descs + first, intervals,
                               d_sub_results, d_offsets, d_results + first, group);
            hipLaunchKernelGGL(interval::join_intervals, dim3(intervals, group), dim3(256), 0, stream, d_descs + first, d_subs,
                               intervals, d_sub_results, d_offsets, d_results + first);
            hip_check(hipGetLastError());
            std::vector<ScanResult> results(group);
            hip_check(hipMemcpyAsync(results.data(), d_results + first, sizeof(ScanResult) * group, hipMemcpyDeviceToHost, stream));
            hip_check(hipStreamSynchronize(stream)); // the private buffers are reused by the next group
            bool again = false;
            for (const ScanResult& r : results)
                again = again || (r.flags & interval::kIntervalRetry) != 0;
            if (!again || capacity == worst)
                break;
            capacity = worst;
        }
        first += group;
    }
}
} // namespace

namespace {
// Lanes per scan of the group encoder (scan_group_encode.hip) for scans the parallel pipeline cannot take -- near-lossless
// single-component, sample-interleaved and line-interleaved scans; 0 = the one-lane kernel (lines that do not fit LDS).
int group_encode_lanes(const ScanDesc& d, uint32_t count)
{
    const bool shape = (d.interleave_mode != 0 && d.components >= 2 && d.components <= 4) || (d.interleave_mode == 0 && d.components == 1);
    if (!shape || encode_engine() == EncodeEngine::serial)
        return 0;
    if (d.reset == 0)
        return 0; // RESET = 256*m is stored as 0 by the reference: N is never halved and outgrows the 8 bits of the packed context
    int best = 0;
    for (int lanes = 64; lanes >= 8; lanes /= 2)
    {
        const uint32_t per_wave = 64u / static_cast<uint32_t>(lanes);
        if (group_encode_lds_bytes(d, per_wave) > kGroupDecodeLds)
            break;
        best = lanes;
        if ((count + per_wave - 1) / per_wave <= kPixelWaves) // (two one-wavefront workgroups per CU find a SIMD each, see decode_group_plan)
            break;
    }
    return best;
}

} // namespace

void launch_encode(const ScanDesc& proto, ScanDesc* d_descs, ScanResult* d_results, uint32_t count, hipStream_t stream)
{
    if (count == 0)
        return;
    if (proto.restart_interval != 0 && proto.restart_interval < proto.height)
    {
        launch_encode_intervals(proto, d_descs, d_results, count, stream);
        return;
    }
    if (!pipeline_eligible(proto))
    {
        if (encode_engine() == EncodeEngine::pipeline)
            raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT);
        const int lanes = group_encode_lanes(proto, count);
        if (lanes != 0)
            launch_encode_group(proto, lanes, d_descs, d_results, count, stream);
        else
            launch_encode_serial(d_descs, d_results, count, stream);
        return;
    }
    if (proto.bits_per_sample > 8)
        run_tile_pipeline<uint16_t>(proto, d_descs, d_results, count, stream);
    else
        run_tile_pipeline<uint8_t>(proto, d_descs, d_results, count, stream);
    // Scans whose destination is within 3 bytes of their size: the reference's verdict depends on its flush history
    // (src/scan_encoder.hpp:117-120), so those few are re-coded by the kernel that restates that history.
    std::vector<ScanResult> results(count);
    hip_check(hipMemcpyAsync(results.data(), d_results, sizeof(ScanResult) * count, hipMemcpyDeviceToHost, stream));
    hip_check(hipStreamSynchronize(stream));
    for (uint32_t i = 0; i < count; ++i)
        if (results[i].errc == kOk && (results[i].flags & 2u) != 0)
            launch_encode_serial(d_descs + i, d_results + i, 1, stream);
}

bool launch_measure(const ScanDesc& proto, const ScanDesc* d_descs, ScanResult* d_results, uint32_t count, hipStream_t stream)
{
    if (count == 0 || proto.restart_interval != 0)
        return false;
    const int lanes = group_encode_lanes(proto, count);
    if (lanes == 0)
        return false;
    launch_measure_group(proto, lanes, d_descs, d_results, count, stream);
    return true;
}

} // namespace jls::dev
