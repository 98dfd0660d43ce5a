// work_areas.h -- what the launch units (decode_launch.hip, encode_launch.hip) need from runtime.hip: the named buffers of a
// thread's work areas, the side streams of the tile pipeline and the budget.  Internal to device/: host/ sees runtime.h only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "runtime.h"

namespace jls::dev {

// Work areas: the HBM (and the side streams) a thread's launches keep between calls.  Every thread has a set of its own (the
// batch API; the workers of multi_device.cpp); the host-pointer ABI runs its merged launches on ONE set per device that is
// shared by all calling threads (SharedAreasScope), so that a pool of 256 threads does not end up with 256 arenas.
// One buffer per role: roles that are live together can never share.
enum class WorkBuffer : int
{
    pipeline, // the tile pipeline's arena
    plane,    // private stream buffers of the planar batch encoder
    pack,     // staging slots of the packed batch encoder
    transcode, // decoded frames of a window of charls_amd_transcode_batch_device
    index_scratch, // scratch frames of the index-only build: the frames that get no seek points, a window at a time
    band_edges, // the restart intervals that stick out of a row band (charls_amd.h part 2m), decoded whole beside it
    // restart-interval decode (launch_decode_intervals) and encode (launch_encode_intervals)
    marks,
    counts,
    interval_scans,
    interval_results,
    join_offsets,
    interval_buffers, // the private streams of the intervals: gigabytes
    interval_line_scratch,
    // the exact decoder's one launch behind a speed path (launch_decode_plain; runs inside the two interval decoders)
    retry_count,
    retry_index,
    retry_descs,
    retry_results,
    // launch_decode_salvage
    salvage_marks,
    salvage_segments,
    salvage_scans,
    salvage_results,
    salvage_lengths,
    salvage_status,
    salvage_counts,
    seek_first, // the kSeekArenas buffers of the seek-point index's batch calls (seek_arena)
    count = seek_first + kSeekArenas
};
DeviceBuffer& work_buffer(WorkBuffer which); // of the calling thread's set, or of the shared set it is on

// The calling thread runs on the shared set of the host-pointer ABI (inside a SharedAreasScope).
bool on_shared_areas() noexcept;

// Work-area budget of this call: the workspace limit, capped by what is free now (plus what the caller already holds).
size_t arena_budget(size_t held);

// Side streams of the pipeline (per set of work areas and device): the stuffing stage of a pass runs on one of them under the
// next pass's first stages, the run chain on another under the walkers of the regular chains.
constexpr int kMaxPipelineLanes = 2;
struct PipelineLanes
{
    hipStream_t streams[kMaxPipelineLanes]{};
    bool created = false;
    int device = -1; // streams belong to a device: a thread that moved on to another one gets new streams there
    ~PipelineLanes() { destroy(); }
    void destroy() noexcept
    {
        if (!created)
            return;
        int current = 0;
        const bool switched = hipGetDevice(&current) == hipSuccess && current != device && hipSetDevice(device) == hipSuccess;
        for (hipStream_t s : streams)
            (void)hipStreamDestroy(s);
        if (switched)
            (void)hipSetDevice(current);
        created = false;
    }
    void ensure()
    {
        int current = 0;
        hip_check(hipGetDevice(&current));
        if (created && current == device)
            return;
        destroy();
        for (hipStream_t& s : streams)
            hip_check(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        created = true;
        device = current;
    }
};
PipelineLanes& pipeline_lanes();

} // namespace jls::dev
