// runtime.hip -- device discovery, buffers, work areas, the serial kernels and the container kernels (see runtime.h); the decoder
// and encoder dispatch are decode_launch.hip and encode_launch.hip.  Compiled for gfx950 only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "runtime.h"
#include "scan_serial.hip"
#include "container_kernels.hip"
#include "work_areas.h"

namespace jls::dev {

namespace {
std::once_flag g_once;
charls_jpegls_errc g_status = CHARLS_AMD_ERRC_DEVICE_UNAVAILABLE;
std::atomic<int32_t> g_engine{0};
std::atomic<uint64_t> g_workspace_limit{0}; // charls_amd_set_workspace_limit; 0 = a quarter of the device

void probe() noexcept
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    {
        (void)hipGetLastError();
        return;
    }
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess)
        return;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess)
        return;
    // The code objects in this library are gfx950 only; any other device cannot run them.
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0 && std::getenv("CHARLS_AMD_ALLOW_ANY_ARCH") == nullptr)
        return;
    g_status = CHARLS_JPEGLS_ERRC_SUCCESS;
}
} // namespace

charls_jpegls_errc device_status() noexcept
{
    std::call_once(g_once, probe);
    return g_status;
}

void require_device()
{
    if (device_status() != CHARLS_JPEGLS_ERRC_SUCCESS)
        raise(CHARLS_AMD_ERRC_DEVICE_UNAVAILABLE);
}

// hipFree waits for every kernel that is running on the device.  While one of this library's decoder launches of the
// host-pointer ABI is in flight on a device -- ONE kernel that runs for seconds -- a block of that device that is given up (a
// buffer that grows) is not freed but set aside, and freed once no such launch is running there (profiles/r05_concurrent_kernels.txt:
// an encoder call that grew the shared work areas beside a running decoder took 2.9 s instead of 2 ms).  What is set aside is
// invisible HBM, so it is bounded: beyond kMaxDeferredBytes per device a block is freed on the spot (and waits), and an
// allocation that fails frees everything that was set aside -- waiting for the running launch if it has to -- and tries again.
namespace {
constexpr int kMaxDevices = 32;
constexpr size_t kMaxDeferredBytes = size_t{4} << 30;
struct DeferredFrees
{
    std::mutex guard;
    std::vector<std::pair<void*, size_t>> blocks[kMaxDevices];
    size_t bytes[kMaxDevices]{};
    std::atomic<int> long_kernels[kMaxDevices]{};
};
DeferredFrees& deferred()
{
    static DeferredFrees* d = new DeferredFrees; // never destroyed: a thread may give a buffer up while the process exits
    return *d;
}
int slot_of(int device) noexcept
{
    return device >= 0 && device < kMaxDevices ? device : 0;
}
int current_device() noexcept
{
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess)
    {
        (void)hipGetLastError();
        device = 0;
    }
    return device;
}
// Frees what was set aside on `device` (the calling thread's current device is restored).  `even_while_running`: the caller
// needs the memory now and waits for the launch that is in flight.
void reap_device(int device, bool even_while_running) noexcept
{
    DeferredFrees& d = deferred();
    const int slot = slot_of(device);
    if (!even_while_running && d.long_kernels[slot].load() > 0)
        return;
    std::vector<std::pair<void*, size_t>> gone;
    {
        std::lock_guard<std::mutex> lock(d.guard);
        gone.swap(d.blocks[slot]);
        d.bytes[slot] = 0;
    }
    if (gone.empty())
        return;
    const int before = current_device();
    if (before != device)
        (void)hipSetDevice(device);
    for (const auto& block : gone)
        (void)hipFree(block.first);
    if (before != device)
        (void)hipSetDevice(before);
}
} // namespace

void* DeviceBuffer::ensure(size_t bytes)
{
    int device = 0;
    hip_check(hipGetDevice(&device));
    // (memory of another device is of no use to the kernels this thread is about to launch: a thread that moved on to
    // another device starts over there)
    if (bytes <= cap_ && ptr_ && device == device_)
        return ptr_;
    release();
    const size_t want = bytes < 256 ? 256 : bytes;
    hipError_t e = hipMalloc(&ptr_, want);
    if (e == hipErrorOutOfMemory)
    { // what this library set aside is memory too
        (void)hipGetLastError();
        ptr_ = nullptr;
        reap_device(device, true);
        e = hipMalloc(&ptr_, want);
    }
    if (e != hipSuccess)
        ptr_ = nullptr;
    hip_check(e);
    cap_ = want;
    device_ = device;
    return ptr_;
}

void reap_deferred_frees() noexcept
{
    for (int device = 0; device < kMaxDevices; ++device)
        if (deferred().bytes[device] != 0) // (a racy look is fine: whoever set a block aside reaps again when its call ends)
            reap_device(device, false);
}

uint64_t deferred_free_bytes() noexcept
{
    DeferredFrees& d = deferred();
    std::lock_guard<std::mutex> lock(d.guard);
    uint64_t total = 0;
    for (int device = 0; device < kMaxDevices; ++device)
        total += d.bytes[device];
    return total;
}

void long_kernel_begins() noexcept
{
    deferred().long_kernels[slot_of(current_device())].fetch_add(1);
}

void long_kernel_ends() noexcept
{
    deferred().long_kernels[slot_of(current_device())].fetch_sub(1);
}

void DeviceBuffer::release() noexcept
{
    if (ptr_)
    {
        DeferredFrees& d = deferred();
        const int slot = slot_of(device_);
        bool set_aside = false;
        if (d.long_kernels[slot].load() > 0)
        {
            std::lock_guard<std::mutex> lock(d.guard);
            if (d.bytes[slot] + cap_ <= kMaxDeferredBytes)
            {
                d.blocks[slot].emplace_back(ptr_, cap_);
                d.bytes[slot] += cap_;
                set_aside = true;
            }
        }
        if (!set_aside)
        { // (the block may live on another device than the thread's current one: a handle that moved on)
            const int before = current_device();
            if (device_ >= 0 && before != device_)
                (void)hipSetDevice(device_);
            (void)hipFree(ptr_);
            if (device_ >= 0 && before != device_)
                (void)hipSetDevice(before);
        }
    }
    ptr_ = nullptr;
    cap_ = 0;
}

PinnedBuffer::~PinnedBuffer()
{
    release();
}

void PinnedBuffer::release() noexcept
{
    if (ptr_)
        (void)hipHostFree(ptr_);
    ptr_ = nullptr;
    cap_ = 0;
}

void* PinnedBuffer::ensure(size_t bytes)
{
    if (bytes <= cap_ && ptr_)
        return ptr_;
    if (ptr_)
        (void)hipHostFree(ptr_);
    ptr_ = nullptr;
    cap_ = 0;
    hip_check(hipHostMalloc(&ptr_, bytes < 256 ? 256 : bytes, hipHostMallocDefault));
    cap_ = bytes < 256 ? 256 : bytes;
    return ptr_;
}

EncodeEngine encode_engine() noexcept
{
    return static_cast<EncodeEngine>(g_engine.load());
}

void set_encode_engine(EncodeEngine e) noexcept
{
    g_engine.store(static_cast<int32_t>(e));
}

void set_workspace_limit(uint64_t bytes) noexcept
{
    g_workspace_limit.store(bytes);
}

namespace {
thread_local uint64_t t_workspace_limit = 0; // set_thread_workspace_limit: this thread's share of the limit
} // namespace

void set_thread_workspace_limit(uint64_t bytes) noexcept
{
    t_workspace_limit = bytes;
}

uint64_t workspace_limit() noexcept
{
    const uint64_t configured = g_workspace_limit.load();
    if (t_workspace_limit == 0)
        return configured;
    return configured != 0 ? std::min(configured, t_workspace_limit) : t_workspace_limit;
}

Timings& last_timings() noexcept
{
    static thread_local Timings t{};
    return t;
}

void launch_encode_serial(const ScanDesc* d_descs, ScanResult* d_results, uint32_t count, hipStream_t stream)
{
    if (count == 0)
        return;
    hipLaunchKernelGGL(encode_scans_serial, dim3(count), dim3(64), 0, stream, d_descs, d_results);
    hip_check(hipGetLastError());
}

void launch_decode_serial(const ScanDesc* d_descs, ScanResult* d_results, uint32_t count, hipStream_t stream)
{
    if (count == 0)
        return;
    hipLaunchKernelGGL(decode_scans_serial, dim3(count), dim3(64), 0, stream, d_descs, d_results);
    hip_check(hipGetLastError());
}

// Work areas (work_areas.h): one DeviceBuffer per role, and the side streams of the tile pipeline.
namespace {
struct WorkAreas
{
    DeviceBuffer buffers[static_cast<int>(WorkBuffer::count)];
    PipelineLanes lanes;
    size_t bytes() const noexcept
    {
        size_t total = 0;
        for (const DeviceBuffer& b : buffers)
            total += b.capacity();
        return total;
    }
    void release() noexcept
    {
        for (DeviceBuffer& b : buffers)
            b.release();
    }
};
thread_local WorkAreas* t_shared_areas = nullptr; // set by SharedAreasScope
WorkAreas& areas()
{
    if (t_shared_areas != nullptr)
        return *t_shared_areas;
    static thread_local WorkAreas mine;
    return mine;
}
} // namespace

DeviceBuffer& work_buffer(WorkBuffer which)
{
    return areas().buffers[static_cast<int>(which)];
}

PipelineLanes& pipeline_lanes()
{
    return areas().lanes;
}

bool on_shared_areas() noexcept
{
    return t_shared_areas != nullptr;
}

namespace {
constexpr size_t kArenaReserve = size_t{8} << 30; // HBM left to the caller (collective buffers, ...) when the device is nearly full
} // namespace

size_t arena_budget(size_t held)
{
    size_t free_bytes = 0, total_bytes = 0;
    if (hipMemGetInfo(&free_bytes, &total_bytes) != hipSuccess)
    {
        (void)hipGetLastError();
        return size_t{1} << 30;
    }
    const uint64_t configured = workspace_limit(); // (with the calling thread's share, where it has one)
    const size_t limit = configured != 0 ? static_cast<size_t>(configured) : total_bytes / 4;
    const size_t reachable = free_bytes + held;
    const size_t usable = reachable > kArenaReserve ? reachable - kArenaReserve : reachable / 2;
    return std::min(limit, usable);
}

// ensure() that reports failure instead of raising (the arena is released, so the next attempt starts clean).
void* try_ensure(DeviceBuffer& buffer, size_t bytes) noexcept
{
    try
    {
        return buffer.ensure(bytes);
    }
    catch (const error&)
    {
        (void)hipGetLastError();
        return nullptr;
    }
}

// Private stream buffers of the batch encoder's planar path (the component scans of a group of frames are coded into them
// and then put in place): gigabytes, so they are kept between calls like the pipeline's work areas -- allocating and
// freeing 8 GiB per call cost three times the coding of 256 4096 x 4096 RGB frames.
DeviceBuffer& plane_arena()
{
    return work_buffer(WorkBuffer::plane);
}

DeviceBuffer& pack_arena()
{
    return work_buffer(WorkBuffer::pack);
}

DeviceBuffer& transcode_arena()
{
    return work_buffer(WorkBuffer::transcode);
}

DeviceBuffer& index_scratch_arena()
{
    return work_buffer(WorkBuffer::index_scratch);
}

DeviceBuffer& band_edges_arena()
{
    return work_buffer(WorkBuffer::band_edges);
}

DeviceBuffer& seek_arena(int which)
{
    return areas().buffers[static_cast<int>(WorkBuffer::seek_first) + which];
}

size_t work_area_budget() noexcept
{
    return arena_budget(areas().bytes());
}

size_t work_area_budget_beside(size_t held_elsewhere) noexcept
{
    return arena_budget(areas().bytes() + held_elsewhere);
}

size_t shared_areas_keep_bytes() noexcept
{
    size_t free_bytes = 0, total_bytes = 0;
    if (hipMemGetInfo(&free_bytes, &total_bytes) != hipSuccess)
    {
        (void)hipGetLastError();
        return size_t{1} << 30;
    }
    const uint64_t configured = g_workspace_limit.load();
    const size_t eighth = total_bytes / 8;
    return configured != 0 ? std::min<size_t>(static_cast<size_t>(configured), eighth) : eighth;
}

// ---- the work areas of the host-pointer ABI: one set per device, used by one merged launch at a time
namespace {
struct SharedAreas
{
    std::mutex turn;
    WorkAreas areas;
    std::atomic<size_t> held{0};
};
std::atomic<SharedAreas*> g_shared[kMaxDevices]{};
SharedAreas& shared_areas(int device)
{
    std::atomic<SharedAreas*>& slot = g_shared[device >= 0 && device < kMaxDevices ? device : 0];
    SharedAreas* s = slot.load(std::memory_order_acquire);
    if (s == nullptr)
    {
        auto* fresh = new SharedAreas; // never destroyed: at process exit the HIP runtime may already be gone
        if (slot.compare_exchange_strong(s, fresh, std::memory_order_acq_rel))
            s = fresh;
        else
            delete fresh;
    }
    return *s;
}
} // namespace

SharedAreasScope::SharedAreasScope()
{
    hip_check(hipGetDevice(&device_));
    SharedAreas& s = shared_areas(device_);
    s.turn.lock();
    t_shared_areas = &s.areas;
}

SharedAreasScope::~SharedAreasScope()
{
    SharedAreas& s = shared_areas(device_);
    s.held.store(s.areas.bytes(), std::memory_order_relaxed);
    t_shared_areas = nullptr;
    s.turn.unlock();
}

size_t SharedAreasScope::bytes() const noexcept
{
    return shared_areas(device_).areas.bytes();
}

void SharedAreasScope::release() noexcept
{
    shared_areas(device_).areas.release();
}

size_t thread_work_area_bytes() noexcept
{
    return areas().bytes();
}

void release_thread_work_areas() noexcept
{
    areas().release();
}

void release_shared_work_areas() noexcept
{
    if (t_shared_areas != nullptr)
        return; // (called from inside a merged launch)
    int current = 0;
    const bool have_device = hipGetDevice(&current) == hipSuccess;
    for (int device = 0; device < kMaxDevices; ++device)
    {
        SharedAreas* s = g_shared[device].load(std::memory_order_acquire);
        if (s == nullptr)
            continue;
        std::lock_guard<std::mutex> turn(s->turn); // (a merged launch that is running finishes first)
        (void)hipSetDevice(device);
        s->areas.lanes.destroy();
        s->areas.release();
        s->held.store(0, std::memory_order_relaxed);
    }
    if (have_device)
        (void)hipSetDevice(current);
}

size_t shared_work_area_bytes() noexcept
{
    size_t total = 0;
    for (int device = 0; device < kMaxDevices; ++device)
        if (SharedAreas* s = g_shared[device].load(std::memory_order_acquire))
            total += s->held.load(std::memory_order_relaxed);
    return total;
}

void release_work_areas() noexcept
{
    areas().release();
    if (t_shared_areas != nullptr)
        return; // (called from inside a merged launch: its areas are the ones just released)
    release_shared_work_areas();
    reap_deferred_frees(); // (blocks that were set aside while a decoder launch of the host-pointer ABI ran)
}

size_t work_area_bytes() noexcept
{
    size_t total = areas().bytes();
    if (t_shared_areas == nullptr)
        for (int device = 0; device < kMaxDevices; ++device)
            if (SharedAreas* s = g_shared[device].load(std::memory_order_acquire))
                total += s->held.load(std::memory_order_relaxed);
    return total;
}


static_assert(sizeof(FrameCursorPod) == sizeof(FrameCursor), "cursor layout");

void launch_place_prologue(uint8_t* slots, uint64_t slot_pitch, const uint8_t* prologue, uint32_t prologue_size,
                           FrameCursorPod* cursors, uint32_t frames, hipStream_t stream)
{
    hipLaunchKernelGGL(place_prologue, dim3(frames), dim3(64), 0, stream, slots, slot_pitch, prologue, prologue_size,
                       reinterpret_cast<FrameCursor*>(cursors), frames);
    hip_check(hipGetLastError());
}

void launch_place_scan_header(uint8_t* slots, uint64_t slot_pitch, const uint8_t* header, uint32_t header_size,
                              FrameCursorPod* cursors, ScanDesc* descs, uint32_t frames, hipStream_t stream)
{
    hipLaunchKernelGGL(place_scan_header, dim3((frames + 63) / 64), dim3(64), 0, stream, slots, slot_pitch, header,
                       header_size, reinterpret_cast<FrameCursor*>(cursors), descs, frames);
    hip_check(hipGetLastError());
}

void launch_advance_cursor(FrameCursorPod* cursors, const ScanResult* results, uint32_t header_size, uint32_t frames,
                           hipStream_t stream)
{
    hipLaunchKernelGGL(advance_cursor, dim3((frames + 63) / 64), dim3(64), 0, stream,
                       reinterpret_cast<FrameCursor*>(cursors), results, header_size, frames);
    hip_check(hipGetLastError());
}

void launch_place_plane_scans(uint8_t* slots, uint64_t slot_pitch, const uint8_t* headers, uint32_t header_size, uint32_t rounds,
                              const uint8_t* private_streams, uint64_t capacity, const ScanResult* results, FrameCursorPod* cursors,
                              uint32_t* redo, uint32_t frames, hipStream_t stream)
{
    hipLaunchKernelGGL(place_plane_scans, dim3(frames * rounds, kPlaceShares), dim3(256), 0, stream, slots, slot_pitch, headers, header_size,
                       rounds, private_streams, capacity, results, reinterpret_cast<const FrameCursor*>(cursors));
    hipLaunchKernelGGL(advance_plane_cursors, dim3((frames + 63) / 64), dim3(64), 0, stream, slot_pitch, header_size, rounds, results,
                       reinterpret_cast<FrameCursor*>(cursors), redo, frames);
    hip_check(hipGetLastError());
}

void launch_find_scan_end(const uint8_t* slots, const MarkerSearch* searches, unsigned long long* found, uint32_t count, hipStream_t stream)
{
    hipLaunchKernelGGL(find_scan_end, dim3(count), dim3(256), 0, stream, slots, searches, found);
    hip_check(hipGetLastError());
}

void launch_place_epilogue(uint8_t* slots, uint64_t slot_pitch, FrameCursorPod* cursors, bool even_size, uint64_t* sizes,
                           uint32_t* errcs, uint32_t frames, hipStream_t stream)
{
    hipLaunchKernelGGL(place_epilogue, dim3((frames + 63) / 64), dim3(64), 0, stream, slots, slot_pitch,
                       reinterpret_cast<FrameCursor*>(cursors), even_size ? 1u : 0u, sizes, errcs, frames);
    hip_check(hipGetLastError());
}

} // namespace jls::dev
