// batch_host.cpp -- the batch API on HOST memory (charls_amd.h part 2i): frames and streams in the caller's host memory, the
// PCIe copies overlapped with the coding inside the call.
//
//  * The frames are walked in the caller's order in WINDOWS (host_schedule.h: plan_windows), as many frames each as the
//    lanes' part of the workspace limit holds.  Window w is served by LANE w % lanes: a worker thread bound to the device for
//    life, with a stream, two device buffers and a pinned staging buffer of its own.  The device calls of part 2e block the
//    thread that makes them, not the copies other lanes have queued: with two or more lanes the upload of window k + 1 and
//    the download of window k - 1 run under the coding of window k.  (A lane is a thread because the work areas of the device
//    calls belong to the thread that made them: multi_device.cpp's Worker is the model.)  The uploads take turns in the
//    order of the windows: lanes that upload at once share the link, end together and then code together.
//  * Encode, per window: the rows go up packed (2-D copies: stride padding never crosses PCIe), the window is coded by
//    charls_amd_encode_batch_device_ragged into a blob of its own with offsets relative to the window, the lane waits at the
//    turnstile for the end offset of the window before it, settles its frames by the serial rule (host_schedule.h:
//    settle_window) and brings the front of the blob down with ONE copy.  The base of a window is a multiple of the alignment,
//    so the blob is in place as it is: no second pack.
//  * Decode, per window: the headers are parsed on the host (the bytes are here), exactly sizes[f] bytes per stream go up
//    into a packed device window, charls_amd_decode_batch_device_ragged decodes into packed device frames, 2-D copies write
//    the rows of the frames that succeeded at the caller's stride.
//  * Memory the caller pinned (hipPointerGetAttributes says so for its first and last byte) is copied from and to directly;
//    pageable memory goes through the lane's pinned staging buffer in two halves, one being filled while the other is copied.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "../device/knobs.h"
#include "../device/runtime.h"
#include "batch_streams.h"
#include "common.h"
#include "host_schedule.h"
#include "seek_index.h"
#include "stream_reader.h"

using namespace jls;
using dev::hip_check;
namespace hs = jls::host_schedule;

namespace {

// ---- charls_amd_host_counters [0] .. [4]
enum Counter
{
    kCalls,
    kWindows,
    kBytesUp,
    kBytesDown,
    kBytesStaged,
    kCounters
};
std::atomic<uint64_t> g_counters[kCounters];

void count(Counter c, uint64_t n) noexcept
{
    g_counters[c].fetch_add(n, std::memory_order_relaxed);
}

constexpr uint32_t kDefaultLanes = 3, kMaxLanes = 8;
constexpr size_t kDefaultStageBytes = size_t{64} << 20, kMinStageBytes = 512;
constexpr int kMaxDevices = 32;

inline size_t align_up(size_t v, size_t a) noexcept
{
    return (v + a - 1) & ~(a - 1);
}

// Whether the device can copy from / to [p, p + bytes) without the runtime staging it: host memory that HIP allocated or
// registered.  Anything else -- plain pageable memory, which older runtimes answer with an error -- goes through the
// lane's staging buffer.
bool pinned_byte(const void* p) noexcept
{
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess)
    {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

bool pinned_range(const void* p, size_t bytes) noexcept
{
    return bytes == 0 || (pinned_byte(p) && pinned_byte(static_cast<const uint8_t*>(p) + bytes - 1));
}

// A lane: a thread bound to one device, which runs one task at a time, and what it keeps between calls.
class Lane
{
public:
    explicit Lane(int device) : device_(device), thread_([this] { loop(); }) {}
    Lane(const Lane&) = delete;
    Lane& operator=(const Lane&) = delete;

    void submit(std::function<void()> task)
    {
        {
            std::lock_guard<std::mutex> lock(m_);
            task_ = std::move(task);
            pending_ = true;
            done_ = false;
        }
        cv_.notify_all();
    }
    charls_jpegls_errc wait()
    {
        std::unique_lock<std::mutex> lock(m_);
        cv_.wait(lock, [this] { return done_; });
        return result_;
    }

    // ---- the lane thread's own (a task reads and writes them; nobody else does)
    bool bound = false; // to the device, with a stream and events: a task on a lane that is not raises
    hipStream_t stream{};
    dev::DeviceBuffer frames, blob; // packed frames; the window's streams
    dev::PinnedBuffer stage;
    hipEvent_t half_done[2]{};

    void account() noexcept
    {
        device_bytes.store(frames.capacity() + blob.capacity() + dev::thread_work_area_bytes(), std::memory_order_relaxed);
        pinned_bytes.store(stage.capacity(), std::memory_order_relaxed);
    }
    void release_all() noexcept
    {
        frames.release();
        blob.release();
        stage.release();
        dev::release_thread_work_areas();
        account();
    }
    std::atomic<uint64_t> device_bytes{0}, pinned_bytes{0};

private:
    void loop()
    {
        bound = hipSetDevice(device_) == hipSuccess && hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) == hipSuccess;
        for (hipEvent_t& e : half_done)
            bound = bound && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
        for (;;) // (the lanes live as long as the process: nothing ends this loop)
        {
            std::function<void()> task;
            {
                std::unique_lock<std::mutex> lock(m_);
                cv_.wait(lock, [this] { return pending_; });
                task = std::move(task_);
                pending_ = false;
            }
            charls_jpegls_errc r = CHARLS_JPEGLS_ERRC_SUCCESS;
            try
            {
                task();
            }
            catch (...)
            {
                r = current_exception_to_errc();
                if (bound)
                    (void)hipStreamSynchronize(stream); // (nothing of a failed task stays queued on buffers the next one reuses)
                (void)hipGetLastError();
            }
            {
                std::lock_guard<std::mutex> lock(m_);
                result_ = r;
                done_ = true;
            }
            cv_.notify_all();
        }
    }

    int device_;
    std::mutex m_;
    std::condition_variable cv_;
    std::function<void()> task_;
    bool pending_ = false, done_ = true;
    charls_jpegls_errc result_ = CHARLS_JPEGLS_ERRC_SUCCESS;
    std::thread thread_; // (last: it starts in the constructor)
};

// The lanes of one device.  Never destroyed: the threads must not race the HIP runtime's own teardown at exit.
struct DeviceLanes
{
    std::mutex call; // calls on one device take turns
    std::vector<Lane*> lanes;
};
std::mutex g_lanes_guard;
DeviceLanes* g_lanes[kMaxDevices]{};

DeviceLanes& lanes_of(int device)
{
    std::lock_guard<std::mutex> lock(g_lanes_guard);
    DeviceLanes*& d = g_lanes[device >= 0 && device < kMaxDevices ? device : 0];
    if (d == nullptr)
        d = new DeviceLanes;
    return *d;
}

// Device bytes the lanes of the calling thread's current device hold now.
size_t lanes_hold() noexcept
{
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess)
    {
        (void)hipGetLastError();
        return 0;
    }
    std::lock_guard<std::mutex> lock(g_lanes_guard);
    const DeviceLanes* d = g_lanes[device >= 0 && device < kMaxDevices ? device : 0];
    size_t held = 0;
    if (d != nullptr)
        for (const Lane* lane : d->lanes)
            held += lane->device_bytes.load(std::memory_order_relaxed);
    return held;
}

// Pageable memory <-> device through the lane's staging buffer, in two halves: while the device copies from (to) one, the
// host fills (empties) the other.  An event per half says when the device is done with it.
class Stager
{
public:
    Stager(Lane& lane, size_t stage_bytes) : lane_(lane)
    {
        half_ = std::max(stage_bytes / 2, kMinStageBytes / 2);
        base_ = static_cast<uint8_t*>(lane.stage.ensure(half_ * 2));
        lane.account();
    }
    // `bytes` of a frame whose rows are `row` bytes long and `stride` apart, from packed position `from` on, between the
    // caller's memory and `where`.
    static void rows_in(uint8_t* where, const uint8_t* pixels, size_t row, size_t stride, size_t from, size_t bytes) noexcept
    {
        while (bytes != 0)
        {
            const size_t r = from / row, c = from % row, n = std::min(row - c, bytes);
            std::memcpy(where, pixels + r * stride + c, n);
            where += n, from += n, bytes -= n;
        }
    }
    static void rows_out(const uint8_t* where, uint8_t* pixels, size_t row, size_t stride, size_t from, size_t bytes) noexcept
    {
        while (bytes != 0)
        {
            const size_t r = from / row, c = from % row, n = std::min(row - c, bytes);
            std::memcpy(pixels + r * stride + c, where, n);
            where += n, from += n, bytes -= n;
        }
    }
    // Up: rows * row bytes of the caller's to d (packed).
    void up(uint8_t* d, const uint8_t* pixels, size_t row, size_t stride, size_t rows)
    {
        const size_t total = row * rows;
        for (size_t done = 0; done < total;)
        {
            size_t n = 0;
            uint8_t* p = take(total - done, n);
            if (stride == row)
                std::memcpy(p, pixels + done, n);
            else
                rows_in(p, pixels, row, stride, done, n);
            hip_check(hipMemcpyAsync(d + done, p, n, hipMemcpyHostToDevice, lane_.stream));
            hip_check(hipEventRecord(lane_.half_done[which_], lane_.stream));
            busy_[which_] = true;
            done += n;
        }
        count(kBytesStaged, total);
    }
    // Down: rows * row bytes from d (packed) to the caller's rows.  The copy into one half runs while the other is emptied.
    void down(const uint8_t* d, uint8_t* pixels, size_t row, size_t stride, size_t rows)
    {
        const size_t total = row * rows;
        struct Piece
        {
            uint8_t* p;
            size_t from, n;
            int half;
        } waiting{nullptr, 0, 0, 0};
        auto empty = [&](const Piece& x) {
            if (x.p == nullptr)
                return;
            hip_check(hipEventSynchronize(lane_.half_done[x.half]));
            busy_[x.half] = false;
            rows_out(x.p, pixels, row, stride, x.from, x.n);
        };
        for (size_t done = 0; done < total;)
        {
            // (a fresh half per piece: the piece before it is emptied while this one is on its way)
            flip();
            const size_t n = std::min(total - done, half_);
            hip_check(hipMemcpyAsync(base_ + which_ * half_, d + done, n, hipMemcpyDeviceToHost, lane_.stream));
            hip_check(hipEventRecord(lane_.half_done[which_], lane_.stream));
            busy_[which_] = true;
            empty(waiting);
            waiting = Piece{base_ + which_ * half_, done, n, which_};
            done += n;
        }
        empty(waiting);
        used_ = half_; // (the next take starts on a fresh half)
        count(kBytesStaged, total);
    }

private:
    void flip()
    {
        which_ ^= 1;
        if (busy_[which_])
        {
            hip_check(hipEventSynchronize(lane_.half_done[which_]));
            busy_[which_] = false;
        }
        used_ = 0;
    }
    // Room in the current half (the other one when this is full): at most `want` bytes, `got` says how many.
    uint8_t* take(size_t want, size_t& got)
    {
        if (used_ == half_)
            flip();
        got = std::min(want, half_ - used_);
        uint8_t* p = base_ + which_ * half_ + used_;
        used_ += got;
        return p;
    }

    Lane& lane_;
    uint8_t* base_{};
    size_t half_{};
    int which_{0};
    size_t used_{0};
    bool busy_[2]{false, false};
};

// Host <-> device copies of one lane: direct for pinned memory, through the stager otherwise.
struct Copier
{
    Lane& lane;
    size_t stage_bytes;
    std::unique_ptr<Stager> stager;

    Stager& staged()
    {
        if (!stager)
            stager = std::make_unique<Stager>(lane, stage_bytes);
        return *stager;
    }
    void up(uint8_t* d, const uint8_t* pixels, size_t row, size_t stride, size_t rows)
    {
        if (row == 0 || rows == 0)
            return;
        const size_t extent = stride * (rows - 1) + row;
        count(kBytesUp, row * rows);
        if (!pinned_range(pixels, extent))
            return staged().up(d, pixels, row, stride, rows);
        if (stride == row || rows == 1)
            hip_check(hipMemcpyAsync(d, pixels, row * rows, hipMemcpyHostToDevice, lane.stream));
        else
            hip_check(hipMemcpy2DAsync(d, row, pixels, stride, row, rows, hipMemcpyHostToDevice, lane.stream));
    }
    void down(const uint8_t* d, uint8_t* pixels, size_t row, size_t stride, size_t rows)
    {
        if (row == 0 || rows == 0)
            return;
        const size_t extent = stride * (rows - 1) + row;
        count(kBytesDown, row * rows);
        if (!pinned_range(pixels, extent))
            return staged().down(d, pixels, row, stride, rows);
        if (stride == row || rows == 1)
            hip_check(hipMemcpyAsync(pixels, d, row * rows, hipMemcpyDeviceToHost, lane.stream));
        else
            hip_check(hipMemcpy2DAsync(pixels, stride, d, row, row, rows, hipMemcpyDeviceToHost, lane.stream));
    }
};

// What a call decides before its windows start: lanes, the windows, every lane's share of the workspace limit.
struct Shape
{
    uint32_t lanes;
    std::vector<uint32_t> window_end;
    size_t budget;       // what all lanes together may hold on the device
    size_t own;          // device bytes of a lane's own two buffers
    size_t thread_limit; // what the device calls a lane makes may grow their work areas to
    size_t stage_bytes;
};

// `weights[f]`: the device bytes frame f needs in a lane's own buffers.  `whole` (decode): a window holds as many frames as
// the budget allows -- decoding is one serial chain per frame, its rate is the number of frames in flight --, and
// a batch that fits one window gets one lane with all of the budget; otherwise (encode) a window is short enough for every
// lane to get at least two: one window's copies run under another's coding only when there is another.  The knobs
// HOST_LANES and HOST_WINDOW_FRAMES force either.
Shape shape_call(const std::vector<uint64_t>& weights, bool whole)
{
    Shape s;
    const uint32_t count = static_cast<uint32_t>(weights.size());
    const long long forced_lanes = knobs::get_or(knobs::kHostLanes, 0), forced_window = knobs::get_or(knobs::kHostWindowFrames, 0);
    s.stage_bytes = static_cast<size_t>(std::max<long long>(knobs::get_or(knobs::kHostStageBytes, kDefaultStageBytes), kMinStageBytes));
    // All lanes together stay within what one thread's work areas may grow to; a lane's own buffers take half of its share
    // and the work areas of the device calls it makes the other half.
    // (what the lanes hold from earlier calls is theirs to use again: it counts as reachable, not as taken)
    const size_t budget = dev::work_area_budget_beside(lanes_hold());
    s.budget = budget;
    const uint64_t largest = count != 0 ? *std::max_element(weights.begin(), weights.end()) : 0;
    auto with_lanes = [&](uint32_t lanes, uint32_t most) {
        const size_t share = budget / lanes;
        s.lanes = lanes;
        s.own = share / 2;
        s.thread_limit = std::max<size_t>(share - s.own, 1);
        s.window_end = hs::plan_windows(weights, most, s.own);
    };
    if (whole && forced_lanes < 1 && forced_window < 1)
    {
        with_lanes(1, count);
        if (s.window_end.size() == 1 && largest <= s.own)
        { // (the one lane claims what it needs, not the whole budget: the idle lanes keep what they hold for the next call)
            uint64_t needed = 0;
            for (const uint64_t w : weights)
                needed += w;
            s.own = static_cast<size_t>(needed);
            s.thread_limit = std::min<size_t>(budget - s.own, std::max<size_t>(s.own, size_t{256} << 20));
            s.thread_limit = std::max<size_t>(s.thread_limit, 1);
            return s;
        }
    }
    uint32_t lanes = static_cast<uint32_t>(forced_lanes >= 1 ? std::min<long long>(forced_lanes, kMaxLanes) : kDefaultLanes);
    while (lanes > 1 && forced_lanes < 1 && largest > budget / lanes / 2)
        --lanes; // (fewer lanes before a frame that does not fit its lane's share)
    if (dev::workspace_limit() != 0 && largest > budget / lanes / 2)
        raise(CHARLS_JPEGLS_ERRC_NOT_ENOUGH_MEMORY);
    const uint32_t most = forced_window >= 1 ? static_cast<uint32_t>(std::min<long long>(forced_window, UINT32_MAX))
                          : whole            ? count
                                             : std::max<uint32_t>(1, (count + 2 * lanes - 1) / (2 * lanes));
    with_lanes(lanes, most);
    s.lanes = std::max<uint32_t>(1, std::min<uint32_t>(s.lanes, static_cast<uint32_t>(s.window_end.size())));
    return s;
}

// What a lane's work throws when it was stopped because another lane failed: that lane's error is the call's.
struct Stopped
{
};

// Runs work(lane, w) for every window w on the lane that serves it, the windows of a lane in rising order, and returns the
// first error.  `on_failure` runs on a lane whose work raised (it frees whoever waits for that lane).
template <typename Work, typename OnFailure>
charls_jpegls_errc on_lanes(const Shape& shape, Work work, OnFailure on_failure)
{
    int device = 0;
    hip_check(hipGetDevice(&device));
    DeviceLanes& d = lanes_of(device);
    std::lock_guard<std::mutex> turn(d.call);
    while (d.lanes.size() < shape.lanes)
    {
        std::lock_guard<std::mutex> lock(g_lanes_guard); // (the counters walk the list under it)
        d.lanes.push_back(new Lane(device));
    }
    // The lanes this call leaves idle keep what they hold only while it fits beside the shares of the others.
    uint64_t idle_hold = 0;
    for (size_t k = shape.lanes; k < d.lanes.size(); ++k)
        idle_hold += d.lanes[k]->device_bytes.load(std::memory_order_relaxed);
    if (idle_hold != 0 && idle_hold + static_cast<uint64_t>(shape.lanes) * (shape.own + shape.thread_limit) > shape.budget)
    {
        for (size_t k = shape.lanes; k < d.lanes.size(); ++k)
            d.lanes[k]->submit([lane = d.lanes[k]] { lane->release_all(); });
        for (size_t k = shape.lanes; k < d.lanes.size(); ++k)
            (void)d.lanes[k]->wait();
    }
    const uint32_t windows = static_cast<uint32_t>(shape.window_end.size());
    count(kCalls, 1);
    count(kWindows, windows);
    std::atomic<int32_t> cause{CHARLS_JPEGLS_ERRC_SUCCESS}; // the error of the lane that failed first, not of those it stopped
    uint32_t submitted = 0;
    try
    {
        for (; submitted < shape.lanes; ++submitted)
        {
            Lane* lane = d.lanes[submitted];
            lane->submit([&, lane, k = submitted] {
                struct ThreadLimit
                {
                    explicit ThreadLimit(uint64_t bytes) { dev::set_thread_workspace_limit(bytes); }
                    ~ThreadLimit() { dev::set_thread_workspace_limit(0); }
                } limit(shape.thread_limit);
                try
                {
                    if (!lane->bound)
                        raise(CHARLS_AMD_ERRC_DEVICE_FAILURE);
                    // What an earlier call under a larger share left behind goes first.  (Against the whole share, not its two
                    // halves: the encoder's areas may end a little above theirs, and giving gigabytes back to the driver
                    // on every call costs more than the call.)
                    if (lane->frames.capacity() + lane->blob.capacity() + dev::thread_work_area_bytes() > shape.own + shape.thread_limit)
                    {
                        lane->frames.release();
                        lane->blob.release();
                        dev::release_thread_work_areas();
                    }
                    for (uint32_t w = k; w < windows; w += shape.lanes)
                    {
                        work(*lane, w);
                        lane->account();
                    }
                }
                catch (const Stopped&)
                {
                    lane->account();
                    raise(CHARLS_AMD_ERRC_DEVICE_FAILURE);
                }
                catch (...)
                {
                    lane->account();
                    int32_t none = CHARLS_JPEGLS_ERRC_SUCCESS;
                    cause.compare_exchange_strong(none, current_exception_to_errc());
                    on_failure();
                    throw;
                }
            });
        }
    }
    catch (...)
    { // (a task could not be handed over: the lanes that got theirs are still waited for -- they refer to this frame's locals)
        int32_t none = CHARLS_JPEGLS_ERRC_SUCCESS;
        cause.compare_exchange_strong(none, current_exception_to_errc());
        on_failure();
    }
    charls_jpegls_errc first_error = CHARLS_JPEGLS_ERRC_SUCCESS;
    for (uint32_t k = 0; k < submitted; ++k)
    {
        const charls_jpegls_errc e = d.lanes[k]->wait();
        if (first_error == CHARLS_JPEGLS_ERRC_SUCCESS)
            first_error = e;
    }
    const auto caused = static_cast<charls_jpegls_errc>(cause.load());
    return caused != CHARLS_JPEGLS_ERRC_SUCCESS ? caused : first_error;
}

// The rows of a frame as the caller holds them: `rows` rows of `row` bytes, `stride` apart (all planes of a planar frame).
struct Extent
{
    size_t row, stride, rows;
    size_t packed() const noexcept { return row * rows; }
};

void check_host_sources(uint32_t frame_count, const charls_amd_frame_source* sources, const uint64_t* offsets, const uint64_t* sizes,
                        const charls_jpegls_errc* errcs, uint32_t offset_alignment)
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
}

void encode_host_ragged(uint32_t frame_count, const charls_amd_frame_source* sources, void* packed, size_t capacity, uint32_t alignment,
                        uint64_t* offsets, uint64_t* sizes, charls_jpegls_errc* errcs)
{
    // ---- every frame's own verdict, extent and slot, as the device call finds them: a frame the encoder refuses is not sent
    std::vector<Extent> extent(frame_count);
    std::vector<uint64_t> slot(frame_count, 0), weights(frame_count, 0);
    for (uint32_t f = 0; f < frame_count; ++f)
    {
        const charls_amd_frame_source& s = sources[f];
        sizes[f] = 0;
        errcs[f] = CHARLS_JPEGLS_ERRC_SUCCESS;
        try
        {
            const EncodePlan plan = plan_encode(s.params, SIZE_MAX, s.stride);
            const charls_frame_info& fi = s.params.frame_info;
            const size_t in_row = plan.scans == 1 ? static_cast<size_t>(fi.component_count) : 1;
            extent[f] = Extent{static_cast<size_t>(fi.width) * in_row * bytes_per_sample(fi.bits_per_sample), plan.stride,
                               static_cast<size_t>(fi.height) * plan.scans};
            slot[f] = s.max_stream_bytes != 0 ? s.max_stream_bytes : estimated_stream_bytes(s.params);
            weights[f] = align_up(extent[f].packed(), 256) + align_up(slot[f] + alignment, 256);
        }
        catch (const error& e)
        {
            errcs[f] = e.code;
        }
    }
    const Shape shape = shape_call(weights, false);
    // Two turnstiles: the uploads take turns in the order of the windows -- lanes that all upload at once share the link, end
    // together and then code together: nothing would run under anything --, and so do the offsets.
    hs::Turnstile uploads, turnstile;
    auto* out = static_cast<uint8_t*>(packed);

    auto window = [&](Lane& lane, uint32_t w) {
        const uint32_t first = w == 0 ? 0 : shape.window_end[w - 1], last = shape.window_end[w];
        Copier copy{lane, shape.stage_bytes, nullptr};
        std::vector<uint32_t> sent; // the frames of the window that go to the device
        size_t frames_bytes = 0, blob_bytes = 16;
        for (uint32_t f = first; f < last; ++f)
            if (errcs[f] == CHARLS_JPEGLS_ERRC_SUCCESS)
            {
                sent.push_back(f);
                frames_bytes += align_up(extent[f].packed(), 256);
                blob_bytes += static_cast<size_t>(hs::round_up(slot[f], alignment));
            }
        const uint32_t n = static_cast<uint32_t>(sent.size());
        std::vector<uint64_t> rel(last - first, 0);
        size_t coded_blob_bytes = 0;
        hs::Carry none{};
        if (!uploads.enter(w, none))
            throw Stopped{};
        if (n == 0)
            uploads.leave(w, none);
        else
        {
            auto* d_frames = static_cast<uint8_t*>(lane.frames.ensure(frames_bytes));
            auto* d_blob = static_cast<uint8_t*>(lane.blob.ensure(blob_bytes));
            lane.account();
            std::vector<charls_amd_frame_source> table(n);
            size_t at = 0;
            for (uint32_t k = 0; k < n; ++k)
            {
                const uint32_t f = sent[k];
                copy.up(d_frames + at, static_cast<const uint8_t*>(sources[f].d_pixels), extent[f].row, extent[f].stride, extent[f].rows);
                table[k] = sources[f];
                table[k].d_pixels = d_frames + at;
                table[k].stride = static_cast<uint32_t>(extent[f].row);
                at += align_up(extent[f].packed(), 256);
            }
            hip_check(hipStreamSynchronize(lane.stream)); // (the encoder works on side streams too: the frames are there first)
            uploads.leave(w, none);
            std::vector<uint64_t> w_offsets(n + 1), w_sizes(n);
            std::vector<charls_jpegls_errc> w_errcs(n);
            const charls_jpegls_errc rc = charls_amd_encode_batch_device_ragged(n, table.data(), d_blob, blob_bytes - 16, alignment, w_offsets.data(),
                                                                                w_sizes.data(), w_errcs.data(), lane.stream);
            if (rc != CHARLS_JPEGLS_ERRC_SUCCESS)
                raise(rc);
            for (uint32_t k = 0; k < n; ++k)
            {
                rel[sent[k] - first] = w_offsets[k];
                sizes[sent[k]] = w_sizes[k];
                errcs[sent[k]] = w_errcs[k];
            }
            coded_blob_bytes = static_cast<size_t>(w_offsets[n]);
        }
        // ---- in the caller's order from here: the windows before this one have left the turnstile
        hs::Carry in{};
        if (!turnstile.enter(w, in))
            throw Stopped{}; // (another lane failed: its error is the call's)
        const hs::Settled settled = hs::settle_window(in, last - first, rel.data(), sizes + first, errcs + first, offsets + first, capacity, alignment);
        if (!settled.consistent || settled.copy_bytes > coded_blob_bytes)
            raise(CHARLS_AMD_ERRC_DEVICE_FAILURE); // (the window's own offsets are not the rule's: nothing of it goes out)
        turnstile.leave(w, settled.out); // (the next window's lane goes on while this one's blob comes down)
        if (settled.copy_bytes != 0)
            copy.down(lane.blob.as<uint8_t>(), out + in.at, settled.copy_bytes, settled.copy_bytes, 1);
        hip_check(hipStreamSynchronize(lane.stream));
    };
    const charls_jpegls_errc rc = on_lanes(shape, window, [&] {
        uploads.abandon();
        turnstile.abandon();
    });
    if (rc != CHARLS_JPEGLS_ERRC_SUCCESS)
        raise(rc);
    offsets[frame_count] = turnstile.carry().at;
}

void decode_host_ragged(uint32_t frame_count, const void* packed, const uint64_t* offsets, const uint64_t* sizes,
                        const charls_amd_frame_dest* dests, charls_amd_codec_params* params_out, charls_jpegls_errc* errcs)
{
    // ---- the headers, where the bytes are: every frame's size, and its destination against it as part 2e checks it
    const auto* in = static_cast<const uint8_t*>(packed);
    std::vector<Extent> extent(frame_count);
    std::vector<uint64_t> weights(frame_count, 0);
    for (uint32_t f = 0; f < frame_count; ++f)
    {
        if (params_out != nullptr)
            params_out[f] = charls_amd_codec_params{};
        errcs[f] = CHARLS_JPEGLS_ERRC_SUCCESS;
        try
        {
            StreamReader reader;
            reader.set_source(in + offsets[f], static_cast<size_t>(sizes[f]));
            reader.read_header();
            if (reader.end_of_image())
                raise(CHARLS_JPEGLS_ERRC_INVALID_OPERATION); // (an abbreviated table stream: nothing to decode)
            const RowStride rs = row_and_stride(reader, dests[f].stride);
            const size_t rows = static_cast<size_t>(reader.frame_info().height) * scans_of_frame(reader);
            if (rs.stride < rs.row)
                raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_STRIDE);
            if (dests[f].capacity_bytes < rs.stride * rows - (rs.stride - rs.row))
                raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_SIZE);
            extent[f] = Extent{rs.row, rs.stride, rows};
            weights[f] = align_up(static_cast<size_t>(sizes[f]), 16) + 16 + align_up(extent[f].packed(), 256);
        }
        catch (const error& e)
        {
            errcs[f] = e.code;
        }
    }
    const Shape shape = shape_call(weights, true);
    hs::Turnstile uploads; // (the uploads of the windows take turns, as in the encoder)

    auto window = [&](Lane& lane, uint32_t w) {
        const uint32_t first = w == 0 ? 0 : shape.window_end[w - 1], last = shape.window_end[w];
        Copier copy{lane, shape.stage_bytes, nullptr};
        std::vector<uint32_t> sent;
        // (+ 32: the decoders load whole aligned 16-byte groups; the margin behind the last stream is part of the allocation)
        size_t frames_bytes = 0, blob_bytes = 32;
        for (uint32_t f = first; f < last; ++f)
            if (errcs[f] == CHARLS_JPEGLS_ERRC_SUCCESS)
            {
                sent.push_back(f);
                frames_bytes += align_up(extent[f].packed(), 256);
                blob_bytes += align_up(static_cast<size_t>(sizes[f]), 16);
            }
        const uint32_t n = static_cast<uint32_t>(sent.size());
        hs::Carry none{};
        if (!uploads.enter(w, none))
            throw Stopped{};
        if (n == 0)
            return uploads.leave(w, none);
        auto* d_frames = static_cast<uint8_t*>(lane.frames.ensure(frames_bytes));
        auto* d_blob = static_cast<uint8_t*>(lane.blob.ensure(blob_bytes));
        lane.account();
        std::vector<uint64_t> w_offsets(n), w_sizes(n);
        std::vector<charls_amd_frame_dest> table(n);
        size_t stream_at = 0, frame_at = 0;
        for (uint32_t k = 0; k < n; ++k)
        {
            const uint32_t f = sent[k];
            copy.up(d_blob + stream_at, in + offsets[f], static_cast<size_t>(sizes[f]), static_cast<size_t>(sizes[f]), 1);
            w_offsets[k] = stream_at;
            w_sizes[k] = sizes[f];
            table[k] = charls_amd_frame_dest{d_frames + frame_at, extent[f].packed(), 0, 0};
            stream_at += align_up(static_cast<size_t>(sizes[f]), 16);
            frame_at += align_up(extent[f].packed(), 256);
        }
        hip_check(hipStreamSynchronize(lane.stream));
        uploads.leave(w, none);
        std::vector<charls_amd_codec_params> w_params(n);
        std::vector<charls_jpegls_errc> w_errcs(n);
        const charls_jpegls_errc rc = charls_amd_decode_batch_device_ragged(n, d_blob, w_offsets.data(), w_sizes.data(), table.data(), w_params.data(),
                                                                            w_errcs.data(), lane.stream);
        if (rc != CHARLS_JPEGLS_ERRC_SUCCESS)
            raise(rc);
        for (uint32_t k = 0; k < n; ++k)
        {
            const uint32_t f = sent[k];
            errcs[f] = w_errcs[k];
            if (params_out != nullptr)
                params_out[f] = w_params[k];
            // (a frame that failed leaves its destination as it was)
            if (w_errcs[k] == CHARLS_JPEGLS_ERRC_SUCCESS)
                copy.down(static_cast<const uint8_t*>(table[k].d_pixels), static_cast<uint8_t*>(dests[f].d_pixels), extent[f].row, extent[f].stride,
                          extent[f].rows);
        }
        hip_check(hipStreamSynchronize(lane.stream));
    };
    const charls_jpegls_errc rc = on_lanes(shape, window, [&] { uploads.abandon(); });
    if (rc != CHARLS_JPEGLS_ERRC_SUCCESS)
        raise(rc);
}

// charls_amd_transcode_batch_host (charls_amd.h part 2j): the windows one after another on ONE lane -- streams up, the device
// call's body (batch_transcode.cpp: transcode_frames) on the device window, the front of its blob down.  Nothing runs under
// anything: a window's copies are two streams per frame, its decode is a dependency chain per frame.
// charls_amd_transcode_batch_host_budget (part 2k) hands over `budgets`, the candidates and `near_out`, which go to the device
// call's body window by window as its budgeted encode step; budgets == nullptr is the plain re-code.
void transcode_host(uint32_t frame_count, const void* packed_in, const uint64_t* offsets_in, const uint64_t* sizes_in,
                    const charls_amd_transcode_spec* specs, uint32_t spec_count, const uint64_t* budgets, const int32_t* near_candidates,
                    uint32_t candidate_count, void* packed_out, size_t capacity, uint32_t alignment, uint64_t* offsets_out,
                    uint64_t* sizes_out, int32_t* near_out, charls_amd_codec_params* params_out, charls_jpegls_errc* errcs)
{
    // ---- the headers, where the bytes are: what every frame will be coded with, the room its stream may take in the device
    // window, and what the device call needs for it in its own areas
    const auto* in = static_cast<const uint8_t*>(packed_in);
    std::vector<charls_amd_codec_params> coded_with(frame_count); // (zeroed where the header does not parse or holds no frame)
    std::vector<uint64_t> slot(frame_count, 0), weights(frame_count, 0);
    uint64_t largest = 0;
    for (uint32_t f = 0; f < frame_count; ++f)
    {
        try
        {
            StreamReader reader;
            reader.set_source(in + offsets_in[f], static_cast<size_t>(sizes_in[f]));
            reader.read_header();
            if (!reader.end_of_image())
            {
                const charls_frame_info& fi = reader.frame_info();
                const size_t bytes = checked_mul(checked_mul(checked_mul(static_cast<size_t>(fi.component_count), fi.height), fi.width),
                                                 bytes_per_sample(fi.bits_per_sample));
                coded_with[f] = transcode_params(params_of(reader), specs[spec_count == 1 ? 0 : f]);
                // The room of the frame's stream in the window's blob.  Plain re-code: the encoder's slot, which no stream it
                // writes exceeds.  Budgeted: the staging follows the MEASURED stream, which may be longer than that estimate
                // (noise coded losslessly) but never than the budget nor than the longest stream the code can produce.
                const uint64_t estimate = estimated_stream_bytes(coded_with[f]);
                slot[f] = hs::round_up(budgets != nullptr ? std::min<uint64_t>(budgets[f], longest_stream_bytes(coded_with[f])) : estimate, alignment);
                largest = std::max<uint64_t>(largest, std::max<uint64_t>(estimate, bytes));
            }
        }
        catch (const error&)
        { // (the device call reports it)
            coded_with[f] = charls_amd_codec_params{};
        }
        weights[f] = align_up(static_cast<size_t>(sizes_in[f]), 16) + 16 + align_up(static_cast<size_t>(slot[f]), 16);
    }
    Shape shape;
    shape.budget = dev::work_area_budget_beside(lanes_hold());
    shape.lanes = 1;
    shape.own = shape.budget / 2; // (the lane's two blobs; the device call's areas get the other half)
    shape.thread_limit = std::max<size_t>(shape.budget - shape.own, 1);
    shape.stage_bytes = static_cast<size_t>(std::max<long long>(knobs::get_or(knobs::kHostStageBytes, kDefaultStageBytes), kMinStageBytes));
    if (dev::workspace_limit() != 0 && largest > shape.thread_limit)
        raise(CHARLS_JPEGLS_ERRC_NOT_ENOUGH_MEMORY);
    const long long forced_window = knobs::get_or(knobs::kHostWindowFrames, 0);
    shape.window_end = hs::plan_windows(weights, forced_window >= 1 ? static_cast<uint32_t>(std::min<long long>(forced_window, UINT32_MAX)) : frame_count,
                                        shape.own);
    auto* out = static_cast<uint8_t*>(packed_out);
    hs::Carry carry{0, false}; // (one lane: its windows run in their order)

    auto window = [&](Lane& lane, uint32_t w) {
        const uint32_t first = w == 0 ? 0 : shape.window_end[w - 1], last = shape.window_end[w], n = last - first;
        if (carry.full)
        { // (behind the capacity: nothing of the window goes up)
            for (uint32_t f = first; f < last; ++f)
            {
                offsets_out[f] = carry.at;
                sizes_out[f] = 0;
                params_out[f] = coded_with[f];
                errcs[f] = CHARLS_JPEGLS_ERRC_DESTINATION_TOO_SMALL;
            }
            transcode_count_behind_capacity(n);
            return;
        }
        Copier copy{lane, shape.stage_bytes, nullptr};
        // (+ 32: the decoders load whole aligned 16-byte groups; the margin behind the last stream is part of the allocation)
        size_t in_bytes = 32, out_bytes = 0;
        for (uint32_t f = first; f < last; ++f)
        {
            in_bytes += align_up(static_cast<size_t>(sizes_in[f]), 16);
            out_bytes += static_cast<size_t>(slot[f]);
        }
        auto* d_in = static_cast<uint8_t*>(lane.blob.ensure(in_bytes));
        auto* d_out = static_cast<uint8_t*>(lane.frames.ensure(out_bytes + 16));
        lane.account();
        std::vector<uint64_t> w_offsets_in(n), w_offsets_out(static_cast<size_t>(n) + 1);
        size_t stream_at = 0;
        for (uint32_t k = 0; k < n; ++k)
        {
            const uint32_t f = first + k;
            copy.up(d_in + stream_at, in + offsets_in[f], static_cast<size_t>(sizes_in[f]), static_cast<size_t>(sizes_in[f]), 1);
            w_offsets_in[k] = stream_at;
            stream_at += align_up(static_cast<size_t>(sizes_in[f]), 16);
        }
        hip_check(hipStreamSynchronize(lane.stream)); // (the device call works on side streams too: the streams are there first)
        // Every stream fits the room its slot gives it, so the window's blob is as large as the caller's buffer needs it to be:
        // what is left of the capacity decides exactly as it does in one call over all frames.
        const uint64_t room = std::min<uint64_t>(out_bytes, capacity - std::min<uint64_t>(carry.at, capacity));
        const uint32_t beyond = transcode_frames(n, d_in, w_offsets_in.data(), sizes_in + first, specs + (spec_count == 1 ? 0 : first),
                                                 spec_count == 1 ? 1 : n, d_out, static_cast<size_t>(room), alignment, w_offsets_out.data(),
                                                 sizes_out + first, params_out + first, errcs + first,
                                                 budgets != nullptr ? transcode_encode_budget(budgets + first, near_candidates, candidate_count, near_out + first)
                                                                    : transcode_encode_plain(),
                                                 lane.stream);
        for (uint32_t k = 0; k < n; ++k)
            offsets_out[first + k] = carry.at + w_offsets_out[k];
        const size_t front = static_cast<size_t>(std::min<uint64_t>(w_offsets_out[n], room)); // (the zeros behind the last frame stop at the capacity)
        if (front != 0)
            copy.down(d_out, out + carry.at, front, front, 1);
        hip_check(hipStreamSynchronize(lane.stream));
        carry.at += w_offsets_out[n];
        carry.full = beyond != n;
    };
    const charls_jpegls_errc rc = on_lanes(shape, window, [] {});
    if (rc != CHARLS_JPEGLS_ERRC_SUCCESS)
        raise(rc);
    offsets_out[frame_count] = carry.at;
}

// charls_amd_index_batch_host (charls_amd.h part 2l): the index-only build on a host blob, the windows one after another on ONE
// lane as those of transcode_host -- streams up into a 16-byte granular device window, the device call's body
// (batch_index.cpp: index_packed_frames) on it.  Nothing comes down: indexes, sizes, parameters and errcs are host memory that
// the body writes itself.
void index_host(uint32_t frame_count, const void* packed, const uint64_t* offsets, const uint64_t* sizes, uint32_t lines, void* indexes,
                size_t index_pitch_bytes, uint64_t* index_sizes, charls_amd_codec_params* params_out, charls_jpegls_errc* errcs)
{
    const auto* in = static_cast<const uint8_t*>(packed);
    std::vector<uint64_t> weights(frame_count);
    for (uint32_t f = 0; f < frame_count; ++f)
        weights[f] = align_up(static_cast<size_t>(sizes[f]), 16) + 16;
    Shape shape;
    shape.budget = dev::work_area_budget_beside(lanes_hold());
    shape.lanes = 1;
    shape.own = shape.budget / 2; // (the lane's blob; the areas of the device call's body get the other half)
    shape.thread_limit = std::max<size_t>(shape.budget - shape.own, 1);
    shape.stage_bytes = static_cast<size_t>(std::max<long long>(knobs::get_or(knobs::kHostStageBytes, kDefaultStageBytes), kMinStageBytes));
    const long long forced_window = knobs::get_or(knobs::kHostWindowFrames, 0);
    shape.window_end = hs::plan_windows(weights, forced_window >= 1 ? static_cast<uint32_t>(std::min<long long>(forced_window, UINT32_MAX)) : frame_count,
                                        shape.own);

    auto window = [&](Lane& lane, uint32_t w) {
        const uint32_t first = w == 0 ? 0 : shape.window_end[w - 1], last = shape.window_end[w], n = last - first;
        Copier copy{lane, shape.stage_bytes, nullptr};
        // (+ 32: the decoders load whole aligned 16-byte groups; the margin behind the last stream is part of the allocation)
        size_t in_bytes = 32;
        for (uint32_t f = first; f < last; ++f)
            in_bytes += align_up(static_cast<size_t>(sizes[f]), 16);
        auto* d_in = static_cast<uint8_t*>(lane.blob.ensure(in_bytes));
        lane.account();
        std::vector<uint64_t> w_offsets(n);
        size_t stream_at = 0;
        for (uint32_t k = 0; k < n; ++k)
        {
            const uint32_t f = first + k;
            copy.up(d_in + stream_at, in + offsets[f], static_cast<size_t>(sizes[f]), static_cast<size_t>(sizes[f]), 1);
            w_offsets[k] = stream_at;
            stream_at += align_up(static_cast<size_t>(sizes[f]), 16);
        }
        hip_check(hipStreamSynchronize(lane.stream));
        index_packed_frames(n, d_in, w_offsets.data(), sizes + first, lines, static_cast<uint8_t*>(indexes) + static_cast<size_t>(first) * index_pitch_bytes,
                            index_pitch_bytes, index_sizes + first, params_out != nullptr ? params_out + first : nullptr, errcs + first, lane.stream);
    };
    const charls_jpegls_errc rc = on_lanes(shape, window, [] {});
    if (rc != CHARLS_JPEGLS_ERRC_SUCCESS)
        raise(rc);
}

} // namespace

// charls_amd_release_work_areas (misc_api.cpp): what the lanes hold, device and pinned.  The threads stay.
void jls::release_host_lanes() noexcept
{
    for (int device = 0; device < kMaxDevices; ++device)
    {
        DeviceLanes* d = nullptr;
        {
            std::lock_guard<std::mutex> lock(g_lanes_guard);
            d = g_lanes[device];
        }
        if (d == nullptr)
            continue;
        try
        {
            std::lock_guard<std::mutex> turn(d->call); // (a call that runs finishes first)
            for (Lane* lane : d->lanes)
                lane->submit([lane] { lane->release_all(); });
            for (Lane* lane : d->lanes)
                (void)lane->wait();
        }
        catch (...)
        {
        }
    }
}

// ---- pinned memory for callers without a HIP header ------------------------------------------------------------------------

extern "C" void* charls_amd_host_alloc(size_t size_bytes)
{
    if (dev::device_status() != CHARLS_JPEGLS_ERRC_SUCCESS)
        return nullptr;
    void* p = nullptr;
    if (hipHostMalloc(&p, size_bytes != 0 ? size_bytes : 1, hipHostMallocPortable) != hipSuccess)
    {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}

extern "C" void charls_amd_host_free(void* memory)
{
    if (memory != nullptr)
        (void)hipHostFree(memory);
}

extern "C" charls_jpegls_errc charls_amd_host_register(void* memory, size_t size_bytes)
try
{
    check_pointer(memory);
    check_argument(size_bytes != 0);
    dev::require_device();
    hip_check(hipHostRegister(memory, size_bytes, hipHostRegisterPortable));
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    (void)hipGetLastError();
    return current_exception_to_errc();
}

extern "C" charls_jpegls_errc charls_amd_host_unregister(void* memory)
try
{
    check_pointer(memory);
    dev::require_device();
    hip_check(hipHostUnregister(memory));
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    (void)hipGetLastError();
    return current_exception_to_errc();
}

extern "C" int32_t charls_amd_host_counters(uint64_t* out, int32_t capacity)
{
    uint64_t v[7];
    for (int i = 0; i < kCounters; ++i)
        v[i] = g_counters[i].load(std::memory_order_relaxed);
    v[5] = v[6] = 0;
    {
        std::lock_guard<std::mutex> lock(g_lanes_guard);
        for (DeviceLanes* d : g_lanes)
            if (d != nullptr)
                for (Lane* lane : d->lanes)
                {
                    v[5] += lane->device_bytes.load(std::memory_order_relaxed);
                    v[6] += lane->pinned_bytes.load(std::memory_order_relaxed);
                }
    }
    int32_t n = 0;
    for (; out != nullptr && n < capacity && n < 7; ++n)
        out[n] = v[n];
    return n;
}

// ---- the calls ---------------------------------------------------------------------------------------------------------------

extern "C" charls_jpegls_errc charls_amd_probe_batch_host_packed(uint32_t frame_count, const void* packed, const uint64_t* offsets,
                                                                 const uint64_t* sizes, charls_amd_codec_params* params_out,
                                                                 uint64_t* frame_bytes_out, charls_jpegls_errc* errcs)
try
{
    check_pointer(offsets);
    check_pointer(sizes);
    check_pointer(params_out);
    check_pointer(frame_bytes_out);
    check_pointer(errcs);
    if (frame_count == 0)
        return CHARLS_JPEGLS_ERRC_SUCCESS;
    check_pointer(packed);
    for (uint32_t f = 0; f < frame_count; ++f)
    {
        uint64_t end;
        if (__builtin_add_overflow(offsets[f], sizes[f], &end))
            raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_SIZE);
    }
    for (uint32_t f = 0; f < frame_count; ++f)
    {
        params_out[f] = charls_amd_codec_params{};
        frame_bytes_out[f] = 0;
        errcs[f] = CHARLS_JPEGLS_ERRC_SUCCESS;
        try
        {
            StreamReader reader;
            reader.set_source(static_cast<const uint8_t*>(packed) + offsets[f], static_cast<size_t>(sizes[f]));
            reader.read_header();
            if (reader.end_of_image())
                continue; // (an abbreviated table stream has no frame: zeros)
            const charls_frame_info& fi = reader.frame_info();
            const size_t bytes = checked_mul(checked_mul(checked_mul(static_cast<size_t>(fi.component_count), fi.height), fi.width),
                                             bytes_per_sample(fi.bits_per_sample));
            params_out[f] = params_of(reader);
            frame_bytes_out[f] = bytes;
        }
        catch (const error& e)
        {
            params_out[f] = charls_amd_codec_params{};
            errcs[f] = e.code;
        }
    }
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}

extern "C" charls_jpegls_errc charls_amd_encode_batch_host_ragged(uint32_t frame_count, const charls_amd_frame_source* sources, void* packed,
                                                                  size_t packed_capacity_bytes, uint32_t offset_alignment, uint64_t* offsets,
                                                                  uint64_t* sizes, charls_jpegls_errc* errcs)
try
{
    check_host_sources(frame_count, sources, offsets, sizes, errcs, offset_alignment);
    if (frame_count == 0)
    {
        offsets[0] = 0;
        return CHARLS_JPEGLS_ERRC_SUCCESS;
    }
    check_pointer(packed);
    dev::require_device();
    encode_host_ragged(frame_count, sources, packed, packed_capacity_bytes, offset_alignment, offsets, sizes, errcs);
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}

extern "C" charls_jpegls_errc charls_amd_decode_batch_host_ragged(uint32_t frame_count, const void* packed, const uint64_t* offsets,
                                                                  const uint64_t* sizes, const charls_amd_frame_dest* dests,
                                                                  charls_amd_codec_params* params_out, charls_jpegls_errc* errcs)
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
    check_pointer(packed);
    for (uint32_t f = 0; f < frame_count; ++f)
    {
        uint64_t end;
        if (__builtin_add_overflow(offsets[f], sizes[f], &end))
            raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_SIZE);
    }
    dev::require_device();
    decode_host_ragged(frame_count, packed, offsets, sizes, dests, params_out, errcs);
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}

// ---- one geometry, frames at a pitch: the tables are built here
extern "C" charls_jpegls_errc charls_amd_encode_batch_host(const charls_amd_codec_params* params, uint32_t frame_count, const void* frames,
                                                           size_t frame_pitch_bytes, uint32_t stride, void* packed, size_t packed_capacity_bytes,
                                                           uint32_t offset_alignment, size_t max_stream_bytes, uint64_t* offsets, uint64_t* sizes,
                                                           charls_jpegls_errc* errcs)
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
    check_pointer(frames);
    check_pointer(packed);
    check_encode_params(*params, frame_pitch_bytes, stride); // (the call's error, as charls_amd_encode_batch_device_packed has it)
    dev::require_device();
    std::vector<charls_amd_frame_source> sources(frame_count);
    for (uint32_t f = 0; f < frame_count; ++f)
        sources[f] = charls_amd_frame_source{*params, static_cast<const uint8_t*>(frames) + static_cast<size_t>(f) * frame_pitch_bytes, stride, 0,
                                             max_stream_bytes};
    encode_host_ragged(frame_count, sources.data(), packed, packed_capacity_bytes, offset_alignment, offsets, sizes, errcs);
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}

extern "C" charls_jpegls_errc charls_amd_decode_batch_host(uint32_t frame_count, const void* packed, const uint64_t* offsets, const uint64_t* sizes,
                                                           void* frames, size_t frame_pitch_bytes, uint32_t stride,
                                                           charls_amd_codec_params* params_out, charls_jpegls_errc* errcs)
try
{
    check_pointer(offsets);
    check_pointer(sizes);
    check_pointer(errcs);
    if (frame_count == 0)
        return CHARLS_JPEGLS_ERRC_SUCCESS;
    check_pointer(packed);
    check_pointer(frames);
    for (uint32_t f = 0; f < frame_count; ++f)
    {
        uint64_t end;
        if (__builtin_add_overflow(offsets[f], sizes[f], &end))
            raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_SIZE);
    }
    dev::require_device();
    std::vector<charls_amd_frame_dest> dests(frame_count);
    for (uint32_t f = 0; f < frame_count; ++f)
        dests[f] = charls_amd_frame_dest{static_cast<uint8_t*>(frames) + static_cast<size_t>(f) * frame_pitch_bytes, frame_pitch_bytes, stride, 0};
    std::vector<charls_amd_codec_params> found(frame_count);
    decode_host_ragged(frame_count, packed, offsets, sizes, dests.data(), found.data(), errcs);
    if (params_out != nullptr)
    { // (ONE element, as the packed call has it: the lowest-index frame that got as far as a scan)
        *params_out = charls_amd_codec_params{};
        for (uint32_t f = 0; f < frame_count; ++f)
            if (found[f].frame_info.width != 0)
            {
                *params_out = found[f];
                break;
            }
    }
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}

// ---- part 2j on host blobs
extern "C" charls_jpegls_errc charls_amd_transcode_batch_host(uint32_t frame_count, const void* packed_in, const uint64_t* offsets_in,
                                                              const uint64_t* sizes_in, const charls_amd_transcode_spec* specs, uint32_t spec_count,
                                                              void* packed_out, size_t packed_capacity_bytes, uint32_t offset_alignment,
                                                              uint64_t* offsets_out, uint64_t* sizes_out, charls_amd_codec_params* params_out,
                                                              charls_jpegls_errc* errcs)
try
{
    check_transcode_call(frame_count, packed_in, offsets_in, sizes_in, specs, spec_count, packed_out, offset_alignment, offsets_out, sizes_out,
                         params_out, errcs);
    if (frame_count == 0)
    {
        offsets_out[0] = 0;
        return CHARLS_JPEGLS_ERRC_SUCCESS;
    }
    dev::require_device();
    transcode_host(frame_count, packed_in, offsets_in, sizes_in, specs, spec_count, nullptr, nullptr, 0, packed_out, packed_capacity_bytes,
                   offset_alignment, offsets_out, sizes_out, nullptr, params_out, errcs);
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}

// ---- part 2k on host blobs
extern "C" charls_jpegls_errc charls_amd_transcode_batch_host_budget(
    uint32_t frame_count, const void* packed_in, const uint64_t* offsets_in, const uint64_t* sizes_in, const charls_amd_transcode_spec* specs,
    uint32_t spec_count, const uint64_t* budgets, const int32_t* near_candidates, uint32_t candidate_count, void* packed_out,
    size_t packed_capacity_bytes, uint32_t offset_alignment, uint64_t* offsets_out, uint64_t* sizes_out, int32_t* near_out,
    charls_amd_codec_params* params_out, charls_jpegls_errc* errcs)
try
{
    check_transcode_budget_call(frame_count, packed_in, offsets_in, sizes_in, specs, spec_count, budgets, near_candidates, candidate_count,
                                packed_out, offset_alignment, offsets_out, sizes_out, near_out, params_out, errcs);
    if (frame_count == 0)
    {
        offsets_out[0] = 0;
        return CHARLS_JPEGLS_ERRC_SUCCESS;
    }
    dev::require_device();
    transcode_host(frame_count, packed_in, offsets_in, sizes_in, specs, spec_count, budgets, near_candidates, candidate_count, packed_out,
                   packed_capacity_bytes, offset_alignment, offsets_out, sizes_out, near_out, params_out, errcs);
    transcode_near_of_uncoded(frame_count, errcs, near_out);
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}

// ---- part 2l on a host blob: the index-only build
extern "C" charls_jpegls_errc charls_amd_index_batch_host(uint32_t frame_count, const void* packed, const uint64_t* offsets, const uint64_t* sizes,
                                                          uint32_t lines_per_seek_point, void* indexes, size_t index_pitch_bytes,
                                                          uint64_t* index_sizes, charls_amd_codec_params* params_out, charls_jpegls_errc* errcs)
try
{
    check_pointer(offsets);
    check_pointer(sizes);
    check_pointer(index_sizes);
    check_pointer(errcs);
    check_argument(lines_per_seek_point > 0);
    if (frame_count == 0)
        return CHARLS_JPEGLS_ERRC_SUCCESS;
    check_pointer(packed);
    check_pointer(indexes);
    for (uint32_t f = 0; f < frame_count; ++f)
    {
        uint64_t end;
        if (__builtin_add_overflow(offsets[f], sizes[f], &end))
            raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_SIZE);
    }
    dev::require_device();
    index_host(frame_count, packed, offsets, sizes, lines_per_seek_point, indexes, index_pitch_bytes, index_sizes, params_out, errcs);
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}
