// stream_windows.h -- what the batch decoders (batch_api.cpp, batch_index.cpp) share on the host: the windows through which
// the part-1 reader parses the marker segments of device-resident streams, and the ordinary decoder launch.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../device/runtime.h"
#include "common.h"
#include "event_timer.h"
#include "stream_reader.h"

namespace jls {

// One window of every listed stream -> a contiguous staging buffer (then ONE device-to-host copy instead of one small,
// synchronously staged copy per frame: 4096 of those were 60 ms per round of the batch decoder).
struct WindowSpec
{
    uint64_t offset; // from the first slot
    uint32_t bytes;
    uint32_t pad;
};
static __global__ void gather_windows(const uint8_t* __restrict__ slots, const WindowSpec* __restrict__ specs, uint8_t* __restrict__ out,
                               uint32_t window)
{
    const WindowSpec w = specs[blockIdx.x];
    const uint8_t* src = slots + w.offset;
    uint8_t* dst = out + (size_t)blockIdx.x * window;
    for (uint32_t b = threadIdx.x; b < w.bytes; b += blockDim.x)
        dst[b] = src[b];
}

struct BatchFrame
{
    StreamReader reader;
    std::vector<uint8_t> window; // host copy of [window_base, window_base + window.size())
    size_t window_base{};
    size_t cursor{};       // absolute offset of the next unparsed byte
    size_t plane_offset{}; // destination offset of the next scan
    uint32_t decoded_components{};
    charls_jpegls_errc errc{};
    bool done{};
};

// stream_at of the slot calls: frame i's stream in slot i, `pitch` bytes apart.  Raises invalid_argument_size for a pitch of
// 0 and for a stream longer than its slot.
inline std::vector<uint64_t> slot_offsets(uint32_t count, size_t pitch, const uint64_t* sizes)
{
    if (pitch == 0)
        raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_SIZE);
    std::vector<uint64_t> stream_at(count);
    for (uint32_t i = 0; i < count; ++i)
    {
        if (sizes[i] > pitch)
            raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_SIZE);
        stream_at[i] = static_cast<uint64_t>(i) * pitch;
    }
    return stream_at;
}

// The streams of a call and the host's windows into them.  Frame i's stream is the sizes[i] bytes at
// d_streams + stream_at[i] (both HOST arrays, which outlive the object).  Every frame's marker segments are parsed on the
// host by the part-1 reader.  Only a window of each stream is fetched: the first `kWindow` bytes up front, later windows at
// the position each scan ended.
class StreamWindows
{
public:
    static constexpr size_t kWindow = 2048;

    StreamWindows(uint32_t count, const void* d_streams, const uint64_t* stream_at, const uint64_t* sizes_arg, hipStream_t s)
        : slots(static_cast<const uint8_t*>(d_streams)), sizes(sizes_arg), stream(s), fr(count), stream_at_(stream_at)
    {
    }

    uint64_t offset_of(uint32_t i) const noexcept { return stream_at_[i]; } // of frame i's stream, from `slots`
    uint8_t* stream_ptr(uint32_t i, size_t cursor) const noexcept { return const_cast<uint8_t*>(slots) + stream_at_[i] + cursor; }

    void fetch(BatchFrame& x, uint32_t i, size_t base, size_t bytes)
    {
        const size_t avail = base < sizes[i] ? static_cast<size_t>(sizes[i]) - base : 0;
        const size_t n = std::min(bytes, avail);
        x.window.resize(n);
        x.window_base = base;
        if (n)
            dev::hip_check(hipMemcpyAsync(x.window.data(), slots + stream_at_[i] + base, n, hipMemcpyDeviceToHost, stream));
    }
    // the same for many frames at once (bases[k] is the offset of frame which[k]'s window): one gather on the device, one copy
    void fetch_many(std::vector<BatchFrame>& set, const std::vector<uint32_t>& which, const std::vector<size_t>& bases)
    {
        const size_t n = which.size();
        if (n == 0)
            return;
        auto* specs = static_cast<WindowSpec*>(h_specs_.ensure(sizeof(WindowSpec) * n));
        for (size_t k = 0; k < n; ++k)
        {
            const uint32_t i = which[k];
            const size_t avail = bases[k] < sizes[i] ? static_cast<size_t>(sizes[i]) - bases[k] : 0;
            specs[k] = WindowSpec{stream_at_[i] + bases[k], static_cast<uint32_t>(std::min(kWindow, avail)), 0};
        }
        d_specs_.ensure(sizeof(WindowSpec) * n);
        d_windows_.ensure(kWindow * n);
        auto* staged = static_cast<uint8_t*>(h_windows_.ensure(kWindow * n));
        dev::hip_check(hipMemcpyAsync(d_specs_.as<WindowSpec>(), specs, sizeof(WindowSpec) * n, hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(gather_windows, dim3(static_cast<uint32_t>(n)), dim3(256), 0, stream, slots, d_specs_.as<const WindowSpec>(),
                           d_windows_.as<uint8_t>(), static_cast<uint32_t>(kWindow));
        dev::hip_check(hipGetLastError());
        dev::hip_check(hipMemcpyAsync(staged, d_windows_.as<uint8_t>(), kWindow * n, hipMemcpyDeviceToHost, stream));
        dev::hip_check(hipStreamSynchronize(stream));
        for (size_t k = 0; k < n; ++k)
        {
            BatchFrame& x = set[which[k]];
            x.window.assign(staged + k * kWindow, staged + k * kWindow + specs[k].bytes);
            x.window_base = bases[k];
        }
    }
    // A parse that runs off the end of the window while the stream has more bytes is retried with a larger window.
    template <typename Body>
    void parse(std::vector<BatchFrame>& set, uint32_t i, Body&& body)
    {
        BatchFrame& x = set[i];
        size_t want = kWindow;
        const StreamReader snapshot = x.reader; // a failed attempt may have advanced the reader's state machine
        for (;;)
        {
            try
            {
                body(x);
                x.errc = CHARLS_JPEGLS_ERRC_SUCCESS;
                return;
            }
            catch (const error& e)
            {
                const bool truncated = x.window_base + x.window.size() < sizes[i];
                if (!truncated || (e.code != CHARLS_JPEGLS_ERRC_NEED_MORE_DATA && e.code != CHARLS_JPEGLS_ERRC_INVALID_MARKER_SEGMENT_SIZE &&
                                   e.code != CHARLS_JPEGLS_ERRC_DEFINE_NUMBER_OF_LINES_MARKER_NOT_FOUND))
                {
                    x.errc = e.code;
                    x.done = true;
                    return;
                }
            }
            want *= 8;
            fetch(x, i, x.window_base, want);
            dev::hip_check(hipStreamSynchronize(stream));
            x.reader = snapshot;
        }
    }
    // Every frame's header, up to the header of its first scan.  An abbreviated table stream has nothing to decode: an error
    // where `tables_are_errors`; the probe reports it as a stream without a frame.
    void read_headers(bool tables_are_errors)
    {
        const uint32_t n = static_cast<uint32_t>(fr.size());
        std::vector<uint32_t> all(n);
        for (uint32_t i = 0; i < n; ++i)
            all[i] = i;
        fetch_many(fr, all, std::vector<size_t>(n, 0));
        for (uint32_t i = 0; i < n; ++i)
            parse(fr, i, [&](BatchFrame& x) {
                x.reader.set_source(x.window.data(), x.window.size());
                x.reader.read_header();
                if (x.reader.end_of_image() && tables_are_errors)
                    raise(CHARLS_JPEGLS_ERRC_INVALID_OPERATION);
                x.cursor = x.window_base + static_cast<size_t>(x.reader.position() - x.window.data());
            });
    }
    // The frames `which` stand at `bases` (behind a scan): what follows is parsed on fresh windows, the next SOS, or the end
    // of the image where last[k].
    void parse_behind_scans(std::vector<BatchFrame>& set, const std::vector<uint32_t>& which, const std::vector<size_t>& bases,
                            const std::vector<uint8_t>& last)
    {
        fetch_many(set, which, bases);
        for (size_t k = 0; k < which.size(); ++k)
        {
            const bool end = last[k] != 0;
            parse(set, which[k], [&](BatchFrame& y) {
                y.reader.continue_on_window(y.window.data(), y.window.size()); // the same reader on the freshly fetched window
                if (end)
                    y.reader.read_end_of_image();
                else
                    y.reader.read_next_start_of_scan();
                y.cursor = y.window_base + static_cast<size_t>(y.reader.position() - y.window.data());
            });
        }
    }

    const uint64_t* offsets() const noexcept { return stream_at_; } // the table the object was made with

    const uint8_t* slots;
    const uint64_t* sizes;
    hipStream_t stream;
    std::vector<BatchFrame> fr;

private:
    const uint64_t* stream_at_;
    dev::DeviceBuffer d_specs_, d_windows_;
    dev::PinnedBuffer h_specs_, h_windows_;
};

// The whole-frame checks of a destination table of the caller's own (batch_streams.h: BatchDests with `ragged`), on frames
// whose headers are read: a stride below the frame's row is invalid_argument_stride, a capacity below the rows of all its
// planes invalid_argument_size, and the frame is done.  Defined in batch_api.cpp.
struct BatchDests;
void check_ragged_dests(StreamWindows& win, const BatchDests& to);

// charls_amd_decode_rows_batch_device_ragged behind its whole-call checks (batch_index.cpp: decode_bands), on frames whose
// headers are read: every frame of `s` that is not done yet gets its band or its errc; errcs[i] = s.fr[i].errc for the others.
void decode_row_bands(StreamWindows& s, const void* indexes, size_t index_pitch_bytes, const uint64_t* index_sizes,
                      const uint32_t* first_rows, const uint32_t* row_counts, const charls_amd_frame_dest* bands,
                      charls_jpegls_errc* errcs);
// The same whole-call checks (batch_index.cpp: the tables, the destinations, the offsets); needs no device.
void check_packed_index_call(uint32_t frame_count, const void* packed, const uint64_t* offsets, const uint64_t* sizes,
                             const charls_amd_frame_dest* dests, const uint64_t* index_sizes, const charls_jpegls_errc* errcs);

// The ordinary decoder launches for a set of scans of any geometry.  The device copies of the descriptors and results and
// the line scratch live as long as the object: a caller that decodes in rounds reuses them.
class DecodeLauncher
{
public:
    // `tolerant_clock`: for a caller that does not report gpu_ms() (EventTimer: nothing about the clock fails the call).
    explicit DecodeLauncher(hipStream_t stream, bool tolerant_clock = false) : stream_(stream), timer_(stream, tolerant_clock) {}

    // Decodes descs[k], all k, and leaves results[k] beside it.  The line scratch of every scan is placed here; scans that can
    // share a kernel specialisation go in one launch (dev::decode_launch_key), whatever their order in `descs`.
    void run(std::vector<ScanDesc>& descs, std::vector<ScanResult>& results)
    {
        const uint32_t n = static_cast<uint32_t>(descs.size());
        results.assign(n, ScanResult{});
        if (n == 0)
            return;
        size_t scratch_total = 0;
        std::vector<size_t> scratch_at(n);
        for (uint32_t k = 0; k < n; ++k)
        {
            scratch_at[k] = scratch_total;
            scratch_total += dev::line_scratch_samples(descs[k].width, descs[k].interleave_mode, descs[k].components) * sizeof(uint16_t);
            scratch_total = (scratch_total + 255) & ~size_t{255};
        }
        auto* scratch = static_cast<uint8_t*>(d_scratch_.ensure(scratch_total));
        std::vector<uint32_t> order(n);
        for (uint32_t k = 0; k < n; ++k)
        {
            order[k] = k;
            descs[k].line_scratch = reinterpret_cast<uint16_t*>(scratch + scratch_at[k]);
        }
        std::stable_sort(order.begin(), order.end(),
                         [&](uint32_t a, uint32_t b) { return dev::decode_launch_key(descs[a]) < dev::decode_launch_key(descs[b]); });
        std::vector<ScanDesc> sorted(n);
        for (uint32_t k = 0; k < n; ++k)
            sorted[k] = descs[order[k]];
        d_descs_.ensure(sizeof(ScanDesc) * n);
        d_results_.ensure(sizeof(ScanResult) * n);
        dev::hip_check(hipMemcpyAsync(d_descs_.as<ScanDesc>(), sorted.data(), sizeof(ScanDesc) * n, hipMemcpyHostToDevice, stream_));
        timer_.start();
        for (uint32_t first = 0; first < n;)
        {
            uint32_t last = first + 1;
            while (last < n && dev::decode_launch_key(sorted[last]) == dev::decode_launch_key(sorted[first]))
                ++last;
            dev::launch_decode(sorted[first], d_descs_.as<ScanDesc>() + first, d_results_.as<ScanResult>() + first, last - first, stream_);
            first = last;
        }
        timer_.stop();
        std::vector<ScanResult> got(n);
        dev::hip_check(hipMemcpyAsync(got.data(), d_results_.as<ScanResult>(), sizeof(ScanResult) * n, hipMemcpyDeviceToHost, stream_));
        dev::hip_check(hipStreamSynchronize(stream_)); // (the device copies are reused by the next call)
        gpu_ms_ += timer_.ms();
        for (uint32_t k = 0; k < n; ++k)
            results[order[k]] = got[k];
    }
    double gpu_ms() const noexcept { return gpu_ms_; } // of every launch so far

private:
    hipStream_t stream_;
    EventTimer timer_;
    dev::DeviceBuffer d_descs_, d_results_, d_scratch_;
    double gpu_ms_{};
};

} // namespace jls
