// batch_api.cpp -- charls_amd_encode_batch_device / charls_amd_decode_batch_device (charls_amd.h part 2).
//
// The batch is the engine's native unit: `frame_count` independent frames resident in HBM, every scan of every frame a
// separate chain of work for the GPU (frames shard with no exchange).  The container bytes around the
// entropy-coded segments are produced by the same StreamWriter the part-1 encoder uses, and parsed by the same
// StreamReader the part-1 decoder uses, so each frame's .jls file / error code is what part 1 gives for that frame.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../device/knobs.h"
#include "../device/runtime.h"
#include "batch_streams.h"
#include "common.h"
#include "event_timer.h"
#include "preset.h"
#include "seek_index.h"
#include "stream_reader.h"
#include "stream_windows.h"
#include "stream_writer.h"

using namespace jls;
using dev::hip_check;

namespace {
// Validation of the coding parameters: the checks charls_jpegls_encoder::encode_components performs before any scan
// is coded (reference src/charls_jpegls_encoder.cpp:182-207, 298-358).
void validate_encode(const charls_amd_codec_params& p, size_t frame_pitch, uint32_t stride_arg, size_t* stride_out,
                     charls_jpegls_pc_parameters* pc_out)
{
    const charls_frame_info& f = p.frame_info;
    check_argument(f.width >= 1 && f.width <= kMaxDimension, CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_WIDTH);
    check_argument(f.height >= 1 && f.height <= kMaxDimension, CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_HEIGHT);
    check_argument(f.bits_per_sample >= kMinBits && f.bits_per_sample <= kMaxBits,
                   CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_BITS_PER_SAMPLE);
    check_argument(f.component_count >= 1 && f.component_count <= kMaxComponents,
                   CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_COMPONENT_COUNT);
    check_argument(p.near_lossless >= 0 && p.near_lossless <= kMaxNear, CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_NEAR_LOSSLESS);
    check_argument(p.interleave_mode >= 0 && p.interleave_mode <= 2, CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_INTERLEAVE_MODE);
    check_argument(p.color_transformation >= 0 && p.color_transformation <= 3,
                   CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_COLOR_TRANSFORMATION);
    check_argument(p.encoding_options <= 7u, CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_ENCODING_OPTIONS);
    if (f.component_count == 1 && p.interleave_mode != 0)
        raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_INTERLEAVE_MODE);
    if (p.interleave_mode != 0 && f.component_count > kMaxComponentsInScan)
        raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_COMPONENT_COUNT);
    const int32_t bit_maxval = bit_max_value(f.bits_per_sample);
    int32_t maxval = bit_maxval;
    if (p.preset_coding_parameters.maximum_sample_value != 0)
    {
        if (p.preset_coding_parameters.maximum_sample_value < 1 || p.preset_coding_parameters.maximum_sample_value > bit_maxval)
            raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_JPEGLS_PC_PARAMETERS);
        maxval = p.preset_coding_parameters.maximum_sample_value;
    }
    if (p.near_lossless > max_near_for(maxval))
        raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_NEAR_LOSSLESS);
    const size_t row = static_cast<size_t>(f.width) * bytes_per_sample(f.bits_per_sample) *
                       (p.interleave_mode == 0 ? 1u : static_cast<size_t>(f.component_count));
    size_t stride = stride_arg;
    if (stride == 0)
        stride = row;
    else if (stride < row)
        raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_STRIDE);
    const size_t need = (p.interleave_mode == 0 ? checked_mul(stride * static_cast<size_t>(f.component_count), f.height)
                                                : checked_mul(stride, f.height)) -
                        (stride - row);
    if (frame_pitch < need)
        raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_SIZE);
    if (!pc_validate(p.preset_coding_parameters, bit_maxval, p.near_lossless, pc_out))
        raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_JPEGLS_PC_PARAMETERS);
    if (p.color_transformation != 0 && !color_transformation_possible(f, p.near_lossless, p.interleave_mode))
        raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_COLOR_TRANSFORMATION);
    if (f.component_count * 3 + 32 > 400)
        raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_COMPONENT_COUNT); // batch API: at most ~120 components (the prologue buffer)
    *stride_out = stride;
}

// A scan of the frames of `p`: one component of a planar frame, all of them otherwise (pc: validated).
ScanSpec scan_spec_for(const charls_amd_codec_params& p, const charls_jpegls_pc_parameters& pc) noexcept
{
    const charls_frame_info& f = p.frame_info;
    return ScanSpec{f.width, f.height, p.interleave_mode == 0 ? 1 : f.component_count, p.interleave_mode, f.bits_per_sample,
                    p.near_lossless, p.color_transformation, pc, p.restart_interval};
}

// The container bytes in front of a frame's first scan, by the writer of part 1; returns their number.
size_t write_prologue(const charls_amd_codec_params& p, const charls_jpegls_pc_parameters& pc, uint8_t* to, size_t capacity)
{
    const charls_frame_info& f = p.frame_info;
    StreamWriter w;
    w.set_destination(to, capacity);
    w.start_of_image();
    if (p.encoding_options & 2u)
    {
        static const char version[] = "charls 3.0.0";
        w.comment(reinterpret_cast<const uint8_t*>(version), sizeof version);
    }
    if (p.color_transformation != 0)
        w.color_transform(p.color_transformation);
    if (w.start_of_frame(f))
        w.oversize_dimensions(f.height, f.width);
    if (!pc_is_default(p.preset_coding_parameters, default_pc(bit_max_value(f.bits_per_sample), p.near_lossless)) ||
        ((p.encoding_options & 4u) && f.bits_per_sample > 12))
        w.preset_coding_parameters(pc);
    if (p.restart_interval != 0)
        w.define_restart_interval(p.restart_interval);
    return w.bytes_written();
}

thread_local bool t_force_rounds = false; // the batch encoder codes the component scans of planar frames one round per component

} // namespace

void jls::check_encode_params(const charls_amd_codec_params& params, size_t frame_bytes, uint32_t stride_arg)
{
    size_t stride = 0;
    charls_jpegls_pc_parameters pc{};
    validate_encode(params, frame_bytes, stride_arg, &stride, &pc);
}

// What the encoder below does with `params` before it codes anything, for a caller that sizes streams without writing them
// (batch_budget.cpp): the same validation, the scan descriptor without its pointers, the container bytes around the segments.
EncodePlan jls::plan_encode(const charls_amd_codec_params& p, size_t frame_bytes, uint32_t stride_arg)
{
    EncodePlan plan{};
    charls_jpegls_pc_parameters pc{};
    validate_encode(p, frame_bytes, stride_arg, &plan.stride, &pc);
    const charls_frame_info& f = p.frame_info;
    plan.scans = p.interleave_mode == 0 ? static_cast<uint32_t>(f.component_count) : 1u;
    const int32_t comps_per_scan = p.interleave_mode == 0 ? 1 : f.component_count;
    plan.scan = desc_of(scan_spec_for(p, pc));
    plan.scan.pixel_stride = plan.stride;
    uint8_t prologue[512];
    plan.container_bytes = write_prologue(p, pc, prologue, sizeof prologue);
    std::vector<uint8_t> tmp(static_cast<size_t>(plan.scans) * 16);
    StreamWriter ws;
    ws.set_destination(tmp.data(), tmp.size());
    for (uint32_t r = 0; r < plan.scans; ++r)
        ws.start_of_scan(comps_per_scan, p.near_lossless, p.interleave_mode);
    plan.container_bytes += ws.bytes_written();
    return plan;
}

// The batch encoder behind charls_amd_encode_batch_device (frames[i] = d_frames + i * frame_pitch_bytes) and
// charls_amd_encode_batch_device_ragged (batch_ragged.cpp: the frames of one group of a window, wherever they lie): frame
// i's pixels start at frames[i].  frame_count >= 1, the pointers are checked by the entry points.
void jls::encode_batch_frames(const charls_amd_codec_params& p, uint32_t frame_count, const uint8_t* const* frames,
                              size_t frame_pitch_bytes, uint32_t stride_arg, void* d_streams, size_t stream_pitch_bytes,
                              uint64_t* sizes, charls_jpegls_errc* errcs, void* hip_stream)
{
    dev::require_device();
    size_t stride = 0;
    charls_jpegls_pc_parameters pc{};
    validate_encode(p, frame_pitch_bytes, stride_arg, &stride, &pc);
    const charls_frame_info& f = p.frame_info;
    auto stream = static_cast<hipStream_t>(hip_stream);

    // ---- container bytes, produced once on the host by the writer of part 1
    uint8_t prologue[512];
    const uint32_t prologue_size = static_cast<uint32_t>(write_prologue(p, pc, prologue, sizeof prologue));

    const uint32_t rounds = p.interleave_mode == 0 ? static_cast<uint32_t>(f.component_count) : 1u;
    const int32_t comps_per_scan = p.interleave_mode == 0 ? 1 : f.component_count;
    std::vector<std::vector<uint8_t>> sos(rounds);
    {
        std::vector<uint8_t> tmp(static_cast<size_t>(rounds) * 16);
        StreamWriter ws; // one writer for all scans: component identifiers keep counting across scans
        ws.set_destination(tmp.data(), tmp.size());
        for (uint32_t r = 0; r < rounds; ++r)
        {
            const size_t before = ws.bytes_written();
            ws.start_of_scan(comps_per_scan, p.near_lossless, p.interleave_mode);
            sos[r].assign(tmp.data() + before, tmp.data() + ws.bytes_written());
        }
    }

    // ---- device work areas
    const size_t scratch_samples = dev::line_scratch_samples(f.width, p.interleave_mode, comps_per_scan);
    dev::DeviceBuffer d_descs, d_results, d_cursors, d_scratch, d_blob, d_sizes, d_errcs;
    d_descs.ensure(sizeof(ScanDesc) * frame_count);
    d_results.ensure(sizeof(ScanResult) * frame_count);
    d_cursors.ensure(sizeof(dev::FrameCursorPod) * frame_count);
    d_scratch.ensure(scratch_samples * sizeof(uint16_t) * frame_count);
    d_sizes.ensure(sizeof(uint64_t) * frame_count);
    d_errcs.ensure(sizeof(uint32_t) * frame_count);
    size_t blob_bytes = prologue_size;
    for (auto& s : sos)
        blob_bytes += s.size();
    std::vector<uint8_t> blob(blob_bytes);
    std::memcpy(blob.data(), prologue, prologue_size);
    {
        size_t o = prologue_size;
        for (auto& s : sos)
        {
            std::memcpy(blob.data() + o, s.data(), s.size());
            o += s.size();
        }
    }
    d_blob.ensure(blob_bytes);
    hip_check(hipMemcpyAsync(d_blob.as<uint8_t>(), blob.data(), blob_bytes, hipMemcpyHostToDevice, stream));

    std::vector<ScanDesc> descs(frame_count);
    const ScanDesc scan = desc_of(scan_spec_for(p, pc)); // every scan of every frame, without its pointers
    auto* slots = static_cast<uint8_t*>(d_streams);

    EventTimer total(stream), scans(stream);
    double scan_ms = 0;
    dev::last_timings().count = 0;
    total.start();
    dev::launch_place_prologue(slots, stream_pitch_bytes, d_blob.as<uint8_t>(), prologue_size,
                               d_cursors.as<dev::FrameCursorPod>(), frame_count, stream);
    size_t blob_offset = prologue_size;
    // ---- the component scans of planar frames TOGETHER (reference src/charls_jpegls_encoder.cpp:209-224 codes them in a plain
    // loop; they share nothing): one launch over frames x components into private buffers, then every frame's scans are put in
    // place behind their SOS headers (place_plane_scans).  Frames go in groups that keep the private buffers under 8 GiB.  A
    // frame with a scan that failed or that ends within 4 bytes of its destination is coded again below, scan by scan with
    // the reference's capacities -- its verdict depends on them there (src/scan_encoder.hpp:117-120).
    std::vector<uint8_t> redo_frames; // 1 = code this frame in rounds (all of them when the scans are not coded together)
    const bool equal_headers = [&] {
        for (auto& h : sos)
            if (h.size() != sos[0].size())
                return false;
        return true;
    }();
    // (Worth it while a round alone does not fill the chip: 256 4096 x 4096 RGB frames code at 17.9 GPix/s together and at
    // 18.8 in rounds of 256 scans -- the scans' second trip through memory --, four 2048 x 2048 frames three times faster.)
    constexpr uint32_t kTogetherFrames = 128;
    if (rounds > 1 && p.restart_interval == 0 && equal_headers && !t_force_rounds && frame_count <= kTogetherFrames &&
        knobs::get_or(knobs::kBatchRounds, 0) == 0)
    {
        const size_t worst = dev::worst_case_scan_bytes(f.width, f.height, 1, f.bits_per_sample);
        const size_t capacity = (std::min(stream_pitch_bytes, worst) + 255) & ~size_t{255};
        // The private buffers are a work area like the pipeline's: they come out of the configured workspace
        // (charls_amd_set_workspace_limit) -- half of what this thread may hold, the pipeline's arena wants the rest --, never
        // more than 8 GiB, and when they cannot be had the frames are coded in rounds, which need none.
        const size_t scratch_bytes = (scratch_samples * sizeof(uint16_t) + 255) & ~size_t{255}; // (the exact re-coding of a scan that ends within 3 bytes of its buffer)
        const size_t per_frame = (capacity + scratch_bytes) * rounds;
        const size_t budget = std::min<size_t>(size_t{8} << 30, dev::work_area_budget() / 2);
        uint32_t group = static_cast<uint32_t>(std::min<size_t>(frame_count, budget / per_frame));
        uint8_t* priv = nullptr;
        while (group >= 1 && (priv = static_cast<uint8_t*>(dev::try_ensure(dev::plane_arena(), per_frame * group))) == nullptr) // (kept between calls)
            group /= 2;
        if (priv != nullptr)
        {
        auto* plane_scratch = reinterpret_cast<uint16_t*>(priv + static_cast<size_t>(capacity) * rounds * group);
        dev::DeviceBuffer d_plane_descs, d_plane_results, d_redo;
        d_plane_descs.ensure(sizeof(ScanDesc) * rounds * group);
        d_plane_results.ensure(sizeof(ScanResult) * rounds * group);
        d_redo.ensure(sizeof(uint32_t) * frame_count);
        std::vector<ScanDesc> plane_descs(static_cast<size_t>(rounds) * group);
        const uint32_t sos_size = static_cast<uint32_t>(sos[0].size());
        for (uint32_t first = 0; first < frame_count; first += group)
        {
            const uint32_t n = std::min(group, frame_count - first);
            for (uint32_t i = 0; i < n; ++i)
                for (uint32_t r = 0; r < rounds; ++r)
                {
                    ScanDesc d = scan; // (one component, ILV_NONE, no restart intervals: this branch's condition above has
                                       // rounds > 1, which only planar frames have, and p.restart_interval == 0)
                    d.pixels = const_cast<uint8_t*>(frames[first + i]) + r * stride * f.height;
                    d.pixel_stride = stride;
                    d.stream = priv + (static_cast<size_t>(i) * rounds + r) * capacity;
                    d.stream_capacity = std::min(stream_pitch_bytes, worst);
                    d.line_scratch = plane_scratch + (static_cast<size_t>(i) * rounds + r) * (scratch_bytes / sizeof(uint16_t));
                    plane_descs[static_cast<size_t>(i) * rounds + r] = d;
                }
            hip_check(hipMemcpyAsync(d_plane_descs.as<ScanDesc>(), plane_descs.data(), sizeof(ScanDesc) * rounds * n, hipMemcpyHostToDevice, stream));
            hip_check(hipStreamSynchronize(stream)); // plane_descs is reused by the next group
            scans.start();
            {
                ScanDesc proto = plane_descs[0];
                dev::launch_encode(proto, d_plane_descs.as<ScanDesc>(), d_plane_results.as<ScanResult>(), rounds * n, stream);
            }
            scans.stop();
            scan_ms += scans.ms();
            dev::launch_place_plane_scans(slots + first * stream_pitch_bytes, stream_pitch_bytes, d_blob.as<uint8_t>() + prologue_size, sos_size,
                                          rounds, priv, capacity, d_plane_results.as<ScanResult>(),
                                          d_cursors.as<dev::FrameCursorPod>() + first, d_redo.as<uint32_t>() + first, n, stream);
        }
        std::vector<uint32_t> redo(frame_count);
        hip_check(hipMemcpyAsync(redo.data(), d_redo.as<uint32_t>(), sizeof(uint32_t) * frame_count, hipMemcpyDeviceToHost, stream));
        hip_check(hipStreamSynchronize(stream));
        redo_frames.assign(frame_count, 0);
        for (uint32_t i = 0; i < frame_count; ++i)
            redo_frames[i] = redo[i] != 0;
        } // (priv)
    }
    const bool in_rounds = redo_frames.empty();
    for (uint32_t r = 0; r < rounds && in_rounds; ++r)
    {
        for (uint32_t i = 0; i < frame_count; ++i)
        {
            ScanDesc d = scan;
            d.pixels = const_cast<uint8_t*>(frames[i]) + (p.interleave_mode == 0 ? r * stride * f.height : 0);
            d.pixel_stride = stride;
            d.line_scratch = d_scratch.as<uint16_t>() + i * scratch_samples;
            descs[i] = d;
        }
        hip_check(hipMemcpyAsync(d_descs.as<ScanDesc>(), descs.data(), sizeof(ScanDesc) * frame_count,
                                 hipMemcpyHostToDevice, stream));
        hip_check(hipStreamSynchronize(stream)); // descs is reused by the next round
        const uint32_t sos_size = static_cast<uint32_t>(sos[r].size());
        dev::launch_place_scan_header(slots, stream_pitch_bytes, d_blob.as<uint8_t>() + blob_offset, sos_size,
                                      d_cursors.as<dev::FrameCursorPod>(), d_descs.as<ScanDesc>(), frame_count, stream);
        scans.start();
        {
            ScanDesc proto = descs[0];
            proto.stream_capacity = stream_pitch_bytes; // upper bound of every frame's remaining capacity
            dev::launch_encode(proto, d_descs.as<ScanDesc>(), d_results.as<ScanResult>(), frame_count, stream);
        }
        scans.stop();
        dev::launch_advance_cursor(d_cursors.as<dev::FrameCursorPod>(), d_results.as<ScanResult>(), sos_size, frame_count,
                                   stream);
        scan_ms += scans.ms();
        blob_offset += sos_size;
    }
    dev::launch_place_epilogue(slots, stream_pitch_bytes, d_cursors.as<dev::FrameCursorPod>(),
                               (p.encoding_options & 1u) != 0, d_sizes.as<uint64_t>(), d_errcs.as<uint32_t>(),
                               frame_count, stream);
    total.stop();
    hip_check(hipMemcpyAsync(sizes, d_sizes.as<uint64_t>(), sizeof(uint64_t) * frame_count, hipMemcpyDeviceToHost, stream));
    static_assert(sizeof(charls_jpegls_errc) == sizeof(uint32_t), "errc size");
    hip_check(hipMemcpyAsync(errcs, d_errcs.as<uint32_t>(), sizeof(uint32_t) * frame_count, hipMemcpyDeviceToHost, stream));
    hip_check(hipStreamSynchronize(stream));
    dev::Timings& t = dev::last_timings();
    t.values[0] = total.ms();
    t.values[1] = scan_ms;
    if (t.count < 2)
        t.count = 2; // the pipeline adds its stage breakdown in values[2..6]
    // frames whose scans could not simply be put in place: scan by scan, with the capacities the reference passes -- every RUN
    // of such frames by one call in rounds (a batch with slots too small for anything flags every frame: one call, not
    // frame_count calls of one frame each); the timings reported are those of this call, not of the re-coding.
    const dev::Timings kept = dev::last_timings();
    for (uint32_t i = 0; i < redo_frames.size();)
    {
        if (!redo_frames[i])
        {
            ++i;
            continue;
        }
        uint32_t last = i + 1;
        while (last < redo_frames.size() && redo_frames[last])
            ++last;
        struct ForceRounds
        {
            ForceRounds() { t_force_rounds = true; }
            ~ForceRounds() { t_force_rounds = false; }
        } force;
        encode_batch_frames(p, last - i, frames + i, frame_pitch_bytes, stride_arg, slots + i * stream_pitch_bytes, stream_pitch_bytes,
                            sizes + i, errcs + i, hip_stream);
        i = last;
    }
    if (!redo_frames.empty())
        dev::last_timings() = kept;
}

extern "C" charls_jpegls_errc charls_amd_encode_batch_device(const charls_amd_codec_params* params, uint32_t frame_count,
                                                             const void* d_frames, size_t frame_pitch_bytes,
                                                             uint32_t stride_arg, void* d_streams,
                                                             size_t stream_pitch_bytes, uint64_t* sizes,
                                                             charls_jpegls_errc* errcs, void* hip_stream)
try
{
    check_pointer(params);
    check_pointer(sizes);
    check_pointer(errcs);
    if (frame_count == 0)
        return CHARLS_JPEGLS_ERRC_SUCCESS;
    check_pointer(d_frames);
    check_pointer(d_streams);
    dev::require_device();
    std::vector<const uint8_t*> frames(frame_count);
    for (uint32_t i = 0; i < frame_count; ++i)
        frames[i] = static_cast<const uint8_t*>(d_frames) + i * frame_pitch_bytes;
    encode_batch_frames(*params, frame_count, frames.data(), frame_pitch_bytes, stride_arg, d_streams, stream_pitch_bytes, sizes, errcs,
                        hip_stream);
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}

// The frames of the slot calls as a table of destinations: what the decoder below takes.
void jls::decode_batch_streams(uint32_t frame_count, const void* d_streams, const uint64_t* stream_at, const uint64_t* sizes,
                               void* d_frames, size_t frame_pitch_bytes, uint32_t stride_arg,
                               charls_amd_codec_params* params_out, charls_jpegls_errc* errcs, void* hip_stream)
{
    std::vector<charls_amd_frame_dest> dests(frame_count);
    for (uint32_t i = 0; i < frame_count; ++i)
        dests[i] = charls_amd_frame_dest{static_cast<uint8_t*>(d_frames) + i * frame_pitch_bytes, frame_pitch_bytes, stride_arg, 0};
    decode_batch_streams(frame_count, d_streams, stream_at, sizes, BatchDests{dests.data(), false, nullptr}, params_out, errcs, hip_stream);
}

namespace {

// The probe: part 1's get_destination_size(stride 0) (decoder_api.cpp: destination_size) beside the parameters; an
// abbreviated table stream has no frame: read_header succeeds on it, and it reports zeros.
void probe_frames(StreamWindows& win, const BatchDests& to, charls_amd_codec_params* params_out, charls_jpegls_errc* errcs)
{
    for (uint32_t i = 0; i < win.fr.size(); ++i)
    {
        BatchFrame& x = win.fr[i];
        params_out[i] = charls_amd_codec_params{};
        to.frame_bytes_out[i] = 0;
        if (x.errc == CHARLS_JPEGLS_ERRC_SUCCESS && !x.reader.end_of_image())
            try
            {
                const charls_frame_info& f = x.reader.frame_info();
                to.frame_bytes_out[i] = checked_mul(checked_mul(checked_mul(static_cast<size_t>(f.component_count), f.height), f.width),
                                                    bytes_per_sample(f.bits_per_sample));
                params_out[i] = params_of(x.reader);
            }
            catch (const error& e)
            {
                x.errc = e.code;
            }
        errcs[i] = x.errc;
    }
    dev::Timings& t = dev::last_timings(); // (no kernel of the decoder ran)
    t.values[0] = t.values[1] = 0;
    t.count = 2;
}

} // namespace

// A destination per frame of the caller's own: stride and capacity against the whole frame -- the rows of all planes of a
// planar frame --, before any of its scans is decoded.  (stream_windows.h: the indexed calls of batch_index.cpp make the same check.)
void jls::check_ragged_dests(StreamWindows& win, const BatchDests& to)
{
    for (uint32_t i = 0; i < win.fr.size(); ++i)
    {
        BatchFrame& x = win.fr[i];
        if (x.done)
            continue;
        const auto [row, stride] = row_and_stride(x.reader, to.dests[i].stride);
        const size_t rows = static_cast<size_t>(x.reader.frame_info().height) * scans_of_frame(x.reader);
        if (stride < row)
            x.errc = CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_STRIDE;
        else if (to.dests[i].capacity_bytes < stride * rows - (stride - row))
            x.errc = CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_SIZE;
        x.done = x.errc != CHARLS_JPEGLS_ERRC_SUCCESS;
    }
}

namespace {

// A decode past the headers: the streams, the launches, where the frames go and what the caller learns of their parameters.
struct BatchDecode
{
    StreamWindows& win;
    DecodeLauncher& launcher;
    const BatchDests& to;
    charls_amd_codec_params* params_out;
    uint32_t params_from; // the frame params_out describes so far: the lowest-index frame that got as far as a scan
};

// What a frame's scan needs besides its stream position: geometry and coding parameters from the reader (which stands
// behind the scan's header), the destination of its first plane.  The launcher places the line scratch.
ScanDesc scan_desc_for(const BatchDecode& b, uint32_t i, const BatchFrame& x)
{
    const charls_frame_info& f = x.reader.frame_info();
    const auto [row, stride] = row_and_stride(x.reader, b.to.dests[i].stride);
    if (stride < row)
        raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_STRIDE);
    const uint32_t nc = x.reader.scan_component_count();
    const size_t need = (x.reader.scan_interleave_mode() == 0 ? stride * nc * f.height : stride * f.height) - (stride - row);
    if (b.to.dests[i].capacity_bytes < x.plane_offset + need)
        raise(CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_SIZE);
    ScanDesc d = desc_of(scan_spec_of(x.reader));
    d.pixels = static_cast<uint8_t*>(b.to.dests[i].d_pixels) + x.plane_offset;
    d.pixel_stride = stride;
    d.stream = b.win.stream_ptr(i, x.cursor);
    d.stream_capacity = b.win.sizes[i] - x.cursor;
    return d;
}

void report_params(BatchDecode& b, const BatchFrame& x, uint32_t index)
{
    if (b.params_out && b.to.ragged)
        b.params_out[index] = params_of(x.reader);
    else if (b.params_out && index < b.params_from)
    {
        *b.params_out = params_of(x.reader);
        b.params_from = index;
    }
}

// A planar frame whose component scans go in the one launch of decode_planar_in_one_launch.
struct Plan
{
    uint32_t frame;
    std::vector<ScanDesc> scans;
    std::vector<size_t> starts;    // first byte of scan c
    std::vector<size_t> marker_at; // the marker found behind scan c
    std::vector<size_t> used;      // bytes scan c consumed
    size_t first_desc{};           // its scans in the launch
    bool ok{true};
};

// ---- Planar frames: the component scans of all of them in ONE launch (the decoder's rate is the number of scans in
// flight: scan by scan, a batch of RGB planes ran three rounds of a third of its scans).  Where scan c + 1 starts is only
// known once scan c has been decoded -- or once the marker that ends scan c has been found: inside an entropy-coded
// segment no 0xFF is followed by a byte with its high bit set, so a search finds it (find_scan_end), and the part-1 reader
// parses on from there, on a COPY of the frame's state.  The copy replaces the frame only if every scan then ends exactly
// at the marker found behind it and the end of the image parses; any frame that does not is decoded again by the rounds
// below, which report whatever part 1 reports for it.  src/charls_jpegls_decoder.cpp:211-236 is the scan-by-scan loop.
void decode_planar_in_one_launch(BatchDecode& b)
{
    StreamWindows& win = b.win;
    std::vector<BatchFrame>& fr = win.fr;
    const hipStream_t stream = win.stream;
    std::vector<BatchFrame> probe;
    std::vector<Plan> plans;
    for (uint32_t i = 0; i < fr.size(); ++i)
    {
        const BatchFrame& x = fr[i];
        if (x.done || x.reader.component_count() < 2 || x.reader.scan_interleave_mode() != 0 || x.reader.scan_component_count() != 1)
            continue;
        if (probe.empty())
            probe = fr; // (readers, windows and cursors of every frame; only the planned ones are touched)
        Plan p;
        p.frame = i;
        try
        { // every plane must fit behind the first (the rounds raise the error where it belongs otherwise)
            const auto [row, stride] = row_and_stride(x.reader, b.to.dests[i].stride);
            if (stride < row || b.to.dests[i].capacity_bytes <
                                    checked_mul(checked_mul(stride, x.reader.frame_info().height), x.reader.component_count()) - (stride - row))
                continue;
            p.scans.push_back(scan_desc_for(b, i, probe[i]));
        }
        catch (const error&)
        {
            continue;
        }
        p.starts.push_back(x.cursor);
        plans.push_back(std::move(p));
    }
    dev::DeviceBuffer d_search, d_found;
    dev::PinnedBuffer h_search, h_found;
    for (uint32_t c = 1; !plans.empty(); ++c)
    {
        std::vector<uint32_t> need; // plans whose frame has a scan c
        for (uint32_t k = 0; k < plans.size(); ++k)
            if (plans[k].ok && probe[plans[k].frame].reader.component_count() > c)
                need.push_back(k);
        if (need.empty())
            break;
        const size_t n = need.size();
        auto* search = static_cast<MarkerSearch*>(h_search.ensure(sizeof(MarkerSearch) * n));
        auto* found = static_cast<unsigned long long*>(h_found.ensure(sizeof(unsigned long long) * n));
        for (size_t q = 0; q < n; ++q)
        {
            const uint32_t i = plans[need[q]].frame;
            search[q] = MarkerSearch{win.offset_of(i) + plans[need[q]].starts.back(), win.offset_of(i) + win.sizes[i]};
        }
        d_search.ensure(sizeof(MarkerSearch) * n);
        d_found.ensure(sizeof(unsigned long long) * n);
        hip_check(hipMemcpyAsync(d_search.as<MarkerSearch>(), search, sizeof(MarkerSearch) * n, hipMemcpyHostToDevice, stream));
        dev::launch_find_scan_end(win.slots, d_search.as<const MarkerSearch>(), d_found.as<unsigned long long>(), static_cast<uint32_t>(n), stream);
        hip_check(hipMemcpyAsync(found, d_found.as<unsigned long long>(), sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, stream));
        hip_check(hipStreamSynchronize(stream));
        std::vector<uint32_t> which;
        std::vector<size_t> bases;
        for (size_t q = 0; q < n; ++q)
        {
            Plan& p = plans[need[q]];
            if (found[q] == kNoMarker)
            {
                p.ok = false;
                continue;
            }
            p.marker_at.push_back(static_cast<size_t>(found[q] - win.offset_of(p.frame)));
            which.push_back(p.frame);
            bases.push_back(p.marker_at.back());
        }
        win.parse_behind_scans(probe, which, bases, std::vector<uint8_t>(which.size(), 0));
        for (size_t q = 0; q < n; ++q)
        {
            Plan& p = plans[need[q]];
            if (!p.ok)
                continue;
            BatchFrame& y = probe[p.frame];
            y.plane_offset += p.scans.back().pixel_stride * p.scans.back().height; // (past the plane of the scan before)
            if (y.done || y.reader.scan_interleave_mode() != 0 || y.reader.scan_component_count() != 1)
            {
                p.ok = false;
                continue;
            }
            try
            {
                p.scans.push_back(scan_desc_for(b, p.frame, y));
                p.starts.push_back(y.cursor);
            }
            catch (const error&)
            {
                p.ok = false;
            }
        }
    }
    std::vector<ScanDesc> descs;
    for (Plan& p : plans)
    {
        p.ok = p.ok && p.scans.size() == probe[p.frame].reader.component_count();
        if (!p.ok)
            continue;
        p.first_desc = descs.size();
        descs.insert(descs.end(), p.scans.begin(), p.scans.end());
    }
    if (descs.empty())
        return;
    std::vector<ScanResult> results;
    b.launcher.run(descs, results);
    std::vector<uint32_t> which;
    std::vector<size_t> bases;
    for (Plan& p : plans)
    {
        if (!p.ok)
            continue;
        for (uint32_t c = 0; c < p.scans.size(); ++c)
        {
            const ScanResult& r = results[p.first_desc + c];
            p.ok = p.ok && r.errc == kOk;
            p.used.push_back(static_cast<size_t>(r.bytes));
        }
        for (uint32_t c = 0; p.ok && c + 1 < p.scans.size(); ++c)
            p.ok = p.starts[c] + p.used[c] == p.marker_at[c]; // the scan ends exactly at the marker found behind it
        if (!p.ok)
            continue;
        probe[p.frame].cursor = p.starts.back() + p.used.back();
        which.push_back(p.frame);
        bases.push_back(probe[p.frame].cursor);
    }
    win.parse_behind_scans(probe, which, bases, std::vector<uint8_t>(which.size(), 1));
    for (Plan& p : plans)
    {
        if (!p.ok)
            continue;
        BatchFrame& y = probe[p.frame];
        if (y.errc != CHARLS_JPEGLS_ERRC_SUCCESS)
            continue; // (the rounds decode it again and report this)
        report_params(b, fr[p.frame], p.frame);
        y.decoded_components = static_cast<uint32_t>(p.scans.size());
        y.done = true;
        fr[p.frame] = std::move(y);
    }
}

// Scan by scan: one round decodes the next scan of every frame that has one, then parses what follows it.
void decode_by_rounds(BatchDecode& b)
{
    std::vector<BatchFrame>& fr = b.win.fr;
    std::vector<ScanDesc> descs;
    std::vector<ScanResult> results;
    std::vector<uint32_t> active;
    for (;;)
    {
        active.clear();
        descs.clear();
        for (uint32_t i = 0; i < fr.size(); ++i)
        {
            BatchFrame& x = fr[i];
            if (x.done)
                continue;
            try
            {
                const ScanDesc d = scan_desc_for(b, i, x);
                report_params(b, x, i);
                descs.push_back(d);
                active.push_back(i);
            }
            catch (const error& e)
            {
                x.errc = e.code;
                x.done = true;
            }
        }
        if (active.empty())
            break;
        b.launcher.run(descs, results);

        // advance every frame past its scan; parse the bytes that follow (next SOS or EOI)
        std::vector<uint32_t> which;
        std::vector<size_t> bases;
        std::vector<uint8_t> last;
        for (uint32_t k = 0; k < active.size(); ++k)
        {
            BatchFrame& x = fr[active[k]];
            if (results[k].errc != kOk)
            {
                x.errc = static_cast<charls_jpegls_errc>(results[k].errc);
                x.done = true;
                continue;
            }
            x.cursor += results[k].bytes;
            x.decoded_components += x.reader.scan_component_count();
            const bool end = x.decoded_components == x.reader.component_count();
            if (!end)
                x.plane_offset += descs[k].pixel_stride * descs[k].height;
            which.push_back(active[k]);
            bases.push_back(x.cursor);
            last.push_back(end ? 1 : 0);
        }
        b.win.parse_behind_scans(fr, which, bases, last);
        for (size_t k = 0; k < which.size(); ++k)
            if (last[k])
                fr[which[k]].done = true;
    }
}

} // namespace

// The batch decoder behind charls_amd_decode_batch_device (slots: stream_at[i] = i * pitch),
// charls_amd_decode_batch_device_packed (batch_packed.cpp: stream_at = the caller's offset table) and the calls of part 2e
// (batch_ragged.cpp: a destination per frame, or none -- the probe): frame i's stream is the sizes[i] bytes at
// d_streams + stream_at[i] and goes to to.dests[i].  frame_count >= 1, the pointers are checked by the entry points.
void jls::decode_batch_streams(uint32_t frame_count, const void* d_streams, const uint64_t* stream_at, const uint64_t* sizes,
                               const BatchDests& to, charls_amd_codec_params* params_out, charls_jpegls_errc* errcs,
                               void* hip_stream)
{
    dev::require_device();
    auto stream = static_cast<hipStream_t>(hip_stream);
    const bool probing = to.dests == nullptr;
    StreamWindows win(frame_count, d_streams, stream_at, sizes, stream);
    win.read_headers(!probing);
    if (probing)
        return probe_frames(win, to, params_out, errcs);
    if (to.ragged)
        check_ragged_dests(win, to);
    DecodeLauncher launcher(stream);
    BatchDecode b{win, launcher, to, params_out, UINT32_MAX};
    if (knobs::get_or(knobs::kBatchRounds, 0) == 0)
        decode_planar_in_one_launch(b);
    decode_by_rounds(b);
    for (uint32_t i = 0; i < frame_count; ++i)
        errcs[i] = win.fr[i].errc;
    if (to.names_table_out != nullptr)
        for (uint32_t i = 0; i < frame_count; ++i)
        { // (the reader keeps, per component, the table id of the scan header that named it)
            const StreamReader& reader = win.fr[i].reader;
            to.names_table_out[i] = 0;
            for (size_t c = 0; c < reader.component_count(); ++c)
                if (reader.mapping_table_id(c) != 0)
                    to.names_table_out[i] = 1;
        }
    dev::Timings& t = dev::last_timings();
    t.values[0] = launcher.gpu_ms();
    t.values[1] = launcher.gpu_ms();
    t.count = 2;
}

extern "C" charls_jpegls_errc charls_amd_decode_batch_device(uint32_t frame_count, const void* d_streams,
                                                             size_t stream_pitch_bytes, const uint64_t* sizes,
                                                             void* d_frames, size_t frame_pitch_bytes,
                                                             uint32_t stride_arg, charls_amd_codec_params* params_out,
                                                             charls_jpegls_errc* errcs, void* hip_stream)
try
{
    check_pointer(sizes);
    check_pointer(errcs);
    if (frame_count == 0)
        return CHARLS_JPEGLS_ERRC_SUCCESS;
    check_pointer(d_streams);
    check_pointer(d_frames);
    dev::require_device();
    const std::vector<uint64_t> stream_at = slot_offsets(frame_count, stream_pitch_bytes, sizes);
    decode_batch_streams(frame_count, d_streams, stream_at.data(), sizes, d_frames, frame_pitch_bytes, stride_arg, params_out, errcs,
                         hip_stream);
    return CHARLS_JPEGLS_ERRC_SUCCESS;
}
catch (...)
{
    return current_exception_to_errc();
}
