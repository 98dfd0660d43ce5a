// batch_streams.h -- what the batch entry points share across translation units (batch_api.cpp, batch_packed.cpp,
// batch_ragged.cpp, batch_budget.cpp).  The decoders' host plumbing -- window parser, ordinary launch -- is stream_windows.h
// (batch_api.cpp, batch_index.cpp), the event-pair timer event_timer.h.
#pragma once
#include <cstdint>
#include <functional>

#include "../device/scan_types.h"
#include "common.h"

namespace jls {

// Where the frames of a decoder call go.  `dests[i]` is frame i's destination: its first row, the bytes the call may write
// from there on, its stride (0 = minimal).  The slot and packed entry points state frames + i * frame_pitch_bytes, the pitch
// and their one stride; charls_amd_decode_batch_device_ragged hands over the caller's table and sets `ragged`:
//  * params_out is then an array, element i describing frame i (it is ONE element otherwise: the lowest-index frame that
//    got as far as a scan), and
//  * stride and capacity are checked against the WHOLE frame (all planes of a planar frame) once its header is parsed, so
//    that nothing of a frame that fails either check is written; the slot calls check scan by scan, as part 1 does.
// `dests == nullptr` is the probe (charls_amd_probe_batch_device_packed): every frame's header is fetched and parsed exactly
// as a decode does it, params_out (an array) and frame_bytes_out are filled, and nothing is launched.
struct BatchDests
{
    const charls_amd_frame_dest* dests;
    bool ragged;
    uint64_t* frame_bytes_out; // the probe only
    // decode only, may be nullptr (HOST, one per frame): 1 where a scan header the decode read names a mapping table (a table
    // id that is not 0 for any component), else 0 -- charls_amd_transcode_batch_device refuses such frames
    uint8_t* names_table_out = nullptr;
};

// The batch decoder with every frame's stream named by an offset of its own: frame i's .jls is the sizes[i] bytes at
// d_streams + stream_at[i] (HOST array; any order, any alignment, streams may abut or coincide: they are only read).
// Raises; errcs[i] and params_out as charls_amd_decode_batch_device.  frame_count >= 1, pointers checked by the caller.
void decode_batch_streams(uint32_t frame_count, const void* d_streams, const uint64_t* stream_at, const uint64_t* sizes,
                          const BatchDests& to, charls_amd_codec_params* params_out, charls_jpegls_errc* errcs, void* hip_stream);
// The same with the frames of the slot calls: frame i at d_frames + i * frame_pitch_bytes, one stride.
void decode_batch_streams(uint32_t frame_count, const void* d_streams, const uint64_t* stream_at, const uint64_t* sizes,
                          void* d_frames, size_t frame_pitch_bytes, uint32_t stride_arg, charls_amd_codec_params* params_out,
                          charls_jpegls_errc* errcs, void* hip_stream);

// charls_amd_decode_batch_device_salvage (batch_salvage.cpp; the part-1 call of the same name hands over ONE frame): the
// ragged decode above, then the salvage round for the frames it failed on.  frame_count >= 1, pointers checked by the caller.
void decode_batch_salvage(uint32_t frame_count, const void* d_packed, const uint64_t* offsets, const uint64_t* sizes,
                          const charls_amd_frame_dest* dests, uint32_t fill_value, charls_amd_codec_params* params_out,
                          charls_amd_salvage_report* reports, uint8_t* interval_status, size_t status_pitch_bytes,
                          charls_jpegls_errc* errcs, void* hip_stream);

// charls_amd_decode_batch_device_salvage_indexed (batch_salvage_index.cpp): decode_batch_salvage, then the index and prefix
// modes of part 2h for the frames it leaves in state 2.  Frame f's index is *parsed_indexes[f] where that array and the
// entry are there (the part-1 call hands over the handle's), else the index_sizes[f] bytes at indexes + f * index_pitch_bytes
// (HOST; index_sizes may be nullptr: no indexes).  frame_count >= 1, flags and pointers checked by the caller.
struct SeekIndex;
void decode_batch_salvage_indexed(uint32_t frame_count, const void* d_packed, const uint64_t* offsets, const uint64_t* sizes,
                                  const SeekIndex* const* parsed_indexes, const void* indexes, size_t index_pitch_bytes,
                                  const uint64_t* index_sizes, const charls_amd_frame_dest* dests, uint32_t fill_value, uint32_t flags,
                                  charls_amd_codec_params* params_out, charls_amd_salvage_report* reports, uint8_t* interval_status,
                                  size_t status_pitch_bytes, charls_jpegls_errc* errcs, void* hip_stream);

// The index-only build of charls_amd_index_batch_device_packed (batch_index.cpp; charls_amd.h part 2l) behind its whole-call
// checks, which the host form (batch_host.cpp) runs on every device window: frame f's index to indexes + f * index_pitch_bytes
// (HOST), its size to index_sizes[f], no pixels anywhere but in a work area of the calling thread.  params_out (an array) may
// be nullptr.  frame_count >= 1, a device is there.  Raises.
void index_packed_frames(uint32_t frame_count, const void* d_packed, const uint64_t* offsets, const uint64_t* sizes,
                         uint32_t lines_per_seek_point, void* indexes, size_t index_pitch_bytes, uint64_t* index_sizes,
                         charls_amd_codec_params* params_out, charls_jpegls_errc* errcs, void* hip_stream);

// The batch encoder behind charls_amd_encode_batch_device with every frame's pixels named by a pointer of its own
// (d_pixels: HOST array of frame_count DEVICE pointers; the slot call passes d_frames + i * frame_pitch_bytes): frame i's
// .jls goes to d_streams + i * stream_pitch_bytes.  `frame_bytes` is what every frame offers from its pointer on (the slot
// call's frame_pitch_bytes).  Raises -- for parameters the encoder refuses: what check_encode_params raises --; sizes and
// errcs as charls_amd_encode_batch_device.  frame_count >= 1, pointers checked by the caller.
void encode_batch_frames(const charls_amd_codec_params& params, uint32_t frame_count, const uint8_t* const* d_pixels,
                         size_t frame_bytes, uint32_t stride_arg, void* d_streams, size_t stream_pitch_bytes, uint64_t* sizes,
                         charls_jpegls_errc* errcs, void* hip_stream);
// The body of charls_amd_encode_batch_device_ragged (batch_ragged.cpp) behind its whole-call checks: frame_count >= 1, the
// tables, every sources[f].d_pixels and d_packed are there, the alignment is valid, a device is.  Returns the first frame, in
// the caller's order, whose end lay beyond packed_capacity_bytes -- that frame and every frame behind it have
// destination_too_small --, or frame_count.
uint32_t encode_ragged_frames(uint32_t frame_count, const charls_amd_frame_source* sources, void* d_packed, size_t packed_capacity_bytes,
                              uint32_t offset_alignment, uint64_t* offsets, uint64_t* sizes, charls_jpegls_errc* errcs, void* hip_stream);
// The body of charls_amd_encode_batch_device_ragged_budget (batch_budget.cpp; charls_amd.h part 2k) behind its whole-call checks,
// factored as encode_ragged_frames is: the frames are sized group by group, every frame's first candidate within budgets[f] is
// picked, and the picked (frame, NEAR) pairs go through ONE encode_ragged_frames.  sources[f].params.near_lossless and
// .max_stream_bytes are not looked at.  Returns the first frame beyond the capacity, or frame_count.  The caller's tables are
// written only when nothing was raised.
uint32_t encode_ragged_budget_frames(uint32_t frame_count, const charls_amd_frame_source* sources, const uint64_t* budgets,
                                     const int32_t* near_candidates, uint32_t candidate_count, void* d_packed, size_t packed_capacity_bytes,
                                     uint32_t offset_alignment, uint64_t* offsets, uint64_t* sizes, int32_t* near_out,
                                     charls_jpegls_errc* errcs, void* hip_stream);
// The whole-call checks on what the budget calls of part 2k take beyond the calls they extend; needs no device.
void check_budget_tables(const uint64_t* budgets, const int32_t* near_candidates, uint32_t candidate_count, const int32_t* near_out);
// Raises what the batch encoder raises for these parameters before it codes anything (needs no GPU).
void check_encode_params(const charls_amd_codec_params& params, size_t frame_bytes, uint32_t stride_arg);

// What encode_batch_frames derives from `params` before it codes anything.  Raises what check_encode_params raises.
struct EncodePlan
{
    size_t stride;            // bytes between rows
    uint32_t scans;           // scans per frame: the components of a planar frame, else 1
    ScanDesc scan;            // a scan of the frame without its pointers; scan r's pixels start r * stride * height into the frame
    uint64_t container_bytes; // everything in front of the EOI marker that is no entropy-coded segment: prologue, SOS headers
};
EncodePlan plan_encode(const charls_amd_codec_params& params, size_t frame_bytes, uint32_t stride_arg);

// charls_jpegls_encoder_get_estimated_destination_size for the frames of `p` (batch_packed.cpp).
size_t estimated_stream_bytes(const charls_amd_codec_params& p);
// An upper bound on the complete .jls the batch encoder can write for the frames of `p` at any NEAR, whatever they hold
// (batch_packed.cpp): no sample takes more than LIMIT bits of ISO 14495-1, in either mode, and stuffing adds at most a bit per
// seven.  What estimated_stream_bytes returns is not such a bound: noise coded losslessly is a little longer.
size_t longest_stream_bytes(const charls_amd_codec_params& p);

// charls_amd_transcode_batch_device (batch_transcode.cpp; charls_amd.h part 2j) in three pieces, which the host form
// (batch_host.cpp) uses too: `p` with the fields that spec.set names replaced; the whole-call checks, which raise before a
// device is asked for (the blobs are DEVICE pointers in one form and HOST pointers in the other: only looked at for NULL);
// and the body behind them -- frame_count >= 1, a device is there --, which returns the first frame, in the caller's order,
// whose end lay beyond packed_capacity_bytes, or frame_count.
//
// The ENCODE STEP of a window is a parameter of the body: it codes the `count` frames `sources` that decoded -- frames
// sent[0 .. count) of the call, in its order, with the spec applied and max_stream_bytes 0 -- to d_packed under the contract of
// encode_ragged_frames, whose arguments and return value the rest are, and leaves in sources[k].params what frame k was coded
// with.  transcode_encode_plain is encode_ragged_frames itself (part 2j); transcode_encode_budget (batch_budget.cpp, part 2k)
// is encode_ragged_budget_frames with budgets[sent[k]], and sets near_out[sent[k]] (-1 for a frame that was not coded).
using TranscodeEncode = std::function<uint32_t(uint32_t count, charls_amd_frame_source* sources, const uint32_t* sent, void* d_packed,
                                               size_t packed_capacity_bytes, uint32_t offset_alignment, uint64_t* offsets, uint64_t* sizes,
                                               charls_jpegls_errc* errcs, void* hip_stream)>;
TranscodeEncode transcode_encode_plain();
TranscodeEncode transcode_encode_budget(const uint64_t* budgets, const int32_t* near_candidates, uint32_t candidate_count, int32_t* near_out);
charls_amd_codec_params transcode_params(charls_amd_codec_params p, const charls_amd_transcode_spec& spec) noexcept;
void check_transcode_call(uint32_t frame_count, const void* packed_in, const uint64_t* offsets_in, const uint64_t* sizes_in,
                          const charls_amd_transcode_spec* specs, uint32_t spec_count, const void* packed_out, uint32_t offset_alignment,
                          const uint64_t* offsets_out, const uint64_t* sizes_out, const charls_amd_codec_params* params_out,
                          const charls_jpegls_errc* errcs);
uint32_t transcode_frames(uint32_t frame_count, const void* d_packed_in, const uint64_t* offsets_in, const uint64_t* sizes_in,
                          const charls_amd_transcode_spec* specs, uint32_t spec_count, void* d_packed_out, size_t packed_capacity_bytes,
                          uint32_t offset_alignment, uint64_t* offsets_out, uint64_t* sizes_out, charls_amd_codec_params* params_out,
                          charls_jpegls_errc* errcs, const TranscodeEncode& encode, void* hip_stream);
// Part 2k, both forms: check_transcode_call plus the budget tables, the candidate count and a spec that sets NEAR (the
// candidates decide it); and, behind the body, near_out[f] = -1 for every frame that was not coded (errcs[f] is not success).
void check_transcode_budget_call(uint32_t frame_count, const void* packed_in, const uint64_t* offsets_in, const uint64_t* sizes_in,
                                 const charls_amd_transcode_spec* specs, uint32_t spec_count, const uint64_t* budgets,
                                 const int32_t* near_candidates, uint32_t candidate_count, const void* packed_out, uint32_t offset_alignment,
                                 const uint64_t* offsets_out, const uint64_t* sizes_out, const int32_t* near_out,
                                 const charls_amd_codec_params* params_out, const charls_jpegls_errc* errcs);
void transcode_near_of_uncoded(uint32_t frame_count, const charls_jpegls_errc* errcs, int32_t* near_out) noexcept;
void transcode_count_behind_capacity(uint64_t frames) noexcept; // charls_amd_transcode_counters [3], for windows the host form does not send

// What the lanes of the host-memory calls (batch_host.cpp; charls_amd.h part 2i) hold, device and pinned, given back: the
// lanes' part of charls_amd_release_work_areas.  A call that runs on them finishes first; the lane threads stay.
void release_host_lanes() noexcept;

// offset_alignment of the packed calls: a power of two in [1, 4096].
inline void check_offset_alignment(uint32_t alignment)
{
    check_argument(alignment >= 1 && alignment <= 4096 && (alignment & (alignment - 1)) == 0);
}

inline uint64_t round_up_to(uint64_t v, uint32_t alignment)
{
    return (v + (alignment - 1)) & ~static_cast<uint64_t>(alignment - 1);
}

} // namespace jls
