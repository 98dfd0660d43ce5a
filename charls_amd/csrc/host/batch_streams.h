// batch_streams.h -- what the batch entry points share across translation units (batch_api.cpp, batch_packed.cpp).
#pragma once
#include <cstdint>

#include "common.h"

namespace jls {

// The batch decoder with every frame's stream named by an offset of its own: frame i's .jls is the sizes[i] bytes at
// d_streams + stream_at[i] (HOST array; any order, any alignment, streams may abut or coincide: they are only read).
// Raises; errcs[i] and params_out as charls_amd_decode_batch_device.  frame_count >= 1, pointers checked by the caller.
void decode_batch_streams(uint32_t frame_count, const void* d_streams, const uint64_t* stream_at, const uint64_t* sizes,
                          void* d_frames, size_t frame_pitch_bytes, uint32_t stride_arg, charls_amd_codec_params* params_out,
                          charls_jpegls_errc* errcs, void* hip_stream);

} // namespace jls
