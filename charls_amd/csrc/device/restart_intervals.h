// restart_intervals.h -- restart intervals as the unit of parallelism INSIDE one scan: what the two halves share
// (restart_intervals_decode.hip in decode_launch.hip, restart_intervals_encode.hip in encode_launch.hip; restart_intervals.hip is both).
//
// At a restart marker the reference's decoder resets everything a scan starts with: contexts, RUNindex, the previous
// line (zeros) and the bit reader (src/scan_decoder_impl.hpp:119-127, src/scan_decoder.hpp:237-243,335-349).  The lines
// of one restart interval are therefore coded exactly like an independent scan of that many lines, and the intervals of
// a scan can be coded by different wavefronts at the same time.
//
//   decode:  find_restart_markers  one wavefront per scan walks the entropy-coded bytes once (0xFF followed by a byte
//                                  >= 0x80 can only be a marker: that is what bit stuffing guarantees) and lists the
//                                  RSTm positions up to the first other marker
//            build_decode_intervals one ScanDesc per interval (rows, stream window up to and including its RSTm)
//            ... the ordinary decoders run on the intervals ...
//            check_intervals        every interval must have ended exactly at its marker and the markers must count
//                                   0..7 cyclically; anything else is left to the sequential exact decoder, which
//                                   reproduces the reference's error codes
//   encode (extension, the reference's encoder cannot emit restart markers):
//            build_encode_intervals intervals are coded into private buffers,
//            plan_join / join_intervals  then concatenated with FF D0+m between them
#pragma once
#include <cstdint>

namespace jls {
namespace interval {

constexpr uint32_t kIntervalRetry = 8u; // ScanResult.flags: decode this scan sequentially
constexpr uint32_t kTooManyMarkers = 0xFFFFFFFFu;
constexpr uint32_t kUndecided = 4u | kIntervalRetry; // fast::kFastRetry or kIntervalRetry left in an interval's result

} // namespace interval
} // namespace jls
