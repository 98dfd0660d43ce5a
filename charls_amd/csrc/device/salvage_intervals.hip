// salvage_intervals.hip -- restart intervals as the unit that CONFINES DAMAGE (charls_amd.h part 2g; host/batch_salvage.cpp).
//
// restart_intervals_decode.hip decodes the intervals of a sound scan side by side and hands anything irregular to the sequential
// decoder, which reports the reference's error for the whole frame.  The kernels here serve frames that already failed that
// way: they say which stretch of a damaged entropy-coded segment is which interval, let the ordinary decoders run on those
// stretches as scans of their own, keep the intervals that decode to exactly their length and fill the rest.
//
//   find_salvage_markers  one wavefront per scan: the RSTm markers of the segment (at most `max_marks` are recorded), where the
//                         segment ends (the first marker that is no RSTm, or the end of the source), whether there were more
//   plan_salvage          one wavefront per scan: the markers m_0 .. m_{M-1} cut the segment into pieces P_0 .. P_M.
//                         p = how many markers count 0, 1, 2 .. (mod 8) from the FRONT, q = how many count N-2, N-3 .. from
//                         the BACK (N intervals).  Piece k < p claims interval k, piece M - t (t < q) claims interval N-1-t; a
//                         piece with two different claims claims nothing, an interval two pieces claim is claimed by none.
//                         No piece is placed by guessing how many markers were lost.  One ScanDesc per interval: the claimed
//                         piece with the marker behind it as the interval's stream (what build_decode_intervals makes of a
//                         sound scan), or an empty scan without room for an interval nobody claims.
//   ... the ordinary decoders run on the intervals (dev::launch_decode_plain) ...
//   judge_and_fill        grid (interval, scan): an interval is KEPT when its scan ended kOk, with no undecided flag, having
//                         consumed exactly its piece (check_intervals' criterion); the rows of every other interval are filled
//                         with the caller's sample value -- after the decoders, which may have written part of them.
//                         It also judges and fills for the salvage through the seek-point index (charls_amd.h part 2h;
//                         host/batch_salvage_index.cpp), where the intervals are work items of decode_scans_wave_resume:
//                         bits of its `wide` argument choose that criterion (kByIndex, kByPrefix).
//
// Memory rules.  The marker search reads whole aligned 16-byte granules that hold at least one byte of the scan's stream
// (find_restart_markers' rule).  judge_and_fill writes the rows of lost intervals and nothing else: bytes [0, row_bytes) of
// every such row, byte stores up to the first and from the last 16-byte boundary inside the row and 16-byte stores between
// (the split of pack_streams.hip).  A 16-bit fill value is little-endian by byte position within the row, so rows at odd
// addresses are filled like any other.
#pragma once
#include <hip/hip_runtime.h>

#include "scan_model.h"

namespace jls {
namespace salvage {

// ScanResult.flags an interval's scan may not keep: fast::kFastRetry | interval::kIntervalRetry (interval::kUndecided).
constexpr uint32_t kUndecidedFlags = 4u | 8u;

// One byte per (scan, interval).
enum : uint8_t
{
    kKept = 0,
    kUnclaimed = 1,  // no piece claimed the interval
    kNotExact = 2,   // its piece did not decode to its exact length
    kNotReached = 3, // the scan was not reached (a parent without a stream)
    kOnTheIndex = 4, // part 2h, set by the host: kept, from a seek point behind a lost interval
    kPrefix = 5,     // part 2h, prefix mode: the scan's rows before its error stay, the rest is filled
};

// judge_and_fill's `wide`: bit 0 says that samples have 16 bits; the others choose the criterion (none: part 2g's).
enum : uint32_t
{
    kWideSamples = 1u,
    kByIndex = 2u,  // intervals between seek points (charls_amd.h part 2h): expect[at] = kEndsInNextPoint, or the bytes the
                    // scan's last interval must have consumed when it ended the scan
    kByPrefix = 4u, // one "interval" per scan, decoded from the top: lost rows begin at the row the result names
};
constexpr uint64_t kEndsInNextPoint = ~uint64_t{0};

// 16 bytes as one load or store through an address-space pointer (a class type cannot be copied through one).
typedef uint32_t Words4 __attribute__((vector_size(16)));

// What the search reports per scan.
struct Segment
{
    uint64_t end;     // offset (from desc.stream) of the first marker that is no RSTm; stream_capacity: none
    uint32_t marks;   // RSTm markers recorded, <= max_marks
    uint32_t overflow; // 1: there were more
};

// One wavefront per scan.  marks[scan * max_marks + j] = offset (from desc.stream) of the 0xFF of the j-th RSTm marker.
__global__ void __launch_bounds__(64) find_salvage_markers(const ScanDesc* __restrict__ descs, uint32_t* __restrict__ marks,
                                                           uint32_t max_marks, Segment* __restrict__ segments)
{
    const ScanDesc d = descs[blockIdx.x];
    const int lane = threadIdx.x;
    const uint64_t mis = (uint64_t)(reinterpret_cast<uintptr_t>(d.stream) & 15u);
    const JLS_GLOBAL_AS uint8_t* gbase = global_ptr(d.stream) - mis; // 16-byte aligned
    const uint64_t u_begin = mis, u_end = mis + d.stream_capacity;
    JLS_GLOBAL_AS uint32_t* out = global_ptr(marks) + (size_t)blockIdx.x * max_marks;
    uint32_t found = 0;
    uint64_t end = d.stream_capacity;
    for (uint64_t u0 = 0; u0 < u_end && d.stream_capacity != 0; u0 += 1024)
    {
        const uint64_t mine = u0 + (uint64_t)lane * 16;
        Words4 raw = {0, 0, 0, 0};
        if (mine < u_end)
            raw = *reinterpret_cast<const JLS_GLOBAL_AS Words4*>(gbase + mine);
        const uint32_t words[4] = {raw[0], raw[1], raw[2], raw[3]};
        uint32_t next_first = 0; // the byte after this lane's 16
        if (mine + 16 < u_end)
            next_first = gbase[mine + 16];
        uint32_t rst_mask = 0, other_mask = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j)
        {
            const uint32_t b = (words[j >> 2] >> ((j & 3) * 8)) & 0xFFu;
            const uint32_t nb = j < 15 ? ((words[(j + 1) >> 2] >> (((j + 1) & 3) * 8)) & 0xFFu) : next_first;
            const uint64_t u = mine + (uint64_t)j;
            const bool inside = u >= u_begin && u + 1 < u_end;
            const bool is_marker = inside && b == 0xFFu && nb >= 0x80u;
            const bool is_rst = is_marker && (nb & 0xF8u) == 0xD0u;
            rst_mask |= (uint32_t)is_rst << j;
            other_mask |= (uint32_t)(is_marker && !is_rst) << j;
        }
        // the first marker that is no RSTm ends the entropy-coded segment
        const unsigned long long lanes_other = __ballot(other_mask != 0);
        int stop_lane = 64, stop_bit = 16;
        if (lanes_other)
        {
            stop_lane = __ffsll(lanes_other) - 1;
            stop_bit = __ffs((int)__shfl((int)other_mask, stop_lane)) - 1;
            end = u0 + (uint64_t)stop_lane * 16 + (uint64_t)stop_bit - u_begin;
        }
        if (lane > stop_lane)
            rst_mask = 0;
        else if (lane == stop_lane)
            rst_mask &= (1u << stop_bit) - 1u;
        // ordered append
        const int mine_count = __popc(rst_mask);
        int inc = mine_count;
        for (int delta = 1; delta < 64; delta <<= 1)
        {
            const int up = __shfl_up(inc, delta);
            if (lane >= delta)
                inc += up;
        }
        uint32_t at = found + (uint32_t)(inc - mine_count);
        uint32_t m = rst_mask;
        while (m)
        {
            const int j = __ffs((int)m) - 1;
            m &= m - 1;
            if (at < max_marks)
                out[at] = (uint32_t)(mine + (uint64_t)j - u_begin);
            ++at;
        }
        const uint32_t added = (uint32_t)__shfl(inc, 63);
        found = found + added < found ? 0xFFFFFFFFu : found + added; // (saturates: only "more than max_marks" matters)
        if (lanes_other)
            break;
    }
    if (lane == 0)
    {
        JLS_GLOBAL_AS Segment* s = global_ptr(segments) + blockIdx.x;
        s->end = end;
        s->marks = found < max_marks ? found : max_marks;
        s->overflow = found > max_marks ? 1u : 0u;
    }
}

// The piece that claims interval j, or -1.  M markers, N intervals, p and q as above (plan_salvage computes them).
JLS_DEV int64_t claiming_piece(uint32_t j, uint32_t M, uint32_t N, uint32_t p, uint32_t q)
{
    // from the front: piece j (j < p), unless the piece also has a claim from the back (M - j < q) on another interval
    bool front = j < p;
    if (front && M - j < q && N - 1 - (M - j) != j)
        front = false;
    // from the back: piece M - t, t = N - 1 - j (t < q), unless the piece also has a claim from the front on another interval
    const uint32_t t = N - 1 - j;
    bool back = t < q;
    const uint32_t kb = back ? M - t : 0u; // (t < q <= M)
    if (back && kb < p && kb != j)
        back = false;
    if (front && back)
        return kb == j ? (int64_t)j : -1; // two different pieces claim it: nobody's
    if (front)
        return (int64_t)j;
    return back ? (int64_t)kb : -1;
}

// One wavefront per scan.  `marks` holds max_marks slots per scan; `intervals` = N = ceil(height / restart_interval), the same
// for every scan of the launch.  subs / expect / status: N entries per scan.  expect[i] = the bytes interval i's scan must
// consume to be kept; counts[2 * scan] = p, counts[2 * scan + 1] = q (for the tests).
__global__ void __launch_bounds__(64) plan_salvage(const ScanDesc* __restrict__ parents, const uint32_t* __restrict__ marks,
                                                   uint32_t max_marks, const Segment* __restrict__ segments, uint32_t intervals,
                                                   ScanDesc* __restrict__ subs, uint64_t* __restrict__ expect,
                                                   uint8_t* __restrict__ status, uint32_t* __restrict__ counts)
{
    const uint32_t s = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const ScanDesc parent = parents[s];
    const Segment seg = segments[s];
    const JLS_GLOBAL_AS uint32_t* mk = global_ptr(marks) + (size_t)s * max_marks;
    const JLS_GLOBAL_AS uint8_t* stream = global_ptr(parent.stream);
    const uint32_t N = intervals, M = seg.marks;
    const uint32_t most = M < N - 1 ? M : N - 1;
    const bool reached = parent.stream_capacity != 0 && parent.height != 0;

    // p: the first marker from the front that does not carry its index mod 8 -- 64 markers per ballot, the first chunk with a
    // mismatch decides
    uint32_t p = most;
    for (uint32_t k0 = 0; k0 < most; k0 += 64)
    {
        const uint32_t k = k0 + lane;
        const bool wrong = k < most && (uint32_t)stream[(uint64_t)mk[k] + 1] != 0xD0u + (k & 7u);
        const unsigned long long bad = __ballot(wrong);
        if (bad)
        {
            p = k0 + (uint32_t)__ffsll(bad) - 1u;
            break;
        }
    }
    // q: the same from the back -- marker M - 1 - t must carry (N - 2 - t) mod 8.  More markers than were recorded: the back
    // of the segment is unknown, q = 0.
    uint32_t q = seg.overflow ? 0u : most;
    for (uint32_t t0 = 0; t0 < q; t0 += 64)
    {
        const uint32_t t = t0 + lane;
        const bool wrong = t < most && (uint32_t)stream[(uint64_t)mk[M - 1 - t] + 1] != 0xD0u + ((N - 2 - t) & 7u);
        const unsigned long long bad = __ballot(wrong);
        if (bad)
        {
            q = t0 + (uint32_t)__ffsll(bad) - 1u;
            break;
        }
    }
    if (lane == 0)
    {
        global_ptr(counts)[2 * s] = p;
        global_ptr(counts)[2 * s + 1] = q;
    }

    const uint32_t lines = parent.restart_interval;
    for (uint32_t j = lane; j < N; j += 64)
    {
        const int64_t piece = reached ? claiming_piece(j, M, N, p, q) : -1;
        ScanDesc d = parent;
        d.restart_interval = 0;
        d.pixels += (uint64_t)j * lines * parent.pixel_stride;
        uint64_t want = 0;
        if (piece < 0)
        { // nobody's: an empty scan without room (build_encode_intervals' dead parents)
            d.height = 0;
            d.stream_capacity = 0;
        }
        else
        {
            const uint32_t k = (uint32_t)piece;
            const uint64_t start = k == 0 ? 0 : (uint64_t)mk[k - 1] + 2;
            const uint64_t piece_end = k < M ? (uint64_t)mk[k] : seg.end;
            // the marker behind the piece belongs to the interval's stream: it terminates the scan
            const uint64_t window_end = piece_end + 2 < parent.stream_capacity ? piece_end + 2 : parent.stream_capacity;
            const uint64_t before = (uint64_t)j * lines;
            d.height = (uint32_t)(parent.height - before < lines ? parent.height - before : lines);
            d.stream += start;
            d.stream_capacity = window_end - start;
            want = piece_end - start;
        }
        const size_t at = (size_t)s * N + j;
        subs[at] = d;
        global_ptr(expect)[at] = want;
        global_ptr(status)[at] = !reached ? kNotReached : (piece < 0 ? kUnclaimed : kKept);
    }
}

constexpr uint32_t kFillThreads = 256;

// grid (intervals, scans) x 256.  status holds plan_salvage's provisional bytes and gets the verdicts.  `fill`: the sample
// value for lost rows; `wide`: 16-bit samples (bit 0) and the criterion (kByIndex, kByPrefix: the intervals are work items
// of decode_scans_wave_resume, `status` and `expect` come from the host, the interval length is the parents'
// restart_interval as ever); row_bytes: the bytes of a row that are pixels (the same for every scan).
__global__ void __launch_bounds__(256) judge_and_fill(const ScanDesc* __restrict__ parents, uint32_t intervals,
                                                      const ScanResult* __restrict__ sub_results, const uint64_t* __restrict__ expect,
                                                      uint8_t* __restrict__ status, uint32_t fill, uint32_t wide, uint64_t row_bytes)
{
    const uint32_t j = blockIdx.x, s = blockIdx.y;
    const size_t at = (size_t)s * intervals + j;
    uint8_t verdict = global_ptr(status)[at]; // (every thread reads it before thread 0 may write it: the barrier below)
    uint64_t whole_rows = 0;                  // rows at the interval's top that stay although it is not kept (kByPrefix)
    if (verdict == kKept)
    {
        const ScanResult r = sub_results[at];
        const uint64_t want = global_ptr(expect)[at];
        if ((wide & kByPrefix) != 0)
        { // a scan from the top on decode_scans_wave_resume, seek::kResumePrefix: an error names the row it came in
            if (r.errc != kOk)
            {
                verdict = kPrefix;
                whole_rows = r.bytes;
            }
        }
        else if ((wide & kByIndex) != 0)
        { // an interval of decode_scans_wave_resume: it ends in the next point's state, or ends the scan where the index says
            // (flag bit 2 is seek::kSeekChecked here, not an undecided speed path)
            const bool holds = want == kEndsInNextPoint ? (r.flags & (2u | 4u)) == 4u : r.bytes == want;
            if (r.errc != kOk || !holds)
                verdict = kNotExact;
        }
        else if (r.errc != kOk || (r.flags & kUndecidedFlags) != 0 || r.bytes != want)
            verdict = kNotExact;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        global_ptr(status)[at] = verdict;
    if (verdict == kKept)
        return;

    const ScanDesc d = parents[s];
    const uint32_t lines = d.restart_interval;
    const uint64_t first = (uint64_t)j * lines + whole_rows;
    if (first >= d.height || whole_rows >= lines)
        return;
    const uint32_t rows = (uint32_t)(d.height - first < lines - whole_rows ? d.height - first : lines - whole_rows);
    const uint32_t lo = fill & 0xFFu, hi = (wide & kWideSamples) != 0 ? (fill >> 8) & 0xFFu : lo;
    const uint64_t pair = (uint64_t)lo | ((uint64_t)hi << 8);
    const uint64_t even = pair * 0x0001000100010001ull;      // a granule that starts on an even byte of the row
    const uint64_t odd = (even >> 8) | ((uint64_t)lo << 56); // on an odd one
    // a wavefront per row, four rows at a time
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (uint32_t r = wave; r < rows; r += kFillThreads / 64)
    {
        JLS_GLOBAL_AS uint8_t* row = global_ptr(d.pixels) + (first + r) * d.pixel_stride;
        const uintptr_t d0 = reinterpret_cast<uintptr_t>(d.pixels) + (uintptr_t)((first + r) * d.pixel_stride), d1 = d0 + row_bytes;
        // [in0, in1): the granules that lie wholly inside the row (in0 >= d1: there is none, the head is everything)
        const uintptr_t in0 = (d0 + 15) & ~uintptr_t{15}, in1 = d1 & ~uintptr_t{15};
        const uintptr_t head_end = in0 < d1 ? in0 : d1;
        if (lane < 32)
        { // head [d0, head_end) and tail [tail_begin, d1): at most 15 bytes each, one byte store per lane
            const uintptr_t tail_begin = in1 > head_end ? in1 : head_end;
            const bool head = lane < 16;
            const uintptr_t to = head ? d0 + lane : tail_begin + (lane - 16);
            if (to < (head ? head_end : d1))
            {
                const uint64_t k = to - d0;
                row[k] = (uint8_t)((k & 1u) ? hi : lo);
            }
        }
        if (in0 >= in1)
            continue;
        const uint64_t granules = (in1 - in0) / 16;
        const uint64_t k0 = in0 - d0; // the row's byte at the first interior granule
        const uint64_t pattern = (k0 & 1u) ? odd : even;
        const Words4 v = {(uint32_t)pattern, (uint32_t)(pattern >> 32), (uint32_t)pattern, (uint32_t)(pattern >> 32)};
        JLS_GLOBAL_AS Words4* interior = reinterpret_cast<JLS_GLOBAL_AS Words4*>(row + k0);
        for (uint64_t g = lane; g < granules; g += 64)
            interior[g] = v;
    }
}

} // namespace salvage
} // namespace jls
