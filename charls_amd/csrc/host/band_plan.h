// band_plan.h -- the planning of a row band through restart markers (charls_amd.h part 2m; host/batch_bands.cpp), pure: no
// device, no stream, nothing but arithmetic, so that tests/band_plan runs it under the host compiler's sanitizers.
//
// A scan of `height` rows with a restart interval of `lines` rows has N = ceil(height / lines) intervals; interval j holds rows
// [j * lines, min(height, (j + 1) * lines)).  RSTm marker k (its 0xFF at marks[k], counted from the scan's first byte) ends
// interval k; the last interval ends with the scan.  The band [first, first + rows) meets intervals j0 .. j1.
#pragma once
#include <cstddef>
#include <cstdint>

namespace jls::band {

inline uint32_t interval_count(uint32_t height, uint32_t lines) noexcept
{
    return static_cast<uint32_t>((static_cast<uint64_t>(height) + lines - 1) / lines);
}

struct Range
{
    uint32_t j0, j1; // the first and the last interval the band meets
};
// rows >= 1, first + rows <= height, lines >= 1.
inline Range intervals_met(uint32_t first, uint32_t rows, uint32_t lines) noexcept
{
    return Range{first / lines, static_cast<uint32_t>((static_cast<uint64_t>(first) + rows - 1) / lines)};
}

// Interval j as a scan of its own, and what of it the band wants.
struct Piece
{
    uint32_t interval;  // j
    uint32_t first_row; // of the interval, in the scan
    uint32_t rows;      // of the interval: the height of its descriptor
    bool edge;          // it sticks out of the band: decoded aside, its wanted rows copied
    uint32_t skip;      // rows of the interval in front of the band (an edge; 0 otherwise)
    uint32_t band_row;  // the row of the band the first wanted row goes to
    uint32_t copy_rows; // wanted rows (an inner interval: all of them)
    uint64_t start;     // its stream, from the scan's first byte: behind marker j - 1, or the segment's start ...
    uint64_t bytes;     // ... up to and including marker j, or to the end of the source (build_decode_intervals' arithmetic)
};

// The rows of interval j and what of them the band wants; the stream window is left empty.
inline Piece piece_rows(uint32_t height, uint32_t lines, uint32_t first, uint32_t rows, uint32_t j) noexcept
{
    const uint64_t begin = static_cast<uint64_t>(j) * lines;
    const uint64_t end = begin + lines < height ? begin + lines : height;
    const uint64_t band_end = static_cast<uint64_t>(first) + rows;
    Piece p{};
    p.interval = j;
    p.first_row = static_cast<uint32_t>(begin);
    p.rows = static_cast<uint32_t>(end - begin);
    p.edge = begin < first || end > band_end;
    const uint64_t from = begin > first ? begin : first;
    const uint64_t to = end < band_end ? end : band_end;
    p.skip = static_cast<uint32_t>(from - begin);
    p.band_row = static_cast<uint32_t>(from - first);
    p.copy_rows = static_cast<uint32_t>(to - from);
    return p;
}

// ... with its stream window.  marks[k] for k < N - 1 (only marks[j - 1] and marks[j] are read); `capacity`: the bytes from the
// scan's first byte to the end of the source.
inline Piece piece_of(uint32_t height, uint32_t lines, uint32_t first, uint32_t rows, uint32_t j, const uint32_t* marks,
                      uint64_t capacity) noexcept
{
    const uint32_t intervals = interval_count(height, lines);
    Piece p = piece_rows(height, lines, first, rows, j);
    p.start = j == 0 ? 0 : static_cast<uint64_t>(marks[j - 1]) + 2;
    const uint64_t stop = j + 1 < intervals ? static_cast<uint64_t>(marks[j]) + 2 : capacity; // its own RSTm terminates an interval
    p.bytes = stop > p.start ? stop - p.start : 0;
    return p;
}

// The bytes behind the 0xFF of markers 0 .. count - 1: RST0 .. RST7, cyclically.
inline bool numbers_cyclic(const uint8_t* numbers, uint32_t count) noexcept
{
    for (uint32_t k = 0; k < count; ++k)
        if (numbers[k] != 0xD0u + (k & 7u))
            return false;
    return true;
}

// ScanResult.flags an interval's scan may not keep: fast::kFastRetry | interval::kIntervalRetry (interval::kUndecided).
constexpr uint32_t kUndecidedFlags = 4u | 8u;

// The verdict on one interval's result (check_intervals' rule): no error, decided, and -- but for the scan's last interval --
// exactly the bytes in front of its marker consumed.
inline bool piece_holds(const Piece& p, uint32_t intervals, uint32_t errc, uint32_t flags, uint64_t consumed) noexcept
{
    if (errc != 0 || (flags & kUndecidedFlags) != 0)
        return false;
    return p.interval + 1 >= intervals || (p.bytes >= 2 && consumed == p.bytes - 2);
}

} // namespace jls::band
