// band_plan_test.cpp -- charls_amd/csrc/host/band_plan.h (row bands through restart markers, charls_amd.h part 2m) on its own:
// for every height 1 .. 20, every restart interval 1 .. 20 and every band of the scan, the pieces of the plan cover exactly the
// band's rows, each once, name no row outside their interval, mark as edges exactly the intervals that stick out of the band,
// and their stream windows are those of build_decode_intervals on a segment laid out here byte by byte.  Then the check of the
// marker numbers and the verdict.  A program of its own, built plain and with -fsanitize=address,undefined
// (tests/test_band_markers_cpu.py).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "host/band_plan.h"

using namespace jls::band;

namespace {

int failures = 0;
#define CHECK(cond)                                                                   \
    do                                                                                \
    {                                                                                 \
        if (!(cond))                                                                  \
        {                                                                             \
            if (++failures <= 20)                                                     \
                std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
        }                                                                             \
    } while (0)

// A segment of `intervals` intervals: interval j takes lengths[j] bytes, FF D0+j behind every interval but the last, and
// `behind` bytes of the source follow (an EOI, the next scan).  Returns the marks; `capacity` is the whole source.
std::vector<uint32_t> lay_out(const std::vector<uint32_t>& lengths, uint32_t behind, uint64_t& capacity,
                              std::vector<uint64_t>& starts, std::vector<uint64_t>& ends)
{
    std::vector<uint32_t> marks;
    uint64_t at = 0;
    for (size_t j = 0; j < lengths.size(); ++j)
    {
        starts.push_back(at);
        at += lengths[j];
        if (j + 1 < lengths.size())
        {
            marks.push_back(static_cast<uint32_t>(at));
            at += 2;
            ends.push_back(at); // (an interval's window includes its own marker)
        }
    }
    capacity = at + behind;
    ends.push_back(capacity); // (the last interval: to the end of the source)
    return marks;
}

void every_band_of_every_small_scan()
{
    uint64_t plans = 0;
    for (uint32_t height = 1; height <= 20; ++height)
        for (uint32_t lines = 1; lines <= 20; ++lines)
        {
            const uint32_t n = interval_count(height, lines);
            CHECK(n >= 1 && static_cast<uint64_t>(n - 1) * lines < height && static_cast<uint64_t>(n) * lines >= height);
            std::vector<uint32_t> lengths(n);
            for (uint32_t j = 0; j < n; ++j)
                lengths[j] = (j * 7 + height) % 5; // (empty intervals among them)
            uint64_t capacity = 0;
            std::vector<uint64_t> starts, ends;
            const std::vector<uint32_t> marks = lay_out(lengths, 2 + lines % 3, capacity, starts, ends);
            // (exactly n - 1 marks: a read of marks[n - 1] is a read out of bounds, which the sanitizer build reports)
            for (uint32_t first = 0; first < height; ++first)
                for (uint32_t rows = 1; first + rows <= height; ++rows)
                {
                    ++plans;
                    const Range met = intervals_met(first, rows, lines);
                    CHECK(met.j0 <= met.j1 && met.j1 < n);
                    CHECK(met.j0 * lines <= first && first < (met.j0 + 1) * lines);
                    CHECK(met.j1 * lines <= first + rows - 1 && first + rows - 1 < (met.j1 + 1) * lines);
                    std::vector<int> painted(rows, 0);
                    uint32_t edges = 0;
                    for (uint32_t j = met.j0; j <= met.j1; ++j)
                    {
                        const Piece p = piece_of(height, lines, first, rows, j, marks.data(), capacity);
                        const Piece q = piece_rows(height, lines, first, rows, j);
                        CHECK(q.first_row == p.first_row && q.rows == p.rows && q.edge == p.edge && q.skip == p.skip &&
                              q.band_row == p.band_row && q.copy_rows == p.copy_rows && q.start == 0 && q.bytes == 0);
                        CHECK(p.interval == j && p.first_row == j * lines);
                        CHECK(p.rows >= 1 && p.rows <= lines && p.first_row + p.rows <= height);
                        CHECK(p.rows == lines || j == n - 1);
                        const bool sticks_out = p.first_row < first || p.first_row + p.rows > first + rows;
                        CHECK(p.edge == sticks_out);
                        CHECK(!p.edge || j == met.j0 || j == met.j1);
                        edges += p.edge;
                        CHECK(p.copy_rows >= 1 && p.skip + p.copy_rows <= p.rows); // no row outside the interval
                        CHECK(p.edge || (p.skip == 0 && p.copy_rows == p.rows));
                        CHECK(p.band_row + p.copy_rows <= rows);
                        for (uint32_t r = 0; r < p.copy_rows && p.band_row + r < rows; ++r)
                        {
                            CHECK(p.first_row + p.skip + r == first + p.band_row + r); // the row of the scan is the row of the band
                            ++painted[p.band_row + r];
                        }
                        CHECK(p.start == starts[j] && p.start + p.bytes == ends[j]); // build_decode_intervals' window
                        CHECK(j == n - 1 || p.bytes == static_cast<uint64_t>(lengths[j]) + 2);
                        CHECK(p.start + p.bytes <= capacity);
                    }
                    CHECK(edges <= 2);
                    for (uint32_t r = 0; r < rows; ++r)
                        CHECK(painted[r] == 1);
                }
        }
    CHECK(plans > 20000);
}

void windows_of_a_damaged_layout()
{
    // marks that do not grow (a forged or misread table): a window is empty, never negative
    const uint32_t marks[3] = {10, 4, 11};
    const Piece a = piece_of(16, 4, 4, 4, 1, marks, 100);
    CHECK(a.start == 12 && a.bytes == 0);
    const Piece b = piece_of(16, 4, 8, 4, 2, marks, 100);
    CHECK(b.start == 6 && b.bytes == 7);
    const Piece last = piece_of(16, 4, 12, 4, 3, marks, 5);
    CHECK(last.start == 13 && last.bytes == 0); // the source ends in front of it
    // the largest geometry the interval decoder takes
    const Piece far = piece_of(65535, 65534, 65534, 1, 1, marks, 1u << 20);
    CHECK(far.first_row == 65534 && far.rows == 1 && !far.edge && far.band_row == 0 && far.copy_rows == 1);
    CHECK(interval_count(0xFFFFFFFFu, 1) == 0xFFFFFFFFu && interval_count(0xFFFFFFFFu, 0xFFFFFFFFu) == 1);
    const Range all = intervals_met(0, 0xFFFFFFFFu, 0xFFFFFFFFu);
    CHECK(all.j0 == 0 && all.j1 == 0);
}

void marker_numbers()
{
    uint8_t numbers[19];
    for (uint32_t k = 0; k < 19; ++k)
        numbers[k] = static_cast<uint8_t>(0xD0 + (k & 7));
    CHECK(numbers_cyclic(numbers, 0) && numbers_cyclic(numbers, 1) && numbers_cyclic(numbers, 8) && numbers_cyclic(numbers, 9) &&
          numbers_cyclic(numbers, 19));
    for (uint32_t bad = 0; bad < 19; ++bad)
        for (uint8_t wrong : {uint8_t{0xD0}, uint8_t{0xD7}, uint8_t{0xD8}, uint8_t{0xCF}, uint8_t{0x00}, uint8_t{0xFF}})
        {
            if (wrong == numbers[bad])
                continue;
            const uint8_t was = numbers[bad];
            numbers[bad] = wrong;
            CHECK(!numbers_cyclic(numbers, 19) && !numbers_cyclic(numbers, bad + 1));
            CHECK(numbers_cyclic(numbers, bad)); // (the markers in front of it still count right)
            numbers[bad] = was;
        }
}

void verdict()
{
    const uint32_t marks[3] = {5, 77, 81};
    const Piece mid = piece_of(16, 4, 4, 4, 1, marks, 100); // bytes [7, 79): 70 coded bytes and the marker
    CHECK(mid.start == 7 && mid.bytes == 72);
    CHECK(piece_holds(mid, 4, 0, 0, 70));
    CHECK(piece_holds(mid, 4, 0, 1, 70));      // 1: "decoded by the exact decoder"
    CHECK(!piece_holds(mid, 4, 0, 0, 69));     // stopped short of its marker
    CHECK(!piece_holds(mid, 4, 0, 0, 71) && !piece_holds(mid, 4, 0, 0, 72));
    CHECK(!piece_holds(mid, 4, 5, 0, 70));     // an error
    CHECK(!piece_holds(mid, 4, 0, 4, 70) && !piece_holds(mid, 4, 0, 8, 70) && !piece_holds(mid, 4, 0, 12, 70)); // undecided
    const Piece last = piece_of(16, 4, 12, 4, 3, marks, 100);
    CHECK(last.start == 83 && last.bytes == 17);
    CHECK(piece_holds(last, 4, 0, 0, 3) && piece_holds(last, 4, 0, 0, 17)); // the last interval ends with the scan, wherever
    CHECK(!piece_holds(last, 4, 4, 0, 3) && !piece_holds(last, 4, 0, 8, 3));
    Piece empty = mid;
    empty.bytes = 1; // a window too short to hold a marker never holds
    CHECK(!piece_holds(empty, 4, 0, 0, 0));
    empty.bytes = 0;
    CHECK(!piece_holds(empty, 4, 0, 0, 0));
    static_assert(kUndecidedFlags == 12u, "fast::kFastRetry | interval::kIntervalRetry");
}

} // namespace

int main()
{
    every_band_of_every_small_scan();
    windows_of_a_damaged_layout();
    marker_numbers();
    verdict();
    if (failures != 0)
    {
        std::printf("%d checks FAILED\n", failures);
        return 1;
    }
    std::printf("band plan ok\n");
    return 0;
}
