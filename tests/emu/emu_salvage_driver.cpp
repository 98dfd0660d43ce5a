// TEST-ONLY driver of the salvage kernels (salvage_intervals.hip compiled for the host), a library of its own
// (tests/test_emu_salvage.py).  The test compares the planner with the pure-Python model of tests/salvage_model.py, gives the
// judge fabricated results and lets the fill run in a canary arena.
//
// The planner also runs in a second way, for the exhaustive test (millions of scans; a thread per lane takes 70 us per scan):
// its lanes one after the other on ONE thread.  plan_salvage's only cross-lane operation is __ballot, and its control flow up
// to every ballot is the same in all lanes, so a ballot whose result is not known yet records the lane's predicate and
// abandons the lane (longjmp); when all 64 lanes have been there the result is known and the lanes run again from the top,
// one ballot further.  In the last pass every lane runs to the end.  Everything the kernel stores, it stores behind its last
// ballot.
#include <csetjmp>
#include <cstdlib>
#include <vector>

#include "emu_launch.h"

namespace emu {
BlockState* g_block = nullptr;
thread_local dim3 t_threadIdx, t_blockIdx, t_blockDim, t_gridDim;
} // namespace emu

namespace replay {
struct State
{
    std::vector<unsigned long long> known; // results of the ballots passed so far
    size_t next{};                         // the ballot the running lane comes to next
    unsigned long long building{};         // predicates of the first unknown ballot
    unsigned lane{}, abandoned{};
    jmp_buf out;
};
thread_local State* t_state = nullptr;
inline unsigned long long ballot(int pred)
{
    State& s = *t_state;
    if (s.next < s.known.size())
        return s.known[s.next++];
    if (pred)
        s.building |= 1ull << s.lane;
    _longjmp(s.out, 1);
}
} // namespace replay

inline unsigned long long salvage_ballot(int pred)
{
    return replay::t_state != nullptr ? replay::ballot(pred) : __ballot(pred);
}
#define __ballot salvage_ballot

#include "../../charls_amd/csrc/device/salvage_intervals.hip"

extern "C" {

size_t emu_sizeof_scan_desc() { return sizeof(jls::ScanDesc); }
size_t emu_sizeof_scan_result() { return sizeof(jls::ScanResult); }
size_t emu_sizeof_segment() { return sizeof(jls::salvage::Segment); }

void emu_salvage_find(const jls::ScanDesc* descs, uint32_t* marks, uint32_t max_marks, jls::salvage::Segment* segments, uint32_t scans)
{
    emu::launch(jls::salvage::find_salvage_markers, dim3(scans), dim3(64), 0, descs, marks, max_marks, segments);
}

void emu_salvage_plan(const jls::ScanDesc* parents, const uint32_t* marks, uint32_t max_marks, const jls::salvage::Segment* segments,
                      uint32_t intervals, jls::ScanDesc* subs, uint64_t* expect, uint8_t* status, uint32_t* counts, uint32_t scans)
{
    emu::launch(jls::salvage::plan_salvage, dim3(scans), dim3(64), 0, parents, marks, max_marks, segments, intervals, subs, expect,
                status, counts);
}

// The same launch, lane by lane on the calling thread (see above).
void emu_salvage_plan_replayed(const jls::ScanDesc* parents, const uint32_t* marks, uint32_t max_marks, const jls::salvage::Segment* segments,
                               uint32_t intervals, jls::ScanDesc* subs, uint64_t* expect, uint8_t* status, uint32_t* counts, uint32_t scans)
{
    replay::State state;
    replay::t_state = &state;
    emu::t_blockDim = dim3(64);
    emu::t_gridDim = dim3(scans);
    for (uint32_t s = 0; s < scans; ++s)
    {
        emu::t_blockIdx = dim3(s);
        state.known.clear();
        for (;;)
        {
            state.building = 0;
            state.abandoned = 0;
            for (state.lane = 0; state.lane < 64; ++state.lane)
            {
                emu::t_threadIdx = dim3(state.lane);
                state.next = 0;
                if (_setjmp(state.out) == 0)
                    jls::salvage::plan_salvage(parents, marks, max_marks, segments, intervals, subs, expect, status, counts);
                else
                    ++state.abandoned;
            }
            if (state.abandoned == 0)
                break;
            if (state.abandoned != 64)
                std::abort(); // the lanes did not come to the same ballot: the kernel is not what this replay assumes
            state.known.push_back(state.building);
        }
    }
    replay::t_state = nullptr;
}

void emu_salvage_judge(const jls::ScanDesc* parents, uint32_t intervals, uint32_t scans, const jls::ScanResult* sub_results,
                       const uint64_t* expect, uint8_t* status, uint32_t fill, uint32_t wide, uint64_t row_bytes)
{
    emu::launch(jls::salvage::judge_and_fill, dim3(intervals, scans), dim3(jls::salvage::kFillThreads), 0, parents, intervals,
                sub_results, expect, status, fill, wide, row_bytes);
}

} // extern "C"
