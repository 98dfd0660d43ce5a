// host_schedule.h -- the window scheduler of the host-memory batch calls (charls_amd.h part 2i; batch_host.cpp), without any
// HIP in it: which frames form which window, which lane serves it, and how the running offset of the packed form is carried
// from window to window when the lanes finish in any order.  tests/host_schedule/host_schedule_test.cpp drives it with fake
// lanes under the sanitizers.
#pragma once
#include <algorithm>
#include <condition_variable>
#include <cstdint>
#include <mutex>
#include <vector>

#include "common.h"

namespace jls::host_schedule {

// The windows of a call: the frames in the caller's order, cut where a window holds `max_frames` frames or the next frame's
// weight -- the device bytes it needs -- no longer fits in `room`.  A window holds at least one frame, whatever its weight.
// Returns one past the last frame of every window (empty for no frames).
inline std::vector<uint32_t> plan_windows(const std::vector<uint64_t>& weights, uint32_t max_frames, uint64_t room)
{
    std::vector<uint32_t> ends;
    const uint32_t count = static_cast<uint32_t>(weights.size());
    uint64_t filled = 0;
    uint32_t held = 0;
    for (uint32_t f = 0; f < count; ++f)
    {
        if (held != 0 && (held >= max_frames || weights[f] > room - std::min(filled, room)))
        {
            ends.push_back(f);
            filled = 0;
            held = 0;
        }
        filled += weights[f];
        ++held;
    }
    if (count != 0)
        ends.push_back(count);
    return ends;
}

// Window w is served by lane w % lanes: a lane sees its windows in rising order.
inline uint32_t lane_of(uint32_t window, uint32_t lanes) noexcept
{
    return window % lanes;
}

// What a window hands to the next: where the next stream starts in the caller's buffer, and whether a frame's end lay beyond
// the capacity (that frame and every frame behind it in the caller's order get destination_too_small).
struct Carry
{
    uint64_t at;
    bool full;
};

inline uint64_t round_up(uint64_t v, uint32_t alignment) noexcept
{
    return (v + (alignment - 1)) & ~static_cast<uint64_t>(alignment - 1);
}

struct Settled
{
    Carry out;
    uint64_t copy_bytes; // the front of the window's own blob that goes to the caller's buffer at the window's base
    bool consistent;     // the window's own offsets, moved by the base, are the offsets the rule gives
};

// The offset rule of part 2d for the `count` frames of one window, coded on their own into a blob with offsets relative to
// the window (`rel_offsets`; the streams back to back under the same alignment, a frame that failed taking no room): offsets,
// sizes and errcs as the one serial walk over all frames gives them, in the caller's order.  The base of a window is a
// multiple of the alignment -- every offset the rule produces is --, so the blob needs no second pack: moved by the base it is
// in place.  Nothing at or beyond `capacity` belongs to the front that is copied.
inline Settled settle_window(Carry in, uint32_t count, const uint64_t* rel_offsets, uint64_t* sizes, charls_jpegls_errc* errcs,
                             uint64_t* offsets, uint64_t capacity, uint32_t alignment) noexcept
{
    const uint64_t base = in.at;
    Settled s{in, 0, true};
    for (uint32_t f = 0; f < count; ++f)
    {
        offsets[f] = s.out.at;
        const bool coded = !s.out.full && errcs[f] == CHARLS_JPEGLS_ERRC_SUCCESS && sizes[f] != 0;
        if (coded && sizes[f] > capacity - std::min(s.out.at, capacity))
            s.out.full = true;
        if (s.out.full)
        {
            errcs[f] = CHARLS_JPEGLS_ERRC_DESTINATION_TOO_SMALL;
            sizes[f] = 0;
            continue;
        }
        if (!coded)
        {
            sizes[f] = 0; // (a frame that failed takes no room)
            continue;
        }
        s.consistent = s.consistent && base + rel_offsets[f] == s.out.at;
        const uint64_t end = s.out.at + sizes[f];
        const uint64_t next = round_up(end, alignment);
        s.copy_bytes = std::min(next, capacity) - base; // (the zeros behind the last frame that fits stop at the capacity)
        s.out.at = next;
    }
    return s;
}

// The windows pass here in their order, whichever lane finished coding first: enter(w) waits until the windows before w have
// left and gives their carry; leave(w) hands this window's on.  A lane that fails abandons the turnstile: every enter()
// that waits, or comes later, returns false.
class Turnstile
{
public:
    bool enter(uint32_t window, Carry& in)
    {
        std::unique_lock<std::mutex> lock(m_);
        cv_.wait(lock, [&] { return abandoned_ || next_ == window; });
        in = carry_;
        return !abandoned_;
    }
    void leave(uint32_t window, Carry out)
    {
        {
            std::lock_guard<std::mutex> lock(m_);
            carry_ = out;
            next_ = window + 1;
        }
        cv_.notify_all();
    }
    void abandon()
    {
        {
            std::lock_guard<std::mutex> lock(m_);
            abandoned_ = true;
        }
        cv_.notify_all();
    }
    Carry carry()
    {
        std::lock_guard<std::mutex> lock(m_);
        return carry_;
    }

private:
    std::mutex m_;
    std::condition_variable cv_;
    uint32_t next_ = 0;
    Carry carry_{0, false};
    bool abandoned_ = false;
};

} // namespace jls::host_schedule
