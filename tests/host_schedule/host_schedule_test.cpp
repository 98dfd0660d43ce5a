// The window scheduler of the host-memory batch calls (charls_amd/csrc/host/host_schedule.h) with fake lanes: threads that
// "code" their windows -- sizes and errcs come from a table drawn at random -- and finish in shuffled order.  Every offset,
// size and errc is compared with ONE serial walk over all frames (the rule of charls_amd.h part 2d, written out again here),
// every window's copy with the bytes that walk would have written.  Pure C++, no GPU; built with and without sanitizers.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

#include "host/host_schedule.h"

namespace hs = jls::host_schedule;

namespace {

int g_failed = 0;
#define CHECK(cond)                                                            \
    do                                                                         \
    {                                                                          \
        if (!(cond))                                                           \
        {                                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            ++g_failed;                                                        \
        }                                                                      \
    } while (0)

constexpr charls_jpegls_errc kOk = CHARLS_JPEGLS_ERRC_SUCCESS, kTooSmall = CHARLS_JPEGLS_ERRC_DESTINATION_TOO_SMALL,
                             kRefused = CHARLS_JPEGLS_ERRC_INVALID_ARGUMENT_STRIDE;

// ---- plan_windows: every frame in exactly one window, in order; no window over max_frames; none over the room unless it
// holds one frame; and no cut that was not needed (the frame behind a cut would not have fitted)
void check_plan(const std::vector<uint64_t>& weights, uint32_t max_frames, uint64_t room)
{
    const std::vector<uint32_t> ends = hs::plan_windows(weights, max_frames, room);
    const uint32_t count = static_cast<uint32_t>(weights.size());
    if (count == 0)
    {
        CHECK(ends.empty());
        return;
    }
    CHECK(!ends.empty() && ends.back() == count);
    uint32_t first = 0;
    for (size_t w = 0; w < ends.size(); ++w)
    {
        CHECK(ends[w] > first);
        uint64_t sum = 0;
        for (uint32_t f = first; f < ends[w]; ++f)
            sum += weights[f];
        CHECK(ends[w] - first <= max_frames);
        CHECK(sum <= room || sum == weights[first]); // (frames that weigh nothing -- refused ones -- ride along)
        if (ends[w] < count)
            CHECK(ends[w] - first == max_frames || sum + weights[ends[w]] > room);
        first = ends[w];
    }
}

struct Batch
{
    std::vector<uint64_t> sizes;           // what the "encoder" gives every frame
    std::vector<charls_jpegls_errc> errcs; // kOk, or the frame's own failure (its size is then ignored)
    uint64_t capacity;
    uint32_t alignment;
};

struct Result
{
    std::vector<uint64_t> offsets, sizes;
    std::vector<charls_jpegls_errc> errcs;
    std::vector<uint8_t> bytes; // the caller's buffer: frame f's bytes are f % 251 + 1, gaps 0, untouched 0xEE
};

uint8_t fill_of(uint32_t f)
{
    return static_cast<uint8_t>(f % 251 + 1);
}

// The serial model: one walk, the caller's order.
Result serial(const Batch& b)
{
    const uint32_t count = static_cast<uint32_t>(b.sizes.size());
    Result r{std::vector<uint64_t>(count + 1), std::vector<uint64_t>(count), std::vector<charls_jpegls_errc>(count),
             std::vector<uint8_t>(b.capacity, 0xEE)};
    uint64_t at = 0;
    bool full = false;
    for (uint32_t f = 0; f < count; ++f)
    {
        r.offsets[f] = at;
        r.sizes[f] = 0;
        r.errcs[f] = b.errcs[f];
        const bool coded = b.errcs[f] == kOk && b.sizes[f] != 0;
        if (!full && coded && at + b.sizes[f] > b.capacity)
            full = true;
        if (full)
        {
            r.errcs[f] = kTooSmall;
            continue;
        }
        if (!coded)
            continue;
        r.sizes[f] = b.sizes[f];
        std::memset(r.bytes.data() + at, fill_of(f), b.sizes[f]);
        const uint64_t end = at + b.sizes[f];
        at = (end + b.alignment - 1) / b.alignment * b.alignment;
        for (uint64_t g = end; g < at && g < b.capacity; ++g)
            r.bytes[g] = 0;
    }
    r.offsets[count] = at;
    return r;
}

// The lanes: window w on thread w % lanes; a window is "coded" into a blob of its own with offsets relative to the window,
// then settled at the turnstile and its front copied out.  `order` shuffles when each window's coding ends.
Result with_lanes(const Batch& b, const std::vector<uint32_t>& window_end, uint32_t lanes, std::mt19937& rng)
{
    const uint32_t count = static_cast<uint32_t>(b.sizes.size());
    Result r{std::vector<uint64_t>(count + 1), std::vector<uint64_t>(count), std::vector<charls_jpegls_errc>(count),
             std::vector<uint8_t>(b.capacity, 0xEE)};
    const uint32_t windows = static_cast<uint32_t>(window_end.size());
    std::vector<uint32_t> delay(windows);
    for (uint32_t& d : delay)
        d = rng() % 300;
    hs::Turnstile turnstile;
    std::atomic<int> inconsistent{0};
    std::vector<std::thread> threads;
    for (uint32_t k = 0; k < lanes; ++k)
        threads.emplace_back([&, k] {
            for (uint32_t w = k; w < windows; w += lanes)
            {
                CHECK(hs::lane_of(w, lanes) == k);
                const uint32_t first = w == 0 ? 0 : window_end[w - 1], last = window_end[w];
                // "code" the window: the blob, the window's own offsets
                std::vector<uint64_t> rel(last - first);
                std::vector<uint8_t> blob;
                uint64_t at = 0;
                for (uint32_t f = first; f < last; ++f)
                {
                    rel[f - first] = at;
                    r.errcs[f] = b.errcs[f];
                    r.sizes[f] = b.errcs[f] == kOk ? b.sizes[f] : 0;
                    if (r.sizes[f] == 0)
                        continue;
                    blob.resize(at, 0);
                    blob.insert(blob.end(), r.sizes[f], fill_of(f));
                    at = hs::round_up(at + r.sizes[f], b.alignment);
                }
                blob.resize(at, 0);
                std::this_thread::sleep_for(std::chrono::microseconds(delay[w])); // (the windows finish in any order)
                hs::Carry in{};
                if (!turnstile.enter(w, in))
                    return;
                const hs::Settled s = hs::settle_window(in, last - first, rel.data(), r.sizes.data() + first, r.errcs.data() + first,
                                                        r.offsets.data() + first, b.capacity, b.alignment);
                // (a window may start beyond the capacity -- the gap behind the last frame that fitted was cut --: it copies nothing)
                if (!s.consistent || s.copy_bytes > blob.size() || (s.copy_bytes != 0 && in.at + s.copy_bytes > b.capacity))
                {
                    std::printf("window %u: consistent %d, copy %llu of a blob of %zu to %llu, capacity %llu\n", w, s.consistent ? 1 : 0,
                                static_cast<unsigned long long>(s.copy_bytes), blob.size(), static_cast<unsigned long long>(in.at),
                                static_cast<unsigned long long>(b.capacity));
                    ++inconsistent;
                    turnstile.abandon();
                    return;
                }
                turnstile.leave(w, s.out);
                if (s.copy_bytes != 0)
                    std::memcpy(r.bytes.data() + in.at, blob.data(), s.copy_bytes); // (after leave: the copies of windows overlap)
            }
        });
    for (std::thread& t : threads)
        t.join();
    CHECK(inconsistent.load() == 0);
    r.offsets[count] = turnstile.carry().at;
    return r;
}

void compare(const Result& a, const Result& b, const char* what)
{
    const bool same = a.offsets == b.offsets && a.sizes == b.sizes && a.errcs == b.errcs && a.bytes == b.bytes;
    if (!same)
        std::printf("FAILED %s: the lanes and the serial walk differ\n", what);
    g_failed += same ? 0 : 1;
}

void scenario(std::mt19937& rng, uint32_t count, uint32_t lanes, uint32_t max_frames, uint32_t alignment, int capacity_kind)
{
    Batch b;
    b.alignment = alignment;
    std::vector<uint64_t> weights(count);
    uint64_t total = 0;
    for (uint32_t f = 0; f < count; ++f)
    {
        const uint32_t kind = rng() % 10;
        b.errcs.push_back(kind == 0 ? kRefused : kind == 1 ? kTooSmall : kOk);
        b.sizes.push_back(kind == 2 ? 0 : 1 + rng() % 700);
        weights[f] = b.errcs[f] == kOk ? 1000 + rng() % 3000 : 0;
        if (b.errcs[f] == kOk)
            total = hs::round_up(total + b.sizes[f], alignment);
    }
    // the capacity: everything fits / exactly / ends inside some frame / cuts a gap / nothing fits
    switch (capacity_kind)
    {
    case 0: b.capacity = total + 100; break;
    case 1: b.capacity = total; break;
    case 2: b.capacity = total == 0 ? 0 : rng() % total; break;
    case 3: b.capacity = total == 0 ? 0 : total - std::min<uint64_t>(total, 1 + rng() % alignment); break;
    default: b.capacity = 0; break;
    }
    const uint64_t room = 2000 + rng() % 9000;
    check_plan(weights, max_frames, room);
    const std::vector<uint32_t> window_end = hs::plan_windows(weights, max_frames, room);
    const Result want = serial(b);
    const Result got = with_lanes(b, window_end, std::max<uint32_t>(1, std::min<uint32_t>(lanes, static_cast<uint32_t>(window_end.size()))), rng);
    compare(got, want, "scenario");
}

void abandoned_turnstile()
{
    // a lane that fails frees the lanes that wait for its window, and whoever comes later
    hs::Turnstile t;
    std::atomic<int> refused{0};
    std::thread waiting([&] {
        hs::Carry in{};
        if (!t.enter(1, in)) // window 0 never leaves
            ++refused;
    });
    t.abandon();
    waiting.join();
    hs::Carry in{};
    CHECK(!t.enter(0, in));
    CHECK(refused.load() == 1);
}

} // namespace

int main()
{
    std::mt19937 rng(20251019);
    check_plan({}, 4, 100);
    check_plan({500}, 1, 100); // one frame over the room still gets a window
    check_plan({10, 10, 10, 10, 10, 10, 10}, 3, 1000);
    CHECK(hs::plan_windows({10, 10, 10, 10, 10, 10, 10}, 3, 1000) == (std::vector<uint32_t>{3, 6, 7}));
    CHECK(hs::plan_windows({60, 60, 30, 90, 5}, 100, 100) == (std::vector<uint32_t>{1, 3, 5}));
    for (uint32_t lanes : {1u, 2u, 3u, 5u})
        for (uint32_t max_frames : {1u, 2u, 3u, 7u, 1000u})
            for (uint32_t alignment : {1u, 2u, 16u, 4096u})
                for (int capacity_kind = 0; capacity_kind < 5; ++capacity_kind)
                    scenario(rng, 1 + rng() % 40, lanes, max_frames, alignment, capacity_kind);
    abandoned_turnstile();
    if (g_failed == 0)
        std::printf("host schedule ok\n");
    return g_failed == 0 ? 0 : 1;
}
