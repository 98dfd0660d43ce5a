// event_timer.h -- GPU time of what a stream runs between two points of the host's program: a pair of hipEvents.
#pragma once
#include <hip/hip_runtime.h>

#include "../device/runtime.h"
#include "common.h"

namespace jls {

class EventTimer
{
public:
    // `tolerant`: for a figure that is only reported.  A record that fails is ignored, ms() does not wait -- it is read behind
    // a synchronisation of the caller's -- and gives 0, with the error cleared, when the runtime does not give the time.
    // Otherwise every failure raises and ms() waits for the stop.
    explicit EventTimer(hipStream_t stream, bool tolerant = false) : stream_(stream), tolerant_(tolerant)
    {
        dev::hip_check(hipEventCreate(&a_));
        if (hipEventCreate(&b_) != hipSuccess)
        {
            (void)hipEventDestroy(a_);
            raise(CHARLS_AMD_ERRC_DEVICE_FAILURE);
        }
    }
    EventTimer(const EventTimer&) = delete;
    EventTimer& operator=(const EventTimer&) = delete;
    ~EventTimer()
    {
        (void)hipEventDestroy(a_);
        (void)hipEventDestroy(b_);
    }
    void start() { check(hipEventRecord(a_, stream_)); }
    void stop() { check(hipEventRecord(b_, stream_)); }
    double ms() // from start to stop
    {
        float v = 0;
        if (!tolerant_)
        {
            dev::hip_check(hipEventSynchronize(b_));
            dev::hip_check(hipEventElapsedTime(&v, a_, b_));
        }
        else if (hipEventElapsedTime(&v, a_, b_) != hipSuccess)
        {
            (void)hipGetLastError();
            v = 0;
        }
        return v;
    }

private:
    void check(hipError_t e) const
    {
        if (!tolerant_)
            dev::hip_check(e);
    }
    hipEvent_t a_{}, b_{};
    hipStream_t stream_;
    bool tolerant_;
};

} // namespace jls
