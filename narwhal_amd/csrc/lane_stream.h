// lane_stream.h -- the streams of a lane (lane_pool.h): an ordinary lane's are plain non-blocking
// streams, a reserved lane's are non-blocking streams at the greatest priority the device reports
// (the calling thread has selected the device).
#pragma once
#include <hip/hip_runtime.h>

namespace nwv {

// out[0] greatest, out[1] least priority of the current device (numerically lower is greater);
// false when the device reports no range (both 0) or the query fails
inline bool stream_priority_range(int out[2]) {
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) {
        (void)hipGetLastError();
        least = greatest = 0;
    }
    out[0] = greatest;
    out[1] = least;
    return least != greatest;
}

inline hipError_t lane_stream_create(hipStream_t* s, bool high_priority) {
    int pr[2];
    if (high_priority && stream_priority_range(pr))
        return hipStreamCreateWithPriority(s, hipStreamNonBlocking, pr[0]);
    return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}

}  // namespace nwv
