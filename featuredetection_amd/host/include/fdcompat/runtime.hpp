// fdcompat/runtime.hpp -- glue between the reference-shaped C++ classes and the C ABI (fd_hip.h):
// one process-wide context and the status-code -> exception translation.  The reference reports
// errors as std::invalid_argument / std::runtime_error / std::logic_error caught in main()
// (ffpDetectApp.cpp:503-515); the same types are thrown here.
#pragma once
#include <stdexcept>
#include <string>
#include <vector>
#include "fd_hip.h"

namespace fdhost {

// Process-wide context (device FD_DEVICE or 0, private stream).  Throws std::runtime_error when no
// gfx950 device is usable: there is no CPU fallback.
fd_ctx* context();

inline void check(int rc) {
    if (rc == FD_OK) return;
    std::string msg = fd_last_error(context());
    switch (rc) {
        case FD_ERR_INVALID_ARGUMENT: throw std::invalid_argument(msg);
        case FD_ERR_LOGIC: throw std::logic_error(msg);
        default: throw std::runtime_error(msg);
    }
}

// The capacity contract of the C ABI's list outputs: call(out, capacity, &count) returns the status and reports the count it
// needed.  One call with room for initialCapacity items; FD_ERR_CAPACITY: one more with room for the reported count.  The final
// status goes through check, so a second FD_ERR_CAPACITY throws, and so does any other failure, without a second call
// (FD_ERR_DEVICE_CAPACITY: a larger output buffer would not help).  Returns the items, trimmed to the count.
// Count: int or int64_t, whichever the wrapped call takes.
template <class T, class Count, class Call>
std::vector<T> with_capacity(Count initialCapacity, Call call) {
    std::vector<T> out((size_t)initialCapacity);
    Count count = 0;
    int rc = call(out.data(), initialCapacity, &count);
    if (rc == FD_ERR_CAPACITY) {
        out.resize((size_t)count);
        rc = call(out.data(), count, &count);
    }
    check(rc);
    out.resize((size_t)count);
    return out;
}

}  // namespace fdhost
