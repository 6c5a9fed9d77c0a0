// hip_host.h -- host-side scaffolding every HIP file of the library shares (host code only): the one way an entry point fails
// (message into taxor_gpu_last_error(), code back to the caller), the check-and-return macros around HIP calls, the owning
// device buffer, a monotonic clock and the grid-size rule.
#pragma once
#include "../../include/taxor_gpu.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <string>

// taxor_gpu_last_error() lives in api.hip; every other file reaches its thread-local message through this hook
extern "C" __attribute__((visibility("hidden"))) void taxor_set_last_error(const char *msg);

namespace taxor {

// record the message, return the code
inline int fail(int code, const std::string &msg)
{
    taxor_set_last_error(msg.c_str());
    return code;
}

__attribute__((format(printf, 2, 3))) inline int fail(int code, const char *fmt, ...)
{
    char buf[768];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    taxor_set_last_error(buf);
    return code;
}

// Check a HIP call, return TAXOR_E_HIP from the enclosing function when it failed.  Two message shapes exist; a file fixes its
// shape (and prefix) in a one-line alias that also passes the call's text:  #define X_TRY(expr) TAXOR_HIP_TRY_AT(expr, #expr)
//   "<prefix>: <expr>: <hip error>"
#define TAXOR_HIP_TRY_PREFIX(prefix, expr, text)                                                                            \
    do {                                                                                                                    \
        const hipError_t e_ = (expr);                                                                                       \
        if (e_ != hipSuccess) return ::taxor::fail(TAXOR_E_HIP, std::string(prefix ": ") + text + ": " + hipGetErrorString(e_)); \
    } while (0)
//   "<expr> failed: <hip error> (<file>:<line>)"
#define TAXOR_HIP_TRY_AT(expr, text)                                                                                        \
    do {                                                                                                                    \
        const hipError_t e_ = (expr);                                                                                       \
        if (e_ != hipSuccess)                                                                                               \
            return ::taxor::fail(TAXOR_E_HIP, "%s failed: %s (%s:%d)", text, hipGetErrorString(e_), __FILE__, __LINE__);    \
    } while (0)

// One hipMalloc block and its owner.  Sizes are the caller's: every allocation has exactly the element count it is asked for,
// so a file's padding rule stands at its call site (or in its one-line helper), not in here.
template <class T> struct DeviceBuf {
    T *p = nullptr;
    uint64_t cap = 0;                    // elements allocated through alloc / reserve / grow (0 for an adopted pointer)

    DeviceBuf() = default;
    DeviceBuf(const DeviceBuf &) = delete;
    DeviceBuf &operator=(const DeviceBuf &) = delete;
    DeviceBuf(DeviceBuf &&o) noexcept : p(o.p), cap(o.cap) { (void)o.take(); }
    DeviceBuf &operator=(DeviceBuf &&o) noexcept
    {
        if (this != &o) {
            release();
            cap = o.cap;
            p = o.take();
        }
        return *this;
    }
    ~DeviceBuf() { release(); }

    // exactly n elements; what the buffer held is gone
    hipError_t alloc(uint64_t n)
    {
        release();
        const hipError_t e = hipMalloc((void **)&p, n * sizeof(T));
        if (e == hipSuccess) cap = n;
        else p = nullptr;
        return e;
    }
    // room for n elements: nothing happens when they fit, else alloc(padded)
    hipError_t reserve(uint64_t n, uint64_t padded) { return n <= cap ? hipSuccess : alloc(padded); }
    // room for n elements with the first `keep` of them preserved: nothing happens when they fit, else a block of `padded`
    // elements takes over (the copy runs on st, which is synchronised)
    hipError_t grow(uint64_t n, uint64_t padded, uint64_t keep, hipStream_t st)
    {
        if (p && n <= cap) return hipSuccess;
        T *q = nullptr;
        hipError_t e = hipMalloc((void **)&q, padded * sizeof(T));
        if (e != hipSuccess) return e;
        if (keep) {
            e = hipMemcpyAsync(q, p, keep * sizeof(T), hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) {
                (void)hipFree(q);
                return e;
            }
        }
        release();
        p = q;
        cap = padded;
        return hipSuccess;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    // hand the block to another owner
    T *take()
    {
        T *q = p;
        p = nullptr;
        cap = 0;
        return q;
    }
};

// seconds on the monotonic clock
inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// blocks for `items` work items at `per_block` each: at least one, at most `cap`
inline int grid_for(uint64_t items, uint64_t per_block, uint64_t cap)
{
    return (int)std::max<uint64_t>(1, std::min<uint64_t>(cap, (items + per_block - 1) / per_block));
}

} // namespace taxor
