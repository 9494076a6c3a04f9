// xpbd_error.h -- the host error layer of the C ABI (not installed).  No device: the planner (xpbd_plan.cpp) uses it too.
#pragma once

#include <cstddef>

namespace xpbd {

// Records the thread's last error message (xpbd_last_error: a thread-local buffer of kErrorBytes, nothing is allocated) and
// returns `code`.  An argument may be the current message itself: set_error(rc, "%s -- more", xpbd_last_error()).
constexpr size_t kErrorBytes = 512;
int set_error(int code, const char *fmt, ...) noexcept __attribute__((format(printf, 2, 3)));
// Inside a catch block: XPBD_E_OOM, with a message naming `who` and the exception.
int abi_exception(const char *who) noexcept;

} // namespace xpbd

#define XPBD_TRY(expr)        \
    do {                      \
        if (int rc_ = (expr)) \
            return rc_;       \
    } while (0)
// Closes the function-try-block of every int entry point of the C ABI: no exception unwinds into the caller.
#define XPBD_ABI_CATCH \
    catch (...) { return ::xpbd::abi_exception(__func__); }
