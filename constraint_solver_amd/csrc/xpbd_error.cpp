// xpbd_error.cpp -- the thread's last error message (xpbd_error.h, xpbd_last_error in include/xpbd.h).
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <exception>

#include "../../include/xpbd.h"
#include "xpbd_error.h"

namespace {

thread_local char g_last_error[xpbd::kErrorBytes];

} // namespace

namespace xpbd {
int set_error(int code, const char *fmt, ...) noexcept
{
    char buf[kErrorBytes]; // (an argument may be g_last_error itself)
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    std::memcpy(g_last_error, buf, sizeof buf);
    return code;
}

int abi_exception(const char *who) noexcept
{
    try {
        throw;
    } catch (const std::exception &e) {
        return set_error(XPBD_E_OOM, "%s: %s", who, e.what());
    } catch (...) {
        return set_error(XPBD_E_OOM, "%s: unknown exception", who);
    }
}
} // namespace xpbd

extern "C" {

const char *xpbd_last_error(void) noexcept { return g_last_error; }

} // extern "C"
