// xpbd_selftest.cpp -- the device self-tests of the C ABI (division and square root, the stepper's short sequences for them, and three bandwidth probes).  They
// touch no world.
#include <cstdint>

#include <hip/hip_runtime_api.h>

#include "xpbd_internal.h"
#include "xpbd_kernels.h"

using xpbd::DeviceBuffer;
using xpbd::set_error;

extern "C" {

int xpbd_selftest_div_sqrt(int32_t device, const double *a, const double *b, double *quotient, double *root,
                           uint32_t n)
try {
    if (n && (!a || !b || !quotient || !root))
        return set_error(XPBD_E_INVALID, "xpbd_selftest_div_sqrt: NULL argument");
    if (n == 0)
        return XPBD_OK;
    XPBD_HIP_TRY(hipSetDevice(device));
    DeviceBuffer buf;
    const size_t bytes = (size_t)n * 8;
    hipError_t e = buf.reserve(4 * bytes);
    if (e != hipSuccess)
        return set_error(XPBD_E_OOM, "xpbd_selftest_div_sqrt: %s", hipGetErrorString(e));
    double *d = buf.as<double>();
    e = hipMemcpy(d, a, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + n, b, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = xpbd::launch_selftest_div_sqrt(d, d + n, d + 2 * (size_t)n, d + 3 * (size_t)n, n, nullptr);
    if (e == hipSuccess) e = hipMemcpy(quotient, d + 2 * (size_t)n, bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(root, d + 3 * (size_t)n, bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess)
        return set_error(XPBD_E_HIP, "xpbd_selftest_div_sqrt: %s", hipGetErrorString(e));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_selftest_exact_math(int32_t device, const double *x, const double *a, double h, uint32_t n, double *fast, double *plain)
try {
    if (n && (!x || !a || !fast || !plain))
        return set_error(XPBD_E_INVALID, "xpbd_selftest_exact_math: NULL argument");
    if (n == 0)
        return XPBD_OK;
    XPBD_HIP_TRY(hipSetDevice(device));
    DeviceBuffer buf;
    const size_t bytes = (size_t)n * 8;
    hipError_t e = buf.reserve(8 * bytes); // x, a, fast[3n], plain[3n]
    if (e != hipSuccess)
        return set_error(XPBD_E_OOM, "xpbd_selftest_exact_math: %s", hipGetErrorString(e));
    double *d = buf.as<double>();
    double *d_fast = d + 2 * (size_t)n, *d_plain = d + 5 * (size_t)n;
    e = hipMemcpy(d, x, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + n, a, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = xpbd::launch_selftest_exact_math(d, d + n, h, n, d_fast, d_plain, nullptr);
    if (e == hipSuccess) e = hipMemcpy(fast, d_fast, 3 * bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(plain, d_plain, 3 * bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess)
        return set_error(XPBD_E_HIP, "xpbd_selftest_exact_math: %s", hipGetErrorString(e));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_selftest_hbm_copy(int32_t device, uint64_t bytes, uint32_t repeats, double *gbytes_per_s)
try {
    if (!gbytes_per_s || bytes < 16 || bytes >= (1ull << 40) || repeats == 0)
        return set_error(XPBD_E_INVALID, "xpbd_selftest_hbm_copy: bad argument");
    *gbytes_per_s = 0.0;
    XPBD_HIP_TRY(hipSetDevice(device));
    bytes &= ~(uint64_t)15;
    DeviceBuffer src, dst;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = src.reserve(bytes);
    if (e == hipSuccess) e = dst.reserve(bytes);
    if (e == hipSuccess) e = hipMemset(src.ptr, 0x3c, bytes);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    float best_ms = 0.0f;
    for (uint32_t variant = 0; variant < xpbd::kCopyVariants && e == hipSuccess; ++variant) { // report the fastest kernel
        const uint32_t nt = variant;
        e = xpbd::launch_copy16(src.ptr, dst.ptr, bytes, nt, nullptr); // warm-up (page tables, clocks)
        if (e == hipSuccess) e = hipEventRecord(e0, nullptr);
        for (uint32_t k = 0; k < repeats && e == hipSuccess; ++k)
            e = xpbd::launch_copy16(src.ptr, dst.ptr, bytes, nt, nullptr);
        if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        float ms = 0.0f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        if (e == hipSuccess && (variant == 0 || ms < best_ms))
            best_ms = ms;
    }
    const float ms = best_ms;
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e != hipSuccess)
        return set_error(e == hipErrorOutOfMemory ? XPBD_E_OOM : XPBD_E_HIP, "xpbd_selftest_hbm_copy: %s", hipGetErrorString(e));
    *gbytes_per_s = 2.0 * (double)bytes * repeats / ((double)ms * 1e-3) / 1e9; // bytes read + bytes written
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_selftest_gather(int32_t device, uint32_t records, uint32_t record_bytes, uint32_t read_bytes, uint32_t repeats, double *gbytes_per_s)
try {
    if (!gbytes_per_s || records < 256 || (records & (records - 1)) != 0 || repeats == 0 || read_bytes > record_bytes)
        return set_error(XPBD_E_INVALID, "xpbd_selftest_gather: records must be a power of two >= 256, read_bytes <= record_bytes");
    *gbytes_per_s = 0.0;
    XPBD_HIP_TRY(hipSetDevice(device));
    const size_t in_bytes = (size_t)records * record_bytes, out_bytes = (size_t)records * 8;
    DeviceBuffer in, out;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = in.reserve(in_bytes);
    if (e == hipSuccess) e = out.reserve(out_bytes);
    if (e == hipSuccess) e = hipMemset(in.ptr, 0, in_bytes);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    float best_ms = 0.0f;
    for (uint32_t k = 0; k < repeats + 1 && e == hipSuccess; ++k) { // (the first launch warms up and is not counted)
        e = hipEventRecord(e0, nullptr);
        if (e == hipSuccess) e = xpbd::launch_gather_records(in.ptr, out.as<double>(), records, record_bytes, read_bytes, nullptr);
        if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        float ms = 0.0f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        if (e == hipSuccess && k > 0 && (k == 1 || ms < best_ms))
            best_ms = ms;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e == hipErrorInvalidValue)
        return set_error(XPBD_E_INVALID, "xpbd_selftest_gather: no kernel for %u bytes read of %u-byte records", read_bytes, record_bytes);
    if (e != hipSuccess)
        return set_error(e == hipErrorOutOfMemory ? XPBD_E_OOM : XPBD_E_HIP, "xpbd_selftest_gather: %s", hipGetErrorString(e));
    *gbytes_per_s = ((double)records * read_bytes + (double)out_bytes) / ((double)best_ms * 1e-3) / 1e9;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_selftest_field_streams(int32_t device, uint64_t bodies, uint32_t tile_major, uint32_t repeats, double *gbytes_per_s)
try {
    if (!gbytes_per_s || bodies < 64 || bodies > (1ull << 28) || repeats == 0)
        return set_error(XPBD_E_INVALID, "xpbd_selftest_field_streams: bad argument");
    *gbytes_per_s = 0.0;
    XPBD_HIP_TRY(hipSetDevice(device));
    bodies = (bodies + 63) / 64 * 64;
    const size_t in_bytes = (size_t)bodies * (xpbd::kDynFields + xpbd::kStatFields) * 8, out_bytes = (size_t)bodies * xpbd::kDynFields * 8;
    DeviceBuffer in, out;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = in.reserve(in_bytes);
    if (e == hipSuccess) e = out.reserve(out_bytes);
    if (e == hipSuccess) e = hipMemset(in.ptr, 0, in_bytes);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    float best_ms = 0.0f;
    for (uint32_t k = 0; k < repeats + 1 && e == hipSuccess; ++k) { // (the first launch warms up and is not counted)
        e = hipEventRecord(e0, nullptr);
        if (e == hipSuccess) e = xpbd::launch_field_streams(in.as<double>(), out.as<double>(), bodies, tile_major != 0, nullptr);
        if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        float ms = 0.0f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        if (e == hipSuccess && k > 0 && (k == 1 || ms < best_ms))
            best_ms = ms;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e != hipSuccess)
        return set_error(e == hipErrorOutOfMemory ? XPBD_E_OOM : XPBD_E_HIP, "xpbd_selftest_field_streams: %s", hipGetErrorString(e));
    *gbytes_per_s = (double)(in_bytes + out_bytes) / ((double)best_ms * 1e-3) / 1e9;
    return XPBD_OK;
} XPBD_ABI_CATCH

} // extern "C"
