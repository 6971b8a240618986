// Shared helpers for the gfx950 kernels of libi2vsgg_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <mutex>
#include "../../include/i2vsgg_hip.h"

#define I2V_WAVE 64

void i2v_set_error(const char* fmt, ...);
extern int g_i2v_tuning[];       // api.cpp; indexed by I2V_TUNE_*

#define I2V_CHECK_ARG(cond, ...)                 \
    do {                                         \
        if (!(cond)) {                           \
            i2v_set_error(__VA_ARGS__);          \
            return I2V_ERR_ARG;                  \
        }                                        \
    } while (0)

#define I2V_CHECK_LAUNCH(name)                                              \
    do {                                                                    \
        hipError_t e__ = hipGetLastError();                                 \
        if (e__ != hipSuccess) {                                            \
            i2v_set_error("%s: launch failed: %s", name, hipGetErrorString(e__)); \
            return I2V_ERR_LAUNCH;                                          \
        }                                                                   \
    } while (0)

// The one owner of the opt-in to large dynamic LDS (hipFuncAttributeMaxDynamicSharedMemorySize): allows Kernel `bytes` of it.
// The attribute belongs to the (kernel, device) pair, so hipFuncSetAttribute runs once per kernel and device ordinal -- `bytes`
// is therefore the most that kernel ever asks for, not one launch's share -- and every later call returns that call's result.
// On failure the caller refuses the launch (I2V_ALLOW_LDS); it does not take another route.
constexpr int I2V_MAX_DEVICES = 64;
template <auto Kernel>
hipError_t i2v_allow_dynamic_lds(size_t bytes) {
    static std::once_flag once[I2V_MAX_DEVICES];
    static hipError_t result[I2V_MAX_DEVICES];
    int dev = 0;
    const hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= I2V_MAX_DEVICES) return hipErrorInvalidDevice;
    std::call_once(once[dev], [&] {
        result[dev] = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    });
    return result[dev];
}

// name: the kernel's, for the message; the kernel itself (its template arguments may hold commas) comes last
#define I2V_ALLOW_LDS(name, bytes, ...)                                                                        \
    do {                                                                                                       \
        const hipError_t e__ = i2v_allow_dynamic_lds<__VA_ARGS__>(bytes);                                      \
        if (e__ != hipSuccess) {                                                                               \
            (void)hipGetLastError();                                                                           \
            i2v_set_error("%s: %zu bytes of dynamic LDS refused: %s", name, (size_t)(bytes), hipGetErrorString(e__)); \
            return I2V_ERR_LAUNCH;                                                                             \
        }                                                                                                      \
    } while (0)

static inline int i2v_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
static inline size_t i2v_align(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }
