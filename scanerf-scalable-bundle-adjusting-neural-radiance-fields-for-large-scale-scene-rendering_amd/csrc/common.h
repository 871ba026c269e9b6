// common.h -- shared host/device helpers for libscanerf_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "scanerf_hip.h"

#define SCANERF_API extern "C" __attribute__((visibility("default")))

namespace scanerf {

constexpr int kWave = 64;          // CDNA4 wavefront
constexpr int kNumCU = 256;        // MI355X
constexpr int kNumXCD = 8;

// thread-local last error (scanerf_last_error)
void set_error(const char *fmt, ...);

inline int check_launch(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return 1;
    }
    return 0;
}

#define SCANERF_REQUIRE(cond, ...)                 \
    do {                                           \
        if (!(cond)) {                             \
            scanerf::set_error(__VA_ARGS__);       \
            return 2;                              \
        }                                          \
    } while (0)

// NO PACKED-F32 ARITHMETIC, and no wait-state guards.  Rounds 1-2 placed guards behind global stores, behind gathers and around
// matrix instructions (closed scheduling regions followed by s_nop) after launch-to-launch differences that came and went with
// the register allocation.  Round 3 found what those differences have in common: packed-f32 instructions (v_pk_mul/add/fma_f32,
// formed by the SLP vectoriser) in a kernel that also runs matrix instructions.  Without them no guard is needed (0 differing
// launches of 1 200 with every guard off, instruction caches swept or not; with them and no guards 199 of 199), so the kernels are
// compiled with -fno-slp-vectorize (csrc/Makefile, tools/isa_audit.py) and the guards are gone from the source: commit 2f39c6d is
// the last tree that can rebuild the guarded listings of that experiment matrix (tools/build_variant.py, tools/guard_probe.py).

// Tuning switches of the A/B experiments (launch shapes, alternative producers): environment variables read at launch time ONLY in
// a library built with -DSCANERF_EXPERIMENTS (make EXP=1); the product build compiles every one of them to its default -- no
// getenv, no hidden global state on a launch path (thread-safe, re-entrant, no globals).
#ifdef SCANERF_EXPERIMENTS
#include <stdlib.h>
inline int tune_int(const char *name, int dflt)
{
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}
inline bool tune_set(const char *name) { return getenv(name) != nullptr; }
#else
inline int tune_int(const char *, int dflt) { return dflt; }
inline bool tune_set(const char *) { return false; }
#endif

// Launch of a kernel that needs more dynamic LDS than the 64 KB a kernel gets unasked: reserve it, then launch.  `op` names the
// operation in the error text.  Returns 0 or SCANERF_REQUIRE's code; the launch itself is checked by the caller (check_launch).
template <typename... Params, typename... Args>
inline int launch_with_lds(void (*kernel)(Params...), int blocks, int threads, size_t lds_bytes, hipStream_t st, const char *op,
                           const Args &...args)
{
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    SCANERF_REQUIRE(e == hipSuccess, "%s: cannot reserve %zu B of LDS: %s", op, lds_bytes, hipGetErrorString(e));
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), lds_bytes, st, args...);
    return 0;
}

inline int ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// Grid for memory-bound 1-thread-per-item kernels: enough blocks to fill 256 CUs several
// times over, grid-stride the rest.
inline int stream_grid(int64_t items, int block, int max_blocks = kNumCU * 16)
{
    int64_t g = (items + block - 1) / block;
    if (g < 1) g = 1;
    if (g > max_blocks) g = max_blocks;
    return (int)g;
}

}  // namespace scanerf
