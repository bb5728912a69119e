// jsp_stamps.h — the one diagnostic build of the kernels (-DJSP_STAMPS, `make
// diag`, read by tools/stamps.py): per-workgroup and per-wave phase timestamps
// for finding where a launch's time goes. Included by jsp_kernels.hip only,
// after the HIP runtime header. The product library is built without
// JSP_STAMPS: every macro below is then empty and nothing is exported.
#pragma once

#ifdef JSP_STAMPS

namespace jsp {
__device__ unsigned long long jsp_dbg[4096 * 8];  // 4096 rows (workgroup, wave or fixed slot) of 8 stamps
}

// real-time stamp (the constant 100 MHz clock) by thread 0 of the workgroup
#define JSP_STAMP(blk, i)                                                                 \
    do {                                                                                  \
        if (threadIdx.x == 0 && (blk) < 4096) jsp_dbg[(blk) * 8 + (i)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
// shader-clock stamp (s_memtime) beside a real-time one: the effective clock of a phase
#define JSP_CLK(blk, i)                                                                   \
    do {                                                                                  \
        if (threadIdx.x == 0 && (blk) < 4096) jsp_dbg[(blk) * 8 + (i)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
#define JSP_DBGV(row, i, v)                                                               \
    do {                                                                                  \
        if (threadIdx.x == 0 && (row) < 4096) jsp_dbg[(row) * 8 + (i)] = (unsigned long long)(v); \
    } while (0)
// per-wave real-time stamp (lane 0 of each wave), and a shader-clock one
#define JSP_WSTAMP(w, i)                                                                  \
    do {                                                                                  \
        if ((threadIdx.x & 63) == 0 && (w) < 4096) jsp_dbg[(w) * 8 + (i)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
#define JSP_WCLK(w, i)                                                                    \
    do {                                                                                  \
        if ((threadIdx.x & 63) == 0 && (w) < 4096) jsp_dbg[(w) * 8 + (i)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
// The two stamps that change what they time: they wait for the loads in flight
// first, so that the phase after them is timed without its operands' latency.
// JSP_STAMP_LOADS: slot i0 before the wait and i1 after it (the loads' time).
#define JSP_STAMP_LOADS(blk, i0, i1)                     \
    do {                                                 \
        JSP_STAMP(blk, i0);                              \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); \
        JSP_STAMP(blk, i1);                              \
    } while (0)
// JSP_WSTAMP_LOADED: every counter drained, then the wave's real-time stamp i
// and shader-clock stamp ci.
#define JSP_WSTAMP_LOADED(w, i, ci)     \
    do {                                \
        __builtin_amdgcn_s_waitcnt(0);  \
        JSP_WSTAMP(w, i);               \
        JSP_WCLK(w, ci);                \
    } while (0)

extern "C" int jsp_debug_stamps(unsigned long long* out, unsigned n) {
    if (n > 4096 * 8) n = 4096 * 8;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(jsp::jsp_dbg), n * sizeof(unsigned long long)) == hipSuccess ? 0 : -2;
}
extern "C" int jsp_debug_clear() {
    static unsigned long long zero[4096 * 8];
    return hipMemcpyToSymbol(HIP_SYMBOL(jsp::jsp_dbg), zero, sizeof zero) == hipSuccess ? 0 : -2;
}

#else

#define JSP_STAMP(blk, i) \
    do {                  \
    } while (0)
#define JSP_CLK(blk, i) \
    do {                \
    } while (0)
#define JSP_DBGV(row, i, v) \
    do {                    \
    } while (0)
#define JSP_WSTAMP(w, i) \
    do {                 \
    } while (0)
#define JSP_WCLK(w, i) \
    do {               \
    } while (0)
#define JSP_STAMP_LOADS(blk, i0, i1) \
    do {                             \
    } while (0)
#define JSP_WSTAMP_LOADED(w, i, ci) \
    do {                            \
    } while (0)

#endif
