// The exchange of the persistent kernels (gfx950): every launch whose workgroups wait for each
// other -- resident chain kernel, lock-step batch, persistent harmonic pass, team sweep, matrix-free
// and stored-kernel passes on teams, one-launch harmonic epilogue.  A double travels as two 8-byte
// granules {tag, 32 bits of the value}; a reader re-reads what it misses until the tags are the
// ones it waits for.
//
// Every wait is bounded, and spin_gave_up is the only place a wait spins: a workgroup that does
// not see its partners within RES_TIMEOUT_TICKS raises the launch's abort word, every other
// workgroup sees the word and leaves too, and the host falls back to a path that needs no
// co-residency (host_ctx.h: ExchangeGuard).  That is what keeps a launch whose workgroups are not
// all resident -- the GPU shared with another process -- from hanging the device.
#pragma once
#include "kernels.hip.h"

namespace ghk {

using u64 = unsigned long long;

constexpr long long RES_TIMEOUT_TICKS = 200000000LL;  // 2 s of the 100 MHz wall clock, per wait

// one double as two tagged granules at g[0], g[1]
__device__ __forceinline__ void st_gran(u64 *g, unsigned tag, double v)
{
    const u64 b = (u64)__double_as_longlong(v);
    __hip_atomic_store(g, ((u64)tag << 32) | (b & 0xffffffffull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(g + 1, ((u64)tag << 32) | (b >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the two halves of ld_gran: the loads (issue early), and what they brought (look late -- the wait
// for the loads sits where the words are first used)
__device__ __forceinline__ void ld_gran_issue(u64 *g, u64 &a, u64 &b)
{
    a = __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    b = __hip_atomic_load(g + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ bool gran_value(u64 a, u64 b, unsigned tag, double &v)
{
    v = __longlong_as_double((long long)((a & 0xffffffffull) | (b << 32)));
    return (unsigned)(a >> 32) == tag && (unsigned)(b >> 32) == tag;
}

__device__ __forceinline__ bool ld_gran(u64 *g, unsigned tag, double &v)
{
    u64 a, b;
    ld_gran_issue(g, a, b);
    return gran_value(a, b, tag, v);
}

// One turn of a wait that has not got what it waits for yet: sleep, and every 64 turns look at the
// wall clock and the abort word.  true: this wait timed out or another workgroup gave up -- the word
// is raised, the caller leaves.  spins and t0 start at 0 with every wait.
__device__ __forceinline__ bool spin_gave_up(unsigned &spins, long long &t0, unsigned *abort_w)
{
    __builtin_amdgcn_s_sleep(1);
    if ((++spins & 63u) == 0) {
        const long long now = wall_clock64();
        const long long t = t0 == 0 ? now : t0;  // (a select: `if (t0 == 0) t0 = now` compiles worse here)
        t0 = t;
        if (__hip_atomic_load(abort_w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u ||
            now - t > RES_TIMEOUT_TICKS) {
            __hip_atomic_store(abort_w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return true;
        }
    }
    return false;
}

// Every lane of the wave re-reads its granules (try_load: true when all of them carry the tag)
// until the whole wave has them.  false: timed out or another workgroup raised the abort word.
template <typename F>
__device__ __forceinline__ bool res_poll(unsigned *abort_w, F &&try_load)
{
    unsigned spins = 0;
    long long t0 = 0;
    for (;;) {
        const bool ok = try_load();
        if (__all(ok)) return true;
        if (spin_gave_up(spins, t0, abort_w)) return false;
    }
}

// At entry of a kernel that leaves its abort word raised across launches (the team family: the host
// re-arms it only after a give-up): an earlier launch on this stream gave up, the host repeats the work.
__device__ __forceinline__ bool gave_up_before(unsigned *abort_w)
{
    return __hip_atomic_load(abort_w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
}

}  // namespace ghk
