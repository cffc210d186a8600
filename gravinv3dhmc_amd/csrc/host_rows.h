// libgravhmc host side: which momentum rows of a trajectory list go to the device from where they lie, and the
// gather of the others into one staging buffer.  Plain C++ (no HIP call, nothing of the context).  Included once
// by gravhmc.hip.
#pragma once

// page-locked host memory handed to the caller (gh_pinned_alloc)
struct PinnedBlock {
    char *base;
    size_t bytes;
};

struct RowCopyPlan {
    std::vector<char> direct;  // per row: sent from where it lies (the whole row inside one pinned block)
    std::vector<int> run_end;  // copy run i is the rows [run_end[i - 1], run_end[i]), the first from row 0
    int n_staged = 0;
};

// K rows of M doubles.  A run is one copy: staged rows are adjacent in the staging buffer, direct rows only where
// they are adjacent at their source.  Looks at the addresses alone.
static RowCopyPlan row_copy_plan(const double *const *src, int K, size_t M, const PinnedBlock *blocks, size_t n_blocks)
{
    RowCopyPlan p;
    p.direct.assign((size_t)K, 0);
    for (int k = 0; k < K; ++k) {
        const uintptr_t lo = (uintptr_t)src[k], hi = lo + M * sizeof(double);
        for (size_t b = 0; b < n_blocks && !p.direct[(size_t)k]; ++b)
            p.direct[(size_t)k] = lo >= (uintptr_t)blocks[b].base && hi <= (uintptr_t)blocks[b].base + blocks[b].bytes;
        p.n_staged += p.direct[(size_t)k] ? 0 : 1;
    }
    for (int k = 1; k <= K; ++k)
        if (k == K || p.direct[(size_t)k] != p.direct[(size_t)k - 1] ||
            (p.direct[(size_t)k] && (uintptr_t)src[k] != (uintptr_t)src[k - 1] + M * sizeof(double)))
            p.run_end.push_back(k);
    return p;
}

// The rows that are not direct into stage (row k at stage + k M) on nthr threads, the caller's included: thread i
// takes the rows [K i / nthr, K (i + 1) / nthr).  A thread that cannot be started (EAGAIN under a limit on the
// process's threads) costs speed only: the caller gathers its rows, and nothing is thrown.
template <class Thread = std::thread>
static void rows_gather(double *stage, const double *const *src, const char *direct, int K, size_t M, int nthr)
{
    auto part = [=](int k0, int k1) {
        for (int k = k0; k < k1; ++k)
            if (!direct[k]) memcpy(stage + (size_t)k * M, src[k], M * sizeof(double));
    };
    auto first = [=](int i) { return (int)((int64_t)K * i / nthr); };
    std::vector<Thread> pool;
    int started = 1;  // (range 0 is the caller's)
    try {
        pool.reserve((size_t)nthr - 1);
        for (; started < nthr; ++started) pool.emplace_back(part, first(started), first(started + 1));
    } catch (...) {
    }
    part(0, first(1));
    part(first(started), K);
    for (Thread &th : pool) th.join();
}
