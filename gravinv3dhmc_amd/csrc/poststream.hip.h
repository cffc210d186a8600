// Streaming posterior: every recorded accepted state is read once where it lies in HBM and folded into running
// statistics of fixed size -- per chain Welford moments and batch means (chain-interleaved like the batch's
// Xc[j][c], stride C), and one pooled histogram per cell (bin-major: the threads of a wave hit consecutive words
// when neighbouring cells fall in the same bin).  One thread per cell, no atomics: every launch goes on the
// context's stream, two updates of one cell never overlap.  The arithmetic below is the contract the tests
// restate in NumPy (tests/poststream_host.py); contraction into fused multiply-adds is off so that the
// restatement's roundings are the kernel's.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace ghk {

constexpr int POST_MAX_CHAINS = 16;
constexpr int POST_MAX_BINS = 256;
constexpr int POST_MAX_Q = 32;

struct PostState {
    double *mean, *M2, *bsum, *bmean, *bM2;  // [j][c], stride C
    unsigned *H;                             // [k][j]
    const double *lo, *hi;                   // unweighted model bounds per cell
    const double *iw;                        // 1 / wm (nullptr: unweighted store)
    int64_t M;
    int C, B, b;
};

// samples each chain slot holds once the launch has run (the launch adds one to the slots it feeds)
struct PostCounts {
    long long n[POST_MAX_CHAINS];
};

__device__ __forceinline__ int post_bin(double m, double lo, double hi, int B)
{
#pragma clang fp contract(off)
    if (hi == lo) return 0;
    const double t = (m - lo) / (hi - lo) * (double)B;
    const double f = floor(t);
    // (comparisons on the double: values far outside the bounds do not fit an int; a NaN ends in bin 0)
    if (!(f > 0.0)) return 0;
    if (f >= (double)(B - 1)) return B - 1;
    return (int)f;
}

// one sample m of chain c at cell j; n: the chain's samples including this one
__device__ __forceinline__ void post_fold(const PostState &s, int64_t j, int c, double m, long long n)
{
#pragma clang fp contract(off)
    const int64_t i = j * s.C + c;
    double mean = s.mean[i];
    const double d = m - mean;
    mean += d / (double)n;
    s.mean[i] = mean;
    s.M2[i] += d * (m - mean);
    const double bs = s.bsum[i] + m;
    if (n % s.b == 0) {
        const long long K = n / s.b;
        const double y = bs / (double)s.b;
        double bm = s.bmean[i];
        const double e = y - bm;
        bm += e / (double)K;
        s.bmean[i] = bm;
        s.bM2[i] += e * (y - bm);
        s.bsum[i] = 0.0;
    } else {
        s.bsum[i] = bs;
    }
    const int k = post_bin(m, s.lo[j], s.hi[j], s.B);
    s.H[(int64_t)k * s.M + j] += 1u;
}

// the current state of ALL chains in `mask` out of the interleaved Xc[j][chain] (stride xstride)
__global__ void __launch_bounds__(256)
post_accum_batch_kernel(PostState s, const double *Xc, int xstride, unsigned mask, PostCounts cnt)
{
#pragma clang fp contract(off)
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= s.M) return;
    const double w = s.iw ? s.iw[j] : 1.0;
    const double *x = Xc + j * xstride;
    for (int c = 0; c < s.C; ++c) {
        if (!(mask & (1u << c))) continue;
        const double m = s.iw ? x[c] * w : x[c];
        post_fold(s, j, c, m, cnt.n[c]);
    }
}

// one chain from a contiguous row; weighted: the row holds x = wm m (else m itself)
__global__ void __launch_bounds__(256)
post_accum_row_kernel(PostState s, const double *x, int chain, int weighted, long long n)
{
#pragma clang fp contract(off)
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= s.M) return;
    const double m = (weighted && s.iw) ? x[j] * s.iw[j] : x[j];
    post_fold(s, j, chain, m, n);
}

// 1 / wm as ring_store_kernel forms it
__global__ void __launch_bounds__(256)
post_recip_kernel(const double *wm, int64_t M, double *iw)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < M) iw[j] = 1.0 / wm[j];
}

// per cell: pooled mean and population std, Gelman-Rubin R-hat, batch-means ESS (summed over the chains);
// n / K: samples and completed batches per chain slot
__global__ void __launch_bounds__(256)
post_finish_kernel(PostState s, PostCounts n, PostCounts K, double *mean, double *sd, double *rhat, double *ess)
{
#pragma clang fp contract(off)
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= s.M) return;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double *mu = s.mean + j * s.C, *m2 = s.M2 + j * s.C, *bm2 = s.bM2 + j * s.C;
    long long ntot = 0, n0 = 0;
    int rec = 0;
    bool same = true;
    for (int c = 0; c < s.C; ++c) {
        if (n.n[c] <= 0) continue;
        if (rec == 0) n0 = n.n[c];
        same = same && n.n[c] == n0;
        rec += 1;
        ntot += n.n[c];
    }
    if (rec == 0) {
        mean[j] = sd[j] = rhat[j] = ess[j] = nan;
        return;
    }
    double sm = 0.0;
    for (int c = 0; c < s.C; ++c)
        if (n.n[c] > 0) sm += (double)n.n[c] * mu[c];
    const double pm = sm / (double)ntot;
    double q = 0.0;
    for (int c = 0; c < s.C; ++c)
        if (n.n[c] > 0) q += m2[c];
    for (int c = 0; c < s.C; ++c)
        if (n.n[c] > 0) {
            const double d = mu[c] - pm;
            q += (double)n.n[c] * (d * d);
        }
    mean[j] = pm;
    sd[j] = sqrt(q / (double)ntot);
    double r = nan;
    if (rec >= 2 && same && n0 >= 2) {
        const double nn = (double)n0;
        double W = 0.0, cm = 0.0;
        for (int c = 0; c < s.C; ++c)
            if (n.n[c] > 0) {
                W += m2[c] / (nn - 1.0);
                cm += mu[c];
            }
        W /= (double)rec;
        cm /= (double)rec;
        double v = 0.0;
        for (int c = 0; c < s.C; ++c)
            if (n.n[c] > 0) {
                const double d = mu[c] - cm;
                v += d * d;
            }
        const double Bv = nn * (v / (double)(rec - 1));
        if (W != 0.0) r = sqrt(((nn - 1.0) / nn * W + Bv / nn) / W);
    }
    rhat[j] = r;
    double e = 0.0;
    for (int c = 0; c < s.C; ++c) {
        if (n.n[c] <= 0) continue;
        double ec = nan;
        if (K.n[c] >= 2) {
            const double den = (double)s.b * bm2[c] / (double)(K.n[c] - 1);
            if (den != 0.0) ec = (double)n.n[c] * (m2[c] / (double)(n.n[c] - 1)) / den;
        }
        e += ec;
    }
    ess[j] = e;
}

struct PostQ {
    double q[POST_MAX_Q];
};

// nq quantiles per cell from the pooled histogram: the smallest occupied bin whose cumulative count reaches
// q n, linear inside it; out[iq][j]
__global__ void __launch_bounds__(256)
post_quantile_kernel(PostState s, long long ntot, int nq, PostQ qs, double *out)
{
#pragma clang fp contract(off)
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= s.M) return;
    const double lo = s.lo[j], hi = s.hi[j];
    for (int iq = 0; iq < nq; ++iq) {
        double v = __longlong_as_double(0x7ff8000000000000ll);
        if (ntot > 0) {
            if (hi == lo) {
                v = lo;
            } else {
                const double target = qs.q[iq] * (double)ntot;
                long long cum = 0;
                for (int k = 0; k < s.B; ++k) {
                    const unsigned h = s.H[(int64_t)k * s.M + j];
                    if (h != 0u && ((double)(cum + h) >= target || cum + h == ntot)) {
                        v = lo + ((double)k + (target - (double)cum) / (double)h) * (hi - lo) / (double)s.B;
                        break;
                    }
                    cum += h;
                }
            }
        }
        out[(int64_t)iq * s.M + j] = v;
    }
}

}  // namespace ghk
