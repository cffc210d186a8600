// Bootstrap replicates of the conjugate-gradient inversion in lock-step (gfx950, wave64).
//
// Up to 16 replicates share the weighted kernel Aw and differ only in the draw counts c_b applied to
// the N-vector between forward and adjoint (reginv.py:715-755 with |Aw_s v - d_s|^2 = sum_r c_r (..)^2),
// so the recurrence of BootStrap.CG (reginv.py:631-713) runs on the skinny GEMMs of batch.hip.h: one
// adjoint (bscg_adjoint_kernel: batch_adjoint_kernel's contraction with the CG epilogue) and two forwards (batch_forward_kernel,
// batch_reduce_kernel: Aw.Iw and Aw.x_new) per lock-step, every product of the sequential loop that
// repeats one the loop already had taken from D.
//
// Layouts: replicate-interleaved X[j][b], I[j][b], Iw[j][b] (M x 16), D[i][b], F[i][b], counts[i][b]
// (ld x 16, zero in rows >= N), residuals R = c o (D - dobs) patch-transposed as batch.hip.h's Rt.
// Per-replicate scalars: one BscgState per slot.  A slot that is not live -- b >= B, or frozen by the
// stop test -- is masked from every write-back: a frozen slot's columns keep the state at the freeze, those of
// a slot b >= B the zeros the start of the group writes (X, Iw, I, the counts, Rt by the initial residual pass),
// and every reduction runs per slot, so nothing of such a slot reaches another one.  All sums run in a fixed
// order (no atomics); a replicate's bits do not depend on the slot it sits in.
#pragma once
#include "batch.hip.h"

namespace ghk {

struct BscgState {
    double alpha;       // regularisation factor of the iteration in progress
    double data, ms;    // data(x), MS(x) at the replicate's current model
    double nI2, mu;     // |I|^2 of the last gradient, mu of the iteration in progress
    double IwI, IwIw;   // Iw.I and |Iw|^2
    double kstep;
    int live;           // 1: advancing; 0: unused slot, or frozen by the stop test
    int n_entries;      // misfit entries recorded
    int n_alpha;        // regularisation factors recorded
    int pad;
};

// MS stabiliser of BootStrap (no prior, beta squared: reginv.py:599-629) at x = mw, w2 = wm^2
__device__ __forceinline__ double bscg_ms(double x, double w2, double beta2)
{
    const double x2 = x * x;
    return (w2 * x2) / (x2 + beta2);
}

__device__ __forceinline__ double bscg_ms_grad(double x, double w2, double beta2)
{
    const double den = x * x + beta2;
    return (2.0 * beta2 * w2 * x) / (den * den);
}

struct BscgAdjArgs {
    const double *Gb, *G;  // as BatchAdjArgs
    int64_t ld, M;
    int np;
    const double *Rt;
    const double *X;       // M x 16
    const double *wm2;     // M
    double beta2;
    const BscgState *st;
    double *I;             // M x 16
    double *nI2_part;      // n_waves x 16
    int n_waves;
};

// I[j][b] = 2 <Aw_j, R_b> + alpha_b g_MS(x[j][b]) and the per-wave partials of |I|^2.  The contraction is
// batch_adjoint_kernel's, statement for statement (two 16-column tiles per wave, ring of three patches, every load
// unconditional); a second kernel rather than a shared device function: with the loop hoisted the compiler gave
// both kernels 114 + 16 registers and 3 waves per SIMD where batch_adjoint_kernel has 108 + 16 and 4.
__global__ void __launch_bounds__(256) bscg_adjoint_kernel(BscgAdjArgs a)
{
    const int lane = threadIdx.x & 63;
    const int lo = lane & 15, k = lane >> 4;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t ntiles = (a.M + 15) / 16;
    const int64_t npairs = (ntiles + 1) / 2;
    const bool tiled = a.Gb != nullptr;
    double s = 0.0;
    for (int64_t pair = wave; pair < npairs; pair += a.n_waves) {
        // column-major G: 16 columns x 64 B per load.  Gb: the tile's operands are one contiguous
        // stream (1 KiB per load), which is what keeps HBM pages open.
        const d2 *gcol[2];
        bool tile_ok[2], col_ok[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t tile = 2 * pair + h;
            const int64_t ja = tile * 16 + lo;  // the column this lane feeds as A operand
            tile_ok[h] = tile < ntiles;
            col_ok[h] = tile_ok[h] && (tiled || ja < a.M);
            gcol[h] = tiled ? reinterpret_cast<const d2 *>(a.Gb) + (tile_ok[h] ? tile : 0) * a.np * 128 + lane
                            : reinterpret_cast<const d2 *>(a.G + (col_ok[h] ? ja : 0) * a.ld) + k;
        }
        const int gstep = tiled ? 128 : 8, ghalf = tiled ? 64 : 4;
        const d2 *rt = reinterpret_cast<const d2 *>(a.Rt) + (k * 16 + lo);
        d4 acc[2] = {d4{0.0, 0.0, 0.0, 0.0}, d4{0.0, 0.0, 0.0, 0.0}};
        // software pipeline: two patches are in flight while one is multiplied (ring of three)
        d2 g0[3][2], g1[3][2], r0[3], r1[3];
        // (every load unconditional -- patches past the end re-read the last one, columns past M the
        // first, and the residual fragment is zeroed AFTER it arrived: one conditional load here and
        // the compiler waits with vmcnt(0) in front of every multiply, so nothing is in flight
        // while a patch is multiplied; see sweep_kernel)
        const int plast = a.np - 1;
        auto fetch = [&](int slot, int p) {
            const bool ok = p < a.np;
            const int pc = ok ? p : plast;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                g0[slot][h] = __builtin_nontemporal_load(gcol[h] + (int64_t)gstep * pc);
                g1[slot][h] = __builtin_nontemporal_load(gcol[h] + (int64_t)gstep * pc + ghalf);
            }
            const d2 ra = rt[128 * pc], rb = rt[128 * pc + 64];
            r0[slot] = ok ? ra : d2{0.0, 0.0};
            r1[slot] = ok ? rb : d2{0.0, 0.0};
        };
        auto mult = [&](int slot) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                acc[h] = mfma_f64(g0[slot][h].x, r0[slot].x, acc[h]);
                acc[h] = mfma_f64(g0[slot][h].y, r0[slot].y, acc[h]);
                acc[h] = mfma_f64(g1[slot][h].x, r1[slot].x, acc[h]);
                acc[h] = mfma_f64(g1[slot][h].y, r1[slot].y, acc[h]);
            }
        };
        fetch(0, 0);
        fetch(1, 1);
        for (int p = 0; p < a.np; p += 3) {  // zero patches beyond np add nothing
            fetch(2, p + 2);
            mult(0);
            fetch(0, p + 3);
            mult(1);
            fetch(1, p + 4);
            mult(2);
        }
        // acc[h][q] = <Aw_j, R_b> for column j = 16 (2 pair + h) + k + 4 q and replicate b = lo
        const bool live = a.st[lo].live != 0;
        const double alpha = a.st[lo].alpha;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (!tile_ok[h]) continue;
            const int64_t j0 = (2 * pair + h) * 16;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int64_t j = j0 + k + 4 * q;
                if (j >= a.M || !live) continue;
                const int64_t idx = j * CB + lo;
                const double g = 2.0 * acc[h][q] + alpha * bscg_ms_grad(a.X[idx], a.wm2[j], a.beta2);
                a.I[idx] = g;
                s += g * g;
            }
        }
    }
    // lanes lo, lo+16, lo+32, lo+48 hold parts of replicate lo: combine in fixed order
    s += __shfl_xor(s, 16, WAVE);
    s += __shfl_xor(s, 32, WAVE);
    if (lane < 16 && wave < a.n_waves) a.nI2_part[(int64_t)wave * CB + lane] = s;
}

// sum over the rows of part[rows][16] for replicate c, by the 1024 threads of a workgroup in fixed order
__device__ __forceinline__ double bscg_rows_sum(const double *part, int rows, int c, double *red)
{
    double s = 0.0;
    for (int t = threadIdx.x; t < rows; t += 1024) s += part[(int64_t)t * CB + c];
    return block_allreduce_sum(s, red, 16);
}

// One workgroup per replicate, after the adjoint: |I|^2 and mu = |I|^2 / |I_old|^2 (k >= 1)
__global__ void __launch_bounds__(1024) bscg_mu_kernel(const double *nI2_part, int n_waves, int k, BscgState *st)
{
    __shared__ double red[16];
    const int c = blockIdx.x;
    if (!st[c].live) return;
    const double s = bscg_rows_sum(nI2_part, n_waves, c, red);
    if (threadIdx.x == 0) {
        st[c].mu = k > 0 ? s / st[c].nI2 : 0.0;
        st[c].nI2 = s;
    }
}

// Direction: Iw = I (k = 0) or I + mu Iw, and the per-block partials of Iw.I and |Iw|^2
// (block = 16 cells x 16 replicates, grid-stride; part: [0] Iw.I, [1] |Iw|^2, gridDim.x x 16 each)
__global__ void __launch_bounds__(256)
bscg_direction_kernel(const double *I, double *Iw, int64_t M, int k, const BscgState *st, double *part)
{
    __shared__ double red[2][16][17];
    const int c = threadIdx.x & 15, q = threadIdx.x >> 4;
    const bool live = st[c].live != 0;
    const double mu = st[c].mu;
    double s1 = 0.0, s2 = 0.0;
    if (live) {
        for (int64_t j = (int64_t)blockIdx.x * 16 + q; j < M; j += (int64_t)gridDim.x * 16) {
            const int64_t idx = j * CB + c;
            const double g = I[idx];
            const double w = k > 0 ? g + mu * Iw[idx] : g;
            Iw[idx] = w;
            s1 += w * g;
            s2 += w * w;
        }
    }
    red[0][q][c] = s1;
    red[1][q][c] = s2;
    __syncthreads();
    if (q < 2) {
        double t = 0.0;
#pragma unroll
        for (int r = 0; r < 16; ++r) t += red[q][r][c];
        part[((int64_t)q * gridDim.x + blockIdx.x) * CB + c] = t;
    }
}

// One workgroup per replicate, after F = Aw.Iw: kstep = Iw.I / (sum_i c_i F_i^2 + alpha |Iw|^2)
__global__ void __launch_bounds__(1024)
bscg_kstep_kernel(const double *F, const double *counts, int64_t N, const double *part, int nblk, BscgState *st)
{
    __shared__ double red[16];
    const int c = blockIdx.x;
    if (!st[c].live) return;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += 1024) {
        const double f = F[i * CB + c];
        s += counts[i * CB + c] * f * f;
    }
    const double den = block_allreduce_sum(s, red, 16);
    const double IwI = bscg_rows_sum(part, nblk, c, red);
    const double IwIw = bscg_rows_sum(part + (int64_t)nblk * CB, nblk, c, red);
    if (threadIdx.x == 0) {
        st[c].IwI = IwI;
        st[c].IwIw = IwIw;
        st[c].kstep = IwI / (den + st[c].alpha * IwIw);
    }
}

// Step: x_new = wm o clamp((x - kstep Iw) o (1 / wm), rhomin, rhomax) in place -- unweight, clamp,
// reweight, as the sequential step does -- and the per-block partials of MS(x_new)
__global__ void __launch_bounds__(256)
bscg_step_kernel(double *X, const double *Iw, const double *wm, const double *iw, const double *wm2, int64_t M, double rhomin,
                 double rhomax, double beta2, const BscgState *st, double *mspart)
{
    __shared__ double red[16][17];
    const int c = threadIdx.x & 15, q = threadIdx.x >> 4;
    const bool live = st[c].live != 0;
    const double kstep = st[c].kstep;
    double s = 0.0;
    if (live) {
        for (int64_t j = (int64_t)blockIdx.x * 16 + q; j < M; j += (int64_t)gridDim.x * 16) {
            const int64_t idx = j * CB + c;
            double t = (X[idx] - kstep * Iw[idx]) * iw[j];
            if (t < rhomin) t = rhomin;
            if (t > rhomax) t = rhomax;
            const double xn = wm[j] * t;
            X[idx] = xn;
            s += bscg_ms(xn, wm2[j], beta2);
        }
    }
    red[q][c] = s;
    __syncthreads();
    if (q == 0) {
        double t = 0.0;
#pragma unroll
        for (int r = 0; r < 16; ++r) t += red[r][c];
        mspart[(int64_t)blockIdx.x * CB + c] = t;
    }
}

struct BscgResArgs {
    int64_t N, ld, M;
    const double *D;        // ld x 16: Aw.x at the replicate's new model
    const double *counts;   // ld x 16
    const double *dobs;     // ld
    const double *mspart;   // n_mspart x 16 (n_mspart = 0: MS is not wanted, the initial evaluation)
    int n_mspart;
    int k;                  // the iteration this evaluation ends; -1: the initial one
    int maxk;
    double q;
    double *Rt;
    BscgState *st;
    double *dmis, *mmis;    // 16 x (maxk - 1)
    double *alpha;          // 16 x maxk
};

// One workgroup per replicate, after D = Aw.x_new: data(x_new), the residuals of the next adjoint, the stop test, the
// iteration's misfit entries and the regularisation factor of the next iteration (BootStrap.CG's alpha rule, with every
// data value taken from the forward that ended the iteration before).
__global__ void __launch_bounds__(1024) bscg_residual_kernel(BscgResArgs a)
{
    __shared__ double red[16];
    const int c = blockIdx.x;
    BscgState &s = a.st[c];
    if (!s.live) {
        // (the initial pass: an unused slot's residuals are zeroed -- the buffer is the chain batch's and may
        // hold an earlier group's; a frozen slot keeps its own)
        if (a.k < 0)
            for (int64_t i = threadIdx.x; i < a.ld; i += 1024) {
                const int64_t p = i >> 4, r = i & 15;
                a.Rt[(((p * 2 + (r >> 3)) * 4 + ((r & 7) >> 1)) * CB + c) * 2 + (r & 1)] = 0.0;
            }
        return;
    }
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < a.ld; i += 1024) {
        double ri = 0.0;
        if (i < a.N) {
            const double res = a.D[i * CB + c] - a.dobs[i];
            const double cn = a.counts[i * CB + c];
            acc += cn * res * res;
            ri = cn * res;
        }
        const int64_t p = i >> 4, r = i & 15;  // row r = 8 h + 2 k + t of patch p
        a.Rt[(((p * 2 + (r >> 3)) * 4 + ((r & 7) >> 1)) * CB + c) * 2 + (r & 1)] = ri;
    }
    const double data = block_allreduce_sum(acc, red, 16);
    const double ms = a.n_mspart > 0 ? bscg_rows_sum(a.mspart, a.n_mspart, c, red) : 0.0;
    if (threadIdx.x != 0) return;
    const double data_prev = s.data;
    s.data = data;
    s.ms = ms;
    if (a.k >= 1) {
        if (data < 0.1) {  // frozen before this iteration's entries are appended, as the sequential loop breaks
            s.live = 0;
            return;
        }
        a.dmis[(int64_t)c * (a.maxk - 1) + s.n_entries] = data / (double)a.N;
        a.mmis[(int64_t)c * (a.maxk - 1) + s.n_entries] = ms / (double)a.M;
        s.n_entries += 1;
    }
    const int next = a.k + 1;
    if (next >= a.maxk) return;
    if (next == 0)
        s.alpha = 0.0;
    else if (next == 1)
        s.alpha = data / ms;
    else if (data_prev - data < 0.01 * data_prev)
        s.alpha = a.q * s.alpha;
    a.alpha[(int64_t)c * a.maxk + s.n_alpha] = s.alpha;
    s.n_alpha += 1;
}

// Start of a group: the B live slots at the weighted start model, every other slot zero; 1 / wm
__global__ void __launch_bounds__(256)
bscg_init_kernel(const double *mw0, const double *wm, int B, int64_t M, double *X, double *I, double *Iw, double *iw,
                 BscgState *st)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < CB) {
        BscgState z{};
        z.live = t < B ? 1 : 0;
        st[t] = z;
    }
    if (t >= M * CB) return;
    const int c = (int)(t & 15);
    const int64_t j = t >> 4;
    X[t] = c < B ? mw0[j] : 0.0;
    I[t] = 0.0;
    Iw[t] = 0.0;
    if (c == 0) iw[j] = 1.0 / wm[j];
}

// models of the B replicates, unweighted and replicate-major: out[b][j] = X[j][b] (1 / wm[j])
__global__ void __launch_bounds__(256)
bscg_models_kernel(const double *X, const double *iw, int B, int64_t M, double *out)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= M * CB) return;
    const int c = (int)(t & 15);
    const int64_t j = t >> 4;
    if (c < B) out[(int64_t)c * M + j] = X[t] * iw[j];
}

}  // namespace ghk
