// Device kernels of libgravhmc (gfx950 / CDNA4, wave64).  Included once by gravhmc.hip.
//
// Data layout in HBM
//   G      column-major N x M, leading dimension ld = roundup(N, 16) doubles, so every cell's
//          column starts on a 128-byte line; rows N..ld-1 are zero.  C2: 10^4 x 5*10^5 = 40 GB.
//   N-vectors (d, r, dobs...) are stored padded to ld with zeros; M-vectors are plain.
//   slab   [n_teams][ld] partial forward products, one row per team of the sweep.
//
// The hot kernel is `sweep_kernel`: ONE pass over G per leapfrog step.  A team (1, 4 or 16
// waves) owns a contiguous range of columns; for each column j it keeps the column in
// registers and does
//     g_j   = 2 * <G_j, r> + greg_j          (adjoint of the step that just finished)
//     p_j  -= c * g_j ;  x_j += dt * p_j ; clamp-and-reflect     (hmc.py:114-152)
//     dacc += G_j * x_j                      (forward of the NEXT step, same registers)
// so the reference's two GEMVs per potential evaluation (potential.py:698,708) cost one read
// of G.  HBM-bound: 0.5 flop/byte; no MFMA (a single chain is a GEMV).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ghk {

constexpr int WAVE = 64;

// ------------------------------------------------------------------ reductions (deterministic)

__device__ __forceinline__ double wave_allreduce_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, WAVE);
    return v;
}

// v + (v of the lane the DPP control selects; 0 where that lane does not exist or the row is masked)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_add(double v)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, ROW_MASK, 0xf, false);
    return v + __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

// Sum over the 64 lanes on the VALU (row_shr 1/2/4/8 scan inside the rows of 16, row_bcast 15/31
// across them, total read from lane 63): fixed order, result uniform.  The LDS-crossbar butterfly
// (ds_bpermute) of wave_allreduce_sum costs ~10x as much when 8 waves reduce several values each.
__device__ __forceinline__ double wave_sum_dpp(double v)
{
    v = dpp_add<0x111, 0xf>(v);
    v = dpp_add<0x112, 0xf>(v);
    v = dpp_add<0x114, 0xf>(v);
    v = dpp_add<0x118, 0xf>(v);
    v = dpp_add<0x142, 0xa>(v);
    v = dpp_add<0x143, 0xc>(v);
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, 63);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), 63);
    return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

// inclusive scan over each row of 16 lanes: lane 15 of a row holds the row's sum
__device__ __forceinline__ double row16_sum_dpp(double v)
{
    v = dpp_add<0x111, 0xf>(v);
    v = dpp_add<0x112, 0xf>(v);
    v = dpp_add<0x114, 0xf>(v);
    v = dpp_add<0x118, 0xf>(v);
    return v;
}

// Block-wide sum, fixed order, result valid in every thread.  red: LDS scratch >= nwaves doubles.
__device__ __forceinline__ double block_allreduce_sum(double v, double *red, int nwaves)
{
    v = wave_allreduce_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < nwaves; ++w) t += red[w];
    return t;
}

// ------------------------------------------------------------------------------ the G sweep

enum : int {
    SW_ADJ = 1,   // dot every column with r
    SW_UPD = 2,   // leapfrog momentum + position update with clamp-and-reflect
    SW_FWD = 4,   // accumulate G_j * x_j into the team's forward partial
    SW_PFIN = 8,  // final half-step momentum update + sum of p^2 (needs SW_ADJ)
    SW_GOUT = 16, // write the gradient 2*dot + greg to g_out (needs SW_ADJ)
    SW_GACC = 64, // with SW_GOUT: add 2*dot to g_out instead of overwriting it (row panels)
    SW_SPEC = 32  // with SW_PFIN|SW_UPD|SW_FWD: the update part is the FIRST step of the next
                  // trajectory, taken speculatively from its freshly drawn momentum pn_in
};

struct SweepArgs {
    const double *G;
    int64_t ld;           // leading dimension of G and row stride of the slab
    int64_t row0, rows;   // row panel handled by this launch (rows: multiple of 16, <= capacity)
    int64_t M;
    int64_t cols_per_team;
    int n_teams;
    int mode;
    const double *r;      // ld, residual (SW_ADJ)
    const double *greg;   // M, alpha * grad R(x) or nullptr
    const double *x_in;   // M: position before the step (SW_UPD) / the vector (SW_FWD only)
    const double *p_in;   // M: momentum before the step (SW_UPD, SW_PFIN)
    double *x_out;        // M (SW_UPD)   -- never aliases x_in: other waves of the team may
    double *p_out;        // M (SW_UPD, SW_PFIN)  still be reading the inputs
    const double *low, *high;
    double c_p;           // momentum coefficient of the SW_PFIN half step (dt/2)
    double c_u;           // momentum coefficient of the SW_UPD step (dt, or dt/2 for a first step)
    double dt;            // position step
    const double *pn_in;  // M (SW_SPEC): momentum drawn for the next trajectory
    double *g_out;        // M (SW_GOUT)
    double *slab;         // gridDim.x x ld (SW_FWD)
    double *pp_part;      // n_teams (SW_PFIN): sum of p_j^2 over the team's columns
    double *dsum;         // gridDim.x or nullptr (SW_FWD, TW > 1): sum over the rows of the block's slab row
};

using d2 = double __attribute__((ext_vector_type(2)));

// read-only inputs of a launch, read through the scalar cache (uniform address: s_load, counted by
// lgkmcnt -- the vector-memory counter then counts column requests only)
typedef const double __attribute__((address_space(4))) *kconst_ptr;
__device__ __forceinline__ kconst_ptr as_kconst(const double *p)
{
    return (kconst_ptr)(unsigned long long)p;
}

template <int EPT2>
struct ColRegs {
    d2 v[EPT2];
    double sc;  // x_j (uniform), requested with the column
};

// TW = waves per team (1, 4, 8, 16).  TW == 1: four independent wave-teams per 256-thread block.
// EPT2 = double2 elements held per thread: capacity = TW*64*EPT2*2 rows >= ld.
// PF = columns prefetched ahead (1 or 2).  NT = non-temporal loads of G (streamed once).
// JOINT: the joint gravity-magnetic store H = [Aw_gz | Aw_tf] (GH_CELL_PRISM_JOINT; a.M = 2m columns of
// a.ld rows).  The first half of the grid owns the gz columns [0, m), the second half the tf columns
// [m, 2m), so no team straddles the boundary; a team's residual in LDS is its own block's r, at
// a.r + blk * ld (r = [r_gz | r_tf], ld each), and its slab row holds its own block's partial forward
// product.
template <int TW, int EPT2, int PF, bool NT, bool JOINT = false>
__global__ void __launch_bounds__((TW == 1 ? 4 : TW) * 64) sweep_kernel(SweepArgs a)
{
    constexpr int TEAM_THREADS = TW * 64;
    constexpr int WG_TEAMS = (TW == 1) ? 4 : 1;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    // LDS: [0, ld) r ; then TW==1: 4 x ld scratch for the cross-wave forward reduce,
    //      TW>1: 2 x (TW + 8) doubles: ping-pong slots of the dot reduction + column scalars.
    double *r_s = smem;
    double *scratch = smem + a.rows;
    constexpr int SLOT = TW + 8;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int ttid = (TW == 1) ? lane : tid;  // thread index inside the team
    const int team = blockIdx.x * WG_TEAMS + ((TW == 1) ? wave : 0);
    const int64_t ld = a.ld;
    const int ld2 = (int)(a.rows >> 1);  // rows of this panel in double2 units
    const int mode = a.mode;
    // (JOINT: blk = the block this workgroup's columns belong to, lb = the workgroup's index inside it)
    int blk = 0, lb = blockIdx.x;
    if constexpr (JOINT) {
        const int half = (int)(gridDim.x >> 1);
        blk = (int)blockIdx.x >= half;
        lb = (int)blockIdx.x - blk * half;
    }

    if (mode & SW_ADJ) {
        const d2 *r2 = reinterpret_cast<const d2 *>(a.r + (JOINT ? blk * ld : 0) + a.row0);
        d2 *rs2 = reinterpret_cast<d2 *>(r_s);
        for (int e = tid; e < ld2; e += blockDim.x) rs2[e] = r2[e];
    }
    __syncthreads();

    // Columns of this team: a contiguous range for the multi-wave teams; the four one-wave teams
    // of a block (TW == 1) interleave inside the block's contiguous range, so a block streams one
    // region of G instead of four distant ones (4096 concurrent DRAM streams cost ~15 % of the
    // bandwidth at 600 x 4*10^5).  Column of iteration i: jb + i * CS, i < cnt.
    constexpr int CS = (TW == 1) ? 4 : 1;
    int64_t jb, jend;
    if constexpr (JOINT) {
        const int64_t m = a.M >> 1, c0 = blk * m;
        if (TW == 1) {
            const int64_t b0c = c0 + (int64_t)lb * (4 * a.cols_per_team);
            jend = b0c + 4 * a.cols_per_team;
            jb = b0c + wave;
        } else {
            jb = c0 + (int64_t)lb * a.cols_per_team;
            jend = jb + a.cols_per_team;
        }
        if (jend > c0 + m) jend = c0 + m;
    } else if (TW == 1) {
        const int64_t b0c = (int64_t)blockIdx.x * (4 * a.cols_per_team);
        jend = b0c + 4 * a.cols_per_team;
        jb = b0c + wave;
    } else {
        jb = (int64_t)team * a.cols_per_team;
        jend = jb + a.cols_per_team;
    }
    if (jend > a.M) jend = a.M;
    int cnt = (jb < jend) ? (int)((jend - jb + CS - 1) / CS) : 0;
    if (team >= a.n_teams) cnt = 0;
    auto colj = [&](int i) -> int64_t { return jb + (int64_t)i * CS; };

    d2 dacc[EPT2];
#pragma unroll
    for (int k = 0; k < EPT2; ++k) dacc[k] = d2{0.0, 0.0};
    double pp = 0.0;

    // Requests of one column.  They must stay in flight ACROSS the processing of the columns before:
    // the compiler counts outstanding vector loads per path and waits for the fewest any path may
    // have issued -- s_waitcnt vmcnt(0), the end of all prefetching, as soon as a younger load is
    // conditional.  So
    //   * the column is loaded unconditionally, threads past its end re-read its last double2 (never
    //     used: the dot and every store are guarded), at 32-bit offsets from a uniform base;
    //   * the per-column scalars come through the scalar cache (every wave loads them itself, x_j
    //     with the column, the others while the dot is reduced: no vector load, no LDS broadcast,
    //     no wave with a longer path than the others).
    unsigned coff[EPT2];
#pragma unroll
    for (int k = 0; k < EPT2; ++k) {
        const int e = k * TEAM_THREADS + ttid;
        coff[k] = (unsigned)(e < ld2 ? e : (ld2 > 0 ? ld2 - 1 : 0)) * (unsigned)sizeof(d2);
    }
    const kconst_ptr kx = as_kconst(a.x_in), kp = as_kconst(a.p_in), klo = as_kconst(a.low), khi = as_kconst(a.high),
                     kgr = as_kconst(a.greg), kpn = as_kconst(a.pn_in);
    auto load_col = [&](ColRegs<EPT2> &c, int64_t j) {
        c.sc = kx ? kx[j] : 0.0;
        const char *col = reinterpret_cast<const char *>(a.G + j * ld + a.row0);
#pragma unroll
        for (int k = 0; k < EPT2; ++k) {
            // (kept 32-bit next to the uniform base -- global_load v, voff, s[base] -- and in its own
            // register: as a copy it lands in the destination registers and waits for their last load)
            asm volatile("" : "+v"(coff[k]));
            const unsigned o = coff[k];
            const d2 *src = reinterpret_cast<const d2 *>(col + o);
            c.v[k] = NT ? __builtin_nontemporal_load(src) : *src;
        }
    };

    // one column: adjoint dot, leapfrog update, forward accumulation.  `it` = j - j0.
    auto process = [&](const ColRegs<EPT2> &cur, int64_t j, int it) {
        double xj = cur.sc;
        if (mode & SW_ADJ) {
            const d2 *rs2 = reinterpret_cast<const d2 *>(r_s);
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < EPT2; ++k) {
                const int e = k * TEAM_THREADS + ttid;
                if (e < ld2) {
                    const d2 rv = rs2[e];
                    s += cur.v[k].x * rv.x;
                    s += cur.v[k].y * rv.y;
                }
            }
            // (multi-wave teams: the sum over the lanes on the VALU -- DPP row scans -- instead of six
            // trips through the LDS crossbar: the per-column chain dot -> slot -> barrier -> update is
            // what a team's columns are serialised on)
            s = (TW > 1) ? wave_sum_dpp(s) : wave_allreduce_sum(s);
            const double cx = cur.sc;
            const double cp = kp ? kp[j] : 0.0, clo = klo ? klo[j] : 0.0, chi = khi ? khi[j] : 0.0,
                         cgr = kgr ? kgr[j] : 0.0, cpn = kpn ? kpn[j] : 0.0;
            if (TW > 1) {
                double *slot = scratch + (it & 1) * SLOT;
                if (lane == 0) slot[wave] = s;
                __syncthreads();
                double t = 0.0;
#pragma unroll
                for (int w = 0; w < TW; ++w) t += slot[w];
                s = t;
            }
            xj = cx;
            const double g = 2.0 * s + cgr;
            if ((mode & SW_GOUT) && ttid == 0) a.g_out[j] = (mode & SW_GACC) ? a.g_out[j] + g : g;
            if (mode & SW_PFIN) {
                const double pf = cp - a.c_p * g;
                pp += pf * pf;
                if (!(mode & SW_SPEC) && ttid == 0) a.p_out[j] = pf;
            }
            if (mode & SW_UPD) {
                const double psrc = (mode & SW_SPEC) ? cpn : cp;
                double pj = psrc - a.c_u * g;
                xj = cx + a.dt * pj;
                if (xj > chi) {
                    xj = chi;
                    pj = -pj;
                } else if (xj < clo) {
                    xj = clo;
                    pj = -pj;
                }
                if (ttid == 0) {
                    a.p_out[j] = pj;
                    a.x_out[j] = xj;
                }
            }
        }
        if (mode & SW_FWD) {
#pragma unroll
            for (int k = 0; k < EPT2; ++k) {
                dacc[k].x += cur.v[k].x * xj;
                dacc[k].y += cur.v[k].y * xj;
            }
        }
    };

    // TW > 1: one team per block, so every wave takes the same trip count (barrier inside).
    // Every trip requests a column -- past the end the last one again (a few L2 hits per team): a
    // request under a condition, even a uniform one, would again turn the waits for the columns in
    // flight into vmcnt(0).
    const int lastc = cnt - 1;
    auto ahead = [&](int i) -> int64_t { return colj(i < lastc ? i : lastc); };
    if (cnt > 0) {
        if (PF == 1) {
            ColRegs<EPT2> b0, b1;
            load_col(b0, colj(0));
            int i = 0;
            for (;;) {
                load_col(b1, ahead(i + 1));
                process(b0, colj(i), i);
                if (++i >= cnt) break;
                load_col(b0, ahead(i + 1));
                process(b1, colj(i), i);
                if (++i >= cnt) break;
            }
        } else {
            ColRegs<EPT2> b0, b1, b2;
            load_col(b0, colj(0));
            load_col(b1, ahead(1));
            int i = 0;
            for (;;) {
                load_col(b2, ahead(i + 2));
                process(b0, colj(i), i);
                if (++i >= cnt) break;
                load_col(b0, ahead(i + 2));
                process(b1, colj(i), i);
                if (++i >= cnt) break;
                load_col(b1, ahead(i + 2));
                process(b2, colj(i), i);
                if (++i >= cnt) break;
            }
        }
    }

    if ((mode & SW_PFIN) && ttid == 0 && team < a.n_teams) a.pp_part[team] = pp;

    if (mode & SW_FWD) {
        if (TW == 1) {
            // sum the block's four wave-teams through LDS, then one slab row per block
            d2 *sc2 = reinterpret_cast<d2 *>(scratch);
#pragma unroll
            for (int k = 0; k < EPT2; ++k) {
                const int e = k * 64 + lane;
                if (e < ld2) sc2[wave * ld2 + e] = dacc[k];
            }
            __syncthreads();
            d2 *out = reinterpret_cast<d2 *>(a.slab + (int64_t)blockIdx.x * ld + a.row0);
            for (int e = tid; e < ld2; e += blockDim.x) {
                const d2 s0 = sc2[e], s1 = sc2[ld2 + e], s2 = sc2[2 * ld2 + e], s3 = sc2[3 * ld2 + e];
                out[e] = ((s0 + s1) + s2) + s3;
            }
        } else {
            d2 *out = reinterpret_cast<d2 *>(a.slab + (int64_t)blockIdx.x * ld + a.row0);
            double ds = 0.0;
#pragma unroll
            for (int k = 0; k < EPT2; ++k) {
                const int e = k * TEAM_THREADS + ttid;
                if (e < ld2) {
                    out[e] = dacc[k];
                    ds += dacc[k].x;
                    ds += dacc[k].y;
                }
            }
            if (a.dsum) {
                // sum of this slab row (pad rows are zero): lets the epilogue know mean(d) before it
                // has reduced the slab (reduce_finish_kernel)
                const double t = block_allreduce_sum(ds, scratch, TW);
                if (tid == 0) a.dsum[blockIdx.x] = t;
            }
        }
    }
}

// -------------------------------------------------- finalize: slab -> d, regulariser, residual

// d[i] = sum_t slab[t][i] (fixed order), partial[b] = sum over the block's rows of
// d[i] + grav_fix[i].  Launch: grid = (ceil(ld/32), nseg), block = (32, 8).  With nseg > 1 the
// slab rows are split in nseg contiguous segments whose sums go to d[seg*ld + i] (a smaller
// slab for a second pass) and `partial` is not written.
__global__ void __launch_bounds__(256) reduce_slab_kernel(const double *slab, int n_rows_slab,
                                                          int64_t ld, int64_t N,
                                                          const double *gfix, double *d,
                                                          double *partial)
{
    __shared__ double red[8][33];
    const int rx = threadIdx.x, ty = threadIdx.y;
    const int64_t i = (int64_t)blockIdx.x * 32 + rx;
    const int nseg = gridDim.y, seg = blockIdx.y;
    const int per = (n_rows_slab + nseg - 1) / nseg;
    const int t0 = seg * per;
    const int t1 = (t0 + per < n_rows_slab) ? t0 + per : n_rows_slab;
    double acc = 0.0;
    if (i < ld) {
        int t = t0 + ty;
        for (; t + 24 < t1; t += 32) {
            const double a0 = slab[(int64_t)t * ld + i];
            const double a1 = slab[(int64_t)(t + 8) * ld + i];
            const double a2 = slab[(int64_t)(t + 16) * ld + i];
            const double a3 = slab[(int64_t)(t + 24) * ld + i];
            acc += a0;
            acc += a1;
            acc += a2;
            acc += a3;
        }
        for (; t < t1; t += 8) acc += slab[(int64_t)t * ld + i];
    }
    red[ty][rx] = acc;
    __syncthreads();
    if (ty == 0) {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) s += red[q][rx];
        if (nseg > 1) {
            if (i < ld) d[(int64_t)seg * ld + i] = s;
            return;
        }
        double dinv = 0.0;
        if (i < ld) {
            d[i] = s;
            if (i < N) dinv = s + (gfix ? gfix[i] : 0.0);
        }
        // 32 active lanes of wave 0: butterfly over 32
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) dinv += __shfl_xor(dinv, off, WAVE);
        if (rx == 0) partial[blockIdx.x] = dinv;
    }
}

struct RegArgs {
    int ms_grad_den_mw;  // 1: MS gradient denominator uses mw^2 (reginv.py:288-292) instead of (mw-mwapr)^2
    int kind;
    int64_t M;
    int nz, ny, nx;
    double alpha, beta;
    const double *x, *mwapr, *wm2;
    double *greg;     // alpha * grad R
    double *regpart;  // per-block partial of R
    // cells sharded over GPUs in whole z-planes (stencil kinds): nz is the GLOBAL plane count, k0
    // the global index of the first local plane, *lo / *hi the plane below / above the local cells
    // (model and prior model) as received from the neighbouring ranks; all zero when unsharded
    int64_t k0;
    const double *xlo, *xhi, *alo, *ahi;
    // several properties of the same mesh stacked in one model vector, property-major (the joint store's 2, the
    // magnetization-vector store's 3): nprop > 1 makes M, nz, ny, nx those of ONE property, gives each property
    // nrb = ceil(M / 256) blocks and applies the regulariser to each property on its own (the block-diagonal
    // fd3djoint: nothing crosses from one property into the next).  0 or 1: one property, as ever.
    int nprop, nrb;
};

// Stencil regularisers (Smoothness, TV), first half: model and prior model of the six neighbours of
// cell j, [2 ax] forward, [2 ax + 1] backward (the cell itself where the mesh ends: not used).  All
// twelve loads are issued before any arithmetic -- one memory latency instead of six in a row --
// and a caller with other work to do can put it between this and reg_stencil_eval.
// SC1: the neighbours' model values are read with agent-scope (sc1) loads that bypass this CU's L1
// (resident chain kernel: other workgroups wrote them, write-through, earlier in the same launch).
template <bool HALO, bool SC1>
__device__ __forceinline__ void reg_stencil_load(const RegArgs &a, int64_t j, double (&xn)[6], double (&an)[6])
{
    const int64_t nx = a.nx, ny = a.ny, nz = a.nz, P = nx * ny;
    const int64_t i = j % nx, jj = (j / nx) % ny, k = j / P + a.k0;
    const int64_t stride[3] = {1, nx, P};
    const bool fwd[3] = {i < nx - 1, jj < ny - 1, k < nz - 1};
    const bool bwd[3] = {i > 0, jj > 0, k > 0};
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const int64_t qf = fwd[ax] ? j + stride[ax] : j, qb = bwd[ax] ? j - stride[ax] : j;
        if (HALO) {
            // beyond the local planes: the neighbouring rank's boundary plane
            xn[2 * ax] = qf >= a.M ? a.xhi[qf - a.M] : a.x[qf];
            an[2 * ax] = qf >= a.M ? a.ahi[qf - a.M] : a.mwapr[qf];
            xn[2 * ax + 1] = qb < 0 ? a.xlo[qb + P] : a.x[qb];
            an[2 * ax + 1] = qb < 0 ? a.alo[qb + P] : a.mwapr[qb];
        } else {
            if (SC1) {
                xn[2 * ax] = __longlong_as_double((long long)__hip_atomic_load(
                    reinterpret_cast<const unsigned long long *>(a.x + qf), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                xn[2 * ax + 1] = __longlong_as_double((long long)__hip_atomic_load(
                    reinterpret_cast<const unsigned long long *>(a.x + qb), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            } else {
                xn[2 * ax] = a.x[qf];
                xn[2 * ax + 1] = a.x[qb];
            }
            an[2 * ax] = a.mwapr[qf];
            an[2 * ax + 1] = a.mwapr[qb];
        }
    }
    __builtin_amdgcn_sched_barrier(0);
}

// Second half: dR/dx_j from v = x_j - prior_j and the neighbours; adds the cell's share of R to
// `val` (potential.py:786-810; the finite-difference operator of potential.py:266-361 is never
// materialised)
__device__ __forceinline__ double reg_stencil_eval(const RegArgs &a, int64_t j, double v, const double (&xn)[6],
                                                   const double (&an)[6], double &val)
{
    const int64_t nx = a.nx, ny = a.ny, nz = a.nz, P = nx * ny;
    const int64_t i = j % nx, jj = (j / nx) % ny, k = j / P + a.k0;
    const bool fwd[3] = {i < nx - 1, jj < ny - 1, k < nz - 1};
    const bool bwd[3] = {i > 0, jj > 0, k > 0};
    double g = 0.0;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        if (fwd[ax]) {
            const double t = v - (xn[2 * ax] - an[2 * ax]);
            if (a.kind == 1) {
                val += t * t;
                g += 2.0 * t;
            } else {
                const double s = sqrt(t * t + a.beta);
                val += s;
                g += t / s;
            }
        }
        if (bwd[ax]) {
            const double t = (xn[2 * ax + 1] - an[2 * ax + 1]) - v;
            if (a.kind == 1)
                g -= 2.0 * t;
            else
                g -= t / sqrt(t * t + a.beta);
        }
    }
    return g;
}

// Regulariser term of cell j at the model a.x (own value xj = a.x[j] passed in; neighbours of the
// stencil kinds are read from a.x): returns dR/dx_j, adds the cell's share of R to `val`
// (potential.py:719-736, 775-810).
template <bool HALO = false, bool SC1 = false>
__device__ __forceinline__ double reg_cell(const RegArgs &a, int64_t j, double xj, double &val)
{
    const double v = xj - a.mwapr[j];
    double g = 0.0;
    if (a.kind == 0) {  // Damping
        val = v * v;
        g = 2.0 * v;
    } else if (a.kind == 2) {  // MS
        const double v2 = v * v, den = v2 + a.beta, w2 = a.wm2[j];
        val = (w2 * v2) / den;
        const double deng = a.ms_grad_den_mw ? xj * xj + a.beta : den;
        g = (2.0 * a.beta * w2 * v) / (deng * deng);
    } else {  // Smoothness (1) / TV (3)
        double xn[6], an[6];
        reg_stencil_load<HALO, SC1>(a, j, xn, an);
        g = reg_stencil_eval(a, j, v, xn, an, val);
    }
    return g;
}

// Regulariser value + gradient of one 256-cell block.  `blk`: index of the block, `red`: 4
// doubles of LDS.
template <bool HALO = false>
__device__ __forceinline__ void reg_block(const RegArgs &a, int blk, double *red)
{
    double val = 0.0;
    if (a.nprop > 1) {
        // block blk is block blk % nrb of property blk / nrb: the same cell code on that property's M entries
        const int h = blk / a.nrb;
        RegArgs p = a;
        p.x += h * a.M;
        p.mwapr += h * a.M;
        p.wm2 += h * a.M;
        const int64_t j = (int64_t)(blk - h * a.nrb) * 256 + threadIdx.x;
        if (j < a.M) a.greg[h * a.M + j] = a.alpha * reg_cell<HALO>(p, j, p.x[j], val);
    } else {
        const int64_t j = (int64_t)blk * 256 + threadIdx.x;
        if (j < a.M) a.greg[j] = a.alpha * reg_cell<HALO>(a, j, a.x[j], val);
    }
    const double tot = block_allreduce_sum(val, red, 4);
    if (threadIdx.x == 0) a.regpart[blk] = tot;
}

// Boundary planes of a sharded model for the exchange by all-reduce: hb[(2 r + which) * P + off] =
// first (which = 0) / last (which = 1) plane of rank r's cells; every rank fills its own two
// slots and zeroes the others, the sum over the ranks is the table of all boundary planes.
__global__ void __launch_bounds__(256)
halo_pack_kernel(const double *v, int64_t M, int64_t P, int rank, int world, double *hb)
{
    const int64_t n = 2 * (int64_t)world * P;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * 256) {
        const int64_t slot = idx / P, off = idx - slot * P;
        double val = 0.0;
        if ((int)(slot >> 1) == rank) val = (slot & 1) ? v[M - P + off] : v[off];
        hb[idx] = val;
    }
}

__global__ void __launch_bounds__(256) reg_kernel(RegArgs a)
{
    __shared__ double red[4];
    if (a.xlo != nullptr || a.xhi != nullptr)
        reg_block<true>(a, blockIdx.x, red);
    else
        reg_block<false>(a, blockIdx.x, red);
}

// Cross-gradient coupling of the joint store (Gallardo & Meju 2003): t = grad u x grad w of the two
// physical, normalised models u = mw_rho winv / s_rho, w = mw_kappa winv / s_kappa, forward differences
// over centre distances at the cells with a forward neighbour on every axis, Phi = sum |t|^2.
struct CrossGradArgs {
    int64_t m;          // cells per property
    int nz, ny, nx;
    double lambda;      // factor of the gradient (the partials of Phi are not scaled)
    double ihx, ihy;    // 1 / spacing
    const double *ihz;  // nz - 1: 1 / distance between the centres of layers k and k + 1
    const double *x;    // 2m: the stacked weighted model
    const double *sw;   // 2m: winv / s of every entry (u = x sw)
    double *g;          // 2m or null: lambda dPhi/dmw, added (ADD) or stored
    double *t;          // 3m or null: t of every cell (0 where it does not contribute)
    double *part;       // one partial of Phi per block
};

// t of cell q (layer kq; a contributing cell) and the derivatives of |t|^2 with respect to its two
// difference vectors, A = 2 (Dw x t), B = 2 (t x Du), each component already divided by its spacing
__device__ __forceinline__ void cg_cell(const CrossGradArgs &a, int64_t q, int kq, double (&t)[3], double (&A)[3],
                                        double (&B)[3])
{
    const int64_t st[3] = {1, a.nx, (int64_t)a.nx * a.ny};
    const double ih[3] = {a.ihx, a.ihy, a.ihz[kq]};
    const double *xw = a.x + a.m, *sww = a.sw + a.m;
    const double u0 = a.x[q] * a.sw[q], w0 = xw[q] * sww[q];
    double Du[3], Dw[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int64_t n = q + st[c];
        Du[c] = (a.x[n] * a.sw[n] - u0) * ih[c];
        Dw[c] = (xw[n] * sww[n] - w0) * ih[c];
    }
    t[0] = Du[1] * Dw[2] - Du[2] * Dw[1];
    t[1] = Du[2] * Dw[0] - Du[0] * Dw[2];
    t[2] = Du[0] * Dw[1] - Du[1] * Dw[0];
    A[0] = 2.0 * (Dw[1] * t[2] - Dw[2] * t[1]) * ih[0];
    A[1] = 2.0 * (Dw[2] * t[0] - Dw[0] * t[2]) * ih[1];
    A[2] = 2.0 * (Dw[0] * t[1] - Dw[1] * t[0]) * ih[2];
    B[0] = 2.0 * (t[1] * Du[2] - t[2] * Du[1]) * ih[0];
    B[1] = 2.0 * (t[2] * Du[0] - t[0] * Du[2]) * ih[1];
    B[2] = 2.0 * (t[0] * Du[1] - t[1] * Du[0]) * ih[2];
}

// Gather form, one cell per thread, both blocks in one launch: a cell's entry of the gradient collects the
// share of its own t (minus, every component) and of the t of its three backward neighbours (plus, the
// component along that axis) -- each t is evaluated again where it is needed (four times in all, from a
// model that the caches hold) instead of being stored by a launch of its own.  No atomics; the block's sum
// of |t|^2 goes to part[blockIdx.x].
template <bool ADD>
__global__ void __launch_bounds__(256) cross_gradient_kernel(CrossGradArgs a)
{
    __shared__ double red[4];
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double phi = 0.0;
    if (p < a.m) {
        const int64_t nx = a.nx, ny = a.ny, P = nx * ny;
        const int i = (int)(p % nx), j = (int)((p / nx) % ny), k = (int)(p / P);
        const bool fx = i < a.nx - 1, fy = j < a.ny - 1, fz = k < a.nz - 1;
        double gu = 0.0, gw = 0.0, t[3] = {0.0, 0.0, 0.0}, tb[3], A[3], B[3];
        if (fx && fy && fz) {
            cg_cell(a, p, k, t, A, B);
            phi = t[0] * t[0] + t[1] * t[1] + t[2] * t[2];
            gu -= A[0] + A[1] + A[2];
            gw -= B[0] + B[1] + B[2];
        }
        if (i > 0 && fy && fz) {
            cg_cell(a, p - 1, k, tb, A, B);
            gu += A[0];
            gw += B[0];
        }
        if (j > 0 && fx && fz) {
            cg_cell(a, p - nx, k, tb, A, B);
            gu += A[1];
            gw += B[1];
        }
        if (k > 0 && fx && fy) {
            cg_cell(a, p - P, k - 1, tb, A, B);
            gu += A[2];
            gw += B[2];
        }
        if (a.g) {
            const double du = a.lambda * (gu * a.sw[p]), dw = a.lambda * (gw * a.sw[a.m + p]);
            a.g[p] = ADD ? a.g[p] + du : du;
            a.g[a.m + p] = ADD ? a.g[a.m + p] + dw : dw;
        }
        if (a.t) {
            a.t[3 * p] = t[0];
            a.t[3 * p + 1] = t[1];
            a.t[3 * p + 2] = t[2];
        }
    }
    const double tot = block_allreduce_sum(phi, red, 4);
    if (threadIdx.x == 0) a.part[blockIdx.x] = tot;
}

// scal_kernel of an evaluation with a coupling term on (the joint store's cross-gradient, the magnetization-vector
// store's amplitude term): the same sums in the same order, U takes lambda Phi, and Phi (n_cgpart partials behind
// those of R) goes to a slot of its own
__global__ void __launch_bounds__(1024) scal_cg_kernel(const double *part, int n_dpart, int n_regpart, int n_cgpart,
                                                       double alpha, double lambda, double *scal, double *phi)
{
    __shared__ double red[16];
    double s2 = 0.0, sr = 0.0, sp = 0.0;
    for (int t = threadIdx.x; t < n_dpart; t += 1024) s2 += part[t];
    for (int t = threadIdx.x; t < n_regpart; t += 1024) sr += part[n_dpart + t];
    for (int t = threadIdx.x; t < n_cgpart; t += 1024) sp += part[n_dpart + n_regpart + t];
    const double ud = block_allreduce_sum(s2, red, 16);
    const double R = block_allreduce_sum(sr, red, 16);
    const double Phi = block_allreduce_sum(sp, red, 16);
    if (threadIdx.x == 0) {
        scal[0] = ud;
        scal[1] = R;
        scal[2] = (ud + alpha * R) + lambda * Phi;
        phi[0] = Phi;
    }
}

// Amplitude coupling of the magnetization-vector store (GH_CELL_PRISM_MVI): the minimum-support functional of the
// cells' amplitude, Phi = sum_c s_c / (s_c + beta), s_c = u_x^2 + u_y^2 + u_z^2 of the physical, normalised
// components u_a[c] = mw[a m + c] winv[a m + c] / scale.  It is the one term that ties the three blocks together.
struct AmpArgs {
    int64_t m;         // cells (entries per component)
    double lambda;     // factor of the gradient (the partials of Phi are not scaled)
    double beta, scale;
    const double *x;   // 3m: the stacked weighted model
    const double *sw;  // 3m: winv / scale of every entry (u = x sw)
    double *g;         // 3m or null: lambda dPhi/dmw, added (ADD) or stored
    double *amp;       // m or null: the physical amplitude scale sqrt(s_c)
    double *part;      // one partial of Phi per block
};

// One cell per thread, the three components in one launch; dPhi/du_a = 2 beta u_a / (s + beta)^2.  No atomics;
// the block's sum of Phi goes to part[blockIdx.x].
template <bool ADD>
__global__ void __launch_bounds__(256) amplitude_kernel(AmpArgs a)
{
    __shared__ double red[4];
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double phi = 0.0;
    if (p < a.m) {
        double u[3], s = 0.0;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            u[q] = a.x[q * a.m + p] * a.sw[q * a.m + p];
            s += u[q] * u[q];
        }
        const double den = s + a.beta;
        phi = s / den;
        if (a.g) {
            const double f = (2.0 * a.beta) / (den * den);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const double dq = a.lambda * ((f * u[q]) * a.sw[q * a.m + p]);
                a.g[q * a.m + p] = ADD ? a.g[q * a.m + p] + dq : dq;
            }
        }
        if (a.amp) a.amp[p] = a.scale * sqrt(s);
    }
    const double tot = block_allreduce_sum(phi, red, 4);
    if (threadIdx.x == 0) a.part[blockIdx.x] = tot;
}
// (both forms exist wherever this header is compiled, also on its own for the build's code check)
template __global__ void amplitude_kernel<true>(AmpArgs);
template __global__ void amplitude_kernel<false>(AmpArgs);

// One launch for the two independent halves of the per-step epilogue: blocks [0, n_red) sum the
// slab rows of one segment for 32 observations each (first stage of the slab reduction, same
// arithmetic as reduce_slab_kernel with nseg > 1), the remaining blocks evaluate the regulariser.
__global__ void __launch_bounds__(256)
reduce_reg_kernel(const double *slab, int n_rows_slab, int64_t ld, int nseg, int n_dpart, double *slab2,
                  RegArgs ra)
{
    __shared__ double red8[8][33];
    __shared__ double red[4];
    const int n_red = n_dpart * nseg;
    if ((int)blockIdx.x >= n_red) {
        reg_block(ra, blockIdx.x - n_red, red);
        return;
    }
    const int rx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int bx = blockIdx.x % n_dpart, seg = blockIdx.x / n_dpart;
    const int64_t i = (int64_t)bx * 32 + rx;
    const int per = (n_rows_slab + nseg - 1) / nseg;
    const int t0 = seg * per;
    const int t1 = (t0 + per < n_rows_slab) ? t0 + per : n_rows_slab;
    double acc = 0.0;
    if (i < ld) {
        // (eight rows in flight per thread, summed in the order of the plain loop)
        int t = t0 + ty;
        for (; t + 56 < t1; t += 64) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = slab[(int64_t)(t + 8 * u) * ld + i];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < 8; ++u) acc += v[u];
            __builtin_amdgcn_sched_barrier(0);
        }
        for (; t < t1; t += 8) acc += slab[(int64_t)t * ld + i];
    }
    red8[ty][rx] = acc;
    __syncthreads();
    if (ty == 0 && i < ld) {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) s += red8[q][rx];
        slab2[(int64_t)seg * ld + i] = s;
    }
}

// The whole per-step epilogue in ONE launch (N >= 2048: enough 32-observation blocks to fill the
// chip) after a sweep that also delivered the sums of its slab rows (dsum).  Because
//     sum_i d_i = sum_t sum_i slab[t][i] = sum_t dsum[t],
// every block knows mean(d + grav_fix) (potential.py:706) before the slab is reduced, so the blocks
// that reduce the slab for 32 observations each can form the residual and their share of |r|^2 at
// once; the other blocks evaluate the regulariser.  What finish_kernel -- ONE workgroup walking
// 570 KB at N = 10^4, 14 us -- did in a second launch is gone; the three scalars are summed from
// the partials by scal_kernel when somebody reads them (once per trajectory).  A last-block ticket
// inside this kernel was tried first: the agent-scope release fence every block needs costs more
// than the launch it saves (30 us).  (The mean is the same number up to the association of its
// sum; a shift delta of the mean changes |r|^2 by N delta^2 only, sum r = 0.)
//
// BLOCKS: the rows are nblk row blocks of Nb observations each (the multi-component store, N = nblk * Nb), every
// one with a mean of its own: dsum then holds nblk rows of n_dsum partial sums, block b's in row b
// (slab_block_sums_kernel), a residual subtracts the mean of the block its observation lies in, and bmean takes
// the nblk means.  |r|^2 is the sum over all blocks, so its partials stay one per 32 observations.
constexpr int MULTI_MAX = 11;  // row blocks at most: every gravity component once
struct ReduceFinishArgs {
    const double *slab;
    int n_rows_slab, n_dpart, n_regpart;
    int64_t ld, N;
    const double *dsum;      // n_dsum partial sums of d over the observations (one per slab row, or as delivered)
    int n_dsum;
    double gfix_sum;         // sum of grav_fix (0 without)
    const double *gfix, *dobs_c;
    double *d, *r, *scal;    // as FinishArgs (scal: only [3] = mean is written here)
    double *r2part;          // n_dpart (ra.regpart: the n_regpart partials of R, kept with them)
    RegArgs ra;
    int nblk;                // BLOCKS: row blocks, Nb observations each, and where their means go
    int64_t Nb;
    double *bmean;
};

// sums[b * n_rows_slab + t] = sum of slab row t over the observations of row block b: what reduce_finish_kernel
// <BLOCKS> turns into the blocks' means.  One workgroup per slab row.  (It walks its row load by load, block after
// block: 38 us per step at 256 rows of 72 KB, DESIGN 4.17 -- a workgroup per (slab row, block) with several loads in
// flight is the next step.)
__global__ void __launch_bounds__(256)
slab_block_sums_kernel(const double *__restrict__ slab, int64_t ld, int64_t Nb, int nblk, double *__restrict__ sums)
{
    __shared__ double red[4];
    const double *row = slab + (int64_t)blockIdx.x * ld;
    for (int b = 0; b < nblk; ++b) {
        double s = 0.0;
        for (int64_t i = threadIdx.x; i < Nb; i += 256) s += row[b * Nb + i];
        const double t = block_allreduce_sum(s, red, 4);
        if (threadIdx.x == 0) sums[(int64_t)b * gridDim.x + blockIdx.x] = t;
    }
}

template <bool BLOCKS>
__global__ void __launch_bounds__(256) reduce_finish_kernel(ReduceFinishArgs a)
{
    __shared__ double red8[8][33];
    __shared__ double red[4];
    const int n_red = a.n_dpart;
    if ((int)blockIdx.x >= n_red) {
        reg_block(a.ra, blockIdx.x - n_red, red);
    } else {
        // mean of d + grav_fix from the slab rows' sums, identical bits in every block
        double mean = 0.0;
        if constexpr (BLOCKS) {
            // (one mean per row block, in LDS; this thread's observation picks its own below)
            __shared__ double mean_s[MULTI_MAX];
            for (int b = 0; b < a.nblk; ++b) {
                double ds = 0.0;
                for (int t = threadIdx.x; t < a.n_dsum; t += 256) ds += a.dsum[(int64_t)b * a.n_dsum + t];
                const double mb = block_allreduce_sum(ds, red, 4) / (double)a.Nb;
                if (threadIdx.x == 0) {
                    mean_s[b] = mb;
                    if (blockIdx.x == 0) a.bmean[b] = mb;
                }
            }
            __syncthreads();
            const int64_t i = (int64_t)blockIdx.x * 32 + (threadIdx.x & 31);
            mean = mean_s[i < a.N ? i / a.Nb : 0];
        } else {
            double ds = 0.0;
            for (int t = threadIdx.x; t < a.n_dsum; t += 256) ds += a.dsum[t];
            mean = (block_allreduce_sum(ds, red, 4) + a.gfix_sum) / (double)a.N;
        }
        const int rx = threadIdx.x & 31, ty = threadIdx.x >> 5;
        const int64_t i = (int64_t)blockIdx.x * 32 + rx;
        double acc = 0.0;
        if (i < a.ld) {
            int t = ty;
            for (; t + 56 < a.n_rows_slab; t += 64) {
                double v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = a.slab[(int64_t)(t + 8 * u) * a.ld + i];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < 8; ++u) acc += v[u];
                __builtin_amdgcn_sched_barrier(0);
            }
            for (; t < a.n_rows_slab; t += 8) acc += a.slab[(int64_t)t * a.ld + i];
        }
        red8[ty][rx] = acc;
        __syncthreads();
        if (ty == 0) {
            double di = 0.0, ri = 0.0;
            if (i < a.ld) {
#pragma unroll
                for (int q = 0; q < 8; ++q) di += red8[q][rx];
                a.d[i] = di;
                if (i < a.N) {
                    const double dinv = di + (a.gfix ? a.gfix[i] : 0.0);
                    ri = (dinv - mean) - a.dobs_c[i];
                }
                a.r[i] = ri;
            }
            double r2 = ri * ri;
#pragma unroll
            for (int off = 16; off >= 1; off >>= 1) r2 += __shfl_xor(r2, off, WAVE);
            if (rx == 0) {
                a.r2part[blockIdx.x] = r2;
                if (blockIdx.x == 0) a.scal[3] = mean;  // (BLOCKS: the first block's)
            }
        }
    }
}

// The scalars of an evaluation whose epilogue ran as reduce_finish_kernel: sums of its partials in
// index order.  Launched only when the host (or the Metropolis test) is about to read them -- once
// per trajectory, not once per step.  part: n_dpart |r|^2 partials, then n_regpart of R.
__global__ void __launch_bounds__(1024) scal_kernel(const double *part, int n_dpart, int n_regpart, double alpha,
                                                    double *scal)
{
    __shared__ double red[16];
    double s2 = 0.0, sr = 0.0;
    for (int t = threadIdx.x; t < n_dpart; t += 1024) s2 += part[t];
    for (int t = threadIdx.x; t < n_regpart; t += 1024) sr += part[n_dpart + t];
    const double ud = block_allreduce_sum(s2, red, 16);
    const double R = block_allreduce_sum(sr, red, 16);
    if (threadIdx.x == 0) {
        scal[0] = ud;
        scal[1] = R;
        scal[2] = ud + alpha * R;
    }
}

struct FinishArgs {
    int64_t N, ld;
    int nseg, n_regpart;
    const double *src;  // nseg x ld partial forward products (nseg = 1: the finished d)
    const double *gfix, *dobs_c, *regpart;
    double alpha;
    double *d;     // ld: forward product d = sum of the segments
    double *r;     // ld (zero padded)
    double *scal;  // [0]=U_data [1]=R [2]=U [3]=mean(dinv)
    // a coupling term whose partials are at hand (the magnetization-vector store's amplitude term), or null:
    // U takes lambda Phi, Phi goes to phi[0]
    const double *cpart;
    int n_cpart;
    double lambda;
    double *phi;
};

// U of finish_kernel: ud + alpha R, plus lambda Phi of a coupling term summed here in sum_kernel's order
__device__ __forceinline__ double finish_total(const FinishArgs &a, double ud, double R, double *red)
{
    double U = ud + a.alpha * R;
    if (a.cpart) {
        double sp = 0.0;
        for (int t = threadIdx.x; t < a.n_cpart; t += 1024) sp += a.cpart[t];
        const double Phi = block_allreduce_sum(sp, red, 16);
        U = U + a.lambda * Phi;
        if (threadIdx.x == 0) a.phi[0] = Phi;
    }
    return U;
}

// Single block: last stage of the slab reduction, mean removal, residual, data misfit
// (potential.py:700-706) and U = U_d + alpha R.  The segment sum uses the association order of
// reduce_slab_kernel (eight strided partial sums, then their sum), so a d that went through that
// kernel first (sharded / wavelet paths, nseg = 1) and a d summed here have the same bits.
__global__ void __launch_bounds__(1024) finish_kernel(FinishArgs a)
{
    __shared__ double red[16];
    if (a.nseg == 1 && a.ld <= 16 * 1024) {
        // One segment (N > 8192: the first stage has summed everything) and at most 16 rows per
        // thread: the rows stay in registers and every pass issues its loads together.  One block
        // is one CU: a row-by-row loop pays a memory round trip per iteration (measured 16 us at
        // N = 10^4, of which the arithmetic is nothing).  Same operations in the same order as the
        // general path below.
        double dv[16], gv[16], ov[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int64_t i = threadIdx.x + 1024 * k;
            const bool in = i < a.ld, inN = i < a.N;
            dv[k] = in ? a.src[i] : 0.0;
            gv[k] = (inN && a.gfix) ? a.gfix[i] : 0.0;
            ov[k] = inN ? a.dobs_c[i] : 0.0;
        }
        __builtin_amdgcn_sched_barrier(0);
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int64_t i = threadIdx.x + 1024 * k;
            // (the general path adds seven zero partial sums to the one segment)
            double di = 0.0;
            di += 0.0 + dv[k];
#pragma unroll
            for (int q = 1; q < 8; ++q) di += 0.0;
            dv[k] = di;
            if (i < a.ld) a.d[i] = di;
            if (i < a.N) s += di + gv[k];
        }
        const double mean = block_allreduce_sum(s, red, 16) / (double)a.N;
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int64_t i = threadIdx.x + 1024 * k;
            double ri = 0.0;
            if (i < a.N) {
                const double dinv = dv[k] + gv[k];
                ri = (dinv - mean) - ov[k];
                acc += ri * ri;
            }
            if (i < a.ld) a.r[i] = ri;
        }
        const double ud = block_allreduce_sum(acc, red, 16);
        double rs = 0.0;
        for (int t = threadIdx.x; t < a.n_regpart; t += 1024) rs += a.regpart[t];
        const double R = block_allreduce_sum(rs, red, 16);
        const double U = finish_total(a, ud, R, red);
        if (threadIdx.x == 0) {
            a.scal[0] = ud;
            a.scal[1] = R;
            a.scal[2] = U;
            a.scal[3] = mean;
        }
        return;
    }
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < a.ld; i += 1024) {
        double q8[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int t = 0; t < a.nseg; t += 8) {
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (t + q < a.nseg) q8[q] += a.src[(int64_t)(t + q) * a.ld + i];
        }
        double di = 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) di += q8[q];
        a.d[i] = di;
        if (i < a.N) s += di + (a.gfix ? a.gfix[i] : 0.0);
    }
    const double mean = block_allreduce_sum(s, red, 16) / (double)a.N;
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < a.ld; i += 1024) {
        double ri = 0.0;
        if (i < a.N) {
            const double dinv = a.d[i] + (a.gfix ? a.gfix[i] : 0.0);
            ri = (dinv - mean) - a.dobs_c[i];
            acc += ri * ri;
        }
        a.r[i] = ri;
    }
    const double ud = block_allreduce_sum(acc, red, 16);
    double rs = 0.0;
    for (int t = threadIdx.x; t < a.n_regpart; t += 1024) rs += a.regpart[t];
    const double R = block_allreduce_sum(rs, red, 16);
    const double U = finish_total(a, ud, R, red);
    if (threadIdx.x == 0) {
        a.scal[0] = ud;
        a.scal[1] = R;
        a.scal[2] = U;
        a.scal[3] = mean;
    }
}

// out[0] = sum of part[0..n) in the same fixed order finish_kernel uses for its partials
__global__ void __launch_bounds__(1024) sum_kernel(const double *part, int n, double *out)
{
    __shared__ double red[16];
    double s = 0.0;
    for (int t = threadIdx.x; t < n; t += 1024) s += part[t];
    const double tot = block_allreduce_sum(s, red, 16);
    if (threadIdx.x == 0) {
        out[0] = tot;
        out[1] = 0.0;
    }
}

// Leapfrog update from a ready gradient g (row-panel path for N > 16384: the adjoint of all
// panels is accumulated first, then this elementwise pass does what sweep_kernel does per column).
__global__ void __launch_bounds__(256) vec_update_kernel(SweepArgs a, const double *g, int64_t M, int n_pp)
{
    __shared__ double red[4];
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int mode = a.mode;
    double pp = 0.0;
    if (j < M) {
        const double grad = g[j];
        if (mode & SW_PFIN) {
            const double pf = a.p_in[j] - a.c_p * grad;
            pp = pf * pf;
            if (!(mode & SW_SPEC)) a.p_out[j] = pf;
        }
        if (mode & SW_UPD) {
            const double psrc = (mode & SW_SPEC) ? a.pn_in[j] : a.p_in[j];
            double pj = psrc - a.c_u * grad;
            double xj = a.x_in[j] + a.dt * pj;
            const double hi = a.high[j], lo = a.low[j];
            if (xj > hi) {
                xj = hi;
                pj = -pj;
            } else if (xj < lo) {
                xj = lo;
                pj = -pj;
            }
            a.p_out[j] = pj;
            a.x_out[j] = xj;
        }
    }
    if (mode & SW_PFIN) {
        const double t = block_allreduce_sum(pp, red, 4);
        if (threadIdx.x == 0) a.pp_part[blockIdx.x] = t;
        // the host sums n_pp partials; a team sweep (teamsweep.hip.h) may have left its own in the
        // entries this launch does not write
        if (blockIdx.x == 0)
            for (int q = (int)gridDim.x + (int)threadIdx.x; q < n_pp; q += 256) a.pp_part[q] = 0.0;
    }
}

// ---- epilogue of an evaluation with the observations sharded over ranks (row blocks): the mean of d + grav_fix
// and |r|^2 are sums over ALL observations -- two scalar all-reduces sit between these three single-block stages
struct RowsFinishArgs {
    int64_t N, ld, N_global;
    int nseg, n_regpart;
    const double *src;      // nseg x ld partial forward products of the local rows
    const double *gfix, *dobs_c, *regpart;
    double alpha;
    double *d, *r, *scal;
    double *rbuf;           // [0] local / global sum of d + grav_fix, [1] local / global |r|^2
};

__global__ void __launch_bounds__(1024) rows_stage_a_kernel(RowsFinishArgs a)
{
    __shared__ double red[16];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < a.ld; i += 1024) {
        double di = 0.0;
        for (int q = 0; q < a.nseg; ++q) di += a.src[(int64_t)q * a.ld + i];
        a.d[i] = di;
        if (i < a.N) s += di + (a.gfix ? a.gfix[i] : 0.0);
    }
    const double t = block_allreduce_sum(s, red, 16);
    if (threadIdx.x == 0) a.rbuf[0] = t;
}

__global__ void __launch_bounds__(1024) rows_stage_b_kernel(RowsFinishArgs a)
{
    __shared__ double red[16];
    const double mean = a.rbuf[0] / (double)a.N_global;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < a.ld; i += 1024) {
        double ri = 0.0;
        if (i < a.N) {
            const double dinv = a.d[i] + (a.gfix ? a.gfix[i] : 0.0);
            ri = (dinv - mean) - a.dobs_c[i];
        }
        a.r[i] = ri;
        s += ri * ri;
    }
    const double t = block_allreduce_sum(s, red, 16);
    if (threadIdx.x == 0) {
        a.rbuf[1] = t;
        a.scal[3] = mean;
    }
}

__global__ void __launch_bounds__(1024) rows_stage_c_kernel(RowsFinishArgs a)
{
    __shared__ double red[16];
    double sr = 0.0;
    for (int t = threadIdx.x; t < a.n_regpart; t += 1024) sr += a.regpart[t];
    const double R = block_allreduce_sum(sr, red, 16);
    if (threadIdx.x == 0) {
        a.scal[0] = a.rbuf[1];
        a.scal[1] = R;
        a.scal[2] = a.rbuf[1] + a.alpha * R;
    }
}

// column norms / scaling without keeping a column in registers (any N): one workgroup per column
__global__ void __launch_bounds__(256)
colnorm_kernel(const double *G, int64_t ld, int64_t M, double wf, double *wm)
{
    __shared__ double red[4];
    for (int64_t j = blockIdx.x; j < M; j += gridDim.x) {
        const d2 *col = reinterpret_cast<const d2 *>(G + j * ld);
        double s = 0.0;
        for (int64_t e = threadIdx.x; e < (ld >> 1); e += 256) {
            const d2 v = col[e];
            s += v.x * v.x;
            s += v.y * v.y;
        }
        const double t = block_allreduce_sum(s, red, 4);
        if (threadIdx.x == 0) wm[j] = (wf == 0.5) ? sqrt(t) : pow(t, wf);
    }
}

__global__ void __launch_bounds__(256)
colscale_kernel(double *G, int64_t ld, int64_t M, const double *wm)
{
    for (int64_t j = blockIdx.x; j < M; j += gridDim.x) {
        const double w = wm[j];
        if (w == 0.0) continue;
        const double inv = 1.0 / w;
        d2 *col = reinterpret_cast<d2 *>(G + j * ld);
        for (int64_t e = threadIdx.x; e < (ld >> 1); e += 256) {
            d2 v = col[e];
            v.x *= inv;
            v.y *= inv;
            col[e] = v;
        }
    }
}

// per-block partial sums of v[j]^2
__global__ void __launch_bounds__(256) sumsq_kernel(const double *v, int64_t M, double *part)
{
    __shared__ double red[4];
    double acc = 0.0;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < M; j += (int64_t)gridDim.x * 256)
        acc += v[j] * v[j];
    const double t = block_allreduce_sum(acc, red, 4);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// ----------------------------------------------------------------- sensitivity weighting

// One team per column at a time: wm_j = (sum_i G_ij^2)^wf ; G_j *= 1/wm_j (potential.py:232-264).
template <int TW, int EPT2>
__global__ void __launch_bounds__((TW == 1 ? 4 : TW) * 64)
weight_kernel(double *G, int64_t ld, int64_t M, int64_t cols_per_team, int n_teams, double wf,
              double *wm)
{
    constexpr int TEAM_THREADS = TW * 64;
    constexpr int WG_TEAMS = (TW == 1) ? 4 : 1;
    __shared__ double red[2][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ttid = (TW == 1) ? lane : tid;
    const int team = blockIdx.x * WG_TEAMS + ((TW == 1) ? wave : 0);
    const int64_t ld2 = ld >> 1;
    int64_t j0 = (int64_t)team * cols_per_team, j1 = j0 + cols_per_team;
    if (j1 > M) j1 = M;
    if (team >= n_teams) j0 = j1 = 0;
    for (int64_t j = j0; j < j1; ++j) {
        double2 *col = reinterpret_cast<double2 *>(G + j * ld);
        double2 c[EPT2];
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < EPT2; ++k) {
            const int64_t e = (int64_t)k * TEAM_THREADS + ttid;
            c[k] = (e < ld2) ? col[e] : make_double2(0.0, 0.0);
            s += c[k].x * c[k].x;
            s += c[k].y * c[k].y;
        }
        s = wave_allreduce_sum(s);
        if (TW > 1) {
            double *rd = red[(j - j0) & 1];
            if (lane == 0) rd[wave] = s;
            __syncthreads();
            double t = 0.0;
#pragma unroll
            for (int w = 0; w < TW; ++w) t += rd[w];
            s = t;
        }
        const double w = (wf == 0.5) ? sqrt(s) : pow(s, wf);
        if (ttid == 0) wm[j] = w;
        if (w != 0.0) {
            const double inv = 1.0 / w;
#pragma unroll
            for (int k = 0; k < EPT2; ++k) {
                const int64_t e = (int64_t)k * TEAM_THREADS + ttid;
                if (e < ld2) col[e] = make_double2(c[k].x * inv, c[k].y * inv);
            }
        }
    }
}

// --------------------------------------------------------------------- kernel assembly
// Strict IEEE evaluation order (no FMA contraction) so the entries track the reference's
// Cython/C and numba/libm arithmetic as closely as the device math library allows.

__device__ __forceinline__ double safe_atan2_d(double y, double x)
{
    // _prism.pyx:16-26 (quadrant folding; the literal is the reference's)
    const double PI_LIT = 3.1415926535897931159979634685441851615906;
    if (y == 0) return 0;
    if (y > 0 && x < 0) return atan2(y, x) - PI_LIT;
    if (y < 0 && x < 0) return atan2(y, x) + PI_LIT;
    return atan2(y, x);
}

__device__ __forceinline__ double safe_log_d(double x)
{
    // _prism.pyx:28-34
    if (x == 0) return 0;
    return log(x);
}

// The 8 corners of the prism b in the order every prism field sums them (_prism.pyx's loops: k: z2, z1; then j: y2,
// y1; then i: x2, x1): f(sign, dx, dy, dz) with sign = (-1)^(i+j+k) and (dx, dy, dz) = corner - observation.
template <class F>
__device__ __forceinline__ void prism_each_corner(double px, double py, double pz, const double *b, F f)
{
#pragma clang fp contract(off)
    const double X[2] = {b[1], b[0]}, Y[2] = {b[3], b[2]}, Z[2] = {b[5], b[4]};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double dz = Z[k] - pz;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const double dy = Y[j] - py;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const double dx = X[i] - px;
                f(((i + j + k) & 1) ? -1.0 : 1.0, dx, dy, dz);
            }
        }
    }
}

// The 8-corner sum of a prism field: acc plus sign * corner(dx, dy, dz) over prism_each_corner's corners, into the one
// accumulator in that order.  The result forms fold the density or the magnetization into corner(): multiplying
// by the sign +-1 is exact, so where it happens changes no bit.  (The loop is written out: on prism_each_corner the
// compile of the whole library -- not that of the build's code check, whose code stays the same -- gives the 1024-thread
// matrix-free kernels of potential / geoid / gx / gy, which spill as they are, 8 more bytes of scratch per lane
// (mf_fused_kernel<1024, 4 / 16, 7>); this form keeps every gravity kernel's code as it was.)
template <class F>
__device__ __forceinline__ double prism_corners(double acc, double px, double py, double pz, const double *b,
                                                F corner)
{
#pragma clang fp contract(off)
    const double X[2] = {b[1], b[0]}, Y[2] = {b[3], b[2]}, Z[2] = {b[5], b[4]};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double dz = Z[k] - pz;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const double dy = Y[j] - py;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const double dx = X[i] - px;
                const double sign = ((i + j + k) & 1) ? -1.0 : 1.0;
                acc += sign * corner(dx, dy, dz);
            }
        }
    }
    return acc;
}

// The six second derivatives of 1/r at one corner (_prism.pyx:52-78: kernelxx, xy, xz, yy, yz, zz), behind the one
// distance: the magnetic fields of prisms are sums of these and of nothing else.  A caller that reads three of them
// pays for three.
struct PrismV {
    double v1, v2, v3, v4, v5, v6;
};
__device__ __forceinline__ PrismV prism_v6(double dx, double dy, double dz)
{
#pragma clang fp contract(off)
    const double r = sqrt(dx * dx + dy * dy + dz * dz);
    PrismV v;
    v.v1 = -safe_atan2_d(dz * dy, dx * r);
    v.v2 = safe_log_d(dz + r);
    v.v3 = safe_log_d(dy + r);
    v.v4 = -safe_atan2_d(dz * dx, dy * r);
    v.v5 = safe_log_d(dx + r);
    v.v6 = -safe_atan2_d(dx * dy, dz * r);
    return v;
}

// CM * T2NT of the reference (constants.py:37,41): 10**-7 * 10**6 rounds to 0.09999999999999999; entries in
// uT per A/m of magnetization along the field (T2NT is 10**6 there, not the 10**9 of an nT scale)
#define TF_SCALE (1e-7 * 1e6)

// f.(V m) at one corner, V = prism_v6 there, in the reference's order -- b = V m first, then f.b
// (_prism.pyx:80-113, prism.py:665-733), not the shorter quadratic form, which rounds differently.
__device__ __forceinline__ double prism_tf_corner(double dx, double dy, double dz, double mx, double my, double mz,
                                                  double fx, double fy, double fz)
{
#pragma clang fp contract(off)
    const PrismV v = prism_v6(dx, dy, dz);
    const double bx = v.v1 * mx + v.v2 * my + v.v3 * mz;
    const double by = v.v2 * mx + v.v4 * my + v.v5 * mz;
    const double bz = v.v3 * mx + v.v5 * my + v.v6 * mz;
    return fx * bx + fy * by + fz * bz;
}

// One (observation, prism) entry of the total-field anomaly for a unit magnetization along the field
// direction (fx, fy, fz) = dircos(inc, dec): CM*T2NT * the corner sum of f.(V f).
__device__ __forceinline__ double prism_tf_entry(double px, double py, double pz, const double *b, double fx,
                                                 double fy, double fz)
{
#pragma clang fp contract(off)
    const double acc = prism_corners(0.0, px, py, pz, b, [&](double dx, double dy, double dz) {
        return prism_tf_corner(dx, dy, dz, fx, fy, fz, fx, fy, fz);
    });
    return acc * TF_SCALE;
}

// prism.tf's `result` (prism.py:665-733): one thread per observation, the cells in mesh order, ONE sum per
// observation over every corner of every cell of (-1)^(i+j+k) f.(V m_c) with the cell's magnetization m_c =
// mag3[3c .. 3c+2], scaled once at the end -- the reference's accumulation order.
__global__ void __launch_bounds__(256)
prism_tf_result_kernel(const double *__restrict__ xp, const double *__restrict__ yp,
                       const double *__restrict__ zp, const double *__restrict__ bounds6,
                       const double *__restrict__ mag3, int64_t N, int64_t M, double fx, double fy, double fz,
                       double *__restrict__ res)
{
#pragma clang fp contract(off)
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= N) return;
    const double px = xp[l], py = yp[l], pz = zp[l];
    double acc = 0.0;
    for (int64_t c = 0; c < M; ++c) {
        const double mx = mag3[3 * c], my = mag3[3 * c + 1], mz = mag3[3 * c + 2];
        acc = prism_corners(acc, px, py, pz, bounds6 + 6 * c, [&](double dx, double dy, double dz) {
            return prism_tf_corner(dx, dy, dz, mx, my, mz, fx, fy, fz);
        });
    }
    res[l] = acc * TF_SCALE;
}

// ---- the other gravity fields of prisms (GH_CELL_PRISM_COMP)

// The components: the values of GH_COMP_* (include/gravhmc.h; gravhmc.hip checks that they agree -- this header
// also compiles on its own, for the build's code check)
enum { COMP_POTENTIAL = 0, COMP_GEOID, COMP_GX, COMP_GY, COMP_GZ, COMP_GXX, COMP_GXY, COMP_GXZ, COMP_GYY, COMP_GYZ,
       COMP_GZZ };

// The scale prism.py applies to kernel2d and result once, at the end (prism.py:151,178-179,231,314,367,...):
// products of the reference constants G, SI2MGAL, SI2EOTVOS, g0 (constants.py:26,29,34,50), rounded once
// as Python rounds them.
template <int COMP>
__device__ __forceinline__ constexpr double prism_comp_scale()
{
    return COMP == COMP_POTENTIAL ? 0.00000006673
           : COMP == COMP_GEOID   ? 0.00000006673 / 9.80
           : COMP <= COMP_GZ      ? 0.00000006673 * 100000.0
                                     : 0.00000006673 * 1000000000.0;
}

// The kernel of one component at one corner (dx, dy, dz) = corner - observation of the prism b: the distance
// and then kernelpot / x / y / z / xx ... zz (_prism.pyx:36-68) in the reference's operation order.  gxy, gxz
// and gyz take the reference's perturbed distance when the point lies on the line of an edge in front of
// the corner (_prism.pyx:346-351, 380-385, 443-448): the entry there is large but finite.
template <int COMP>
__device__ __forceinline__ double prism_comp_corner(double dx, double dy, double dz, const double *b)
{
#pragma clang fp contract(off)
    double r;
    if (COMP == COMP_GXY && dx == 0 && dy == 0 && dz < 0) {
        const double t1 = 0.00001 * (b[1] - b[0]), t2 = 0.00001 * (b[3] - b[2]);
        r = sqrt(t1 * t1 + t2 * t2 + dz * dz);
    } else if (COMP == COMP_GXZ && dx == 0 && dz == 0 && dy < 0) {
        const double t1 = 0.00001 * (b[1] - b[0]), t2 = 0.00001 * (b[5] - b[4]);
        r = sqrt(t1 * t1 + t2 * t2 + dy * dy);
    } else if (COMP == COMP_GYZ && dy == 0 && dz == 0 && dx < 0) {
        const double t1 = 0.00001 * (b[3] - b[2]), t2 = 0.00001 * (b[5] - b[4]);
        r = sqrt(t1 * t1 + t2 * t2 + dx * dx);
    } else {
        r = sqrt(dx * dx + dy * dy + dz * dz);
    }
    if (COMP == COMP_POTENTIAL || COMP == COMP_GEOID)
        return dx * dy * safe_log_d(dz + r) + dy * dz * safe_log_d(dx + r) + dx * dz * safe_log_d(dy + r) -
               0.5 * (dx * dx) * safe_atan2_d(dz * dy, dx * r) - 0.5 * (dy * dy) * safe_atan2_d(dz * dx, dy * r) -
               0.5 * (dz * dz) * safe_atan2_d(dx * dy, dz * r);
    if (COMP == COMP_GX)
        return -(dy * safe_log_d(dz + r) + dz * safe_log_d(dy + r) - dx * safe_atan2_d(dz * dy, dx * r));
    if (COMP == COMP_GY)
        return -(dz * safe_log_d(dx + r) + dx * safe_log_d(dz + r) - dy * safe_atan2_d(dx * dz, dy * r));
    if (COMP == COMP_GZ)
        return -(dx * safe_log_d(dy + r) + dy * safe_log_d(dx + r) - dz * safe_atan2_d(dx * dy, dz * r));
    if (COMP == COMP_GXX) return -safe_atan2_d(dz * dy, dx * r);
    if (COMP == COMP_GXY) return safe_log_d(dz + r);
    if (COMP == COMP_GXZ) return safe_log_d(dy + r);
    if (COMP == COMP_GYY) return -safe_atan2_d(dz * dx, dy * r);
    if (COMP == COMP_GYZ) return safe_log_d(dx + r);
    return -safe_atan2_d(dx * dy, dz * r);  // COMP_GZZ
}

// One (observation, prism) entry of a component for a density of 1: scale * the corner sum of its kernel
// (prism.py:102-662 with _prism.pyx's loops).
template <int COMP>
__device__ __forceinline__ double prism_comp_entry(double px, double py, double pz, const double *b)
{
#pragma clang fp contract(off)
    const double acc = prism_corners(0.0, px, py, pz, b, [&](double dx, double dy, double dz) {
        return prism_comp_corner<COMP>(dx, dy, dz, b);
    });
    return acc * prism_comp_scale<COMP>();
}

// The entry of a component chosen at run time (the matrix-free passes: one component per context, so the
// branch is uniform).  gz is not among them: a gz context is GH_CELL_PRISM and runs prism_comp_entry<COMP_GZ>.
// Two families, so that a pass can hold the one it runs: the tensor (one log or atan2 per corner) and the
// potential / geoid / gx / gy (six or three per corner).
__device__ __forceinline__ double prism_field_entry_rt(int comp, double px, double py, double pz, const double *b)
{
    switch (comp) {
    case COMP_POTENTIAL: return prism_comp_entry<COMP_POTENTIAL>(px, py, pz, b);
    case COMP_GEOID: return prism_comp_entry<COMP_GEOID>(px, py, pz, b);
    case COMP_GX: return prism_comp_entry<COMP_GX>(px, py, pz, b);
    default: return prism_comp_entry<COMP_GY>(px, py, pz, b);
    }
}

__device__ __forceinline__ double prism_tensor_entry_rt(int comp, double px, double py, double pz, const double *b)
{
    switch (comp) {
    case COMP_GXX: return prism_comp_entry<COMP_GXX>(px, py, pz, b);
    case COMP_GXY: return prism_comp_entry<COMP_GXY>(px, py, pz, b);
    case COMP_GXZ: return prism_comp_entry<COMP_GXZ>(px, py, pz, b);
    case COMP_GYY: return prism_comp_entry<COMP_GYY>(px, py, pz, b);
    case COMP_GYZ: return prism_comp_entry<COMP_GYZ>(px, py, pz, b);
    default: return prism_comp_entry<COMP_GZZ>(px, py, pz, b);
    }
}

__device__ __forceinline__ double prism_comp_entry_rt(int comp, double px, double py, double pz, const double *b)
{
    return comp >= COMP_GXX ? prism_tensor_entry_rt(comp, px, py, pz, b) : prism_field_entry_rt(comp, px, py, pz, b);
}

// Dense assembly of one prism field F (COMP_* or PRISM_TF, whose direction is dir): one thread per (obs, cell)
// entry, obs fastest (coalesced store), zero padding rows to ld.  One instantiation per field, so that each
// keeps its own register budget.  The launch writes ld rows of every column of a store whose columns are ldg
// rows apart: ldg == ld for a store of this field alone, ldg > ld for one row block of the multi-component
// store (GH_CELL_PRISM_MULTI: G then points at the block's first row).
constexpr int PRISM_TF = COMP_GZZ + 1;
template <int F>
__global__ void __launch_bounds__(256)
prism_kernel(const double *__restrict__ xp, const double *__restrict__ yp, const double *__restrict__ zp,
             const double *__restrict__ bounds6, int64_t N, int64_t M, int64_t ld, double3 dir,
             double *__restrict__ G, int64_t ldg)
{
    // grid-stride: a launch is limited to 2^32 work-items, ld*M reaches 5*10^9 at C2
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < ld * M;
         idx += (int64_t)gridDim.x * 256) {
        const int64_t c = idx / ld, l = idx - c * ld;
        double v = 0.0;
        if (l < N) {
            if constexpr (F == PRISM_TF)
                v = prism_tf_entry(xp[l], yp[l], zp[l], bounds6 + 6 * c, dir.x, dir.y, dir.z);
            else
                v = prism_comp_entry<F>(xp[l], yp[l], zp[l], bounds6 + 6 * c);
        }
        G[c * ldg + l] = v;
    }
}

// The row blocks of a multi-component store (GH_CELL_PRISM_MULTI): block b = rows [b * Nb, (b + 1) * Nb) of every
// column, scaled by w[b] (the data weighting Wb).
struct RowBlocks {
    int n;
    int64_t Nb;
    double w[MULTI_MAX];
};

// Wb A: every entry of row block b times w[b] (padding rows belong to no block and stay zero)
__global__ void __launch_bounds__(256) scale_rowblocks_kernel(double *__restrict__ G, int64_t ld, int64_t M, RowBlocks rb)
{
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < ld * M; idx += (int64_t)gridDim.x * 256) {
        const int64_t c = idx / ld, l = idx - c * ld;
        if (l < rb.n * rb.Nb) G[idx] *= rb.w[l / rb.Nb];
    }
}

// Joint gravity-magnetic store (GH_CELL_PRISM_JOINT): one thread per (obs, cell) pair writes both blocks of
// H = [A_gz | A_tf], the gz entry to column c and the tf entry to column m + c.  One corner loop serves both
// fields: the distance r, log(dx + r), log(dy + r) and atan2(dx dy, dz r) of a corner are the same function
// of the same operands in gz's and tf's corner (prism_comp_corner<COMP_GZ>, prism_tf_corner), so gz's corner reads
// them from prism_v6 -- v3, v5 and -v6, the negation exact -- and no bit changes; each field keeps its own
// accumulator, in prism_corners' order, and its own scale.  Every entry equals prism_kernel<COMP_GZ> /
// prism_kernel<PRISM_TF>'s bit for bit.
__global__ void __launch_bounds__(256)
prism_joint_kernel(const double *__restrict__ xp, const double *__restrict__ yp, const double *__restrict__ zp,
                   const double *__restrict__ bounds6, int64_t N, int64_t m, int64_t ld, double3 dir,
                   double *__restrict__ H)
{
#pragma clang fp contract(off)
    const double fx = dir.x, fy = dir.y, fz = dir.z;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < ld * m;
         idx += (int64_t)gridDim.x * 256) {
        const int64_t c = idx / ld, l = idx - c * ld;
        double vg = 0.0, vt = 0.0;
        if (l < N) {
            double ag = 0.0, at = 0.0;
            prism_each_corner(xp[l], yp[l], zp[l], bounds6 + 6 * c, [&](double sign, double dx, double dy, double dz) {
#pragma clang fp contract(off)
                const PrismV v = prism_v6(dx, dy, dz);
                ag += sign * -(dx * v.v3 + dy * v.v5 - dz * -v.v6);
                const double bx = v.v1 * fx + v.v2 * fy + v.v3 * fz;
                const double by = v.v2 * fx + v.v4 * fy + v.v5 * fz;
                const double bz = v.v3 * fx + v.v5 * fy + v.v6 * fz;
                at += sign * (fx * bx + fy * by + fz * bz);
            });
            vg = ag * prism_comp_scale<COMP_GZ>();
            vt = at * TF_SCALE;
        }
        H[idx] = vg;
        H[idx + ld * m] = vt;
    }
}

// Magnetization-vector store (GH_CELL_PRISM_MVI): one thread per (obs, cell) pair writes the pair's entry of all
// three blocks of A = [A_x | A_y | A_z], to columns c, m + c and 2m + c.  Block a is the total-field anomaly of
// the prisms magnetized 1 A/m along axis a: prism_tf_corner with m = e_a, where b = V e_a is column a of V
// exactly (v * 1 + v' * 0 + v'' * 0), so the entry's corner term is f . (column a of V) in the reference's order
// fx bx + fy by + fz bz.  The six second derivatives of a corner -- three atan2 and three log -- are evaluated
// ONCE and serve the three accumulators; three prism_kernel<PRISM_TF> passes would evaluate them three times.
__global__ void __launch_bounds__(256)
prism_mvi_kernel(const double *__restrict__ xp, const double *__restrict__ yp, const double *__restrict__ zp,
                 const double *__restrict__ bounds6, int64_t N, int64_t m, int64_t ld, double3 dir,
                 double *__restrict__ A)
{
#pragma clang fp contract(off)
    const double fx = dir.x, fy = dir.y, fz = dir.z;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < ld * m;
         idx += (int64_t)gridDim.x * 256) {
        const int64_t c = idx / ld, l = idx - c * ld;
        double ax = 0.0, ay = 0.0, az = 0.0;
        if (l < N) {
            prism_each_corner(xp[l], yp[l], zp[l], bounds6 + 6 * c, [&](double sign, double dx, double dy, double dz) {
#pragma clang fp contract(off)
                const PrismV v = prism_v6(dx, dy, dz);
                ax += sign * (fx * v.v1 + fy * v.v2 + fz * v.v3);
                ay += sign * (fx * v.v2 + fy * v.v4 + fz * v.v5);
                az += sign * (fx * v.v3 + fy * v.v5 + fz * v.v6);
            });
        }
        // (coalesced: consecutive threads, consecutive rows of one column, in each of the three blocks)
        A[c * ld + l] = ax * TF_SCALE;
        A[(m + c) * ld + l] = ay * TF_SCALE;
        A[(2 * m + c) * ld + l] = az * TF_SCALE;
    }
}

// ---- vector magnetic data: bx, by, bz of prisms (GH_CELL_PRISM_MVI_DATA)

// The data components: the values of GH_BCOMP_* (include/gravhmc.h; gravhmc.hip checks that they agree)
enum { BCOMP_TF = 0, BCOMP_BX, BCOMP_BY, BCOMP_BZ };
constexpr int BCOMP_MAX = 4;  // row blocks at most: every data component once
struct BComps {
    int n;
    int comp[BCOMP_MAX];
};

// Vector-data magnetization store (GH_CELL_PRISM_MVI_DATA): columns as prism_mvi_kernel's, [A_x | A_y | A_z] of m
// cells each, rows in bc.n blocks of Nb observations, block b the data component bc.comp[b].  One thread per
// (obs, cell) pair evaluates the six second derivatives v1..v6 = xx, xy, xz, yy, yz, zz of each corner ONCE and
// writes the pair's entry of every (data block, axis block).  The entry of component bx and axis a is what
// _prism.bx accumulates for that prism with (mx, my, mz) = e_a (_prism.pyx:116-142): sum of (+-)(v1 mx + v2 my +
// v3 mz) = the corner sum of v1, v2 or v3 alone (v * 1 + v' * 0 + v'' * 0 is v: every v is finite); by takes
// (v2, v4, v5), bz (v3, v5, v6).  So six sums S1..S6 serve the nine (component, axis) entries, and bx's column of
// axis y IS by's column of axis x.  A tf block is f . (column a of V) in _prism.tf's order fx bx + fy by + fz bz
// with sums of its own: bit for bit prism_mvi_kernel's entries.  All scaled once by CM * T2NT.
// Threads walk the Nb rows of a block, then the ld - n Nb padding rows below the stack, which they zero.
__global__ void __launch_bounds__(256)
prism_mvi_data_kernel(const double *__restrict__ xp, const double *__restrict__ yp, const double *__restrict__ zp,
                      const double *__restrict__ bounds6, int64_t Nb, int64_t m, int64_t ld, double3 dir, BComps bc,
                      double *__restrict__ A)
{
#pragma clang fp contract(off)
    const double fx = dir.x, fy = dir.y, fz = dir.z;
    const int64_t Lr = Nb + (ld - bc.n * Nb);
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < Lr * m; idx += (int64_t)gridDim.x * 256) {
        const int64_t c = idx / Lr, l = idx - c * Lr;
        if (l >= Nb) {
            const int64_t row = bc.n * Nb + (l - Nb);
            A[c * ld + row] = 0.0;
            A[(m + c) * ld + row] = 0.0;
            A[(2 * m + c) * ld + row] = 0.0;
            continue;
        }
        double s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0, s6 = 0.0;
        double ax = 0.0, ay = 0.0, az = 0.0;
        prism_each_corner(xp[l], yp[l], zp[l], bounds6 + 6 * c, [&](double sign, double dx, double dy, double dz) {
#pragma clang fp contract(off)
            const PrismV v = prism_v6(dx, dy, dz);
            s1 += sign * v.v1;
            s2 += sign * v.v2;
            s3 += sign * v.v3;
            s4 += sign * v.v4;
            s5 += sign * v.v5;
            s6 += sign * v.v6;
            ax += sign * (fx * v.v1 + fy * v.v2 + fz * v.v3);
            ay += sign * (fx * v.v2 + fy * v.v4 + fz * v.v5);
            az += sign * (fx * v.v3 + fy * v.v5 + fz * v.v6);
        });
        // (coalesced: consecutive threads, consecutive rows of one column, in every block)
#pragma unroll
        for (int q = 0; q < BCOMP_MAX; ++q) {
            if (q < bc.n) {
                const int comp = bc.comp[q];
                const double ex = comp == BCOMP_TF ? ax : comp == BCOMP_BX ? s1 : comp == BCOMP_BY ? s2 : s3;
                const double ey = comp == BCOMP_TF ? ay : comp == BCOMP_BX ? s2 : comp == BCOMP_BY ? s4 : s5;
                const double ez = comp == BCOMP_TF ? az : comp == BCOMP_BX ? s3 : comp == BCOMP_BY ? s5 : s6;
                const int64_t row = q * Nb + l;
                A[c * ld + row] = ex * TF_SCALE;
                A[(m + c) * ld + row] = ey * TF_SCALE;
                A[(2 * m + c) * ld + row] = ez * TF_SCALE;
            }
        }
    }
}

// prism._bx / _by / _bz's `res` (prism.py:735-870): one thread per observation, the cells in mesh order, ONE sum per
// observation over every corner of every cell of (-1)^(i+j+k) (row B of V) . m_c with the cell's magnetization m_c =
// mag3[3c .. 3c+2], scaled once at the end -- the reference's accumulation order.  Only the three derivatives of
// the component's row are read, so only they are evaluated, as _prism.bx / by / bz do.
template <int B>
__global__ void __launch_bounds__(256)
prism_b_result_kernel(const double *__restrict__ xp, const double *__restrict__ yp, const double *__restrict__ zp,
                      const double *__restrict__ bounds6, const double *__restrict__ mag3, int64_t N, int64_t M,
                      double *__restrict__ res)
{
#pragma clang fp contract(off)
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= N) return;
    const double px = xp[l], py = yp[l], pz = zp[l];
    double acc = 0.0;
    for (int64_t c = 0; c < M; ++c) {
        const double mx = mag3[3 * c], my = mag3[3 * c + 1], mz = mag3[3 * c + 2];
        acc = prism_corners(acc, px, py, pz, bounds6 + 6 * c, [&](double dx, double dy, double dz) {
#pragma clang fp contract(off)
            const PrismV v = prism_v6(dx, dy, dz);
            if constexpr (B == BCOMP_BX)
                return v.v1 * mx + v.v2 * my + v.v3 * mz;
            else if constexpr (B == BCOMP_BY)
                return v.v2 * mx + v.v4 * my + v.v5 * mz;
            else
                return v.v3 * mx + v.v5 * my + v.v6 * mz;
        });
    }
    res[l] = acc * TF_SCALE;
}

// Two-pass population standard deviation of the two unweighted blocks of a joint store (numpy.std, ddof 0):
// pass 0 sums the entries, pass 1 the squares of their distances to mean[blk].  blockIdx.y = block; every
// thread keeps a compensated (Kahan) sum over its grid-stride share, the workgroup sums its 256 threads and
// writes part[blk * gridDim.x + blockIdx.x] (the host sums the partials).  Padding rows (l >= N) are skipped.
__global__ void __launch_bounds__(256)
joint_std_kernel(const double *__restrict__ H, int64_t N, int64_t m, int64_t ld, int pass,
                 const double *__restrict__ mean, double *__restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ double red[4];
    const int blk = blockIdx.y;
    const double *B = H + (int64_t)blk * ld * m;
    const double mu = pass ? mean[blk] : 0.0;
    double s = 0.0, comp = 0.0;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < ld * m; idx += (int64_t)gridDim.x * 256) {
        const int64_t c = idx / ld, l = idx - c * ld;
        if (l >= N) continue;
        double v = B[idx];
        if (pass) {
            v -= mu;
            v = v * v;
        }
        const double y = v - comp;
        const double t = s + y;
        comp = (t - s) - y;
        s = t;
    }
    const double tot = block_allreduce_sum(s, red, 4);
    if (threadIdx.x == 0) part[(int64_t)blk * gridDim.x + blockIdx.x] = tot;
}

// Columns [j0, j0 + n) of a column-major ld-row matrix times s (the balance of the joint store's tf block)
__global__ void __launch_bounds__(256)
scale_cols_kernel(double *__restrict__ H, int64_t ld, int64_t j0, int64_t n, double s)
{
    double *B = H + j0 * ld;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < ld * n; idx += (int64_t)gridDim.x * 256)
        B[idx] *= s;
}

template <int COMP>
__device__ __forceinline__ double prism_comp_result_one(double px, double py, double pz,
                                                        const double *__restrict__ bounds6,
                                                        const double *__restrict__ dens, int64_t M)
{
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int64_t c = 0; c < M; ++c) {
        const double *b = bounds6 + 6 * c;
        const double d = dens[c];
        acc = prism_corners(acc, px, py, pz, b, [&](double dx, double dy, double dz) {
            return prism_comp_corner<COMP>(dx, dy, dz, b) * d;
        });
    }
    return acc * prism_comp_scale<COMP>();
}

// prism.<component>'s `result` (prism.py:102-662): one thread per observation, ONE sum per observation of
// ((-1)^(i+j+k) kernel) * density over every corner of every cell in mesh order, scaled once at the end --
// the reference's accumulation order.  The component is uniform over the launch.
__global__ void __launch_bounds__(256)
prism_comp_result_kernel(const double *__restrict__ xp, const double *__restrict__ yp,
                         const double *__restrict__ zp, const double *__restrict__ bounds6,
                         const double *__restrict__ dens, int64_t N, int64_t M, int comp, double *__restrict__ res)
{
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= N) return;
    const double px = xp[l], py = yp[l], pz = zp[l];
    double v;
    switch (comp) {
    case COMP_POTENTIAL: v = prism_comp_result_one<COMP_POTENTIAL>(px, py, pz, bounds6, dens, M); break;
    case COMP_GEOID: v = prism_comp_result_one<COMP_GEOID>(px, py, pz, bounds6, dens, M); break;
    case COMP_GX: v = prism_comp_result_one<COMP_GX>(px, py, pz, bounds6, dens, M); break;
    case COMP_GY: v = prism_comp_result_one<COMP_GY>(px, py, pz, bounds6, dens, M); break;
    case COMP_GZ: v = prism_comp_result_one<COMP_GZ>(px, py, pz, bounds6, dens, M); break;
    case COMP_GXX: v = prism_comp_result_one<COMP_GXX>(px, py, pz, bounds6, dens, M); break;
    case COMP_GXY: v = prism_comp_result_one<COMP_GXY>(px, py, pz, bounds6, dens, M); break;
    case COMP_GXZ: v = prism_comp_result_one<COMP_GXZ>(px, py, pz, bounds6, dens, M); break;
    case COMP_GYY: v = prism_comp_result_one<COMP_GYY>(px, py, pz, bounds6, dens, M); break;
    case COMP_GYZ: v = prism_comp_result_one<COMP_GYZ>(px, py, pz, bounds6, dens, M); break;
    default: v = prism_comp_result_one<COMP_GZZ>(px, py, pz, bounds6, dens, M); break;
    }
    res[l] = v;
}

constexpr int TESS_STACK = 100;  // tesseroid.py:79

struct TessStats {
    unsigned long long leaves;
    int overflow;
};

// obs (lon, lat, height) -> (lon rad, sin lat, cos lat, R + h)   (tesseroid.py:109-123)
__global__ void tess_convert_kernel(const double *lon, const double *lat, const double *h,
                                    int64_t N, double *lon_r, double *sinlat, double *coslat,
                                    double *radius, double *sinlon = nullptr, double *coslon = nullptr)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const double d2r = 3.14159265358979323846 / 180;
    lon_r[i] = lon[i] * d2r;
    const double la = lat[i] * d2r;
    sinlat[i] = sin(la);
    coslat[i] = cos(la);
    radius[i] = 6378137.0 + h[i];
    if (sinlon) {
        sinlon[i] = sin(lon_r[i]);
        coslon[i] = cos(lon_r[i]);
    }
}

// ---- the other gravity fields of tesseroids (GH_CELL_TESSEROID_COMP)

// The GLQ leaf of one field at one sub-tesseroid (_tesseroid_numba.py:161-332: kernelV, kernelx, kernely,
// kernelz, kernelxx ... kernelzz), unscaled, in the reference's operation order.  The potential's leaf serves the
// geoid as well.  l_sqr**1.5 is l*sqrt(l), and l_sqr**2.5 is (l*l)*sqrt(l):
// neither is bitwise Python's pow(), both are within a few ulp of it per node.  kernelxy,
// kernelyy and kernelyz take cos / sin(lonc - lon), the others cos(lon - lonc), as the reference does.
template <int LEAF>
__device__ __forceinline__ double tess_comp_leaf(double lon, double sinlat, double coslat, double radius,
                                                 const double (&lonc)[2], const double (&sinlatc)[2],
                                                 const double (&coslatc)[2], const double (&rc)[2])
{
#pragma clang fp contract(off)
    const double r_sqr = radius * radius;
    double result = 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        constexpr bool flip = LEAF == COMP_GXY || LEAF == COMP_GYY || LEAF == COMP_GYZ;
        const double coslon = flip ? cos(lonc[i] - lon) : cos(lon - lonc[i]);
        const double sinlon = (LEAF == COMP_GY || flip) ? sin(lonc[i] - lon) : 0.0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const double kphi = coslat * sinlatc[j] - sinlat * coslatc[j] * coslon;
            const double cospsi = sinlat * sinlatc[j] + coslat * coslatc[j] * coslon;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const double rc_sqr = rc[k] * rc[k];
                const double l_sqr = r_sqr + rc_sqr - 2 * radius * rc[k] * cospsi;
                const double kappa = rc_sqr * coslatc[j];
                const double sl = sqrt(l_sqr);
                if (LEAF == COMP_POTENTIAL) {
                    result += kappa / sl;
                } else if (LEAF == COMP_GX) {
                    result += kappa * rc[k] * kphi / (l_sqr * sl);
                } else if (LEAF == COMP_GY) {
                    result += kappa * (rc[k] * coslatc[j] * sinlon / (l_sqr * sl));
                } else if (LEAF == COMP_GZ) {
                    result += kappa * (rc[k] * cospsi - radius) / (l_sqr * sl);
                } else if (LEAF == COMP_GXX) {
                    const double t = rc[k] * kphi;
                    result += kappa * (3 * (t * t) - l_sqr) / ((l_sqr * l_sqr) * sl);
                } else if (LEAF == COMP_GXY) {
                    result += kappa * 3 * rc_sqr * kphi * coslatc[j] * sinlon / ((l_sqr * l_sqr) * sl);
                } else if (LEAF == COMP_GXZ) {
                    result += kappa * 3 * rc[k] * kphi * (rc[k] * cospsi - radius) / ((l_sqr * l_sqr) * sl);
                } else if (LEAF == COMP_GYY) {
                    const double deltay = rc[k] * coslatc[j] * sinlon;
                    result += kappa * (3 * (deltay * deltay) - l_sqr) / ((l_sqr * l_sqr) * sl);
                } else if (LEAF == COMP_GYZ) {
                    const double deltay = rc[k] * coslatc[j] * sinlon;
                    const double deltaz = rc[k] * cospsi - radius;
                    result += kappa * 3. * deltay * deltaz / ((l_sqr * l_sqr) * sl);
                } else {  // COMP_GZZ
                    const double deltaz = rc[k] * cospsi - radius;
                    result += kappa * (3 * (deltaz * deltaz) - l_sqr) / ((l_sqr * l_sqr) * sl);
                }
            }
        }
    }
    if (LEAF == COMP_GZ) result *= -1;
    return result;
}

// The leaf of a field chosen at run time (the matrix-free passes: one field per context, a uniform branch)
__device__ __forceinline__ double tess_comp_leaf_rt(int comp, double lon, double sinlat, double coslat, double radius,
                                                    const double (&lonc)[2], const double (&sinlatc)[2],
                                                    const double (&coslatc)[2], const double (&rc)[2])
{
    switch (comp) {
    case COMP_POTENTIAL:
    case COMP_GEOID: return tess_comp_leaf<COMP_POTENTIAL>(lon, sinlat, coslat, radius, lonc, sinlatc, coslatc, rc);
    case COMP_GX: return tess_comp_leaf<COMP_GX>(lon, sinlat, coslat, radius, lonc, sinlatc, coslatc, rc);
    case COMP_GY: return tess_comp_leaf<COMP_GY>(lon, sinlat, coslat, radius, lonc, sinlatc, coslatc, rc);
    case COMP_GZ: return tess_comp_leaf<COMP_GZ>(lon, sinlat, coslat, radius, lonc, sinlatc, coslatc, rc);
    case COMP_GXX: return tess_comp_leaf<COMP_GXX>(lon, sinlat, coslat, radius, lonc, sinlatc, coslatc, rc);
    case COMP_GXY: return tess_comp_leaf<COMP_GXY>(lon, sinlat, coslat, radius, lonc, sinlatc, coslatc, rc);
    case COMP_GXZ: return tess_comp_leaf<COMP_GXZ>(lon, sinlat, coslat, radius, lonc, sinlatc, coslatc, rc);
    case COMP_GYY: return tess_comp_leaf<COMP_GYY>(lon, sinlat, coslat, radius, lonc, sinlatc, coslatc, rc);
    case COMP_GYZ: return tess_comp_leaf<COMP_GYZ>(lon, sinlat, coslat, radius, lonc, sinlatc, coslatc, rc);
    default: return tess_comp_leaf<COMP_GZZ>(lon, sinlat, coslat, radius, lonc, sinlatc, coslatc, rc);
    }
}

// The scale tesseroid.py applies to kernel2d and result once, after the sum (tesseroid.py:324-508): G for
// the potential, G/g0 (the product formed first) for the geoid, SI2MGAL then G for gx, SI2MGAL then Gs for
// gy -- the reference's spherical constant, 1000 times smaller than G (constants.py:32) -- SI2MGAL then G for
// gz, and SI2EOTVOS then G for the tensor.
__device__ __forceinline__ double tess_comp_scale(int comp, double acc)
{
#pragma clang fp contract(off)
    switch (comp) {
    case COMP_POTENTIAL: return acc * 0.00000006673;
    case COMP_GEOID: return acc * (0.00000006673 / 9.80);
    case COMP_GX:
    case COMP_GZ: return acc * 100000.0 * 0.00000006673;
    case COMP_GY: return acc * 100000.0 * 0.00000000006673;
    default: return acc * 1000000000.0 * 0.00000006673;
    }
}

// The reference's adaptive subdivision of one (observation, tesseroid) pair (_tesseroid_numba.py:32-71, 75-157:
// distance_size, divisions, split, scale_nodes) with a private 100-entry LIFO stack of sub-tesseroids -- written
// here ONCE, for every field of tesseroids.  A sub-tesseroid that is not split is a leaf: leaf(lonc, sinlatc, coslatc,
// rc, scale) gets its 2x2x2 Gauss-Legendre nodes and its weight and adds what the field sums.  error_code
// accumulates the engine's error codes (non-zero => the reference warns), nleaf counts the leaves, overflow flags
// a full stack.
template <class Leaf>
__device__ __forceinline__ void tess_traverse(double lon, double sinlat, double coslat, double radius,
                                              const double *bounds, double ratio, int &error_code,
                                              unsigned long long &nleaf, bool &overflow, Leaf leaf)
{
#pragma clang fp contract(off)
    const double MEAN_R = 6378137.0;
    const double d2r = 3.14159265358979323846 / 180;
    const double node[2] = {-0.577350269189625731058868041146, 0.577350269189625731058868041146};
    double stack[TESS_STACK][6];
#pragma unroll
    for (int q = 0; q < 6; ++q) stack[0][q] = bounds[q];
    int stktop = 0;
    while (stktop >= 0) {
        const double w = stack[stktop][0], e = stack[stktop][1], s = stack[stktop][2],
                     n = stack[stktop][3], top = stack[stktop][4], bottom = stack[stktop][5];
        stktop -= 1;
        // distance_size
        const double rt = 0.5 * (top + bottom) + MEAN_R;
        const double lont = d2r * 0.5 * (w + e);
        const double latt = d2r * 0.5 * (s + n);
        const double sinlatt = sin(latt), coslatt = cos(latt);
        const double cospsi0 = sinlat * sinlatt + coslat * coslatt * cos(lon - lont);
        const double distance = sqrt(radius * radius + rt * rt - 2 * radius * rt * cospsi0);
        const double rtop = top + MEAN_R;
        const double Llon = rtop * acos(sinlatt * sinlatt + (coslatt * coslatt) * cos(d2r * (e - w)));
        const double Llat =
            rtop * acos(sin(d2r * n) * sin(d2r * s) + cos(d2r * n) * cos(d2r * s));
        const double Lr = top - bottom;
        // divisions
        int nlon = 1, nlat = 1, nr = 1, err = 0;
        if (distance <= ratio * Llon) {
            if (Llon <= 0.1) err = -1; else nlon = 2;
        }
        if (distance <= ratio * Llat) {
            if (Llat <= 0.1) err = -1; else nlat = 2;
        }
        if (distance <= ratio * Lr) {
            if (Lr <= 1e3) err = -1; else nr = 2;
        }
        error_code += err;
        const int new_cells = nlon * nlat * nr;
        if (new_cells > 1) {
            if (new_cells + (stktop + 1) > TESS_STACK) {
                overflow = true;
                break;
            }
            const double dlon = (e - w) / nlon, dlat = (n - s) / nlat, dr = (top - bottom) / nr;
            for (int i = 0; i < nlon; ++i)
                for (int j = 0; j < nlat; ++j)
                    for (int k = 0; k < nr; ++k) {
                        stktop += 1;
                        stack[stktop][0] = w + i * dlon;
                        stack[stktop][1] = w + (i + 1) * dlon;
                        stack[stktop][2] = s + j * dlat;
                        stack[stktop][3] = s + (j + 1) * dlat;
                        stack[stktop][4] = bottom + (k + 1) * dr;
                        stack[stktop][5] = bottom + k * dr;
                    }
        } else {
            // scale_nodes
            double lonc[2], sinlatc[2], coslatc[2], rc[2];
            const double dlon = d2r * (e - w), dlat = d2r * (n - s), dr = top - bottom;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                lonc[i] = 0.5 * dlon * node[i] + d2r * 0.5 * (e + w);
                const double latc = 0.5 * dlat * node[i] + d2r * 0.5 * (n + s);
                sinlatc[i] = sin(latc);
                coslatc[i] = cos(latc);
                rc[i] = (0.5 * dr * node[i] + 0.5 * (top + bottom) + MEAN_R);
            }
            leaf(lonc, sinlatc, coslatc, rc, dlon * dlat * dr * 0.125);
            nleaf += 1;
        }
    }
}

// One (observation, tesseroid) entry of a field, unscaled: tess_traverse with the field's GLQ leaf
// (_tesseroid_numba.py:207-222), every leaf times its weight into one sum.  LEAF < 0: the leaf of `comp`, chosen at
// run time.
template <int LEAF>
__device__ double tess_comp_entry(int comp, double lon, double sinlat, double coslat, double radius,
                                  const double *bounds, double ratio, int &error_code, unsigned long long &nleaf,
                                  bool &overflow)
{
#pragma clang fp contract(off)
    double acc = 0.0;
    tess_traverse(lon, sinlat, coslat, radius, bounds, ratio, error_code, nleaf, overflow,
                  [&](const double (&lonc)[2], const double (&sinlatc)[2], const double (&coslatc)[2],
                      const double (&rc)[2], double scale) {
#pragma clang fp contract(off)
                      const double k = LEAF >= 0 ? tess_comp_leaf<(LEAF >= 0 ? LEAF : 0)>(lon, sinlat, coslat, radius, lonc,
                                                                                           sinlatc, coslatc, rc)
                                                 : tess_comp_leaf_rt(comp, lon, sinlat, coslat, radius, lonc, sinlatc,
                                                                     coslatc, rc);
                      acc += scale * k;
                  });
    return acc;
}

// What a tesseroid pass reports besides its entries: the overflow flag, and one atomic per wave for the leaf count
__device__ __forceinline__ void tess_report(unsigned long long nleaf, bool overflow, TessStats *stats)
{
    if (overflow) atomicExch(&stats->overflow, 1);
    unsigned long long tot = nleaf;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) tot += __shfl_xor(tot, off, WAVE);
    if ((threadIdx.x & 63) == 0) atomicAdd(&stats->leaves, tot);
}

// Dense assembly of one field, one thread per (obs, cell) pair, obs fastest, into `rows` rows of every column of a
// store of leading dimension ld (from G on): the first N of them the observations' entries, the rest zero; the error
// codes summed per cell into err_cell, the leaf count and the overflow flag into stats.  One instantiation
// per leaf: the leaf fixes the scale, except the potential's, which serves the geoid too (`comp` picks its
// scale).  G == nullptr: the statistics only (the matrix-free build, which stores no entry).
template <int LEAF>
__global__ void __launch_bounds__(64)
tess_comp_kernel(const double *__restrict__ lon_r, const double *__restrict__ sinlat_a,
                 const double *__restrict__ coslat_a, const double *__restrict__ radius_a,
                 const double *__restrict__ bounds6, int64_t N, int64_t M, int64_t rows, int64_t ld, double ratio, int comp,
                 double *__restrict__ G, int *__restrict__ err_cell, TessStats *stats)
{
    unsigned long long nleaf = 0;
    bool overflow = false;
    for (int64_t idx = (int64_t)blockIdx.x * 64 + threadIdx.x; idx < rows * M;
         idx += (int64_t)gridDim.x * 64) {
        const int64_t c = idx / rows, l = idx - c * rows;
        if (l >= N) {
            if (G) G[c * ld + l] = 0.0;
            continue;
        }
        int error_code = 0;
        const double v = tess_comp_entry<LEAF>(comp, lon_r[l], sinlat_a[l], coslat_a[l], radius_a[l], bounds6 + 6 * c,
                                               ratio, error_code, nleaf, overflow);
        if (G) G[c * ld + l] = tess_comp_scale(LEAF == COMP_POTENTIAL ? comp : LEAF, v);
        if (error_code != 0) atomicAdd(&err_cell[c], error_code);
    }
    tess_report(nleaf, overflow, stats);
}

// The row blocks of the tesseroid multi-component store (GH_CELL_TESSEROID_MULTI): field, ratio and data weight
struct TessBlocks {
    int n;
    int comp[MULTI_MAX];
    double ratio[MULTI_MAX];
    double w[MULTI_MAX];
};

// The shift-invariant table of the tesseroid multi-component store: rows (class, shift) of every cell row of
// longitude index 0, tess_comp_kernel's layout (ld rows per column, zero behind the first N).  The class is (block,
// latitude, height): row l belongs to block l / rows_per_block, and its entry is that block's field at that block's
// ratio, scaled as gh_set_cells_tess scales it, times the block's data weight.  The leaf is chosen at run time
// (tess_comp_entry<-1>: the same leaf functions in the same order as the dense store's instantiations).
__global__ void __launch_bounds__(64)
tess_multi_table_kernel(const double *__restrict__ lon_r, const double *__restrict__ sinlat_a,
                        const double *__restrict__ coslat_a, const double *__restrict__ radius_a,
                        const double *__restrict__ bounds6, int64_t N, int64_t M, int64_t ld, int64_t rows_per_block,
                        TessBlocks tb, double *__restrict__ T, int *__restrict__ err_cell, TessStats *stats)
{
    unsigned long long nleaf = 0;
    bool overflow = false;
    for (int64_t idx = (int64_t)blockIdx.x * 64 + threadIdx.x; idx < ld * M;
         idx += (int64_t)gridDim.x * 64) {
        const int64_t c = idx / ld, l = idx - c * ld;
        if (l >= N) {
            T[idx] = 0.0;
            continue;
        }
        const int b = (int)(l / rows_per_block);
        const int comp = tb.comp[b];
        int error_code = 0;
        const double v = tess_comp_entry<-1>(comp, lon_r[l], sinlat_a[l], coslat_a[l], radius_a[l], bounds6 + 6 * c,
                                             tb.ratio[b], error_code, nleaf, overflow);
        T[idx] = tess_comp_scale(comp, v) * tb.w[b];
        if (error_code != 0) atomicAdd(&err_cell[c], error_code);
    }
    tess_report(nleaf, overflow, stats);
}

// ------------------------------------------------------------- wavelet-compressed forward
// db4 / 'periodization' analysis step along one axis of a batch of 3-D tensors, the transform
// PyWavelets applies for gravmag/compressor3D.py:34,60 and compressor1D.py:32,54 (wavedecn /
// wavedec, level 2).  An odd length n is first extended by repeating the last sample
// (n' = n + 1) and the signal is treated as n'-periodic:
//     out[o] = sum_j f[j] * x[(4 + 2 o - j) mod n'],  o = 0 .. n'/2 - 1
// (f = dec_lo -> approximation, dec_hi -> detail).  Pinned only by the reference's logged
// wavelet-run misfits (7 digits): PyWavelets is not vendored with the reference.

__constant__ double DB4_LO[8] = {-0.010597401785069032, 0.0328830116668852, 0.030841381835560764,
                                 -0.18703481171909309, -0.027983769416859854, 0.6308807679298589,
                                 0.7148465705529157, 0.2303778133088965};
__constant__ double DB4_HI[8] = {-0.2303778133088965, 0.7148465705529157, -0.6308807679298589,
                                 -0.027983769416859854, 0.18703481171909309, 0.030841381835560764,
                                 -0.0328830116668852, -0.010597401785069032};

struct DwtArgs {
    const double *in;
    double *out;
    int64_t batch;
    int64_t in_bstride, out_bstride;  // elements between consecutive batch items
    int e[3];                         // extents of the input block (axis 0 slowest)
    int64_t in_s[3], out_s[3];        // element strides of the three axes
    int64_t in_off[3][2];             // the block may be split in two pieces along each axis
    int in_split[3];                  //   (a | d halves of an earlier pass): index >= split
                                      //   lives at in_off[ax][1] + (index - split)
    int axis;                         // axis being transformed
    int64_t out_off[3][2];            // same piece layout for the output; along `axis` piece 0
    int out_split[3];                 //   receives the approximation, piece 1 the detail
};

__device__ __forceinline__ int64_t piece_pos(int idx, int split, const int64_t off[2])
{
    return idx < split ? off[0] + idx : off[1] + (idx - split);
}

__global__ void __launch_bounds__(256) dwt_axis_kernel(DwtArgs a)
{
    const int ax = a.axis;
    const int n = a.e[ax];
    const int np = n + (n & 1);
    const int half = np >> 1;
    int oe[3] = {a.e[0], a.e[1], a.e[2]};
    oe[ax] = half;
    const int64_t per = (int64_t)oe[0] * oe[1] * oe[2];
    const int64_t total = per * a.batch;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total;
         t += (int64_t)gridDim.x * 256) {
        const int64_t b = t / per;
        int64_t q = t - b * per;
        int i[3];
        i[2] = (int)(q % oe[2]);
        q /= oe[2];
        i[1] = (int)(q % oe[1]);
        i[0] = (int)(q / oe[1]);
        int64_t ibase = b * a.in_bstride, obase = b * a.out_bstride;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            if (d == ax) continue;
            ibase += piece_pos(i[d], a.in_split[d], a.in_off[d]) * a.in_s[d];
            obase += piece_pos(i[d], a.out_split[d], a.out_off[d]) * a.out_s[d];
        }
        const int o = i[ax];
        double lo = 0.0, hi = 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            int k = (4 + 2 * o - j) % np;
            if (k < 0) k += np;
            if (k >= n) k = n - 1;  // the repeated last sample of an odd-length signal
            const double v = a.in[ibase + piece_pos(k, a.in_split[ax], a.in_off[ax]) * a.in_s[ax]];
            lo += DB4_LO[j] * v;
            hi += DB4_HI[j] * v;
        }
        a.out[obase + (a.out_off[ax][0] + o) * a.out_s[ax]] = lo;
        a.out[obase + (a.out_off[ax][1] + o) * a.out_s[ax]] = hi;
    }
}

// The whole multi-level transform of ONE model vector in one launch of one workgroup: the working
// block lives in LDS, every pass reads it, keeps its outputs in registers across a barrier and
// writes them back in place (intermediate passes: dense block; the last pass of a level: the packed
// coefficient vector in global memory, plus the approximation block back to LDS for the next
// level).  Replaces levels x axes launches of dwt_axis_kernel (and the memset of the coefficient
// vector: the gaps odd lengths leave in the packing are zeroed once) per potential evaluation of a
// compressed problem too large for the resident chain kernel (the reference's ratiogrid example).
// Same taps, same index arithmetic, same order of the eight products as dwt_axis_kernel.
constexpr int DWT_LDS_THREADS = 1024;
constexpr int DWT_LDS_NP = 10;      // (lo, hi) pairs a thread holds per pass: blocks <= 20480 doubles
constexpr int DWT_LDS_MAXPASS = 12;

struct DwtLdsPass {
    int e[3];          // extents of the input block (dense in LDS)
    int axis, last;
    int split[3];      // last pass: first index of the detail piece per axis (INT_MAX: untransformed)
    int64_t off1[3];   // last pass: packed offset of the detail piece per axis
};

struct DwtLdsPlan {
    int npass;
    int64_t M;         // model length = volume of pass 0's block
    int64_t Cs[3];     // strides of the packed coefficient cube
    DwtLdsPass p[DWT_LDS_MAXPASS];
};

__global__ void __launch_bounds__(DWT_LDS_THREADS)
dwt_lds_kernel(DwtLdsPlan plan, const double *__restrict__ x, double *__restrict__ coeff)
{
    extern __shared__ __attribute__((aligned(16))) double blk[];
    const int tid = threadIdx.x;
    for (int64_t i = tid; i < plan.M; i += DWT_LDS_THREADS) blk[i] = x[i];
    __syncthreads();
    for (int pi = 0; pi < plan.npass; ++pi) {
        const DwtLdsPass &P = plan.p[pi];
        const int ax = P.axis;
        const int n = P.e[ax], np = n + (n & 1), half = np >> 1;
        int oe[3] = {P.e[0], P.e[1], P.e[2]};
        oe[ax] = half;
        const int per = oe[0] * oe[1] * oe[2];
        const int is[3] = {P.e[1] * P.e[2], P.e[2], 1};
        double lo[DWT_LDS_NP], hi[DWT_LDS_NP];
#pragma unroll
        for (int q = 0; q < DWT_LDS_NP; ++q) {
            const int t = tid + q * DWT_LDS_THREADS;
            lo[q] = hi[q] = 0.0;
            if (t < per) {
                int r = t, i[3];
                i[2] = r % oe[2];
                r /= oe[2];
                i[1] = r % oe[1];
                i[0] = r / oe[1];
                const int o = i[ax];
                int base = 0;
#pragma unroll
                for (int d = 0; d < 3; ++d)
                    if (d != ax) base += i[d] * is[d];
                double l = 0.0, h = 0.0;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    int k = (4 + 2 * o - j) % np;
                    if (k < 0) k += np;
                    if (k >= n) k = n - 1;  // the repeated last sample of an odd-length signal
                    const double v = blk[base + k * is[ax]];
                    l += DB4_LO[j] * v;
                    h += DB4_HI[j] * v;
                }
                lo[q] = l;
                hi[q] = h;
            }
        }
        __syncthreads();  // every read of this pass is done: the block may be overwritten
        int de[3] = {P.e[0], P.e[1], P.e[2]};   // dense output block (intermediate pass)
        de[ax] = 2 * half;
        int ae[3];                               // approximation block the next level reads (last pass)
#pragma unroll
        for (int d = 0; d < 3; ++d) ae[d] = (P.split[d] == 0x7fffffff) ? P.e[d] : P.split[d];
        ae[ax] = half;
#pragma unroll
        for (int q = 0; q < DWT_LDS_NP; ++q) {
            const int t = tid + q * DWT_LDS_THREADS;
            if (t < per) {
                int r = t, i[3];
                i[2] = r % oe[2];
                r /= oe[2];
                i[1] = r % oe[1];
                i[0] = r / oe[1];
                const int o = i[ax];
                if (!P.last) {
                    const int os[3] = {de[1] * de[2], de[2], 1};
                    int base = 0;
#pragma unroll
                    for (int d = 0; d < 3; ++d)
                        if (d != ax) base += i[d] * os[d];
                    blk[base + o * os[ax]] = lo[q];
                    blk[base + (half + o) * os[ax]] = hi[q];
                } else {
                    int64_t ob = 0;
                    bool approx = true;
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        if (d == ax) continue;
                        const int64_t pos = i[d] < P.split[d] ? (int64_t)i[d] : P.off1[d] + (i[d] - P.split[d]);
                        ob += pos * plan.Cs[d];
                        approx = approx && i[d] < P.split[d];
                    }
                    coeff[ob + (int64_t)o * plan.Cs[ax]] = lo[q];
                    coeff[ob + (P.off1[ax] + o) * plan.Cs[ax]] = hi[q];
                    if (approx) {
                        const int as[3] = {ae[1] * ae[2], ae[2], 1};
                        int base = 0;
#pragma unroll
                        for (int d = 0; d < 3; ++d) base += (d == ax ? o : i[d]) * as[d];
                        blk[base] = lo[q];
                    }
                }
            }
        }
        __syncthreads();
    }
}

// rows [i0, i0+nrows) of the column-major G as a dense row-major block out[nrows][M]
__global__ void __launch_bounds__(256)
gather_rows_kernel(const double *G, int64_t ld, int64_t M, int64_t i0, int64_t nrows, double *out)
{
    __shared__ double tile[32][33];
    // 32 x 32 tiles: coalesced read along i (column-major), coalesced write along j
    const int64_t jt = (int64_t)blockIdx.x * 32, it = (int64_t)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    for (int r = ty; r < 32; r += 8) {
        const int64_t j = jt + r, i = it + tx;
        tile[r][tx] = (j < M && i < nrows) ? G[j * ld + i0 + i] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int64_t i = it + r, j = jt + tx;
        if (i < nrows && j < M) out[i * M + j] = tile[tx][r];
    }
}

// number of coefficients of each row that survive the hard threshold (compressor3D.py:36)
__global__ void __launch_bounds__(256)
csr_count_kernel(const double *C, int64_t ncols, double thr, int *count)
{
    __shared__ double red[4];
    const double *row = C + (int64_t)blockIdx.x * ncols;
    double n = 0.0;
    for (int64_t k = threadIdx.x; k < ncols; k += 256) {
        const double v = row[k];
        n += (fabs(v) >= thr && v != 0.0) ? 1.0 : 0.0;
    }
    const double t = block_allreduce_sum(n, red, 4);
    if (threadIdx.x == 0) count[blockIdx.x] = (int)t;
}

// ordered compaction of one row into CSR (column indices ascending, like scipy's csr_matrix)
__global__ void __launch_bounds__(256)
csr_fill_kernel(const double *C, int64_t ncols, double thr, const int64_t *indptr, int64_t row0,
                int *indices, double *data)
{
    __shared__ int wsum[4];
    __shared__ int base_s;
    const double *row = C + (int64_t)blockIdx.x * ncols;
    int64_t base = indptr[row0 + blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t k0 = 0; k0 < ncols; k0 += 256) {
        const int64_t k = k0 + threadIdx.x;
        const double v = (k < ncols) ? row[k] : 0.0;
        const bool keep = (k < ncols) && fabs(v) >= thr && v != 0.0;
        const unsigned long long m = __ballot(keep);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int woff = 0;
        for (int w = 0; w < wave; ++w) woff += wsum[w];
        const int tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (keep) {
            indices[base + woff + before] = (int)k;
            data[base + woff + before] = v;
        }
        base += tot;
        __syncthreads();
    }
    (void)base_s;
}

// y = A x for CSR A: one wave per row, fixed-order lane-strided partial sums + butterfly.
// gridDim.y > 1: a batch of vectors, x and y advance by xb / yb doubles per batch entry.
__global__ void __launch_bounds__(256)
spmv_kernel(const int64_t *indptr, const int *indices, const double *data, const double *x,
            int64_t nrows, int64_t ld, double *y, int64_t xb = 0, int64_t yb = 0)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= ld) return;
    x += (int64_t)blockIdx.y * xb;
    y += (int64_t)blockIdx.y * yb;
    double s = 0.0;
    if (row < nrows) {
        const int64_t k1 = indptr[row + 1];
        for (int64_t k = indptr[row] + lane; k < k1; k += 64) s += data[k] * x[indices[k]];
    }
    s = wave_allreduce_sum(s);
    if (lane == 0) y[row] = s;
}

// rows j0 .. j0+nb-1 of the M x M identity (unit model vectors), row stride M
__global__ void __launch_bounds__(256) unit_rows_kernel(double *X, int64_t M, int64_t j0, int64_t nb)
{
    const int64_t n = nb * M;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * 256) {
        const int64_t b = idx / M, j = idx - b * M;
        X[idx] = (j == j0 + b) ? 1.0 : 0.0;
    }
}

// Diagnostic only (gh_debug_stream_read): pure streaming read of G, no reductions/barriers --
// the ceiling the sweep is compared with on the same device in the same session.
template <bool NT>
__global__ void __launch_bounds__(1024) stream_read_kernel(const double *G, int64_t n2, double *out)
{
    const d2 *g = reinterpret_cast<const d2 *>(G);
    d2 acc = d2{0.0, 0.0};
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + 3 * stride < n2; i += 4 * stride) {
        d2 a0, a1, a2, a3;
        if (NT) {
            a0 = __builtin_nontemporal_load(g + i);
            a1 = __builtin_nontemporal_load(g + i + stride);
            a2 = __builtin_nontemporal_load(g + i + 2 * stride);
            a3 = __builtin_nontemporal_load(g + i + 3 * stride);
        } else {
            a0 = g[i];
            a1 = g[i + stride];
            a2 = g[i + 2 * stride];
            a3 = g[i + 3 * stride];
        }
        acc += (a0 + a1) + (a2 + a3);
    }
    for (; i < n2; i += stride) acc += g[i];
    if (acc.x + acc.y == 1.2345e300) out[0] = acc.x;  // keep the loads alive
}

// ---------------------------------------------------------------- posterior sample window
// Accepted samples m = x / wm (hmc.py:328) are kept in a ring of the last K models in HBM, so
// the statistics the reference's plot scripts compute from the tail of model.dat
// (plot_uniform.py:44-55,103-104: np.mean / np.std over the last 100 rows) need no text I/O.

__global__ void __launch_bounds__(256)
ring_store_kernel(const double *x, const double *wm, int64_t M, double *slot)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const double w = wm ? wm[j] : 1.0;
    slot[j] = x[j] * (1.0 / w);  // WmInv @ mw: the reference multiplies by the stored reciprocal
}

// two-pass mean / population std over the K' valid slots, per cell (numpy's definition)
__global__ void __launch_bounds__(256)
ring_stats_kernel(const double *ring, int64_t M, int nvalid, double *mean, double *sd)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    double s = 0.0;
    for (int k = 0; k < nvalid; ++k) s += ring[(int64_t)k * M + j];
    const double mu = s / (double)nvalid;
    double q = 0.0;
    for (int k = 0; k < nvalid; ++k) {
        const double d = ring[(int64_t)k * M + j] - mu;
        q += d * d;
    }
    mean[j] = mu;
    sd[j] = sqrt(q / (double)nvalid);
}

// ------------------------------------------------------------------------- matrix-free path
// G is never stored: every entry is re-evaluated where it is needed, for problems whose kernel
// matrix does not fit in HBM.  N <= 16384: ONE evaluation per entry and leapfrog step
// (mf_fused_kernel below: the dense sweep's fusion on computed entries); larger N: two
// (mf_adjoint_kernel for the adjoint / update, mf_forward_kernel for the forward).  Wavefront and
// block reductions only, no MFMA.  The weighted kernel is Aw_ij = K_ij / wm_j with the column norms
// wm computed by mf_colnorm_kernel.

struct MfGeom {
    int kind;  // 0 prism, 1 tesseroid, 2 prism total field, 3 / 4 prism / tesseroid gravity component (GH_CELL_*)
    int comp;  // kinds 3, 4: the component (COMP_*; in what was kind's padding, the struct keeps its size)
    double radius_u;  // tesseroids, every observation at one height: its radius R + h (else 0)
    int64_t N, M;
    const double *o0, *o1, *o2, *o3;  // prism: x,y,z,- (total field: x,y,z,(fx,fy,fz))  tesseroid: lon_r, sinlat, coslat, radius
    const double *o4, *o5;            // tesseroid: sin lon, cos lon (fast leaf)
    const double *bounds6;
    double ratio;
};
static_assert(sizeof(MfGeom) == 96, "MfGeom is a kernel argument of every matrix-free pass: keep its size");

// The entry form of the generic passes below: MF_E_GEN = g.kind 0 prism gz / 1 tesseroid, MF_E_TF = the
// prisms' total-field entry (GH_CELL_PRISM_TF; the field direction is the three doubles at g.o3), MF_E_COMP =
// a prism gravity component (GH_CELL_PRISM_COMP; g.comp), MF_E_TESS = a tesseroid gravity component
// (GH_CELL_TESSEROID_COMP; g.comp: tess_comp_entry with the leaf chosen at run time, scaled as the dense
// assembly scales it).  The passes are templated on it so that the gz and tesseroid instantiations keep their
// register budget.
enum { MF_E_GEN = 0, MF_E_TF = 1, MF_E_COMP = 2, MF_E_TESS = 3 };
template <int E>
__device__ __forceinline__ double mf_entry(const MfGeom &g, int64_t i, const double *b)
{
    if (E == MF_E_TF) return prism_tf_entry(g.o0[i], g.o1[i], g.o2[i], b, g.o3[0], g.o3[1], g.o3[2]);
    if (E == MF_E_COMP) return prism_comp_entry_rt(g.comp, g.o0[i], g.o1[i], g.o2[i], b);
    if (E != MF_E_TESS && g.kind == 0) return prism_comp_entry<COMP_GZ>(g.o0[i], g.o1[i], g.o2[i], b);
    int err = 0;
    unsigned long long nl = 0;
    bool ov = false;
    if (E == MF_E_TESS)
        return tess_comp_scale(g.comp, tess_comp_entry<-1>(g.comp, g.o0[i], g.o1[i], g.o2[i], g.o3[i], b, g.ratio,
                                                           err, nl, ov));
    return tess_comp_scale(COMP_GZ, tess_comp_entry<COMP_GZ>(COMP_GZ, g.o0[i], g.o1[i], g.o2[i], g.o3[i], b, g.ratio,
                                                             err, nl, ov));
}

// wm_j = (sum_i K_ij^2)^wf: one wave per cell, lanes over observations
template <int E>
__global__ void __launch_bounds__(256) mf_colnorm_kernel(MfGeom g, double wf, double *wm)
{
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= g.M) return;
    const double *b = g.bounds6 + 6 * j;
    double s = 0.0;
    for (int64_t i = lane; i < g.N; i += 64) {
        const double k = mf_entry<E>(g, i, b);
        s += k * k;
    }
    s = wave_allreduce_sum(s);
    if (lane == 0) wm[j] = (wf == 0.5) ? sqrt(s) : pow(s, wf);
}

// Adjoint + leapfrog update for one cell per wave: the matrix-free counterpart of the ADJ /
// UPD / PFIN / GOUT / SPEC part of sweep_kernel (same arithmetic per column).
template <int E>
__global__ void __launch_bounds__(256) mf_adjoint_kernel(MfGeom g, SweepArgs a, const double *wm)
{
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t j = (int64_t)blockIdx.x * 4 + wave;
    const int mode = a.mode;
    double pp = 0.0;
    if (j < g.M) {
        const double *b = g.bounds6 + 6 * j;
        double s = 0.0;
        for (int64_t i = lane; i < g.N; i += 64) s += mf_entry<E>(g, i, b) * a.r[i];
        s = wave_allreduce_sum(s);
        const double w = wm[j];
        s = (w != 0.0) ? s * (1.0 / w) : s;
        const double gr = a.greg ? a.greg[j] : 0.0;
        const double grad = 2.0 * s + gr;
        if ((mode & SW_GOUT) && lane == 0) a.g_out[j] = grad;
        if (mode & SW_PFIN) {
            const double pf = a.p_in[j] - a.c_p * grad;
            pp = pf * pf;
            if (!(mode & SW_SPEC) && lane == 0) a.p_out[j] = pf;
        }
        if (mode & SW_UPD) {
            const double psrc = (mode & SW_SPEC) ? a.pn_in[j] : a.p_in[j];
            double pj = psrc - a.c_u * grad;
            double xj = a.x_in[j] + a.dt * pj;
            const double hi = a.high[j], lo = a.low[j];
            if (xj > hi) {
                xj = hi;
                pj = -pj;
            } else if (xj < lo) {
                xj = lo;
                pj = -pj;
            }
            if (lane == 0) {
                a.p_out[j] = pj;
                a.x_out[j] = xj;
            }
        }
    }
    if (mode & SW_PFIN) {
        if (lane == 0) red[wave] = pp;
        __syncthreads();
        if (threadIdx.x == 0) a.pp_part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    }
}

// Forward partials: thread = observation, blockIdx.y = chunk of cells; slab[chunk][i]
template <int E>
__global__ void __launch_bounds__(256)
mf_forward_kernel(MfGeom g, const double *x, const double *wm, int64_t cells_per_chunk, int64_t ld,
                  double *slab)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ld) return;
    const int64_t j0 = (int64_t)blockIdx.y * cells_per_chunk;
    int64_t j1 = j0 + cells_per_chunk;
    if (j1 > g.M) j1 = g.M;
    double acc = 0.0;
    if (i < g.N) {
        for (int64_t j = j0; j < j1; ++j) {
            const double w = wm ? wm[j] : 1.0;
            const double xs = (w != 0.0) ? x[j] * (1.0 / w) : x[j];
            acc += mf_entry<E>(g, i, g.bounds6 + 6 * j) * xs;
        }
    }
    slab[(int64_t)blockIdx.y * ld + i] = acc;
}


// rows [i0, i0 + nrows) of the WEIGHTED kernel of a matrix-free context as a dense row-major block
// out[nrows][M] (what gather_rows_kernel copies out of a stored G): the wavelet compressor's input
// (compressor3D.kernelcompressor transforms whole rows).  Entries by the generic engines (mf_entry: the
// values the dense assembly stores), divided by the column's weight as the in-place weighting does.
template <int E>
__global__ void __launch_bounds__(256)
mf_rows_kernel(MfGeom g, const double *__restrict__ wm, int64_t i0, int64_t nrows, double *__restrict__ out)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = blockIdx.y;
    if (j >= g.M || i >= nrows) return;
    const double k = mf_entry<E>(g, i0 + i, g.bounds6 + 6 * j);
    const double w = wm ? wm[j] : 1.0;
    out[i * g.M + j] = (w != 0.0) ? k * (1.0 / w) : k;
}

// ---- fused matrix-free pass: every entry evaluated ONCE per leapfrog step -------------------
// The dense sweep's fusion applied to entries that are computed instead of loaded: a workgroup owns
// column j, evaluates its N entries once (kept in LDS), forms the dot with r, applies the leapfrog
// update of cell j and adds the column times the NEW x_j to its forward partial -- N*M entry
// evaluations per step instead of 2*N*M (mf_adjoint_kernel + mf_forward_kernel, still used for
// N > 16384).  Columns are dealt to the workgroups round-robin (cells near the poles / the top
// layer cost several times the average: contiguous ranges would leave one workgroup with all of
// them); the order of every sum is fixed by indices only, so results are reproducible bit for bit.
//
// Tesseroids: what depends on the cell alone -- the root's centre, its three size measures with
// the two acos, the 2x2x2 GLQ nodes with their sin/cos -- is evaluated once per cell by
// tess_cellconst_kernel (11 of the 14 trigonometric calls of a pair that needs no subdivision, and
// that is 99.9 % of the pairs of the global model) with the same expressions, hence the same bits,
// as tess_comp_entry<COMP_GZ>; a pair whose root must be subdivided (or flags an error) takes the engine itself.

constexpr int TESS_NC = 32;  // doubles per cell in the table of cell constants

// [0] rt [1] rt*rt [2] lont [3] sinlatt [4] coslatt [5] ratio*Llon [6] ratio*Llat [7] ratio*Lr
// [8,9] lonc [10,11] sinlatc [12,13] coslatc [14,15] rc [16,17] rc*rc
// [18..21] kappa[j][k] = rc[k]^2 * coslatc[j]  [22] scale  [23] -
// [24,25] cos lonc  [26,27] sin lonc   (fast leaf: cos(lon - lonc) by the addition theorem)
__global__ void __launch_bounds__(256)
tess_cellconst_kernel(const double *__restrict__ bounds6, int64_t M, double ratio, double *__restrict__ cc)
{
#pragma clang fp contract(off)
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const double MEAN_R = 6378137.0;
    const double d2r = 3.14159265358979323846 / 180;
    const double node[2] = {-0.577350269189625731058868041146, 0.577350269189625731058868041146};
    const double *b = bounds6 + 6 * j;
    const double w = b[0], e = b[1], s = b[2], n = b[3], top = b[4], bottom = b[5];
    double *o = cc + (int64_t)TESS_NC * j;
    // distance_size of the root (_tesseroid_numba.py:94-111)
    const double rt = 0.5 * (top + bottom) + MEAN_R;
    const double lont = d2r * 0.5 * (w + e);
    const double latt = d2r * 0.5 * (s + n);
    const double sinlatt = sin(latt), coslatt = cos(latt);
    const double rtop = top + MEAN_R;
    const double Llon = rtop * acos(sinlatt * sinlatt + (coslatt * coslatt) * cos(d2r * (e - w)));
    const double Llat = rtop * acos(sin(d2r * n) * sin(d2r * s) + cos(d2r * n) * cos(d2r * s));
    const double Lr = top - bottom;
    o[0] = rt;
    o[1] = rt * rt;
    o[2] = lont;
    o[3] = sinlatt;
    o[4] = coslatt;
    o[5] = ratio * Llon;
    o[6] = ratio * Llat;
    o[7] = ratio * Lr;
    // scale_nodes of the root taken as a leaf (_tesseroid_numba.py:75-91)
    const double dlon = d2r * (e - w), dlat = d2r * (n - s), dr = top - bottom;
    double coslatc[2], rc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        o[8 + i] = 0.5 * dlon * node[i] + d2r * 0.5 * (e + w);
        const double latc = 0.5 * dlat * node[i] + d2r * 0.5 * (n + s);
        o[10 + i] = sin(latc);
        coslatc[i] = cos(latc);
        o[12 + i] = coslatc[i];
        rc[i] = (0.5 * dr * node[i] + 0.5 * (top + bottom) + MEAN_R);
        o[14 + i] = rc[i];
        o[16 + i] = rc[i] * rc[i];
    }
#pragma unroll
    for (int jn = 0; jn < 2; ++jn)
#pragma unroll
        for (int k = 0; k < 2; ++k) o[18 + 2 * jn + k] = (rc[k] * rc[k]) * coslatc[jn];
    o[22] = dlon * dlat * dr * 0.125;
    o[23] = o[22] * (-100000.0 * 0.00000006673);  // (tess_leaf_fast: scale and sign in one factor)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        o[24 + i] = cos(o[8 + i]);
        o[26 + i] = sin(o[8 + i]);
    }
    // (tess_leaf_fast: weight of node (lat j, r k) times r_k)
#pragma unroll
    for (int jn = 0; jn < 2; ++jn)
#pragma unroll
        for (int k = 0; k < 2; ++k) o[28 + 2 * jn + k] = o[18 + 2 * jn + k] * rc[k];
}

__device__ __noinline__ double tess_entry_slow(double lon, double sinlat, double coslat, double radius,
                                               const double *bounds, double ratio, unsigned &nleaf)
{
    int err = 0;
    unsigned long long nl = 0;
    bool ov = false;
    const double v =
        tess_comp_scale(COMP_GZ, tess_comp_entry<COMP_GZ>(COMP_GZ, lon, sinlat, coslat, radius, bounds, ratio, err, nl, ov));
    nleaf += (unsigned)nl;
    return v;
}

// The root taken as ONE 2x2x2 GLQ leaf (a pair that needs no subdivision), from the cell's constants:
// the bits tess_comp_entry<COMP_GZ> produces for such a pair.
__device__ __forceinline__ double tess_leaf_cc(double lon, double sinlat, double coslat, double radius,
                                               const double *__restrict__ cc)
{
#pragma clang fp contract(off)
    const double r_sqr = radius * radius;
    double result = 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const double coslon = cos(lon - cc[8 + i]);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const double cospsi = sinlat * cc[10 + j] + coslat * cc[12 + j] * coslon;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const double rck = cc[14 + k];
                const double l_sqr = r_sqr + cc[16 + k] - 2 * radius * rck * cospsi;
                result += cc[18 + 2 * j + k] * (rck * cospsi - radius) / (l_sqr * sqrt(l_sqr));
            }
        }
    }
    result *= -1;
    double acc = 0.0;
    acc += cc[22] * result;
    return acc * 100000.0 * 0.00000006673;
}

// The same root leaf with the arithmetic re-arranged for throughput (the per-step pass of the
// matrix-free mode; the decisions -- which pairs are NOT a single leaf -- were taken once, exactly,
// when the near-field table was built).  cos(lon - lonc) by the addition theorem from sin / cos of
// the observation's longitude (tabulated per observation) and of the nodes' (per cell): 2 FMAs
// instead of a ~55-instruction cos; 1 / l^3 from the hardware reciprocal square root and one Newton
// factor (to ~2e-15) instead of an IEEE sqrt and an IEEE divide (~28 instructions); contraction
// allowed.  The reference itself writes l_sqr**1.5
// (_tesseroid_numba.py:218), so no form is bitwise its pow(); this one agrees with tess_leaf_cc to
// <= 1e-13 of the entry for pairs that are far by the reference's own criterion (the conditioning
// of l^2 = r^2 + r'^2 - 2 r r' cos psi is the formulation's: an ulp of cos psi moves l^2 by
// 2 r r' 1e-16 ~ 1e-2 m^2 against l^2 >= 1e10 m^2).  Stated tolerance of the path: 1e-10.
// (Measured at C4 against the dense engine with y refined by one / two Newton steps and then cubed:
// forward 6.5e-15 / 6.2e-15, gradient 9.8e-15 / 7.3e-15 -- the hardware estimate is good to ~2^-26
// and what remains is the conditioning of l^2.)
__device__ __forceinline__ double tess_leaf_fast(double sinlon, double coslon_o, double sinlat, double coslat,
                                                 double radius, const double *__restrict__ cc)
{
    // Per node: l = |r - r_c|^2 by one fma, y = v_rsq_f64(l) (~2^-26), and instead of refining y and
    // cubing the result, the cube of the raw y times one Newton factor:
    //     l^(-3/2) = y^3 (2.5 - 1.5 l y^2) (1 + 7.5 d^2 + ...),  d = relative error of y,
    // i.e. 2*10^-15: eight operations and the rsq per node where the refined form took ten.  The
    // node's weight and (r_c cos(psi) - r) are one fma of cos(psi) with coefficients that do not
    // depend on the node's longitude (kappa_jk r_c: tabulated per cell; kappa_jk r: per entry).
    const double r_sqr = radius * radius;
    const double A0 = r_sqr + cc[16], A1 = r_sqr + cc[17];
    const double tr = -2.0 * radius;
    const double m0 = cc[14] * tr, m1 = cc[15] * tr;
    const double G00 = cc[28], G01 = cc[29], G10 = cc[30], G11 = cc[31];
    const double H00 = -cc[18] * radius, H01 = -cc[19] * radius, H10 = -cc[20] * radius, H11 = -cc[21] * radius;
    const double P0 = coslat * cc[12], P1 = coslat * cc[13], Q0 = sinlat * cc[10], Q1 = sinlat * cc[11];
    double result = 0.0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const double coslon = fma(sinlon, cc[26 + i], coslon_o * cc[24 + i]);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const double cospsi = fma(j ? P1 : P0, coslon, j ? Q1 : Q0);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const double l = fma(k ? m1 : m0, cospsi, k ? A1 : A0);
                const double y = __builtin_amdgcn_rsq(l);
                const double y2 = y * y;
                const double y3 = y2 * y;
                // y^3 (2.5 - 1.5 l y^2) as y^3 + 1.5 (y^3 (1 - l y^2)): one constant that is not an
                // inline operand instead of two (each costs two moves per use: an instruction reads
                // one scalar register pair at most)
                const double w = fma(y3 * fma(-l, y2, 1.0), 1.5, y3);
                const double fg = fma(j ? (k ? G11 : G10) : (k ? G01 : G00), cospsi,
                                      j ? (k ? H11 : H10) : (k ? H01 : H00));
                result = fma(fg, w, result);
            }
        }
    }
    return result * cc[23];
}

// tess_leaf_fast with what depends on (observation radius, cell) alone hoisted out of the entry: for
// observations at ONE height these eight numbers are per-column constants.
// pre = {r^2 + rc0^2, r^2 + rc1^2, -2 r rc0, -2 r rc1, -kappa_00 r, -kappa_01 r, -kappa_10 r, -kappa_11 r}
__device__ __forceinline__ void tess_leaf_fast_pre(double radius, const double *__restrict__ cc, double (&pre)[8])
{
    const double r_sqr = radius * radius;
    const double tr = -2.0 * radius;
    pre[0] = r_sqr + cc[16];
    pre[1] = r_sqr + cc[17];
    pre[2] = cc[14] * tr;
    pre[3] = cc[15] * tr;
    pre[4] = -cc[18] * radius;
    pre[5] = -cc[19] * radius;
    pre[6] = -cc[20] * radius;
    pre[7] = -cc[21] * radius;
}

__device__ __forceinline__ double tess_leaf_fast_ru(double sinlon, double coslon_o, double sinlat, double coslat,
                                                    const double *__restrict__ cc, const double (&pre)[8])
{
    const double A0 = pre[0], A1 = pre[1], m0 = pre[2], m1 = pre[3];
    const double G00 = cc[28], G01 = cc[29], G10 = cc[30], G11 = cc[31];
    const double H00 = pre[4], H01 = pre[5], H10 = pre[6], H11 = pre[7];
    const double P0 = coslat * cc[12], P1 = coslat * cc[13], Q0 = sinlat * cc[10], Q1 = sinlat * cc[11];
    double result = 0.0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const double coslon = fma(sinlon, cc[26 + i], coslon_o * cc[24 + i]);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const double cospsi = fma(j ? P1 : P0, coslon, j ? Q1 : Q0);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const double l = fma(k ? m1 : m0, cospsi, k ? A1 : A0);
                const double y = __builtin_amdgcn_rsq(l);
                const double y2 = y * y;
                const double y3 = y2 * y;
                const double w = fma(y3 * fma(-l, y2, 1.0), 1.5, y3);
                const double fg = fma(j ? (k ? G11 : G10) : (k ? G01 : G00), cospsi,
                                      j ? (k ? H11 : H10) : (k ? H01 : H00));
                result = fma(fg, w, result);
            }
        }
    }
    return result * cc[23];
}

// Does the pair need more than the root leaf (subdivision, or an error flag)?  The root's
// distance / size test of tess_comp_entry (_tesseroid_numba.py:94-111,135-157) with the same bits.
__device__ __forceinline__ bool tess_is_near_cc(double lon, double sinlat, double coslat, double radius,
                                                const double *__restrict__ cc)
{
#pragma clang fp contract(off)
    const double cospsi0 = sinlat * cc[3] + coslat * cc[4] * cos(lon - cc[2]);
    const double distance = sqrt(radius * radius + cc[1] - 2 * radius * cc[0] * cospsi0);
    return (distance <= cc[5]) || (distance <= cc[6]) || (distance <= cc[7]);
}

// One (observation, tesseroid) entry from the cell's constants; same bits as tess_comp_entry<COMP_GZ>.
__device__ __forceinline__ double tess_entry_cc(double lon, double sinlat, double coslat, double radius,
                                                const double *__restrict__ cc, const double *bounds, double ratio,
                                                unsigned &nleaf)
{
    if (tess_is_near_cc(lon, sinlat, coslat, radius, cc))
        return tess_entry_slow(lon, sinlat, coslat, radius, bounds, ratio, nleaf);
    nleaf += 1;
    return tess_leaf_cc(lon, sinlat, coslat, radius, cc);
}

// Near-field table.  Whether a pair needs the adaptive subdivision depends on the geometry alone,
// and those pairs (0.02 % of the global model's 5.3*10^8, but 50 .. 2000 times the work of a far
// pair each, and concentrated in the columns of the top layer and of the poles) are what unbalances
// the matrix-free pass.  They are found once (count + ordered fill, one workgroup per column),
// their entries evaluated once by the adaptive engine and kept as a sparse per-column list (row index,
// value); the per-step pass evaluates the root leaf for every pair and then overwrites the listed
// rows.  Everything else of G is still never stored.
struct MfNear {
    const int64_t *ptr;  // M + 1
    const int *row;      // ptr[M]
    const double *val;   // ptr[M], entries in mGal per g/cm^3 (unweighted, like the dense G)
};

__global__ void __launch_bounds__(256)
tess_near_count_kernel(MfGeom g, const double *__restrict__ cellc, int *__restrict__ count)
{
    __shared__ int wsum[4];
    const int64_t j = blockIdx.x;
    const double *cc = cellc + (int64_t)TESS_NC * j;
    int n = 0;
    for (int64_t i = threadIdx.x; i < g.N; i += 256)
        n += tess_is_near_cc(g.o0[i], g.o1[i], g.o2[i], g.o3[i], cc) ? 1 : 0;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) n += __shfl_xor(n, off, WAVE);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) count[j] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// ordered compaction (rows ascending) + the entries themselves; leaves: GLQ leaves of these pairs
__global__ void __launch_bounds__(256)
tess_near_fill_kernel(MfGeom g, const double *__restrict__ cellc, const int64_t *__restrict__ ptr,
                      int *__restrict__ row, double *__restrict__ val, unsigned long long *leaves)
{
    __shared__ int wsum[4];
    const int64_t j = blockIdx.x;
    const double *cc = cellc + (int64_t)TESS_NC * j;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t base = ptr[j];
    if (ptr[j + 1] == base) return;
    unsigned nl = 0;
    for (int64_t i0 = 0; i0 < g.N; i0 += 256) {
        const int64_t i = i0 + threadIdx.x;
        const bool near = i < g.N && tess_is_near_cc(g.o0[i], g.o1[i], g.o2[i], g.o3[i], cc);
        const unsigned long long m = __ballot(near);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int woff = 0;
        for (int w = 0; w < wave; ++w) woff += wsum[w];
        const int tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (near) {
            row[base + woff + before] = (int)i;
            val[base + woff + before] =
                tess_entry_slow(g.o0[i], g.o1[i], g.o2[i], g.o3[i], g.bounds6 + 6 * j, g.ratio, nl);
        }
        base += tot;
        __syncthreads();
    }
    unsigned long long t = nl;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) t += __shfl_xor(t, off, WAVE);
    if (lane == 0 && t) atomicAdd(leaves, t);
}

struct MfStats {
    unsigned long long entries, leaves;
};

// T threads per workgroup, EPT rows per thread (row of slot k: t + k*T): T*EPT >= ld; KIND: 0 prisms,
// 1 tesseroids with the subdivision inside the pass, 2 / 3 tesseroids with the near-field table and the
// exact-order / the fast root leaf, 5 prisms' total field, 6 / 7 prisms' gradient tensor / potential, geoid, gx,
// gy (the component g.comp is a uniform branch inside the family; one kernel for all ten components held 272
// registers at <256, 4>, one wave per SIMD instead of two) (separate kernels: the prism entry's log/atan2 and the
// tesseroid entry's trigonometry would otherwise share one register budget; 4 is taken by mfbatch.hip.h's kinds).
// LDS: T*EPT doubles (the column) + 2 x (T/64 + 8) doubles (ping-pong slots of the dot).
template <int T, int EPT, int KIND>
__global__ void __launch_bounds__(T)
mf_fused_kernel(MfGeom g, SweepArgs a, const double *__restrict__ wm, const double *__restrict__ cellc,
                MfNear near, MfStats *stats)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int NW = T / 64;
    constexpr int SLOT = NW + 8;
    double *Ks = smem;
    double *scratch = smem + (size_t)T * EPT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mode = a.mode;
    const int64_t N = g.N;
    constexpr bool TABLE = KIND == 2 || KIND == 3;  // tesseroids with the near-field table
    const int ept = (int)((a.ld + T - 1) / T);  // slots in use (<= EPT)
    // (KIND 5: the field direction, the same for every entry)
    const double fx = KIND == 5 ? g.o3[0] : 0.0, fy = KIND == 5 ? g.o3[1] : 0.0, fz = KIND == 5 ? g.o3[2] : 0.0;
    const int comp = (KIND == 6 || KIND == 7) ? g.comp : 0;  // (KIND 6, 7: the component)
    double dacc[EPT];
#pragma unroll
    for (int k = 0; k < EPT; ++k) dacc[k] = 0.0;
    double pp = 0.0;
    unsigned nleaf = 0, nent = 0;
    // (table forms: a thread's rows of r are the same for every column -- kept in registers)
    double rr[TABLE ? EPT : 1];
    if (TABLE) {
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
            const int64_t i = tid + (int64_t)k * T;
            rr[k] = ((mode & SW_ADJ) && k < ept && i < N) ? a.r[i] : 0.0;
        }
    }
    int it = 0;
    for (int64_t j = blockIdx.x; j < g.M; j += gridDim.x, ++it) {
        const double *b = g.bounds6 + 6 * j;
        const double *cc = cellc ? cellc + (int64_t)TESS_NC * j : nullptr;
        double s = 0.0;
        if (KIND == 3) {
            // every pair as its root leaf (no test, no divergence); the rows of the near-field list
            // are then overwritten with their stored entries, and the dot reads the finished column.
            // The observation's five numbers for slot k + 1 are requested before slot k is evaluated
            // (they are the same for every column: L2 hits, but ~1 us away): at 160 instructions
            // per slot the pass otherwise waits for memory more than half of its time.
            int64_t i = tid;
            double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0, c4 = 0.0;
            if (i < N) {
                c0 = g.o4[i];
                c1 = g.o5[i];
                c2 = g.o1[i];
                c3 = g.o2[i];
                c4 = g.o3[i];
            }
#pragma unroll 1
            for (int k = 0; k < ept; ++k) {
                const int64_t in = i + T;
                double n0 = 0.0, n1 = 0.0, n2 = 0.0, n3 = 0.0, n4 = 0.0;
                if (k + 1 < ept && in < N) {
                    n0 = g.o4[in];
                    n1 = g.o5[in];
                    n2 = g.o1[in];
                    n3 = g.o2[in];
                    n4 = g.o3[in];
                }
                double v = 0.0;
                if (i < N) {
                    v = tess_leaf_fast(c0, c1, c2, c3, c4, cc);
                    nent += 1;
                }
                Ks[(size_t)k * T + tid] = v;
                i = in;
                c0 = n0;
                c1 = n1;
                c2 = n2;
                c3 = n3;
                c4 = n4;
            }
        }
        if (KIND == 2) {
#pragma unroll 1
            for (int k = 0; k < ept; ++k) {
                const int64_t i = tid + (int64_t)k * T;
                double v = 0.0;
                if (i < N) {
                    v = tess_leaf_cc(g.o0[i], g.o1[i], g.o2[i], g.o3[i], cc);
                    nent += 1;
                }
                Ks[(size_t)k * T + tid] = v;
            }
        }
        if (TABLE) {
            const int64_t q0 = near.ptr[j], q1 = near.ptr[j + 1];
            if (q1 > q0) {
                __syncthreads();
                for (int64_t q = q0 + tid; q < q1; q += T) Ks[near.row[q]] = near.val[q];
                __syncthreads();
            }
            if (mode & SW_ADJ) {
#pragma unroll
                for (int k = 0; k < EPT; ++k)
                    if (k < ept) s += Ks[(size_t)k * T + tid] * rr[k];
            }
        } else {
#pragma unroll 1
            for (int k = 0; k < ept; ++k) {
                const int64_t i = tid + (int64_t)k * T;
                double v = 0.0;
                if (i < N) {
                    if (KIND == 0) {
                        v = prism_comp_entry<COMP_GZ>(g.o0[i], g.o1[i], g.o2[i], b);
                        nleaf += 1;
                    } else if (KIND == 5) {
                        v = prism_tf_entry(g.o0[i], g.o1[i], g.o2[i], b, fx, fy, fz);
                        nleaf += 1;
                    } else if (KIND == 6) {
                        v = prism_tensor_entry_rt(comp, g.o0[i], g.o1[i], g.o2[i], b);
                        nleaf += 1;
                    } else if (KIND == 7) {
                        v = prism_field_entry_rt(comp, g.o0[i], g.o1[i], g.o2[i], b);
                        nleaf += 1;
                    } else {
                        v = tess_entry_cc(g.o0[i], g.o1[i], g.o2[i], g.o3[i], cc, b, g.ratio, nleaf);
                    }
                    nent += 1;
                    if (mode & SW_ADJ) s += v * a.r[i];
                }
                Ks[(size_t)k * T + tid] = v;
            }
        }
        double xj;
        if (mode & SW_ADJ) {
            s = wave_allreduce_sum(s);
            double *slot = scratch + (it & 1) * SLOT;
            if (lane == 0) slot[wave] = s;
            __syncthreads();
            double t = 0.0;
#pragma unroll
            for (int w = 0; w < NW; ++w) t += slot[w];
            const double w = wm[j];
            t = (w != 0.0) ? t * (1.0 / w) : t;
            const double gr = a.greg ? a.greg[j] : 0.0;
            const double grad = 2.0 * t + gr;
            xj = (mode & (SW_UPD | SW_FWD)) ? a.x_in[j] : 0.0;
            if ((mode & SW_GOUT) && tid == 0) a.g_out[j] = grad;
            if (mode & SW_PFIN) {
                const double pf = a.p_in[j] - a.c_p * grad;
                pp += pf * pf;
                if (!(mode & SW_SPEC) && tid == 0) a.p_out[j] = pf;
            }
            if (mode & SW_UPD) {
                const double psrc = (mode & SW_SPEC) ? a.pn_in[j] : a.p_in[j];
                double pj = psrc - a.c_u * grad;
                xj = xj + a.dt * pj;
                const double hi = a.high[j], lo = a.low[j];
                if (xj > hi) {
                    xj = hi;
                    pj = -pj;
                } else if (xj < lo) {
                    xj = lo;
                    pj = -pj;
                }
                if (tid == 0) {
                    a.p_out[j] = pj;
                    a.x_out[j] = xj;
                }
            }
        } else {
            xj = a.x_in[j];
        }
        if (mode & SW_FWD) {
            const double w = wm ? wm[j] : 1.0;
            const double xs = (w != 0.0) ? xj * (1.0 / w) : xj;
#pragma unroll
            for (int k = 0; k < EPT; ++k)
                if (k < ept) dacc[k] += Ks[(size_t)k * T + tid] * xs;
        }
    }
    if ((mode & SW_PFIN) && tid == 0) a.pp_part[blockIdx.x] = pp;
    if (mode & SW_FWD) {
        double *out = a.slab + (int64_t)blockIdx.x * a.ld;
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
            const int64_t i = tid + (int64_t)k * T;
            if (i < a.ld) out[i] = dacc[k];
        }
    }
    if (stats) {
        unsigned long long e = nent, l = TABLE ? nent : nleaf;  // (KIND 2, 3: one root leaf per entry)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            e += __shfl_xor(e, off, WAVE);
            l += __shfl_xor(l, off, WAVE);
        }
        if (lane == 0) {
            atomicAdd(&stats->entries, e);
            atomicAdd(&stats->leaves, l);
        }
    }
}


// ---- the fast tesseroid pass with its per-column latencies taken out of the way -----------------
// mf_fused_kernel<.., 3> moves through a column in lock-step phases (28 cell constants by scalar
// loads -> slots -> barrier -> seven per-cell scalars -> update -> forward) and, with ONE workgroup
// per CU, nothing overlaps the ~1 us memory round trips at the phase boundaries: the SQ counters
// showed VALU busy 59 % at 171 instructions per slot.  Here wave 0 requests the NEXT column's cell
// constants and per-cell scalars while the current column's slots are evaluated and parks them in
// LDS before the column's barrier; every wave then picks them up from LDS (a broadcast read made
// uniform with readfirstlane) -- ~100 cycles instead of an L2 round trip.  Same arithmetic, same
// order of the sums as mf_fused_kernel<.., 3>: identical bits.
__device__ __forceinline__ double uniform_d(double v)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readfirstlane((int)b);
    const int hi = __builtin_amdgcn_readfirstlane((int)(b >> 32));
    return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

template <int T, int EPT>
__global__ void __launch_bounds__(T)
mf_tess_fast_kernel(MfGeom g, SweepArgs a, const double *__restrict__ wm, const double *__restrict__ cellc,
                    MfNear near, MfStats *stats)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int NW = T / 64;
    constexpr int SLOT = NW + 8;
    constexpr int NSC = 16;                     // per-cell scalars parked per column
    double *Ks = smem;
    double *rs = Ks + (size_t)T * EPT;          // r, padded with zeros to T * EPT
    double *scratch = rs + (size_t)T * EPT;     // 2 x SLOT: ping-pong slots of the dot
    double *ccs = scratch + 2 * SLOT;           // 2 x 32: cell constants of this / the next column
    double *cs = ccs + 64;                      // 3 x NSC: x, p, low, high, greg, pn, wm, near.ptr[j], [j+1]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mode = a.mode;
    const int64_t N = g.N;
    const int ept = (int)((a.ld + T - 1) / T);
    double dacc[EPT];
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const int64_t i = tid + (int64_t)k * T;
        dacc[k] = 0.0;
        rs[(size_t)k * T + tid] = ((mode & SW_ADJ) && i < N) ? a.r[i] : 0.0;
    }
    double pp = 0.0;
    unsigned nent = 0;
    // What wave 0 fetches for a column -- lanes 0..27 the cell constants, lanes 32..38 the scalars,
    // lanes 39, 40 the bounds of the near-field table -- is ONE 8-byte load from a per-lane base with a
    // per-lane column stride, looked at a column later.  (Three branches, one of them choosing its
    // vector among seven kernel arguments -- which the compiler turns into a load of the pointer from
    // the argument segment -- and each consuming its value at once were three to four serial memory
    // round trips in front of wave 0's share of every column, the other waves waiting at the
    // barrier.  Absent vectors read `cellc` and are replaced when parked.)
    const int sq = lane - 32;
    const char *fbase = reinterpret_cast<const char *>(cellc);
    int64_t fstride = 0;
    bool fabsent = true, fint = false;
    if (wave == 0) {
        if (lane < TESS_NC) {
            fbase = reinterpret_cast<const char *>(cellc + lane);
            fstride = TESS_NC * (int64_t)sizeof(double);
            fabsent = false;
        } else if (sq >= 0 && sq < 7) {
            const double *v = sq == 0 ? a.x_in : sq == 1 ? a.p_in : sq == 2 ? a.low : sq == 3 ? a.high
                            : sq == 4 ? a.greg : sq == 5 ? a.pn_in : wm;
            fabsent = v == nullptr;
            if (v) fbase = reinterpret_cast<const char *>(v);
            fstride = v ? (int64_t)sizeof(double) : 0;
        } else if (sq == 7 || sq == 8) {
            fbase = reinterpret_cast<const char *>(near.ptr + (sq - 7));
            fstride = sizeof(int64_t);
            fabsent = false;
            fint = true;
        }
    }
    auto fetch = [&](int64_t j) -> unsigned long long {
        return *reinterpret_cast<const unsigned long long *>(fbase + j * fstride);
    };
    auto park = [&](unsigned long long raw, int itn) {
        double v = fint ? (double)(long long)raw : __longlong_as_double((long long)raw);  // (exact: far below 2^53)
        if (fabsent) v = sq == 6 ? 1.0 : 0.0;
        // (the column's weight is parked as its reciprocal, rounded as 1.0 / w is: one division per
        // column instead of two in every wave)
        if (sq == 6) v = (v != 0.0) ? 1.0 / v : 1.0;
        if (lane < TESS_NC) ccs[(itn & 1) * 32 + lane] = v;
        else if (lane >= 32 && lane < 41) cs[(itn % 3) * NSC + (lane - 32)] = v;
    };
    if (wave == 0 && (int64_t)blockIdx.x < g.M) park(fetch(blockIdx.x), 0);
    // the observation's five numbers for slot 0 never change: kept in registers
    double f0 = 0.0, f1 = 0.0, f2 = 0.0, f3 = 0.0, f4 = 0.0;
    if (tid < N) {
        f0 = g.o4[tid];
        f1 = g.o5[tid];
        f2 = g.o1[tid];
        f3 = g.o2[tid];
        f4 = g.o3[tid];
    }
    __syncthreads();
    const unsigned toff = (unsigned)tid * (unsigned)sizeof(double);
    const unsigned olast = (unsigned)(N - 1) * (unsigned)sizeof(double);
    int it = 0;
    for (int64_t j = blockIdx.x; j < g.M; j += gridDim.x, ++it) {
        const int64_t jn = j + gridDim.x;
        unsigned long long nxt = 0;
        if (wave == 0 && jn < g.M) nxt = fetch(jn);   // in flight while the slots are evaluated
        // this column's cell constants, uniform
        double cc[TESS_NC];
#pragma unroll
        for (int q = 8; q < TESS_NC; ++q) cc[q] = uniform_d(ccs[(it & 1) * 32 + q]);
        // The slots of this column, two per trip: while one is evaluated the observer constants of
        // the next are in flight, and "next" becomes "current" by taking turns between two register
        // sets, not by five 64-bit moves per entry.  Their loads are unconditional (rows past the end
        // re-read the last row; such slots are not evaluated) at a 32-bit byte offset from the five
        // fixed bases (global_load v, voff, s[base]): no zeroing, no branch, no 64-bit address sums.
        double a0 = f0, a1 = f1, a2 = f2, a3 = f3, a4 = f4, b0, b1, b2, b3, b4;
        unsigned off = toff;
#define GH_OBS_LOAD(n0, n1, n2, n3, n4)                                                                  \
    {                                                                                                    \
        off = off + (unsigned)(T * sizeof(double));                                                      \
        unsigned oc = off < olast ? off : olast;                                                         \
        asm volatile("" : "+v"(oc));                                                                     \
        n0 = *reinterpret_cast<const double *>(reinterpret_cast<const char *>(g.o4) + oc);               \
        n1 = *reinterpret_cast<const double *>(reinterpret_cast<const char *>(g.o5) + oc);               \
        n2 = *reinterpret_cast<const double *>(reinterpret_cast<const char *>(g.o1) + oc);               \
        n3 = *reinterpret_cast<const double *>(reinterpret_cast<const char *>(g.o2) + oc);               \
        n4 = *reinterpret_cast<const double *>(reinterpret_cast<const char *>(g.o3) + oc);               \
    }
#define GH_SLOT_EVAL(c0, c1, c2, c3, c4, kk)                                                             \
    {                                                                                                    \
        double v = 0.0;                                                                                  \
        if (tid + (int64_t)(kk) * T < N) {                                                               \
            v = tess_leaf_fast(c0, c1, c2, c3, c4, cc);                                                  \
            nent += 1;                                                                                   \
        }                                                                                                \
        Ks[(size_t)(kk) * T + tid] = v;                                                                  \
    }
#pragma unroll 1
        for (int k = 0; k < ept; k += 2) {
            GH_OBS_LOAD(b0, b1, b2, b3, b4)
            GH_SLOT_EVAL(a0, a1, a2, a3, a4, k)
            if (k + 1 >= ept) break;
            GH_OBS_LOAD(a0, a1, a2, a3, a4)
            GH_SLOT_EVAL(b0, b1, b2, b3, b4, k + 1)
        }
#undef GH_OBS_LOAD
#undef GH_SLOT_EVAL
        const double *sc = cs + (it % 3) * NSC;
        const int64_t q0 = (int64_t)sc[7], q1 = (int64_t)sc[8];
        if (q1 > q0) {
            __syncthreads();
            for (int64_t q = q0 + tid; q < q1; q += T) Ks[near.row[q]] = near.val[q];
            __syncthreads();
        }
        double s = 0.0;
        if (mode & SW_ADJ) {
#pragma unroll
            for (int k = 0; k < EPT; ++k)
                if (k < ept) s += Ks[(size_t)k * T + tid] * rs[(size_t)k * T + tid];
            s = wave_sum_dpp(s);
        }
        double *slot = scratch + (it & 1) * SLOT;
        if (lane == 0) slot[wave] = s;
        if (wave == 0 && jn < g.M) park(nxt, it + 1);
        __syncthreads();
        const double iw = sc[6];  // 1 / w_j (1 where the column has no weight)
        double xj = sc[0];
        if (mode & SW_ADJ) {
            double t = 0.0;
#pragma unroll
            for (int wv = 0; wv < NW; ++wv) t += slot[wv];
            t = t * iw;
            const double grad = 2.0 * t + sc[4];
            if ((mode & SW_GOUT) && tid == 0) a.g_out[j] = grad;
            if (mode & SW_PFIN) {
                const double pf = sc[1] - a.c_p * grad;
                pp += pf * pf;
                if (!(mode & SW_SPEC) && tid == 0) a.p_out[j] = pf;
            }
            if (mode & SW_UPD) {
                const double psrc = (mode & SW_SPEC) ? sc[5] : sc[1];
                double pj = psrc - a.c_u * grad;
                xj = xj + a.dt * pj;
                const double hi = sc[3], lo = sc[2];
                if (xj > hi) {
                    xj = hi;
                    pj = -pj;
                } else if (xj < lo) {
                    xj = lo;
                    pj = -pj;
                }
                if (tid == 0) {
                    a.p_out[j] = pj;
                    a.x_out[j] = xj;
                }
            }
        }
        if (mode & SW_FWD) {
            const double xs = xj * iw;
#pragma unroll
            for (int k = 0; k < EPT; ++k)
                if (k < ept) dacc[k] += Ks[(size_t)k * T + tid] * xs;
        }
    }
    if ((mode & SW_PFIN) && tid == 0) a.pp_part[blockIdx.x] = pp;
    if (mode & SW_FWD) {
        double *out = a.slab + (int64_t)blockIdx.x * a.ld;
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
            const int64_t i = tid + (int64_t)k * T;
            if (i < a.ld) out[i] = dacc[k];
        }
    }
    if (stats) {
        unsigned long long e = nent;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) e += __shfl_xor(e, off, WAVE);
        if (lane == 0) {
            atomicAdd(&stats->entries, e);
            atomicAdd(&stats->leaves, e);
        }
    }
}

}  // namespace ghk
