// Chain batches on the translation-invariant store (lattice.hip.h): 16 chains per read of the table (gfx950).
//
// The single-chain passes of the table are FMA-issue and LDS bound: a thread's 64 FMAs of a step take 24 doubles
// from LDS, and a staged table value serves one chain.  With the chains of a batch as the third dimension the
// correlation of one (layer, output row, input row)
//     out[o][c] = sum_i row[i - o + const] in[i][c]                c = chain slot 0 .. 15
// is a product of a Toeplitz matrix with a 16-column matrix, and v_mfma_f64_16x16x4 does it:
//     A (16 outputs x 4 inputs)   the Toeplitz block of the staged table row: lane (m, kk) reads row[i0 + kk - o0 - m]
//                                 -- one double at a per-lane address, 19 distinct consecutive doubles per wave
//     B (4 inputs x 16 chains)    in[i0 + kk][c]: 64 contiguous doubles per wave
// 2 LDS doubles per lane for 16 FMAs per lane without any reuse; a wave owns LATB_RW output rows x up to LATB_NT
// tiles of 16 outputs and reuses B for all of them: 9 LDS doubles per 128 FMAs per lane (the single-chain pass: 48).
// fp64 MFMA runs at the vector rate on this chip, so the gain is LDS traffic and issue slots: one MFMA
// instruction per 1024 FMAs, no address arithmetic per chain.
//
// Partition (host_lattice.h: latb_plan), as lat_pass_kernel's: per (layer | chunk of layers, tile of LATB_TR output
// rows, range of tiles of the fast axis), all input rows in turn.  Workgroup = 4 waves, wave w the output rows
// row0 + 2 w, + 1; no sum over waves.  LDS per input row: the LATB_TR table rows of the (output row, input row)
// pairs, WL = NFip + WT values each (WT = 16 x the most tiles a workgroup has), and the input row, NFip x 16.
// Plain launches, no waits between workgroups.  Every sum runs in an order fixed by indices alone (layers, input
// rows, inputs ascending) and column c of an MFMA result depends on column c of B alone: a chain's result does not
// depend on what the other slots hold, and results are reproducible bit for bit.
//
// The adjoint ends with the batch's per-chain update: mfb_adjoint_kernel's arithmetic per (cell, chain), through
// mfb_update.  Included after mfbatch.hip.h (rt_offset, mfb_update).
//
// A third form serves the bootstrap batch (bscg.hip.h) on a gh_set_translation_invariant replicates table: the same
// adjoint over the table for 16 replicate slots, ending with bscg_adjoint_kernel's epilogue -- the CG gradient I and
// the workgroup's partial of |I|^2 per slot -- instead of the leapfrog update.  It is an instantiation of the one
// kernel: the epilogue's arguments are a type the form selects (LatbEpi), so that the chain forms' signature and
// statements are what they were and their registers with them (the numbers of the three).  Included after
// bscg.hip.h (BscgState, bscg_ms_grad).
//
// Row blocks (the multi-component store on the table asked for with gh_set_cells_multi_table_chains; lattice.hip.h:
// LatBlocks, nb tables T[b], block-major): two more instantiations of the one kernel, LATB_FWD_MB and LATB_ADJ_MB, added
// the way the CG form was -- their arguments (LatbBlockArgs) are again the epilogue's type, and the three forms above
// keep their signature, statements and registers (DESIGN 4.21, row "chains on blocks": the numbers of the five).  The forward takes the block as
// blockIdx.z under one gather of X, contracts T[b] and writes slab[chunk][b Nb + obs][16] times w_b; the adjoint, on the
// single block's grid, runs the input rows of block 0, 1, ... nb - 1 into the SAME accumulators -- rl16[b] (w_b r of
// block b) against T[b] -- before the one update.  The blocks take turns in the tile: the LDS is the single block's.
// Order of the sums: blocks, input rows, inputs ascending.
#pragma once

namespace ghk {

constexpr int LATB_THREADS = 256;
constexpr int LATB_RW = 2;              // output rows per wave
constexpr int LATB_TR = 4 * LATB_RW;    // output rows per workgroup
constexpr int LATB_NT = 4;              // tiles of 16 outputs per wave and output row, at most
constexpr int LATB_MAX_CHUNKS = 32;     // forward: slab rows at most

struct LatbPlan {
    int ntiles;  // tiles of 16 outputs along the fast axis
    int FT;      // workgroups along the fast axis: workgroup ft owns the tiles [ft ntiles / FT, (ft + 1) ntiles / FT)
    int WT;      // 16 x the most tiles of a workgroup
    int WL;      // staged values per table row: NFip + WT
    int lpc;     // forward: layers per chunk (slab row); adjoint: 1
};

// The CG epilogue's arguments (bscg.hip.h: BscgAdjArgs without the dense operands)
struct LatbCgArgs {
    const double *X;       // M x 16
    const double *wm2;     // M
    double beta2;
    const BscgState *st;
    double *I;             // M x 16
    double *nI2_part;      // (adjoint workgroups) x 16
};

// The chain batch's arguments on the table of row blocks (lattice.hip.h: LatBlocks): the leapfrog update's, and the blocks
struct LatbBlockArgs {
    BatchAdjArgs a;
    LatBlocks bl;
};

// What follows the contraction.  LATB_FWD: the slab; LATB_ADJ: the chain batch's leapfrog update; LATB_CG: the
// bootstrap batch's gradient.  LATB_ADJ_MB, LATB_FWD_MB: the two chain forms over row blocks (below)
enum { LATB_ADJ = 0, LATB_FWD = 1, LATB_CG = 2, LATB_ADJ_MB = 3, LATB_FWD_MB = 4 };
template <int FORM> struct LatbEpi { typedef BatchAdjArgs type; };
template <> struct LatbEpi<LATB_CG> { typedef LatbCgArgs type; };
template <> struct LatbEpi<LATB_ADJ_MB> { typedef LatbBlockArgs type; };
template <> struct LatbEpi<LATB_FWD_MB> { typedef LatbBlockArgs type; };

// (the leapfrog update's arguments of a chain form)
__device__ __forceinline__ const BatchAdjArgs &latb_update_args(const BatchAdjArgs &a) { return a; }
__device__ __forceinline__ const BatchAdjArgs &latb_update_args(const LatbBlockArgs &a) { return a.a; }

// X[M][16] (the caller's cell order) times iw -> xl16[nz][nx][nyp][16] (zero beyond ny), as mfb_forward_kernel scales X
__global__ void __launch_bounds__(256) latb_gather_x_kernel(LatGeom l, const double *X, const double *iw, double *xl16)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t e = t >> 4;
    const int c = (int)(t & 15);
    if (e >= (int64_t)l.nz * l.nx * l.ny) return;
    const int64_t row = e / l.ny;
    const int b = (int)(e - row * l.ny);
    const int64_t j = l.cell_of[e];
    xl16[(row * l.nyp + b) * CB + c] = X[j * CB + c] * iw[j];
}

// Rt (patch-transposed residuals of the batch, the caller's observation order) -> rl16[b][p][q][c] = w_b Rt[b Nb +
// obs_of[p, q]][c] (zero beyond qy), the bl.n blocks of r; the single table: one block of weight 1, rl16[px][qyp][16]
__global__ void __launch_bounds__(256) latb_gather_r_blocks_kernel(LatGeom l, LatBlocks bl, const double *Rt, double *rl16)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t e = t >> 4;
    const int c = (int)(t & 15);
    const int64_t PQ = (int64_t)l.px * l.qy;
    if (e >= PQ * bl.n) return;
    const int b = (int)(e / PQ);
    const int64_t pq = e - (int64_t)b * PQ;
    const int p = (int)(pq / l.qy), q = (int)(pq - (int64_t)p * l.qy);
    rl16[(((int64_t)b * l.px + p) * l.qyp + q) * CB + c] = bl.w[b] * Rt[rt_offset(b * bl.Nb + l.obs_of[pq], c)];
}

// One pass over the table for all 16 chain slots.  FWD: in16 = xl16, blockIdx.y = chunk of pl.lpc layers,
// slab[chunk][obs][16] takes the partial forward product (a: not read); else in16 = rl16, blockIdx.y = layer, and
// the (cell, chain) pairs' update follows the dots (pp_part[(blockIdx.y * gridDim.x + blockIdx.x)][16]).
// blockIdx.x = (tile of output rows) * pl.FT + range of tiles of the fast axis.
// Dynamic LDS: (LATB_TR pl.WL + 16 NFip) doubles = 192 NFip + 64 pl.WT bytes, and no static LDS: what the plan checks
// against the 160 KB of a workgroup is all the kernel asks for.
// FORM = LATB_CG: the adjoint's grid and operands; per (cell jc, slot c) with the correlation s
//     I[jc][c] = 2 s iw[jc] + alpha_c g_MS(X[jc][c])          where st[c].live, else I keeps what it holds
// and the workgroup's partial of |I|^2 per slot in row blockIdx.y * gridDim.x + blockIdx.x of a.nI2_part (zero for a
// slot that is not live), summed as the chain form sums |p|^2: through the tile, waves, then the four lane groups.
// FORM = LATB_FWD_MB / LATB_ADJ_MB: the chain forms over the row blocks a.bl.  Forward: blockIdx.z = block b, T[b], outputs
// to slab[chunk][b Nb + obs][16] times w_b; adjoint: in16 = rl16[nb][px][qyp][16], the input rows of every block in turn
// against T[b], then the update (a.a).
template <int FORM>
__global__ void __launch_bounds__(LATB_THREADS)
latb_pass_kernel(LatGeom g, LatbPlan pl, const double *__restrict__ in16, typename LatbEpi<FORM>::type a,
                 const double *__restrict__ iw, double *__restrict__ slab, int64_t ld)
{
    constexpr bool FWD = FORM == LATB_FWD || FORM == LATB_FWD_MB;
    constexpr bool MB = FORM == LATB_ADJ_MB || FORM == LATB_FWD_MB;
    extern __shared__ __attribute__((aligned(16))) double latb_lds[];  // (the kernel's only LDS: the plan's bytes are all of it)
    const int NRo = FWD ? g.px : g.nx, NFo = FWD ? g.qy : g.ny;
    const int NRi = FWD ? g.nx : g.px, NFip = FWD ? g.nyp : g.qyp;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = lane & 15, kk = lane >> 4;
    const int rt = (int)(blockIdx.x / pl.FT), ft = (int)(blockIdx.x % pl.FT);
    const int row0 = rt * LATB_TR;
    const int t0 = ft * pl.ntiles / pl.FT, t1 = (ft + 1) * pl.ntiles / pl.FT;
    const int nt = t1 - t0, ot0 = 16 * t0;
    const int WT = pl.WT, WL = pl.WL;
    double *tabs = latb_lds;
    double *ins = tabs + LATB_TR * WL;
    const int k0 = FWD ? (int)blockIdx.y * pl.lpc : (int)blockIdx.y;
    const int k1 = FWD ? min(g.nz, k0 + pl.lpc) : k0 + 1;
    const int nin = NFip * CB;

    d4 acc[LATB_RW][LATB_NT];
#pragma unroll
    for (int r = 0; r < LATB_RW; ++r)
#pragma unroll
        for (int t = 0; t < LATB_NT; ++t) acc[r][t] = d4{0.0, 0.0, 0.0, 0.0};

    // (row blocks: the adjoint's blocks in turn, the forward's one block)
    int b0 = 0, b1 = 1;
    if constexpr (MB) {
        b0 = FWD ? (int)blockIdx.z : 0;
        b1 = FWD ? b0 + 1 : a.bl.n;
    }
    // the lane's A operand of (output row r, tile t) at step i0: staged value i - o + ot0 + WT - 1 with i = i0 + kk,
    // o = ot0 + 16 t + m
    const double *abase = tabs + (w * LATB_RW) * WL + (kk - m + WT - 1);
    for (int k = k0; k < k1; ++k)
    for (int blk = b0; blk < b1; ++blk) {  // (one block but in the adjoint over row blocks: the loop's bounds are constants)
        const double *Tk = g.T + (MB ? (int64_t)blk * g.nz + k : (int64_t)k) * g.U * g.V;
        const double *inl = FWD ? in16 + (int64_t)k * g.nx * nin : MB ? in16 + (int64_t)blk * g.px * nin : in16;
        for (int ir = 0; ir < NRi; ++ir) {
            __syncthreads();  // (the previous input row's reads of tabs / ins)
            // (wave w stages the table rows w, w + 4; a lane the values lane, lane + 64, ...)
            for (int r = w; r < LATB_TR; r += 4) {
                const int u = FWD ? (row0 + r) - ir + g.nx - 1 : ir - (row0 + r) + g.nx - 1;
                const bool uok = u >= 0 && u < g.U;
                const double *Tu = Tk + (int64_t)(uok ? u : 0) * g.V;
                for (int wl = lane; wl < WL; wl += 64) {
                    const int d = wl - ot0 - WT + 1;  // i - o
                    const int v = (FWD ? -d : d) + g.ny - 1;
                    tabs[r * WL + wl] = (uok && v >= 0 && v < g.V) ? Tu[v] : 0.0;
                }
            }
            const double *inr = inl + (int64_t)ir * nin;
            for (int e = tid; e < nin; e += LATB_THREADS) ins[e] = inr[e];
            __syncthreads();
            for (int i0 = 0; i0 < NFip; i0 += 4) {
                const double bv = ins[i0 * CB + lane];  // in[i0 + kk][m]
#pragma unroll
                for (int r = 0; r < LATB_RW; ++r)
#pragma unroll
                    for (int t = 0; t < LATB_NT; ++t)
                        if (t < nt) acc[r][t] = mfma_f64(abase[r * WL + i0 - 16 * t], bv, acc[r][t]);
            }
        }
    }

    // acc[r][t][q] of lane (m, kk): output row row0 + 2 w + r, output ot0 + 16 t + kk + 4 q, chain m
    const int c = m;
    double pp = 0.0;
    // (the CG form: the slot's state, read once)
    bool live = false;
    double alpha = 0.0;
    if constexpr (FORM == LATB_CG) {
        live = a.st[c].live != 0;
        alpha = a.st[c].alpha;
    }
#pragma unroll
    for (int r = 0; r < LATB_RW; ++r) {
        const int orow = row0 + w * LATB_RW + r;
#pragma unroll
        for (int t = 0; t < LATB_NT; ++t) {
            if (t >= nt || orow >= NRo) continue;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int o = ot0 + 16 * t + kk + 4 * q;
                if (o >= NFo) continue;
                if constexpr (FWD && MB) {
                    slab[((int64_t)blockIdx.y * ld + b0 * a.bl.Nb + g.obs_of[(int64_t)orow * g.qy + o]) * CB + c] =
                        acc[r][t][q] * a.bl.w[b0];
                } else if constexpr (FWD) {
                    slab[((int64_t)blockIdx.y * ld + g.obs_of[(int64_t)orow * g.qy + o]) * CB + c] = acc[r][t][q];
                } else if constexpr (FORM == LATB_CG) {
                    // (bscg_adjoint_kernel's arithmetic per cell and replicate; a slot that is not live keeps its I)
                    if (!live) continue;
                    const int64_t jc = g.cell_of[((int64_t)k0 * g.nx + orow) * g.ny + o];
                    const int64_t idx = jc * CB + c;
                    double s = acc[r][t][q];
                    s = s * iw[jc];
                    const double gI = 2.0 * s + alpha * bscg_ms_grad(a.X[idx], a.wm2[jc], a.beta2);
                    a.I[idx] = gI;
                    pp += gI * gI;
                } else {
                    // (mfb_adjoint_kernel's arithmetic per cell and chain)
                    const int64_t jc = g.cell_of[((int64_t)k0 * g.nx + orow) * g.ny + o];
                    const int64_t idx = jc * CB + c;
                    double s = acc[r][t][q];
                    s = s * iw[jc];
                    const BatchAdjArgs &ua = latb_update_args(a);
                    (void)mfb_update(ua, idx, jc, c, 2.0 * s + (ua.GREG ? ua.GREG[idx] : 0.0), true, pp);
                }
            }
        }
    }
    if constexpr (!FWD) {
        // the 16 lanes-of-a-chain of the workgroup, in wave and lane order, through the tile nobody reads any more
        // (256 doubles; the smallest tile is 8 x 24 + 16 x 8 = 320)
        double *ppred = latb_lds;
        __syncthreads();  // (the other waves' last reads of tabs / ins)
        ppred[w * 64 + lane] = pp;
        __syncthreads();
        bool wanted;
        double *part;
        if constexpr (FORM == LATB_CG) {
            wanted = tid < CB;  // (every slot's row is written: bscg_mu_kernel reads the live ones)
            part = a.nI2_part;
        } else {
            const BatchAdjArgs &ua = latb_update_args(a);
            wanted = ua.pp_part && tid < CB && (ua.phase[tid] == PH_PFIN || ua.phase[tid] == PH_PFIN_SPEC);
            part = ua.pp_part;
        }
        if (wanted) {
            double s = 0.0;
#pragma unroll
            for (int ww = 0; ww < 4; ++ww)
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) s += ppred[ww * 64 + gq * 16 + tid];
            part[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * CB + tid] = s;
        }
    }
}

}  // namespace ghk
