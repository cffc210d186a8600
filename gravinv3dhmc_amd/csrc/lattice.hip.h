// Translation-invariant store for regular prism grids under gridded data (gfx950): the Cartesian counterpart
// of the shift-invariant table of the spherical grids (lonsym.hip.h).
//
// Cells: the full product of nx x-intervals of one width hx, ny y-intervals of one width hy and nz layers,
// cell (k, a, b).  Observations: a full px x qy rectangle of the lattice x = xo + p hx, y = yo + q hy at one
// height, observation (p, q).  Every prism field of such a pair depends on (k, p - a, q - b) alone, so the whole
// kernel is
//     K[(p, q), (k, a, b)] = T[k][u][v]      u = p - a + nx - 1 in [0, U),  v = q - b + ny - 1 in [0, V)
// with U = nx + px - 1, V = ny + qy - 1: nz U V doubles (cells 100 x 100 x 50 under 100 x 100 observations:
// 15.8 MB instead of 40 GB), L2 / Infinity-Cache resident.  lat_fill_kernel evaluates each entry with the entry
// functions of the dense assembly (mf_entry<E>) on the pair with the smallest (p, q) that has the offset, from
// the caller's coordinates: the entry IS the dense store's entry of that pair.
//
// Both products are correlations along the fast lattice axis, per (layer, cell row a, observation row p):
//     adjoint   g[k,a,b] = sum_p sum_q T[k][p-a+nx-1][q-b+ny-1] r[p,q]
//     forward   d[p,q]   = sum_k sum_a sum_b T[k][p-a+nx-1][q-b+ny-1] xs[k,a,b]        xs = x / wm
// and lat_pass_kernel<FWD, MB> is ONE kernel for both: "output rows" (a | p) of NFo outputs (b | q), "input rows"
// (p | a) of NFi inputs (q | b); the forward reads the table row backwards, which turns it into the adjoint's
// form  out[o] = sum_i row[i - o + const] in[i].  Plain launches, no waits between workgroups.
//
// Tiling.  One value from L2 per FMA would move the dense store's 40 GB through L2 instead of HBM, one value
// from LDS per FMA is capped by the LDS array at 8-32 doubles per clock and CU against 64 fp64 FMAs.  So the
// correlation is register-blocked as a sliding window: a thread owns R = 8 consecutive outputs and consumes
// S = 8 consecutive inputs per step; the 64 FMAs of a step need R + S - 1 = 15 consecutive table values (16
// are read: four ds_read_b128 pairs) and 8 inputs, 24 doubles from LDS -- 2.7 FMAs per LDS double, and the
// input reads are one address per wave (broadcast).  R = S = 8 costs 16 + 32 + 16 VGPRs for accumulators,
// window and inputs: the kernel compiles to 64 VGPRs, so the waves a CU holds are set by the LDS tile (five
// workgroups at the shape below) and the LDS latency is hidden by the other waves, not by unrolling; R = S = 16
// would double the FMAs per LDS double at four times the registers.  Measured: 21 - 33 TFLOP/s,
// 27 - 42 % of the fp64 vector peak.
//   workgroup  256 threads = 4 waves.  A wave's 64 lanes are 64 output blocks: TR output rows x nobt blocks of 8
//              outputs (nobt = min(64, ceil(NFo / 8)), TR = 64 / nobt; a fast axis longer than 512 outputs is
//              split over FT workgroups).  The four waves take four consecutive INPUT rows, so the input row is
//              uniform in a wave, and their partial sums are added in wave order at the end.
//   LDS        per step of four input rows: the TR + 3 table rows the (output row, input row) pairs share, WL =
//              NFi8 + 8 nobt values each, and the four input rows; 16 KB for the final sum over the waves.
//              Cells 100 x 100 under 100 x 100 observations: 7 x 208 + 4 x 104 + 2048 doubles = 31 KB, five
//              workgroups per CU.
//   banks      lanes of neighbouring output blocks read windows 64 B apart: read straight, the 16 lanes of a
//              ds_read_b128 group would fall on four 256-B bank rows (4-way conflict).  A table row is therefore
//              kept as four planes: the t-th 16-byte piece of every 64-byte block in plane t, so that
//              neighbouring lanes read neighbouring 16-byte slots.
// Every sum runs in an order fixed by indices alone (inputs ascending inside a row, input rows of a wave
// ascending, layers ascending, waves 0..3): results are reproducible bit for bit.  The update arithmetic behind
// the adjoint is mf_adjoint_kernel's, expression for expression.
//
// Row blocks (the multi-component store on the table, gh_set_cells_multi_table): nb components of the same cells at the
// same points are nb tables T[b][k][u][v], block-major, each the unweighted table of its field; the data weights w_b
// are not in them.  rl is [b][p][.] = w_b r of block b, the forward multiplies a finished output sum by w_b.  The
// adjoint (MB) runs the steps of four input rows block after block into the SAME accumulators -- a step never mixes
// two blocks, the rows past px of a block's last step are zeros -- then the one cell update; the forward takes the
// block as blockIdx.z and shares xl.  The LDS tile is the single block's.  Order of the sums: block, input row, input.
//
// Block-diagonal layers (BD; the joint gravity-magnetic store on the table, gh_set_cells_joint_table; latjoint.hip.h):
// the table has 2 nz layers, layer L = b nz + k the field b (0 gz, 1 tf) of a unit property b in the geometry's layer
// k, and layer L meets the observation block L / nz ALONE.  rl is [2][p][.] = w_b r of block b.  The adjoint's workgroup
// of layer L reads rl[L / nz] where the other forms read rl[0]; the forward's chunks of layers never cross the
// boundary between the properties: gridDim.y / 2 chunks each, chunk c of property b the layers b nz + c lpc ..., its
// partial sum times w_b into slab row blockIdx.y -- the first half of the slab rows sums to d of block 0, the second
// to d of block 1, each row c->ld long (the block's own).  Everything else is the single block's pass.
#pragma once

namespace ghk {

constexpr int LAT_R = 8;        // outputs per thread = inputs per step
constexpr int LAT_G = 4;        // waves of a workgroup = input rows per step
constexpr int LAT_THREADS = 256;

struct LatGeom {
    int nx, ny, nz, px, qy;
    int U, V;             // nx + px - 1, ny + qy - 1
    int nyp, qyp;         // ny, qy rounded up to 8
    const double *T;      // [nz][U][V] (row blocks: [nb][nz][U][V])
    const int *cell_of;   // [nz][nx][ny]: the caller's cell
    const int *obs_of;    // [px][qy]: the caller's observation
    double *rl;           // [px][qyp]: r in lattice order (zero beyond qy); row blocks: [nb][px][qyp], w_b r
    double *xl;           // [nz][nx][nyp]: x / wm in lattice order (zero beyond ny)
};

// The n blocks of r, Nb observations apart, block b times w[b] (host_lattice.h: lattice_r_blocks) -- or, for the column
// norms, the n tables of a layer (lattice_tables).  The scalar table: one of weight 1
struct LatBlocks {
    int n;
    int64_t Nb;
    double w[MULTI_MAX];
};

// partition of one pass (host_lattice.h: lat_plan)
struct LatPlan {
    int nobt;   // output blocks of 8 per output row and workgroup (<= 64)
    int TR;     // output rows per workgroup
    int FT;     // workgroups along the fast axis
    int WL;     // staged values per table row: NFi8 + 8 nobt
    int lpc;    // forward: layers per chunk (slab row); adjoint: 1
};

// T[k][u][v] from the pair with the smallest (p, q) of offset (u, v); T2: from the pair with the largest
template <int E>
__global__ void __launch_bounds__(256) lat_fill_kernel(MfGeom g, LatGeom l, double *T, double *T2)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t UV = (int64_t)l.U * l.V;
    if (e >= UV * l.nz) return;
    const int k = (int)(e / UV);
    const int u = (int)((e - k * UV) / l.V), v = (int)(e - k * UV - (int64_t)u * l.V);
    const int du = u - (l.nx - 1), dv = v - (l.ny - 1);  // p - a, q - b
    const int p0 = du > 0 ? du : 0, q0 = dv > 0 ? dv : 0;
    const int p1 = min(l.px - 1, du + l.nx - 1), q1 = min(l.qy - 1, dv + l.ny - 1);
    {
        const int64_t i = l.obs_of[(int64_t)p0 * l.qy + q0];
        const int64_t j = l.cell_of[((int64_t)k * l.nx + (p0 - du)) * l.ny + (q0 - dv)];
        T[e] = mf_entry<E>(g, i, g.bounds6 + 6 * j);
    }
    {
        const int64_t i = l.obs_of[(int64_t)p1 * l.qy + q1];
        const int64_t j = l.cell_of[((int64_t)k * l.nx + (p1 - du)) * l.ny + (q1 - dv)];
        T2[e] = mf_entry<E>(g, i, g.bounds6 + 6 * j);
    }
}

// wm_j = (sum_b w_b^2 sum over the cell's px x qy window of T_b^2)^wf: thread = cell in lattice order, the bl.n tables of
// its layer ascending.  One table of weight 1 is the single table's norm bit for bit: 0 + (1 * 1) s == s, fused or not
__global__ void __launch_bounds__(256) lat_colnorm_blocks_kernel(LatGeom l, LatBlocks bl, double wf, double *wm)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)l.nz * l.nx * l.ny) return;
    const int b = (int)(e % l.ny), a = (int)((e / l.ny) % l.nx), k = (int)(e / ((int64_t)l.ny * l.nx));
    double st = 0.0;
    for (int blk = 0; blk < bl.n; ++blk) {
        const double *Tk = l.T + ((int64_t)blk * l.nz + k) * l.U * l.V;
        double s = 0.0;
        for (int p = 0; p < l.px; ++p) {
            const double *row = Tk + (int64_t)(p - a + l.nx - 1) * l.V + (l.ny - 1 - b);
            for (int q = 0; q < l.qy; ++q) s += row[q] * row[q];
        }
        st += (bl.w[blk] * bl.w[blk]) * s;
    }
    wm[l.cell_of[e]] = (wf == 0.5) ? sqrt(st) : pow(st, wf);
}

// r (the caller's order) -> rl[b][p][q] = w_b r[b Nb + obs_of[p, q]], the bl.n blocks of r (one block of weight 1: r itself)
__global__ void __launch_bounds__(256) lat_gather_r_blocks_kernel(LatGeom l, LatBlocks bl, const double *r)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t PQ = (int64_t)l.px * l.qy;
    if (e >= PQ * bl.n) return;
    const int b = (int)(e / PQ);
    const int64_t o = e - b * PQ;
    const int p = (int)(o / l.qy), q = (int)(o - (int64_t)p * l.qy);
    l.rl[((int64_t)b * l.px + p) * l.qyp + q] = bl.w[b] * r[b * bl.Nb + l.obs_of[o]];
}

// x / wm (the caller's order; wm: or nullptr, the unweighted kernel) -> xl, as mf_forward_kernel scales x
__global__ void __launch_bounds__(256) lat_gather_x_kernel(LatGeom l, const double *x, const double *wm)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)l.nz * l.nx * l.ny) return;
    const int64_t row = e / l.ny;
    const int b = (int)(e - row * l.ny);
    const int64_t j = l.cell_of[e];
    const double w = wm ? wm[j] : 1.0;
    l.xl[row * l.nyp + b] = (w != 0.0) ? x[j] * (1.0 / w) : x[j];
}

// One pass over the table.  FWD: blockIdx.y = chunk of pl.lpc layers, slab[chunk][i] takes the partial forward
// product; else blockIdx.y = layer, and the cells' update follows the dots (a.mode: SW_ADJ with SW_UPD / SW_PFIN /
// SW_SPEC / SW_GOUT as in mf_adjoint_kernel; pp_part[blockIdx.y * gridDim.x + blockIdx.x]).  blockIdx.x =
// (tile of output rows) * pl.FT + tile of the fast axis.  Dynamic LDS: (pl.TR + 3) pl.WL + 4 NFi8 + 2048 doubles.
// MB: row blocks (bl).  FWD: blockIdx.z = block, outputs to slab[chunk][b Nb + obs] times w_b; else the steps of four
// input rows run block after block over rl[b] with T[b], before the one update.  !MB: bl is not read.
// BD (with !MB): block-diagonal layers, see the head of the file; bl.w[b] weighs the forward of property b.
template <bool FWD, bool MB, bool BD = false>
__global__ void __launch_bounds__(LAT_THREADS) lat_pass_kernel(LatGeom g, LatPlan pl, SweepArgs a, const double *wm,
                                                               int64_t ld, LatBlocks bl)
{
    extern __shared__ __attribute__((aligned(16))) double lat_lds[];
    __shared__ double ppred[LAT_G];
    const int NRo = FWD ? g.px : g.nx, NFo = FWD ? g.qy : g.ny;
    const int NRi = FWD ? g.nx : g.px, NFip = FWD ? g.nyp : g.qyp;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int nobt = pl.nobt, TR = pl.TR, WL = pl.WL;
    const int row0 = (int)(blockIdx.x / pl.FT) * TR, ot0 = (int)(blockIdx.x % pl.FT) * nobt * LAT_R;
    const int tnp = nobt * LAT_R;
    const int TRW = TR + LAT_G - 1;  // table rows the TR x 4 (output row, input row) pairs of a step share
    const int nb2 = WL / 4;          // doubles per plane of a staged table row
    double *tabs = lat_lds;
    double *ins = tabs + TRW * WL;
    double *red = ins + LAT_G * NFip;
    const int orow = lane / nobt, ob = lane - orow * nobt;
    const bool act = orow < TR;
    static_assert(!(MB && BD), "block-diagonal layers are a form of the single table");
    // (BD: nzl layers per property; the forward's property and its chunk from blockIdx.y)
    const int nzl = BD ? g.nz / 2 : g.nz;
    const int prop = (BD && FWD) ? (int)blockIdx.y / ((int)gridDim.y / 2) : 0;
    const int kb = (BD && FWD) ? prop * nzl + ((int)blockIdx.y - prop * ((int)gridDim.y / 2)) * pl.lpc : 0;
    const int k0 = (BD && FWD) ? kb : FWD ? (int)blockIdx.y * pl.lpc : (int)blockIdx.y;
    const int k1 = (BD && FWD) ? min((prop + 1) * nzl, k0 + pl.lpc) : FWD ? min(g.nz, k0 + pl.lpc) : k0 + 1;

    double acc[LAT_R];
#pragma unroll
    for (int rr = 0; rr < LAT_R; ++rr) acc[rr] = 0.0;

    // (the adjoint's blocks in turn, the forward's one block)
    const int b0 = (MB && FWD) ? (int)blockIdx.z : 0;
    const int b1 = (MB && !FWD) ? bl.n : b0 + 1;
    for (int k = k0; k < k1; ++k) {
        for (int blk = b0; blk < b1; ++blk) {
            const double *Tk = g.T + ((int64_t)blk * g.nz + k) * g.U * g.V;
            const double *inl = FWD ? g.xl + (int64_t)k * g.nx * g.nyp
                                    : g.rl + (int64_t)(BD ? k / nzl : blk) * g.px * g.qyp;
            for (int ir0 = 0; ir0 < NRi; ir0 += LAT_G) {
                __syncthreads();  // (the previous step's reads of tabs / ins)
                // table rows u_lo .. u_lo + TRW - 1; staged index wl <-> v (the forward reads the row backwards)
                const int u_lo = FWD ? row0 - (ir0 + LAT_G - 1) + g.nx - 1 : ir0 - row0 - TR + g.nx;
                for (int e = tid; e < TRW * WL; e += LAT_THREADS) {
                    const int ur = e / WL, wl = e - ur * WL;
                    const int u = u_lo + ur;
                    const int v = FWD ? ot0 - wl + tnp + g.ny - 2 : wl - tnp - ot0 + g.ny;
                    const double val = (u >= 0 && u < g.U && v >= 0 && v < g.V) ? Tk[(int64_t)u * g.V + v] : 0.0;
                    tabs[ur * WL + ((wl >> 1) & 3) * nb2 + 2 * (wl >> 3) + (wl & 1)] = val;
                }
                for (int e = tid; e < LAT_G * NFip; e += LAT_THREADS) {
                    const int gi = e / NFip, i = e - gi * NFip;
                    ins[e] = (ir0 + gi < NRi) ? inl[(int64_t)(ir0 + gi) * NFip + i] : 0.0;
                }
                __syncthreads();
                if (act) {
                    const int ur = FWD ? orow - w + LAT_G - 1 : w - orow + TR - 1;
                    const double *trow = tabs + ur * WL;
                    const double *in = ins + w * NFip;
                    for (int i0 = 0; i0 < NFip; i0 += LAT_R) {
                        // the window: staged values 8 B0 .. 8 B0 + 15 (tw[t] pairs with input s and output rr = s + 7 - t)
                        const int B0 = (i0 >> 3) - ob + nobt - 1;
                        double tw[2 * LAT_R], iv[LAT_R];
    #pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const d2 lo = *reinterpret_cast<const d2 *>(trow + t * nb2 + 2 * B0);
                            const d2 hi = *reinterpret_cast<const d2 *>(trow + t * nb2 + 2 * B0 + 2);
                            tw[2 * t] = lo.x;
                            tw[2 * t + 1] = lo.y;
                            tw[8 + 2 * t] = hi.x;
                            tw[8 + 2 * t + 1] = hi.y;
                            const d2 vi = *reinterpret_cast<const d2 *>(in + i0 + 2 * t);
                            iv[2 * t] = vi.x;
                            iv[2 * t + 1] = vi.y;
                        }
    #pragma unroll
                        for (int s = 0; s < LAT_R; ++s)
    #pragma unroll
                            for (int rr = 0; rr < LAT_R; ++rr) acc[rr] += tw[s - rr + LAT_R - 1] * iv[s];
                    }
                }
            }
        }
    }

    // the four waves' partial sums, added in wave order
#pragma unroll
    for (int rr = 0; rr < LAT_R; ++rr) red[(w * 64 + lane) * LAT_R + rr] = acc[rr];
    __syncthreads();
    const int mode = a.mode;
    double pp = 0.0;
    for (int h = 0; h < 2; ++h) {
        const int e = tid + h * LAT_THREADS;
        const int slot = e >> 3, rr = e & 7;
        const int so = slot / nobt, sb = slot - so * nobt;
        const int orow_abs = row0 + so, o = ot0 + sb * LAT_R + rr;
        if (so >= TR || orow_abs >= NRo || o >= NFo) continue;
        double s = ((red[slot * LAT_R + rr] + red[(64 + slot) * LAT_R + rr]) + red[(128 + slot) * LAT_R + rr]) +
                   red[(192 + slot) * LAT_R + rr];
        if (FWD) {
            if (MB)
                a.slab[(int64_t)blockIdx.y * ld + b0 * bl.Nb + g.obs_of[(int64_t)orow_abs * g.qy + o]] = s * bl.w[b0];
            else if (BD)
                a.slab[(int64_t)blockIdx.y * ld + g.obs_of[(int64_t)orow_abs * g.qy + o]] = s * bl.w[prop];
            else
                a.slab[(int64_t)blockIdx.y * ld + g.obs_of[(int64_t)orow_abs * g.qy + o]] = s;
        } else {
            // (mf_adjoint_kernel's arithmetic per cell)
            const int64_t j = g.cell_of[((int64_t)k0 * g.nx + orow_abs) * g.ny + o];
            const double wj = wm[j];
            s = (wj != 0.0) ? s * (1.0 / wj) : s;
            const double gr = a.greg ? a.greg[j] : 0.0;
            const double grad = 2.0 * s + gr;
            if (mode & SW_GOUT) a.g_out[j] = grad;
            if (mode & SW_PFIN) {
                const double pf = a.p_in[j] - a.c_p * grad;
                pp += pf * pf;
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
    }
    if (!FWD && (mode & SW_PFIN)) {
        pp = wave_allreduce_sum(pp);
        if (lane == 0) ppred[w] = pp;
        __syncthreads();
        if (tid == 0) a.pp_part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = ((ppred[0] + ppred[1]) + ppred[2]) + ppred[3];
    }
}

}  // namespace ghk
