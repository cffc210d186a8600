// Folded store of a prism gz kernel whose cells and observations are symmetric under the two mirrors
// x -> 2cx - x and y -> 2cy - y (host_fold.h detects them).  Included once by gravhmc.hip.
//
// The group {e, sx, sy, sxy}, indexed g = 0..3 with composition g ^ h, acts freely on both sides and
// G(s_g i, s_g j) = G(i, j), so a quarter of G is distinct.  With F the fundamental observations (one per
// orbit, obs_img[f][g] = index of s_g f) and the cell orbits (cell_orbit[o][k] = index of s_k j_o):
//
//     S[o][f][k] = mean over g of Aw(s_g f, s_g s_k j_o)          f < nF, rows padded to ldF (zeros)
//
// one block of 4 ldF doubles per cell orbit, the four sub-columns of an observation side by side.  For the
// cells s_h j_o of the orbit and the observations s_g f:
//
//     dot[h]      += sum_k S[o][f][k] r[s_(k^h) f]        (adjoint)
//     dpart[s_g f] += sum_h S[o][f][g^h] x[s_h j_o]       (forward)
//
// 8 FMA per double read (2 in sweep_kernel), a quarter of the bytes per fused step.
#pragma once

namespace ghk {

struct FoldArgs {
    const double *S;         // n_orb x 4 ldF
    const int *obs_img;      // nF x 4
    const int *cell_orbit;   // n_orb x 4
    int nF, ldF;             // ldF: multiple of 16
    int64_t n_orb;
    int64_t orb_per_team;
    int n_pp;                // entries of pp_part (SW_PFIN): those past the grid are zeroed
    int64_t N;               // observations: slab rows N .. ld-1 are written as zeros
};

typedef const d2 __attribute__((address_space(1))) *gconst_d2ptr;

// S from the weighted dense store: one workgroup per orbit, the four entries of each orbit averaged in a
// fixed order.  dev_bits: max over the store of max_g |entry - mean| / (largest |mean| of the orbit's
// block), as the bits of a non-negative double (atomicMax on them orders like the values).
__global__ void __launch_bounds__(256) fold_build_kernel(const double *G, int64_t ld, FoldArgs f, double *S,
                                                         unsigned long long *dev_bits)
{
    __shared__ double red[2][4];
    const int64_t o = blockIdx.x;
    const int n = 4 * f.ldF;
    int co[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) co[g] = f.cell_orbit[4 * o + g];
    double dev = 0.0, amax = 0.0;
    for (int e = threadIdx.x; e < n; e += blockDim.x) {
        const int i = e >> 2, k = e & 3;
        double mean = 0.0;
        if (i < f.nF) {
            double v[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) v[g] = G[(int64_t)co[k ^ g] * ld + f.obs_img[4 * i + g]];
            mean = (((v[0] + v[1]) + v[2]) + v[3]) * 0.25;
#pragma unroll
            for (int g = 0; g < 4; ++g) dev = fmax(dev, fabs(v[g] - mean));
            amax = fmax(amax, fabs(mean));
        }
        S[o * n + e] = mean;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        dev = fmax(dev, __shfl_xor(dev, off, WAVE));
        amax = fmax(amax, __shfl_xor(amax, off, WAVE));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red[0][wave] = dev;
        red[1][wave] = amax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) {
            dev = fmax(dev, red[0][w]);
            amax = fmax(amax, red[1][w]);
        }
        const double rel = amax > 0.0 ? dev / amax : 0.0;
        atomicMax(dev_bits, (unsigned long long)__double_as_longlong(rel));
    }
}

__device__ __forceinline__ double readlane_d(double v, int l)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, l);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

template <int EPT2>
struct FoldCol {
    d2 v[EPT2];
    int j;        // cell h = (lane >> 3) & 3 of the orbit
    int jn;       // the same cell of the orbit this buffer takes next, two blocks on (requested behind this block)
    double cv;    // per-cell inputs, lane-distributed: lane 8h + q holds input q of cell h (FOLD_IN_*)
};

// the per-cell inputs of an orbit, one per lane 8h + q (h < 4): requested with the orbit's block (their cell
// indices one block earlier, all through the vector-memory counter), gathered into lane 8h by DPP after the dots
// are known.  No scalar load in the loop: an s_load would share lgkmcnt with the LDS reads of r and put its
// latency into every block's chain.
constexpr int FOLD_SLOT = 16 * 16 + 8;  // doubles (16 waves x 4 rows x 4 dots, padded)

enum { FOLD_IN_X = 0, FOLD_IN_P, FOLD_IN_GREG, FOLD_IN_HI, FOLD_IN_LO, FOLD_IN_PN, FOLD_IN_GACC, FOLD_IN_N };

// v of the lane DPP control CTRL selects (0 where there is none)
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double v)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xf, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

// v of lane l + Q of the same row of 16 (row_shl Q; 0 past the row's end)
template <int Q>
__device__ __forceinline__ double dpp_from_up(double v)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, 0x100 | Q, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), 0x100 | Q, 0xf, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

// One team of 16 waves per workgroup, one orbit block at a time (EPT2 double2 per thread: 2048 EPT2 rows
// of S), one block in flight ahead together with its cells' inputs (at C2: EPT2 = 5).  Every mode of sweep_kernel
// (SW_ADJ / UPD / FWD / PFIN / GOUT / GACC / SPEC, dsum) over a whole panel; M-vectors in the caller's cell order,
// the slab row in the caller's observation order.  Thread t holds double2 e = k 1024 + t of a block, i.e.
// S[o][e >> 1][2m], S[o][e >> 1][2m + 1] with m = t & 1: its adjoint terms u[q] = S[2m] r[s_q f] + S[2m+1] r[s_(q^1) f]
// belong to dot[q ^ 2m], its forward terms acc[q] = S[2m] x[q] + S[2m+1] x[q^1] to the observation s_(q^2m) f.
// The four cells' updates run side by side in lanes 0, 8, 16, 24 (the arithmetic of sweep_kernel per cell).
template <int EPT2>
__global__ void __launch_bounds__(1024) fold_sweep_kernel(SweepArgs a, FoldArgs f)
{
    constexpr int TT = 1024, NW = 16;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    // LDS: [0, 4 ldF) r at the four images of each fundamental observation; 2 x FOLD_SLOT ping-pong slots of
    // the four dots of an orbit (one per row of 16 lanes of every wave)
    double *rF = smem;
    double *scratch = smem + 4 * f.ldF;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int n2 = 2 * f.ldF;  // double2 per block
    const int mode = a.mode;

    if (mode & SW_ADJ) {
        for (int e = tid; e < 4 * f.ldF; e += TT) rF[e] = (e >> 2) < f.nF ? a.r[f.obs_img[e]] : 0.0;
    }
    __syncthreads();

    const int64_t ob = (int64_t)blockIdx.x * f.orb_per_team;
    int64_t oend = ob + f.orb_per_team;
    if (oend > f.n_orb) oend = f.n_orb;
    const int cnt = ob < oend ? (int)(oend - ob) : 0;

    d2 acc[EPT2][2];  // [k][0] = (acc[0], acc[1]), [k][1] = (acc[2], acc[3])
#pragma unroll
    for (int k = 0; k < EPT2; ++k) acc[k][0] = acc[k][1] = d2{0.0, 0.0};
    double pp = 0.0;

    // (as in sweep_kernel: unconditional loads at 32-bit offsets from a uniform base, threads past the end
    // re-read the last double2.  Only the last of a thread's double2 can lie past the end, (EPT2 - 1) 1024 < 2 ldF:
    // the others share one offset from bases k 1024 double2 apart, and one LDS address serves all of them --
    // registers kept out of the loop, which has none to spare)
    unsigned voff = (unsigned)tid * (unsigned)sizeof(d2);
    unsigned coff_last;
    {
        const int e = (EPT2 - 1) * TT + tid;
        coff_last = (unsigned)(e < n2 ? e : n2 - 1) * (unsigned)sizeof(d2);
    }
    const bool last_in = (EPT2 - 1) * TT + tid < n2;
    // (no null pointers here: launch_fold points the inputs a mode does not read at zeros, so every per-cell
    // load is unconditional; lanes 32..63 repeat lanes 0..31)
    const int hl = (lane >> 3) & 3, ql = lane & 7;
    const double *in_base = ql == FOLD_IN_P      ? a.p_in
                            : ql == FOLD_IN_GREG ? a.greg
                            : ql == FOLD_IN_HI   ? a.high
                            : ql == FOLD_IN_LO   ? a.low
                            : ql == FOLD_IN_PN   ? a.pn_in
                            : (ql == FOLD_IN_GACC && (mode & SW_GACC)) ? a.g_out
                                                                       : a.x_in;
    const int lastc = cnt - 1;
    auto orb = [&](int i) -> int64_t { return ob + (i < lastc ? i : lastc); };
    // (a buffer requests the cell indices of its own next orbit, two blocks ahead: handing an index from one
    // buffer to the other made the compiler copy it at the loop's back edge, behind a wait for every request
    // in flight)
    auto load_col = [&](FoldCol<EPT2> &c, int64_t o, int64_t o_after) {
        // (the index first: a wait for it then never waits for this block)
        const int jn = f.cell_orbit[4 * o_after + hl];
        const unsigned long long col = (unsigned long long)(f.S + o * (int64_t)(4 * f.ldF));
#pragma unroll
        for (int k = 0; k < EPT2 - 1; ++k) {
            unsigned long long colk = col + (unsigned long long)k * TT * sizeof(d2);
            asm volatile("" : "+s"(colk));
            asm volatile("" : "+v"(voff));
            c.v[k] = __builtin_nontemporal_load(reinterpret_cast<gconst_d2ptr>(colk + voff));
        }
        asm volatile("" : "+v"(coff_last));
        c.v[EPT2 - 1] = __builtin_nontemporal_load(reinterpret_cast<gconst_d2ptr>(col + coff_last));
        // (the inputs' addresses wait for this orbit's indices, requested two blocks earlier: after this block's
        // requests, not before them)
        asm volatile("" : "+v"(c.jn)::"memory");
        c.j = c.jn;
        c.cv = in_base[c.j];
        c.jn = jn;
    };

    auto process = [&](const FoldCol<EPT2> &cur, int it) {
        // lane 8h: the inputs of cell h
        double xl = cur.cv;
        const double pl = dpp_from_up<FOLD_IN_P>(cur.cv);
        double xh[4];
        if (mode & SW_ADJ) {
            // (row i = (k 1024 + t) / 2 of r at rF + 32 i = rF + 32 (t / 2) + 16384 k)
            const d2 *rF2 = reinterpret_cast<const d2 *>(rF) + 2 * (tid >> 1);
            double u0 = 0.0, u1 = 0.0, u2 = 0.0, u3 = 0.0;
#pragma unroll
            for (int k = 0; k < EPT2; ++k) {
                if (k < EPT2 - 1 || last_in) {
                    const d2 ra = rF2[k * TT], rb = rF2[k * TT + 1];
                    const d2 v = cur.v[k];
                    u0 += v.x * ra.x;
                    u0 += v.y * ra.y;
                    u1 += v.x * ra.y;
                    u1 += v.y * ra.x;
                    u2 += v.x * rb.x;
                    u2 += v.y * rb.y;
                    u3 += v.x * rb.y;
                    u3 += v.y * rb.x;
                }
            }
            // odd threads: u[q] is a term of dot[q ^ 2].  The four dots reduced together: lane pairs (quad_perm
            // [1,0,3,2]) leave dots 0, 1 in even lanes and 2, 3 in odd ones, pairs of pairs ([2,3,0,1]) one dot per
            // lane, dot 2 (l & 1) + ((l >> 1) & 1) of its quad; row_shr 4, 8 sum the quads of a row of 16 into
            // lanes 16 r + 12 .. 15.  Every sum even lane / lower half first.
            const bool odd = (tid & 1) != 0, hi2 = (tid & 2) != 0;
            const double w0 = odd ? u2 : u0, w1 = odd ? u3 : u1, w2 = odd ? u0 : u2, w3 = odd ? u1 : u3;
            const double a0 = (odd ? w2 : w0) + dpp_mov<0xb1>(odd ? w0 : w2);
            const double a1 = (odd ? w3 : w1) + dpp_mov<0xb1>(odd ? w1 : w3);
            double sq = (hi2 ? a1 : a0) + dpp_mov<0x4e>(hi2 ? a0 : a1);
            sq = dpp_add<0x114, 0xf>(sq);
            sq = dpp_add<0x118, 0xf>(sq);
            // slot[w 16 + q 4 + r]: dot q of row r of wave w
            double *slot = scratch + (it & 1) * FOLD_SLOT;
            if ((lane & 15) >= 12) slot[wave * 16 + (((lane & 1) << 1) | ((lane >> 1) & 1)) * 4 + (lane >> 4)] = sq;
            __syncthreads();
            // lane l of every wave takes the dot l & 3 of wave l >> 2 (its four rows, one 32-byte read); sums over
            // the waves in fixed order: the four of a row of 16 lanes (row_shr 4, 8: lane 16 r + 12 + h), then the
            // four rows
            const d2 *sl = reinterpret_cast<const d2 *>(slot + (lane >> 2) * 16 + (lane & 3) * 4);
            const d2 ra = sl[0], rb = sl[1];
            double sv = (ra.x + ra.y) + (rb.x + rb.y);
            sv = dpp_add<0x114, 0xf>(sv);
            sv = dpp_add<0x118, 0xf>(sv);
            double t[4];
#pragma unroll
            for (int h = 0; h < 4; ++h)
                t[h] = ((readlane_d(sv, 12 + h) + readlane_d(sv, 28 + h)) + readlane_d(sv, 44 + h)) + readlane_d(sv, 60 + h);
            // cell h in lane 8h (same arithmetic per cell as sweep_kernel); wave 0 stores
            const double th = hl == 0 ? t[0] : hl == 1 ? t[1] : hl == 2 ? t[2] : t[3];
            const double g = 2.0 * th + dpp_from_up<FOLD_IN_GREG>(cur.cv);
            double pv = 0.0, pf = 0.0;
            if (mode & SW_PFIN) {
                pf = pl - a.c_p * g;
                pv = pf;
            }
            if (mode & SW_UPD) {
                const double chi = dpp_from_up<FOLD_IN_HI>(cur.cv), clo = dpp_from_up<FOLD_IN_LO>(cur.cv);
                const double psrc = (mode & SW_SPEC) ? dpp_from_up<FOLD_IN_PN>(cur.cv) : pl;
                double pj = psrc - a.c_u * g;
                double xj = xl + a.dt * pj;
                if (xj > chi) {
                    xj = chi;
                    pj = -pj;
                } else if (xj < clo) {
                    xj = clo;
                    pj = -pj;
                }
                pv = pj;
                xl = xj;
            }
            if (mode & SW_PFIN) {
                // (in the cells' order, as the dense sweep adds them)
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    const double q = readlane_d(pf, 8 * h);
                    pp += q * q;
                }
            }
            if (tid < 32 && ql == 0) {
                const int j = cur.j;
                if (mode & SW_GOUT) a.g_out[j] = (mode & SW_GACC) ? dpp_from_up<FOLD_IN_GACC>(cur.cv) + g : g;
                if (mode & SW_UPD) {
                    a.p_out[j] = pv;
                    a.x_out[j] = xl;
                } else if ((mode & SW_PFIN) && !(mode & SW_SPEC)) {
                    a.p_out[j] = pv;
                }
            }
        }
        if (mode & SW_FWD) {
#pragma unroll
            for (int h = 0; h < 4; ++h) xh[h] = readlane_d(xl, 8 * h);
#pragma unroll
            for (int k = 0; k < EPT2; ++k) {
                const d2 v = cur.v[k];
                acc[k][0].x += v.x * xh[0];
                acc[k][0].x += v.y * xh[1];
                acc[k][0].y += v.x * xh[1];
                acc[k][0].y += v.y * xh[0];
                acc[k][1].x += v.x * xh[2];
                acc[k][1].x += v.y * xh[3];
                acc[k][1].y += v.x * xh[3];
                acc[k][1].y += v.y * xh[2];
            }
        }
        // (the block is consumed on every path the compiler sees: otherwise it waits for the block's requests
        // before it reuses their registers at the top of the loop, i.e. before the next block is requested)
#pragma unroll
        for (int k = 0; k < EPT2; ++k) asm volatile("" ::"v"(cur.v[k]));
    };

    if (cnt > 0) {
        FoldCol<EPT2> b0, b1;
        b0.jn = f.cell_orbit[4 * orb(0) + hl];
        b1.jn = f.cell_orbit[4 * orb(1) + hl];
        load_col(b0, orb(0), orb(2));
        int i = 0;
        for (;;) {
            load_col(b1, orb(i + 1), orb(i + 3));
            process(b0, i);
            if (++i >= cnt) break;
            load_col(b0, orb(i + 1), orb(i + 3));
            process(b1, i);
            if (++i >= cnt) break;
        }
    }

    if ((mode & SW_PFIN) && tid == 0) {
        a.pp_part[blockIdx.x] = pp;
        for (int t = (int)(blockIdx.x + gridDim.x); t < f.n_pp; t += (int)gridDim.x) a.pp_part[t] = 0.0;
    }

    if (mode & SW_FWD) {
        // the observation s_(2m) f gets acc[0] of thread m = 0 plus acc[2] of m = 1 (and the reverse for m = 1:
        // the same sum, in the other order -- one expression serves both), s_(2m+1) f acc[1] plus acc[3]
        double *out = a.slab + (int64_t)blockIdx.x * a.ld;
        double ds = 0.0;
#pragma unroll
        for (int k = 0; k < EPT2; ++k) {
            const int e = k * TT + tid;
            const double p2 = __shfl_xor(acc[k][1].x, 1, WAVE), p3 = __shfl_xor(acc[k][1].y, 1, WAVE);
            const double tA = acc[k][0].x + p2, tB = acc[k][0].y + p3;
            const int i = e >> 1;
            if (e < n2 && i < f.nF) {
                const int m2 = 2 * (tid & 1);
                out[f.obs_img[4 * i + m2]] = tA;
                out[f.obs_img[4 * i + m2 + 1]] = tB;
                ds += tA;
                ds += tB;
            }
        }
        for (int64_t e = f.N + tid; e < a.ld; e += TT) out[e] = 0.0;
        if (a.dsum) {
            const double t = block_allreduce_sum(ds, scratch, NW);
            if (tid == 0) a.dsum[blockIdx.x] = t;
        }
    }
}

// ------------------------------------------------------------------ the diagonal reflection on top of the mirrors
//
// Where cells and observations are also symmetric under tau: (x, y) -> (cx + (y - cy), cy + (x - cx)) (square
// columns, the same grid of observations along x and y; host_fold.h finds it), Aw(tau i, tau j) = Aw(i, j), so the
// block of a cell orbit o holds the entries of its partner orbit tau o as well, row for row:
//
//     dotT[h]        = sum_f sum_k S[o][f][k] r[tau s_(k^h) f]        the cell tau s_h j_o
//     dpartT[s_g f] += sum_h S[o][f][g^h] x[tau s_h j_o]              lands in slab[tau s_g f]
//
// i.e. the sums above with r o tau and x o tau.  One read of S[o] then serves eight cells, the store is what it
// was (for a pair both blocks hold the mean over all eight images, fold_pair_mean_kernel), and a sweep reads the
// leaders' blocks and those of the orbits that are their own partners (the cell columns on a diagonal) only:
// 16 FMA per double read.

struct FoldPairArgs {
    const int *wtab;         // n_work x 16: [0, 4) cells s_h j_o of the leading orbit, [4, 8) tau s_h j_o (~ of the
                             // entry four to the left where the orbit has no partner), [8] the orbit, then padding
    const int *ptab;         // fold_pair_cols(ROWS) x 512 x 4: the observation behind every value of r in LDS and behind
                             // every forward sum of thread t (-1: none), in the row order of fold_pair_rows_kernel
    int64_t n_work, work_per_team;
};
constexpr int FOLD_PAIR_W = 16;
constexpr int FOLD_PSLOT = 64;  // doubles: 8 waves x 8 dots

// The rows of a block folded over tau as well.  With tau f = s_(c_f) f' (row_tau[f] = 4 f' + c_f) and
// tau s_g = s_swap(g) tau, the partner terms of row f read r at, and add into d at, the four observations of row f'
// (and those of f' the four of f): a thread that holds both rows needs r at eight observations and eight forward
// sums for the two.  Thread t of 512 owns the rows k 512 + t of a block, k < ROWS, in slots:
//     pair slot s < NP = (ROWS - 1) / 2     rows 2 s (row f as stored) and 2 s + 1 (row f' as the representative
//                                           tau f of its orbit: its sub-columns k ^ c_f)
//     lone slot NP <= s < NS = ROWS - NP    row NP + s alone: r at s_g tau f from LDS and its own four tau sums
// Column 2 s of ptab holds the observations s_g f of the slot's first row, column 2 s + 1 the observations s_g tau f
// (those of the second row where there is one).  With A the first row, B the second, As = (A0, A2, A1, A3), ra / rb
// the two columns of r, x the orbit's cells, y = x o tau, ys = (y0, y2, y1, y3) and t(S, w)[q] = sum_k S[k] w[k ^ q]:
//     dot[h]     += t(A, ra)[h] + t(B, rb)[h]            dotT[swap h] += t(As, rb)[h] + t(Bs, ra)[h]
//     d[s_g f]   += t(A, x)[g] + t(Bs, ys)[g]            d[s_g tau f] += t(B, x)[g] + t(As, ys)[g]
// 16 FMA per double read as before; a lone slot is a pair slot without B.
constexpr int fold_pair_slots(int rows) { return (rows - 1) / 2; }
constexpr int fold_pair_cols(int rows) { return 2 * (rows - fold_pair_slots(rows)); }

// The store in the paired sweep's row order, block by block in place (one workgroup per block, the block in LDS):
// row n becomes row code[n] >> 2 of fold_build_kernel's order with its sub-columns k ^ (code[n] & 3), or zeros
// (code[n] < 0).  Within a group of w = min(512, ldF - 512 k) rows k 512 + t the first halves (sub-columns 0, 1) of all
// rows come first, then the second halves: the 64 lanes of a wave read 1 KiB in one piece with either of a row's two
// 16-byte loads (a row's 32 bytes side by side made every load touch twice the lines it used).
__global__ void __launch_bounds__(512) fold_pair_rows_kernel(FoldArgs f, const int *code, double *S)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int n = 4 * f.ldF;
    double *blk = S + (int64_t)blockIdx.x * n;
    for (int e = threadIdx.x; e < n; e += blockDim.x) smem[e] = blk[e];
    __syncthreads();
    for (int e = threadIdx.x; e < n; e += blockDim.x) {
        const int cd = code[e >> 2];
        const int k = e >> 11, t = (e >> 2) & 511, w = min(512, f.ldF - 512 * k);
        blk[2048 * k + 2 * (((e >> 1) & 1) * w + t) + (e & 1)] = cd >= 0 ? smem[(cd & ~3) | ((e ^ cd) & 3)] : 0.0;
    }
}

// Both blocks of a pair (or the two halves of a block that is its own partner) become the mean of what
// fold_build_kernel left in them: S[o][f][k] and S[o'][f'][swap(k) ^ c_o ^ c_f] (row_tau[f] = 4 f' + c_f with
// tau f = s_(c_f) f', orb_tau[o] = 4 o' + c_o alike, swap: bits 0 and 1 exchanged) are the same entry of Aw.
// a + b = b + a: the bits do not depend on which orbit leads.  dev_bits: max |entry - mean| / (largest |mean| of the
// block), as in fold_build_kernel.
__global__ void __launch_bounds__(256) fold_pair_mean_kernel(FoldArgs f, const int *row_tau, const int *orb_tau, double *S,
                                                             unsigned long long *dev_bits)
{
    __shared__ double red[2][4];
    const int64_t o = blockIdx.x;
    const int ot = orb_tau[o];
    const int64_t o2 = ot >> 2;
    const int co = ot & 3;
    const int n = 4 * f.nF;
    const int64_t ldb = 4 * (int64_t)f.ldF;
    double dev = 0.0, amax = 0.0;
    if (o <= o2) {
        for (int e = threadIdx.x; e < n; e += blockDim.x) {
            const int k = e & 3, rt = row_tau[e >> 2];
            const int ks = ((k & 1) << 1) | (k >> 1);
            const int e2 = (rt & ~3) | (ks ^ co ^ (rt & 3));
            if (o < o2 || e < e2) {
                const double u = S[o * ldb + e], v = S[o2 * ldb + e2];
                const double m = (u + v) * 0.5;
                S[o * ldb + e] = m;
                S[o2 * ldb + e2] = m;
                dev = fmax(dev, fabs(u - m));
                amax = fmax(amax, fabs(m));
            } else if (e == e2) {
                amax = fmax(amax, fabs(S[o * ldb + e]));
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        dev = fmax(dev, __shfl_xor(dev, off, WAVE));
        amax = fmax(amax, __shfl_xor(amax, off, WAVE));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red[0][wave] = dev;
        red[1][wave] = amax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) {
            dev = fmax(dev, red[0][w]);
            amax = fmax(amax, red[1][w]);
        }
        const double rel = amax > 0.0 ? dev / amax : 0.0;
        atomicMax(dev_bits, (unsigned long long)__double_as_longlong(rel));
    }
}

template <int ROWS>
struct FoldPairCol {
    d2 v[ROWS][2];  // sub-columns 0..1 and 2..3 of the thread's rows k 512 + t (the order of fold_pair_rows_kernel)
    int j;          // lane 32 s + 8 h + q: cell h of the orbit (s = 0) or of its partner (s = 1)
    int jn, on;     // the same of the work item this buffer takes next, and that item's orbit
    bool live;      // the cell exists (partner lanes of an orbit without a partner: false)
    double cv;      // per-cell inputs as in FoldCol
};

// The paired form of fold_sweep_kernel: 8 waves per workgroup, a whole folded row (4 k) of ROWS rows per thread in
// the slots above, two blocks in flight ahead with their cells' inputs, no scalar load in the loop (the work item's
// orbit comes with the cell indices, three blocks ahead, through a vector load).  LDS: r behind every entry of ptab
// (fold_pair_cols(ROWS) x 512 x 4 doubles: 96 KiB at five rows), 2 x FOLD_PSLOT ping-pong slots of the eight dots.
// The eight cells' updates run side by side in lanes 8 h (the orbit) and 32 + 8 h (its partner) with the arithmetic
// of fold_sweep_kernel per cell.
template <int ROWS>
__global__ void __launch_bounds__(512) fold_pair_sweep_kernel(SweepArgs a, FoldArgs f, FoldPairArgs p)
{
    constexpr int TT = 512, NW = 8;
    constexpr int NP = fold_pair_slots(ROWS), NS = ROWS - NP, NC = fold_pair_cols(ROWS);
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double *rL = smem;
    double *scratch = smem + NC * TT * 4;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int mode = a.mode;

    if (mode & SW_ADJ) {
        for (int e = tid; e < NC * TT * 4; e += TT) {
            const int i = p.ptab[e];
            rL[e] = i >= 0 ? a.r[i] : 0.0;
        }
    }
    __syncthreads();

    const int64_t wb = (int64_t)blockIdx.x * p.work_per_team;
    int64_t wend = wb + p.work_per_team;
    if (wend > p.n_work) wend = p.n_work;
    const int cnt = wb < wend ? (int)(wend - wb) : 0;

    // [s][c][0] = the forward sums at the observations s_0, s_1 of column 2 s + c of ptab, [s][c][1] = at s_2, s_3
    d2 acc[NS][2][2];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s][0][0] = acc[s][0][1] = acc[s][1][0] = acc[s][1][1] = d2{0.0, 0.0};
    double pp = 0.0;

    // (only the last of a thread's rows, the first row of the last slot, can lie past the block: (ROWS - 1) 512 < ldF.
    // It re-reads the block's last row and takes no part in the adjoint's sums; its forward sums have no observation
    // in ptab)
    const int row_last = (ROWS - 1) * TT + tid;
    const bool last_in = row_last < f.ldF;
    // (a group of rows holds the first halves of its rows, then the second halves: fold_pair_rows_kernel)
    const int w_last = f.ldF - (ROWS - 1) * TT;
    unsigned voff = (unsigned)tid * 16u;
    unsigned coff_last = (unsigned)(last_in ? tid : w_last - 1) * 16u;

    const int hl = (lane >> 3) & 3, ql = lane & 7, sl = lane >> 5;
    const double *in_base = ql == FOLD_IN_P      ? a.p_in
                            : ql == FOLD_IN_GREG ? a.greg
                            : ql == FOLD_IN_HI   ? a.high
                            : ql == FOLD_IN_LO   ? a.low
                            : ql == FOLD_IN_PN   ? a.pn_in
                            : (ql == FOLD_IN_GACC && (mode & SW_GACC)) ? a.g_out
                                                                       : a.x_in;
    const int lastc = cnt - 1;
    auto item = [&](int i) -> int64_t { return wb + (i < lastc ? i : lastc); };
    auto load_col = [&](FoldPairCol<ROWS> &c, int64_t w_after) {
        // (this item's cell and orbit, requested three blocks ago, leave their registers before the next item's are
        // requested into them: otherwise the compiler keeps two sets and copies one to the other at the loop's back
        // edge, behind a wait for the requests just made)
        asm volatile("" : "+v"(c.jn), "+v"(c.on)::"memory");
        const int64_t o = __builtin_amdgcn_readfirstlane(c.on);
        c.live = c.jn >= 0;
        c.j = c.live ? c.jn : ~c.jn;
        asm volatile("" : "+v"(c.j));
        c.jn = p.wtab[FOLD_PAIR_W * w_after + (lane >> 3)];
        c.on = p.wtab[FOLD_PAIR_W * w_after + 8];
        const unsigned long long col = (unsigned long long)(f.S + o * (int64_t)(4 * f.ldF));
#pragma unroll
        for (int k = 0; k < ROWS - 1; ++k) {
            unsigned long long colk = col + (unsigned long long)k * TT * 32u, colh = colk + TT * 16u;
            asm volatile("" : "+s"(colk));
            asm volatile("" : "+s"(colh));
            asm volatile("" : "+v"(voff));
            c.v[k][0] = __builtin_nontemporal_load(reinterpret_cast<gconst_d2ptr>(colk + voff));
            c.v[k][1] = __builtin_nontemporal_load(reinterpret_cast<gconst_d2ptr>(colh + voff));
        }
        unsigned long long coll = col + (unsigned long long)(ROWS - 1) * TT * 32u, collh = coll + (unsigned)w_last * 16u;
        asm volatile("" : "+s"(coll));
        asm volatile("" : "+s"(collh));
        asm volatile("" : "+v"(coff_last));
        c.v[ROWS - 1][0] = __builtin_nontemporal_load(reinterpret_cast<gconst_d2ptr>(coll + coff_last));
        c.v[ROWS - 1][1] = __builtin_nontemporal_load(reinterpret_cast<gconst_d2ptr>(collh + coff_last));
        c.cv = in_base[c.j];
    };

    // t[q] += sum_k S[f][k] w[k ^ q] of one row: (wa, wb) = w[0..1], w[2..3]
    auto row_fma = [](const d2 v0, const d2 v1, const d2 wa, const d2 wb2, d2 &t01, d2 &t23) {
        t01.x += v0.x * wa.x;
        t01.x += v0.y * wa.y;
        t01.x += v1.x * wb2.x;
        t01.x += v1.y * wb2.y;
        t01.y += v0.x * wa.y;
        t01.y += v0.y * wa.x;
        t01.y += v1.x * wb2.y;
        t01.y += v1.y * wb2.x;
        t23.x += v0.x * wb2.x;
        t23.x += v0.y * wb2.y;
        t23.x += v1.x * wa.x;
        t23.x += v1.y * wa.y;
        t23.y += v0.x * wb2.y;
        t23.y += v0.y * wb2.x;
        t23.y += v1.x * wa.y;
        t23.y += v1.y * wa.x;
    };

    auto process = [&](const FoldPairCol<ROWS> &cur, int it) {
        double xl = cur.cv;
        const double pl = dpp_from_up<FOLD_IN_P>(cur.cv);
        if (mode & SW_ADJ) {
            const d2 *r2 = reinterpret_cast<const d2 *>(rL) + 2 * tid;
            d2 ua = d2{0.0, 0.0}, ub = ua, wa = ua, wb = ua;  // (ua, ub): dot[0..3], (wa, wb): dotT[swap 0..3]
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int k = s < NP ? 2 * s : NP + s;
                if (k < ROWS - 1 || last_in) {
                    const d2 ra0 = r2[4 * s * TT], ra1 = r2[4 * s * TT + 1];
                    const d2 rb0 = r2[(4 * s + 2) * TT], rb1 = r2[(4 * s + 2) * TT + 1];
                    const d2 a0 = cur.v[k][0], a1 = cur.v[k][1];
                    row_fma(a0, a1, ra0, ra1, ua, ub);
                    row_fma(d2{a0.x, a1.x}, d2{a0.y, a1.y}, rb0, rb1, wa, wb);
                    if (s < NP) {
                        const d2 b0 = cur.v[k + 1][0], b1 = cur.v[k + 1][1];
                        row_fma(b0, b1, rb0, rb1, ua, ub);
                        row_fma(d2{b0.x, b1.x}, d2{b0.y, b1.y}, ra0, ra1, wa, wb);
                    }
                }
            }
            // the eight dots reduced together: lane pairs leave the orbit's four in even lanes and the partner's in odd
            // ones, pairs of pairs dots 2 b, 2 b + 1 of them in the lanes with (l >> 1) & 1 = b, row_shr 4, 8 sum the
            // quads of a row of 16 into its lanes 12 .. 15, two exchanges the four rows.  Fixed order throughout.
            const bool odd = (lane & 1) != 0, hi2 = (lane & 2) != 0;
            const double u[4] = {ua.x, ua.y, ub.x, ub.y}, ut[4] = {wa.x, wb.x, wa.y, wb.y};
            double b[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) b[q] = (odd ? ut[q] : u[q]) + dpp_mov<0xb1>(odd ? u[q] : ut[q]);
            double s0 = (hi2 ? b[2] : b[0]) + dpp_mov<0x4e>(hi2 ? b[0] : b[2]);
            double s1 = (hi2 ? b[3] : b[1]) + dpp_mov<0x4e>(hi2 ? b[1] : b[3]);
            s0 = dpp_add<0x114, 0xf>(s0);
            s0 = dpp_add<0x118, 0xf>(s0);
            s1 = dpp_add<0x114, 0xf>(s1);
            s1 = dpp_add<0x118, 0xf>(s1);
            s0 += __shfl_xor(s0, 16, WAVE);
            s1 += __shfl_xor(s1, 16, WAVE);
            s0 += __shfl_xor(s0, 32, WAVE);
            s1 += __shfl_xor(s1, 32, WAVE);
            // slot[8 w + 4 s + h]: dot h of the orbit (s = 0) / its partner (s = 1), wave w
            double *slot = scratch + (it & 1) * FOLD_PSLOT;
            if (lane >= 12 && lane < 16) {
                const int c = lane - 12;
                *reinterpret_cast<d2 *>(slot + wave * 8 + 4 * (c & 1) + 2 * (c >> 1)) = d2{s0, s1};
            }
            __syncthreads();
            // lane l: wave l >> 3, dot l & 7; the eight waves in fixed order
            double sv = slot[lane];
            sv = dpp_add<0x118, 0xf>(sv);
            sv += __shfl_xor(sv, 16, WAVE);
            sv += __shfl_xor(sv, 32, WAVE);
            const double th = __shfl(sv, 8 + 4 * sl + hl, WAVE);
            const double g = 2.0 * th + dpp_from_up<FOLD_IN_GREG>(cur.cv);
            double pv = 0.0, pf = 0.0;
            if (mode & SW_PFIN) {
                pf = pl - a.c_p * g;
                pv = pf;
            }
            if (mode & SW_UPD) {
                const double chi = dpp_from_up<FOLD_IN_HI>(cur.cv), clo = dpp_from_up<FOLD_IN_LO>(cur.cv);
                const double psrc = (mode & SW_SPEC) ? dpp_from_up<FOLD_IN_PN>(cur.cv) : pl;
                double pj = psrc - a.c_u * g;
                double xj = xl + a.dt * pj;
                if (xj > chi) {
                    xj = chi;
                    pj = -pj;
                } else if (xj < clo) {
                    xj = clo;
                    pj = -pj;
                }
                pv = pj;
                xl = xj;
            }
            if (mode & SW_PFIN) {
                // (the orbit's cells, then its partner's: a cell that is not there adds +0)
                const double pz = cur.live ? pf : 0.0;
#pragma unroll
                for (int h = 0; h < 8; ++h) {
                    const double q = readlane_d(pz, 8 * h);
                    pp += q * q;
                }
            }
            if (tid < 64 && ql == 0 && cur.live) {
                const int j = cur.j;
                if (mode & SW_GOUT) a.g_out[j] = (mode & SW_GACC) ? dpp_from_up<FOLD_IN_GACC>(cur.cv) + g : g;
                if (mode & SW_UPD) {
                    a.p_out[j] = pv;
                    a.x_out[j] = xl;
                } else if ((mode & SW_PFIN) && !(mode & SW_SPEC)) {
                    a.p_out[j] = pv;
                }
            }
        }
        if (mode & SW_FWD) {
            const double xz = cur.live ? xl : 0.0;
            const d2 xa = d2{readlane_d(xz, 0), readlane_d(xz, 8)}, xb = d2{readlane_d(xz, 16), readlane_d(xz, 24)};
            const d2 ya = d2{readlane_d(xz, 32), readlane_d(xz, 40)}, yb = d2{readlane_d(xz, 48), readlane_d(xz, 56)};
            const d2 ysa = d2{ya.x, yb.x}, ysb = d2{ya.y, yb.y};
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int k = s < NP ? 2 * s : NP + s;
                const d2 a0 = cur.v[k][0], a1 = cur.v[k][1];
                row_fma(a0, a1, xa, xb, acc[s][0][0], acc[s][0][1]);
                row_fma(d2{a0.x, a1.x}, d2{a0.y, a1.y}, ysa, ysb, acc[s][1][0], acc[s][1][1]);
                if (s < NP) {
                    const d2 b0 = cur.v[k + 1][0], b1 = cur.v[k + 1][1];
                    row_fma(b0, b1, xa, xb, acc[s][1][0], acc[s][1][1]);
                    row_fma(d2{b0.x, b1.x}, d2{b0.y, b1.y}, ysa, ysb, acc[s][0][0], acc[s][0][1]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < ROWS; ++k) {
            asm volatile("" ::"v"(cur.v[k][0]));
            asm volatile("" ::"v"(cur.v[k][1]));
        }
    };

    if (cnt > 0) {
        // (a buffer takes every third item and requests the cells and the orbit of its own next one: past the end
        // the requests repeat the last item and nothing uses them)
        FoldPairCol<ROWS> b0, b1, b2;
        b0.jn = p.wtab[FOLD_PAIR_W * item(0) + (lane >> 3)];
        b0.on = p.wtab[FOLD_PAIR_W * item(0) + 8];
        b1.jn = p.wtab[FOLD_PAIR_W * item(1) + (lane >> 3)];
        b1.on = p.wtab[FOLD_PAIR_W * item(1) + 8];
        b2.jn = p.wtab[FOLD_PAIR_W * item(2) + (lane >> 3)];
        b2.on = p.wtab[FOLD_PAIR_W * item(2) + 8];
        load_col(b0, item(3));
        load_col(b1, item(4));
        // (no way out of the loop between its three blocks: the compiler routes such an exit through a block with an
        // edge back to the loop's head, and then waits there as if a request made one block ago had been made three ago)
        int i = 0;
        for (; i + 2 < cnt; i += 3) {
            load_col(b2, item(i + 5));
            process(b0, i);
            load_col(b0, item(i + 6));
            process(b1, i + 1);
            load_col(b1, item(i + 7));
            process(b2, i + 2);
        }
        if (i < cnt) process(b0, i);
        if (i + 1 < cnt) process(b1, i + 1);
    }

    if ((mode & SW_PFIN) && tid == 0) {
        a.pp_part[blockIdx.x] = pp;
        for (int t = (int)(blockIdx.x + gridDim.x); t < f.n_pp; t += (int)gridDim.x) a.pp_part[t] = 0.0;
    }

    if (mode & SW_FWD) {
        // every stored row is the first row of a slot or the second of a pair slot: their sums go to their observations
        // (each observation once), then, behind a barrier, the tau sums of the lone slots are added at theirs (another
        // thread's observations of the same slab row); the row's sum in the same order
        double *out = a.slab + (int64_t)blockIdx.x * a.ld;
        const int4 *pt = reinterpret_cast<const int4 *>(p.ptab) + tid;
        double ds = 0.0;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if ((c & 1) && (c >> 1) >= NP) continue;
            const int4 oi = pt[c * TT];
            if (oi.x >= 0) {
                const d2 s01 = acc[c >> 1][c & 1][0], s23 = acc[c >> 1][c & 1][1];
                out[oi.x] = s01.x;
                out[oi.y] = s01.y;
                out[oi.z] = s23.x;
                out[oi.w] = s23.y;
                ds += s01.x;
                ds += s01.y;
                ds += s23.x;
                ds += s23.y;
            }
        }
        for (int64_t e = f.N + tid; e < a.ld; e += TT) out[e] = 0.0;
        __syncthreads();
#pragma unroll
        for (int s = NP; s < NS; ++s) {
            const int4 oi = pt[(2 * s + 1) * TT];
            if (oi.x >= 0) {
                const d2 s01 = acc[s][1][0], s23 = acc[s][1][1];
                out[oi.x] += s01.x;
                out[oi.y] += s01.y;
                out[oi.z] += s23.x;
                out[oi.w] += s23.y;
                ds += s01.x;
                ds += s01.y;
                ds += s23.x;
                ds += s23.y;
            }
        }
        if (a.dsum) {
            const double t = block_allreduce_sum(ds, scratch, NW);
            if (tid == 0) a.dsum[blockIdx.x] = t;
        }
    }
}

}  // namespace ghk
