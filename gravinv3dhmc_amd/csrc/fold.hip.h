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

typedef const int __attribute__((address_space(4))) *kconst_iptr;
__device__ __forceinline__ kconst_iptr as_kconst_i(const int *p)
{
    return (kconst_iptr)(unsigned long long)p;
}

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
    int j[4];  // the orbit's cells (uniform)
};

// One team of 16 waves per workgroup, one orbit block at a time (EPT2 double2 per thread: 2048 EPT2 rows
// of S), one block in flight ahead (at C2: EPT2 = 5, 128 VGPRs, no scratch).  Every mode of sweep_kernel (SW_ADJ / UPD / FWD / PFIN / GOUT / GACC /
// SPEC, dsum) over a whole panel; M-vectors in the caller's cell order, the slab row in the caller's
// observation order.  Thread t holds double2 e = k 1024 + t of a block, i.e. S[o][e >> 1][2m], S[o][e >> 1][2m + 1]
// with m = t & 1: its adjoint terms u[q] = S[2m] r[s_q f] + S[2m+1] r[s_(q^1) f] belong to dot[q ^ 2m], its
// forward terms acc[q] = S[2m] x[q] + S[2m+1] x[q^1] to the observation s_(q^2m) f.
template <int EPT2>
__global__ void __launch_bounds__(1024) fold_sweep_kernel(SweepArgs a, FoldArgs f)
{
    constexpr int TT = 1024, NW = 16, SLOT = 4 * NW + 8;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    // LDS: [0, 4 ldF) r at the four images of each fundamental observation; 2 x SLOT ping-pong slots of the
    // four dots of an orbit
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
    // re-read the last double2; per-cell scalars through the scalar cache, the orbit's cell indices requested
    // one block ahead of the scalars they address)
    unsigned coff[EPT2];
#pragma unroll
    for (int k = 0; k < EPT2; ++k) {
        const int e = k * TT + tid;
        coff[k] = (unsigned)(e < n2 ? e : n2 - 1) * (unsigned)sizeof(d2);
    }
    // (no null pointers here: launch_fold points the inputs a mode does not read at zeros, so every per-cell
    // scalar load is unconditional)
    const kconst_ptr kx = as_kconst(a.x_in), kp = as_kconst(a.p_in), klo = as_kconst(a.low), khi = as_kconst(a.high),
                     kgr = as_kconst(a.greg), kpn = as_kconst(a.pn_in);
    const kconst_iptr kco = as_kconst_i(f.cell_orbit);
    const int lastc = cnt - 1;
    auto orb = [&](int i) -> int64_t { return ob + (i < lastc ? i : lastc); };
    int jn[4];
    auto load_idx = [&](int64_t o) {
#pragma unroll
        for (int h = 0; h < 4; ++h) jn[h] = kco[4 * o + h];
    };
    auto load_col = [&](FoldCol<EPT2> &c, int64_t o, int64_t o_next) {
#pragma unroll
        for (int h = 0; h < 4; ++h) c.j[h] = jn[h];
        const char *col = reinterpret_cast<const char *>(f.S + o * (int64_t)(4 * f.ldF));
#pragma unroll
        for (int k = 0; k < EPT2; ++k) {
            asm volatile("" : "+v"(coff[k]));
            const d2 *src = reinterpret_cast<const d2 *>(col + coff[k]);
            c.v[k] = __builtin_nontemporal_load(src);
        }
        load_idx(o_next);
    };

    auto process = [&](const FoldCol<EPT2> &cur, int it) {
        double xh[4];
#pragma unroll
        for (int h = 0; h < 4; ++h) xh[h] = kx[cur.j[h]];
        if (mode & SW_ADJ) {
            const d2 *rF2 = reinterpret_cast<const d2 *>(rF);
            double u0 = 0.0, u1 = 0.0, u2 = 0.0, u3 = 0.0;
#pragma unroll
            for (int k = 0; k < EPT2; ++k) {
                const int e = k * TT + tid;
                if (e < n2) {
                    const int i = e >> 1;
                    const d2 ra = rF2[2 * i], rb = rF2[2 * i + 1];
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
            // odd threads: u[q] is a term of dot[q ^ 2]
            const bool odd = (tid & 1) != 0;
            const double s0 = wave_sum_dpp(odd ? u2 : u0), s1 = wave_sum_dpp(odd ? u3 : u1),
                         s2 = wave_sum_dpp(odd ? u0 : u2), s3 = wave_sum_dpp(odd ? u1 : u3);
            d2 *slot = reinterpret_cast<d2 *>(scratch + (it & 1) * SLOT);
            if (lane == 0) {
                slot[2 * wave] = d2{s0, s1};
                slot[2 * wave + 1] = d2{s2, s3};
            }
            __syncthreads();
            // lane l of every wave takes the dot l & 3 of wave l >> 2; sums over the waves in fixed order: the four
            // of a row of 16 lanes (row_shr 4, 8: lane 16 r + 12 + h), then the four rows (one LDS read per lane, not
            // 64 values per thread)
            double sv = reinterpret_cast<const double *>(slot)[lane];
            sv = dpp_add<0x114, 0xf>(sv);
            sv = dpp_add<0x118, 0xf>(sv);
            double t[4];
#pragma unroll
            for (int h = 0; h < 4; ++h)
                t[h] = ((readlane_d(sv, 12 + h) + readlane_d(sv, 28 + h)) + readlane_d(sv, 44 + h)) + readlane_d(sv, 60 + h);
            // the orbit's four cells, one after the other (same arithmetic per cell as sweep_kernel); thread h < 4
            // stores cell h
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const int j = cur.j[h];
                const double cp = kp[j];
                const double g = 2.0 * t[h] + kgr[j];
                double pv = 0.0;
                if (mode & SW_PFIN) {
                    const double pf = cp - a.c_p * g;
                    pp += pf * pf;
                    pv = pf;
                }
                if (mode & SW_UPD) {
                    const double chi = khi[j], clo = klo[j];
                    const double psrc = (mode & SW_SPEC) ? kpn[j] : cp;
                    double pj = psrc - a.c_u * g;
                    double xj = xh[h] + a.dt * pj;
                    if (xj > chi) {
                        xj = chi;
                        pj = -pj;
                    } else if (xj < clo) {
                        xj = clo;
                        pj = -pj;
                    }
                    pv = pj;
                    xh[h] = xj;
                }
                if (tid == h) {
                    if (mode & SW_GOUT) a.g_out[j] = (mode & SW_GACC) ? a.g_out[j] + g : g;
                    if (mode & SW_UPD) {
                        a.p_out[j] = pv;
                        a.x_out[j] = xh[h];
                    } else if ((mode & SW_PFIN) && !(mode & SW_SPEC)) {
                        a.p_out[j] = pv;
                    }
                }
            }
        }
        if (mode & SW_FWD) {
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
    };

    if (cnt > 0) {
        FoldCol<EPT2> b0, b1;
        load_idx(orb(0));
        load_col(b0, orb(0), orb(1));
        int i = 0;
        for (;;) {
            load_col(b1, orb(i + 1), orb(i + 2));
            process(b0, i);
            if (++i >= cnt) break;
            load_col(b0, orb(i + 1), orb(i + 2));
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

}  // namespace ghk
