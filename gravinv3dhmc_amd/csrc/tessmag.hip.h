// The magnetic induction of uniformly magnetized tesseroids (GH_CELL_TESS_MVI_DATA): bx, by, bz and the total
// field of a magnetization VECTOR per cell, on the adaptive 2x2x2 Gauss-Legendre engine of the gravity fields.
//
// Poisson's relation: with V_ab(o, c) the six second derivatives of the integral of dV / l over cell c, taken at the
// observation o in its local frame x north, y east, z up -- the unscaled sums of tess_comp_entry<COMP_GXX ..
// COMP_GZZ> (kernels.hip.h) -- the induction of the cell magnetized with m_c (A/m, uniform in the Cartesian sense)
// is, in that frame,
//     (B_x, B_y, B_zup) = CM T2NT  V(o, c)  Q(o, c)  m_c,        Q(o, c) = [n_o e_o u_o]^T [n_c e_c -u_c]
// with n, e, u the north, east and up unit vectors (ECEF) of the observation and of the cell's CENTRE (the
// midpoints of its lon / lat bounds; sub-tesseroids of the subdivision keep the parent's vector and frame): m_c is
// given north-east-DOWN at the cell, the outputs are bx = B_x (north), by = B_y (east), bz = -B_zup (down) at the
// observation.  ONE traversal of the subdivision per (observation, cell) pair serves all six sums: the distance /
// size test, the stack and the nodes do not depend on the field, only the leaf's last expression does -- so the
// traversal is the gravity fields' own (tess_traverse), called with a leaf of six sums.
#pragma once
#include "kernels.hip.h"

namespace ghk {

constexpr int TESS_MAG_FRAME = 9;  // doubles per cell of tess_mag_cellframe_kernel

// What depends on the cell alone, once per cell instead of once per pair: the ECEF unit vectors n_c, e_c and
// d_c = -u_c at the cell's centre, frame[9 c + 3 a + k] = component k of axis a (north, east, down).
__global__ void __launch_bounds__(256)
tess_mag_cellframe_kernel(const double *__restrict__ bounds6, int64_t m, double *__restrict__ frame)
{
#pragma clang fp contract(off)
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= m) return;
    const double d2r = 3.14159265358979323846 / 180;
    const double *b = bounds6 + 6 * c;
    const double lam = d2r * 0.5 * (b[0] + b[1]), phi = d2r * 0.5 * (b[2] + b[3]);
    const double sl = sin(lam), cl = cos(lam), sp = sin(phi), cp = cos(phi);
    double *f = frame + TESS_MAG_FRAME * c;
    f[0] = -sp * cl;
    f[1] = -sp * sl;
    f[2] = cp;
    f[3] = -sl;
    f[4] = cl;
    f[5] = 0.0;
    f[6] = -(cp * cl);
    f[7] = -(cp * sl);
    f[8] = -sp;
}

// The six second-derivative sums of one GLQ leaf, V[0..5] = xx, xy, xz, yy, yz, zz, from the node quantities they
// share.  Every sum keeps the expression and the operation order of its tess_comp_leaf counterpart (kernelxx ..
// kernelzz); cos(lon - lonc) serves the three leaves that take cos(lonc - lon) as well (the arguments are exact
// negations of each other and cos is even).
__device__ __forceinline__ void tess_mag_leaf(double lon, double sinlat, double coslat, double radius,
                                              const double (&lonc)[2], const double (&sinlatc)[2],
                                              const double (&coslatc)[2], const double (&rc)[2], double (&V)[6])
{
#pragma clang fp contract(off)
    const double r_sqr = radius * radius;
#pragma unroll
    for (int q = 0; q < 6; ++q) V[q] = 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const double coslon = cos(lon - lonc[i]);
        const double sinlon = sin(lonc[i] - lon);
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
                const double l5 = (l_sqr * l_sqr) * sl;
                const double t = rc[k] * kphi;
                const double deltay = rc[k] * coslatc[j] * sinlon;
                const double deltaz = rc[k] * cospsi - radius;
                V[0] += kappa * (3 * (t * t) - l_sqr) / l5;
                V[1] += kappa * 3 * rc_sqr * kphi * coslatc[j] * sinlon / l5;
                V[2] += kappa * 3 * rc[k] * kphi * deltaz / l5;
                V[3] += kappa * (3 * (deltay * deltay) - l_sqr) / l5;
                V[4] += kappa * 3. * deltay * deltaz / l5;
                V[5] += kappa * (3 * (deltaz * deltaz) - l_sqr) / l5;
            }
        }
    }
}

// One (observation, tesseroid) pair: tess_traverse (kernels.hip.h), the one traversal of every tesseroid field, with
// all six sums accumulated at every leaf, acc[q] += scale * V_leaf[q] as tess_comp_entry does for its one field.
__device__ void tess_mag_entry(double lon, double sinlat, double coslat, double radius, const double *bounds,
                               double ratio, int &error_code, unsigned long long &nleaf, bool &overflow,
                               double (&acc)[6])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int q = 0; q < 6; ++q) acc[q] = 0.0;
    tess_traverse(lon, sinlat, coslat, radius, bounds, ratio, error_code, nleaf, overflow,
                  [&](const double (&lonc)[2], const double (&sinlatc)[2], const double (&coslatc)[2],
                      const double (&rc)[2], double scale) {
#pragma clang fp contract(off)
                      double V[6];
                      tess_mag_leaf(lon, sinlat, coslat, radius, lonc, sinlatc, coslatc, rc, V);
#pragma unroll
                      for (int q = 0; q < 6; ++q) acc[q] += scale * V[q];
                  });
}

// The observations as the kernels read them: tess_convert_kernel's six outputs, n values each
struct TessMagObs {
    const double *lon, *sinlat, *coslat, *radius, *sinlon, *coslon;
};

// (bx, by, bz) at observation l of cell c magnetized 1 A/m along its axis a (north, east, down), unscaled:
// V (xx, xy, xz, yy, yz, zz) times column a of Q, the last row negated (z up -> z down).
__device__ __forceinline__ void tess_mag_compose(const double (&V)[6], const double (&no)[3], const double (&eo)[3],
                                                 const double (&uo)[3], const double *__restrict__ fa, double &bx,
                                                 double &by, double &bz)
{
#pragma clang fp contract(off)
    const double q0 = no[0] * fa[0] + no[1] * fa[1] + no[2] * fa[2];
    const double q1 = eo[0] * fa[0] + eo[1] * fa[1] + eo[2] * fa[2];
    const double q2 = uo[0] * fa[0] + uo[1] * fa[1] + uo[2] * fa[2];
    bx = V[0] * q0 + V[1] * q1 + V[2] * q2;
    by = V[1] * q0 + V[3] * q1 + V[4] * q2;
    bz = -(V[2] * q0 + V[4] * q1 + V[5] * q2);
}

__device__ __forceinline__ void tess_mag_obs_frame(const TessMagObs &o, int64_t l, double (&no)[3], double (&eo)[3],
                                                   double (&uo)[3])
{
#pragma clang fp contract(off)
    const double sp = o.sinlat[l], cp = o.coslat[l], sl = o.sinlon[l], cl = o.coslon[l];
    no[0] = -sp * cl;
    no[1] = -sp * sl;
    no[2] = cp;
    eo[0] = -sl;
    eo[1] = cl;
    eo[2] = 0.0;
    uo[0] = cp * cl;
    uo[1] = cp * sl;
    uo[2] = sp;
}

// The data weights of the row blocks, for the shift-invariant table (which takes them when it is filled)
struct BWeights {
    double w[BCOMP_MAX];
};

// Assembly of the tesseroid magnetization store: columns [K_N | K_E | K_D] of m cells each, rows in bc.n
// blocks of Nb observations (block b the data component bc.comp[b]), column-major with ld, as a
// GH_CELL_PRISM_MVI_DATA store.  One thread per (obs, cell) pair, obs fastest, laid out as tess_comp_kernel: one
// traversal, then the pair's entry of every (data block, axis block).  A tf block is fdir[3 l ..] . (bx, by, bz),
// the direction taken at the observation.  Threads walk the Nb rows of a block, then the ld - n Nb padding rows
// below the stack, which they zero.  Error codes per cell into err_cell, leaves and overflow into stats.
// WEIGHTED: every entry of block b times bw.w[b] (the table); without it the dense store's code, bit for bit.
template <bool WEIGHTED>
__device__ __forceinline__ void
tess_mag_body(const TessMagObs &o, const double *__restrict__ bounds6, const double *__restrict__ frame,
              const double *__restrict__ fdir, int64_t Nb, int64_t m, int64_t ld, double ratio, const BComps &bc,
              const BWeights &bw, double *__restrict__ A, int *__restrict__ err_cell, TessStats *stats)
{
#pragma clang fp contract(off)
    unsigned long long nleaf = 0;
    bool overflow = false;
    const int64_t Lr = Nb + (ld - bc.n * Nb);
    for (int64_t idx = (int64_t)blockIdx.x * 64 + threadIdx.x; idx < Lr * m; idx += (int64_t)gridDim.x * 64) {
        const int64_t c = idx / Lr, l = idx - c * Lr;
        if (l >= Nb) {
            const int64_t row = bc.n * Nb + (l - Nb);
            A[c * ld + row] = 0.0;
            A[(m + c) * ld + row] = 0.0;
            A[(2 * m + c) * ld + row] = 0.0;
            continue;
        }
        int error_code = 0;
        double V[6];
        tess_mag_entry(o.lon[l], o.sinlat[l], o.coslat[l], o.radius[l], bounds6 + 6 * c, ratio, error_code, nleaf,
                       overflow, V);
        if (error_code != 0) atomicAdd(&err_cell[c], error_code);
        double no[3], eo[3], uo[3];
        tess_mag_obs_frame(o, l, no, eo, uo);
        double fx = 0.0, fy = 0.0, fz = 0.0;
        if (fdir) {
            fx = fdir[3 * l];
            fy = fdir[3 * l + 1];
            fz = fdir[3 * l + 2];
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            double bx, by, bz;
            tess_mag_compose(V, no, eo, uo, frame + TESS_MAG_FRAME * c + 3 * a, bx, by, bz);
            const double tf = fx * bx + fy * by + fz * bz;
            // (coalesced: consecutive threads, consecutive rows of one column, in every block)
#pragma unroll
            for (int q = 0; q < BCOMP_MAX; ++q) {
                if (q < bc.n) {
                    const int comp = bc.comp[q];
                    const double v = comp == BCOMP_TF ? tf : comp == BCOMP_BX ? bx : comp == BCOMP_BY ? by : bz;
                    A[(a * m + c) * ld + q * Nb + l] = WEIGHTED ? (v * TF_SCALE) * bw.w[q] : v * TF_SCALE;
                }
            }
        }
    }
    tess_report(nleaf, overflow, stats);
}

// Dense assembly (gh_build_G of a GH_CELL_TESS_MVI_DATA context without the table)
__global__ void __launch_bounds__(64)
tess_mag_kernel(TessMagObs o, const double *__restrict__ bounds6, const double *__restrict__ frame,
                const double *__restrict__ fdir, int64_t Nb, int64_t m, int64_t ld, double ratio, BComps bc,
                double *__restrict__ A, int *__restrict__ err_cell, TessStats *stats)
{
    tess_mag_body<false>(o, bounds6, frame, fdir, Nb, m, ld, ratio, bc, BWeights{}, A, err_cell, stats);
}

// The shift-invariant table of the store (host_lonsym.h), ONE launch: the same body over synthetic points and the
// cells of longitude index 0.  With Nb = na1 n points (class, shift) -- class = (latitude, height) --, m = nc1 cell
// rows and ld = ldT the store's layout IS the table's,
//     T[(a nc1 + row) ldT + (b na1 + cls) n + d]:
// the axis block a is a coordinate of the table's row, the data block b one of the observation class.  fdir holds
// the direction of every synthetic point's class; every entry takes its block's data weight.
__global__ void __launch_bounds__(64)
tess_mag_table_kernel(TessMagObs o, const double *__restrict__ bounds6, const double *__restrict__ frame,
                      const double *__restrict__ fdir, int64_t Nb, int64_t m, int64_t ld, double ratio, BComps bc,
                      BWeights bw, double *__restrict__ T, int *__restrict__ err_cell, TessStats *stats)
{
    tess_mag_body<true>(o, bounds6, frame, fdir, Nb, m, ld, ratio, bc, bw, T, err_cell, stats);
}

// The field without a store: one workgroup per observation; thread t takes the cells t, t + 256, ... in mesh
// order, each with its own vector mag3[3 c ..] (north, east, down at the cell), and keeps one sum per axis; the
// block sum is in a fixed order (wave, then the four waves in turn).  res[l] is the component `comp` (BCOMP_*;
// the total field projects on fdir[3 l ..]), scaled once.
__global__ void __launch_bounds__(256)
tess_mag_result_kernel(TessMagObs o, const double *__restrict__ bounds6, const double *__restrict__ frame,
                       const double *__restrict__ fdir, const double *__restrict__ mag3, int64_t Nb, int64_t m,
                       double ratio, int comp, double *__restrict__ res, int *__restrict__ err_cell, TessStats *stats)
{
#pragma clang fp contract(off)
    __shared__ double red[4];
    unsigned long long nleaf = 0;
    bool overflow = false;
    const int64_t l = blockIdx.x;  // (the grid has Nb workgroups)
    double no[3], eo[3], uo[3];
    tess_mag_obs_frame(o, l, no, eo, uo);
    const double lon = o.lon[l], sinlat = o.sinlat[l], coslat = o.coslat[l], radius = o.radius[l];
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int64_t c = threadIdx.x; c < m; c += 256) {
        int error_code = 0;
        double V[6];
        tess_mag_entry(lon, sinlat, coslat, radius, bounds6 + 6 * c, ratio, error_code, nleaf, overflow, V);
        if (error_code != 0) atomicAdd(&err_cell[c], error_code);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            double bx, by, bz;
            tess_mag_compose(V, no, eo, uo, frame + TESS_MAG_FRAME * c + 3 * a, bx, by, bz);
            const double ma = mag3[3 * c + a];
            sx += bx * ma;
            sy += by * ma;
            sz += bz * ma;
        }
    }
    const double bx = block_allreduce_sum(sx, red, 4);
    const double by = block_allreduce_sum(sy, red, 4);
    const double bz = block_allreduce_sum(sz, red, 4);
    if (threadIdx.x == 0) {
        double v = comp == BCOMP_BX ? bx : comp == BCOMP_BY ? by : bz;
        if (comp == BCOMP_TF) v = fdir[3 * l] * bx + fdir[3 * l + 1] * by + fdir[3 * l + 2] * bz;
        res[l] = v * TF_SCALE;
    }
    tess_report(nleaf, overflow, stats);
}

}  // namespace ghk
