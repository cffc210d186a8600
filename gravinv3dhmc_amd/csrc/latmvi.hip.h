// The magnetization-vector stores on the translation-invariant table (gfx950): the fill of lattice.hip.h's table for
// GH_CELL_PRISM_MVI_DATA set onto it (gh_set_cells_mvi_table).
//
// The unknown of cell (k, a, b) along axis ax is column ax m + cell, and both products sum over cells and axes alike:
//     d[p,q] = sum_ax sum_k sum_a sum_b T[ax][k][p-a+nx-1][q-b+ny-1] x[ax][k,a,b] / wm
// which is the table of lattice.hip.h with 3 nz "layers": layer L = ax nz + k, cell_of[L][a][b] = ax m + cell (k, a, b),
// T[L] the field of a unit magnetization along ax.  The passes, gathers, column norms and reductions of lattice.hip.h
// run on LatGeom::nz = 3 nz layers as they are; data components are its row blocks, T[b][L][u][v].  What is new is
// this fill: every magnetic prism field of a pair depends on (k, p - a, q - b) alone, and the nine (data component,
// axis) entries of a pair come from the same six corner sums (kernels.hip.h: prism_mvi_data_kernel).
#pragma once

namespace ghk {

// One thread per geometric offset (k, u, v), k < nzg = l.nz / 3: the corner sums of the pair with the smallest (p, q) of
// the offset, and of the pair with the largest, once each; T[b][ax nzg + k][u][v] (T2: the largest pair's) for every
// data block b of bc and every axis.  The arithmetic is prism_mvi_data_kernel's, expression for expression (whose tf
// sums are prism_mvi_kernel's): every entry IS the dense store's entry of its pair.  l.cell_of: the expanded map,
// whose first nzg layers are the geometry's cells (axis x: 0 m + cell).
__global__ void __launch_bounds__(256) lat_fill_mvi_kernel(const double *xp, const double *yp, const double *zp,
                                                           const double *bounds6, LatGeom l, int nzg, double3 dir,
                                                           BComps bc, double *T, double *T2)
{
#pragma clang fp contract(off)
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t UV = (int64_t)l.U * l.V;
    if (e >= UV * nzg) return;
    const int k = (int)(e / UV);
    const int64_t uv = e - k * UV;
    const int u = (int)(uv / l.V), v = (int)(uv - (int64_t)u * l.V);
    const int du = u - (l.nx - 1), dv = v - (l.ny - 1);  // p - a, q - b
    const int p0 = du > 0 ? du : 0, q0 = dv > 0 ? dv : 0;
    const int p1 = min(l.px - 1, du + l.nx - 1), q1 = min(l.qy - 1, dv + l.ny - 1);
    const double fx = dir.x, fy = dir.y, fz = dir.z;
    bool tf = false;
    for (int q = 0; q < bc.n; ++q) tf = tf || bc.comp[q] == BCOMP_TF;
    for (int h = 0; h < 2; ++h) {
        const int p = h ? p1 : p0, q = h ? q1 : q0;
        const int64_t i = l.obs_of[(int64_t)p * l.qy + q];
        const int64_t j = l.cell_of[((int64_t)k * l.nx + (p - du)) * l.ny + (q - dv)];
        double s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0, s6 = 0.0;
        double ax = 0.0, ay = 0.0, az = 0.0;
        prism_each_corner(xp[i], yp[i], zp[i], bounds6 + 6 * j, [&](double sign, double dx, double dy, double dz) {
#pragma clang fp contract(off)
            const PrismV w = prism_v6(dx, dy, dz);
            s1 += sign * w.v1;
            s2 += sign * w.v2;
            s3 += sign * w.v3;
            s4 += sign * w.v4;
            s5 += sign * w.v5;
            s6 += sign * w.v6;
            if (tf) {
                ax += sign * (fx * w.v1 + fy * w.v2 + fz * w.v3);
                ay += sign * (fx * w.v2 + fy * w.v4 + fz * w.v5);
                az += sign * (fx * w.v3 + fy * w.v5 + fz * w.v6);
            }
        });
        double *out = h ? T2 : T;
#pragma unroll
        for (int b = 0; b < BCOMP_MAX; ++b) {
            if (b < bc.n) {
                const int comp = bc.comp[b];
                const double ex = comp == BCOMP_TF ? ax : comp == BCOMP_BX ? s1 : comp == BCOMP_BY ? s2 : s3;
                const double ey = comp == BCOMP_TF ? ay : comp == BCOMP_BX ? s2 : comp == BCOMP_BY ? s4 : s5;
                const double ez = comp == BCOMP_TF ? az : comp == BCOMP_BX ? s3 : comp == BCOMP_BY ? s5 : s6;
                double *Tb = out + (int64_t)b * 3 * nzg * UV + (int64_t)k * UV + uv;
                Tb[0] = ex * TF_SCALE;
                Tb[(int64_t)nzg * UV] = ey * TF_SCALE;
                Tb[(int64_t)2 * nzg * UV] = ez * TF_SCALE;
            }
        }
    }
}

}  // namespace ghk
