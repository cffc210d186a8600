// The joint gravity-magnetic store on the translation-invariant table (gfx950): GH_CELL_PRISM_JOINT set onto the
// table of lattice.hip.h (gh_set_cells_joint_table).
//
// The dense joint store is H = [A_gz Wm^-1 | s A_tf Wm^-1] over the same m cells under the same n points: block-diagonal
// in the stacked layout, the density columns meet the gz rows alone and the magnetization columns the tf rows alone.
// On the table the property of a column is one more layer coordinate, as the axis of a magnetization vector is
// (latmvi.hip.h): 2 nz layers, layer L = b nz + k, cell_of[L][a][b] = b m + cell (k, a, b), T[0 .. nz) the gz table of a
// gh_set_cells_prism context on the geometry and T[nz .. 2 nz) the tf table of a gh_set_cells_tf context, bit for bit
// (lat_fill_kernel<MF_E_GEN> / <MF_E_TF>, one launch each).  Unlike the axes of a vector the two properties do not
// share their rows: lat_pass_kernel<FWD, false, true> is the pass whose layer L reads and writes the observation
// block L / nz alone (lattice.hip.h, "Block-diagonal layers").  A 2 x 2 table of row blocks with two zero tables would
// run twice the passes over twice the memory for the same sums.  The gathers and the column norms run on the 2 nz
// layers as they are (lat_gather_x_kernel; lat_colnorm_blocks_kernel with its ONE table of weight 1; lat_gather_r_blocks_kernel
// with its TWO blocks of r ld apart and the weights {1, s}): host_lattice.h, the LAT_JOINT row.
//
// What is new here is the data balance s = std(A_gz) / std(A_tf): the population standard deviations over all n m
// entries of each unweighted block, which the dense store reads off its columns (joint_std_kernel) and the table has
// to weigh -- the entry T[b][k][u][v] stands for every (observation, cell) pair of offset (u, v) in layer k.
#pragma once

namespace ghk {

// pairs (p, a), p < np, a < nc, with p - a + nc - 1 = u: the multiplicity of an offset along one axis
__device__ __forceinline__ int lat_offset_pairs(int u, int nc, int np)
{
    return min(min(u, nc + np - 2 - u), min(nc, np) - 1) + 1;
}

// Two-pass population standard deviation of the two unweighted blocks from their tables (numpy.std, ddof 0): pass 0
// sums mult T, pass 1 mult (T - mean[blk])^2, mult = lat_offset_pairs(u) lat_offset_pairs(v).  blockIdx.y = block, l.nz =
// 2 nz layers; every thread keeps a compensated (Kahan) sum over its grid-stride share, the workgroup sums its 256
// threads and writes part[blk * gridDim.x + blockIdx.x] (the host sums the partials and divides by n m), as
// joint_std_kernel does on the dense store.
__global__ void __launch_bounds__(256) lat_joint_std_kernel(LatGeom l, int pass, const double *__restrict__ mean,
                                                            double *__restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ double red[4];
    const int blk = blockIdx.y;
    const int nzl = l.nz / 2;
    const int64_t UV = (int64_t)l.U * l.V, n = UV * nzl;
    const double *B = l.T + (int64_t)blk * n;
    const double mu = pass ? mean[blk] : 0.0;
    double s = 0.0, comp = 0.0;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * 256) {
        const int64_t uv = idx % UV;
        const int u = (int)(uv / l.V), v = (int)(uv - (int64_t)u * l.V);
        const double mult = (double)lat_offset_pairs(u, l.nx, l.px) * (double)lat_offset_pairs(v, l.ny, l.qy);
        double t = B[idx];
        if (pass) {
            t -= mu;
            t = t * t;
        }
        const double y = mult * t - comp;
        const double z = s + y;
        comp = (z - s) - y;
        s = z;
    }
    const double tot = block_allreduce_sum(s, red, 4);
    if (threadIdx.x == 0) part[(int64_t)blk * gridDim.x + blockIdx.x] = tot;
}

}  // namespace ghk
