// libgravhmc host side: the per-evaluation epilogue (slab -> d, regulariser, residual, scalars)
// and the work buffers.  Included once by gravhmc.hip.
#pragma once

// rows of the slab the last forward launch wrote
static int slab_rows_live(const gh_ctx *c) { return c->slab_live > 0 ? c->slab_live : c->grid; }

// slab -> d ; regulariser ; residual + scalars.  x: position the forward belongs to.
// slab (c->grid rows) -> d_out (+ per-block partial sums of d + grav_fix).  Many slab rows
// (small problems spread over many workgroups) are summed in two passes so that no thread walks
// hundreds of rows serially.
static void reduce_slab(gh_ctx *c, const double *gfix, double *d_out)
{
    const dim3 blocks(c->work.n_dpart, 1), threads(32, 8);
    if (c->joint) {
        // the joint store: the first half of the live slab rows sums to d_gz, the second to d_tf ([gz: ld | tf: ld]) --
        // the sweep's workgroups, or on the table the forward's chunks of layers
        const int half = slab_rows_live(c) / 2;
        for (int h = 0; h < 2; ++h)
            reduce_slab_kernel<<<blocks, threads, 0, c->stream>>>(c->slab + (int64_t)h * half * c->ld, half, c->ld,
                                                                  store_points(c), nullptr, d_out + h * c->ld, c->dpart);
        return;
    }
    (void)lonsym_post_now(c);  // (harmonic shift-invariant store: the sweep left D^ partials, not a slab row)
    const int rows = slab_rows_live(c);
    if (rows > 64 && c->slab2) {
        const int nseg = c->work.slab2_rows;
        reduce_slab_kernel<<<dim3(c->work.n_dpart, nseg), threads, 0, c->stream>>>(c->slab, rows, c->ld, c->N, nullptr,
                                                                                 c->slab2, c->dpart);
        reduce_slab_kernel<<<blocks, threads, 0, c->stream>>>(c->slab2, nseg, c->ld, c->N, gfix, d_out, c->dpart);
    } else {
        reduce_slab_kernel<<<blocks, threads, 0, c->stream>>>(c->slab, rows, c->ld, c->N, gfix, d_out, c->dpart);
    }
}

// The joint store's epilogue: the existing epilogue kernels run once per block, on that block's half of the
// slab rows, of d, r, dobsw and of the model, with no mean (reduce_finish_kernel with no slab-row sums and no
// grav_fix removes a mean of exactly 0.0: r = d - dobsw) and the regulariser of that block alone (the
// stencil of fd3djoint: the regulariser does not couple the blocks; the cross-gradient term, when switched on,
// follows in a launch of its own).  Partials: |r|^2 of gz, of tf, then R of gz, of tf (then Phi) -- scal_kernel
// (scal_cg_kernel) sums them.  Below 2048 rows (few 32-row blocks for many slab rows) reduce_reg_kernel first
// folds the block's slab rows into slab2 segments, as the single-property path does: more than 64 slab rows per
// block (slab2 exists whenever the grid has more than 64, host_layout.h).
static bool joint_two_stage(const gh_ctx *c) { return c->joint && c->ld < 2048 && slab_rows_live(c) / 2 > 64; }

// The cross-gradient coupling at x (2m), both blocks in one launch: g (or null) takes lambda dPhi/dmw -- added to
// what is there (the epilogue: behind the two blocks' regulariser) or stored --, t (or null) the vectors, part the
// ceil(m / 256) partials of Phi.
static void launch_cross_gradient(gh_ctx *c, const double *x, double lambda, double *g, bool add, double *t, double *part)
{
    const gh_ctx::CrossGrad &cg = c->cg;
    CrossGradArgs a{};
    a.m = store_cells(c);
    a.nz = cg.shape[0];
    a.ny = cg.shape[1];
    a.nx = cg.shape[2];
    a.lambda = lambda;
    a.ihx = cg.ihx;
    a.ihy = cg.ihy;
    a.ihz = cg.ihz;
    a.x = x;
    a.sw = cg.sw;
    a.g = g;
    a.t = t;
    a.part = part;
    hipLaunchKernelGGL(add ? cross_gradient_kernel<true> : cross_gradient_kernel<false>, dim3((unsigned)((a.m + 255) / 256)),
                       dim3(256), 0, c->stream, a);
}

static bool cross_gradient_on(const gh_ctx *c) { return c->joint && c->cg.set && c->cg.lambda > 0.0; }

// The amplitude coupling of the magnetization-vector store at x (M = 3m): g (or null) takes lambda dPhi/dmw -- added
// to what is there (the epilogue: behind the regulariser) or stored --, amp (or null) the cells' amplitudes, part
// the ceil(m / 256) partials of Phi.
static void launch_amplitude(gh_ctx *c, const double *x, double lambda, double *g, bool add, double *amp, double *part)
{
    AmpArgs a{};
    a.m = store_cells(c);
    a.lambda = lambda;
    a.beta = c->amp.beta;
    a.scale = c->amp.scale;
    a.x = x;
    a.sw = c->amp.sw;
    a.g = g;
    a.amp = amp;
    a.part = part;
    hipLaunchKernelGGL(add ? amplitude_kernel<true> : amplitude_kernel<false>, dim3((unsigned)((a.m + 255) / 256)), dim3(256), 0,
                       c->stream, a);
}

static bool amplitude_on(const gh_ctx *c) { return c->mvi && c->amp.set && c->amp.lambda > 0.0; }

// a coupling term rides on the evaluations: its Phi has a slot per state set and lambda Phi is part of U
static bool coupling_on(const gh_ctx *c) { return cross_gradient_on(c) || amplitude_on(c); }

// properties stacked in the model vector, each regularised on its own (RegArgs::nprop)
static int reg_props(const gh_ctx *c) { return c->joint ? 2 : c->mvi ? 3 : 1; }

// The regulariser at x, alpha grad R to greg, partials to c->regpart (the callers that keep them in a state set's
// `part` point regpart there).  prop < 0: the whole model vector in one launch -- stores of several properties:
// block by block on each, RegArgs::nprop (fd3djoint: the stencil never crosses into the next block).  prop >= 0:
// that property alone, as the joint epilogue runs it.
static RegArgs reg_args(const gh_ctx *c, const double *x, double *greg, int prop)
{
    const WorkLayout &w = c->work;
    const int64_t m = c->M / w.props, off = prop > 0 ? prop * m : 0;
    RegArgs ra{};
    ra.kind = c->reg_kind;
    ra.M = w.props > 1 ? m : c->M;
    ra.nz = c->shape[0];
    ra.ny = c->shape[1];
    ra.nx = c->shape[2];
    ra.alpha = c->alpha;
    ra.beta = c->beta;
    ra.x = x + off;
    ra.mwapr = c->mwapr + off;
    ra.wm2 = c->wm2 + off;
    ra.greg = greg + off;
    ra.regpart = c->regpart;
    if (prop < 0 && w.props > 1) {
        ra.nprop = w.props;
        ra.nrb = w.reg_blocks;
    }
    return ra;
}

// reduce_finish_kernel's arguments for block h of the observations (joint store: 0 gz, 1 tf; every other store: 0,
// all of them): `rows` slab rows -> d, r of the block, its |r|^2 partials, and the regulariser ra with its own.
// (zero: no sums of the slab rows and no grav_fix, a mean of exactly 0.0 is removed -- the joint store's case)
static ReduceFinishArgs reduce_finish_args(const gh_ctx *c, const gh_ctx::StateSet &o, int h, const double *slab, int rows,
                                           const RegArgs &ra, int n_reg)
{
    const int64_t off = h * c->ld;
    ReduceFinishArgs fa{};
    fa.slab = slab;
    fa.n_rows_slab = rows;
    fa.n_dpart = c->work.n_dpart;
    fa.n_regpart = n_reg;
    fa.ld = c->ld;
    fa.dobs_c = c->dobs_c + off;
    fa.d = o.d + off;
    fa.r = o.r + off;
    fa.scal = o.scal;
    fa.r2part = o.part + c->work.r2(h);
    fa.ra = ra;
    return fa;
}

static int finalize_joint(gh_ctx *c, const double *x, const gh_ctx::StateSet &o)
{
    const WorkLayout &w = c->work;
    const int half = slab_rows_live(c) / 2;
    const bool two_stage = joint_two_stage(c);
    if (two_stage && !c->slab2) return fail(c, GH_ERR_ARG, "joint epilogue: no slab2 (ensure_work not run)");
    for (int h = 0; h < 2; ++h) {
        RegArgs ra = reg_args(c, x, o.greg, h);
        ra.regpart = o.part + w.reg(h);
        const double *slab = c->slab + (int64_t)h * half * c->ld;
        int rows = half, n_reg = w.reg_blocks;
        if (two_stage) {
            double *seg = c->slab2 + (int64_t)h * w.slab2_rows * c->ld;
            reduce_reg_kernel<<<dim3((unsigned)(w.n_dpart * w.slab2_rows + n_reg)), dim3(256), 0, c->stream>>>(
                slab, half, c->ld, w.slab2_rows, w.n_dpart, seg, ra);
            slab = seg;
            rows = w.slab2_rows;
            n_reg = 0;  // (done)
        }
        ReduceFinishArgs fa = reduce_finish_args(c, o, h, slab, rows, ra, n_reg);
        fa.N = store_points(c);
        reduce_finish_kernel<false><<<dim3((unsigned)(w.n_dpart + n_reg)), dim3(256), 0, c->stream>>>(fa);
    }
    // the coupling: lambda grad Phi on top of both blocks' alpha grad R, its partials behind those of R
    if (cross_gradient_on(c)) launch_cross_gradient(c, x, c->cg.lambda, o.greg, true, nullptr, o.part + w.coupling());
    HIPCHK(c, hipGetLastError());
    o.pending = true;
    return GH_OK;
}

// ---- the single-property epilogues: one chooser, one function per form

enum EpiForm { EPI_JOINT, EPI_ROWS, EPI_CELLS, EPI_WAVELET, EPI_LONSYM_FUSED, EPI_ONE_LAUNCH, EPI_TWO_STAGE, EPI_PLAIN };

// harmonic shift-invariant store: the sweep left D^ partials; either the fused epilogue consumes them or they are
// turned into the slab row first (lonsym_post_now)
static bool lonsym_fused_epilogue(const gh_ctx *c, const gh_ctx::StateSet &o)
{
    return lonsym_harmonic(c) && c->ls->fused && c->ls->post_pending && o.part;
}

static EpiForm epilogue_form(const gh_ctx *c, const gh_ctx::StateSet &o)
{
    if (c->joint) return EPI_JOINT;
    if (shard_rows(c)) return EPI_ROWS;
    if (c->sh.kind != 0) return EPI_CELLS;
    if (c->wv.on) return EPI_WAVELET;
    if (lonsym_fused_epilogue(c, o)) return EPI_LONSYM_FUSED;
    // the slab rows' sums at hand (and N >= 2048); the multi-component store's sums per row block come from a
    // launch of their own, whatever N
    if ((c->dsum_live || c->mc.n > 0) && o.part) return EPI_ONE_LAUNCH;
    if (c->grid > 64 && c->slab2) return EPI_TWO_STAGE;
    return EPI_PLAIN;
}

// what FinishArgs and RowsFinishArgs share: nseg rows of src -> d, r, scalars, with the sum of n_regpart partials of R
template <typename Args>
static void finish_fields(Args &fa, const gh_ctx *c, const gh_ctx::StateSet &o, const double *src, int nseg,
                          const double *regpart, int n_regpart)
{
    fa.N = c->N;
    fa.ld = c->ld;
    fa.nseg = nseg;
    fa.n_regpart = n_regpart;
    fa.src = src;
    fa.gfix = c->have_fix ? c->gfix : nullptr;
    fa.dobs_c = c->dobs_c;
    fa.regpart = regpart;
    fa.alpha = c->alpha;
    fa.d = o.d;
    fa.r = o.r;
    fa.scal = o.scal;
}

// The forms that leave no partials end in the single-block finish_kernel: nseg rows of src -> d, mean, r, scalars.
// (magnetization-vector store, coupling on: one launch behind the regulariser's adds lambda grad Phi; its partials
// go to a buffer finish_kernel sums)
static int epi_finish(gh_ctx *c, const double *x, const gh_ctx::StateSet &o, const double *src, int nseg,
                      const double *regpart, int n_regpart)
{
    o.pending = false;
    FinishArgs fa{};
    if (amplitude_on(c)) {
        launch_amplitude(c, x, c->amp.lambda, o.greg, true, nullptr, c->amppart);
        fa.cpart = c->amppart;
        fa.n_cpart = (int)c->work.amppart;
        fa.lambda = c->amp.lambda;
        fa.phi = o.phi;
    }
    finish_fields(fa, c, o, src, nseg, regpart, n_regpart);
    finish_kernel<<<dim3(1), dim3(1024), 0, c->stream>>>(fa);
    HIPCHK(c, hipGetLastError());
    return GH_OK;
}

// observations sharded over the ranks: d, r of the local rows; the mean and |r|^2 are sums over all ranks (two
// scalar all-reduces); the regulariser is replicated with the model
static int epi_rows(gh_ctx *c, const double *x, const gh_ctx::StateSet &o, const RegArgs &ra)
{
    reg_kernel<<<dim3(c->work.n_regpart), dim3(256), 0, c->stream>>>(ra);
    RowsFinishArgs fa{};
    int nseg = slab_rows_live(c);
    if (c->wv.on) {
        // the local rows of the compressed operator (every rank compressed its own rows of Aw): one finished row
        TRY(wavelet_forward(c, x, c->slab));
        nseg = 1;
    }
    finish_fields(fa, c, o, c->slab, nseg, c->regpart, c->work.n_regpart);
    fa.N_global = c->sh.N_global;
    fa.rbuf = c->sh.rbuf;
    rows_stage_a_kernel<<<dim3(1), dim3(1024), 0, c->stream>>>(fa);
    TRY(comm_allreduce(c, c->sh.rbuf, 1));
    rows_stage_b_kernel<<<dim3(1), dim3(1024), 0, c->stream>>>(fa);
    TRY(comm_allreduce(c, c->sh.rbuf + 1, 1));
    rows_stage_c_kernel<<<dim3(1), dim3(1024), 0, c->stream>>>(fa);
    HIPCHK(c, hipGetLastError());
    o.pending = false;
    return GH_OK;
}

// sharded cells: local forward partial and local regulariser sum travel in ONE all-reduce, then every rank
// finishes the (replicated) data part identically
static int epi_cells(gh_ctx *c, const double *x, const gh_ctx::StateSet &o, RegArgs ra)
{
    gh_ctx::Shard &sh = c->sh;
    const int n_reg = c->work.n_regpart;
    double *buf = sh.buf, *regsum = buf + c->ld;
    reduce_slab(c, nullptr, buf);
    if (sh.halo) {
        // stencil regulariser: the boundary planes of x travel with the forward partial, the regulariser (which
        // needs them) is summed by a second, two-double all-reduce
        const int64_t P = sh.P, nh = 2 * (int64_t)sh.world * P;
        double *hb = buf + c->ld + 8;
        halo_pack_kernel<<<dim3((unsigned)std::min<int64_t>(1024, (nh + 255) / 256)), dim3(256), 0, c->stream>>>(
            x, c->M, P, sh.rank, sh.world, hb);
        TRY(comm_allreduce(c, buf, (int64_t)c->ld + 8 + nh));
        ra.k0 = sh.m0 / P;
        ra.xlo = sh.rank > 0 ? hb + ((int64_t)(sh.rank - 1) * 2 + 1) * P : nullptr;
        ra.xhi = sh.rank + 1 < sh.world ? hb + (int64_t)(sh.rank + 1) * 2 * P : nullptr;
        ra.alo = sh.alo;
        ra.ahi = sh.ahi;
        regsum = sh.rb;
    }
    reg_kernel<<<dim3(n_reg), dim3(256), 0, c->stream>>>(ra);
    sum_kernel<<<dim3(1), dim3(1024), 0, c->stream>>>(c->regpart, n_reg, regsum);
    TRY(sh.halo ? comm_allreduce(c, sh.rb, 2) : comm_allreduce(c, buf, c->ld + 2));
    return epi_finish(c, x, o, buf, 1, regsum, 1);
}

// forward through the compressed operator: d is already complete
static int epi_wavelet(gh_ctx *c, const double *x, const gh_ctx::StateSet &o, const RegArgs &ra)
{
    TRY(wavelet_forward(c, x, o.d));
    reg_kernel<<<dim3(c->work.n_regpart), dim3(256), 0, c->stream>>>(ra);
    return epi_finish(c, x, o, o.d, 1, c->regpart, c->work.n_regpart);
}

// harmonic shift-invariant store: partial sums -> d -> mean -> r -> R^ of the next adjoint, and the regulariser,
// in ONE launch (lonsymh_epilogue_kernel)
static int epi_lonsym_fused(gh_ctx *c, const gh_ctx::StateSet &o, const RegArgs &ra)
{
    const WorkLayout &w = c->work;
    LonSymHost &h = *c->ls;
    LhEpiArgs e{};
    e.nparts = h.hgrid;
    e.n_dpart = w.n_dpart;
    e.ld = c->ld;
    e.N = c->N;
    e.gfix = c->have_fix ? c->gfix : nullptr;
    e.dobs_c = c->dobs_c;
    e.d = o.d;
    e.r = o.r;
    e.scal = o.scal;
    e.r2part = o.part + w.r2(0);
    e.csum = h.csum;
    TRY(xg_prepare(c, h.epi, false, 1));
    e.tag = ++h.epi.tag;
    e.abort_w = h.epi.abort_w;
    e.ra = ra;
    e.ra.regpart = o.part + w.reg(0);
    lonsymh_epilogue_kernel<<<dim3((unsigned)(h.na + w.n_regpart)), dim3(256), 0, c->stream>>>(lonsymh_geom(c), e);
    HIPCHK(c, hipGetLastError());
    h.post_pending = false;
    h.rhat_of = o.r;
    o.pending = true;
    return GH_OK;
}

// the whole epilogue in one launch, partials left in o.part (scal_ready sums them once per trajectory)
static int epi_one_launch(gh_ctx *c, const double *x, const gh_ctx::StateSet &o, const RegArgs &ra)
{
    const WorkLayout &w = c->work;
    const double *gfix = c->have_fix ? c->gfix : nullptr;
    RegArgs rp = ra;
    rp.regpart = o.part + w.reg(0);
    ReduceFinishArgs fa = reduce_finish_args(c, o, 0, c->slab, slab_rows_live(c), rp, w.n_regpart);
    fa.N = c->N;
    fa.dsum = c->dsum;
    fa.n_dsum = c->dsum_n > 0 ? c->dsum_n : fa.n_rows_slab;
    fa.gfix_sum = gfix ? c->gfix_sum : 0.0;
    fa.gfix = gfix;
    const dim3 grid((unsigned)(w.n_dpart + w.n_regpart));
    if (c->mc.n > 0) {
        // one mean per component: r_b = (d_b - mean d_b) - (dobs_b - mean dobs_b) in every row block
        fa.nblk = c->mc.n;
        fa.Nb = store_points(c);
        fa.bmean = c->mc.bmean;
        fa.dsum = c->mc.bsum;
        fa.n_dsum = fa.n_rows_slab;
        if (lonsym_one_row(c)) {
            // (the shift-invariant table: the pass delivered the sum of every class, block after block -- the
            // classes of block b are its n_dsum partials, summed in index order)
            fa.n_dsum = lonsym_classes(c) / c->mc.n;
        } else {
            slab_block_sums_kernel<<<dim3((unsigned)fa.n_rows_slab), dim3(256), 0, c->stream>>>(c->slab, c->ld, fa.Nb, fa.nblk,
                                                                                                c->mc.bsum);
        }
        reduce_finish_kernel<true><<<grid, dim3(256), 0, c->stream>>>(fa);
    } else {
        reduce_finish_kernel<false><<<grid, dim3(256), 0, c->stream>>>(fa);
    }
    // (magnetization-vector store, coupling on: lambda grad Phi behind the regulariser's, its partials behind those of R)
    if (amplitude_on(c)) launch_amplitude(c, x, c->amp.lambda, o.greg, true, nullptr, o.part + w.coupling());
    HIPCHK(c, hipGetLastError());
    o.pending = true;
    return GH_OK;
}

// many slab rows: first stage of the reduction and the regulariser share one launch, finish_kernel sums the segments
static int epi_two_stage(gh_ctx *c, const double *x, const gh_ctx::StateSet &o, const RegArgs &ra)
{
    const WorkLayout &w = c->work;
    reduce_reg_kernel<<<dim3((unsigned)(w.n_dpart * w.slab2_rows + w.n_regpart)), dim3(256), 0, c->stream>>>(
        c->slab, slab_rows_live(c), c->ld, w.slab2_rows, w.n_dpart, c->slab2, ra);
    return epi_finish(c, x, o, c->slab2, w.slab2_rows, c->regpart, w.n_regpart);
}

static int epi_plain(gh_ctx *c, const double *x, const gh_ctx::StateSet &o, const RegArgs &ra)
{
    reg_kernel<<<dim3(c->work.n_regpart), dim3(256), 0, c->stream>>>(ra);
    return epi_finish(c, x, o, c->slab, slab_rows_live(c), c->regpart, c->work.n_regpart);
}

static int finalize(gh_ctx *c, const double *x, const gh_ctx::StateSet &o)
{
    const EpiForm form = epilogue_form(c, o);
    if (form == EPI_JOINT) return finalize_joint(c, x, o);
    if (form != EPI_LONSYM_FUSED) TRY(lonsym_post_now(c));
    const RegArgs ra = reg_args(c, x, o.greg, -1);
    if (form == EPI_ROWS) return epi_rows(c, x, o, ra);
    // (the multi-component store has one epilogue, the one with a mean per row block: never the single-mean forms)
    if (c->mc.n > 0 && !o.part)
        return fail(c, GH_ERR_ARG, "multi-component epilogue: the state set has no partials (ensure_work not run)");
    switch (form) {
    case EPI_CELLS: return epi_cells(c, x, o, ra);
    case EPI_WAVELET: return epi_wavelet(c, x, o, ra);
    case EPI_LONSYM_FUSED: return epi_lonsym_fused(c, o, ra);
    case EPI_ONE_LAUNCH: return epi_one_launch(c, x, o, ra);
    case EPI_TWO_STAGE: return epi_two_stage(c, x, o, ra);
    default: return epi_plain(c, x, o, ra);
    }
}

// scal[0..2] of a state set, summed from the partials of a one-launch epilogue if still pending
static int scal_ready(gh_ctx *c, const gh_ctx::StateSet &o)
{
    if (!o.pending) return GH_OK;
    const WorkLayout &w = c->work;
    // (|r|^2 partials of all blocks, then R partials of all properties, then those of the coupling term)
    const int nd = (int)w.reg(0), nr = (int)(w.coupling() - w.reg(0));
    if (cross_gradient_on(c))
        scal_cg_kernel<<<dim3(1), dim3(1024), 0, c->stream>>>(o.part, nd, nr, w.reg_blocks, c->alpha, c->cg.lambda, o.scal, o.phi);
    else if (amplitude_on(c))
        scal_cg_kernel<<<dim3(1), dim3(1024), 0, c->stream>>>(o.part, nd, nr, w.reg_blocks, c->alpha, c->amp.lambda, o.scal, o.phi);
    else
        scal_kernel<<<dim3(1), dim3(1024), 0, c->stream>>>(o.part, nd, nr, c->alpha, o.scal);
    HIPCHK(c, hipGetLastError());
    o.pending = false;
    return GH_OK;
}

// scal[0..3] of a state set through the pinned buffer; U3: {U, |r|^2 term, R term}, the order the chain keeps them in
static int read_state_scalars(gh_ctx *c, const gh_ctx::StateSet &o, double U3[3])
{
    double *h = c->h_scal + c->work.h_state();
    TRY(d2h(c, h, o.scal, 4));
    U3[0] = h[2];
    U3[1] = h[0];
    U3[2] = h[1];
    return GH_OK;
}

// one double of the device through the pinned buffer
static int read_value(gh_ctx *c, const double *src, double *value)
{
    double *h = c->h_scal + c->work.h_state();
    TRY(d2h(c, h, src, 1));
    *value = *h;
    return GH_OK;
}

// forward sweep of x (device) + finalize
static int eval_forward(gh_ctx *c, const double *x, const gh_ctx::StateSet &o)
{
    if (!c->wv.on) {
        SweepArgs a{};
        a.mode = SW_FWD;
        a.x_in = x;
        a.slab = c->slab;
        TRY(launch_sweep(c, a));
    }
    return finalize(c, x, o);
}

// The work buffers: allocated once, at the first evaluation, by the layout of the context as it stands then.  Every
// later call computes the layout again and refuses a context that has outgrown them (work_claim, host_sweep.h).
static int ensure_work(gh_ctx *c, const char *who = "evaluation")
{
    const size_t M = (size_t)c->M;
    if (c->work_ready) {
        const WorkLayout now = work_layout(work_shape(c));
        // (row shards set up after an evaluation: the one buffer whose existence, not size, depends on the call order)
        if (now.gbuf) TRY(dalloc(c, &c->gbuf, M));
        return work_claim(c, who, work_demand_of(now));
    }
    c->work_epilogue1 = env_int("GRAVHMC_EPILOGUE1", 1) != 0;
    const WorkLayout w = work_layout(work_shape(c));
    // (joint store: observation-space vectors [gz: ld | tf: ld]; slab rows stay c->ld long: a workgroup's partial
    // forward product covers its own block)
    const size_t ld = (size_t)c->ld * (c->joint ? 2 : 1);
    TRY(dalloc(c, &c->scal_all, 16));
    // (joint and magnetization-vector stores: Phi of the coupling term per state set)
    if (w.props > 1) TRY(dalloc(c, &c->cg.phi_all, 4));
    for (int i = 0; i < 4; ++i) {
        gh_ctx::StateSet &st = c->st[i];
        TRY(dalloc(c, &st.r, ld));
        TRY(dalloc(c, &st.greg, M));
        TRY(dalloc(c, &st.d, ld));
        if (w.part_form != WORK_PART_NONE) TRY(dalloc(c, &st.part, (size_t)w.size()));
        st.scal = c->scal_all + 4 * i;
        if (w.props > 1) st.phi = c->cg.phi_all + i;
        TRY(dalloc(c, &c->xb[i], M));
    }
    for (double **v : {&c->pb[0], &c->pb[1], &c->pn, &c->tmpM, &c->low, &c->high, &c->mwapr, &c->wm2}) TRY(dalloc(c, v, M));
    TRY(dalloc(c, &c->tmpN, ld));
    if (w.gbuf) TRY(dalloc(c, &c->gbuf, M));
    TRY(dalloc(c, &c->slab, (size_t)w.slab_rows * (size_t)c->ld));
    if (w.slab2_rows > 0) TRY(dalloc(c, &c->slab2, (size_t)w.slab2_rows * ld));
    if (w.bsum > 0) {
        TRY(dalloc(c, &c->mc.bsum, (size_t)w.bsum));
        TRY(dalloc(c, &c->mc.bmean, (size_t)c->mc.n));
    }
    if (w.dsum > 0) TRY(dalloc(c, &c->dsum, (size_t)w.dsum));
    if (w.amppart > 0) TRY(dalloc(c, &c->amppart, (size_t)w.amppart));
    TRY(dalloc(c, &c->dpart, (size_t)w.n_dpart));
    TRY(dalloc(c, &c->regpart, (size_t)w.n_regpart));
    for (double **v : {&c->pp_part, &c->ppn_part}) TRY(dalloc(c, v, (size_t)w.pp));
    for (double **v : {&c->pp0_part, &c->pn0_part}) TRY(dalloc(c, v, (size_t)w.pp0));
    if (!c->h_scal) HIPCHK(c, hipHostMalloc((void **)&c->h_scal, w.h_size() * sizeof(double)));
    c->work = w;
    c->work_ready = true;
    return GH_OK;
}

static int need(gh_ctx *c, bool cond, const char *what)
{
    if (!cond) return fail(c, GH_ERR_ARG, "%s", what);
    return GH_OK;
}
