// libgravhmc host side: the per-evaluation epilogue (slab -> d, regulariser, residual, scalars)
// and the work buffers.  Included once by gravhmc.hip.
#pragma once

// slab -> d ; regulariser ; residual + scalars.  x: position the forward belongs to.
// slab (c->grid rows) -> d_out (+ per-block partial sums of d + grav_fix).  Many slab rows
// (small problems spread over many workgroups) are summed in two passes so that no thread walks
// hundreds of rows serially.
static void reduce_slab(gh_ctx *c, const double *gfix, double *d_out)
{
    if (c->joint) {
        // the joint store: the first half of the slab rows sums to d_gz, the second to d_tf ([gz: ld | tf: ld])
        const int half = c->grid / 2;
        for (int h = 0; h < 2; ++h)
            reduce_slab_kernel<<<dim3(c->n_dpart, 1), dim3(32, 8), 0, c->stream>>>(
                c->slab + (int64_t)h * half * c->ld, half, c->ld, store_points(c), nullptr, d_out + h * c->ld, c->dpart);
        return;
    }
    (void)lonsym_post_now(c);  // (harmonic shift-invariant store: the sweep left D^ partials, not a slab row)
    const int rows = c->slab_live > 0 ? c->slab_live : c->grid;
    if (rows > 64 && c->slab2) {
        const int nseg = c->slab2_rows;
        reduce_slab_kernel<<<dim3(c->n_dpart, nseg), dim3(32, 8), 0, c->stream>>>(c->slab, rows, c->ld, c->N,
                                                                                  nullptr, c->slab2, c->dpart);
        reduce_slab_kernel<<<dim3(c->n_dpart, 1), dim3(32, 8), 0, c->stream>>>(c->slab2, nseg, c->ld, c->N,
                                                                               gfix, d_out, c->dpart);
    } else {
        reduce_slab_kernel<<<dim3(c->n_dpart, 1), dim3(32, 8), 0, c->stream>>>(c->slab, rows, c->ld, c->N, gfix,
                                                                               d_out, c->dpart);
    }
}

// The joint store's epilogue: the existing epilogue kernels run once per block, on that block's half of the
// slab rows, of d, r, dobsw and of the model, with no mean (reduce_finish_kernel with no slab-row sums and no
// grav_fix removes a mean of exactly 0.0: r = d - dobsw) and the regulariser of that block alone (the
// stencil of fd3djoint: the regulariser does not couple the blocks; the cross-gradient term, when switched on,
// follows in a launch of its own).  Partials: |r|^2 of gz, of tf, then R of gz, of tf (then Phi) -- scal_kernel
// (scal_cg_kernel) sums them.  Below 2048 rows (few 32-row blocks for many slab rows) reduce_reg_kernel first
// folds the block's slab rows into slab2 segments, as the single-property path does.
// (two stages: fewer than 2048 rows and more than 64 slab rows per block; ensure_work then has slab2, as it
// allocates it whenever the grid has more than 64 rows)
static bool joint_two_stage(const gh_ctx *c)
{
    return c->joint && c->ld < 2048 && c->grid / 2 > 64;
}

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
    const dim3 grid((unsigned)((a.m + 255) / 256));
    if (add)
        cross_gradient_kernel<true><<<grid, dim3(256), 0, c->stream>>>(a);
    else
        cross_gradient_kernel<false><<<grid, dim3(256), 0, c->stream>>>(a);
}

static bool cross_gradient_on(const gh_ctx *c)
{
    return c->joint && c->cg.set && c->cg.lambda > 0.0;
}

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
    const dim3 grid((unsigned)((a.m + 255) / 256));
    if (add)
        amplitude_kernel<true><<<grid, dim3(256), 0, c->stream>>>(a);
    else
        amplitude_kernel<false><<<grid, dim3(256), 0, c->stream>>>(a);
}

static bool amplitude_on(const gh_ctx *c)
{
    return c->mvi && c->amp.set && c->amp.lambda > 0.0;
}

// a coupling term rides on the evaluations: its Phi has a slot per state set and lambda Phi is part of U
static bool coupling_on(const gh_ctx *c)
{
    return cross_gradient_on(c) || amplitude_on(c);
}

// properties stacked in the model vector, each regularised on its own (RegArgs::nprop)
static int reg_props(const gh_ctx *c)
{
    return c->joint ? 2 : c->mvi ? 3 : 1;
}

static int finalize_joint(gh_ctx *c, const double *x, const gh_ctx::StateSet &o)
{
    const int half = c->grid / 2;
    const int64_t m = store_cells(c), ld = c->ld;
    const int nrb = (int)((m + 255) / 256);  // regulariser blocks per property
    const bool two_stage = joint_two_stage(c);
    if (two_stage && !c->slab2) return fail(c, GH_ERR_ARG, "joint epilogue: no slab2 (ensure_work not run)");
    for (int h = 0; h < 2; ++h) {
        RegArgs ra{};
        ra.ms_grad_den_mw = 0;
        ra.kind = c->reg_kind;
        ra.M = m;
        ra.nz = c->shape[0];
        ra.ny = c->shape[1];
        ra.nx = c->shape[2];
        ra.alpha = c->alpha;
        ra.beta = c->beta;
        ra.x = x + h * m;
        ra.mwapr = c->mwapr + h * m;
        ra.wm2 = c->wm2 + h * m;
        ra.greg = o.greg + h * m;
        ra.regpart = o.part + 2 * c->n_dpart + h * nrb;
        ReduceFinishArgs fa{};
        fa.slab = c->slab + (int64_t)h * half * ld;
        fa.n_rows_slab = half;
        int n_reg = nrb;
        if (two_stage) {
            const int nseg = c->slab2_rows;
            double *seg = c->slab2 + (int64_t)h * nseg * ld;
            reduce_reg_kernel<<<dim3((unsigned)(c->n_dpart * nseg + nrb)), dim3(256), 0, c->stream>>>(
                fa.slab, half, ld, nseg, c->n_dpart, seg, ra);
            fa.slab = seg;
            fa.n_rows_slab = nseg;
            n_reg = 0;  // (done)
        }
        fa.n_dpart = c->n_dpart;
        fa.n_regpart = n_reg;
        fa.ld = ld;
        fa.N = store_points(c);
        fa.dsum = nullptr;
        fa.n_dsum = 0;
        fa.gfix_sum = 0.0;
        fa.gfix = nullptr;
        fa.dobs_c = c->dobs_c + h * ld;
        fa.d = o.d + h * ld;
        fa.r = o.r + h * ld;
        fa.scal = o.scal;
        fa.r2part = o.part + h * c->n_dpart;
        fa.ra = ra;
        reduce_finish_kernel<false><<<dim3((unsigned)(c->n_dpart + n_reg)), dim3(256), 0, c->stream>>>(fa);
    }
    // the coupling: lambda grad Phi on top of both blocks' alpha grad R, its partials behind those of R
    if (cross_gradient_on(c))
        launch_cross_gradient(c, x, c->cg.lambda, o.greg, true, nullptr, o.part + 2 * c->n_dpart + 2 * nrb);
    HIPCHK(c, hipGetLastError());
    o.pending = true;
    return GH_OK;
}

static int finalize(gh_ctx *c, const double *x, const gh_ctx::StateSet &o)
{
    if (c->joint) return finalize_joint(c, x, o);
    double *d_out = o.d, *r_out = o.r, *greg_out = o.greg, *scal_out = o.scal;
    RegArgs ra{};
    ra.ms_grad_den_mw = 0;
    ra.kind = c->reg_kind;
    ra.M = c->M;
    ra.nz = c->shape[0];
    ra.ny = c->shape[1];
    ra.nx = c->shape[2];
    ra.alpha = c->alpha;
    ra.beta = c->beta;
    ra.x = x;
    ra.mwapr = c->mwapr;
    ra.wm2 = c->wm2;
    ra.greg = greg_out;
    ra.regpart = c->regpart;
    if (c->mvi) {
        // (three properties of one mesh: the regulariser block by block on each, RegArgs::nprop)
        ra.M = store_cells(c);
        ra.nprop = 3;
        ra.nrb = (int)((ra.M + 255) / 256);
    }
    // (magnetization-vector store, coupling on: one launch behind the regulariser's adds lambda grad Phi; its
    // partials go behind those of R where the epilogue leaves partials, else to a buffer finish_kernel sums)
    const bool amp_on = amplitude_on(c);
    const double *gfix = c->have_fix ? c->gfix : nullptr;
    const double *regpart = c->regpart;
    int n_regpart = c->n_regpart;
    const double *src;
    int nseg;
    // harmonic shift-invariant store: the sweep left D^ partials; either the fused epilogue below consumes them or
    // they are turned into the slab row first
    const bool fused_epi = lonsym_harmonic(c) && c->ls->fused && c->ls->post_pending && o.part != nullptr;
    if (!fused_epi) TRY(lonsym_post_now(c));
    if (shard_rows(c)) {
        // observations sharded over the ranks: d, r of the local rows; the mean and |r|^2 are sums over all
        // ranks (two scalar all-reduces); the regulariser is replicated with the model
        reg_kernel<<<dim3(c->n_regpart), dim3(256), 0, c->stream>>>(ra);
        RowsFinishArgs fa{};
        fa.N = c->N;
        fa.ld = c->ld;
        fa.N_global = c->sh.N_global;
        fa.nseg = c->slab_live > 0 ? c->slab_live : c->grid;
        if (c->wv.on) {
            // the local rows of the compressed operator (every rank compressed its own rows of Aw): one finished row
            TRY(wavelet_forward(c, x, c->slab));
            fa.nseg = 1;
        }
        fa.n_regpart = c->n_regpart;
        fa.src = c->slab;
        fa.gfix = gfix;
        fa.dobs_c = c->dobs_c;
        fa.regpart = c->regpart;
        fa.alpha = c->alpha;
        fa.d = d_out;
        fa.r = r_out;
        fa.scal = scal_out;
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
    // (the multi-component store has one epilogue, the one with a mean per row block: never the single-mean forms below)
    if (c->mc.n > 0 && !o.part)
        return fail(c, GH_ERR_ARG, "multi-component epilogue: the state set has no partials (ensure_work not run)");
    if (c->sh.kind != 0) {
        // sharded cells: local forward partial and local regulariser sum travel in ONE
        // all-reduce, then every rank finishes the (replicated) data part identically
        double *buf = c->sh.buf;
        reduce_slab(c, nullptr, buf);
        if (c->sh.halo) {
            // stencil regulariser: the boundary planes of x travel with the forward partial, the
            // regulariser (which needs them) is summed by a second, two-double all-reduce
            gh_ctx::Shard &sh = c->sh;
            const int64_t P = sh.P, nh = 2 * (int64_t)sh.world * P;
            double *hb = buf + c->ld + 8;
            halo_pack_kernel<<<dim3((unsigned)std::min<int64_t>(1024, (nh + 255) / 256)), dim3(256), 0, c->stream>>>(
                x, c->M, P, sh.rank, sh.world, hb);
            TRY(comm_allreduce(c, buf, (int64_t)c->ld + 8 + nh));
            ra.nz = c->shape[0];
            ra.k0 = sh.m0 / P;
            ra.xlo = sh.rank > 0 ? hb + ((int64_t)(sh.rank - 1) * 2 + 1) * P : nullptr;
            ra.xhi = sh.rank + 1 < sh.world ? hb + (int64_t)(sh.rank + 1) * 2 * P : nullptr;
            ra.alo = sh.alo;
            ra.ahi = sh.ahi;
            reg_kernel<<<dim3(c->n_regpart), dim3(256), 0, c->stream>>>(ra);
            sum_kernel<<<dim3(1), dim3(1024), 0, c->stream>>>(c->regpart, c->n_regpart, sh.rb);
            TRY(comm_allreduce(c, sh.rb, 2));
            regpart = sh.rb;
        } else {
            reg_kernel<<<dim3(c->n_regpart), dim3(256), 0, c->stream>>>(ra);
            sum_kernel<<<dim3(1), dim3(1024), 0, c->stream>>>(c->regpart, c->n_regpart, buf + c->ld);
            TRY(comm_allreduce(c, buf, c->ld + 2));
            regpart = buf + c->ld;
        }
        src = buf;
        nseg = 1;
        n_regpart = 1;
    } else if (c->wv.on) {
        // forward through the compressed operator: d_out is already complete
        TRY(wavelet_forward(c, x, d_out));
        reg_kernel<<<dim3(c->n_regpart), dim3(256), 0, c->stream>>>(ra);
        src = d_out;
        nseg = 1;
    } else if (fused_epi) {
        // harmonic shift-invariant store: partial sums -> d -> mean -> r -> R^ of the next adjoint, and the
        // regulariser, in ONE launch (lonsymh_epilogue_kernel)
        LonSymHost &h = *c->ls;
        LhEpiArgs e{};
        e.nparts = h.hgrid;
        e.n_dpart = c->n_dpart;
        e.ld = c->ld;
        e.N = c->N;
        e.gfix = gfix;
        e.dobs_c = c->dobs_c;
        e.d = d_out;
        e.r = r_out;
        e.scal = scal_out;
        e.r2part = o.part;
        e.csum = h.csum;
        TRY(xg_prepare(c, h.epi, false, 1));
        e.tag = ++h.epi.tag;
        e.abort_w = h.epi.abort_w;
        e.ra = ra;
        e.ra.regpart = o.part + c->n_dpart;
        lonsymh_epilogue_kernel<<<dim3((unsigned)(h.na + c->n_regpart)), dim3(256), 0, c->stream>>>(lonsymh_geom(c), e);
        HIPCHK(c, hipGetLastError());
        h.post_pending = false;
        h.rhat_of = r_out;
        o.pending = true;
        return GH_OK;
    } else if ((c->dsum_live || c->mc.n > 0) && o.part) {
        // the slab rows' sums at hand (and N >= 2048): the whole epilogue in one launch
        // (multi-component store: the sums per row block come from a launch of their own, whatever N)
        ReduceFinishArgs fa{};
        fa.slab = c->slab;
        fa.n_rows_slab = c->slab_live > 0 ? c->slab_live : c->grid;
        fa.n_dpart = c->n_dpart;
        fa.n_regpart = c->n_regpart;
        fa.ld = c->ld;
        fa.N = c->N;
        fa.dsum = c->dsum;
        fa.n_dsum = c->dsum_n > 0 ? c->dsum_n : fa.n_rows_slab;
        fa.gfix_sum = gfix ? c->gfix_sum : 0.0;
        fa.gfix = gfix;
        fa.dobs_c = c->dobs_c;
        fa.d = d_out;
        fa.r = r_out;
        fa.scal = scal_out;
        fa.r2part = o.part;
        fa.ra = ra;
        fa.ra.regpart = o.part + c->n_dpart;
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
            reduce_finish_kernel<true><<<dim3((unsigned)(c->n_dpart + c->n_regpart)), dim3(256), 0, c->stream>>>(fa);
        } else {
            reduce_finish_kernel<false><<<dim3((unsigned)(c->n_dpart + c->n_regpart)), dim3(256), 0, c->stream>>>(fa);
        }
        if (amp_on) launch_amplitude(c, x, c->amp.lambda, greg_out, true, nullptr, o.part + c->n_dpart + c->n_regpart);
        HIPCHK(c, hipGetLastError());
        o.pending = true;
        return GH_OK;
    } else if (c->grid > 64 && c->slab2) {
        // many slab rows: first stage of the reduction and the regulariser share one launch,
        // finish_kernel sums the 16 segments
        nseg = c->slab2_rows;
        reduce_reg_kernel<<<dim3((unsigned)(c->n_dpart * nseg + c->n_regpart)), dim3(256), 0, c->stream>>>(
            c->slab, c->slab_live > 0 ? c->slab_live : c->grid, c->ld, nseg, c->n_dpart, c->slab2, ra);
        src = c->slab2;
    } else {
        reg_kernel<<<dim3(c->n_regpart), dim3(256), 0, c->stream>>>(ra);
        src = c->slab;
        nseg = c->slab_live > 0 ? c->slab_live : c->grid;
    }
    o.pending = false;
    FinishArgs fa{};
    if (amp_on) {
        launch_amplitude(c, x, c->amp.lambda, greg_out, true, nullptr, c->amppart);
        fa.cpart = c->amppart;
        fa.n_cpart = (int)((store_cells(c) + 255) / 256);
        fa.lambda = c->amp.lambda;
        fa.phi = o.phi;
    }
    fa.N = c->N;
    fa.ld = c->ld;
    fa.nseg = nseg;
    fa.n_regpart = n_regpart;
    fa.src = src;
    fa.gfix = gfix;
    fa.dobs_c = c->dobs_c;
    fa.regpart = regpart;
    fa.alpha = c->alpha;
    fa.d = d_out;
    fa.r = r_out;
    fa.scal = scal_out;
    finish_kernel<<<dim3(1), dim3(1024), 0, c->stream>>>(fa);
    HIPCHK(c, hipGetLastError());
    return GH_OK;
}

// scal[0..2] of a state set, summed from the partials of a one-launch epilogue if still pending
static int scal_ready(gh_ctx *c, const gh_ctx::StateSet &o)
{
    if (!o.pending) return GH_OK;
    // (joint store: |r|^2 partials of both blocks, then R partials of both blocks)
    const int nd = c->joint ? 2 * c->n_dpart : c->n_dpart;
    const int nr = c->joint ? 2 * (int)((store_cells(c) + 255) / 256) : c->n_regpart;
    if (cross_gradient_on(c))
        scal_cg_kernel<<<dim3(1), dim3(1024), 0, c->stream>>>(o.part, nd, nr, nr / 2, c->alpha, c->cg.lambda, o.scal, o.phi);
    else if (amplitude_on(c))
        scal_cg_kernel<<<dim3(1), dim3(1024), 0, c->stream>>>(o.part, nd, nr, nr / 3, c->alpha, c->amp.lambda, o.scal, o.phi);
    else
        scal_kernel<<<dim3(1), dim3(1024), 0, c->stream>>>(o.part, nd, nr, c->alpha, o.scal);
    HIPCHK(c, hipGetLastError());
    o.pending = false;
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

static int ensure_work(gh_ctx *c)
{
    // (joint store: observation-space vectors [gz: ld | tf: ld])
    const size_t M = (size_t)c->M, ld = (size_t)c->ld * (c->joint ? 2 : 1);
    TRY(dalloc(c, &c->scal_all, 16));
    for (int i = 0; i < 4; ++i) {
        TRY(dalloc(c, &c->st[i].r, ld));
        TRY(dalloc(c, &c->st[i].greg, M));
        TRY(dalloc(c, &c->st[i].d, ld));
        c->st[i].scal = c->scal_all + 4 * i;
        TRY(dalloc(c, &c->xb[i], M));
    }
    TRY(dalloc(c, &c->pb[0], M));
    TRY(dalloc(c, &c->pb[1], M));
    TRY(dalloc(c, &c->pn, M));
    if (c->n_panels > 1 || shard_rows(c)) TRY(dalloc(c, &c->gbuf, M));
    // (N > 16384: the team sweep writes one slab row per team, up to 128, whatever the panel grid)
    // (the harmonic forms of the shift-invariant store deliver ONE finished slab row)
    // (slab rows are c->ld long, also on the joint store: a workgroup's partial forward product covers its own block)
    TRY(dalloc(c, &c->slab, (size_t)(lonsym_one_row(c) ? 1 : c->n_panels > 1 ? std::max(c->grid, 128) : c->grid) * (size_t)c->ld));
    if (c->grid > 64) {
        // segments left for the single-block finish_kernel: as many as keep its read at ~128 KB
        // (C1: 16 x 608 rows; C2: 1 x 10^4 -- sixteen there made that one block read 1.3 MB, 57 us)
        c->slab2_rows = (int)std::max<int64_t>(1, std::min<int64_t>(16, 16384 / (int64_t)c->ld));
        TRY(dalloc(c, &c->slab2, (size_t)c->slab2_rows * ld));
    }
    c->n_dpart = (int)((c->ld + 31) / 32);
    if (c->joint) {
        // (the joint epilogue always leaves its partials: |r|^2 of both blocks, R of both blocks, then -- coupling
        // on -- Phi of the cross-gradient term, one per 256 cells of a property)
        TRY(dalloc(c, &c->cg.phi_all, 4));
        for (int i = 0; i < 4; ++i) {
            TRY(dalloc(c, &c->st[i].part, 2 * (size_t)c->n_dpart + 3 * (size_t)((store_cells(c) + 255) / 256)));
            c->st[i].phi = c->cg.phi_all + i;
        }
    } else if (c->mc.n > 0) {
        // (the multi-component store's epilogue always runs as reduce_finish_kernel<BLOCKS>: its partials, the
        // slab rows' sums per row block and the blocks' means)
        // (on the shift-invariant table: the classes' sums, which are the blocks' partials there)
        TRY(dalloc(c, &c->mc.bsum, std::max((size_t)c->mc.n * (size_t)std::max(c->grid, 128),
                                            lonsym_on(c) ? (size_t)lonsym_classes(c) : (size_t)0)));
        TRY(dalloc(c, &c->mc.bmean, (size_t)c->mc.n));
        // (vector-data magnetization store: R's blocks are counted per property -- up to two more than ceil(M / 256) --
        // and the amplitude term's partials follow them, one per 256 cells)
        for (int i = 0; i < 4; ++i)
            TRY(dalloc(c, &c->st[i].part, (size_t)c->n_dpart + (size_t)((c->M + 255) / 256) +
                                              (c->mvi ? 3 + (size_t)((store_cells(c) + 255) / 256) : 0)));
    } else if (c->ld >= 2048 && ((c->TW > 1 && c->n_panels == 1 && !c->mf) || lonsym_on(c)) && env_int("GRAVHMC_EPILOGUE1", 1) != 0) {
        TRY(dalloc(c, &c->dsum, (size_t)std::max(std::max(c->grid, 128), lonsym_on(c) ? lonsym_classes(c) : 0)));
        // (magnetization-vector store: up to three more partials of R, its blocks being counted per property, and
        // behind them those of the amplitude term, one per 256 cells)
        for (int i = 0; i < 4; ++i)
            TRY(dalloc(c, &c->st[i].part, (size_t)c->n_dpart + (size_t)((c->M + 255) / 256) +
                                              (c->mvi ? 3 + (size_t)((store_cells(c) + 255) / 256) : 0)));
    }
    if (c->mvi) {
        // Phi of the amplitude term per state set, and its partials where the epilogue keeps none (finish_kernel)
        TRY(dalloc(c, &c->cg.phi_all, 4));
        for (int i = 0; i < 4; ++i) c->st[i].phi = c->cg.phi_all + i;
        TRY(dalloc(c, &c->amppart, (size_t)((store_cells(c) + 255) / 256)));
    }
    // (joint and magnetization-vector stores: the regulariser runs per property, ceil(m / 256) blocks each)
    c->n_regpart = reg_props(c) * (int)((c->M / reg_props(c) + 255) / 256);
    c->n_pp0 = (int)std::min<int64_t>(1024, (c->M + 255) / 256);
    TRY(dalloc(c, &c->dpart, (size_t)c->n_dpart));
    TRY(dalloc(c, &c->regpart, (size_t)c->n_regpart));
    TRY(dalloc(c, &c->pp_part, (size_t)c->n_teams));
    TRY(dalloc(c, &c->ppn_part, (size_t)c->n_teams));
    TRY(dalloc(c, &c->pp0_part, (size_t)c->n_pp0));
    TRY(dalloc(c, &c->pn0_part, (size_t)c->n_pp0));
    TRY(dalloc(c, &c->tmpM, M));
    TRY(dalloc(c, &c->tmpN, ld));
    TRY(dalloc(c, &c->low, M));
    TRY(dalloc(c, &c->high, M));
    if (!c->mwapr) {
        TRY(dalloc(c, &c->mwapr, M));
    }
    if (!c->wm2) {
        TRY(dalloc(c, &c->wm2, M));
    }
    if (!c->h_scal) {
        c->h_scal_n = 16 + 2 * (size_t)c->n_teams + 2 * (size_t)c->n_pp0;
        HIPCHK(c, hipHostMalloc((void **)&c->h_scal, c->h_scal_n * sizeof(double)));
    }
    return GH_OK;
}

static int need(gh_ctx *c, bool cond, const char *what)
{
    if (!cond) return fail(c, GH_ERR_ARG, "%s", what);
    return GH_OK;
}
