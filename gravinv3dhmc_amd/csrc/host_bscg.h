// libgravhmc host side: bootstrap replicates of the conjugate-gradient inversion in lock-step (bscg.hip.h).
// Included once by gravhmc.hip.
#pragma once

static const char *const BSCG_WHO = "the bootstrap batch (gh_bscg_run)";

// Which contexts the bootstrap batch runs on: one GPU's dense, weighted store of one field, or the translation-invariant
// table asked for with gh_set_translation_invariant(4) (lattice_reps: the table's batch passes, latbatch.hip.h).
static int bscg_refuse(gh_ctx *c, int B, int maxk)
{
    const bool table = lattice_reps(c);
    // (a store of blocks names itself: each is dense and unsharded, but for the tesseroid forms on the table)
    // (the table of blocks that takes chain batches names the table, as the single-block table of chains does)
    const char *what = c->ls && tess_mag_store(c) ? "the tesseroid magnetization store on the shift-invariant table"
                                                  : store_of(c).rows_name;
    if (lattice_mvi(c) || lattice_multi_chains(c))
        what = lattice_form(c).name;
    else if (what)
        ;
    else if (c->ls)
        what = "a shift-invariant store";
    else if (c->lat && !table)
        what = LATTICE_NAME;
    else if (c->mf && !table)
        what = "a matrix-free context";
    else if (c->sh.kind != 0)
        what = "a sharded context";
    else if (c->fd.valid && c->fd.gen == c->G_gen)
        what = "a context whose sweeps read the folded store";
    else if (c->wv.on)
        what = "a context with the wavelet-compressed forward (another operator)";
    if (what) return fail(c, GH_ERR_UNSUPPORTED, "%s runs on the dense stored kernel of one GPU, not on %s", BSCG_WHO, what);
    if (table && !lattice_on(c)) return fail(c, GH_ERR_UNSUPPORTED, "%s needs the table of %s (gh_build_G)", BSCG_WHO, LATTICE_NAME);
    if (!table && !c->G) return fail(c, GH_ERR_UNSUPPORTED, "%s needs the dense stored kernel (gh_build_G / gh_upload_G)", BSCG_WHO);
    if (!c->weighted)
        return fail(c, GH_ERR_UNSUPPORTED, "%s needs the weighted kernel: call gh_weight first (an unweighted store has no Wm)",
                    BSCG_WHO);
    if (B < 1 || B > CB) return fail(c, GH_ERR_UNSUPPORTED, "%s takes 1..16 replicates per group, got %d", BSCG_WHO, B);
    if (maxk < 2) return fail(c, GH_ERR_UNSUPPORTED, "%s needs maxk >= 2, got %d", BSCG_WHO, maxk);
    if (table) TRY(latb_plan(c, "gh_bscg_run"));  // (an extent the batch tile cannot hold: refused before anything is made)
    return GH_OK;
}

// D = Aw.X of all slots: batch_forward_kernel and batch_reduce_kernel as the chain batch launches them; on the table
// the batch forward over it (latb_pass_kernel<LATB_FWD>) and the reduction of its slab rows, one per chunk of layers
static int bscg_forward(gh_ctx *c, const double *X, double *D)
{
    gh_ctx::Batch &b = c->bt;
    if (lattice_on(c)) {
        latb_launch_forward(c, X);
        const int64_t n16 = c->ld * CB;
        batch_reduce_kernel<<<blocks256(n16), dim3(256), 0, c->stream>>>(b.slab, b.slab_live, n16, D);
        HIPCHK(c, hipGetLastError());
        c->bs.forward_sweeps += 1;
        return GH_OK;
    }
    BatchFwdArgs f;
    f.G = c->G;
    f.ld = c->ld;
    f.M = c->M;
    f.N = c->N;
    f.X = X;
    f.cols_per_block = b.cols_per_block;
    f.slab = b.slab;
    batch_forward_kernel<<<dim3((unsigned)((c->ld + 511) / 512), (unsigned)b.n_colblocks), dim3(256), 0, c->stream>>>(f);
    const int64_t n16 = c->ld * CB;
    batch_reduce_kernel<<<blocks256(n16), dim3(256), 0, c->stream>>>(b.slab, b.n_colblocks, n16, D);
    HIPCHK(c, hipGetLastError());
    c->bs.forward_sweeps += 1;
    return GH_OK;
}

// One group of B replicates: maxk lock-steps enqueued on the context's stream, one synchronisation at the end.
// The vectors live in the chain batch's buffers (batch_alloc) where the shapes coincide: X = Xc, I = GREGc,
// Iw = Pw[0], D = Dc, F = Dw, Rt = Rtc, the counts in Rtw, the |I|^2 partials in pp_part, the models on their way
// out in stage; a chain batch of the context has to be initialised again afterwards.
static int bscg_run(gh_ctx *c, int B, const double *counts, const double *dobs, const double *mw0, double rhomin,
                    double rhomax, double beta2, double q, int maxk, double *models, double *dmis, double *mmis,
                    double *alpha, int *n_entries, int *n_alpha)
{
    gh_ctx::Batch &b = c->bt;
    gh_ctx::Bscg &s = c->bs;
    const int64_t M = c->M, N = c->N, ld = c->ld;
    TRY(ensure_work(c, "gh_bscg_run"));
    TRY(batch_alloc(c));
    // (the adjoint's operand-ordered copy of G where HBM has room -- a second ld x M doubles that stay until
    // gh_destroy, also on a context whose chain batch runs on teams and would not make it; the same bits without)
    // (the table has no G to copy; its passes divide by wm through b.iw, which gh_batch_init fills for the chains)
    const bool table = lattice_on(c);
    if (!table) TRY(batch_relayout(c));
    b.ready = false;         // the chain batch's state is overwritten
    b.run = gh_ctx::Batch::Run();
    c->rs.b_on = false;
    double *X = b.Xc, *I = b.GREGc, *Iw = b.Pw[0], *D = b.Dc, *F = b.Dw, *Rt = b.Rtc, *Cn = b.Rtw;
    s.nblk = (int)std::min<int64_t>(1024, (M + 15) / 16);
    TRY(dalloc(c, &s.st, CB));
    TRY(dalloc(c, &s.crow, (size_t)CB * (size_t)N));
    TRY(dalloc(c, &s.dobs, (size_t)ld));
    TRY(dalloc(c, &s.mw0, (size_t)M));
    TRY(dalloc(c, &s.iw, (size_t)M));
    TRY(dalloc(c, &s.dirpart, 2 * (size_t)s.nblk * CB));
    TRY(dalloc(c, &s.mspart, (size_t)s.nblk * CB));
    if (maxk > s.res_maxk) {
        s.res = nullptr;  // (the old block stays in the allocation list until gh_destroy)
        TRY(dalloc(c, &s.res, 3 * (size_t)CB * (size_t)maxk));
        s.res_maxk = maxk;
    }
    double *d_dmis = s.res, *d_mmis = s.res + (size_t)CB * (maxk - 1), *d_alpha = s.res + 2 * (size_t)CB * (maxk - 1);
    s.forward_sweeps = s.adjoint_sweeps = s.lock_steps = 0;

    // inputs (the caller's arrays are used until this function returns, after the one synchronisation below)
    HIPCHK(c, hipMemcpyAsync(s.crow, counts, sizeof(double) * (size_t)B * (size_t)N, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(s.dobs, dobs, sizeof(double) * (size_t)N, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(s.mw0, mw0, sizeof(double) * (size_t)M, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(Cn, 0, sizeof(double) * (size_t)ld * CB, c->stream));
    HIPCHK(c, hipMemsetAsync(s.res, 0, sizeof(double) * 3 * (size_t)CB * (size_t)maxk, c->stream));
    batch_interleave_kernel<<<blocks256(N * CB), dim3(256), 0, c->stream>>>(s.crow, B, N, Cn);
    bscg_init_kernel<<<blocks256(M * CB), dim3(256), 0, c->stream>>>(s.mw0, c->wm, B, M, X, I, Iw, s.iw, s.st);
    if (table) mfb_invw_kernel<<<blocks256(M), dim3(256), 0, c->stream>>>(c->wm, M, b.iw);
    HIPCHK(c, hipGetLastError());

    BscgResArgs ra;
    ra.N = N;
    ra.ld = ld;
    ra.M = M;
    ra.D = D;
    ra.counts = Cn;
    ra.dobs = s.dobs;
    ra.mspart = s.mspart;
    ra.maxk = maxk;
    ra.q = q;
    ra.Rt = Rt;
    ra.st = s.st;
    ra.dmis = d_dmis;
    ra.mmis = d_mmis;
    ra.alpha = d_alpha;
    BscgAdjArgs aa;
    aa.Gb = b.Gb;
    aa.G = c->G;
    aa.ld = ld;
    aa.M = M;
    aa.np = (int)(ld / 16);
    aa.Rt = Rt;
    aa.X = X;
    aa.wm2 = c->wm2;
    aa.beta2 = beta2;
    aa.st = s.st;
    aa.I = I;
    aa.nI2_part = b.pp_part;
    aa.n_waves = b.n_waves;
    LatbCgArgs la;
    la.X = X;
    la.wm2 = c->wm2;
    la.beta2 = beta2;
    la.st = s.st;
    la.I = I;
    la.nI2_part = b.pp_part;

    // the initial evaluation: D = Aw.x0, data(x0), the residuals, alpha of iteration 0
    TRY(bscg_forward(c, X, D));
    ra.k = -1;
    ra.n_mspart = 0;
    bscg_residual_kernel<<<dim3(CB), dim3(1024), 0, c->stream>>>(ra);
    for (int k = 0; k < maxk; ++k) {
        // (b.n_waves: on the table the adjoint's workgroups, bgx_adj nz, one row of partials each)
        if (table)
            latb_launch_cg_adjoint(c, Rt, la);
        else
            bscg_adjoint_kernel<<<dim3((unsigned)(b.n_waves / 4)), dim3(256), 0, c->stream>>>(aa);
        s.adjoint_sweeps += 1;
        bscg_mu_kernel<<<dim3(CB), dim3(1024), 0, c->stream>>>(b.pp_part, b.n_waves, k, s.st);
        bscg_direction_kernel<<<dim3((unsigned)s.nblk), dim3(256), 0, c->stream>>>(I, Iw, M, k, s.st, s.dirpart);
        TRY(bscg_forward(c, Iw, F));
        bscg_kstep_kernel<<<dim3(CB), dim3(1024), 0, c->stream>>>(F, Cn, N, s.dirpart, s.nblk, s.st);
        bscg_step_kernel<<<dim3((unsigned)s.nblk), dim3(256), 0, c->stream>>>(X, Iw, c->wm, s.iw, c->wm2, M, rhomin, rhomax,
                                                                            beta2, s.st, s.mspart);
        TRY(bscg_forward(c, X, D));
        ra.k = k;
        ra.n_mspart = s.nblk;
        bscg_residual_kernel<<<dim3(CB), dim3(1024), 0, c->stream>>>(ra);
        HIPCHK(c, hipGetLastError());
        s.lock_steps += 1;
    }
    bscg_models_kernel<<<blocks256(M * CB), dim3(256), 0, c->stream>>>(X, s.iw, B, M, b.stage);
    HIPCHK(c, hipGetLastError());

    // results: one read per group
    std::vector<double> res(3 * (size_t)CB * (size_t)maxk);
    BscgState st[CB];
    HIPCHK(c, hipMemcpyAsync(models, b.stage, sizeof(double) * (size_t)B * (size_t)M, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(res.data(), s.res, sizeof(double) * res.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(st, s.st, sizeof st, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t e = (size_t)maxk - 1;
    memcpy(dmis, res.data(), sizeof(double) * (size_t)B * e);
    memcpy(mmis, res.data() + (size_t)CB * e, sizeof(double) * (size_t)B * e);
    memcpy(alpha, res.data() + 2 * (size_t)CB * e, sizeof(double) * (size_t)B * (size_t)maxk);
    for (int r = 0; r < B; ++r) {
        n_entries[r] = st[r].n_entries;
        n_alpha[r] = st[r].n_alpha;
    }
    return GH_OK;
}
