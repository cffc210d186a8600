// libgravhmc host side: planning and launching the persistent harmonic pass of the shift-invariant store
// (lonres.hip.h), and the batch of chains on that store.  Included once by gravhmc.hip.
#pragma once

typedef void (*lonres_fn_t)(LonResArgs);
static lonres_fn_t lonres_fn(int rw)
{
    return rw <= 1 ? lonsymh_resident_kernel<1> : rw == 2 ? lonsymh_resident_kernel<2> : rw == 3 ? lonsymh_resident_kernel<3>
                                                                                               : lonsymh_resident_kernel<4>;
}

// Can the chain of this context run inside lonsymh_resident_kernel?  The harmonic store on one device, every
// workgroup of the pass resident (one per CU: its rows of the table live in its registers) and all cell rows in
// ONE group of rows per workgroup, a class owner for every class.
static bool lonres_plan(gh_ctx *c)
{
    if (!lonsym_harmonic(c)) return false;
    LonSymHost &h = *c->ls;
    LonSymHost::Res &r = h.res;
    if (r.state != 0) return r.state > 0;
    r.state = -1;
    if (env_int("GRAVHMC_LONSYM_RESIDENT", 1) == 0) return false;
    if (c->sh.kind != 0 || c->wv.on) return false;
    if (h.hgrid > LR_MAXWG || h.hgrid < h.na || (int64_t)h.hgrid * h.rw < h.nc || h.na > 64 || h.n > 126 || h.n < 2 || h.max_extra > 2) return false;
    int lds_max = 0;
    if (hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device) != hipSuccess) return false;
    r.lds = lonres_lds_doubles(h.n, h.nf, h.na, h.rw) * sizeof(double);
    if (r.lds > (size_t)lds_max) return false;
    lonres_fn_t f = lonres_fn(h.rw);
    if (allow_dynamic_lds(reinterpret_cast<const void *>(f), r.lds) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(f), LR_THREADS, r.lds) != hipSuccess ||
        per_cu < 1 || (int64_t)per_cu * c->cus < h.hgrid) {
        (void)hipGetLastError();
        return false;
    }
    r.state = 1;
    return true;
}

// lonres_plan + what depends on the regulariser set at the moment (the stencil kinds need the model's shape)
static bool lonres_usable(gh_ctx *c)
{
    if (!lonres_plan(c)) return false;
    return c->reg_kind >= 0 && c->reg_kind <= 3 && (c->reg_kind == 0 || c->reg_kind == 2 || c->shape[0] > 0);
}

// K trajectories of the context's chain in one launch (same contract as gh_chain_run / chain_run_resident).
// GH_RESIDENT_ABORTED: the kernel gave up waiting for its workgroups, nothing was changed.
// st: the context whose chain runs (c itself, or one of the light contexts of a batch of chains: the launch, its
// tables and exchange buffers are c's).  p0rows (or nullptr): the K momentum rows where they lie, instead of p0s.
static int chain_run_lonres(gh_ctx *c, gh_ctx *st, int K, const int *L, const double *p0s, const double *const *p0rows, const double *us,
                            double dt, int64_t stop_at_accepts, int64_t record_from, int *accepted, double *out5s, double *x_out,
                            int *n_run)
{
    LonSymHost &h = *c->ls;
    LonSymHost::Res &r = h.res;
    const size_t M = (size_t)c->M;
    const int nwg = h.hgrid;
    const size_t E = (size_t)h.na * (size_t)h.nf;
    HIPCHK(c, hipSetDevice(c->device));
    if (!r.slab) {
        TRY(dalloc(c, &r.slab, ((size_t)nwg + 8) * E));
        TRY(dalloc(c, &r.flagg, (size_t)nwg + 8));
        TRY(dalloc(c, &r.xccg, (size_t)nwg + 8));
        TRY(dalloc(c, &r.xslabg, 2 * (size_t)RES_CLUSTERS * E * 2));
        TRY(dalloc(c, &r.rhatg, 2 * E));
        TRY(dalloc(c, &r.clsg, 2 * 64 * 4));
        TRY(dalloc(c, &r.scalg, 2 * (size_t)LR_MAXWG * 2));
        TRY(dalloc(c, &r.ppg, 2 * (size_t)LR_MAXWG * 2));
        TRY(dalloc(c, &r.xpub, 2 * (size_t)c->M));
        TRY(xg_alloc(c, r.xg, {{r.flagg, ((size_t)nwg + 8) * sizeof(ghk::u64)},
                               {r.xccg, ((size_t)nwg + 8) * sizeof(ghk::u64)},
                               {r.xslabg, 2 * (size_t)RES_CLUSTERS * E * 2 * sizeof(ghk::u32x4)},
                               {r.clsg, 2 * 64 * 4 * sizeof(ghk::u32x4)},
                               {r.scalg, 2 * (size_t)LR_MAXWG * 2 * sizeof(ghk::u32x4)},
                               {r.ppg, 2 * (size_t)LR_MAXWG * 2 * sizeof(ghk::u32x4)}}));
        TRY(dalloc(c, &r.n_run, 4));
        TRY(dalloc(c, &r.ucur, 4));
        // M^ = the transform of the slots' observation counts: R^ of a residual of ones
        TRY(dalloc(c, &r.mhat, E));
        {
            double *ones = nullptr;
            TRY(dalloc(c, &ones, (size_t)c->ld));
            const std::vector<double> hv((size_t)c->N, 1.0);
            HIPCHK(c, hipMemcpyAsync(ones, hv.data(), hv.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
            lonsymh_rhat_kernel<<<dim3((unsigned)h.na), dim3(256), 0, c->stream>>>(lonsymh_geom(c), ones);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(r.mhat, h.Rhat, E * sizeof(ghk::d2), hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            h.rhat_of = nullptr;
        }
        if (env_int("GRAVHMC_LONSYM_TIMING", 0)) TRY(dalloc(c, &r.dbg, 16));
        HIPCHK(c, hipEventCreate(&r.ev0));
        HIPCHK(c, hipEventCreate(&r.ev1));
    }
    const bool want_x = x_out != nullptr || st->ring != nullptr || c->ps.on;
    TrajLists &tl = r.lists;
    TRY(traj_lists_reserve(c, tl, K));
    int64_t steps = 1;
    for (int k = 0; k < K; ++k) steps += L[k];
    TRY(xg_prepare(c, r.xg, true, (uint64_t)steps + 2, (uint64_t)K + 2));
    TRY(traj_upload(c, tl, K, p0rows ? nullptr : p0s, p0rows, us, L));
    LonResArgs a{};
    a.g = lonsymh_geom(c);
    a.g.dbg = nullptr;
    a.N = c->N;
    a.M = c->M;
    a.nwg = nwg;
    if (env_int("GRAVHMC_LONRES_TEST_ABORT", 0)) a.nwg += 8;  // test hook: partners that do not exist
    a.try_local = env_int("GRAVHMC_RESIDENT_LOCAL", 1);
    a.wm = st->weighted ? st->wm : nullptr;
    a.low = st->low;
    a.high = st->high;
    a.mwapr = st->mwapr;
    a.wm2 = st->wm2;
    a.kind = st->reg_kind;
    a.nz = st->shape[0];
    a.ny = st->shape[1];
    a.nx = st->shape[2];
    a.xpub = r.xpub;
    a.ms_grad_den_mw = 0;
    a.alpha = st->alpha;
    a.beta = st->beta;
    a.dobs_c = st->dobs_c;
    a.gfix = st->have_fix ? st->gfix : nullptr;
    a.gfix_sum = st->have_fix ? st->gfix_sum : 0.0;
    a.Mhat = r.mhat;
    a.x_cur = st->xb[st->xcur];
    a.K = K;
    a.L = tl.L;
    a.p0s = tl.p0s;
    a.us = tl.us;
    a.dt = dt;
    a.stop_at_accepts = stop_at_accepts;
    a.accept_count0 = st->accept_count;
    a.accepted = tl.accepted;
    a.out5s = tl.out5s;
    a.xacc = want_x ? tl.xacc : nullptr;
    a.n_run = r.n_run;
    a.ucur = r.ucur;
    a.slab = r.slab;
    a.flagg = r.flagg;
    a.xslabg = r.xslabg;
    a.rhatg = r.rhatg;
    a.clsg = r.clsg;
    a.scalg = r.scalg;
    a.ppg = r.ppg;
    a.xccg = r.xccg;
    a.tag0 = r.xg.tag;
    a.tagE0 = r.xg.tagE;
    a.ltag = r.xg.ltag + 1u;
    a.abort_w = r.xg.abort_w;
    a.dbg = r.dbg;
    lonres_fn_t f = lonres_fn(h.rw);
    HIPCHK(c, allow_dynamic_lds(reinterpret_cast<const void *>(f), r.lds));
    TRY(prof_launch_mark(c, r.ev0));
    // (a plain launch: the grid was checked against the occupancy query in lonres_plan; every wait inside is bounded)
    hipLaunchKernelGGL(f, dim3((unsigned)nwg), dim3(LR_THREADS), r.lds, c->stream, a);
    HIPCHK(c, hipGetLastError());
    TRY(prof_launch_mark(c, r.ev1));
    int h_run[4] = {0, 0, 0, 0};
    double h_u[4] = {0, 0, 0, 0};
    TRY(xg_read(c, r.xg));
    HIPCHK(c, hipMemcpyAsync(h_run, r.n_run, sizeof h_run, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_u, r.ucur, 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(accepted, tl.accepted, (size_t)K * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(out5s, tl.out5s, (size_t)K * 5 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    r.xg.ltag += 1u;
    if (r.xg.seen[0] != 0u) {
        const bool for_good = xg_give_up(r.xg, 3);
        if (for_good) r.state = -1;
        fprintf(stderr, "libgravhmc: the persistent harmonic pass timed out waiting for its workgroups (%d of 3); %s with one "
                        "launch per phase\n", r.xg.aborts, for_good ? "continuing for good" : "running this batch");
        return GH_RESIDENT_ABORTED;
    }
    r.xg.tag += (unsigned)h_run[1];
    r.xg.tagE += (unsigned)h_run[2];
    r.launches += 1;
    r.evals += h_run[1];
    r.trajectories += h_run[0];
    TRY(prof_launch_end(c, r.ev0, r.ev1, h_run[1]));
    *n_run = h_run[0];
    for (int k = 0; k < h_run[0]; ++k)
        if (accepted[k]) TRY(chain_accept_row(c, st, tl.xacc + (size_t)k * M, record_from, x_out ? x_out + (size_t)k * M : nullptr));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // (d, r and the scalars of the current sample are behind x now: chain_state_fresh brings them up to date for
    // whoever reads them next)
    st->U_cur[0] = h_u[0];
    st->U_cur[1] = h_u[1];
    st->U_cur[2] = h_u[2];
    st->spec_valid = st->pn_valid = false;
    st->st_stale = true;
    return GH_OK;
}

static int chain_trajectory_impl(gh_ctx *, const double *, double, int, double, const double *, int *, double[5]);  // host_chain.h

// ---- a batch of chains on the shift-invariant store (BASELINE configs[3]: "8 chains"; the reference runs them
// as MPI ranks, example/global/run_main.sh:16, each with its own 4.25 GB kernel).  A step of ONE chain on the
// table keeps a fraction of the chip busy for ~60 us, most of it latency: the chains are C light contexts
// that share the parent's tables (T, T^: read-only) and problem vectors, each with its own stream, chain
// state and work buffers, driven by one host thread each -- their passes overlap on the GPU.
static int kids_make(gh_ctx *c, int C, const double *x0s, const double *low, const double *high)
{
    for (gh_ctx *k : c->kids) gh_destroy(k);
    c->kids.clear();
    for (int i = 0; i < C; ++i) {
        gh_ctx *k = nullptr;
        const int rc0 = gh_create(&k, c->device, c->N, c->M);
        if (rc0 != GH_OK) return fail(c, rc0, "gh_batch_init: %s", gh_last_error(nullptr));
        c->kids.push_back(k);
        k->cell_kind = c->cell_kind;
        k->ratio = c->ratio;
        for (int q = 0; q < 3; ++q) k->tf_dir[q] = c->tf_dir[q];
        k->tf_dir_d = c->tf_dir_d;
        k->comp = c->comp;  // (GH_CELL_TESSEROID_COMP never gets here: the shift-invariant store refuses it)
        k->have_obs = k->have_cells = k->have_G = true;
        k->mf = true;
        k->weighted = c->weighted;
        k->wm = c->wm;
        k->wm2 = c->wm2;
        k->dobs_c = c->dobs_c;
        k->gfix = c->gfix;
        k->gfix_sum = c->gfix_sum;
        k->mwapr = c->mwapr;
        k->have_data = c->have_data;
        k->have_fix = c->have_fix;
        k->have_reg = c->have_reg;
        k->reg_kind = c->reg_kind;
        for (int q = 0; q < 3; ++q) k->shape[q] = c->shape[q];
        k->alpha = c->alpha;
        k->beta = c->beta;
        k->ls = new LonSymHost(*c->ls);  // (the tables are the parent's; the pass's work buffers are its own)
        k->ls->Rhat = k->ls->Dpart = nullptr;
        k->ls->res = LonSymHost::Res();
        k->ls->res.state = -1;  // (the persistent pass takes every CU: not for chains that share the GPU)
        k->ls->dbg = nullptr;
        k->ls->csum = nullptr;
        k->ls->epi = ExchangeGuard();
        k->ls->rhat_of = nullptr;
        k->ls->post_pending = false;
        if (k->ls->harm) {
            int rc = dalloc(k, &k->ls->Rhat, (size_t)k->ls->na * (size_t)k->ls->nf);
            if (rc == GH_OK) rc = dalloc(k, &k->ls->Dpart, (size_t)k->ls->hgrid * (size_t)k->ls->na * (size_t)k->ls->nf);
            if (rc == GH_OK && k->ls->fused) rc = dalloc(k, &k->ls->csum, 2 * (size_t)k->ls->na);
            if (rc == GH_OK && k->ls->fused)
                rc = xg_alloc(k, k->ls->epi, {{k->ls->csum, sizeof(unsigned long long) * 2 * (size_t)k->ls->na}});
            if (rc != GH_OK) return fail(c, rc, "gh_batch_init: %s", gh_last_error(k));
        }
        if (k->ls->wide) {
            k->ls->Xhat = nullptr;
            int rc = dalloc(k, &k->ls->Rhat, (size_t)k->ls->na * (size_t)k->ls->nfp);
            if (rc == GH_OK) rc = dalloc(k, &k->ls->Xhat, (size_t)k->ls->nc * (size_t)k->ls->nf);
            if (rc == GH_OK) rc = dalloc(k, &k->ls->Dpart, (size_t)k->ls->wparts * (k->ls->wmirror ? 2 : 1) * (size_t)k->ls->na * (size_t)k->ls->nfp);
            if (rc != GH_OK) return fail(c, rc, "gh_batch_init: %s", gh_last_error(k));
        }
        int rc = configure_mf(k);
        if (rc == GH_OK) rc = dalloc(k, &k->mf_stats, 1);
        if (rc == GH_OK) rc = gh_chain_init(k, x0s + (size_t)i * (size_t)c->M, low, high);
        if (rc != GH_OK) return fail(c, rc, "gh_batch_init (chain %d): %s", i, gh_last_error(k));
    }
    c->bt.C = C;
    c->bt.ready = true;
    c->bt.run = gh_ctx::Batch::Run();
    return GH_OK;
}

// T trajectories of every chain (lists chain-major), each chain on its own thread and stream; results of
// chain i in slots i * Tout + t.  Nothing stays in flight.
static int kids_run(gh_ctx *c, int T, const int *L, const double *const *p0rows, const double *p0flat, const double *us,
                    double dt, int *accepted, double *out5s, double *x_out, int Tout)
{
    const int C = (int)c->kids.size();
    const size_t M = (size_t)c->M;
    std::vector<int> rcs((size_t)C, GH_OK);
    std::mutex post_mu;  // (the pooled histogram is shared: the chains' accumulate launches take turns)
    // On the harmonic store the chains TAKE TURNS in the persistent launch (lonres.hip.h) -- a
    // chain's whole list in one launch with the table in the workgroups' registers: one chain alone runs faster that way
    // (35 k steps/s at C4) than eight side by side on the launches per phase (29-32 k together).  A launch that gives up
    // leaves its chain untouched: that chain and the ones behind it run on their own streams as below.
    int first_threaded = 0;
    if (T > 0 && lonres_usable(c)) {
        for (int i = 0; i < C; ++i) {
            gh_ctx *k = c->kids[(size_t)i];
            int n_run = 0;
            const size_t o = (size_t)i * (size_t)Tout;
            const int rc = chain_run_lonres(c, k, T, L + (size_t)i * T, p0flat ? p0flat + (size_t)i * T * M : nullptr,
                                            p0rows ? p0rows + (size_t)i * T : nullptr, us + (size_t)i * T, dt, 0, 0, accepted + o,
                                            out5s + o * 5, x_out ? x_out + o * M : nullptr, &n_run);
            if (rc == GH_RESIDENT_ABORTED) break;
            if (rc != GH_OK) return rc;
            first_threaded = i + 1;
        }
        if (first_threaded == C) return GH_OK;
    }
    auto work = [&](int i) {
        gh_ctx *k = c->kids[(size_t)i];
        if (hipSetDevice(k->device) != hipSuccess) {
            rcs[(size_t)i] = GH_ERR_HIP;
            return;
        }
        for (int t = 0; t < T; ++t) {
            const size_t src = (size_t)i * T + t, dst = (size_t)i * Tout + t;
            const double *p0 = p0flat ? p0flat + src * M : p0rows[src];
            const double *pn = (t + 1 < T) ? (p0flat ? p0flat + (src + 1) * M : p0rows[src + 1]) : nullptr;
            int acc = 0;
            double o5[5];
            int rc = chain_trajectory_impl(k, p0, dt, L[src], us[src], pn, &acc, o5);
            if (rc == GH_OK && acc) {
                std::lock_guard<std::mutex> lock(post_mu);
                const int64_t fed = c->ps.launches;
                rc = post_feed_batch_row(c, i, k->xb[k->xcur], k->stream);
                if (rc == GH_OK && c->ps.launches != fed && hipStreamSynchronize(k->stream) != hipSuccess) rc = GH_ERR_HIP;
            }
            if (rc == GH_OK && x_out && acc) rc = gh_chain_get_x(k, x_out + dst * M);
            if (rc != GH_OK) {
                rcs[(size_t)i] = rc;
                return;
            }
            accepted[dst] = acc;
            memcpy(out5s + dst * 5, o5, 5 * sizeof(double));
        }
    };
    std::vector<std::thread> pool;
    for (int i = first_threaded + 1; i < C; ++i) pool.emplace_back(work, i);
    work(first_threaded);
    for (std::thread &th : pool) th.join();
    for (int i = 0; i < C; ++i)
        if (rcs[(size_t)i] != GH_OK) return fail(c, rcs[(size_t)i], "chain %d: %s", i, gh_last_error(c->kids[(size_t)i]));
    return GH_OK;
}
