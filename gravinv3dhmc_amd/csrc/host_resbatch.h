// libgravhmc host side: the chains of a batch in LOCK-STEP inside the resident batch kernel (resbatch.hip.h).
// Included once by gravhmc.hip.
#pragma once

typedef void (*resbatch_fn_t)(ResBatchArgs);

template <int KS>
static resbatch_fn_t resbatch_for_ks(int nt, bool greg)
{
    if (greg) return nt <= 1 ? resident_batch_kernel<KS, 1, true> : resident_batch_kernel<KS, 2, true>;
    return nt <= 1 ? resident_batch_kernel<KS, 1, false> : resident_batch_kernel<KS, 2, false>;
}

// ks: k-steps (4 rows) per wave of the adjoint, 32 ks >= ld; compiled for ld <= 640.  greg: the adjoint's
// operand in registers (compressed forward: LDS holds another matrix)
static resbatch_fn_t resbatch_for(int ks, int nt, bool greg)
{
    switch (ks) {
    case 5: return resbatch_for_ks<5>(nt, greg);
    case 10: return resbatch_for_ks<10>(nt, greg);
    case 15: return resbatch_for_ks<15>(nt, greg);
    case 20: return resbatch_for_ks<20>(nt, greg);
    }
    return nullptr;
}

// Can the batch of C chains run in lock-step?  The problem must fit the resident chain kernel with every
// column of a workgroup in LDS (no split / stream mode), at most 32 columns per workgroup and 640 rows.
// The decision alone (nothing allocated, nothing of the context's lock-step state touched): instantiation and LDS
// request for C chains.
static bool resbatch_shape(gh_ctx *c, int C, int *ks, int *nt, size_t *lds)
{
    gh_ctx::Resident &r = c->rs;
    *ks = *nt = 0;
    *lds = 0;
    if (env_int("GRAVHMC_RESIDENT_BATCH", 1) == 0 || C < 2 || C > 16) return false;
    if (!resident_usable(c) || r.split || r.stream || r.cpw > 32 || c->ld > 640 || c->ld % 16 != 0) return false;
    *ks = (int)((c->ld + 159) / 160) * 5;
    *nt = (r.cpw + 15) / 16;
    *lds = resbatch_lds_doubles(c->ld, r.cpw, c->have_fix, c->wv.on) * sizeof(double);
    if (*lds > (size_t)r.lds_max) return false;
    resbatch_fn_t f = resbatch_for(*ks, *nt, c->wv.on);
    if (!f) return false;
    int per_cu = 0;
    if (allow_dynamic_lds(reinterpret_cast<const void *>(f), *lds) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(f), RB_THREADS, *lds) != hipSuccess ||
        per_cu < 1 || (int64_t)per_cu * c->cus < r.nwg) {
        (void)hipGetLastError();
        return false;
    }
    return true;
}

static bool resbatch_plan(gh_ctx *c, int C)
{
    gh_ctx::Resident &r = c->rs;
    gh_ctx::Resident::LockStep &b = r.ls;
    b.on = false;
    int ks = 0, nt = 0;
    size_t lds_bytes = 0;
    if (!resbatch_shape(c, C, &ks, &nt, &lds_bytes)) return false;
    b.ks = ks;
    b.nt = nt;
    b.C = C;
    b.lds = lds_bytes;
    const size_t M = (size_t)c->M, ldx = (size_t)c->ld + RB_XROWS;
    if (dalloc(c, &b.slabd, (size_t)(r.nwg + 8) * ldx * 16) != GH_OK || dalloc(c, &b.flagg, (size_t)r.nwg + 8) != GH_OK ||
        dalloc(c, &b.xslabg, 2 * (size_t)RES_CLUSTERS * ldx * 16) != GH_OK ||
        dalloc(c, &b.dclg, (size_t)RES_CLUSTERS * ldx * 16) != GH_OK || dalloc(c, &b.xccg, (size_t)r.nwg + 8) != GH_OK ||
        dalloc(c, &b.xpub, 2 * 16 * M) != GH_OK || dalloc(c, &b.xs, 16 * M) != GH_OK || dalloc(c, &b.ps, 16 * M) != GH_OK ||
        dalloc(c, &b.pst, 16 * M) != GH_OK || dalloc(c, &b.cst, 16 * RB_CST) != GH_OK || dalloc(c, &b.n_io, 128) != GH_OK ||
        xg_alloc(c, b.xg, {{b.flagg, ((size_t)r.nwg + 8) * sizeof(ghk::u64)},
                           {b.xslabg, 2 * (size_t)RES_CLUSTERS * ldx * 16 * sizeof(ghk::u32x4)},
                           {b.dclg, (size_t)RES_CLUSTERS * ldx * 16 * sizeof(ghk::u32x4)},
                           {b.xccg, ((size_t)r.nwg + 8) * sizeof(ghk::u64)}}) != GH_OK)
        return false;
    if (env_int("GRAVHMC_RESIDENT_TIMING", 0) && dalloc(c, &b.dbg, 32) != GH_OK) return false;
    if (!r.ev0 && (hipEventCreate(&r.ev0) != hipSuccess || hipEventCreate(&r.ev1) != hipSuccess)) return false;
    // (a new batch: nothing in flight)
    if (hipMemsetAsync(b.cst, 0, 16 * RB_CST * sizeof(double), c->stream) != hipSuccess) return false;
    for (bool &f2 : b.active) f2 = false;
    b.on = true;
    return true;
}

// Potential and gradient at the chains' current samples, once per gh_batch_init: a launch of the resident
// chain kernel without trajectories (its start-up evaluates every chain and keeps the results on the device).
static int resbatch_state(gh_ctx *c)
{
    gh_ctx::Resident &r = c->rs;
    if (r.b_state) return GH_OK;
    ResLaunch q;
    q.C = r.ls.C;
    q.K = 0;
    q.x_dev = r.bx;
    q.gcur_dev = r.bg;
    q.ucur_dev = r.bu;
    q.have_state = 0;
    int h_run[4] = {0, 0, 0, 0};
    TRY(resident_launch(c, q, nullptr, nullptr, h_run));
    r.b_state = true;
    return GH_OK;
}

// One launch: up to T further trajectories of every chain (lists chain-major: element (ch, t) at ch * T + t).
// carry: end as soon as a chain has nothing left to start (trajectories in flight continue in the next
// call); otherwise every list is run to its end.  Results of chain ch in slots ch * Tout + i, Tout = T + 1
// with carry.  GH_RESIDENT_ABORTED: the kernel gave up waiting for its workgroups, nothing was changed.
static int resbatch_launch(gh_ctx *c, int T, const int *L, const double *const *p0rows, const double *p0flat,
                           const double *us, double dt, bool carry, int *accepted, double *out5s, double *x_out,
                           int *n_started, int *n_done)
{
    gh_ctx::Resident &r = c->rs;
    gh_ctx::Resident::LockStep &b = r.ls;
    const size_t M = (size_t)c->M;
    const int C = b.C, Tout = carry ? T + 1 : T;
    HIPCHK(c, hipSetDevice(c->device));
    const int K = C * T, Kout = C * std::max(Tout, 1);
    TrajLists &tl = b.lists;
    TRY(traj_lists_reserve(c, tl, std::max(K, Kout)));
    int64_t steps = 0;
    for (int k = 0; k < K; ++k) steps += L[k] + 1;
    steps += 64 * 17;  // (what is in flight; generous)
    TRY(xg_prepare(c, b.xg, true, (uint64_t)steps + 2));
    // device rows chain-major (ch * T + t), like the lists
    TRY(traj_upload(c, tl, K, p0flat, p0rows, us, L));
    ResBatchArgs a{};
    a.G = c->G;
    a.Gl = c->wv.on ? c->wv.F : c->G;
    a.ld = c->ld;
    a.N = c->N;
    a.M = c->M;
    a.cols_per_wg = r.cpw;
    a.nwg = r.nwg;
    if (env_int("GRAVHMC_RESBATCH_TEST_ABORT", 0)) a.nwg += 8;  // test hook: partners that do not exist
    a.try_local = env_int("GRAVHMC_RESIDENT_LOCAL", 1);
    a.gfix = c->have_fix ? c->gfix : nullptr;
    a.dobs_c = c->dobs_c;
    a.low = c->low;
    a.high = c->high;
    a.kind = c->reg_kind;
    a.nz = c->shape[0];
    a.ny = c->shape[1];
    a.nx = c->shape[2];
    a.alpha = c->alpha;
    a.beta = c->beta;
    a.mwapr = c->mwapr;
    a.wm2 = c->wm2;
    a.C = C;
    a.T = T;
    a.L = tl.L;
    a.p0s = tl.p0s;
    a.us = tl.us;
    a.dt = dt;
    a.stop_any = carry ? 1 : 0;
    a.x_cur = r.bx;
    a.g_cur = r.bg;
    a.u_cur = r.bu;
    a.xs_io = b.xs;
    a.ps_io = b.ps;
    a.pst_io = b.pst;
    a.cst_io = b.cst;
    a.Tout = std::max(Tout, 1);
    a.accepted = tl.accepted;
    a.out5s = tl.out5s;
    a.xacc = (x_out || c->ps.on) ? tl.xacc : nullptr;
    a.n_io = b.n_io;
    a.slabd = b.slabd;
    a.flagg = b.flagg;
    a.xslabg = b.xslabg;
    a.dclg = b.dclg;
    a.xccg = b.xccg;
    a.xpub = b.xpub;
    a.tag0 = b.xg.tag;
    a.ltag = b.xg.ltag + 1u;
    a.abort_w = b.xg.abort_w;
    a.dbg = b.dbg;
    resbatch_fn_t f = resbatch_for(b.ks, b.nt, c->wv.on);
    // (gh_set_data may have added or removed the fixed part of the data term since the batch was planned)
    b.lds = resbatch_lds_doubles(c->ld, r.cpw, c->have_fix, c->wv.on) * sizeof(double);
    if (b.lds > (size_t)r.lds_max) return fail(c, GH_ERR_UNSUPPORTED, "resident batch kernel: the problem no longer fits the LDS");
    HIPCHK(c, allow_dynamic_lds(reinterpret_cast<const void *>(f), b.lds));
    TRY(prof_launch_mark(c, r.ev0));
    // (a plain launch: the grid was checked against the occupancy query in resbatch_plan; every wait inside is bounded)
    hipLaunchKernelGGL(f, dim3(r.nwg), dim3(RB_THREADS), b.lds, c->stream, a);
    HIPCHK(c, hipGetLastError());
    TRY(prof_launch_mark(c, r.ev1));
    int h_n[128];
    TRY(xg_read(c, b.xg));
    HIPCHK(c, hipMemcpyAsync(h_n, b.n_io, sizeof h_n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    b.xg.ltag += 1u;
    if (b.xg.seen[0] != 0u) {
        xg_give_up(b.xg, 1);
        fprintf(stderr, "libgravhmc: resident batch kernel timed out waiting for its workgroups; the chains take turns in "
                        "the resident chain kernel from here on\n");
        return GH_RESIDENT_ABORTED;
    }
    const int lock_steps = h_n[32];
    b.xg.tag += (unsigned)lock_steps;
    b.launches += 1;
    b.lock_steps += lock_steps;
    // results
    std::vector<int> acc((size_t)Kout);
    std::vector<double> o5((size_t)Kout * 5);
    HIPCHK(c, hipMemcpyAsync(acc.data(), tl.accepted, (size_t)Kout * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(o5.data(), tl.out5s, (size_t)Kout * 5 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // accepted models: one copy per chain (its done slots are adjacent) into pinned staging, rows picked from there --
    // a copy per accepted row into the caller's pageable array costs ~15 us each, hundreds per call
    bool want_rows = false;
    for (int ch = 0; ch < C; ++ch) {
        const int nd = h_n[16 + ch];
        if (nd > a.Tout || h_n[ch] > T)
            return fail(c, GH_ERR_HIP, "resident batch kernel: chain %d reports %d results in %d slots (%d of %d started)", ch, nd,
                        a.Tout, h_n[ch], T);
        // (the streaming posterior reads the accepted models where the kernel left them, in each chain's order)
        for (int i = 0; i < nd; ++i)
            if (acc[(size_t)ch * a.Tout + i]) TRY(post_feed_batch_row(c, ch, tl.xacc + ((size_t)ch * a.Tout + i) * M, c->stream));
        if (!x_out) continue;
        int last = -1;
        for (int i = 0; i < nd; ++i)
            if (acc[(size_t)ch * a.Tout + i]) last = i;
        if (last < 0) continue;
        if (!want_rows && (size_t)Kout * M > tl.h_xstage_n) {
            if (tl.h_xstage) HIPCHK(c, hipHostFree(tl.h_xstage));
            tl.h_xstage = nullptr;
            tl.h_xstage_n = (size_t)std::max(Kout, 32) * M;
            HIPCHK(c, hipHostMalloc((void **)&tl.h_xstage, tl.h_xstage_n * sizeof(double)));
        }
        want_rows = true;
        const size_t s0 = (size_t)ch * a.Tout;
        HIPCHK(c, hipMemcpyAsync(tl.h_xstage + s0 * M, tl.xacc + s0 * M, (size_t)(last + 1) * M * sizeof(double), hipMemcpyDeviceToHost,
                                 c->stream));
    }
    if (want_rows) HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int ch = 0; ch < C; ++ch) {
        const int nd = h_n[16 + ch];
        for (int i = 0; i < nd; ++i) {
            const size_t slot = (size_t)ch * a.Tout + i;
            accepted[slot] = acc[slot];
            memcpy(out5s + slot * 5, o5.data() + slot * 5, 5 * sizeof(double));
            if (x_out && acc[slot]) memcpy(x_out + slot * M, tl.h_xstage + slot * M, M * sizeof(double));
        }
        if (n_started) n_started[ch] = h_n[ch];
        if (n_done) n_done[ch] = nd;
        b.active[ch] = h_n[64 + ch] != 0;
        b.lost += h_n[48 + ch];
        b.chain_steps += h_n[80 + ch];
    }
    return prof_launch_end(c, r.ev0, r.ev1, lock_steps);
}

// The kernel gave up: the trajectories in flight start again from their chains' current samples (their own
// momentum, length and variate were kept on the device) in front of the new lists, on the chains-take-turns
// kernel.  Fills the host copies the caller needs to build that launch.
static int resbatch_inflight(gh_ctx *c, std::vector<int> &chains, std::vector<int> &L, std::vector<double> &us,
                             std::vector<double> &p0s)
{
    gh_ctx::Resident::LockStep &b = c->rs.ls;
    const size_t M = (size_t)c->M;
    std::vector<double> cst(16 * RB_CST);
    TRY(d2h(c, cst.data(), b.cst, cst.size()));
    for (int ch = 0; ch < b.C; ++ch)
        if (cst[(size_t)RB_CST * ch] != 0.0) {
            chains.push_back(ch);
            L.push_back((int)cst[(size_t)RB_CST * ch + 2]);
            us.push_back(cst[(size_t)RB_CST * ch + 3]);
            p0s.resize(p0s.size() + M);
            TRY(d2h(c, p0s.data() + p0s.size() - M, b.pst + (size_t)ch * M, M));
        }
    HIPCHK(c, hipMemsetAsync(b.cst, 0, 16 * RB_CST * sizeof(double), c->stream));
    for (bool &f : b.active) f = false;
    return GH_OK;
}
