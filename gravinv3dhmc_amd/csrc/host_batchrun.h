// libgravhmc host side: the two schedules of the fp64-MFMA chain batch, built from the steps of host_batch.h --
// lock-step rounds (gh_batch_trajectory) and desynchronised chains (gh_batch_run).  Two independent drivers:
// the tests compare one with the other.  Included once by gravhmc.hip.
#pragma once

// One round in lock-step: a trajectory of L[k] steps of every chain, Lmax + 1 sweeps.  *failed: a fused team pass
// of this round gave up -- nothing of the chains' current states was touched, the caller runs the round again
// (the fused form is off from here on).
static int batch_round_lockstep(gh_ctx *c, const double *p0s, double dt, const int *L, const double *us, int *accepted,
                                double *out5s, bool *failed)
{
    gh_ctx::Batch &b = c->bt;
    const int C = b.C;
    int Lmax = 0;
    for (int k = 0; k < C; ++k) Lmax = std::max(Lmax, L[k]);
    TRY(batch_upload_rows(c, p0s, C, b.Pw[0]));
    batch_sumsq_kernel<<<dim3((unsigned)b.n_pp0), dim3(256), 0, c->stream>>>(b.Pw[0], c->M, b.pp0_part);
    BatchSet in = b.cur();
    int pin = 0, xo = 0;
    for (int s = 0; s <= Lmax; ++s) {
        int phase[CB];
        bool first[CB], any_upd = false;
        for (int k = 0; k < CB; ++k) {
            phase[k] = (k < C && s < L[k]) ? PH_UPD : (k < C && s == L[k]) ? PH_PFIN : PH_IDLE;
            first[k] = s == 0;
            any_upd = any_upd || phase[k] == PH_UPD;
        }
        BatchAdjArgs a = batch_sweep_args(c, in, b.Pw[pin], nullptr, b.Xw[xo], b.Pw[pin ^ 1], dt, phase, first);
        TRY(batch_launch_adjoint(c, a, any_upd));
        in = b.work(xo, 0);
        if (any_upd) TRY(batch_evaluate(c, in.X, in.D, in.GREG, in.Rt));
        pin ^= 1;
        xo ^= 1;
    }
    HIPCHK(c, hipMemcpyAsync(b.h, b.scal, sizeof(double) * CB * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.h + b.h_pp(), b.pp_part, sizeof(double) * (size_t)b.n_waves * CB, hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipMemcpyAsync(b.h + b.h_pp0(), b.pp0_part, sizeof(double) * (size_t)b.n_pp0 * CB, hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    TRY(mfb_fused_failed(c, failed));
    if (*failed) return GH_OK;
    unsigned mask = 0;
    for (int k = 0; k < C; ++k) {
        const double pp1 = b.h_sum(b.h_pp(), b.n_waves, k), pp0 = b.h_sum(b.h_pp0(), b.n_pp0, k);
        accepted[k] = metropolis_step(pp0, pp1, b.h + 4 * k, us[k], b.U[k], out5s + 5 * k) ? 1 : 0;
        if (accepted[k]) mask |= 1u << k;
    }
    if (mask) {
        batch_copy_state(c, in, b.cur(), mask);  // (the last sweep's input: the proposals)
        HIPCHK(c, hipGetLastError());
        TRY(post_feed_batch(c, b.Xc, mask));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return GH_OK;
}

// ---- The chains desynchronised: per sweep every chain is in its own phase.  A chain that finished a trajectory
// starts the next one of its list in the following sweep -- or, when the list's next momentum is known and the
// proposal is accepted, has taken its first step already in the sweep of the final half step (PH_PFIN_SPEC).
// The part of the state that outlives the call (gh_ctx::Batch::Run) does so when the caller asks for n_started /
// n_done: the call then ends as soon as a chain has nothing left to start, the others keep their trajectory in
// flight and carry on in the next call -- no sweep is ever spent waiting for the slowest chain.  Without them
// every chain's T trajectories are completed.
struct BatchRun {
    gh_ctx *c;
    // the call: lists chain-major (T per chain), results in slots ch * Tout + i -- T per chain, plus one in
    // carry-over mode for the trajectory that came in flight
    const int T, *L;
    const double *const *p0s, *us, dt;
    int *accepted;
    double *out5s, *x_out;
    const bool carry;
    gh_ctx::Batch &b = c->bt;
    gh_ctx::Batch::Run &run = b.run;
    const bool use_spec = env_int("GRAVHMC_BATCH_SPEC", 1) != 0;
    const int C = b.C, Tout = carry ? T + 1 : T;
    const size_t M = (size_t)c->M;
    // (matrix-free team pass: b.Pstart keeps the momentum every trajectory in flight started with, for a replay)
    const bool keep_pstart = b.fus_on;
    int q_of[CB] = {}, done_of[CB] = {};  // trajectories of its list a chain has started / completed
    // The momentum of the trajectory a chain starts next waits in one of the chain's two staging rows (b.stage /
    // b.stage2, used alternately); it is sent on the copy stream while sweeps run.
    bool staged[CB] = {};
    int pending[CB], n_pending = 0;  // chains whose next momentum is still to be sent ahead
    unsigned fin = 0, spec = 0;  // the last sweep: chains that took their final half step / also a speculative first step
    int rs = 0, x_prop = 0;      // ... the working set and the models it read (the proposals of the chains that finished)

    // buffers, the working state of a run that starts afresh, the first momenta
    int begin()
    {
        const size_t n16 = M * CB, l16 = (size_t)c->ld * CB;
        if (!c->copy_stream) {
            HIPCHK(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
            HIPCHK(c, hipEventCreateWithFlags(&c->copy_ev, hipEventDisableTiming));
        }
        // two working sets: a sweep reads set run.ws, the evaluation behind it writes the other one
        TRY(dalloc(c, &b.stage2, n16));
        TRY(dalloc(c, &b.GREGw2, n16));
        TRY(dalloc(c, &b.Dw2, l16));
        TRY(dalloc(c, &b.Rtw2, l16));
        TRY(dalloc(c, &b.scal2, CB * 4));
        TRY(dalloc(c, &b.Pn, n16));
        TRY(dalloc(c, &b.pn0_part, (size_t)b.n_pp0 * CB));
        if (keep_pstart) TRY(dalloc(c, &b.Pstart, n16));
        if (!run.live) {
            // working state <- current state of every chain
            run = gh_ctx::Batch::Run();
            batch_copy_state(c, b.cur(), b.work(0, 0), (C >= 32) ? 0xffffffffu : ((1u << C) - 1u));
            HIPCHK(c, hipGetLastError());
            run.live = true;
        } else if (run.dt != dt) {
            for (int k = 0; k < C; ++k)
                if (run.active[k]) return fail(c, GH_ERR_ARG, "gh_batch_run: dt changed while trajectories are in flight");
        }
        run.dt = dt;
        for (int ch = 0; ch < C && T > 0; ++ch) {
            if (!run.active[ch])
                TRY(upload(ch, c->stream));
            else
                pending[n_pending++] = ch;
        }
        return GH_OK;
    }

    // list element q_of[ch] -> the chain's free staging row
    int upload(int ch, hipStream_t st)
    {
        run.par[ch] ^= 1;
        HIPCHK(c, hipMemcpyAsync((run.par[ch] ? b.stage2 : b.stage) + (size_t)ch * M, p0s[(size_t)ch * T + q_of[ch]],
                                 M * sizeof(double), hipMemcpyHostToDevice, st));
        staged[ch] = true;
        return GH_OK;
    }

    // staged rows of the chains in `mask` (sent now if not sent ahead) -> their columns of the interleaved array dst
    int scatter_staged(unsigned mask, double *dst)
    {
        TRY(wait_copies());
        unsigned even = 0, odd = 0;
        for (int ch = 0; ch < C; ++ch)
            if (mask & (1u << ch)) {
                if (!staged[ch]) TRY(upload(ch, c->stream));
                (run.par[ch] ? odd : even) |= 1u << ch;
            }
        const int64_t n16 = c->M * CB;
        if (even) batch_scatter_kernel<<<blocks256(n16), dim3(256), 0, c->stream>>>(b.stage, c->M, even, dst);
        if (odd) batch_scatter_kernel<<<blocks256(n16), dim3(256), 0, c->stream>>>(b.stage2, c->M, odd, dst);
        return GH_OK;
    }

    // (momenta sent ahead on the copy stream: wait for its last copy)
    int wait_copies()
    {
        HIPCHK(c, hipEventRecord(c->copy_ev, c->copy_stream));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->copy_ev, 0));
        return GH_OK;
    }

    // a chain takes the trajectory at the head of its list: bookkeeping shared by both kinds of start
    void take_next(int ch, double pp0_val, int s_first)
    {
        const size_t slot = (size_t)ch * T + q_of[ch];
        run.pp0[ch] = pp0_val;
        run.L_cur[ch] = L[slot];
        run.u_cur[ch] = us[slot];
        run.s_of[ch] = s_first;
        run.active[ch] = true;
        q_of[ch] += 1;
        staged[ch] = false;
        // the one after goes ahead once the next sweep has been queued (the staging copy blocks this thread, not the GPU)
        if (q_of[ch] < T) pending[n_pending++] = ch;
    }

    // false: the call is over.  starters: the idle chains with a trajectory left to start
    bool work_left(unsigned *starters) const
    {
        bool starved = false, any_active = false;
        *starters = 0;
        for (int k = 0; k < C; ++k) {
            if (!run.active[k] && q_of[k] < T) *starters |= 1u << k;
            if (run.active[k] || q_of[k] < T) any_active = true; else starved = true;
        }
        return carry && T > 0 ? !starved : any_active;
    }

    // working state <- current state, momenta of the chains in `mask` <- their next trajectory
    int start_chains(unsigned mask)
    {
        TRY(scatter_staged(mask, b.Pw[run.pin]));
        if (keep_pstart) batch_copy_cols(c, b.Pw[run.pin], b.Pstart, mask);
        batch_copy_state(c, b.cur(), b.work(run.xi, run.ws), mask);
        batch_sumsq_kernel<<<dim3((unsigned)b.n_pp0), dim3(256), 0, c->stream>>>(b.Pw[run.pin], c->M, b.pp0_part);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(b.h + b.h_pp0(), b.pp0_part, sizeof(double) * (size_t)b.n_pp0 * CB, hipMemcpyDeviceToHost,
                                 c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int ch = 0; ch < C; ++ch)
            if (mask & (1u << ch)) take_next(ch, b.h_sum(b.h_pp0(), b.n_pp0, ch), 0);
        return GH_OK;
    }

    // one sweep, every active chain in its own phase; the evaluation at the new models; the momenta that can go ahead
    int sweep()
    {
        int phase[CB];
        bool first[CB] = {}, any_upd = false;
        fin = spec = 0;
        for (int k = 0; k < CB; ++k) {
            phase[k] = PH_IDLE;
            if (k >= C || !run.active[k]) continue;
            if (run.s_of[k] < run.L_cur[k]) {
                phase[k] = PH_UPD;
                first[k] = run.s_of[k] == 0;
            } else {
                fin |= 1u << k;
                // the chain's next trajectory is known: its first step rides on this sweep
                phase[k] = (use_spec && q_of[k] < T) ? PH_PFIN_SPEC : PH_PFIN;
                if (phase[k] == PH_PFIN_SPEC) spec |= 1u << k;
            }
            any_upd = any_upd || phase[k] != PH_PFIN;
        }
        rs = run.ws;
        x_prop = run.xi;
        BatchAdjArgs a = batch_sweep_args(c, b.work(x_prop, rs), b.Pw[run.pin], b.Pn, b.Xw[x_prop ^ 1], b.Pw[run.pin ^ 1],
                                          dt, phase, first);
        if (spec) {
            TRY(scatter_staged(spec, b.Pn));
            batch_sumsq_kernel<<<dim3((unsigned)b.n_pp0), dim3(256), 0, c->stream>>>(b.Pn, c->M, b.pn0_part);
        }
        TRY(batch_launch_adjoint(c, a, any_upd));
        if (any_upd) {
            const BatchSet out = b.work(x_prop ^ 1, rs ^ 1);
            TRY(batch_evaluate(c, out.X, out.D, out.GREG, out.Rt, b.scal_of(rs ^ 1)));
            run.ws = rs ^ 1;
        }
        for (int i = 0; i < n_pending; ++i) TRY(upload(pending[i], c->copy_stream));
        n_pending = 0;
        run.xi ^= 1;
        run.pin ^= 1;
        for (int k = 0; k < C; ++k)
            if (run.active[k]) run.s_of[k] += 1;
        return GH_OK;
    }

    // what the Metropolis test of the chains in `fin` needs: their proposals' potentials (in the set the sweep
    // READ), the sums of the final half step and of the speculative starts.  *failed: see replay()
    int read_back(bool *failed)
    {
        HIPCHK(c, hipMemcpyAsync(b.h, b.scal_of(rs), sizeof(double) * CB * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(b.h + b.h_pp(), b.pp_part, sizeof(double) * (size_t)b.n_waves * CB, hipMemcpyDeviceToHost,
                                 c->stream));
        if (spec)
            HIPCHK(c, hipMemcpyAsync(b.h + b.h_pn0(), b.pn0_part, sizeof(double) * (size_t)b.n_pp0 * CB,
                                     hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return mfb_fused_failed(c, failed);
    }

    // A team pass since the last look gave up: what the trajectories in flight accumulated since is void, the
    // chains' current states are intact (nothing is committed before this point) -- every active chain starts
    // its trajectory again from its current state and its own momentum, on the two-pass kernels (which need no
    // co-residency)
    int replay()
    {
        if (!b.Pstart) return fail(c, GH_ERR_HIP, "gh_batch_run: the fused matrix-free batch pass timed out");
        unsigned act = 0;
        for (int k = 0; k < C; ++k)
            if (run.active[k]) {
                act |= 1u << k;
                run.s_of[k] = 0;
            }
        batch_copy_cols(c, b.Pstart, b.Pw[run.pin], act);
        batch_copy_state(c, b.cur(), b.work(run.xi, run.ws), act);
        HIPCHK(c, hipGetLastError());
        return GH_OK;
    }

    // the chains that took their final half step in the last sweep: Metropolis test, the accepted proposals
    // become the current states; a chain whose speculative first step holds carries on with that trajectory
    int finish_chains()
    {
        unsigned mask = 0;
        for (int k = 0; k < C; ++k) {
            if (!(fin & (1u << k))) continue;
            const size_t slot = (size_t)k * Tout + done_of[k];
            const bool acc = metropolis_step(run.pp0[k], b.h_sum(b.h_pp(), b.n_waves, k), b.h + 4 * k, run.u_cur[k], b.U[k],
                                             out5s + 5 * slot);
            accepted[slot] = acc ? 1 : 0;
            if (acc) mask |= 1u << k;
        }
        if (mask) {
            batch_copy_state(c, b.work(x_prop, rs), b.cur(), mask);
            HIPCHK(c, hipGetLastError());
            TRY(post_feed_batch(c, b.Xc, mask));
            if (x_out)
                for (int k = 0; k < C; ++k)
                    if (mask & (1u << k)) {
                        batch_extract_kernel<<<blocks256(c->M), dim3(256), 0, c->stream>>>(b.Xc, k, c->M, c->tmpM);
                        TRY(d2h(c, x_out + ((size_t)k * Tout + done_of[k]) * M, c->tmpM, M));
                    }
        }
        for (int k = 0; k < C; ++k)
            if (fin & (1u << k)) {
                run.active[k] = false;
                done_of[k] += 1;
                if ((spec & mask) & (1u << k)) {
                    // accepted, and the first step of the next trajectory has been taken: carry on
                    take_next(k, b.h_sum(b.h_pn0(), b.n_pp0, k), 1);
                    if (keep_pstart) batch_copy_cols(c, b.Pn, b.Pstart, 1u << k);
                }
            }
        return GH_OK;
    }

    int go(int *n_started, int *n_done)
    {
        TRY(begin());
        for (unsigned starters; work_left(&starters);) {
            if (starters) TRY(start_chains(starters));
            TRY(sweep());
            if (!fin) continue;
            bool failed = false;
            TRY(read_back(&failed));
            TRY(failed ? replay() : finish_chains());
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipStreamSynchronize(c->copy_stream));
        bool any_active = false;
        for (int k = 0; k < C; ++k) {
            if (n_done) {
                n_started[k] = q_of[k];
                n_done[k] = done_of[k];
            }
            any_active = any_active || run.active[k];
        }
        if (!any_active) run.live = false;  // (the working buffers are rebuilt from the current state next time)
        return GH_OK;
    }
};
