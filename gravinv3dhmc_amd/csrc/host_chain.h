// libgravhmc host side: one trajectory of the single chain on the sweep path (the launches of host_sweep.h, one
// per leapfrog step), with the speculative first step of the next one.  Included once by gravhmc.hip.
#pragma once

// d, r and the scalars of the current sample after launches of the resident chain kernel
static int chain_state_fresh(gh_ctx *c)
{
    if (!c->st_stale) return GH_OK;
    TRY(eval_forward(c, c->xb[c->xcur], c->st[c->cur]));
    TRY(scal_ready(c, c->st[c->cur]));
    TRY(read_state_scalars(c, c->st[c->cur], c->U_cur));
    c->st_stale = false;
    return GH_OK;
}

static inline int other_of3(int a, int b)
{
    for (int i = 0; i < 3; ++i)
        if (i != a && i != b) return i;
    return 0;
}

// The momentum of the NEXT trajectory: a pointer known when the call is made (p, or nullptr: none), or `late`,
// consulted once, right before the upload on the copy stream -- the trajectory feeder (host_feed.h) draws that row
// while this trajectory's sweeps are already queued, and blocks there until it is complete (nullptr: the stream ended).
struct P0Next {
    const double *p = nullptr;
    const double *(*late)(void *) = nullptr;
    void *user = nullptr;
};

// next: momentum of the NEXT trajectory, valid until this call returns.  Announced
// this way (gh_chain_run) it is uploaded on a second stream while this trajectory's sweeps run --
// through the public gh_chain_prefetch_momentum the upload happens before them, with the GPU idle.
static int chain_trajectory_impl(gh_ctx *c, const double *p0, double dt, int L, double u, P0Next next,
                                 int *accepted, double out5[5])
{
    if (!c || !p0 || !accepted || !out5) return fail(c, GH_ERR_ARG, "gh_chain_trajectory: null pointer");
    TRY(need(c, c->chain_ready, "gh_chain_trajectory: call gh_chain_init first"));
    if (L < 1) return fail(c, GH_ERR_ARG, "gh_chain_trajectory: L must be >= 1");
    HIPCHK(c, hipSetDevice(c->device));
    TRY(chain_state_fresh(c));
    // (sweeps launched from here may run on teams of workgroups whose time-out this function handles)
    struct TeamsOk {
        gh_ctx *c;
        ~TeamsOk() { c->chain_teams_ok = false; }
    } teams_guard{c};
    c->chain_teams_ok = true;
    const size_t M = (size_t)c->M;
    const WorkLayout &w = c->work;
    const int nt = c->n_teams;
    // Was the first step of this trajectory already taken speculatively by the previous call's
    // last sweep (same momentum, same dt, previous proposal accepted)?
    const bool use_spec = c->spec_valid && c->spec_dt == dt && p0[0] == c->spec_probe[0] &&
                          p0[c->M / 2] == c->spec_probe[1] && p0[c->M - 1] == c->spec_probe[2];
    int xin, pin, sin, s0;
    if (use_spec) {
        xin = c->spec_x;
        pin = c->spec_p;
        sin = c->spec_set;
        s0 = 1;
        c->spec_hits += 1;
    } else {
        // momentum upload + kinetic energy of p0 (hmc.py:95-104)
        HIPCHK(c, hipMemcpyAsync(c->pb[0], p0, M * sizeof(double), hipMemcpyHostToDevice, c->stream));
        sumsq_kernel<<<dim3(c->work.pp0), dim3(256), 0, c->stream>>>(c->pb[0], c->M, c->pp0_part);
        xin = c->xcur;
        pin = 0;
        sin = c->cur;
        s0 = 0;
        if (c->spec_valid) c->spec_misses += 1;
    }
    c->spec_valid = false;
    for (int s = s0; s < L; ++s) {
        const int xout = other_of3(c->xcur, xin);
        const int sout = (sin != c->cur) ? sin : other_of3(c->cur, c->cur);
        SweepArgs a{};
        a.mode = SW_ADJ | SW_UPD | (c->wv.on ? 0 : SW_FWD);
        a.r = c->st[sin].r;
        a.greg = c->st[sin].greg;
        a.x_in = c->xb[xin];
        a.p_in = c->pb[pin];
        a.x_out = c->xb[xout];
        a.p_out = c->pb[pin ^ 1];
        a.low = c->low;
        a.high = c->high;
        a.c_u = (s == 0) ? dt * 0.5 : dt;
        a.dt = dt;
        a.slab = c->slab;
        TRY(launch_sweep(c, a));
        TRY(finalize(c, c->xb[xout], c->st[sout]));
        xin = xout;
        pin ^= 1;
        sin = sout;
    }
    // Last half step of the momentum + kinetic energy (hmc.py:151-157).  When the caller has
    // announced the next trajectory's momentum, the same sweep also takes that trajectory's
    // first leapfrog step from the proposal (valid if the proposal is accepted): the gradient
    // at the proposal is needed by both, so the extra sweep per trajectory disappears.
    bool spec = c->pn_valid;
    double probe[3] = {c->pn_probe[0], c->pn_probe[1], c->pn_probe[2]};
    double pn_pp0 = c->pn_pp0;
    bool pn_deferred = false;
    const double *p0_next = next.late ? next.late(next.user) : next.p;
    if (p0_next) {
        if (!c->copy_stream) {
            HIPCHK(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
            HIPCHK(c, hipEventCreateWithFlags(&c->copy_ev, hipEventDisableTiming));
        }
        // (c->pn was last read by the previous trajectory's final sweep, which has completed)
        HIPCHK(c, hipMemcpyAsync(c->pn, p0_next, M * sizeof(double), hipMemcpyHostToDevice, c->copy_stream));
        HIPCHK(c, hipEventRecord(c->copy_ev, c->copy_stream));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->copy_ev, 0));
        // its initial kinetic energy, summed exactly like gh_chain_prefetch_momentum does
        sumsq_kernel<<<dim3(c->work.pp0), dim3(256), 0, c->stream>>>(c->pn, c->M, c->pn0_part);
        probe[0] = p0_next[0];
        probe[1] = p0_next[c->M / 2];
        probe[2] = p0_next[c->M - 1];
        spec = true;
        pn_deferred = true;
    }
    const int xs = other_of3(c->xcur, xin), ss = other_of3(c->cur, sin);
    {
        SweepArgs a{};
        a.mode = SW_ADJ | SW_PFIN;
        a.r = c->st[sin].r;
        a.greg = c->st[sin].greg;
        a.p_in = c->pb[pin];
        a.p_out = c->pb[pin ^ 1];
        a.c_p = dt * 0.5;
        a.pp_part = c->pp_part;
        if (spec) {
            a.mode |= SW_SPEC | SW_UPD | (c->wv.on ? 0 : SW_FWD);
            a.pn_in = c->pn;
            a.x_in = c->xb[xin];
            a.x_out = c->xb[xs];
            a.low = c->low;
            a.high = c->high;
            a.c_u = dt * 0.5;
            a.dt = dt;
            a.slab = c->slab;
        }
        TRY(launch_sweep(c, a));
        if (spec) TRY(finalize(c, c->xb[xs], c->st[ss]));
    }
    double *h = c->h_scal, *h_pp = h + w.h_pp(), *h_pp0 = h + w.h_pp0(), *h_pn0 = h + w.h_pn0();
    TRY(scal_ready(c, c->st[sin]));
    if (spec) TRY(scal_ready(c, c->st[ss]));
    HIPCHK(c, hipMemcpyAsync(h + w.h_state(), c->st[sin].scal, 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    const bool cg_on = coupling_on(c);  // (cross-gradient or amplitude term: Phi has a slot per state set)
    if (cg_on) HIPCHK(c, hipMemcpyAsync(h + w.h_phi(), c->st[sin].phi, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_pp, c->pp_part, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost,
                             c->stream));
    if (spec) {
        HIPCHK(c, hipMemcpyAsync(h + w.h_spec(), c->st[ss].scal, 4 * sizeof(double), hipMemcpyDeviceToHost,
                                 c->stream));
    }
    if (!use_spec)
        HIPCHK(c, hipMemcpyAsync(h_pp0, c->pp0_part, (size_t)w.pp0 * sizeof(double),
                                 hipMemcpyDeviceToHost, c->stream));
    if (pn_deferred)
        HIPCHK(c, hipMemcpyAsync(h_pn0, c->pn0_part, (size_t)w.pp0 * sizeof(double),
                                 hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // a team sweep of this trajectory gave up (its workgroups were not all resident): nothing of
    // the chain's current state was touched -- run the trajectory again, in row panels.  Sharded
    // chain: decided by all ranks together, below (the flag rides on the scalar all-reduce)
    TRY(lonsym_epilogue_check(c));
    bool failed = false;
    TRY(team_failed(c, &failed));
    if (!failed) TRY(mft_failed(c, &failed));  // (matrix-free chain on teams: same contract)
    auto redo = [&]() -> int {
        c->spec_valid = c->pn_valid = false;
        const int rc = chain_trajectory_impl(c, p0, dt, L, u, P0Next{p0_next}, accepted, out5);
        team_resume(c);
        return rc;
    };
    if (failed && c->sh.kind == 0) return redo();
    if (pn_deferred) {
        double s = 0.0;
        for (int t = 0; t < w.pp0; ++t) s += h_pn0[t];
        pn_pp0 = s;
    }
    double pp1 = 0.0, pp0 = 0.0;
    for (int t = 0; t < nt; ++t) pp1 += h_pp[t];
    if (use_spec)
        pp0 = c->spec_pp0;
    else
        for (int t = 0; t < w.pp0; ++t) pp0 += h_pp0[t];
    double pn_pp0_g = pn_pp0;
    if (shard_cols(c)) {
        // kinetic energies are sums over cells: combine the ranks' parts (same bits everywhere)
        double v[4] = {pp1, use_spec ? 0.0 : pp0, spec ? pn_pp0 : 0.0, failed ? 1.0 : 0.0};
        if (failed) v[0] = v[1] = v[2] = 0.0;  // (whatever the aborted sweeps left: not worth a NaN in the sum)
        TRY(comm_allreduce_host(c, v, 4));
        if (v[3] != 0.0) {
            // some rank's team sweep gave up: its slab went into everybody's d and r through the
            // all-reduces of this trajectory -- every rank repeats it, in row panels, together
            if (!failed) TRY(team_mark_failed(c, "another rank's"));
            return redo();
        }
        pp1 = v[0];
        if (!use_spec) pp0 = v[1];
        pn_pp0_g = v[2];
    }
    const bool acc = metropolis_step(pp0, pp1, h + w.h_state(), u, c->U_cur, out5);
    if (acc) {
        c->xcur = xin;
        c->cur = sin;
        if (cg_on) c->cg.phi_cur = h[w.h_phi()];
        if (spec) {
            c->spec_valid = true;
            c->spec_dt = dt;
            c->spec_pp0 = pn_pp0_g;
            c->spec_x = xs;
            c->spec_p = pin ^ 1;
            c->spec_set = ss;
            c->spec_probe[0] = probe[0];
            c->spec_probe[1] = probe[1];
            c->spec_probe[2] = probe[2];
        }
    } else if (spec) {
        c->spec_misses += 1;  // the speculative step belonged to a rejected proposal
    }
    c->pn_valid = false;
    *accepted = acc ? 1 : 0;
    c->cg.phi_last = c->cg.phi_cur;  // (Phi of the state the chain is left in, as out5[0..2])
    return GH_OK;
}

static int chain_trajectory_impl(gh_ctx *c, const double *p0, double dt, int L, double u, const double *p0_next,
                                 int *accepted, double out5[5])
{
    return chain_trajectory_impl(c, p0, dt, L, u, P0Next{p0_next}, accepted, out5);
}
