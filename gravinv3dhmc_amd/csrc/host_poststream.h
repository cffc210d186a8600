// libgravhmc host side: the streaming posterior (poststream.hip.h) -- its state, the hooks the chain paths
// call where an accepted state lies in HBM, and what the gh_posterior_stream_* entry points do.  With no stream
// allocated every hook returns before it touches the device.  Included once by gravhmc.hip.
#pragma once

static dim3 post_grid(const gh_ctx *c) { return dim3((unsigned)((c->M + 255) / 256)); }

// the chain's accepted state number `cnt` (1-based) is inside the recording window
static bool post_due(const gh_ctx::PostStream &p, int64_t cnt)
{
    return p.on && cnt > p.from && cnt - p.from <= p.count;
}

static PostCounts post_counts(const int64_t *v)
{
    PostCounts o;
    for (int i = 0; i < POST_MAX_CHAINS; ++i) o.n[i] = v[i];
    return o;
}

static void post_count_sample(gh_ctx::PostStream &p, int chain)
{
    p.n[chain] += 1;
    if (p.n[chain] % p.d.b == 0) p.K[chain] += 1;
}

// One sample of chain slot `chain` from a contiguous device row (weighted: x = wm m), on stream s -- the
// context's own, or one that is synchronised with it before anything else touches the state.
static int post_feed_row(gh_ctx *c, int chain, const double *x_dev, bool weighted, hipStream_t s)
{
    gh_ctx::PostStream &p = c->ps;
    if (!p.on || chain < 0 || chain >= p.d.C) return GH_OK;
    post_count_sample(p, chain);
    post_accum_row_kernel<<<post_grid(c), dim3(256), 0, s>>>(p.d, x_dev, chain, weighted ? 1 : 0, (long long)p.n[chain]);
    HIPCHK(c, hipGetLastError());
    p.launches += 1;
    return GH_OK;
}

// Single chain: state number st->accept_count of the chain whose state `st` holds (the context itself, or a
// chain of a batch on the shift-invariant store: then the batch's bookkeeping applies).
static int post_feed_single(gh_ctx *c, gh_ctx *st, const double *x_dev)
{
    if (st == c) {
        if (!post_due(c->ps, st->accept_count)) return GH_OK;
        return post_feed_row(c, c->ps.slot, x_dev, c->weighted, c->stream);
    }
    for (size_t i = 0; i < c->kids.size(); ++i)
        if (c->kids[i] == st) {
            c->bt_accepts[i] += 1;
            if (!post_due(c->ps, c->bt_accepts[i])) return GH_OK;
            return post_feed_row(c, (int)i, x_dev, c->weighted, c->stream);
        }
    return GH_OK;
}

// The contiguous device row x_dev into the next slot of st's ring of accepted samples.
static int ring_store_row(gh_ctx *c, gh_ctx *st, const double *x_dev)
{
    ring_store_kernel<<<post_grid(c), dim3(256), 0, c->stream>>>(x_dev, c->weighted ? c->wm : nullptr, c->M,
                                                                st->ring + (size_t)st->ring_next * (size_t)c->M);
    HIPCHK(c, hipGetLastError());
    st->ring_next = (st->ring_next + 1) % st->ring_K;
    st->ring_count += 1;
    return GH_OK;
}

// The chain whose state `st` holds accepted the state in x_dev: counted, into the ring once record_from states
// were accepted, to the streaming posterior, and to the caller's row x_out (or nullptr) -- on c's stream.
static int chain_accept_row(gh_ctx *c, gh_ctx *st, const double *x_dev, int64_t record_from, double *x_out)
{
    st->accept_count += 1;
    if (st->ring && st->accept_count > record_from) TRY(ring_store_row(c, st, x_dev));
    TRY(post_feed_single(c, st, x_dev));
    if (x_out) HIPCHK(c, hipMemcpyAsync(x_out, x_dev, (size_t)c->M * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return GH_OK;
}

// A chain of a batch accepted the state in the contiguous device row x_dev.
static int post_feed_batch_row(gh_ctx *c, int chain, const double *x_dev, hipStream_t s)
{
    c->bt_accepts[chain] += 1;
    if (!post_due(c->ps, c->bt_accepts[chain])) return GH_OK;
    return post_feed_row(c, chain, x_dev, c->weighted, s);
}

// The chains in `mask` accepted the states that lie in the interleaved Xc[j][chain]: one launch for all that are due.
static int post_feed_batch(gh_ctx *c, const double *Xc, unsigned mask)
{
    gh_ctx::PostStream &p = c->ps;
    unsigned due = 0;
    for (int k = 0; k < CB; ++k)
        if (mask & (1u << k)) {
            c->bt_accepts[k] += 1;
            if (k < p.d.C && post_due(p, c->bt_accepts[k])) due |= 1u << k;
        }
    if (!due) return GH_OK;
    for (int k = 0; k < CB; ++k)
        if (due & (1u << k)) post_count_sample(p, k);
    post_accum_batch_kernel<<<post_grid(c), dim3(256), 0, c->stream>>>(p.d, Xc, CB, due, post_counts(p.n));
    HIPCHK(c, hipGetLastError());
    p.launches += 1;
    return GH_OK;
}

template <typename T>
static void post_release(gh_ctx *c, T *&p)
{
    dev_release(c, p);
}

static int post_free(gh_ctx *c)
{
    gh_ctx::PostStream &p = c->ps;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    post_release(c, p.d.mean);
    post_release(c, p.d.M2);
    post_release(c, p.d.bsum);
    post_release(c, p.d.bmean);
    post_release(c, p.d.bM2);
    post_release(c, p.d.H);
    post_release(c, p.lo);
    post_release(c, p.hi);
    post_release(c, p.iw);
    post_release(c, p.row);
    post_release(c, p.out);
    post_release(c, p.qout);
    p = gh_ctx::PostStream();
    return GH_OK;
}

// 1 / wm of the weights the context has NOW: at allocation on a weighted context, and again from gh_weight (a stream
// that is older than the weights gets its row here; one that outlives them follows the new ones).
static int post_weights(gh_ctx *c)
{
    gh_ctx::PostStream &p = c->ps;
    p.d.iw = nullptr;  // (an unweighted store: the rows hold m itself)
    if (!c->weighted) return GH_OK;
    TRY(dalloc(c, &p.iw, (size_t)c->M, false));
    post_recip_kernel<<<post_grid(c), dim3(256), 0, c->stream>>>(c->wm, c->M, p.iw);
    HIPCHK(c, hipGetLastError());
    p.d.iw = p.iw;
    return GH_OK;
}

static int post_alloc(gh_ctx *c, int chains, int bins, int batch_len, int64_t record_from, int64_t record_count,
                      const double *lo, const double *hi)
{
    gh_ctx::PostStream &p = c->ps;
    const size_t M = (size_t)c->M, MC = M * (size_t)chains;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = dalloc(c, &p.d.mean, MC);
    if (rc == GH_OK) rc = dalloc(c, &p.d.M2, MC);
    if (rc == GH_OK) rc = dalloc(c, &p.d.bsum, MC);
    if (rc == GH_OK) rc = dalloc(c, &p.d.bmean, MC);
    if (rc == GH_OK) rc = dalloc(c, &p.d.bM2, MC);
    if (rc == GH_OK) rc = dalloc(c, &p.d.H, M * (size_t)bins);
    if (rc == GH_OK) rc = dalloc(c, &p.lo, M, false);
    if (rc == GH_OK) rc = dalloc(c, &p.hi, M, false);
    if (rc == GH_OK) rc = dalloc(c, &p.row, M, false);
    if (rc == GH_OK) rc = dalloc(c, &p.out, 4 * M, false);
    if (rc == GH_OK) rc = h2d(c, p.lo, lo, M);
    if (rc == GH_OK) rc = h2d(c, p.hi, hi, M);
    if (rc != GH_OK) {
        const std::string why = c->err;
        post_free(c);
        c->err = why;
        return rc;
    }
    p.d.lo = p.lo;
    p.d.hi = p.hi;
    p.d.M = c->M;
    p.d.C = chains;
    p.d.B = bins;
    p.d.b = batch_len;
    p.from = record_from;
    p.count = record_count;
    p.slot = 0;
    rc = post_weights(c);
    if (rc != GH_OK) {
        const std::string why = c->err;
        post_free(c);
        c->err = why;
        return rc;
    }
    p.on = true;
    return GH_OK;
}

static int post_read(gh_ctx *c, int64_t *n_per_chain, double *mean, double *sd, double *rhat, double *ess,
                     double *chain_mean, double *chain_M2)
{
    gh_ctx::PostStream &p = c->ps;
    const size_t M = (size_t)c->M;
    const int C = p.d.C;
    HIPCHK(c, hipSetDevice(c->device));
    if (n_per_chain)
        for (int k = 0; k < C; ++k) n_per_chain[k] = p.n[k];
    if (mean || sd || rhat || ess) {
        post_finish_kernel<<<post_grid(c), dim3(256), 0, c->stream>>>(p.d, post_counts(p.n), post_counts(p.K), p.out, p.out + M,
                                                                       p.out + 2 * M, p.out + 3 * M);
        HIPCHK(c, hipGetLastError());
        if (mean) TRY(d2h(c, mean, p.out, M));
        if (sd) TRY(d2h(c, sd, p.out + M, M));
        if (rhat) TRY(d2h(c, rhat, p.out + 2 * M, M));
        if (ess) TRY(d2h(c, ess, p.out + 3 * M, M));
    }
    // per chain: rows of the caller's (chains x M) arrays out of the interleaved state
    std::vector<double> tmp;
    for (int which = 0; which < 2; ++which) {
        double *dst = which ? chain_M2 : chain_mean;
        if (!dst) continue;
        tmp.resize(M * (size_t)C);
        TRY(d2h(c, tmp.data(), which ? p.d.M2 : p.d.mean, tmp.size()));
        for (size_t j = 0; j < M; ++j)
            for (int k = 0; k < C; ++k) dst[(size_t)k * M + j] = tmp[j * (size_t)C + (size_t)k];
    }
    return GH_OK;
}

static int post_quantiles(gh_ctx *c, int nq, const double *q, double *out)
{
    gh_ctx::PostStream &p = c->ps;
    const size_t M = (size_t)c->M;
    HIPCHK(c, hipSetDevice(c->device));
    if ((size_t)nq * M > p.qout_n) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        post_release(c, p.qout);
        TRY(dalloc(c, &p.qout, (size_t)nq * M, false));
        p.qout_n = (size_t)nq * M;
    }
    PostQ qs = {};
    for (int i = 0; i < nq; ++i) qs.q[i] = q[i];
    long long ntot = 0;
    for (int k = 0; k < p.d.C; ++k) ntot += p.n[k];
    post_quantile_kernel<<<post_grid(c), dim3(256), 0, c->stream>>>(p.d, ntot, nq, qs, p.qout);
    HIPCHK(c, hipGetLastError());
    return d2h(c, out, p.qout, (size_t)nq * M);
}
