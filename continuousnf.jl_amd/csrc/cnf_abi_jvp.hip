// C ABI of libcnfhip.so, forward mode of one model (the ensemble form is ens_eval's `jv`, cnf_abi_ens.hip).
#include "cnf_abi_int.h"
using namespace cnfabi;

// ---- forward-mode derivatives (include/cnfhip_jvp.h; cnf_tangent.hip) ------------------------------------------------------------
// Both entry points are: the solve of the call they extend -- inference's with SolveCall's `jvp` hook: it keeps the step
// attempts in jvp_trace and enqueues k_tangent_wave behind a one-launch solve, or files the accepted steps of the
// one-attempt-at-a-time route --, the tangent launch over the host-filed steps where it has not gone out yet, and the primal
// outputs handed over once nothing can fail any more.
static const int JVP_TRACE_DEFAULT = 4096, JVP_TRACE_MAX = 65536;
// what both calls check before any device is asked for, and the envelope
static cnf_status jvp_check(cnf_handle h, int mode, int B, bool ptrs_ok, const float* d_ps, const float* d_x, int R, int trace_cap) {
    if (!h) return CNF_ERR_BAD_ARG;
    if (mode != CNF_MODE_TEST && mode != CNF_MODE_TRAIN) return fail(h, CNF_ERR_BAD_ARG, "unknown mode");
    if (!ptrs_ok) return fail(h, CNF_ERR_BAD_ARG, "null pointer");
    if (!d_ps && !d_x) return fail(h, CNF_ERR_BAD_ARG, "both directions are null");
    if (R < 1 || R > TG_MAX_R) return fail(h, CNF_ERR_BAD_ARG, "R must be within [1, 65535]");
    if (trace_cap < 0 || trace_cap > JVP_TRACE_MAX) return fail(h, CNF_ERR_BAD_ARG, "trace_cap must be within [0, 65536]");
    if (B < 1) return fail(h, CNF_ERR_BAD_SHAPE, "a tangent call needs B >= 1");
    if (!tangent_supported(h->nd_wave))
        return fail(h, CNF_ERR_UNSUPPORTED, "tangents: two layers, tanh then tanh or identity, n_in <= 16, at most 64 hidden units (16 with the identity), no conditioning");
    if (h->bd.kind) return fail(h, CNF_ERR_UNSUPPORTED, "tangents: the default base distribution only");
    if (h->shard_reduce != nullptr || h->shard_comm != nullptr) return fail(h, CNF_ERR_UNSUPPORTED, "tangents: no lock-step shards");
    return CNF_OK;
}
// behind the solve: the tangent launch where the solve's route left it to the caller, then the accepted steps onto the handle
static cnf_status jvp_finish(cnf_handle h, JvpCall& jc, const cnf_solve_stats& sst, int* launches, hipStream_t st) {
    if (jc.enqueued) {
        const int att = sst.naccept + sst.nreject;
        if (att > jc.trace_cap) return fail(h, CNF_ERR_UNSUPPORTED, "the solve made more step attempts than trace_cap");
        std::vector<float> rows((size_t)4 * att);
        if (att > 0) HIPCHK(h, hipMemcpyAsync(rows.data(), h->jvp_trace, rows.size() * sizeof(float), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
        h->jvp_t.clear(); h->jvp_h.clear();
        for (int i = 0; i < att; ++i)
            if (rows[4 * (size_t)i + 3] != 0.f) { h->jvp_t.push_back(rows[4 * (size_t)i]); h->jvp_h.push_back(rows[4 * (size_t)i + 1]); }
        return CNF_OK;
    }
    if (!jc.host_steps) return fail(h, CNF_ERR_UNSUPPORTED, "tangents: the solve took a route that files no steps");
    const size_t n = jc.t.size();
    if (n > (size_t)jc.trace_cap) return fail(h, CNF_ERR_UNSUPPORTED, "the solve took more steps than trace_cap");
    std::vector<float> rows(4 * n);
    for (size_t i = 0; i < n; ++i) { rows[4 * i] = jc.t[i]; rows[4 * i + 1] = jc.h[i]; rows[4 * i + 2] = 0.f; rows[4 * i + 3] = 1.f; }
    if (n > 0) HIPCHK(h, hipMemcpyAsync(h->jvp_trace, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice, st));
    jc.ta.st = h->last_state; jc.ta.trace = h->jvp_trace; jc.ta.trace_cap = jc.trace_cap; jc.ta.n_rows = (int)n;
    const cnf_status s = tangent_launch(jc.ta, jc.train, st);
    if (s != CNF_OK) return fail(h, s, "the tangent launch failed to start");
    ++*launches;
    HIPCHK(h, hipStreamSynchronize(st));                   // (`rows` is on its way until here)
    h->jvp_t = jc.t; h->jvp_h = jc.h;
    return CNF_OK;
}

extern "C" cnf_status cnf_inference_jvp(cnf_handle h, int mode, const float* xs, const float* eps, int B, const float* d_ps,
                                        const float* d_xs, int R, const cnf_solve_opts* opts, int trace_cap, float* logpx, float* regs,
                                        float* d_out, cnf_solve_stats* stats, void* stream) {
    const bool train = mode == CNF_MODE_TRAIN;
    cnf_status s = jvp_check(h, mode, B, xs && opts && logpx && regs && d_out && (!train || eps), d_ps, d_xs, R, trace_cap);
    if (s != CNF_OK) return s;
    h->jvp_valid = false;
    if (!wave_solve_supported(h->nd_wave, train, B)) return fail(h, CNF_ERR_UNSUPPORTED, "tangents: no one-launch solve of this batch size");
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(h, hipSetDevice(h->device));
    JvpCall jc;
    jc.train = train; jc.trace_cap = trace_cap > 0 ? trace_cap : JVP_TRACE_DEFAULT;
    const size_t Bz = (size_t)B;
    if ((size_t)4 * jc.trace_cap > h->jvp_trace.capacity() || 4 * Bz > h->jvp_buf.capacity()) {
        HIPCHK(h, hipStreamSynchronize(st));
        RESERVE(h, h->jvp_trace, (size_t)4 * jc.trace_cap);
        RESERVE(h, h->jvp_buf, (4 * Bz + 1023) & ~(size_t)1023);
    }
    float* p_logpx = h->jvp_buf; float* p_regs = p_logpx + Bz;
    TangentArgs& ta = jc.ta;
    ta.nd = h->nd_wave; ta.P = h->d_params; ta.dP = d_ps; ta.n_params = (int)h->n_params; ta.eps = train ? eps : nullptr;
    ta.B = B; ta.R = R; ta.sampling = 0; ta.x = xs; ta.dX = d_xs; ta.out = d_out;
    cnf_solve_stats sst{};
    s = inference_impl(h, mode, xs, eps, p_logpx, p_regs, nullptr, nullptr, B, opts, &sst, stream, &jc);
    if (s != CNF_OK) return s;
    int launches = sst.launches;
    if ((s = jvp_finish(h, jc, sst, &launches, st)) != CNF_OK) return s;
    HIPCHK(h, hipMemcpyAsync(logpx, p_logpx, Bz * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIPCHK(h, hipMemcpyAsync(regs, p_regs, 3 * Bz * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIPCHK(h, hipStreamSynchronize(st));
    h->jvp_valid = true;
    if (stats) { *stats = sst; stats->launches = launches; }
    return CNF_OK;
}

// Sampling.  Its primal half is cnf_generate_record's own RECORDED solve, not the plain one-launch solve: `generate(with_logp)` is
// that call, and the two routes differ in the last bits (and sometimes by a step) -- so that (z, logq) are that call's bit for
// bit, the solve is taken on its route, the accepted steps come back with the record's step sizes, and the tangent launch
// follows over them.  Like every solve it ends the record on the handle; the step sizes cnf_grad_steps reports are put back.
extern "C" cnf_status cnf_generate_jvp(cnf_handle h, int mode, const float* z0, const float* eps, int B, const float* d_ps,
                                       const float* d_z0, int R, const cnf_solve_opts* opts, int trace_cap, float* z_out, float* logq,
                                       float* d_z, float* d_logq, cnf_solve_stats* stats, void* stream) {
    const bool train = mode == CNF_MODE_TRAIN;
    cnf_status s = jvp_check(h, mode, B, z0 && opts && z_out && logq && d_z && d_logq && (!train || eps), d_ps, d_z0, R, trace_cap);
    if (s != CNF_OK) return s;
    h->jvp_valid = false;
    hipStream_t st = (hipStream_t)stream;
    if ((s = grad_prologue(h, mode, B, true, "a tangent call needs B >= 1", train, st)) != CNF_OK) return s;
    HIPCHK(h, hipSetDevice(h->device));
    JvpCall jc;
    jc.train = train; jc.trace_cap = trace_cap > 0 ? trace_cap : JVP_TRACE_DEFAULT;
    const int n_in = h->nd.n_in, D = rows_of(h, mode);
    const size_t Bz = (size_t)B, nz = (size_t)n_in * Bz;
    if ((size_t)4 * jc.trace_cap > h->jvp_trace.capacity() || nz + Bz > h->jvp_buf.capacity()) {
        HIPCHK(h, hipStreamSynchronize(st));
        RESERVE(h, h->jvp_trace, (size_t)4 * jc.trace_cap);
        RESERVE(h, h->jvp_buf, (nz + Bz + 1023) & ~(size_t)1023);
    }
    float* p_z = h->jvp_buf; float* p_logq = p_z + nz;
    // u0 = [z0; 0] where cnf_generate_record assembles it
    float* u0 = h->g_US[0];
    HIPCHK(h, hipMemsetAsync(u0, 0, (size_t)D * Bz * sizeof(float), st));
    HIPCHK(h, hipMemcpy2DAsync(u0, (size_t)D * sizeof(float), z0, (size_t)n_in * sizeof(float), (size_t)n_in * sizeof(float), Bz,
                               hipMemcpyDeviceToDevice, st));
    TangentArgs& ta = jc.ta;
    ta.nd = h->nd_wave; ta.P = h->d_params; ta.dP = d_ps; ta.n_params = (int)h->n_params; ta.eps = train ? eps : nullptr;
    ta.B = B; ta.R = R; ta.sampling = 1; ta.x = z0; ta.dX = d_z0; ta.out = d_z; ta.out_logq = d_logq;
    Recorder rec;
    cnf_solve_stats sst{};
    const std::vector<float> kept_hs = h->last_hs;
    s = record_solve(h, mode, u0, train ? eps : nullptr, B, opts, rec, sst, stream);
    h->last_hs = kept_hs;
    if (s != CNF_OK) return s;
    int launches = sst.launches;
    launch_generate_post(n_in, D, h->bd, h->g_US[1], z0, p_z, p_logq, B, st);
    HIPCHK(h, hipGetLastError());
    ++launches;
    // the accepted steps: the record's signed sizes, the times as the controller adds them up (the last step ends at t1)
    jc.host_steps = true;
    float t = opts->t0;
    for (float hn : rec.hs) { jc.t.push_back(t); jc.h.push_back(hn); t += hn; }
    if ((s = jvp_finish(h, jc, sst, &launches, st)) != CNF_OK) return s;
    HIPCHK(h, hipMemcpyAsync(z_out, p_z, nz * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIPCHK(h, hipMemcpyAsync(logq, p_logq, Bz * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIPCHK(h, hipStreamSynchronize(st));
    h->jvp_valid = true;
    if (stats) { *stats = sst; stats->launches = launches; }
    return CNF_OK;
}

extern "C" int cnf_jvp_steps(cnf_handle h, float* t_host, float* h_host, int cap) {
    return h ? copy_steps(h->jvp_valid, h->jvp_t, h->jvp_h, t_host, h_host, cap) : -1;
}
