// C ABI of libcnfhip.so (see include/cnfhip.h): handle management, parameter upload, the
// RHS entry point, the on-device Tsit5 driver, post-processing, the loss sums and every gradient route of one model.  The
// families built on top of these have files of their own: cnf_abi_ens.hip (ensembles), cnf_abi_jvp.hip (forward mode); what
// they use of this file is declared in cnf_abi_int.h.
#include "cnf_abi_int.h"
#include "cnf_switch.h"
using namespace cnfabi;

#define CNF_ABI_VERSION 1

extern "C" const char* cnf_status_string(cnf_status s) {
    switch (s) {
        case CNF_OK: return "ok";
        case CNF_ERR_BAD_ARG: return "bad argument";
        case CNF_ERR_BAD_SHAPE: return "bad shape";
        case CNF_ERR_HIP: return "HIP runtime error";
        case CNF_ERR_NO_DEVICE: return "no gfx950 device";
        case CNF_ERR_MAXITERS: return "maxiters reached";
        case CNF_ERR_UNSUPPORTED: return "unsupported configuration";
        case CNF_ERR_NO_PARAMS: return "parameters not set";
        case CNF_ERR_NONFINITE: return "non-finite solver state";
        case CNF_ERR_RCCL: return "RCCL error";
    }
    return "unknown status";
}

extern "C" const char* cnf_last_error(cnf_handle h) { return h ? h->err.c_str() : "null handle"; }
extern "C" int cnf_abi_version(void) { return CNF_ABI_VERSION; }
extern "C" int cnf_state_rows(cnf_handle h, int mode) { return h ? rows_of(h, mode) : -1; }

// ---------------------------------------------------------------------------------------
extern "C" cnf_status cnf_create(cnf_handle* out, const cnf_config* cfg) {
    if (!out || !cfg || !cfg->dims || !cfg->acts) return CNF_ERR_BAD_ARG;
    *out = nullptr;
    if (cfg->n_layers < 1 || cfg->n_layers > CNF_MAX_LAYERS) return CNF_ERR_BAD_SHAPE;
    if (cfg->nvars < 1 || cfg->naugs < 0) return CNF_ERR_BAD_SHAPE;
    if (cfg->ad != CNF_AD_VJP && cfg->ad != CNF_AD_JVP) return CNF_ERR_BAD_ARG;
    const int n_in = cfg->nvars + cfg->naugs;
    if (cfg->n_cond < 0) return CNF_ERR_BAD_SHAPE;
    if (cfg->dims[0] != n_in + cfg->n_cond || cfg->dims[cfg->n_layers] != n_in) return CNF_ERR_BAD_SHAPE;
    for (int l = 0; l <= cfg->n_layers; ++l)
        if (cfg->dims[l] < 1 || cfg->dims[l] > 4096) return CNF_ERR_BAD_SHAPE;
    for (int l = 0; l < cfg->n_layers; ++l)
        if (cfg->acts[l] < CNF_ACT_IDENTITY || cfg->acts[l] > CNF_ACT_ELU) return CNF_ERR_BAD_ARG;

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return CNF_ERR_NO_DEVICE;
    if (cfg->device < 0 || cfg->device >= ndev) return CNF_ERR_BAD_ARG;

    cnf_ctx* h = new (std::nothrow) cnf_ctx();
    if (!h) return CNF_ERR_BAD_ARG;
    h->device = cfg->device;
    NetDesc& nd = h->nd;
    nd.n_layers = cfg->n_layers;
    int off = 0, mx = 0, sum = 0;
    for (int l = 0; l <= cfg->n_layers; ++l) {
        nd.dims[l] = l == 0 ? n_in : cfg->dims[l];     // the kernels see the z columns only
        mx = nd.dims[l] > mx ? nd.dims[l] : mx;
        sum += nd.dims[l];
    }
    nd.n_cond = cfg->n_cond;
    for (int l = 0; l < cfg->n_layers; ++l) {
        nd.acts[l] = cfg->acts[l];
        nd.w_off[l] = off;
        if (l == 0) nd.wy_off = off + n_in * nd.dims[1];
        off += cfg->dims[l] * nd.dims[l + 1];          // the flat vector holds every column
        nd.b_off[l] = off;
        off += nd.dims[l + 1];
    }
    h->n_params = (size_t)off;
    nd.n_in = n_in;
    nd.nvars = cfg->nvars;
    nd.naugs = cfg->naugs;
    nd.norm_z = cfg->lambda1 != 0.f;       // src/base_icnf.jl:48
    nd.norm_j = cfg->lambda2 != 0.f;       // src/base_icnf.jl:49
    nd.norm_z_aug = cfg->lambda3 != 0.f;   // src/base_icnf.jl:50
    nd.jvp = cfg->ad == CNF_AD_JVP;
    nd.max_dim = mx;
    nd.sum_dims = sum;
    h->lam[0] = cfg->lambda1; h->lam[1] = cfg->lambda2; h->lam[2] = cfg->lambda3;

    // A ONE-layer tanh network (`Dense(n => n, tanh)`: the network of the reference's benchmark suite, benchmark/benchmarks.jl:29)
    // runs on the two-layer wave kernels as (that layer, identity): W_2 = I and b_2 = 0 are kept behind the parameters.
    h->nd_wave = nd;
    size_t id_tail = 0;
    if (cfg->n_layers == 1 && cfg->acts[0] == CNF_ACT_TANH && n_in <= 16) {
        NetDesc& w = h->nd_wave;
        w.n_layers = 2; w.dims[2] = n_in; w.acts[1] = CNF_ACT_IDENTITY;
        w.w_off[1] = off; w.b_off[1] = off + n_in * n_in;
        w.sum_dims = sum + n_in; w.id2 = 1;
        id_tail = (size_t)n_in * n_in + n_in;
    }
    hipError_t e = hipSetDevice(h->device);
    if (e == hipSuccess) e = (hipError_t)h->d_params.reserve(h->n_params + id_tail);
    if (e == hipSuccess && id_tail) {
        std::vector<float> idm(id_tail, 0.f);
        for (int i = 0; i < n_in; ++i) idm[(size_t)i * n_in + i] = 1.f;
        e = hipMemcpy(h->d_params + h->n_params, idm.data(), id_tail * sizeof(float), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = (hipError_t)h->d_state.reserve(2);
    // (the one-launch solve uses it as 8-byte words: 2 x 1024 of the meetings, 2048 of the loss-sum partials)
    if (e == hipSuccess) e = (hipError_t)h->partials.reserve(8 * MAX_PARTIALS);
    if (e == hipSuccess) e = hipMemset(h->partials, 0, 8 * MAX_PARTIALS * sizeof(float));
    if (e == hipSuccess) e = (hipError_t)h->h_state.reserve(3);
    if (e == hipSuccess) e = (hipError_t)h->d_sums.reserve(SUMS_WORDS);
    if (e == hipSuccess) e = hipMemset(h->d_sums, 0, SUMS_WORDS * sizeof(float));
    if (e == hipSuccess) e = (hipError_t)h->h_sums.reserve(4);
    // (four slots: the streamed solves use slot 0; the one-launch solves take slots 1, 2, 3 in turn, so that up to three
    // submitted launches can be in flight -- and one of them be run again on the streamed driver -- without overwriting
    // each other's final state)
    if (e == hipSuccess) e = (hipError_t)h->h_mirror.reserve(4);
    if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&h->d_mirror, h->h_mirror, 0);
    if (e == hipSuccess) memset(h->h_mirror, 0, 4 * sizeof(cnf_ctx::HostMirror));     // tag 0 is never a launch index (mirror_base starts at 1)
    if (e != hipSuccess) {
        cnf_destroy(h);
        return CNF_ERR_HIP;
    }
    mfma_plan_init(h->mfma, nd);
    *out = h;
    return CNF_OK;
}

// submitted launches still in flight read the handle's buffers: calls that change or free them wait for those launches
// (the submissions stay collectable: their outcome sits in the host mirror)
static void sync_submitted(cnf_handle h) {
    for (const auto& sub : h->submitted)
        if (sub.launched) (void)hipStreamSynchronize(sub.st);
}
// a handle destroyed with submissions outstanding gives up its claim on the process-wide launch order
static void release_submitted(cnf_handle h) {
    std::unique_lock<std::mutex> lock(g_persist_mu);
    for (const auto& sub : h->submitted)
        if (sub.launched) --g_submitted_inflight;
    h->submitted.clear();
}
// Before the parameters or the conditioning of a handle change, every inference submitted on it is brought to its END --
// outcome read, and a launch that ran out of a wait run again on the streamed driver NOW, with the parameters and the
// conditioning it was submitted with -- and stays in the queue as a completed entry for its collect call.
static cnf_status settle_submitted(cnf_handle h);

extern "C" cnf_status cnf_destroy(cnf_handle h) {
    if (!h) return CNF_ERR_BAD_ARG;
    // Called from a finaliser after the HIP runtime has shut down (process exit): nothing may call into HIP to free memory any
    // more, and the buffers free themselves when the handle is destroyed -- so on this path it is NOT destroyed.  The few
    // hundred bytes of host memory go with the process.
    if (hipSetDevice(h->device) != hipSuccess) { (void)hipGetLastError(); return CNF_OK; }
    sync_submitted(h);
    release_submitted(h);
    mfma_plan_free(h->mfma);
    delete h;
    return CNF_OK;
}

// what every parameter upload begins and ends with, around its own copy into d_params
static cnf_status params_check(cnf_handle h, const float* flat, size_t n) {
    if (!h || !flat) return CNF_ERR_BAD_ARG;
    if (n != h->n_params) return fail(h, CNF_ERR_BAD_SHAPE, "parameter count does not match the layer sizes");
    HIPCHK(h, hipSetDevice(h->device));
    return CNF_OK;
}
enum ParamsWait { PARAMS_NO_WAIT, PARAMS_WAIT_STREAM, PARAMS_WAIT_DEVICE };
static cnf_status params_uploaded(cnf_handle h, hipStream_t s, ParamsWait wait) {
    cnf_status ms = mfma_plan_pack(h->mfma, h->nd, h->d_params, s);
    if (ms != CNF_OK) return fail(h, ms, "MFMA weight packing failed");
    if (wait == PARAMS_WAIT_STREAM) HIPCHK(h, hipStreamSynchronize(s));
    if (wait == PARAMS_WAIT_DEVICE) HIPCHK(h, hipDeviceSynchronize());
    h->have_params = true;
    h->rec.end();
    h->pt_valid = false;
    h->img_valid = false;
    h->bimg_valid = false;
    h->cond_B = 0;       // the conditioning bias depends on W1 and b1
    return CNF_OK;
}

extern "C" cnf_status cnf_set_params(cnf_handle h, const float* flat_dev, size_t n, void* stream) {
    cnf_status ss = params_check(h, flat_dev, n);
    if (ss != CNF_OK || (ss = settle_submitted(h)) != CNF_OK) return ss;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(h, hipMemcpyAsync(h->d_params, flat_dev, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    return params_uploaded(h, s, PARAMS_WAIT_STREAM);
}

extern "C" cnf_status cnf_set_params_host(cnf_handle h, const float* flat, size_t n) {
    cnf_status ss = params_check(h, flat, n);
    if (ss != CNF_OK || (ss = settle_submitted(h)) != CNF_OK) return ss;
    HIPCHK(h, hipMemcpy(h->d_params, flat, n * sizeof(float), hipMemcpyHostToDevice));
    return params_uploaded(h, nullptr, PARAMS_WAIT_DEVICE);
}

// ---------------------------------------------------------------------------------------
static cnf_status ensure_capacity(cnf_handle h, int B) {
    if ((size_t)B <= h->cap_B) return CNF_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());
    const size_t want = ((size_t)B + 255) & ~(size_t)255;
    const size_t Dmax = (size_t)h->nd.n_in + 3;
    const size_t ws_1 = (size_t)2 * h->nd.sum_dims + (size_t)2 * h->nd.max_dim;       // floats per sample
    const hipError_t arena_alloc = (hipError_t)h->arena.reserve((ws_1 + 9 * Dmax + 4) * want + want / 16);
    // The pointers below exist only while the arena does: a failed reserve has left it empty, and they are all carved from
    // null with no capacity (every offset is 0) before the error is returned.
    const size_t cap = arena_alloc == hipSuccess ? want : 0;
    const size_t st_f = Dmax * cap;
    float* p = h->arena;
    h->ws = p; p += ws_1 * cap;
    for (int i = 0; i < 2; ++i) { h->U[i] = p; p += st_f; }
    for (int i = 0; i < 2; ++i) { h->K1[i] = p; p += st_f; }
    for (int i = 0; i < 5; ++i) { h->Ks[i] = p; p += st_f; }
    h->tmp_logpx = p; p += cap;
    h->tmp_regs = p; p += 3 * cap;
    h->post_part = p; p += cap / 16;
    h->cap_B = cap;
    HIPCHK(h, arena_alloc);
    return CNF_OK;
}

// staging area for host-pointer calls: at least `nfloats` floats of device memory owned by the handle
static cnf_status ensure_stage(cnf_handle h, size_t nfloats) {
    if (nfloats <= h->stage.capacity()) return CNF_OK;
    HIPCHK(h, hipDeviceSynchronize());
    RESERVE(h, h->stage, (nfloats + 4095) & ~(size_t)4095);
    return CNF_OK;
}

static cnf_status check_call(cnf_handle h, int mode, int B) {
    if (!h) return CNF_ERR_BAD_ARG;
    if (mode != CNF_MODE_TEST && mode != CNF_MODE_TRAIN) return fail(h, CNF_ERR_BAD_ARG, "unknown mode");
    if (B < 0) return fail(h, CNF_ERR_BAD_SHAPE, "negative batch");
    if (!h->have_params) return fail(h, CNF_ERR_NO_PARAMS, "cnf_set_params has not been called");
    if (h->nd.n_cond > 0 && B > 0 && h->cond_B != B)
        return fail(h, CNF_ERR_NO_PARAMS, "conditional model: call cnf_set_cond with the ys of this batch first");
    h->mfma.cond = h->nd.n_cond > 0 ? h->d_cond : nullptr;
    h->mfma.cbs = h->cbs;
    // any other call on the handle first completes the inferences submitted on it (their statistics are dropped)
    while (!h->collecting && !h->submitted.empty()) {
        const cnf_status s = collect_one(h, nullptr);
        if (s != CNF_OK) return s;
    }
    return CNF_OK;
}

// basedist of construct (src/base_icnf.jl:16-21).  The arrays are checked and copied here; prec = W' W is formed in double from
// the float W given (so it is the derivative of the log-density the device evaluates) and rounded once.
extern "C" cnf_status cnf_set_basedist(cnf_handle h, int kind, const float* mean, const float* whiten, const float* chol,
                                       float logconst) {
    if (!h) return CNF_ERR_BAD_ARG;
    if (kind < 0 || kind > 2) return fail(h, CNF_ERR_BAD_ARG, "basedist kind must be 0 (default), 1 (diagonal) or 2 (dense)");
    if (hipSetDevice(h->device) != hipSuccess) { (void)hipGetLastError(); return fail(h, CNF_ERR_NO_DEVICE, "no device"); }
    const size_t n = (size_t)h->nd.n_in, m = kind == 2 ? n * n : n;
    std::vector<float> host;
    if (kind != 0) {
        if (!mean || !whiten || !chol) return fail(h, CNF_ERR_BAD_ARG, "null pointer");
        if (!std::isfinite(logconst)) return fail(h, CNF_ERR_BAD_ARG, "logconst is not finite");
        for (size_t i = 0; i < n; ++i)
            if (!std::isfinite(mean[i])) return fail(h, CNF_ERR_BAD_ARG, "basedist: non-finite mean");
        host.assign(n + 3 * m, 0.f);
        float *hm = host.data(), *hw = hm + n, *hl = hw + m, *hp = hl + m;
        for (size_t i = 0; i < n; ++i) hm[i] = mean[i];
        for (size_t i = 0; i < n; ++i) {
            const size_t d = kind == 2 ? i * n + i : i;
            if (!std::isfinite(whiten[d]) || !(whiten[d] > 0.f) || !std::isfinite(chol[d]) || !(chol[d] > 0.f))
                return fail(h, CNF_ERR_BAD_ARG, "basedist: the diagonals of whiten and chol must be finite and > 0");
            for (size_t j = 0; kind == 2 && j < i; ++j)
                if (!std::isfinite(whiten[i * n + j]) || !std::isfinite(chol[i * n + j]))
                    return fail(h, CNF_ERR_BAD_ARG, "basedist: non-finite entry");
        }
        if (kind == 1) {
            for (size_t i = 0; i < n; ++i) { hw[i] = whiten[i]; hl[i] = chol[i]; hp[i] = (float)((double)whiten[i] * whiten[i]); }
        } else {
            for (size_t i = 0; i < n; ++i)
                for (size_t j = 0; j <= i; ++j) { hw[i * n + j] = whiten[i * n + j]; hl[i * n + j] = chol[i * n + j]; }
            for (size_t i = 0; i < n; ++i)
                for (size_t j = 0; j <= i; ++j) {
                    double acc = 0.0;
                    for (size_t k = i; k < n; ++k) acc += (double)hw[k * n + i] * hw[k * n + j];      // (W' W)_ij, k >= max(i, j)
                    hp[i * n + j] = hp[j * n + i] = (float)acc;
                }
        }
    }
    // (a submitted inference, or its fallback, evaluates the base it was submitted with: none may be outstanding)
    { const cnf_status ss = settle_submitted(h); if (ss != CNF_OK) return ss; }
    HIPCHK(h, hipDeviceSynchronize());
    h->d_bd.release();
    h->bd = BaseDist{};
    h->rec.end();
    if (kind == 0) return CNF_OK;
    RESERVE(h, h->d_bd, host.size());
    HIPCHK(h, hipMemcpy(h->d_bd, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    h->bd.kind = kind; h->bd.mean = h->d_bd; h->bd.whiten = h->d_bd + n; h->bd.chol = h->d_bd + n + m; h->bd.prec = h->d_bd + n + 2 * m;
    h->bd.logconst = logconst;
    return CNF_OK;
}

extern "C" cnf_status cnf_base_sample(cnf_handle h, const float* normals, float* z0, int B, void* stream) {
    if (!h || !normals || !z0) return CNF_ERR_BAD_ARG;
    if (B < 0) return fail(h, CNF_ERR_BAD_SHAPE, "negative batch");
    if (normals == z0) return fail(h, CNF_ERR_BAD_ARG, "normals and z0 must be distinct buffers");
    if (B == 0) return CNF_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t n = (size_t)h->nd.n_in * B;
    if (h->bd.kind == 0) HIPCHK(h, hipMemcpyAsync(z0, normals, n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    else launch_base_sample(h->nd.n_in, h->bd, normals, z0, B, (hipStream_t)stream);
    HIPCHK(h, hipGetLastError());
    return CNF_OK;
}

extern "C" cnf_status cnf_set_cond(cnf_handle h, const float* ys, int B, void* stream) {
    if (!h) return CNF_ERR_BAD_ARG;
    if (h->nd.n_cond == 0) return fail(h, CNF_ERR_BAD_ARG, "not a conditional model (n_cond == 0)");
    if (!h->have_params) return fail(h, CNF_ERR_NO_PARAMS, "cnf_set_params has not been called");
    if (!ys || B < 1) return fail(h, CNF_ERR_BAD_ARG, "ys must be n_cond x B with B >= 1");
    HIPCHK(h, hipSetDevice(h->device));
    // (a submitted inference reads d_cond until it ends, and its fallback would read it again: none may be outstanding)
    { const cnf_status ss = settle_submitted(h); if (ss != CNF_OK) return ss; }
    h->rec.end();
    const int cbs = (h->nd.dims[1] + 15) & ~15;
    if (h->cond_B != B || h->cbs != cbs) {
        HIPCHK(h, hipDeviceSynchronize());
        h->d_cond.release();             // (sized for this batch exactly, a smaller one too)
        h->d_ys.release();
        h->cond_B = 0;
        RESERVE(h, h->d_cond, (size_t)B * cbs);
        RESERVE(h, h->d_ys, (size_t)B * h->nd.n_cond);
        h->cbs = cbs;
    }
    // the gradient path needs ys itself (d loss / d W1[:, n_in:] = sum_b abar_1 ys')
    HIPCHK(h, hipMemcpyAsync(h->d_ys, ys, (size_t)B * h->nd.n_cond * sizeof(float), hipMemcpyDeviceToDevice,
                             (hipStream_t)stream));
    launch_cond_bias(h->nd, h->d_params, ys, h->d_cond, cbs, B, (hipStream_t)stream);
    HIPCHK(h, hipGetLastError());
    h->cond_B = B;
    return CNF_OK;
}

extern "C" cnf_status cnf_set_cond_host(cnf_handle h, const float* ys, int B) {
    if (!h) return CNF_ERR_BAD_ARG;
    if (!ys || B < 1 || h->nd.n_cond == 0) return fail(h, CNF_ERR_BAD_ARG, "bad conditioning input");
    HIPCHK(h, hipSetDevice(h->device));
    cnf_status s = ensure_stage(h, (size_t)B * h->nd.n_cond);
    if (s != CNF_OK) return s;
    float* d = h->stage;
    HIPCHK(h, hipMemcpy(d, ys, (size_t)B * h->nd.n_cond * sizeof(float), hipMemcpyHostToDevice));
    s = cnf_set_cond(h, d, B, nullptr);
    hipError_t e = hipDeviceSynchronize();      // cnf_set_cond keeps its own copy of ys: the staging area is free again
    if (s == CNF_OK && e != hipSuccess) s = fail(h, CNF_ERR_HIP, hipGetErrorString(e));
    return s;
}

static bool trace_ok(cnf_handle h) {
    const GradLayout g = grad_layout(h->nd);
    return trace_mfma_supported(h->nd, adj_mfma_layout(h->nd, g));
}
// TrainMode with the JVP compute mode on a network the fused step kernel cannot hold
static bool jvp_aux_ok(cnf_handle h) {
    const GradLayout g = grad_layout(h->nd);
    return jvp_mfma_supported(h->nd, adj_mfma_layout(h->nd, g));
}
extern "C" int cnf_kernel_for(cnf_handle h, int mode, int B) {
    if (!h) return -1;
    if (mfma_supported(h->mfma, h->nd, mode == CNF_MODE_TRAIN, B)) return CNF_KERNEL_MFMA;
    if (mode == CNF_MODE_TRAIN) return jvp_aux_ok(h) ? CNF_KERNEL_MFMA : CNF_KERNEL_GENERIC;
    return trace_ok(h) ? CNF_KERNEL_MFMA : CNF_KERNEL_GENERIC;
}

// padded forward/reverse weight images shared by the pullback and the exact-trace kernels: allocated on first use ...
static cnf_status reserve_adj_images(cnf_handle h) {
    RESERVE(h, h->d_adj_img, (size_t)adj_mfma_layout(h->nd, grad_layout(h->nd)).img_floats);
    return CNF_OK;
}
// ... and packed on first use after a parameter change
static cnf_status ensure_adj_images(cnf_handle h, hipStream_t st) {
    const GradLayout g = grad_layout(h->nd);
    const AdjMfmaLayout m = adj_mfma_layout(h->nd, g);
    { const cnf_status rs = reserve_adj_images(h); if (rs != CNF_OK) return rs; }
    if (!h->img_valid) {
        HIPCHK(h, launch_pack_adj_images(h->nd, g, m, h->d_params, h->d_adj_img, st));
        h->img_valid = true;
    }
    return CNF_OK;
}

// one evaluation with an auxiliary MFMA kernel (TestMode: exact trace; TrainMode: JVP): u -> du (or k7)
// nk > 0 (inside a solve): the kernel forms the Runge-Kutta stage state from nk stage derivatives itself (and, for
// stage 6, stores it as the new solution); otherwise it evaluates at `u`
namespace {
struct TraceFuse {          // norms / controller / the whole attempt inside the trace launch (k_trace3s; see TraceArgs)
    int norm_kind = -1;     // 0 / 1: norms of the automatic initial dt; 2: the error norm of an attempt
    bool step = false;      // the six stage evaluations of an attempt in one launch
    void* mirror = nullptr;
    unsigned seq = 0;
};
// how a call evaluates through an auxiliary MFMA kernel behind the generic driver (on: it does)
struct AuxEval {
    bool on = false;
    bool train = false;           // false: TestMode exact trace; true: TrainMode JVP
    const float* eps = nullptr;
};
}  // namespace
static bool trace_fused_ok(cnf_handle h, const AuxEval& aux, int B) {
    const GradLayout g = grad_layout(h->nd);
    return !aux.train && trace_fused_supported(h->nd, adj_mfma_layout(h->nd, g), B);
}
static cnf_status launch_trace(cnf_handle h, const AuxEval& aux, const float* u, float* du, bool in_solve, bool du_is_k7, int B, hipStream_t st,
                               int nk = 0, const float* coef = nullptr, bool also_unew = false, const TraceFuse* fuse = nullptr) {
    const GradLayout g = grad_layout(h->nd);
    const AdjMfmaLayout m = adj_mfma_layout(h->nd, g);
    TraceArgs a{};
    a.u = u; a.du = du; a.ys = h->nd.n_cond > 0 ? h->d_ys : nullptr;
    a.st = in_solve ? h->d_state.data() : nullptr;
    set_rk_buffers(h, a);
    a.du_is_k7 = du_is_k7 ? 1 : 0;
    a.B = B;
    a.nk = in_solve ? nk : 0;
    for (int i = 0; i < a.nk && i < 6; ++i) a.coef[i] = coef[i];
    a.also_unew = also_unew ? 1 : 0;
    a.norm_kind = -1;
    if (fuse) {
        a.norm_kind = fuse->norm_kind; a.fused_step = fuse->step ? 1 : 0;
        a.partials = h->partials; a.ticket = sums_word<unsigned>(h, SUMS_NORM_TICKET); a.st_mut = h->d_state;
        a.n_total = (float)((size_t)rows_of(h, CNF_MODE_TEST) * B);
        a.mirror = fuse->mirror; a.seq = fuse->seq;
    }
    if (aux.train && h->nd.jvp) HIPCHK(h, launch_jvp_mfma(h->nd, g, m, h->d_adj_img, a, aux.eps, st));
    else HIPCHK(h, launch_trace_mfma(h->nd, g, m, h->d_adj_img, a, st));
    return CNF_OK;
}

static cnf_status resolve_kernel(cnf_handle h, int mode, int B, int requested, int* out) {
    const bool ok = mfma_supported(h->mfma, h->nd, mode == CNF_MODE_TRAIN, B) ||
                    (mode == CNF_MODE_TEST && trace_ok(h)) || (mode == CNF_MODE_TRAIN && jvp_aux_ok(h));
    if (requested == CNF_KERNEL_AUTO) { *out = ok ? CNF_KERNEL_MFMA : CNF_KERNEL_GENERIC; return CNF_OK; }
    if (requested == CNF_KERNEL_GENERIC) { *out = CNF_KERNEL_GENERIC; return CNF_OK; }
    if (requested == CNF_KERNEL_MFMA) {
        if (!ok) return fail(h, CNF_ERR_UNSUPPORTED, "the MFMA path has no kernel for this network/mode");
        *out = CNF_KERNEL_MFMA;
        return CNF_OK;
    }
    return fail(h, CNF_ERR_BAD_ARG, "unknown kernel selector");
}

extern "C" cnf_status cnf_solve_kernel_time(cnf_handle h, int enable, float* mean_us, int* launches) {
    if (!h) return CNF_ERR_BAD_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());
    unsigned long long w[3] = {0, 0, 0};
    HIPCHK(h, hipMemcpy(w, sums_word<void>(h, SUMS_CLOCK), sizeof w, hipMemcpyDeviceToHost));
    if (mean_us) *mean_us = w[2] ? (float)((double)w[1] * 0.01 / (double)w[2]) : 0.f;       // s_memrealtime: 100 MHz
    if (launches) *launches = (int)w[2];
    HIPCHK(h, hipMemset(sums_word<void>(h, SUMS_CLOCK), 0, sizeof w));
    h->time_kernel = enable != 0;
    return CNF_OK;
}

extern "C" cnf_status cnf_set_step_trace(cnf_handle h, float* trace_dev, int cap_attempts) {
    if (!h || cap_attempts < 0 || (cap_attempts > 0 && !trace_dev)) return CNF_ERR_BAD_ARG;
    h->step_trace = cap_attempts > 0 ? trace_dev : nullptr;
    h->step_trace_cap = cap_attempts;
    return CNF_OK;
}

extern "C" cnf_status cnf_selftest_split_product(const float* A, const float* Bt, float* C, int K) {
    if (!A || !Bt || !C || K < 32 || K % 32 != 0 || K > 4096) return CNF_ERR_BAD_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return CNF_ERR_NO_DEVICE;
    float* d = nullptr;
    const size_t na = (size_t)16 * K;
    if (hipMalloc(&d, (2 * na + 256) * sizeof(float)) != hipSuccess) return CNF_ERR_HIP;
    hipError_t e = hipMemcpy(d, A, na * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + na, Bt, na * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = split_product_test_launch(d, d + na, d + 2 * na, K, nullptr);
    if (e == hipSuccess) e = hipMemcpy(C, d + 2 * na, 256 * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    return e == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}

// test support: workgroups that hold a CU each (all of its LDS) for a bounded time
__global__ void __launch_bounds__(64) k_hold_cu(unsigned long long ticks) {
    extern __shared__ char hold_lds[];
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
    if (threadIdx.x == 0) hold_lds[0] = 1;
}
extern "C" cnf_status cnf_selftest_hold_cus(int n_workgroups, int microseconds, void* stream) {
    if (n_workgroups < 1 || n_workgroups > 4096 || microseconds < 1 || microseconds > 100000) return CNF_ERR_BAD_ARG;
    constexpr int LDS = 160 * 1024;
    if (hipFuncSetAttribute((const void*)k_hold_cu, hipFuncAttributeMaxDynamicSharedMemorySize, LDS) != hipSuccess) return CNF_ERR_HIP;
    hipLaunchKernelGGL(k_hold_cu, dim3(n_workgroups), dim3(64), LDS, (hipStream_t)stream, 100ull * (unsigned long long)microseconds);
    return hipGetLastError() == hipSuccess ? CNF_OK : CNF_ERR_HIP;
}
extern "C" int cnf_solve_fallbacks(cnf_handle h) { return h ? h->fallbacks : -1; }
extern "C" int cnf_set_grad_split(int mode) {
    const int was = adj_split_mode();
    set_adj_split_mode(mode);
    return was;
}

extern "C" cnf_status cnf_set_solve_wait(cnf_handle h, int wait_us, int poll_limit) {
    if (!h) return CNF_ERR_BAD_ARG;
    if (wait_us > 0) h->wait_us = wait_us;
    if (poll_limit > 0) h->poll_limit = poll_limit;
    return CNF_OK;
}

extern "C" cnf_status cnf_rhs_work(cnf_handle h, int mode, int B, double* flops, double* bytes) {
    if (!h || !flops || !bytes) return CNF_ERR_BAD_ARG;
    const NetDesc& nd = h->nd;
    double M = 0, P = 0;
    for (int l = 0; l < nd.n_layers; ++l) {
        M += (double)nd.dims[l] * nd.dims[l + 1];
        P += (double)nd.dims[l] * nd.dims[l + 1] + nd.dims[l + 1];
    }
    const double n_in = nd.n_in, D = rows_of(h, mode);
    if (mode == CNF_MODE_TRAIN) {
        *flops = B * (4.0 * M + 6.0 * n_in);
        *bytes = 4.0 * B * (n_in + n_in + D) + 4.0 * P;
    } else {
        // exact trace: minimal formulation for 2-layer nets, tr J = d1^T (W1 .* W2^T) d2 = forward
        // + one h x n_in product (B*3M); otherwise forward + n_in tangent sweeps
        if (nd.n_layers == 2) *flops = B * 3.0 * M;
        else *flops = B * (2.0 * M + n_in * 2.0 * M);
        *bytes = 4.0 * B * (n_in + D) + 4.0 * P;
    }
    return CNF_OK;
}

// ---------------------------------------------------------------------------------------
// RHS (a1/a2/a3)
// ---------------------------------------------------------------------------------------
extern "C" cnf_status cnf_rhs(cnf_handle h, int mode, int kernel, const float* u,
                              const float* eps, float* du, int B, void* stream) {
    cnf_status s = check_call(h, mode, B);
    if (s != CNF_OK) return s;
    if (!u || !du) return fail(h, CNF_ERR_BAD_ARG, "null state pointer");
    if (u == du) return fail(h, CNF_ERR_BAD_ARG, "u and du must not alias");
    if (mode == CNF_MODE_TRAIN && !eps) return fail(h, CNF_ERR_BAD_ARG, "eps is required in TrainMode");
    if (B == 0) return CNF_OK;
    int k;
    if ((s = resolve_kernel(h, mode, B, kernel, &k)) != CNF_OK) return s;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    if (k == CNF_KERNEL_MFMA && !mfma_supported(h->mfma, h->nd, mode == CNF_MODE_TRAIN, B)) {
        // TestMode, three or more layers: exact trace on MFMA; TrainMode/JVP beyond LDS (cnf_trace.hip)
        if ((s = ensure_adj_images(h, st)) != CNF_OK) return s;
        const AuxEval aux{true, mode == CNF_MODE_TRAIN, eps};
        if ((s = launch_trace(h, aux, u, du, false, false, B, st)) != CNF_OK) return s;
    } else if (k == CNF_KERNEL_MFMA) {
        s = mfma_rhs(h->mfma, h->nd, mode == CNF_MODE_TRAIN, u, eps, du, B, st);
        if (s != CNF_OK) return fail(h, s, "MFMA RHS launch failed");
    } else {
        if ((s = ensure_capacity(h, B)) != CNF_OK) return s;
        RhsArgs a{};
        a.st = nullptr; a.B = B; a.S = h->cap_B; a.train = mode == CNF_MODE_TRAIN;
        a.ws = h->ws; a.eps = eps; a.u = u; a.du = du; a.nk = 0;
        a.cond = h->mfma.cond; a.cbs = h->cbs;
        launch_rhs_generic(h->nd, h->d_params, a, st);
    }
    HIPCHK(h, hipGetLastError());
    return CNF_OK;
}

extern "C" cnf_status cnf_rhs_host(cnf_handle h, int mode, int kernel, const float* u,
                                   const float* eps, float* du, int B) {
    cnf_status s = check_call(h, mode, B);
    if (s != CNF_OK) return s;
    if (!u || !du) return fail(h, CNF_ERR_BAD_ARG, "null state pointer");
    if (B == 0) return CNF_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t D = rows_of(h, mode), n_in = h->nd.n_in;
    if ((s = ensure_stage(h, (2 * D + n_in) * B)) != CNF_OK) return s;
    float* u_d = h->stage;
    float* du_d = u_d + D * B;
    float* e_d = eps ? du_d + D * B : nullptr;
    HIPCHK(h, hipMemcpy(u_d, u, D * B * sizeof(float), hipMemcpyHostToDevice));
    if (eps) HIPCHK(h, hipMemcpy(e_d, eps, n_in * B * sizeof(float), hipMemcpyHostToDevice));
    s = cnf_rhs(h, mode, kernel, u_d, e_d, du_d, B, nullptr);
    if (s == CNF_OK) {
        hipError_t e = hipMemcpy(du, du_d, D * B * sizeof(float), hipMemcpyDeviceToHost);
        if (e != hipSuccess) s = fail(h, CNF_ERR_HIP, hipGetErrorString(e));
    }
    return s;
}

// ---------------------------------------------------------------------------------------
// Tsit5 driver (a7: base_sol, src/base_icnf.jl:137-143)
// ---------------------------------------------------------------------------------------
static int enqueue_attempt_generic(cnf_handle h, const AuxEval& aux, int train, const float* eps, int B,
                                    int nblk, hipStream_t s, bool with_controller = true,
                                    float* dump = nullptr, size_t dump_stride = 0, void* mirror = nullptr,
                                    unsigned seq = 0) {
    RhsArgs a{};
    a.st = h->d_state; a.B = B; a.S = h->cap_B; a.train = train; a.ws = h->ws; a.eps = eps;
    a.cond = h->mfma.cond; a.cbs = h->cbs;
    set_rk_buffers(h, a);
    if (aux.on && with_controller && !dump && trace_fused_ok(h, aux, B)) {
        // TestMode on the 32-128-128-32 shape: the six stage evaluations, the error norm and the controller in ONE launch
        TraceFuse f; f.norm_kind = 2; f.step = true; f.mirror = mirror; f.seq = seq;
        (void)launch_trace(h, aux, nullptr, nullptr, true, false, B, s, 0, nullptr, false, &f);
        return 1;
    }
    for (int stage = 1; stage <= 6 && aux.on; ++stage) {     // the auxiliary kernel forms its stage state itself
        float coef[6];
        tsit5_row(stage, coef);
        (void)launch_trace(h, aux, nullptr, stage < 6 ? h->Ks[stage - 1] : nullptr, true, stage == 6, B, s, stage, coef, stage == 6);
    }
    for (int stage = 1; stage <= 6 && !aux.on; ++stage) {      // computes k_{stage+1}
        a.nk = stage;
        tsit5_row(stage, a.coef);
        a.ustage = (dump && stage < 6) ? dump + (size_t)(stage - 1) * dump_stride : nullptr;   // stage states 2..6
        a.ustage_is_unew = stage == 6;
        a.du_is_k7 = stage == 6;
        a.du = stage < 6 ? h->Ks[stage - 1] : nullptr;
        launch_rhs_generic(h->nd, h->d_params, a, s);
    }
    NormArgs n{};
    n.st = h->d_state; n.kind = 2; n.n = (size_t)rows_of(h, train) * B;
    set_rk_buffers(h, n);
    n.partials = h->partials;
    if (with_controller) {      // error norm + controller in one launch
        n.ticket = sums_word<unsigned>(h, SUMS_NORM_TICKET); n.st_mut = h->d_state; n.ctrl_phase = 2; n.n_total = (float)n.n;
        n.mirror = mirror; n.seq = seq;
    }
    launch_norm_partials(n, nblk, s);
    return 7;                            // six stage evaluations + the error norm (with the controller)
}

extern "C" cnf_status cnf_set_shard_reduce(cnf_handle h, cnf_shard_reduce_fn fn, void* user) {
    if (!h) return CNF_ERR_BAD_ARG;
    h->shard_reduce = fn;
    h->shard_user = user;
    return CNF_OK;
}

// Lock-step controller: local partial sums -> (p0, p1, n_local) -> host -> sum over the shards ->
// back to the device -> controller on the global sums.  One stream synchronisation per call.
static cnf_status lockstep_controller(cnf_handle h, StepState* state, const float* partials, int phase,
                                      float n_local, hipStream_t st) {
    launch_reduce_partials(state, partials, h->d_sums, n_local, st);
    if (h->shard_comm) {                 // RCCL: the three floats never leave the device
        if (cnf_comm_allreduce(h->shard_comm, h->d_sums, 3, st) != CNF_OK) return fail(h, CNF_ERR_RCCL, cnf_comm_last_error());
        launch_controller_sums(state, h->d_sums, phase, st);
        return CNF_OK;
    }
    HIPCHK(h, hipMemcpyAsync(h->h_sums, h->d_sums, 3 * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    if (h->shard_reduce(h->h_sums, 3, h->shard_user) != 0)
        return fail(h, CNF_ERR_BAD_ARG, "shard_reduce callback reported failure");
    HIPCHK(h, hipMemcpyAsync(h->d_sums, h->h_sums, 3 * sizeof(float), hipMemcpyHostToDevice, st));
    launch_controller_sums(state, h->d_sums, phase, st);
    return CNF_OK;
}

static size_t traj_slot_floats(cnf_handle h) { return 6 * ((size_t)h->nd.n_in + 3) * h->grad_cap_B; }
// make room for `steps` slots (contiguous: the step kernel indexes it by the accepted-step counter)
static cnf_status traj_reserve(cnf_handle h, int steps) {
    if (steps <= h->traj_cap) return CNF_OK;
    int cap = h->traj_cap ? h->traj_cap : 32;
    while (cap < steps) cap *= 2;
    const size_t slot = traj_slot_floats(h);
    // grown with its contents kept: new buffers, copy, swap -- the old ones (or, on an error, the new ones) go with nt / nh
    DevBuf<float> nt, nh;
    HIPCHK(h, hipDeviceSynchronize());
    RESERVE(h, nt, slot * cap);
    if (nh.reserve((size_t)cap) != 0) return fail(h, CNF_ERR_HIP, "hipMalloc of the trajectory step-size array failed");
    if (h->traj) {
        HIPCHK(h, hipMemcpy(nt, h->traj, slot * h->traj_cap * sizeof(float), hipMemcpyDeviceToDevice));
        HIPCHK(h, hipMemcpy(nh, h->traj_hs, (size_t)h->traj_cap * sizeof(float), hipMemcpyDeviceToDevice));
    }
    h->traj.swap(nt); h->traj_hs.swap(nh); h->traj_cap = cap;
    return CNF_OK;
}
static cnf_status traj_slot(cnf_handle h, int n, float** out) {
    cnf_status s = traj_reserve(h, n + 1);
    if (s != CNF_OK) return s;
    *out = h->traj + (size_t)n * traj_slot_floats(h);
    return CNF_OK;
}

static void enqueue_post(cnf_handle h, int train, const StepState* state, const PostHook& ph, int B, bool need_done,
                         hipStream_t st) {
    launch_post_state(h->nd, train, state, h->U[0], h->U[1], ph.logpx, ph.regs, B, st, need_done, ph.sums5, h->post_part,
                      sums_word<unsigned>(h, SUMS_POST_TICKET));
}
namespace {
// The path of a bare solve (cnf_solve_path): the caller's save times and where their slices go.  In the launch of the wave
// kernel where it has a PATH form; else one attempt at a time on the per-stage kernels, k_dense_out behind every accepted step.
struct PathHook {
    const float* saveat;           // host, [K]: checked by the caller (finite, monotone along the span, inside it)
    int K;
    float* out;                    // device, [K][B][D]
};
// What a caller asks of solve_core: the solve itself, then the hooks (at most one of rec / path / jvp) and whether the call
// waits for the stream before it returns
struct SolveCall {
    int mode, B;
    const float *u0, *eps;
    float* u_out;                  // may be null: the state stays in U[cur]
    const cnf_solve_opts* opts;
    cnf_solve_stats* stats;
    void* stream;
    Recorder* rec = nullptr; PostHook* post = nullptr; PathHook* path = nullptr; JvpCall* jvp = nullptr;
    bool final_sync = true;
};
}  // namespace

// One-launch solves of this process: one at a time (two would each hold CUs the other is waiting for), except that
// submitted launches may queue up behind each other on ONE stream.
std::mutex cnfabi::g_persist_mu;
int cnfabi::g_submitted_inflight = 0;               // (both under g_persist_mu)
hipStream_t cnfabi::g_submitted_stream = nullptr;

// Wait for a consistent snapshot of the mirror slot `hm` whose tag is news (`fresh(tag)`): *snap / *sq.  The spin backs off:
// pause first, yield the core once the wait outlasts a few launches.  A faulted kernel would never publish: every 100000
// spins the stream is asked -- an error is the call's, an idle stream without the snapshot is `unpublished`, an idle stream
// with it ends the wait.
template <class Fresh>
static cnf_status mirror_wait(cnf_handle h, const volatile cnf_ctx::HostMirror* hm, hipStream_t st, StepState* snap, unsigned* sq,
                              Fresh fresh, const char* unpublished) {
    for (long spins = 0;; ++spins) {
        if (cnf_mirror_read(hm, snap, sq) && fresh(*sq)) return CNF_OK;
        if (spins < 4096) _mm_pause();
        else sched_yield();
        if (spins % 100000 == 99999) {
            hipError_t qe = hipStreamQuery(st);
            if (qe != hipSuccess && qe != hipErrorNotReady) HIPCHK(h, qe);
            if (qe == hipSuccess) return cnf_mirror_read(hm, snap, sq) && fresh(*sq) ? CNF_OK : fail(h, CNF_ERR_HIP, unpublished);
        }
    }
}

// the statistics of a solve that ended in the state `fin`
void cnfabi::fill_stats(cnf_solve_stats* stats, const StepState& fin, int nf, int kernel_used, int launches) {
    if (!stats) return;
    stats->nf = nf;
    stats->naccept = fin.naccept;
    stats->nreject = fin.nreject;
    stats->t_final = fin.t;
    stats->dt_last = fin.dt;
    stats->kernel_used = kernel_used;
    stats->launches = launches;
}

// The outcome of the one-launch solve with launch index `seq`: its final state arrives in its slot of the host mirror.
// *aborted: a wait inside the kernel ran out (the state says so itself: n_partials < 0) -- nothing of the launch is used,
// the abort word is cleared (after the stream has drained: launches queued behind it read it too) and the caller runs
// the solve again on the streamed driver.
static cnf_status finish_one_launch(cnf_handle h, unsigned seq, int slot, hipStream_t st, StepState* fin, bool* aborted) {
    unsigned sq = 0;
    const cnf_status ws = mirror_wait(h, h->h_mirror + slot, st, fin, &sq, [seq](unsigned tag) { return tag == seq; },
                                      "the solve kernel finished without publishing a state");
    if (ws != CNF_OK) return ws;
    *aborted = fin->n_partials < 0;
    if (*aborted) {
        // A workgroup dispatched late may have run after workgroup 0 advanced the index base and left words tagged with
        // the NEXT launch's first meeting: with the stream drained, the meeting words are cleared along with the abort word.
        HIPCHK(h, hipStreamSynchronize(st));
        HIPCHK(h, hipMemset(h->partials, 0, 8 * MAX_PARTIALS * sizeof(float)));
        HIPCHK(h, hipMemset(sums_word<int>(h, SUMS_ABORT), 0, sizeof(int)));
    } else if (!fin->done && !fin->nonfinite) return fail(h, CNF_ERR_MAXITERS, "maxiters reached before t1");
    return CNF_OK;
}

// the bounds of a wait inside a one-launch solve of this handle (cnf_set_solve_wait; CNF_SOLVE_WAIT_US, CNF_SOLVE_POLL_LIMIT)
void cnfabi::set_wait_bounds(cnf_handle h, Solve3Args& sv) {
    sv.spin_limit = h->poll_limit > 0 ? h->poll_limit : cnf_switch<SW_SOLVE_POLL_LIMIT>();
    const int wus = h->wait_us > 0 ? h->wait_us : cnf_switch<SW_SOLVE_WAIT_US>();
    sv.wait_ticks = wus < 20000000 ? 100u * (unsigned)wus : 2000000000u;   // (per tile: the launcher scales it)
}
// what every solve asks of its options
cnf_status cnfabi::check_solve_opts(cnf_handle h, const cnf_solve_opts* opts) {
    if (!(opts->t0 == opts->t0) || !(opts->t1 == opts->t1) || opts->t0 == opts->t1)
        return fail(h, CNF_ERR_BAD_ARG, "empty or NaN time span");
    if (!opts->adaptive && !(opts->dt > 0.f)) return fail(h, CNF_ERR_BAD_ARG, "fixed stepping needs dt > 0");
    if (opts->adaptive && (!(opts->abstol >= 0.f) || !(opts->reltol >= 0.f) || (opts->abstol == 0.f && opts->reltol == 0.f)))
        return fail(h, CNF_ERR_BAD_ARG, "bad tolerances");
    if (opts->dt < 0.f) return fail(h, CNF_ERR_BAD_ARG, "dt must be >= 0 (direction comes from the span)");
    if (opts->maxiters < 1) return fail(h, CNF_ERR_BAD_ARG, "maxiters must be >= 1");
    return CNF_OK;
}
// the state a solve starts from; n_partials: the error partials (blocks, tiles) that meet per attempt
StepState cnfabi::init_step_state(const cnf_solve_opts* opts, int n_partials) {
    StepState init;
    memset(&init, 0, sizeof init);
    init.t = init.t0 = opts->t0;
    init.dt = opts->dt;
    init.qold = 1e-4f;
    init.abstol = opts->abstol; init.reltol = opts->reltol;
    init.adaptive = opts->adaptive ? 1 : 0;
    init.n_partials = n_partials;
    step_state_set_t1(&init, opts->t1);
    return init;
}

namespace {
// One call on its way through the drivers below: the call, its route (cnf_solve_plan.h) and what the drivers share
struct SolveRun {
    const SolveCall& c;
    SolveRoute rt;
    AuxEval aux;
    int k = 0, train = 0, D = 0, nblk = 0;     // nblk: error partials = blocks of whichever kernel writes them
    size_t n = 0;                  // floats of the state
    hipStream_t st = nullptr;
    StepState* init = nullptr;     // the state the solve starts from (pinned)
    bool final_sync = true;
    int launches = 0, nf = 0;
};

// Gradient path on the device-indexed routes: every attempt files u_n and its stage states in the slot of step `naccept`; the
// store is sized beforehand and the solve repeated if it took more steps than fit
struct TrajDump { float* dump = nullptr; size_t slot = 0; int dcap = 0; };
}  // namespace
static cnf_status traj_dump(cnf_handle h, size_t n, TrajDump* d) {
    const cnf_status s = traj_reserve(h, 64);
    if (s != CNF_OK) return s;
    d->slot = traj_slot_floats(h); d->dcap = h->traj_cap;
    d->dump = h->traj + n;                           // stage area of slot 0; u_n sits one array before
    return CNF_OK;
}
// ... and its step sizes back from the device into rec->hs (enqueued: the caller waits for the stream)
static cnf_status recorder_fetch_hs(cnf_handle h, Recorder* rec, const StepState& fin, hipStream_t st) {
    rec->n = fin.naccept;
    rec->overflow = !rec->wg && fin.naccept > h->traj_cap;
    rec->hs.assign((size_t)(rec->overflow ? 0 : fin.naccept), 0.f);
    if (!rec->overflow && fin.naccept > 0)
        HIPCHK(h, hipMemcpyAsync(rec->hs.data(), rec->wg ? rec->wg->hs_out : h->traj_hs, (size_t)fin.naccept * sizeof(float),
                                 hipMemcpyDeviceToHost, st));
    return CNF_OK;
}
// the accepted steps of a path call, as cnf_path_steps hands them out
static void path_keep_steps(cnf_handle h, std::vector<float>& t, std::vector<float>& hh, bool nonfinite) { h->path_t.swap(t); h->path_h.swap(hh); h->path_valid = !nonfinite; }
// ... of the in-launch route: the pairs the launch filed, back from the device
static cnf_status path_fetch_steps(cnf_handle h, const StepState& fin, hipStream_t st) {
    std::vector<float> pairs((size_t)2 * fin.naccept), t((size_t)fin.naccept), hh((size_t)fin.naccept);
    if (fin.naccept > 0) HIPCHK(h, hipMemcpyAsync(pairs.data(), h->d_path_steps, pairs.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    for (int i = 0; i < fin.naccept; ++i) { t[i] = pairs[2 * i]; hh[i] = pairs[2 * i + 1]; }
    path_keep_steps(h, t, hh, fin.nonfinite != 0);
    return CNF_OK;
}

// What every driver ends with: the final state to u_out (copy), what a device-indexed route filed on the device back to the host
// (device_steps: the recorder's step sizes, the path's step pairs), the wait, the statistics, the non-finite return
static cnf_status finish_solve(cnf_handle h, SolveRun& r, const StepState* state_dev, const StepState& fin, bool copy, bool device_steps,
                               int nf, int kernel_used) {
    Recorder* rec = r.c.rec;
    if (copy) { launch_copy_final(state_dev, h->U[0], h->U[1], r.c.u_out, r.n, r.st); ++r.launches; }
    HIPCHK(h, hipGetLastError());
    if (device_steps && rec) {
        const cnf_status s = recorder_fetch_hs(h, rec, fin, r.st);
        if (s != CNF_OK) return s;
        if (rec->wg) rec->wg_done = true;
        else r.final_sync = true;
    }
    if (device_steps && r.c.path && fin.naccept <= PATH_STEPS_CAP) {
        const cnf_status s = path_fetch_steps(h, fin, r.st);
        if (s != CNF_OK) return s;
    }
    // the step count is already known from the last mirror; the copy is stream-ordered work.  Callers that
    // hand u_out to the host wait here, cnf_inference goes straight on to the post-processing kernel.
    if (r.final_sync) HIPCHK(h, hipStreamSynchronize(r.st));
    fill_stats(r.c.stats, fin, nf, kernel_used, r.launches);
    if (fin.nonfinite) {
        // (the step sizes above may still be on their way into rec->hs, which the caller drops on this return)
        if (rec && rec->wg) HIPCHK(h, hipStreamSynchronize(r.st));
        return fail(h, CNF_ERR_NONFINITE, "solver state became NaN/Inf");
    }
    return CNF_OK;
}

// A submitted inference or gradient (grad): the one-launch solve with index `seq` is on its way; cnf_inference_collect /
// cnf_loss_grad_collect read its outcome from its mirror slot.  Under g_persist_mu.
static void leave_in_flight(cnf_handle h, const SolveRun& r, unsigned seq, int mslot, bool grad) {
    const SolveCall& c = r.c;
    cnf_ctx::Submitted sub;
    sub.launched = true; sub.grad = grad; sub.seq = seq; sub.slot = mslot; sub.hairer = r.rt.hairer; sub.mode = c.mode; sub.B = c.B;
    sub.k = grad ? CNF_KERNEL_MFMA : r.k; sub.opts = *c.opts; sub.st = r.st;
    if (!grad) { sub.xs = c.post->xs; sub.eps = c.eps; sub.logpx = c.post->logpx; sub.regs = c.post->regs; sub.sums5 = c.post->sums5; }
    h->submitted.push_back(sub);
    h->sub_taken = true;
    ++g_submitted_inflight; g_submitted_stream = r.st;
    if (c.post) c.post->launched = true;
    if (grad) c.rec->wg_submitted = true;
}

// The whole solve in ONE launch where the handle and the batch allow it (k_solve3b / k_solve3jb): the weights and the
// Runge-Kutta rows stay on the CUs for all attempts, the workgroups exchange two floats per attempt;
// ... or of a small two-layer network, one wave per 16-sample tile, registers only (k_solve_wave, cnf_wave.hip)
// ... or of config 5's network at eight columns per CU (k_solve_bcast, cnf_bcast.hip)
// ... or of the 32-128-128-32 network in TestMode (exact trace: k_trace3s<SOLVE>, cnf_trace.hip).
// The call ends here with the status returned -- finished, left in flight (submitted), or handed back to the gradient's caller
// (rec->wg_failed) -- unless *host_driven: no kernel took the batch, or the launch gave up, and a host-driven driver runs the
// solve (from u0 again).  One such kernel at a time in this process (two would each hold CUs the other is waiting for), except
// that launches queued on ONE stream run one after the other by themselves (submitted inferences): the lock is held until this
// function returns, whichever way.
static cnf_status solve_one_launch(cnf_handle h, SolveRun& r, bool* host_driven) {
    const SolveCall& c = r.c;
    const SolveRoute& rt = r.rt;
    Recorder* rec = c.rec; PostHook* post = c.post; PathHook* path = c.path; JvpCall* jvp = c.jvp;
    const cnf_solve_opts* opts = c.opts;
    const int B = c.B, train = r.train;  const size_t n = r.n;  hipStream_t st = r.st;
    cnf_status s = CNF_OK;
    *host_driven = false;
    std::unique_lock<std::mutex> persist_lock(g_persist_mu);
    if (g_submitted_inflight > 0 && g_submitted_stream != st) HIPCHK(h, hipStreamSynchronize(g_submitted_stream));
    const unsigned base = h->mirror_base;
    const int mslot = 1 + (int)(h->one_launch_count % 3);
    Solve3Args sv{};
    sv.part = h->partials; sv.base_dev = sums_word<unsigned>(h, SUMS_MEET_BASE); sv.abort_flag = sums_word<int>(h, SUMS_ABORT);
    sv.t_out = h->time_kernel ? sums_word<unsigned long long>(h, SUMS_CLOCK) : nullptr;
    sv.maxiters = (int)opts->maxiters; sv.hairer = rt.hairer ? 1 : 0; sv.init = *r.init;
    // How long a wait inside the kernel lasts before it gives up: bounded in TIME (the kernel's 100 MHz clock) -- 2 ms per
    // tile a workgroup carries (a meeting's arrivals are microseconds apart when every workgroup is placed; a workgroup
    // that is not placed because another tenant holds its CU makes the launch give up after that long, and the streamed
    // solve starts).  CNF_SOLVE_WAIT_US overrides; CNF_SOLVE_POLL_LIMIT bounds the number of polls instead (tests: 1).
    set_wait_bounds(h, sv);
    sv.trace = h->step_trace; sv.trace_cap = h->step_trace_cap;
    if (jvp) { sv.trace = h->jvp_trace; sv.trace_cap = jvp->trace_cap; }
    // (k_trace3s<SOLVE> works on the integrator's buffers: u0 is assembled / copied into U[0] in front of it, the
    // post-processing follows it -- three launches per inference)
    if (rt.tsolve_ok) {
        if (post && post->xs) launch_build_u0(post->xs, h->U[0], h->nd.nvars, r.D, B, st);
        else if (c.u0 != h->U[0]) HIPCHK(h, hipMemcpyAsync(h->U[0], c.u0, n * sizeof(float), hipMemcpyDeviceToDevice, st));
        ++r.launches;
    }
    const bool fused_io = post && post->xs && !rt.tsolve_ok;   // inference: u0 from the data columns and the post-processing in the launch
    if (fused_io) { sv.xs = post->xs; sv.logpx = post->logpx; sv.regs = post->regs; sv.sums5 = post->sums5; if (rec) sv.u_out = c.u_out; }
    else { sv.u0 = c.u0; sv.u_out = rt.tsolve_ok ? nullptr : c.u_out; }   // (the launcher reads u0 in place or copies it into U[0])
    TrajDump td;
    if (rec && !rec->wg && (s = traj_dump(h, n, &td)) != CNF_OK) return s;
    s = CNF_ERR_UNSUPPORTED;
    WavePathArgs wp{};
    if (path && rt.wave_ok) {                        // the save times to the device; the launch files its accepted steps
        RESERVE(h, h->d_saveat, (size_t)path->K);
        RESERVE(h, h->d_path_steps, (size_t)2 * PATH_STEPS_CAP);
        HIPCHK(h, hipMemcpyAsync(h->d_saveat, path->saveat, (size_t)path->K * sizeof(float), hipMemcpyHostToDevice, st));
        wp.times = h->d_saveat; wp.K = path->K; wp.out = path->out; wp.steps = h->d_path_steps; wp.steps_cap = PATH_STEPS_CAP;
    }
    if (rt.wave_ok)
        s = wave_solve_launch(h->nd_wave, train != 0, h->d_params, h->nd.n_cond > 0 ? h->d_cond : nullptr, h->cbs, h->d_state, h->U[0],
                              c.eps, B, st, h->d_mirror + mslot, base, sv, rec ? rec->wg : nullptr, nullptr, path ? &wp : nullptr);
    // (the gradient in the launch of the solve exists on the wave kernel only: if that launch could not start, the caller
    // runs the streamed gradient path)
    if (rec && rec->wg && s != CNF_OK) { rec->wg_failed = true; return CNF_OK; }
    if (rt.tsolve_ok) {
        const GradLayout g = grad_layout(h->nd);
        const AdjMfmaLayout m = adj_mfma_layout(h->nd, g);
        TraceArgs ta{};
        ta.B = B; set_rk_buffers(h, ta);
        ta.norm_kind = -1; ta.st_mut = h->d_state; ta.n_total = (float)n;
        ta.mirror = h->d_mirror + mslot; ta.seq = base;
        s = launch_trace_solve(h->nd, g, m, h->d_adj_img, ta, sv, st) == hipSuccess ? CNF_OK : CNF_ERR_UNSUPPORTED;
        if (s != CNF_OK) (void)hipGetLastError();
    }
    if (rt.bcast_ok) {
        BcastRecord brec{td.dump, n, td.slot, td.dcap, h->traj_hs};
        Solve3Args svb = sv;
        if (rec && c.u_out) svb.u_out = c.u_out;     // (this kernel writes the final state where it is wanted)
        s = bcast_solve_launch(h->nd, train != 0, h->d_params, h->d_bimg, h->d_state, h->U[0], c.eps, B, st, h->d_mirror + mslot, base, svb, h->device,
                               h->d_bstore, h->nd.n_cond > 0 ? h->d_cond : nullptr, h->cbs, rec ? &brec : nullptr);
        if (s == CNF_OK && rec && c.u_out) sv.u_out = c.u_out;
    }
    if (s == CNF_ERR_UNSUPPORTED && rt.use_mfma && !jvp)
        s = mfma_solve_persistent(h->mfma, h->nd, train, h->d_state, h->U, c.eps, B, st, h->d_mirror + mslot, base, sv, h->device,
                                  td.dump, n, td.slot, td.dcap, h->traj_hs, h->K1);
    if (s == CNF_ERR_UNSUPPORTED) { *host_driven = true; return CNF_OK; }
    if (s != CNF_OK) return fail(h, s, "one-launch solve failed to start");
    ++r.launches;
    h->mirror_base = base + 1;
    ++h->one_launch_count;
    h->last_state = h->d_state;
    HIPCHK(h, hipGetLastError());
    if (jvp) {
        // the tangent launch, right behind the solve on its stream: no host wait in between.  It reads the solve's final
        // state first and writes nothing for a solve that gave up (the stepwise driver then files the steps)
        JvpCall& jc = *jvp;
        jc.ta.st = h->d_state; jc.ta.trace = h->jvp_trace; jc.ta.trace_cap = jc.trace_cap; jc.ta.n_rows = -1;
        if ((s = tangent_launch(jc.ta, jc.train, st)) != CNF_OK) return fail(h, s, "the tangent launch failed to start");
        jc.enqueued = true;
        ++r.launches;
    }
    const bool sub_grad = rec && rec->wg;
    if (h->submitting && (sub_grad || (fused_io && !rec && !c.u_out))) { leave_in_flight(h, r, base, mslot, sub_grad); return CNF_OK; }
    StepState fin{}; bool aborted = false;
    if ((s = finish_one_launch(h, base, mslot, st, &fin, &aborted)) != CNF_OK) return s;
    if (!aborted) {
        if (fused_io) post->launched = true;
        else if (post) { enqueue_post(h, train, h->d_state, *post, B, false, st); ++r.launches; post->launched = true; }
        return finish_solve(h, r, h->d_state, fin, c.u_out && !sv.u_out, true, (rt.hairer ? 2 : 1) + 6 * (fin.naccept + fin.nreject),
                            rt.wave_ok ? CNF_KERNEL_MFMA : r.k);
    }
    // A workgroup did not arrive within the wait bound: something else holds CUs (another stream or process, a CU
    // mask).  The launch has ended (every wait is bounded); nothing of its result is used.  The solve runs again from
    // u0 on a host-driven driver, which needs no co-residency.
    ++h->fallbacks;
    if (rec && rec->wg) { rec->wg_failed = true; return CNF_OK; }      // (the caller runs the streamed gradient path)
    // (u0 == h->U[0] was solved in place; it can only be rebuilt when the caller's data columns are still at hand --
    // `inference_impl` passes them in post->xs, solve_start assembles u0 from them again)
    if (!fused_io && c.u0 == h->U[0] && !(post && post->xs))
        return fail(h, CNF_ERR_HIP, "one-launch solve: a workgroup did not arrive and u0 was solved in place (set CNF_PERSISTENT=0)");
    *host_driven = true;
    return CNF_OK;
}

// One right-hand side of the start of a host-driven solve, on the route's kernel.  Stage 0: k1 = f(u0) -> K1[0]; stage 1: f1 = f(u0 + h k1) -> Ks[0].  *fuse, in: the
// norm of the automatic initial dt that belongs to the stage and its controller phase ride in the launch (the last workgroup to
// finish runs the phase); out: they did (the fused step kernel may answer "not this batch" for stage 0).
static cnf_status eval_rhs(cnf_handle h, SolveRun& r, int stage, bool* fuse) {
    const int B = r.c.B, train = r.train;
    const float* eps = r.c.eps;
    hipStream_t st = r.st;
    unsigned* ticket = sums_word<unsigned>(h, SUMS_NORM_TICKET);
    cnf_status s = CNF_OK;
    ++r.launches;
    if (r.rt.use_mfma) {
        if (stage == 0 && *fuse) {
            s = mfma_rhs_init0(h->mfma, h->nd, train, h->d_state, h->U[0], eps, h->K1[0], h->partials, ticket, B, st);
            if (s == CNF_OK) return s;
            if (s != CNF_ERR_UNSUPPORTED) return fail(h, s, "MFMA RHS launch failed");
            *fuse = false;
        }
        if (stage == 0) s = mfma_rhs(h->mfma, h->nd, train, h->U[0], eps, h->K1[0], B, st);
        else if (*fuse) s = mfma_rhs_stage(h->mfma, h->nd, train, h->d_state, h->U, h->K1, h->Ks, eps, 1, B, st, h->d_state, h->partials, ticket);
        else s = mfma_rhs_stage(h->mfma, h->nd, train, h->d_state, h->U, h->K1, h->Ks, eps, 1, B, st);
        return s == CNF_OK ? s : fail(h, s, "MFMA RHS launch failed");
    }
    if (r.aux.on) {
        const float one = 1.f;
        TraceFuse f; f.norm_kind = stage;
        if (stage == 0) return launch_trace(h, r.aux, h->U[0], h->K1[0], *fuse, false, B, st, 0, nullptr, false, *fuse ? &f : nullptr);
        return launch_trace(h, r.aux, nullptr, h->Ks[0], true, false, B, st, 1, &one, false, *fuse ? &f : nullptr);
    }
    RhsArgs a{};
    a.B = B; a.S = h->cap_B; a.train = train; a.ws = h->ws; a.eps = eps; a.cond = h->mfma.cond; a.cbs = h->cbs;
    if (stage == 0) { a.u = h->U[0]; a.du = h->K1[0]; }
    else { a.st = h->d_state; set_rk_buffers(h, a); a.nk = 1; a.coef[0] = 1.f; a.du = h->Ks[0]; }
    launch_rhs_generic(h->nd, h->d_params, a, st);
    return CNF_OK;
}
// One norm of the automatic initial dt (kind 0 / 1) and the controller phase of the same number: lock-step through the shards'
// sum, else in the launch of the norm (the last block to finish runs the controller)
static cnf_status initdt_norm(cnf_handle h, SolveRun& r, int kind) {
    NormArgs na{};
    na.st = h->d_state; na.n = r.n; na.partials = h->partials; na.kind = kind;
    set_rk_buffers(h, na);
    if (r.rt.lockstep) {
        launch_norm_partials(na, r.nblk, r.st);
        r.launches += 2;
        return lockstep_controller(h, h->d_state, h->partials, kind, (float)r.n, r.st);
    }
    na.ticket = sums_word<unsigned>(h, SUMS_NORM_TICKET); na.st_mut = h->d_state; na.ctrl_phase = kind; na.n_total = (float)r.n;
    launch_norm_partials(na, r.nblk, r.st);
    r.launches += 1;
    return CNF_OK;
}
// The initial state and u0, k1 = f(u0), and the automatic initial dt (Hairer; OrdinaryDiffEq's ode_determine_initdt, third
// party).  On the fused step kernel and on k_trace3s the two norms and their controller phases ride in the two RHS launches:
// 2 launches, not 4.
static cnf_status solve_start(cnf_handle h, SolveRun& r) {
    const SolveCall& c = r.c;
    const SolveRoute& rt = r.rt;
    cnf_status s = CNF_OK;
    if (c.post && c.post->xs) launch_build_u0(c.post->xs, h->U[0], h->nd.nvars, r.D, c.B, r.st, h->d_state, r.init);   // (u0 == h->U[0])
    else launch_set_state(h->d_state, *r.init, r.st);
    if (c.u0 != h->U[0]) HIPCHK(h, hipMemcpyAsync(h->U[0], c.u0, r.n * sizeof(float), hipMemcpyDeviceToDevice, r.st));
    bool fused = rt.hairer && ((rt.use_mfma && !rt.lockstep) || (r.aux.on && rt.trace_fused));
    if ((s = eval_rhs(h, r, 0, &fused)) != CNF_OK) return s;
    r.nf = 1;
    if (rt.hairer && fused) {
        if ((s = eval_rhs(h, r, 1, &fused)) != CNF_OK) return s;
        r.nf += 1;
    } else if (rt.hairer) {
        if ((s = initdt_norm(h, r, 0)) != CNF_OK) return s;
        if ((s = eval_rhs(h, r, 1, &fused)) != CNF_OK) return s;
        if ((s = initdt_norm(h, r, 1)) != CNF_OK) return s;
        r.nf += 1;
    }
    HIPCHK(h, hipGetLastError());
    return CNF_OK;
}

// The interpolation of the accepted step (t_attempt, h_attempt) at every save time up to its end -- the last step everything left
// (k_dense_out); u_n, k_1 sit in the buffer set the controller has just left, u_{n+1}, k_7 in the current one
static void path_dense_out(cnf_handle h, SolveRun& r, const StepState& snap, float t_attempt, float h_attempt, int* pcur) {
    const PathHook* path = r.c.path;
    const float t_end = snap.t, tdir = snap.tdir;
    const int cur = snap.cur;
    DenseOutArgs da{};
    da.u = h->U[cur ^ 1]; da.unew = h->U[cur]; da.k[0] = h->K1[cur ^ 1]; da.k[6] = h->K1[cur];
    for (int i = 0; i < 5; ++i) da.k[1 + i] = h->Ks[i];
    da.n = r.n; da.out = path->out; da.h = h_attempt;
    for (; *pcur < path->K; ++*pcur) {
        const float tau = path->saveat[*pcur];
        if (!snap.done && tdir * (tau - t_end) > 0.f) break;
        const float th = (tau - t_attempt) / h_attempt;
        const int c = da.count++;
        da.slice[c] = *pcur; da.exact[c] = (tau == t_end || !(th < 1.f)) ? 1 : 0;
        tsit5_dense_b(th, da.b[c]);
        if (da.count == DENSE_OUT_MAX) { launch_dense_out(da, r.st); ++r.launches; da.count = 0; }
    }
    if (da.count > 0) { launch_dense_out(da, r.st); ++r.launches; }
}

// One attempt at a time, the host reading the state after each (who needs that: cnf_solve_plan.h, `stepwise`)
static cnf_status solve_stepwise(cnf_handle h, SolveRun& r) {
    const SolveCall& c = r.c;
    const SolveRoute& rt = r.rt;
    Recorder* rec = c.rec; PathHook* path = c.path; JvpCall* jvp = c.jvp;
    const cnf_solve_opts* opts = c.opts;
    const int B = c.B, train = r.train;  const size_t n = r.n;  hipStream_t st = r.st;
    cnf_status s = CNF_OK;
    StepState* snap = &h->h_state[0];
    float h_attempt = 0.f, t_attempt = 0.f;
    int seen_accept = 0, pcur = 0;                   // pcur: the next save time
    std::vector<float> path_t, path_h;
    if (path || jvp) {
        HIPCHK(h, hipMemcpyAsync(snap, h->d_state, sizeof(StepState), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
        h_attempt = snap->h; t_attempt = snap->t;
        if (jvp) { jvp->enqueued = false; jvp->host_steps = true; jvp->t.clear(); jvp->h.clear(); }
        for (; path && pcur < path->K && path->saveat[pcur] == opts->t0; ++pcur)      // save times at the start: u0 itself
            HIPCHK(h, hipMemcpyAsync(path->out + (size_t)pcur * n, h->U[0], n * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    if (rec) {
        float* slot0;
        if ((s = traj_slot(h, 0, &slot0)) != CNF_OK) return s;
        HIPCHK(h, hipMemcpyAsync(slot0, h->U[0], n * sizeof(float), hipMemcpyDeviceToDevice, st));
        HIPCHK(h, hipMemcpyAsync(snap, h->d_state, sizeof(StepState), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
        h_attempt = snap->h;
        rec->hs.clear(); rec->n = 0;
    }
    // Lock-step over an RCCL communicator: nothing of an attempt leaves the stream (step kernel, the reduction of the
    // partials, the all-reduce of three floats, the controller), so FOUR attempts are enqueued per look at the state --
    // every shard holds the same state bit for bit, sees `done` in the same attempt and enqueues the same number of
    // collectives; attempts queued past the end find `done` and change nothing.
    const int chunk = (rt.lockstep && h->shard_comm && rt.use_mfma && !rec) ? 4 : 1;
    for (long it = 0;; it += chunk) {
        if (it >= (long)opts->maxiters) return fail(h, CNF_ERR_MAXITERS, "maxiters reached before t1");
        for (int ci = 0; ci < chunk && it + ci < (long)opts->maxiters; ++ci) {
            float* dump = nullptr;
            if (rec) {                               // stage states of the attempt from u_{seen_accept}
                float* slot;
                if ((s = traj_slot(h, seen_accept, &slot)) != CNF_OK) return s;
                dump = slot + n;
            }
            if (rt.use_mfma) {
                s = mfma_step(h->mfma, h->nd, train, h->d_state, h->d_state + 1, h->U, h->K1, h->Ks, c.eps,
                              h->partials, h->partials, false, false, B, st, dump, n);
                if (s != CNF_OK) return fail(h, s, "MFMA step launch failed");
                r.launches += 1;
            } else r.launches += enqueue_attempt_generic(h, r.aux, train, c.eps, B, r.nblk, st, false, dump, n);
            if (rt.lockstep && (s = lockstep_controller(h, h->d_state, h->partials, 2, (float)n, st)) != CNF_OK) return s;
            if (!rt.lockstep) launch_controller(h->d_state, h->partials, 2, (float)n, st);
            r.launches += rt.lockstep ? 2 : 1;
        }
        HIPCHK(h, hipMemcpyAsync(snap, h->d_state, sizeof(StepState), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
        const bool accepted = snap->naccept > seen_accept;
        if (accepted) seen_accept = snap->naccept;
        if (rec && accepted) {
            float* slot;
            if ((s = traj_slot(h, seen_accept, &slot)) != CNF_OK) return s;
            HIPCHK(h, hipMemcpyAsync(slot, h->U[snap->cur], n * sizeof(float), hipMemcpyDeviceToDevice, st));
            rec->hs.push_back(h_attempt);
            rec->n = seen_accept;
        }
        if (jvp && !rec && !path && accepted) { jvp->t.push_back(t_attempt); jvp->h.push_back(h_attempt); }   // for its replay
        if (path && accepted) {
            path_t.push_back(t_attempt); path_h.push_back(h_attempt);
            path_dense_out(h, r, *snap, t_attempt, h_attempt, &pcur);
        }
        h_attempt = snap->h; t_attempt = snap->t;
        if (snap->done) break;
    }
    if (path) path_keep_steps(h, path_t, path_h, snap->nonfinite != 0);
    h->last_state = h->d_state;
    r.final_sync = true;
    return finish_solve(h, r, h->d_state, *snap, c.u_out != nullptr, false, r.nf + 6 * (snap->naccept + snap->nreject),
                        (r.k == CNF_KERNEL_MFMA && !rt.use_mfma && !r.aux.on) ? CNF_KERNEL_GENERIC : r.k);
}

// Streamed solve: launches are kept a few attempts ahead of the last state the host has seen.  The controller of an
// attempt runs on the device -- inside the NEXT launch of the fused step kernel, or in the last block of the error-norm
// kernel on the per-stage paths -- and whoever ran it mirrors the new state to pinned host memory under the launch
// index; the host polls that index: no events, no copies, no stand-alone controller, no chunk boundaries.
// Launches queued past the end find `done` and exit at once.
static cnf_status solve_streamed(cnf_handle h, SolveRun& r) {
    const SolveCall& c = r.c;
    const bool use_mfma = r.rt.use_mfma;
    Recorder* rec = c.rec; PostHook* post = c.post;
    const cnf_solve_opts* opts = c.opts;
    const int B = c.B, train = r.train;  const size_t n = r.n;  hipStream_t st = r.st;
    cnf_status s = CNF_OK;
    StepState* cur_state = h->d_state;   // slot holding the live integrator state
    int pp = 0;                          // partials buffer the NEXT launch reads
    bool done = false; StepState fin{};
    long post_at = -1, seen_done = -1;  // launches enqueued when the post-processing was last enqueued; the launch that published `done`
    const int AHEAD = 3;
    const volatile cnf_ctx::HostMirror* hm = h->h_mirror;
    const unsigned base = h->mirror_base;
    long sent = 0, seen = 0;       // launches (fused) / attempts (per-stage) enqueued; newest mirror index read
    const long max_sent = (long)opts->maxiters + (use_mfma ? 1 : 0);   // fused: one more launch runs the last controller
    TrajDump td;
    if (rec && (s = traj_dump(h, n, &td)) != CNF_OK) return s;
    // attempts the newest snapshot says are still needed, (t1 - t)/dt rounded up (the controller rarely shrinks dt
    // near the end); -1 = no snapshot yet.  Launches beyond that would only find `done` and exit.
    long need = -1;
    for (;;) {
        while (sent < max_sent && sent - seen < AHEAD && !done &&
               (need < 0 || sent - seen < need + (use_mfma ? 1 : 0))) {      // fused: + the launch that runs the last controller
            if (use_mfma) {
                // launch i applies the controller of attempt i-1 and publishes under index i
                const bool apply = sent > 0;
                StepState* st_next = cur_state == h->d_state ? h->d_state + 1 : h->d_state;
                s = mfma_step(h->mfma, h->nd, train, cur_state, st_next, h->U, h->K1, h->Ks, c.eps,
                              h->partials + 2 * MAX_PARTIALS * pp, h->partials + 2 * MAX_PARTIALS * (pp ^ 1), apply,
                              false, B, st, td.dump, n, h->d_mirror, base + (unsigned)sent, td.slot, td.dcap, h->traj_hs);
                if (s != CNF_OK) return fail(h, s, "MFMA step launch failed");
                if (apply) cur_state = st_next;
                pp ^= 1;
                ++r.launches;
            } else {
                // attempt i ends with its own controller and publishes under index i + 1
                r.launches += enqueue_attempt_generic(h, r.aux, train, c.eps, B, r.nblk, st, true, nullptr, 0, h->d_mirror,
                                                      base + (unsigned)sent + 1);
            }
            ++sent;
        }
        h->mirror_base = base + (unsigned)sent + 1;
        // everything the estimate asks for is in the queue: the post-processing goes right behind it (fused path: the
        // state slot the newest launch writes is the one a `done` would be published in)
        if (post && !rec && use_mfma && !done && need >= 0 && sent - seen >= need + 1 && post_at != sent) {
            enqueue_post(h, train, cur_state, *post, B, true, st);
            post_at = sent;
            ++r.launches;
        }
        if (done) break;
        if (seen >= (long)opts->maxiters) {
            HIPCHK(h, hipStreamSynchronize(st));
            return fail(h, CNF_ERR_MAXITERS, "maxiters reached before t1");
        }
        // wait for a consistent snapshot newer than the last one read
        unsigned sq = 0; StepState snap;
        if ((s = mirror_wait(h, hm, st, &snap, &sq, [base, seen](unsigned tag) { return (int)(tag - base) > (int)seen; },
                             "step kernels finished without publishing a state")) != CNF_OK) return s;
        seen = (long)(sq - base);
        if (snap.done) { fin = snap; done = true; seen_done = seen; }
        need = 1;
        if (snap.dt > 0.f) {
            const double left = std::fabs((double)snap.t1 - (double)snap.t) / (double)snap.dt;
            need = left > 1e6 ? 1000000 : (long)std::ceil(left - 1e-6);
            if (need < 1) need = 1;
        }
    }
    h->last_state = cur_state;
    if (post) {
        // the speculative launch counts if it was enqueued behind the launch that published `done` (mirror index
        // `seen`, i.e. launch number seen on the fused path: the launches are numbered from 0)
        if (!(post_at > seen_done)) { enqueue_post(h, train, cur_state, *post, B, false, st); ++r.launches; }
        post->launched = true;
    }
    return finish_solve(h, r, cur_state, fin, c.u_out != nullptr, true, r.nf + 6 * (fin.naccept + fin.nreject), r.k);
}

// Every solve: the call's checks, its route (cnf_solve_plan.h), then the drivers.
static cnf_status solve_core(cnf_handle h, const SolveCall& c) {
    cnf_status s = check_call(h, c.mode, c.B);
    if (s != CNF_OK) return s;
    h->rec.end();                      // (every solve may overwrite what a record consists of)
    if (!c.u0 || !c.opts) return fail(h, CNF_ERR_BAD_ARG, "null pointer");
    const bool train = c.mode == CNF_MODE_TRAIN;
    if (train && !c.eps) return fail(h, CNF_ERR_BAD_ARG, "eps is required in TrainMode");
    if ((s = check_solve_opts(h, c.opts)) != CNF_OK) return s;
    if (c.stats) memset(c.stats, 0, sizeof *c.stats);
    if (c.B == 0) return CNF_OK;
    SolveRun r{c};
    if ((s = resolve_kernel(h, c.mode, c.B, c.opts->kernel, &r.k)) != CNF_OK) return s;
    if ((s = ensure_capacity(h, c.B)) != CNF_OK) return s;
    HIPCHK(h, hipSetDevice(h->device));
    r.st = (hipStream_t)c.stream; r.train = train; r.D = rows_of(h, c.mode); r.n = (size_t)r.D * c.B; r.final_sync = c.final_sync;
    const SolveAsk ask{r.k == CNF_KERNEL_MFMA, c.opts->kernel == CNF_KERNEL_GENERIC, train, c.opts->adaptive != 0, c.opts->dt == 0.f,
                       h->shard_reduce != nullptr || h->shard_comm != nullptr, h->no_persist, c.rec != nullptr, c.rec && c.rec->wg,
                       c.post && c.post->xs, c.path != nullptr, c.jvp != nullptr, h->nd.n_cond != 0, h->nd_wave.id2 != 0};
    SolveCaps caps{};
    caps.mfma_ok = mfma_supported(h->mfma, h->nd, train, c.B);
    caps.wave_solve_ok = wave_solve_supported(h->nd_wave, train, c.B);
    caps.wave_grad_ok = ask.rec_wg && wave_grad_supported(h->nd_wave, c.B, train);
    caps.bcast_solve_ok = bcast_solve_supported(h->nd, train, c.B, h->device);
    caps.bcast_store_is_zero = bcast_store_floats(c.B, h->device) == 0;
    const AuxEval may{ask.k_mfma && !caps.mfma_ok, train, c.eps};      // (the auxiliary kernels cannot run otherwise)
    caps.trace_fused_ok = may.on && trace_fused_ok(h, may, c.B);
    caps.trace_solve_ok = caps.trace_fused_ok && trace_solve_supported(h->nd, adj_mfma_layout(h->nd, grad_layout(h->nd)), c.B, h->device);
    r.rt = solve_route(ask, caps);
    r.aux = AuxEval{r.rt.trace_on, train, c.eps};
    if (r.aux.on && (s = ensure_adj_images(h, r.st)) != CNF_OK) return s;
    r.nblk = r.rt.partials == PARTIALS_TRACE_GRID ? trace_fused_grid(c.B)
           : r.rt.partials == PARTIALS_MFMA_GRID ? mfma_grid_for(h->mfma, c.B, c.rec != nullptr, train)
           : (int)std::min<size_t>((r.n + 255) / 256, 256);
    r.init = init_state(h);
    *r.init = init_step_state(c.opts, r.nblk);
    if (r.rt.wg_refused) { c.rec->wg_failed = true; return CNF_OK; }
    if (r.rt.bcast_prepare) {
        RESERVE(h, h->d_bimg, bcast_img_floats());          // (allocated on first use)
        if (!h->bimg_valid) { bcast_pack(h->nd, h->d_params, h->d_bimg, r.st); HIPCHK(h, hipGetLastError()); h->bimg_valid = true; }
        const size_t need = bcast_store_floats(c.B, h->device);        // several tiles per workgroup: their rows live in global memory
        if (need > h->d_bstore.capacity()) {
            HIPCHK(h, hipStreamSynchronize(r.st));
            RESERVE(h, h->d_bstore, need);
        }
    }
    if (r.rt.one_launch) {
        bool host_driven = false;
        s = solve_one_launch(h, r, &host_driven);
        if (!host_driven) return s;
    }
    if ((s = solve_start(h, r)) != CNF_OK) return s;
    return r.rt.stepwise ? solve_stepwise(h, r) : solve_streamed(h, r);
}

extern "C" cnf_status cnf_solve_tsit5(cnf_handle h, int mode, const float* u0,
                                      const float* eps, float* u_out, int B,
                                      const cnf_solve_opts* opts, cnf_solve_stats* stats,
                                      void* stream) {
    if (h && !u_out) return fail(h, CNF_ERR_BAD_ARG, "null pointer");
    return solve_core(h, SolveCall{mode, B, u0, eps, u_out, opts, stats, stream});
}

// ---- flow paths (include/cnfhip_path.h) ----
// What is wrong with the save times of a path call (cnf_solve_path and the two calls of include/cnfhip_path_vjp.h), or null: K >= 1
// finite times, monotone along opts->t0 -> opts->t1 and inside that closed span.  Looks at no handle.
const char* cnfabi::saveat_error(const cnf_solve_opts* opts, const float* saveat_host, int K) {
    if (!opts || !saveat_host) return "null pointer";
    if (K < 1) return "saveat is empty";
    if (!std::isfinite(opts->t0) || !std::isfinite(opts->t1) || opts->t0 == opts->t1) return "empty or non-finite time span";
    const float dir = opts->t1 >= opts->t0 ? 1.f : -1.f;
    for (int i = 0; i < K; ++i) {
        const float tau = saveat_host[i];
        if (!std::isfinite(tau)) return "saveat must be finite";
        if (dir * (tau - opts->t0) < 0.f || dir * (opts->t1 - tau) < 0.f) return "saveat must lie inside the time span";
        if (i > 0 && dir * (tau - saveat_host[i - 1]) < 0.f) return "saveat must be monotone along the direction of integration";
    }
    return nullptr;
}
extern "C" cnf_status cnf_solve_path(cnf_handle h, int mode, const float* u0, const float* eps, float* u_out, int B,
                                     const cnf_solve_opts* opts, const float* saveat_host, int K, float* path_out_dev,
                                     cnf_solve_stats* stats, void* stream) {
    // the save times against the span, before the handle is looked at
    const char* bad = !path_out_dev ? "null pointer" : saveat_error(opts, saveat_host, K);
    if (bad) return h ? fail(h, CNF_ERR_BAD_ARG, bad) : CNF_ERR_BAD_ARG;
    if (!h) return CNF_ERR_BAD_ARG;
    if (!u_out) return fail(h, CNF_ERR_BAD_ARG, "null pointer");
    if (h->shard_reduce != nullptr || h->shard_comm != nullptr)
        return fail(h, CNF_ERR_UNSUPPORTED, "cnf_solve_path: lock-step shards have no path");
    h->path_valid = false;
    PathHook ph{saveat_host, K, path_out_dev};
    SolveCall call{mode, B, u0, eps, u_out, opts, stats, stream};
    call.path = &ph;
    return solve_core(h, call);
}

// The host step readers (cnf_path_steps, cnf_path_vjp_steps, cnf_jvp_steps, cnf_grad_steps): the accepted steps (t_n, h_n) a call
// left on the host, up to `cap` of them into whichever array is not null; the number there is, or -1 when there is none
int cnfabi::copy_steps(bool valid, const std::vector<float>& t, const std::vector<float>& hh, float* t_host, float* h_host, int cap) {
    if (!valid) return -1;
    const int n = (int)t.size();
    for (int i = 0; i < n && i < cap; ++i) {
        if (t_host) t_host[i] = t[i];
        if (h_host) h_host[i] = hh[i];
    }
    return n;
}
extern "C" int cnf_path_steps(cnf_handle h, float* t_host, float* h_host, int cap) {
    return h ? copy_steps(h->path_valid, h->path_t, h->path_h, t_host, h_host, cap) : -1;
}

extern "C" cnf_status cnf_solve_tsit5_host(cnf_handle h, int mode, const float* u0, const float* eps,
                                           float* u_out, int B, const cnf_solve_opts* opts,
                                           cnf_solve_stats* stats) {
    cnf_status s = check_call(h, mode, B);
    if (s != CNF_OK) return s;
    if (!u0 || !u_out || !opts) return fail(h, CNF_ERR_BAD_ARG, "null pointer");
    if (B == 0) { if (stats) memset(stats, 0, sizeof *stats); return CNF_OK; }
    HIPCHK(h, hipSetDevice(h->device));
    const size_t D = rows_of(h, mode), n_in = h->nd.n_in;
    if ((s = ensure_stage(h, (2 * D + n_in) * B)) != CNF_OK) return s;
    float* u_d = h->stage;
    float* o_d = u_d + D * B;
    float* e_d = eps ? o_d + D * B : nullptr;
    HIPCHK(h, hipMemcpy(u_d, u0, D * B * sizeof(float), hipMemcpyHostToDevice));
    if (eps) HIPCHK(h, hipMemcpy(e_d, eps, n_in * B * sizeof(float), hipMemcpyHostToDevice));
    s = cnf_solve_tsit5(h, mode, u_d, e_d, o_d, B, opts, stats, nullptr);
    if (s == CNF_OK) {
        hipError_t e = hipMemcpy(u_out, o_d, D * B * sizeof(float), hipMemcpyDeviceToHost);
        if (e != hipSuccess) s = fail(h, CNF_ERR_HIP, hipGetErrorString(e));
    }
    return s;
}

// ---------------------------------------------------------------------------------------
// assembly / post-processing / loss (a6, a8, a9)
// ---------------------------------------------------------------------------------------
extern "C" cnf_status cnf_build_u0(cnf_handle h, int mode, const float* xs, float* u0, int B,
                                   void* stream) {
    if (!h || !xs || !u0) return CNF_ERR_BAD_ARG;
    if (mode != CNF_MODE_TEST && mode != CNF_MODE_TRAIN) return fail(h, CNF_ERR_BAD_ARG, "unknown mode");
    if (B < 0) return fail(h, CNF_ERR_BAD_SHAPE, "negative batch");
    if (B == 0) return CNF_OK;
    HIPCHK(h, hipSetDevice(h->device));
    launch_build_u0(xs, u0, h->nd.nvars, rows_of(h, mode), B, (hipStream_t)stream);
    HIPCHK(h, hipGetLastError());
    return CNF_OK;
}

extern "C" cnf_status cnf_inference_post(cnf_handle h, int mode, const float* u_final,
                                         float* logpx, float* regs, int B, void* stream) {
    if (!h || !u_final || !logpx || !regs) return CNF_ERR_BAD_ARG;
    if (mode != CNF_MODE_TEST && mode != CNF_MODE_TRAIN) return fail(h, CNF_ERR_BAD_ARG, "unknown mode");
    if (B < 0) return fail(h, CNF_ERR_BAD_SHAPE, "negative batch");
    if (B == 0) return CNF_OK;
    HIPCHK(h, hipSetDevice(h->device));
    launch_post(h->nd, mode == CNF_MODE_TRAIN, u_final, logpx, regs, B, (hipStream_t)stream);
    if (h->bd.kind)          // logpdf(icnf.basedist, z) - dlogp, afresh (the regulariser rows stay)
        launch_base_post(h->nd.n_in, rows_of(h, mode), h->bd, nullptr, u_final, nullptr, logpx, regs, B, nullptr, nullptr, nullptr,
                         (hipStream_t)stream);
    HIPCHK(h, hipGetLastError());
    return CNF_OK;
}

cnf_status cnfabi::inference_impl(cnf_handle h, int mode, const float* xs, const float* eps,
                                 float* logpx, float* regs, float* u_final, float* sums5, int B,
                                 const cnf_solve_opts* opts, cnf_solve_stats* stats, void* stream, JvpCall* jvp) {
    cnf_status s = check_call(h, mode, B);
    if (s != CNF_OK) return s;
    if (!xs || !logpx || !regs || !opts) return fail(h, CNF_ERR_BAD_ARG, "null pointer");
    if (stats) memset(stats, 0, sizeof *stats);
    if (B == 0) {
        if (sums5) HIPCHK(h, hipMemsetAsync(sums5, 0, 5 * sizeof(float), (hipStream_t)stream));
        return CNF_OK;
    }
    HIPCHK(h, hipSetDevice(h->device));
    if ((s = ensure_capacity(h, B)) != CNF_OK) return s;
    // no allocations and no copies on this path: u0 is assembled in the integrator's own state buffer, and the
    // post-processing reads the final state from wherever the integrator left it
    PostHook ph{logpx, regs, sums5, xs};
    SolveCall call{mode, B, h->U[0], eps, u_final, opts, stats, stream};
    call.post = &ph; call.jvp = jvp; call.final_sync = false;
    if (s == CNF_OK) s = solve_core(h, call);
    if (s == CNF_OK && !ph.launched) {                      // (the one-attempt-at-a-time drivers leave it to the caller)
        enqueue_post(h, mode == CNF_MODE_TRAIN, h->last_state, ph, B, false, (hipStream_t)stream);   // stream-ordered
        HIPCHK(h, hipGetLastError());
    }
    if (s == CNF_OK && h->bd.kind) {
        // a non-default base distribution: one more launch behind the solve (and its N(0, I) post-processing) overwrites logpx
        // and the sums from the final state in the integrator's buffer -- also behind a submitted launch, in stream order
        launch_base_post(h->nd.n_in, rows_of(h, mode), h->bd, h->last_state, h->U[0], h->U[1], logpx, regs, B, sums5, h->post_part,
                         sums_word<unsigned>(h, SUMS_POST_TICKET), (hipStream_t)stream);
        HIPCHK(h, hipGetLastError());
        if (stats) stats->launches += 1;
    }
    return s;
}

// ---- submitted inferences: enqueue now, collect later (the GPU goes from one solve straight into the next) ----
// The end of one submitted launch: wait for its outcome; a launch that ran out of a wait is run again on the streamed driver.
static cnf_status finish_submission(cnf_handle h, const cnf_ctx::Submitted& sub, cnf_solve_stats* stats) {
    HIPCHK(h, hipSetDevice(h->device));
    StepState fin{};
    bool aborted = false;
    cnf_status s;
    {
        std::unique_lock<std::mutex> lock(g_persist_mu);
        s = finish_one_launch(h, sub.seq, sub.slot, sub.st, &fin, &aborted);
        --g_submitted_inflight;
    }
    if (s != CNF_OK) return s;
    if (!aborted) {
        fill_stats(stats, fin, (sub.hairer ? 2 : 1) + 6 * (fin.naccept + fin.nreject), sub.k, 1);
        if (fin.nonfinite) return fail(h, CNF_ERR_NONFINITE, "solver state became NaN/Inf");
        return CNF_OK;
    }
    ++h->fallbacks;
    if (sub.grad)         // (its gradient was written as zeros and its loss as NaN by k_grad_finish: the caller runs the batch again)
        return fail(h, CNF_ERR_UNSUPPORTED, "the submitted gradient launch gave up (a wait ran out, or more steps than its store holds): "
                                            "zeros were delivered; run the batch again with cnf_loss_grad");
    const bool was = h->collecting;
    h->collecting = true; h->no_persist = true;
    s = inference_impl(h, sub.mode, sub.xs, sub.eps, sub.logpx, sub.regs, nullptr, sub.sums5, sub.B, &sub.opts, stats, sub.st);
    h->no_persist = false; h->collecting = was;
    return s;
}

// The oldest submitted inference, completed and taken off the queue.
cnf_status cnfabi::collect_one(cnf_handle h, cnf_solve_stats* stats) {
    cnf_ctx::Submitted sub = h->submitted.front();
    h->submitted.pop_front();
    if (stats) *stats = sub.stats;
    if (!sub.launched) return sub.status;
    return finish_submission(h, sub, stats);
}

static cnf_status settle_submitted(cnf_handle h) {
    const bool was = h->collecting;
    h->collecting = true;                     // (the fallback's own calls must not drain the queue they are part of)
    for (auto& sub : h->submitted) {
        if (!sub.launched) continue;
        cnf_solve_stats st{};
        sub.status = finish_submission(h, sub, &st);
        sub.stats = st;
        sub.launched = false;
    }
    h->collecting = was;
    return CNF_OK;                            // (each outcome, errors included, is its collect call's)
}

extern "C" cnf_status cnf_inference_submit(cnf_handle h, int mode, const float* xs, const float* eps, float* logpx,
                                           float* regs, float* sums5, int B, const cnf_solve_opts* opts, void* stream) {
    if (!h) return CNF_ERR_BAD_ARG;
    if (h->submitted.size() >= 3) return fail(h, CNF_ERR_BAD_ARG, "three inferences are submitted already: collect one first");
    h->collecting = true; h->submitting = true; h->sub_taken = false;
    cnf_solve_stats st{};
    const cnf_status s = inference_impl(h, mode, xs, eps, logpx, regs, nullptr, sums5, B, opts, &st, stream);
    h->submitting = false; h->collecting = false;
    if (!h->sub_taken) {                      // completed on the spot (another driver, an empty batch, or an error)
        cnf_ctx::Submitted sub;
        sub.status = s; sub.stats = st;
        h->submitted.push_back(sub);
    }
    return CNF_OK;                            // (the outcome, errors included, is the matching collect call's)
}

extern "C" cnf_status cnf_inference_collect(cnf_handle h, cnf_solve_stats* stats) {
    if (!h) return CNF_ERR_BAD_ARG;
    if (stats) memset(stats, 0, sizeof *stats);
    if (h->submitted.empty()) return fail(h, CNF_ERR_BAD_ARG, "no inference is submitted");
    h->collecting = true;
    const cnf_status s = collect_one(h, stats);
    h->collecting = false;
    return s;
}

extern "C" int cnf_inference_pending(cnf_handle h) { return h ? (int)h->submitted.size() : -1; }

extern "C" cnf_status cnf_inference(cnf_handle h, int mode, const float* xs, const float* eps,
                                    float* logpx, float* regs, float* u_final, int B,
                                    const cnf_solve_opts* opts, cnf_solve_stats* stats,
                                    void* stream) {
    return inference_impl(h, mode, xs, eps, logpx, regs, u_final, nullptr, B, opts, stats, stream);
}

extern "C" cnf_status cnf_inference_sums(cnf_handle h, int mode, const float* xs, const float* eps, float* logpx,
                                         float* regs, float* sums5, int B, const cnf_solve_opts* opts,
                                         cnf_solve_stats* stats, void* stream) {
    if (h && !sums5) return fail(h, CNF_ERR_BAD_ARG, "null pointer");
    // the sums ride in the post-processing launch (block partials, the last block adds them in block order)
    return inference_impl(h, mode, xs, eps, logpx, regs, nullptr, sums5, B, opts, stats, stream);
}

extern "C" cnf_status cnf_inference_host(cnf_handle h, int mode, const float* xs,
                                         const float* eps, float* logpx, float* regs,
                                         float* u_final, int B, const cnf_solve_opts* opts,
                                         cnf_solve_stats* stats) {
    cnf_status s = check_call(h, mode, B);
    if (s != CNF_OK) return s;
    if (!xs || !logpx || !regs || !opts) return fail(h, CNF_ERR_BAD_ARG, "null pointer");
    if (B == 0) { if (stats) memset(stats, 0, sizeof *stats); return CNF_OK; }
    HIPCHK(h, hipSetDevice(h->device));
    const size_t D = rows_of(h, mode), n_in = h->nd.n_in, nv = h->nd.nvars;
    const size_t out_f = (size_t)B * (4 + D);
    if ((s = ensure_stage(h, (nv + n_in) * B + out_f)) != CNF_OK) return s;
    float* xs_d = h->stage;
    float* out_d = xs_d + nv * B;
    float* e_d = eps ? out_d + out_f : nullptr;
    HIPCHK(h, hipMemcpy(xs_d, xs, nv * B * sizeof(float), hipMemcpyHostToDevice));
    if (eps) HIPCHK(h, hipMemcpy(e_d, eps, n_in * B * sizeof(float), hipMemcpyHostToDevice));
    float* lp = out_d; float* rg = out_d + B; float* uf = out_d + 4 * (size_t)B;
    s = cnf_inference(h, mode, xs_d, e_d, lp, rg, uf, B, opts, stats, nullptr);
    if (s == CNF_OK) {
        hipError_t e = hipMemcpy(logpx, lp, (size_t)B * sizeof(float), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(regs, rg, 3 * (size_t)B * sizeof(float), hipMemcpyDeviceToHost);
        if (e == hipSuccess && u_final) e = hipMemcpy(u_final, uf, D * B * sizeof(float), hipMemcpyDeviceToHost);
        if (e != hipSuccess) s = fail(h, CNF_ERR_HIP, hipGetErrorString(e));
    }
    return s;
}

extern "C" cnf_status cnf_loss_sums(cnf_handle h, const float* logpx, const float* regs, int B,
                                    float* sums5, void* stream) {
    if (!h || !logpx || !regs || !sums5) return CNF_ERR_BAD_ARG;
    if (B < 0) return fail(h, CNF_ERR_BAD_SHAPE, "negative batch");
    HIPCHK(h, hipSetDevice(h->device));
    launch_loss_sums(logpx, regs, B, sums5, (hipStream_t)stream);
    HIPCHK(h, hipGetLastError());
    return CNF_OK;
}

extern "C" cnf_status cnf_loss_allreduce(cnf_handle h, cnf_comm comm, float* sums5, void* stream) {
    if (!h || !comm || !sums5) return CNF_ERR_BAD_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    if (cnf_comm_allreduce(comm, sums5, 5, stream) != CNF_OK) return fail(h, CNF_ERR_RCCL, cnf_comm_last_error());
    return CNF_OK;
}

extern "C" cnf_status cnf_set_shard_comm(cnf_handle h, cnf_comm comm) {
    if (!h) return CNF_ERR_BAD_ARG;
    h->shard_comm = comm;
    return CNF_OK;
}

// (lam: the handle's regularisers, or a heterogeneous ensemble member's own)
cnf_status cnfabi::loss_from_sums_lam(cnf_handle h, int mode, const float* sums5, const float* lam, float* loss) {
    if (!h || !sums5 || !loss) return CNF_ERR_BAD_ARG;
    const double cnt = sums5[4];
    if (!(cnt > 0)) return fail(h, CNF_ERR_BAD_SHAPE, "empty batch");
    if (mode == CNF_MODE_TRAIN)      // src/icnf.jl:489
        *loss = (float)((-(double)sums5[0] + (double)lam[0] * sums5[1] + (double)lam[1] * sums5[2] +
                         (double)lam[2] * sums5[3]) / cnt);
    else                             // src/base_icnf.jl:496
        *loss = (float)(-(double)sums5[0] / cnt);
    return CNF_OK;
}
extern "C" cnf_status cnf_loss_from_sums(cnf_handle h, int mode, const float* sums5, float* loss) {
    return loss_from_sums_lam(h, mode, sums5, h ? h->lam : nullptr, loss);
}

// ---------------------------------------------------------------------------------------
// Gradient of the TrainMode loss w.r.t. the parameters.
// Reference: MLJModelInterface.fit differentiates loss(icnf, TrainMode(), xs, ps, st) with Enzyme
// through the solve (src/exts/mlj_ext/core_icnf.jl:59-73, src/icnf.jl:481-490).
// ---------------------------------------------------------------------------------------
static cnf_status ensure_grad_capacity(cnf_handle h, int B) {
    HIPCHK(h, hipSetDevice(h->device));
    const GradLayout g = grad_layout(h->nd);
    RESERVE(h, h->d_PT, h->n_params);                      // (allocated on first use, as the images are)
    { const cnf_status rs = reserve_adj_images(h); if (rs != CNF_OK) return rs; }
    if ((size_t)B <= h->grad_cap_B) return CNF_OK;
    HIPCHK(h, hipDeviceSynchronize());
    h->traj.release(); h->traj_hs.release();               // (its slots are sized by grad_cap_B)
    const size_t want = ((size_t)B + 63) & ~(size_t)63;
    const size_t D = (size_t)h->nd.n_in + 3, n_in = h->nd.n_in;
    // the four factor arrays hold the 6 stages of `fsteps` steps: one batch contraction per fsteps steps
    // (K = 6 fsteps B); as many steps as fit a 1 GiB budget, at most 32
    const size_t per_step_1 = 12 * ((size_t)g.sum_in + g.sum_out);           // floats per sample
    size_t fsteps = ((size_t)1 << 28) / (per_step_1 * want);
    if (fsteps < 1) fsteps = 1;
    if (fsteps > 32) fsteps = 32;
    h->grad_fsteps = (int)fsteps;
    const size_t tail = ((size_t)GRAD_MAX_KSPLIT + 1) * h->n_params;
    const hipError_t arena_alloc = (hipError_t)h->grad_arena.reserve((5 * D + 7 * n_in + fsteps * per_step_1) * want + tail);
    // As in ensure_capacity: what is carved from the arena exists only while it does, and neither does what was computed into
    // it -- the gradient cnf_grad_x hands out, a recorded solve, the trajectory.  A failed reserve leaves all of it cleared.
    const size_t cap = arena_alloc == hipSuccess ? want : 0;
    h->rec.clear(); h->traj_cap = 0;
    float* p = h->grad_arena;
    for (int i = 0; i < 5; ++i) { h->g_US[i] = p; p += D * cap; }
    for (int i = 0; i < 6; ++i) { h->g_W[i] = p; p += n_in * cap; }
    h->g_lam = p; p += n_in * cap;
    h->g_HS = p; p += fsteps * 6 * (size_t)g.sum_in * cap;
    h->g_TS = p; p += fsteps * 6 * (size_t)g.sum_in * cap;
    h->g_AB = p; p += fsteps * 6 * (size_t)g.sum_out * cap;
    h->g_PB = p; p += fsteps * 6 * (size_t)g.sum_out * cap;
    h->g_part = p; p += cap ? (size_t)GRAD_MAX_KSPLIT * h->n_params : 0;
    h->g_grad = p;
    h->grad_cap_B = cap;
    HIPCHK(h, arena_alloc);
    return CNF_OK;
}

// Step slots of an in-launch gradient's trajectory store of `per_step` floats per accepted step (one model's, or all the members'
// of an ensemble): WV_GCAP, halved while the store exceeds 2^28 floats = 1 GiB (B = 8192: 256 steps), but 64 at least.
// *fit: how many such stores keep those 64 slots each within that budget.
int cnfabi::traj_step_slots(size_t per_step, size_t* fit) {
    constexpr size_t budget = (size_t)1 << 28;
    constexpr int least = 64;
    if (fit) *fit = budget / (per_step * least);
    int cap = WV_GCAP;
    while (cap > least && per_step * cap > budget) cap /= 2;
    return cap;
}

// loss_and_grad of small batches of a small two-layer tanh network (or a one-layer one through its appended identity layer):
// the solve, the loss sums and the whole discrete adjoint in ONE launch, one wave per 16 samples (k_solve_wave<GRAD>,
// cnf_wave.hip), then the sum of the waves' partials.  TrainMode (VJP compute mode) and TestMode (exact trace).  *done = false:
// not this network / batch, or the launch gave up (a wait ran out, more steps than its store holds) -- nothing was written.
static cnf_status wave_loss_grad(cnf_handle h, int mode, const float* xs, const float* eps, int B, const cnf_solve_opts* opts,
                                 float* loss_out, float* grad, cnf_solve_stats* stats, void* stream, bool* done,
                                 float* loss_dev = nullptr /* submit: the loss goes here (device), nothing is waited for */) {
    *done = false;
    h->rec.backward_begins();                              // (the in-launch gradient carries no d / d ys)
    cnf_status s = CNF_OK;
    hipStream_t st = (hipStream_t)stream;
    const bool train = mode == CNF_MODE_TRAIN;
    if (opts->kernel == CNF_KERNEL_GENERIC || !wave_grad_supported(h->nd_wave, B, train)) return CNF_OK;
    {
        const size_t per_step = wave_grad_traj_floats(h->nd_wave, B);
        int cap = traj_step_slots(per_step);
        // behind the trajectory: the step sizes, and one partial of the flat gradient per wave when there are more waves than
        // the arena's GRAD_MAX_KSPLIT partials
        const int waves = wave_grad_waves(B);
        const size_t part_f = waves > GRAD_MAX_KSPLIT ? (size_t)waves * h->n_params : 0;
        // TrainMode / VJP at small batches: the forward pass also files its evaluations' intermediates (the backward pass then
        // skips half of its products), while at least 256 steps of them fit in 256 MiB
        size_t rich_step = wave_grad_rich_floats(h->nd_wave, B, train);
        if (rich_step * 256 > ((size_t)1 << 26)) rich_step = 0;
        if (rich_step) { while (rich_step * cap > ((size_t)1 << 26)) cap /= 2; }
        const size_t need = per_step * cap + WV_GCAP + part_f + rich_step * cap;
        if (need > h->wg_traj.capacity()) {
            HIPCHK(h, hipDeviceSynchronize());
            RESERVE(h, h->wg_traj, need);
        }
        WaveGradArgs wg;
        wg.traj = h->wg_traj; wg.traj_cap = cap; wg.hs_out = h->wg_traj + per_step * cap;
        wg.gpart = part_f ? h->wg_traj + per_step * cap + WV_GCAP : h->g_part;
        wg.lam_out = h->g_lam; wg.n_params = (int)h->n_params;
        wg.ys = h->nd.n_cond > 0 ? h->d_ys : nullptr;
        wg.rich = rich_step ? h->wg_traj + per_step * cap + WV_GCAP + part_f : nullptr;
        wg.lam1 = h->lam[0]; wg.lam2 = h->lam[1]; wg.lam3 = h->lam[2];
        Recorder rec;
        rec.wg = &wg;
        cnf_solve_stats sst{};
        PostHook ph{h->tmp_logpx, h->tmp_regs, h->d_sums, xs};
        SolveCall call{mode, B, h->U[0], eps, nullptr, opts, &sst, stream};
        call.rec = &rec; call.post = &ph; call.final_sync = false;
        if ((s = solve_core(h, call)) != CNF_OK) return s;
        if (rec.wg_submitted) {
            HIPCHK(h, launch_grad_finish(wg.gpart, grad, (int)h->n_params, waves, h->d_state, h->d_sums, h->lam[0], h->lam[1], h->lam[2],
                                         train ? 1 : 0, loss_dev, st));
            h->rec.backward_done(B, false);
            *done = true;
            return CNF_OK;
        }
        if (rec.wg_done) {
            HIPCHK(h, launch_grad_reduce(wg.gpart, grad, (int)h->n_params, waves, st));
            float* sums = loss_sums_host(h);
            HIPCHK(h, hipMemcpyAsync(sums, h->d_sums, 5 * sizeof(float), hipMemcpyDeviceToHost, st));
            HIPCHK(h, hipStreamSynchronize(st));
            h->last_hs = rec.hs;
            h->rec.backward_done(B, false);
            sst.launches += 1;
            if ((s = cnf_loss_from_sums(h, mode, sums, loss_out)) != CNF_OK) return s;
            if (stats) *stats = sst;
            *done = true;
        }
    }
    return CNF_OK;
}

// What the five gradient entry points begin with (cnf_loss_grad, cnf_loss_grad_test, cnf_inference_record, cnf_generate_record,
// cnf_loss_grad_submit): the call's checks in their one order, then room for B samples.  ptrs_ok: none of the pointers THIS
// entry point needs is null; width: the TrainMode pullback kernels must take the network; cw / gz0: the call packs per-sample
// cotangents / keeps the base draw (d_cw, d_gz0; grown behind a wait for the stream).
cnf_status cnfabi::grad_prologue(cnf_handle h, int mode, int B, bool ptrs_ok, const char* empty_batch, bool width, hipStream_t st,
                                bool cw, bool gz0) {
    cnf_status s = check_call(h, mode, B);
    if (s != CNF_OK) return s;
    if (!ptrs_ok) return fail(h, CNF_ERR_BAD_ARG, "null pointer");
    if (B < 1) return fail(h, CNF_ERR_BAD_SHAPE, empty_batch);
    if (width && !grad_supported(h->nd, grad_layout(h->nd))) return fail(h, CNF_ERR_UNSUPPORTED, "network too wide for the gradient kernels");
    if ((s = ensure_capacity(h, B)) != CNF_OK) return s;
    if ((s = ensure_grad_capacity(h, B)) != CNF_OK) return s;
    const size_t nw = cw ? (size_t)3 * B : 0, nz = gz0 ? (size_t)h->nd.n_in * B : 0;
    if (nw > h->d_cw.capacity() || nz > h->d_gz0.capacity()) {
        HIPCHK(h, hipStreamSynchronize(st));
        RESERVE(h, h->d_cw, (nw + 1023) & ~(size_t)1023);
        RESERVE(h, h->d_gz0, (nz + 1023) & ~(size_t)1023);
    }
    return CNF_OK;
}
static const char* const EMPTY_LOSS_BATCH = "the loss is a mean over the batch: B must be >= 1";

// The RECORDED solve of the gradient entry points, from u0: stage states in the trajectory store, the final state in g_US[1],
// the signed step sizes in last_hs.  A solve of more steps than the store has slots grows it and runs again.
// TestMode records in solve_stepwise (host-driven, one attempt at a time), the one place
// where a TestMode solve records: networks whose TestMode otherwise runs inside the fused step kernels (two layers, closed-form
// trace) take the generic right-hand side there.
cnf_status cnfabi::record_solve(cnf_handle h, int mode, const float* u0, const float* eps, int B, const cnf_solve_opts* opts, Recorder& rec,
                               cnf_solve_stats& sst, void* stream, PostHook* ph) {
    cnf_status s = CNF_OK;
    cnf_solve_opts ropts = *opts;
    if (mode == CNF_MODE_TEST && mfma_supported(h->mfma, h->nd, false, B)) ropts.kernel = CNF_KERNEL_GENERIC;
    for (;;) {
        if (ph) ph->launched = false;
        SolveCall call{mode, B, u0, eps, h->g_US[1], &ropts, &sst, stream};
        call.rec = &rec; call.post = ph;
        if ((s = solve_core(h, call)) != CNF_OK) return s;
        if (!rec.overflow) break;
        if ((s = traj_reserve(h, rec.n + 8)) != CNF_OK) return s;       // more steps than slots: grow, solve again
    }
    h->last_hs = rec.hs;
    return CNF_OK;
}

// The forward half of cnf_loss_grad (and cnf_inference_record in TrainMode): u0, the RECORDED solve -- stage states in the
// trajectory store, the final state in g_US[1] --, logpx / regs in tmp_logpx / tmp_regs and the five loss sums in d_sums.
static cnf_status train_forward(cnf_handle h, const float* xs, const float* eps, int B, const cnf_solve_opts* opts, Recorder& rec,
                                cnf_solve_stats& sst, void* stream) {
    const int mode = CNF_MODE_TRAIN;
    cnf_status s = CNF_OK;
    hipStream_t st = (hipStream_t)stream;
    const int n_in = h->nd.n_in, D = n_in + 3;
    // ---- forward: u0, recorded solve, loss ------------------------------------------------------
    // (as an inference does: u0 is assembled from the data columns and the post-processing and the five loss sums are formed
    // inside the one-launch solves -- the recording forms included --, behind the solve otherwise; the final state goes
    // straight to fsol where the kernel can write it there)
    float* fsol = h->g_US[1];
    PostHook ph{h->tmp_logpx, h->tmp_regs, h->d_sums, xs};
    if ((s = record_solve(h, mode, h->U[0], eps, B, opts, rec, sst, stream, &ph)) != CNF_OK) return s;
    if (!ph.launched) {                                    // (the one-attempt-at-a-time drivers leave it to the caller)
        enqueue_post(h, 1, h->last_state, ph, B, false, st);
        HIPCHK(h, hipGetLastError());
    }
    if (h->bd.kind) {                                      // the loss of a non-default base distribution: logpx and the sums afresh
        launch_base_post(n_in, D, h->bd, nullptr, fsol, nullptr, h->tmp_logpx, h->tmp_regs, B, h->d_sums, h->post_part,
                         sums_word<unsigned>(h, SUMS_POST_TICKET), st);
        HIPCHK(h, hipGetLastError());
    }
    return CNF_OK;
}

// d / d ys (cnf_set_grad_ys): room for the row sums S1 [B][dims[1]] and the result [B][n_cond] behind them.  Grow-only; like the
// other on-demand buffers it grows behind a wait for the stream, so the steady state allocates nothing.
static float* gy_result(cnf_handle h, int B) { return h->d_gy + (size_t)B * h->nd.dims[1]; }
static cnf_status ensure_gy(cnf_handle h, int B, hipStream_t st) {
    const size_t need = (size_t)B * ((size_t)h->nd.dims[1] + h->nd.n_cond);
    if (need > h->d_gy.capacity()) {
        HIPCHK(h, hipStreamSynchronize(st));
        RESERVE(h, h->d_gy, (need + 4095) & ~(size_t)4095);
    }
    return CNF_OK;
}

// The backward half of cnf_loss_grad (and cnf_inference_pullback in TrainMode): the discrete adjoint of the recorded steps `hs`
// (sizes; their stage states lie in the trajectory store, the final state in g_US[1]) into grad, d / d u(t0) into g_lam.
// The cotangent it starts from is one of three (Cotangent).  LOSS: of the loss -- three launch-wide scalars and
// k_final_cotangent / k_base_cotangent, the arithmetic cnf_loss_grad has always had.  ROWS = [4][B] (rows logpx, E, n, A):
// k_vjp_cotangent forms the terminal cotangent and packs the per-sample weights of the scalar rows into d_cw, which every
// pullback kernel then reads in place of the scalars.  SAMPLE (cnf_generate_pullback): the same per-sample pullback seeded by
// k_generate_cotangent instead.
namespace {
struct Cotangent {
    enum Kind { LOSS, ROWS, SAMPLE } kind;
    const float* rows;             // ROWS: [4][B]
    const float *z, *logq;         // SAMPLE: [B][n_in], [B]; one of them may be null
    bool per_sample() const { return kind != LOSS; }
};
}  // namespace
static const Cotangent COT_LOSS{Cotangent::LOSS, nullptr, nullptr, nullptr};
static cnf_status train_backward(cnf_handle h, const float* eps, int B, int kernel, const std::vector<float>& rec_hs, const Cotangent& cot,
                                 float* grad, hipStream_t st) {
    cnf_status s = CNF_OK;
    const NetDesc& nd = h->nd;
    const int n_in = nd.n_in, D = n_in + 3;
    const size_t n = (size_t)D * B;
    const GradLayout gl = grad_layout(nd);
    const AdjMfmaLayout am = adj_mfma_layout(nd, gl);
    // the pullback kernel follows the kernel choice of the solve: GENERIC -> VALU, otherwise MFMA when it fits
    const bool adj_mfma = kernel != CNF_KERNEL_GENERIC && adj_mfma_supported(nd, am);
    const int rec_n = (int)rec_hs.size();
    const float* cw = cot.per_sample() ? h->d_cw : nullptr;
    // d / d ys: the layer-1 segment of the AB rows of every run, summed per sample beside the run's contraction (gy_runs counts them)
    h->rec.backward_begins();
    const bool want_gy = h->grad_ys;
    int gy_runs = 0;
    if (want_gy && (s = ensure_gy(h, B, st)) != CNF_OK) return s;
    // ---- backward: discrete adjoint of the recorded steps ---------------------------------------
    // capacity is in samples of cap_B; with B <= cap_B at least grad_fsteps steps fit
    // (CNF_GRAD_FSTEPS=n: contract after every n steps instead -- measurements: fewer steps per contraction keep the factor rows
    // in the infinity cache, more amortise its launch)
    const int fsteps_env = cnf_switch<SW_GRAD_FSTEPS>();
    int fsteps = (int)std::min<size_t>(32, (size_t)h->grad_fsteps * h->grad_cap_B / (size_t)B);
    if (fsteps_env > 0 && fsteps_env < fsteps) fsteps = fsteps_env;
    int ksplit = 1, filed = 0;
    HIPCHK(h, hipMemsetAsync(h->g_part, 0, (size_t)GRAD_MAX_KSPLIT * h->n_params * sizeof(float), st));
    const float* fsol = h->g_US[1];
    switch (cot.kind) {
        case Cotangent::SAMPLE: launch_generate_cotangent(n_in, cot.z, cot.logq, h->g_lam, h->d_cw, B, st); HIPCHK(h, hipGetLastError()); break;
        case Cotangent::ROWS: launch_vjp_cotangent(nd, D, h->bd, 1, fsol, cot.rows, h->g_lam, h->d_cw, B, st); HIPCHK(h, hipGetLastError()); break;
        case Cotangent::LOSS:
            if (h->bd.kind) { launch_base_cotangent(nd, D, h->bd, h->lam[2], fsol, h->g_lam, B, st); HIPCHK(h, hipGetLastError()); }
            else HIPCHK(h, launch_final_cotangent(nd, h->lam[2], fsol, h->g_lam, B, st));
    }
    const float invB = 1.0f / (float)B;
    // constant scalar rows; with per-sample weights the kernels multiply cw[r][b] in where these scalars stand, so they are 1
    const float lam_l = cw ? 1.0f : invB, lam_E = cw ? 1.0f : h->lam[0] * invB, lam_n = cw ? 1.0f : h->lam[1] * invB;
    static const AdjTableau T = adj_tableau(tsit5_row);
    if (adj_mfma && adj3b_supported(nd) && h->mfma.d_img3b) {
        // The headline shape: the steps whose factor rows fit the arena in ONE launch on split-bf16 products (cnf_adj3b.hip;
        // the image is the forward kernels'), then one contraction over them -- 2 launches per run of steps instead of one
        // per step and one per run.
        if ((s = traj_reserve(h, rec_n)) != CNF_OK) return s;
        const int run = std::min(fsteps, ADJ3B_MAX_STEPS);
        for (int hi = rec_n - 1; hi >= 0; hi -= run) {
            const int lo = std::max(0, hi - run + 1), cnt = hi - lo + 1;
            Adj3bSteps M{};
            M.traj = h->traj; M.slot_stride = traj_slot_floats(h); M.n = n;
            M.step_hi = hi; M.step_lo = lo;
            for (int j = 0; j < cnt; ++j) M.hs[j] = rec_hs[hi - j];
            M.eps = eps; M.lam = h->g_lam; M.lam_out = h->g_lam;
            M.HS = h->g_HS; M.TS = h->g_TS; M.AB = h->g_AB; M.PB = h->g_PB;
            M.lam_l = lam_l; M.lam_E = lam_E; M.lam_n = lam_n;
            M.cw = cw;
            memcpy(M.bw, T.b, sizeof M.bw);
            memcpy(M.kc, T.kc, sizeof M.kc);
            M.B = B;
            if (adj3b_split(B, cnt)) {          // (batches that leave CUs idle: two launches, the parked state in between)
                const size_t need = adj3b_park_floats(B, cnt);
                if (need > h->d_park.capacity()) {
                    HIPCHK(h, hipStreamSynchronize(st));
                    if (h->d_park.reserve(need) != 0) (void)hipGetLastError();  // (no room for the parked state: null, one launch per run)
                }
                M.park = h->d_park;
            }
            HIPCHK(h, launch_adj3b(nd, gl, h->mfma.d_img3b, M, st));
            int ks, ch;
            grad_ksplit(nd, gl, 6 * cnt * B, &ks, &ch);
            if (ks > ksplit) ksplit = ks;
            HIPCHK(h, launch_wgrad(nd, gl, h->g_AB, h->g_PB, h->g_HS, h->g_TS, h->g_part, (int)h->n_params, 6 * cnt * B, ks, ch, st));
        }
    } else {
    // (MFMA pullback: the steps of a run are gathered and launched together -- as two launches over the whole run where the batch
    // leaves CUs idle, else one launch per step)
    int run0 = 0;                                          // first entry of the current run in h_steps
    if (adj_mfma && (size_t)rec_n > h->h_steps.capacity()) {      // (the pair grows together; h_steps is reserved last)
        HIPCHK(h, hipStreamSynchronize(st));
        h->d_steps.release(); h->h_steps.release();
        RESERVE(h, h->d_steps, (size_t)rec_n + 32);
        RESERVE(h, h->h_steps, (size_t)rec_n + 32);
    }
    for (int step = rec_n - 1; step >= 0; --step) {
        float* un;
        if ((s = traj_slot(h, step, &un)) != CNF_OK) return s;
        const float hs = rec_hs[step];
        // stage states: U_1 = u_n, U_2..U_6 were filed behind it by the forward pass
        const float* US[6];
        for (int i = 0; i < 6; ++i) US[i] = un + (size_t)i * n;
        AdjStepArgs S{};
        for (int i = 5; i >= 0; --i) {
            AdjArgs a{};
            a.P = h->d_params; a.PT = h->d_PT; a.ustage = US[i]; a.eps = eps;
            a.ys = nd.n_cond > 0 ? h->d_ys : nullptr;
            a.lam = h->g_lam;
            a.nw = 0;
            for (int m = i + 1; m < 6; ++m) { a.w[a.nw] = h->g_W[m]; a.wc[a.nw] = T.a[m][i]; ++a.nw; }
            for (int k = a.nw; k < 5; ++k) { a.w[k] = h->g_lam; a.wc[k] = 0.f; }     // unused slots: a readable array, weight 0
            a.cb = T.b[i]; a.hstep = hs;
            a.c_l = hs * T.b[i] * lam_l; a.c_E = hs * T.b[i] * lam_E; a.c_n = hs * T.b[i] * lam_n;
            a.cw = cw;
            a.w_out = h->g_W[i];
            // every stage evaluation files its factors behind the earlier ones: rows [slot B, (slot + 1) B)
            const size_t slot = (size_t)filed * 6 + i;
            a.HS = h->g_HS + slot * B * gl.sum_in; a.TS = h->g_TS + slot * B * gl.sum_in;
            a.AB = h->g_AB + slot * B * gl.sum_out; a.PB = h->g_PB + slot * B * gl.sum_out;
            a.B = B;
            if (adj_mfma) S.st[i] = a;
            else HIPCHK(h, launch_adj(nd, gl, a, st));
        }
        if (adj_mfma) {        // the six stage pullbacks and the lambda update of this step in ONE launch
            S.first = 5; S.last = 0; S.B = B; S.lam_update = 1; S.lam_out = h->g_lam;
            memcpy(S.kc, T.kc, sizeof S.kc);
            h->h_steps[rec_n - 1 - step] = S;
        } else {
            StageK ws{};
            ws.nk = 6;
            for (int i = 0; i < 6; ++i) ws.k[i] = h->g_W[i];
            HIPCHK(h, launch_lambda_update(h->g_lam, ws, (size_t)n_in * B, st));
        }
        // Wbar += sum over the filed stage evaluations and their samples: one contraction with K = 6 filed B
        if (++filed == fsteps || step == 0) {
            if (adj_mfma) {                                // the run's pullbacks
                const int cnt = filed;
                // (two launches per SUB-run of steps whose parked rows stay in the infinity cache -- measured at config 5's network:
                // whole runs of 10-22 steps, 0.2-0.8 GB of rows, cost 2 % at B = 256 and 6 % at 2048 against step by step)
                const size_t per_step = adj_mfma_scratch_floats(am, (size_t)B, 1);
                int nsub = (int)std::max<size_t>(1, std::min<size_t>((size_t)cnt, ((size_t)48 << 20) / (per_step * sizeof(float))));
                bool two = adj_mfma_run_split(nd, am, B, nsub);
                if (two) {
                    const size_t need = per_step * nsub;
                    if (need > h->d_sc.capacity()) {
                        HIPCHK(h, hipStreamSynchronize(st));
                        if (h->d_sc.reserve(need) != 0) { (void)hipGetLastError(); two = false; }   // (no room for the parked rows: one launch per step)
                    }
                }
                if (two) {
                    HIPCHK(h, hipMemcpyAsync(h->d_steps + run0, h->h_steps + run0, (size_t)cnt * sizeof(AdjStepArgs), hipMemcpyHostToDevice, st));
                    for (int j = 0; j < cnt; j += nsub)
                        HIPCHK(h, launch_adj_mfma_run(nd, gl, am, h->d_adj_img, h->d_steps + run0 + j, h->h_steps + run0 + j, std::min(nsub, cnt - j),
                                                      B, h->d_sc, st));
                } else {
                    for (int j = 0; j < cnt; ++j) HIPCHK(h, launch_adj_mfma_step(nd, gl, am, h->d_adj_img, h->h_steps[run0 + j], st));
                }
                run0 += cnt;
            }
            int ks, ch;
            grad_ksplit(nd, gl, 6 * filed * B, &ks, &ch);
            if (ks > ksplit) ksplit = ks;
            HIPCHK(h, launch_wgrad(nd, gl, h->g_AB, h->g_PB, h->g_HS, h->g_TS, h->g_part, (int)h->n_params,
                                   6 * filed * B, ks, ch, st));
            if (want_gy) HIPCHK(h, launch_cond_rowsum(nd, gl, am, h->g_AB, h->d_gy, B, 6 * filed, gy_runs++ == 0, st));
            filed = 0;
        }
    }
    }
    HIPCHK(h, launch_grad_reduce(h->g_part, grad, (int)h->n_params, ksplit, st));
    h->rec.backward_done(B, false);                        // (g_lam now holds d loss / d u(t0): cnf_grad_x)
    if (want_gy) {                                         // gy = W_1y' S1, once per pullback  (no run at all: no step, gy = 0)
        if (!gy_runs) HIPCHK(h, hipMemsetAsync(h->d_gy, 0, (size_t)B * nd.dims[1] * sizeof(float), st));
        HIPCHK(h, launch_cond_project(nd, h->d_params, h->d_gy, gy_result(h, B), B, st));
        h->rec.backward_done(B, true);                     // (cnf_grad_ys)
    }
    return CNF_OK;
}

// what the TrainMode pullback reads of the current parameters: their transpose and the padded weight images
// (pt_valid and img_valid stay two flags: the exact-trace kernels pack the images alone, ensure_adj_images)
static cnf_status ensure_pullback_params(cnf_handle h, hipStream_t st) {
    if (h->pt_valid) return CNF_OK;
    const GradLayout gl = grad_layout(h->nd);
    HIPCHK(h, launch_transpose_params(h->nd, h->d_params, h->d_PT, st));
    HIPCHK(h, launch_pack_adj_images(h->nd, gl, adj_mfma_layout(h->nd, gl), h->d_params, h->d_adj_img, st));
    h->pt_valid = true;
    return CNF_OK;
}

extern "C" cnf_status cnf_loss_grad(cnf_handle h, const float* xs, const float* eps, int B,
                                    const cnf_solve_opts* opts, float* loss_out, float* grad,
                                    cnf_solve_stats* stats, void* stream) {
    const int mode = CNF_MODE_TRAIN;
    hipStream_t st = (hipStream_t)stream;
    cnf_status s = grad_prologue(h, mode, B, xs && eps && opts && loss_out && grad, EMPTY_LOSS_BATCH, true, st);
    if (s != CNF_OK) return s;
    if ((s = ensure_pullback_params(h, st)) != CNF_OK) return s;

    if (!h->bd.kind && !h->grad_ys) {   // small batches of a small two-layer tanh network: everything in one launch (wave_loss_grad above)
        bool done = false;
        if ((s = wave_loss_grad(h, mode, xs, eps, B, opts, loss_out, grad, stats, stream, &done)) != CNF_OK || done) return s;
    }

    Recorder rec;
    cnf_solve_stats sst{};
    if ((s = train_forward(h, xs, eps, B, opts, rec, sst, stream)) != CNF_OK) return s;
    // (the five sums travel to the host behind the backward pass: the loss VALUE is not needed to start it)
    float* sums = loss_sums_host(h);
    HIPCHK(h, hipMemcpyAsync(sums, h->d_sums, 5 * sizeof(float), hipMemcpyDeviceToHost, st));

    if ((s = train_backward(h, eps, B, opts->kernel, rec.hs, COT_LOSS, grad, st)) != CNF_OK) return s;
    HIPCHK(h, hipStreamSynchronize(st));
    h->rec.begin(REC_LOSS, mode, B);                       // (cnf_base_logpdf_pullback: the final state stays in g_US[1])
    if ((s = cnf_loss_from_sums(h, mode, sums, loss_out)) != CNF_OK) return s;
    if (stats) *stats = sst;
    return CNF_OK;
}

// The forward half of cnf_loss_grad_test (and cnf_inference_record in TestMode): the recorded exact-trace solve -- u_n of every
// accepted step in the trajectory store, the final state in g_US[1] --, logpx in tmp_logpx, the loss sums in d_sums.
static cnf_status test_forward(cnf_handle h, const float* xs, int B, const cnf_solve_opts* opts, Recorder& rec, cnf_solve_stats& sst,
                               void* stream) {
    const int mode = CNF_MODE_TEST;
    cnf_status s = CNF_OK;
    hipStream_t st = (hipStream_t)stream;
    const NetDesc& nd = h->nd;
    const int n_in = nd.n_in, D = n_in + 1;
    float* u0 = h->g_US[0];
    launch_build_u0(xs, u0, nd.nvars, D, B, st);
    // (the recorded forward pass files u_n after every accepted step: record_solve)
    float* fsol = h->g_US[1];
    if ((s = record_solve(h, mode, u0, nullptr, B, opts, rec, sst, stream)) != CNF_OK) return s;
    launch_post(nd, 0, fsol, h->tmp_logpx, h->tmp_regs, B, st);
    if (h->bd.kind) {          // a non-default base distribution: its log-density, and its d loss / d z(t1) for k_adj_test
        launch_base_post(n_in, D, h->bd, nullptr, fsol, nullptr, h->tmp_logpx, h->tmp_regs, B, nullptr, nullptr, nullptr, st);
        launch_base_cotangent(nd, D, h->bd, 0.f, fsol, h->g_W[0], B, st);
    }
    launch_loss_sums(h->tmp_logpx, h->tmp_regs, B, h->d_sums, st);
    return CNF_OK;
}

// The backward half: k_adj_test (cnf_gradt.hip) over all recorded steps in one launch, then the sum of its partials.  LOSS: the
// cotangent of the loss (1 / B per sample); ROWS: k_vjp_cotangent leaves d / d z(t1) in g_W[0] and w_l = -cot_l in d_cw
// (rows E, n, A do not exist in TestMode: their cotangents are not read); SAMPLE: k_generate_cotangent leaves them instead.
static cnf_status test_backward(cnf_handle h, int B, const std::vector<float>& rec_hs, const Cotangent& cot, float* grad, hipStream_t st) {
    cnf_status s = CNF_OK;
    const NetDesc& nd = h->nd;
    const int rec_n = (int)rec_hs.size();
    h->rec.backward_begins();
    if (h->grad_ys && (s = ensure_gy(h, B, st)) != CNF_OK) return s;
    switch (cot.kind) {
        case Cotangent::SAMPLE: launch_generate_cotangent(nd.n_in, cot.z, cot.logq, h->g_W[0], h->d_cw, B, st); HIPCHK(h, hipGetLastError()); break;
        case Cotangent::ROWS: launch_vjp_cotangent(nd, nd.n_in + 1, h->bd, 0, h->g_US[1], cot.rows, h->g_W[0], h->d_cw, B, st); HIPCHK(h, hipGetLastError()); break;
        case Cotangent::LOSS: break;       // (test_forward has left the base's d loss / d z(t1) in g_W[0], if there is one)
    }
    // the step sizes to the device (behind the steps in the trajectory store's step-size array), scratch and partials of the kernel
    if ((s = traj_reserve(h, rec_n + 1)) != CNF_OK) return s;
    if (rec_n > 0) HIPCHK(h, hipMemcpyAsync(h->traj_hs, rec_hs.data(), (size_t)rec_n * sizeof(float), hipMemcpyHostToDevice, st));
    const int G = adj_test_workgroups(B);
    const size_t per_wg = adj_test_scratch_floats(nd) + h->n_params;
    if ((size_t)G * per_wg > h->d_gt.capacity()) {
        HIPCHK(h, hipStreamSynchronize(st));
        RESERVE(h, h->d_gt, (size_t)G * per_wg);
    }
    float* first;
    if ((s = traj_slot(h, 0, &first)) != CNF_OK) return s;
    AdjTestArgs ta{};
    ta.P = h->d_params; ta.traj = first; ta.slot_stride = traj_slot_floats(h); ta.hs = h->traj_hs; ta.nsteps = rec_n;
    ta.ys = nd.n_cond > 0 ? h->d_ys : nullptr; ta.lam_l = 1.0f / (float)B; ta.lam_out = h->g_lam;
    ta.lam_init = (cot.per_sample() || h->bd.kind) ? h->g_W[0] : nullptr;
    ta.w_l = cot.per_sample() ? h->d_cw : nullptr;
    ta.gy = h->grad_ys ? gy_result(h, B) : nullptr;
    ta.gpart = h->d_gt; ta.scratch = h->d_gt + (size_t)G * h->n_params; ta.scratch_per_wg = adj_test_scratch_floats(nd);
    ta.B = B; ta.n_params = (int)h->n_params;
    if (launch_adj_test(nd, ta, st) != hipSuccess) { (void)hipGetLastError(); return fail(h, CNF_ERR_UNSUPPORTED, "network too wide for the TestMode adjoint kernel"); }
    HIPCHK(h, launch_grad_reduce(h->d_gt, grad, (int)h->n_params, G, st));
    h->rec.backward_done(B, h->grad_ys);                   // (g_lam holds d loss / d z(t0): cnf_grad_x; k_adj_test left d / d ys: cnf_grad_ys)
    return CNF_OK;
}

// TestMode: loss(icnf, TestMode(), xs, ps, st) = -mean(logpx) (src/base_icnf.jl:489-497) and its gradient w.r.t. the flat
// parameters through the exact-trace solve -- what the reference's call tests and its benchmark suite differentiate besides
// the TrainMode loss (test/call_tests.jl `diff_loss` with omode = TestMode(); benchmark/benchmarks.jl:60-99 "AD-1-order" /
// "test").  Implemented for the networks k_solve_wave<GRAD> takes (two tanh layers or one, n_in <= 16, <= 64 hidden units,
// n_in + n_cond <= 16, B <= 8192); CNF_ERR_UNSUPPORTED otherwise.
extern "C" cnf_status cnf_loss_grad_test(cnf_handle h, const float* xs, int B, const cnf_solve_opts* opts, float* loss_out,
                                         float* grad, cnf_solve_stats* stats, void* stream) {
    const int mode = CNF_MODE_TEST;
    hipStream_t st = (hipStream_t)stream;
    cnf_status s = grad_prologue(h, mode, B, xs && opts && loss_out && grad, EMPTY_LOSS_BATCH, false, st);
    if (s != CNF_OK) return s;
    bool done = false;
    if (!h->bd.kind && !h->grad_ys && (s = wave_loss_grad(h, mode, xs, nullptr, B, opts, loss_out, grad, stats, stream, &done)) != CNF_OK) return s;
    if (done) return CNF_OK;
    // ---- every other network: the recorded exact-trace solve, then k_adj_test (cnf_gradt.hip) over all of its steps in one launch ----
    Recorder rec;
    cnf_solve_stats sst{};
    if ((s = test_forward(h, xs, B, opts, rec, sst, stream)) != CNF_OK) return s;
    float* sums = loss_sums_host(h);
    HIPCHK(h, hipMemcpyAsync(sums, h->d_sums, 5 * sizeof(float), hipMemcpyDeviceToHost, st));
    if ((s = test_backward(h, B, rec.hs, COT_LOSS, grad, st)) != CNF_OK) return s;
    HIPCHK(h, hipStreamSynchronize(st));
    h->rec.begin(REC_LOSS, mode, B);                       // (cnf_base_logpdf_pullback: the final state stays in g_US[1])
    if ((s = cnf_loss_from_sums(h, mode, sums, loss_out)) != CNF_OK) return s;
    if (stats) { *stats = sst; stats->launches += 2; }
    return CNF_OK;
}

// The host-array forms of the two: xs (and in TrainMode eps) through the handle's staging area, the gradient through g_grad.
static cnf_status loss_grad_staged(cnf_handle h, int mode, const float* xs, const float* eps, int B, const cnf_solve_opts* opts,
                                   float* loss_out, float* grad, cnf_solve_stats* stats) {
    const bool train = mode == CNF_MODE_TRAIN;
    cnf_status s = check_call(h, mode, B);
    if (s != CNF_OK) return s;
    if (!xs || !grad || (train && !eps)) return fail(h, CNF_ERR_BAD_ARG, "null pointer");
    if (B < 1) return fail(h, CNF_ERR_BAD_SHAPE, EMPTY_LOSS_BATCH);
    HIPCHK(h, hipSetDevice(h->device));
    if ((s = ensure_grad_capacity(h, B)) != CNF_OK) return s;
    const size_t nx = (size_t)h->nd.nvars * B, ne = train ? (size_t)h->nd.n_in * B : 0;
    if ((s = ensure_stage(h, nx + ne)) != CNF_OK) return s;
    float* x_d = h->stage;
    float* e_d = x_d + nx;
    HIPCHK(h, hipMemcpy(x_d, xs, nx * sizeof(float), hipMemcpyHostToDevice));
    if (train) HIPCHK(h, hipMemcpy(e_d, eps, ne * sizeof(float), hipMemcpyHostToDevice));
    s = train ? cnf_loss_grad(h, x_d, e_d, B, opts, loss_out, h->g_grad, stats, nullptr)
              : cnf_loss_grad_test(h, x_d, B, opts, loss_out, h->g_grad, stats, nullptr);
    if (s != CNF_OK) return s;
    HIPCHK(h, hipMemcpy(grad, h->g_grad, h->n_params * sizeof(float), hipMemcpyDeviceToHost));
    return CNF_OK;
}
extern "C" cnf_status cnf_loss_grad_host(cnf_handle h, const float* xs, const float* eps, int B, const cnf_solve_opts* opts,
                                         float* loss_out, float* grad, cnf_solve_stats* stats) {
    return loss_grad_staged(h, CNF_MODE_TRAIN, xs, eps, B, opts, loss_out, grad, stats);
}
extern "C" cnf_status cnf_loss_grad_test_host(cnf_handle h, const float* xs, int B, const cnf_solve_opts* opts, float* loss_out,
                                              float* grad, cnf_solve_stats* stats) {
    return loss_grad_staged(h, CNF_MODE_TEST, xs, nullptr, B, opts, loss_out, grad, stats);
}

// ---- differentiable inference: the two halves of cnf_loss_grad / cnf_loss_grad_test as entry points of their own -----------------
// cnf_inference_record is the forward half (the recorded solve; outputs as cnf_inference), cnf_inference_pullback the backward
// half for ANY cotangent of the four outputs: sum_b sum_r cot[r][b] d out_r[b] / d ps.  The samples are independent given the
// accepted steps, so the generalisation of the loss's pullback is exact: the three launch-wide scalars of the scalar rows become
// three floats per sample (k_vjp_cotangent packs them next to the general terminal cotangent; the pullback kernels read them
// through AdjArgs::cw / Adj3bSteps::cw / AdjTestArgs::w_l, null on every other call).
// k_solve_wave<GRAD>, the in-launch gradient of small networks, is NOT extended: it carries the cotangent of the loss only, so a
// recorded call on such a network takes the recorded solve and the MFMA / generic pullback, as a non-default basedist already does.
// Rows the handle does not integrate carry no cotangent: lambda1 = 0 -> E = 0 and cot_E is ignored, likewise lambda2 / n and
// lambda3 / A, and rows 1-3 in TestMode.  A caller who wants d E builds the model with lambda1 != 0.
extern "C" cnf_status cnf_inference_record(cnf_handle h, int mode, const float* xs, const float* eps, int B, const cnf_solve_opts* opts,
                                           float* logpx, float* regs, cnf_solve_stats* stats, void* stream) {
    const bool train = mode == CNF_MODE_TRAIN;
    hipStream_t st = (hipStream_t)stream;
    cnf_status s = grad_prologue(h, mode, B, xs && opts && logpx && regs && (!train || eps), "a recorded inference needs B >= 1", train, st, true);
    if (s != CNF_OK) return s;
    Recorder rec;
    cnf_solve_stats sst{};
    if (train) s = train_forward(h, xs, eps, B, opts, rec, sst, stream);
    else s = test_forward(h, xs, B, opts, rec, sst, stream);
    if (s != CNF_OK) return s;
    HIPCHK(h, hipMemcpyAsync(logpx, h->tmp_logpx, (size_t)B * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIPCHK(h, hipMemcpyAsync(regs, h->tmp_regs, (size_t)3 * B * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIPCHK(h, hipStreamSynchronize(st));
    h->rec.begin(REC_INFERENCE, mode, B, opts->kernel, train ? eps : nullptr);
    if (stats) *stats = sst;
    return CNF_OK;
}

// What the two pullbacks share: the record of `kind` at this batch size, or the entry point's refusal (which changes nothing);
// then the backward half of the record's mode for the cotangent given, enqueued on `st`.  A pullback that fails half way has
// overwritten part of the record: it is gone.
static cnf_status record_pullback(cnf_handle h, CnfRecKind kind, const Cotangent& cot, int B, float* grad, hipStream_t st, const char* refusal) {
    if (!h->rec.pullable(kind, B) || (size_t)h->last_hs.size() == 0 || !h->d_cw || (kind == REC_GENERATE && !h->d_gz0))
        return fail(h, CNF_ERR_BAD_ARG, refusal);
    HIPCHK(h, hipSetDevice(h->device));
    cnf_status s;
    const std::vector<float> hs = h->last_hs;
    if (h->rec.mode() == CNF_MODE_TRAIN) {
        if ((s = ensure_pullback_params(h, st)) != CNF_OK) return s;
        s = train_backward(h, h->rec.eps(), B, h->rec.kernel(), hs, cot, grad, st);
    } else {
        s = test_backward(h, B, hs, cot, grad, st);
    }
    if (s != CNF_OK) h->rec.pullback_failed();
    return s;
}

extern "C" cnf_status cnf_inference_pullback(cnf_handle h, const float* cot, int B, float* grad, void* stream) {
    if (!h) return CNF_ERR_BAD_ARG;
    if (!cot || !grad) return fail(h, CNF_ERR_BAD_ARG, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    const cnf_status s = record_pullback(h, REC_INFERENCE, Cotangent{Cotangent::ROWS, cot, nullptr, nullptr}, B, grad, st,
                                         "no recorded inference of a batch of this size: call cnf_inference_record first");
    if (s != CNF_OK) return s;
    HIPCHK(h, hipStreamSynchronize(st));
    return CNF_OK;
}

// ---- differentiable sampling: generate with the log-density of the sample, and its pullback -----------------------------------
// cnf_generate_record integrates u0 = [z0; 0] over the span the caller gives (reverse(tspan)) with the solve RECORDED, as
// cnf_inference_record does, and reads both outputs off the one final state: z = its rows 1..n_in and
// logq = logpdf(basedist, z0) + dlogp (sign +: the dlogp row integrates -tr J along the way the sample travels, `inference`
// subtracts what it gains on the way back).  cnf_generate_pullback is the discrete adjoint of those steps for any cotangent of
// (z, logq): the terminal cotangent is lam = cot_z on the state rows and +cot_logq on the dlogp row (k_generate_cotangent), zero
// on the E and n rows, and the pullback kernels are those of cnf_inference_pullback, unchanged -- signed step sizes included.
// d / d z0 is what they leave in g_lam plus cot_logq d logpdf(basedist, z0) / d z0 (k_generate_z0_grad).
extern "C" cnf_status cnf_generate_record(cnf_handle h, int mode, const float* z0, const float* eps, int B, const cnf_solve_opts* opts,
                                          float* z_out, float* logq, cnf_solve_stats* stats, void* stream) {
    const bool train = mode == CNF_MODE_TRAIN;
    hipStream_t st = (hipStream_t)stream;
    cnf_status s = grad_prologue(h, mode, B, z0 && opts && z_out && logq && (!train || eps), "a recorded sampling solve needs B >= 1", train, st,
                                 true, true);
    if (s != CNF_OK) return s;
    const int n_in = h->nd.n_in, D = rows_of(h, mode);
    const size_t nz = (size_t)n_in * B;
    // u0 = [z0; 0] in g_US[0] (not in the integrator's own U[0]: a one-launch solve that gives up is run again from it), and the
    // handle's copy of z0 for the pullback
    float* u0 = h->g_US[0];
    HIPCHK(h, hipMemsetAsync(u0, 0, (size_t)D * B * sizeof(float), st));
    HIPCHK(h, hipMemcpy2DAsync(u0, (size_t)D * sizeof(float), z0, (size_t)n_in * sizeof(float), (size_t)n_in * sizeof(float), (size_t)B,
                               hipMemcpyDeviceToDevice, st));
    HIPCHK(h, hipMemcpyAsync(h->d_gz0, z0, nz * sizeof(float), hipMemcpyDeviceToDevice, st));
    Recorder rec;
    cnf_solve_stats sst{};
    if ((s = record_solve(h, mode, u0, train ? eps : nullptr, B, opts, rec, sst, stream)) != CNF_OK) return s;
    launch_generate_post(n_in, D, h->bd, h->g_US[1], h->d_gz0, z_out, logq, B, st);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(st));
    h->rec.begin(REC_GENERATE, mode, B, opts->kernel, train ? eps : nullptr);      // (and no cnf_grad_x / cnf_grad_ys any more)
    if (stats) { *stats = sst; stats->launches += 1; }
    return CNF_OK;
}

extern "C" cnf_status cnf_generate_pullback(cnf_handle h, const float* cot_z, const float* cot_logq, int B, float* grad, float* grad_z0,
                                            void* stream) {
    if (!h) return CNF_ERR_BAD_ARG;
    if (!grad) return fail(h, CNF_ERR_BAD_ARG, "null pointer");
    if (!cot_z && !cot_logq) return fail(h, CNF_ERR_BAD_ARG, "both cotangents are null");
    hipStream_t st = (hipStream_t)stream;
    const cnf_status s = record_pullback(h, REC_GENERATE, Cotangent{Cotangent::SAMPLE, nullptr, cot_z, cot_logq}, B, grad, st,
                                         "no recorded sampling solve of a batch of this size: call cnf_generate_record first");
    if (s != CNF_OK) return s;
    h->rec.sampling_pullback_done();                       // (g_lam is d / d u(t_start) of a SAMPLING solve: cnf_grad_x is not defined for it)
    if (grad_z0) {
        launch_generate_z0_grad(h->nd.n_in, h->bd, h->g_lam, cot_logq, h->d_gz0, grad_z0, B, st);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipStreamSynchronize(st));
    return CNF_OK;
}

// ---- a learnable base distribution: the gradient w.r.t. mean and chol (include/cnfhip_basegrad.h, cnf_basegrad.hip) -------------
// Both entry points are one batch contraction and a tail, enqueued on the caller's stream; the handle's buffer for them grows
// behind a wait for the device and is cleared then (its ticket words must be zero before the first launch; their region does
// not depend on the kind of the base, cnf_basegrad_plan.h, so a change of kind on a live handle finds them zero as well).
static cnf_status base_grad_buffer(cnf_handle h, int B, BaseGradPlan& plan, hipStream_t st) {
    plan = base_grad_plan(h->nd.n_in, h->bd.kind, B);
    if (plan.ntiles > 65535) return fail(h, CNF_ERR_UNSUPPORTED, "base distribution too large for the gradient kernel's grid");
    if (plan.floats > h->d_bg.capacity()) {
        HIPCHK(h, hipDeviceSynchronize());                 // (an earlier pullback on ANY stream may still read the old buffer)
        RESERVE(h, h->d_bg, (plan.floats + 4095) & ~(size_t)4095);
        HIPCHK(h, hipMemsetAsync(h->d_bg, 0, h->d_bg.capacity() * sizeof(float), st));
    }
    return CNF_OK;
}

extern "C" cnf_status cnf_base_logpdf_pullback(cnf_handle h, const float* w, int B, float* g_mean, float* g_chol, void* stream) {
    if (!h) return CNF_ERR_BAD_ARG;
    if (!w || !g_mean || !g_chol) return fail(h, CNF_ERR_BAD_ARG, "null pointer");
    if (h->bd.kind == 0) return fail(h, CNF_ERR_BAD_ARG, "the default base distribution has no mean or chol to differentiate");
    const float* src = nullptr;
    int stride = 0;
    switch (h->rec.base_source(B)) {
        case CnfRecord::SRC_Z0: src = h->d_gz0; stride = h->nd.n_in; break;
        case CnfRecord::SRC_FINAL_STATE: src = h->g_US[1]; stride = rows_of(h, h->rec.mode()); break;
        case CnfRecord::SRC_NONE: break;
    }
    if (!src) return fail(h, CNF_ERR_BAD_ARG, "no recorded solve of a batch of this size: call cnf_inference_record or cnf_generate_record first");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    BaseGradPlan plan;
    const cnf_status s = base_grad_buffer(h, B, plan, st);
    if (s != CNF_OK) return s;
    HIPCHK(h, launch_base_logpdf_pullback(h->nd.n_in, h->bd, src, stride, w, B, h->d_bg, plan, g_mean, g_chol, st));
    return CNF_OK;
}

extern "C" cnf_status cnf_base_sample_pullback(cnf_handle h, const float* normals, const float* g_z0, int B, float* g_mean,
                                               float* g_chol, void* stream) {
    if (!h) return CNF_ERR_BAD_ARG;
    if (!normals || !g_z0 || !g_mean || !g_chol) return fail(h, CNF_ERR_BAD_ARG, "null pointer");
    if (h->bd.kind == 0) return fail(h, CNF_ERR_BAD_ARG, "the default base distribution has no mean or chol to differentiate");
    if (B < 1) return fail(h, CNF_ERR_BAD_ARG, "B must be >= 1");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    BaseGradPlan plan;
    const cnf_status s = base_grad_buffer(h, B, plan, st);
    if (s != CNF_OK) return s;
    HIPCHK(h, launch_base_sample_pullback(h->nd.n_in, h->bd.kind, normals, g_z0, B, h->d_bg, plan, g_mean, g_chol, st));
    return CNF_OK;
}

// ---- submitted gradients: a training loop that never waits for the GPU ---------------------------------------------------------
// cnf_loss_grad_submit enqueues what cnf_loss_grad (TrainMode) / cnf_loss_grad_test (TestMode) compute -- solve, loss, discrete
// adjoint, the sum of the partials -- and returns; the loss (one float) and the gradient are left in DEVICE memory, stream-
// ordered, for whatever the caller enqueues next (the optimiser's update, then cnf_set_params_async with the new parameters and
// the next submission).  cnf_loss_grad_collect (oldest first; the queue is the one of cnf_inference_submit: at most three in
// flight, all on one stream) reports how the launch ended; a launch that gave up has delivered ZEROS and a NaN loss and is
// reported as CNF_ERR_UNSUPPORTED.  Only where the gradient runs in the launch of the solve (k_solve_wave<GRAD>); otherwise
// CNF_ERR_UNSUPPORTED at once, and the caller uses the synchronous call.
extern "C" cnf_status cnf_loss_grad_submit(cnf_handle h, int mode, const float* xs, const float* eps, int B, const cnf_solve_opts* opts,
                                           float* loss_dev, float* grad, void* stream) {
    if (!h) return CNF_ERR_BAD_ARG;
    if (h->submitted.size() >= 3) return fail(h, CNF_ERR_BAD_ARG, "three launches are submitted already: collect one first");
    // (the gradient inside the solve's launch carries the N(0, I) cotangent: refused at once, nothing is enqueued)
    if (h->bd.kind) return fail(h, CNF_ERR_UNSUPPORTED, "no in-launch gradient with a non-default base distribution: use cnf_loss_grad");
    if (h->grad_ys) return fail(h, CNF_ERR_UNSUPPORTED, "no in-launch gradient w.r.t. ys (cnf_set_grad_ys is on): use cnf_loss_grad");
    h->collecting = true;
    cnf_status s = grad_prologue(h, mode, B, xs && opts && loss_dev && grad && (mode != CNF_MODE_TRAIN || eps), EMPTY_LOSS_BATCH, false,
                                 (hipStream_t)stream);
    bool done = false;
    if (s == CNF_OK) {
        h->submitting = true; h->sub_taken = false;
        s = wave_loss_grad(h, mode, xs, eps, B, opts, nullptr, grad, nullptr, stream, &done, loss_dev);
        h->submitting = false;
    }
    h->collecting = false;
    if (s != CNF_OK) return s;
    if (!done) return fail(h, CNF_ERR_UNSUPPORTED, "no in-launch gradient for this network / batch: use cnf_loss_grad");
    return CNF_OK;
}

extern "C" cnf_status cnf_loss_grad_collect(cnf_handle h, cnf_solve_stats* stats) { return cnf_inference_collect(h, stats); }

// cnf_set_params without the host waits: the copy (and the packing launches) are enqueued on `stream` and the call returns.
// For a caller whose every launch on this handle goes to that one stream (then stream order is all the synchronisation there
// is to do): the parameter update between two submitted gradients.
extern "C" cnf_status cnf_set_params_async(cnf_handle h, const float* flat_dev, size_t n, void* stream) {
    cnf_status ss = params_check(h, flat_dev, n);
    if (ss != CNF_OK) return ss;
    hipStream_t s = (hipStream_t)stream;
    if (g_submitted_inflight > 0 && g_submitted_stream != s)
        return fail(h, CNF_ERR_BAD_ARG, "cnf_set_params_async: launches are in flight on another stream");
    // A submitted INFERENCE that gives up is run again by its collect call -- with the parameters (and conditioning) the handle
    // holds then.  Changing them under it would silently change its result: such submissions are settled first (host wait).
    // Submitted gradients are not re-run (a launch that gave up reports CNF_ERR_UNSUPPORTED), so they stay in flight.
    for (const auto& sub : h->submitted)
        if (sub.launched && !sub.grad) { if ((ss = settle_submitted(h)) != CNF_OK) return ss; break; }
    HIPCHK(h, hipMemcpyAsync(h->d_params, flat_dev, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    return params_uploaded(h, s, PARAMS_NO_WAIT);
}

// d loss / d xs of the last cnf_loss_grad call: the adjoint state at t0 is d loss / d u(t0), and u0 = (xs; zeros) -- its first
// nvars rows, [B][nvars] as xs is laid out.  (The backward sweep leaves it in g_lam; nothing is recomputed.)
extern "C" cnf_status cnf_grad_x(cnf_handle h, float* gx, int B, void* stream) {
    if (!h || !gx) return CNF_ERR_BAD_ARG;
    if (!h->rec.grad_x_ok(B) || !h->g_lam) return fail(h, CNF_ERR_BAD_ARG, "cnf_grad_x: no gradient of a batch of this size has been computed");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpy2DAsync(gx, (size_t)h->nd.nvars * sizeof(float), h->g_lam, (size_t)h->nd.n_in * sizeof(float),
                               (size_t)h->nd.nvars * sizeof(float), (size_t)B, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return CNF_OK;
}

// The switch of the gradient w.r.t. the conditioning inputs: plain host state, nothing is invalidated.
extern "C" cnf_status cnf_set_grad_ys(cnf_handle h, int enable) {
    if (!h) return CNF_ERR_BAD_ARG;
    if (h->nd.n_cond <= 0) return fail(h, CNF_ERR_BAD_ARG, "cnf_set_grad_ys: the model has no conditioning inputs");
    h->grad_ys = enable != 0;
    return CNF_OK;
}

// d / d ys of the last gradient call, [B][n_cond] as cnf_set_cond takes ys (left behind by k_cond_project / k_adj_test).
extern "C" cnf_status cnf_grad_ys(cnf_handle h, float* gy, int B, void* stream) {
    if (!h || !gy) return CNF_ERR_BAD_ARG;
    if (!h->rec.grad_ys_ok(B) || !h->d_gy)
        return fail(h, CNF_ERR_BAD_ARG, "cnf_grad_ys: no gradient of a batch of this size has been computed with cnf_set_grad_ys on");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(gy, gy_result(h, B), (size_t)B * h->nd.n_cond * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return CNF_OK;
}

extern "C" int cnf_grad_steps(cnf_handle h, float* hs, int cap) {
    return h ? copy_steps(true, h->last_hs, h->last_hs, hs, nullptr, cap) : -1;
}

