// k_tangent_wave -- the TANGENT of a finished solve of a small two-layer network: R directions (dps, dx) pushed forward through
// the Tsit5 steps the solve accepted, one WAVE per (16-sample tile, direction), nothing but registers.
//
// What the reference runs here: `DifferentiationInterface.gradient(diff_loss, AutoEnzyme(mode = Forward), ps | xs)` in every
// block of test/call_tests.jl (:32-66, :239-252) -- n_params (or nvars B) pushforwards of the loss through inference_prob /
// base_sol / inference_sol (src/base_icnf.jl:266-286, :137-143, :167-189) and their sampling counterparts (:358-380, :202-211).
//
// As everywhere in this library the derivative is the one of the DISCRETE map through the accepted steps: the step sizes are
// constants.  So the tangent solve has no controller, hence no error norm, hence nothing for the tiles to agree on: there is
// no meeting, no poll, no atomic and no LDS in this kernel, and its only loop is bounded by the attempt count the solve left in
// device memory, read once.  The state u is integrated again beside its tangent (six evaluations per accepted step, FSAL), with
// the gradient form's tanh (tanh_grad), so that tangent and adjoint differentiate the same arithmetic.
//
// Per evaluation (a1 = W1 z + b1, h1 = s(a1), d1 = s', dd1 = s''; the same for layer 2; g2 = eps d2; D. = the tangent):
//   Da1 = W1 Dz + DW1 z + Db1     Dh1 = d1 Da1     Dd1 = dd1 Da1
//   Da2 = W2 Dh1 + DW2 h1 + Db2   Dzdot = d2 Da2   Dd2 = dd2 Da2
//   VJP mode:   Dtb1 = W2' (eps Dd2) + DW2' g2;  Dpb1 = Dtb1 d1 + tb1 Dd1;  D(eps'J) = W1' Dpb1 + DW1' pb1
//               Dldot = -eps . D(eps'J);  Dn = (eps'J) . D(eps'J) / |eps'J|
//   JVP mode:   the product rule on J eps = d2 (W2 (d1 (W1 eps)));  Dldot = -eps . D(J eps);  Dn = (J eps) . D(J eps) / |J eps|
//   TestMode:   the product rule on tr J = d1' (C d2), C = W1 .* W2':  DC = DW1 .* W2' + W1 .* DW2'
//   DE = zdot . Dzdot / |zdot|;  DE, Dn are 0 where the norm is 0 (the backward sweep's convention, cnf_wave.hip).
// Weights AND weight tangents are MFMA A fragments held for the whole launch, in the layout of k_solve_wave; the products, the
// lane sums and the stage table are that kernel's own (cnf_wave_dev.h).
#include "cnf_tangent.h"
#include "cnf_wave_dev.h"

namespace {

constexpr int TG_VJP = 0, TG_JVP = 1, TG_TEST = 2;

// ENS (cnf_inference_jvp_many / cnf_generate_jvp_many, include/cnfhip_ensemble_jvp.h): M independent members in one launch, the
// grid (tiles, R, M).  Everything a launch has ONE of, a member has its own copy of, at the strides of TangentEns: the prologue
// moves the input pointers on to the member's copy -- scalar arithmetic on the kernel arguments and the block index alone -- and
// the body behind it is the single model's; the trace rows are indexed by member in the step loop and the outputs move on at
// the stores (see there).  The guard is the member's own: it reads the member's own StepState.  `counts`: a member's
// own batch size; tiles at or beyond ceil(counts[m] / 16) leave at once, no column at or behind the count is read or written,
// and the row strides of the [R][4][B] / [R][B][rows] arrays stay the launch's B.  The other instantiations take an empty third
// argument and are the code they were.
struct TangentNoEns {};
template <bool ENS> struct TangentEnsArg { typedef TangentNoEns type; };
template <> struct TangentEnsArg<true> { typedef TangentEns type; };

template <int NI, int NH, int MODE, bool ID2, bool ENS = false>
__global__ void __launch_bounds__(64) k_tangent_wave(const TangentArgs a_, const WvTab tab, const typename TangentEnsArg<ENS>::type en) {
    constexpr bool TRAIN = MODE != TG_TEST;
    const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
    const int wid = (int)blockIdx.x, dir = (int)blockIdx.y;
    TangentArgs a = a_;
    int nlive = a.B;                                       // the columns that exist (ENS with counts: the member's own)
    if constexpr (ENS) {
        const size_t mb = (size_t)blockIdx.z;
        a.P += mb * en.p_stride;
        if (a.dP) a.dP += mb * en.dp_stride;
        if (a.eps) a.eps += mb * en.eps_stride;
        a.x += mb * en.x_stride;
        if (a.dX) a.dX += mb * en.dx_stride;
        a.st += mb;
        if (en.counts) {
            nlive = en.counts[mb];
            if (wid >= ((nlive + 15) >> 4)) return;
        }
    }
    // ---- the guard: the solve's own final state.  Nothing is written for a solve that gave up (n_partials < 0), did not reach
    // t1, went non-finite, or made more attempts than the trace holds; the count is read here, once. ----
    const int s_done = __builtin_amdgcn_readfirstlane(a.st->done), s_nonf = __builtin_amdgcn_readfirstlane(a.st->nonfinite);
    const int s_part = __builtin_amdgcn_readfirstlane(a.st->n_partials);
    const int s_att = __builtin_amdgcn_readfirstlane(a.st->naccept) + __builtin_amdgcn_readfirstlane(a.st->nreject);
    const int natt = a.n_rows >= 0 ? a.n_rows : s_att;
    if (!s_done || s_nonf || s_part < 0 || natt > a.trace_cap) return;

    const NetDesc& nd = a.nd;
    const int n_in = nd.n_in, nh = nd.dims[1];
    const float* P = a.P;
    // (an APPENDED identity layer lives behind the parameters: it has no direction)
    const float* dP = a.dP ? a.dP + (size_t)dir * (size_t)a.n_params : nullptr;
    const bool d2nd = dP != nullptr && !nd.id2;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

    // ---- weights and their tangents as A operands (k_solve_wave's layout: lane (q, i), k-step j of input tile kt ->
    // M[16 m + i][16 kt + 4 q + j]) ----
    constexpr bool REV = MODE == TG_VJP, CL = MODE == TG_TEST;
    float fW1[NH][NI][4], fW2[NI][NH][4], gW1[NH][NI][4], gW2[NI][NH][4];
    float fW2T[REV ? NH : 1][NI][4], fW1T[REV ? NI : 1][NH][4], gW2T[REV ? NH : 1][NI][4], gW1T[REV ? NI : 1][NH][4];
    float fC[CL ? NH : 1][NI][4], gC[CL ? NH : 1][NI][4];
    auto w1 = [&](const float* p, int o, int k) { return (p && o < nh && k < n_in) ? p[nd.w_off[0] + o + (size_t)k * nh] : 0.f; };
    auto w2 = [&](const float* p, int o, int k) { return (p && o < n_in && k < nh) ? p[nd.w_off[1] + o + (size_t)k * n_in] : 0.f; };
    const float* dP2 = d2nd ? dP : nullptr;
#pragma unroll
    for (int m = 0; m < NH; ++m)
#pragma unroll
        for (int kt = 0; kt < NI; ++kt)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int o = 16 * m + c, k = 16 * kt + 4 * q + j;
                fW1[m][kt][j] = w1(P, o, k); gW1[m][kt][j] = w1(dP, o, k);
                if (REV) { fW2T[m][kt][j] = w2(P, k, o); gW2T[m][kt][j] = w2(dP2, k, o); }
                if (CL) {
                    fC[m][kt][j] = w1(P, o, k) * w2(P, k, o);
                    gC[m][kt][j] = w1(dP, o, k) * w2(P, k, o) + w1(P, o, k) * w2(dP2, k, o);
                }
            }
#pragma unroll
    for (int m = 0; m < NI; ++m)
#pragma unroll
        for (int kt = 0; kt < NH; ++kt)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int o = 16 * m + c, k = 16 * kt + 4 * q + j;
                fW2[m][kt][j] = w2(P, o, k); gW2[m][kt][j] = w2(dP2, o, k);
                if (REV) { fW1T[m][kt][j] = w1(P, k, o); gW1T[m][kt][j] = w1(dP, k, o); }
            }
    // biases and their tangents in the accumulator layout (rows 16 m + 4 q + j)
    const int smp = wid * 16 + c;
    const bool live = smp < nlive;                         // a column at or behind B is neither read nor written
    const size_t sb = live ? (size_t)smp : 0;
    f32x4 b1v[NH], gb1[NH], b2v[NI], gb2[NI], rmask[NI];
#pragma unroll
    for (int m = 0; m < NH; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = 16 * m + 4 * q + j;
            b1v[m][j] = r < nh ? P[nd.b_off[0] + r] : 0.f;
            gb1[m][j] = (dP && r < nh) ? dP[nd.b_off[0] + r] : 0.f;
        }
#pragma unroll
    for (int m = 0; m < NI; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = 16 * m + 4 * q + j;
            b2v[m][j] = r < n_in ? P[nd.b_off[1] + r] : 0.f;
            gb2[m][j] = (dP2 && r < n_in) ? dP2[nd.b_off[1] + r] : 0.f;
            rmask[m][j] = r < n_in ? 1.f : 0.f;
        }

    // ---- state and tangent: z rows (u, k1..k7) twice, the probe rows, ONE scalar tangent row per lane group (q = 0: dlogp,
    // 1: E, 2: n; the scalar rows themselves feed nothing) ----
    f32x4 uz[NI], kz[7][NI], tu[NI], tk[7][NI], ep[NI];
    float tus = 0.f, tks[7];
    float z0dz0 = 0.f;                                     // sampling: z0 . Dz0
    const int xrows = a.sampling ? n_in : nd.nvars;
    const float* dXr = a.dX ? a.dX + (size_t)dir * (size_t)a.B * (size_t)xrows : nullptr;
#pragma unroll
    for (int m = 0; m < NI; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = 16 * m + 4 * q + j;
            const bool ok = live && r < xrows;
            uz[m][j] = ok ? a.x[sb * xrows + r] : 0.f;     // u0 = (xs; 0)  |  (z0; 0)
            tu[m][j] = (ok && dXr) ? dXr[sb * xrows + r] : 0.f;
            ep[m][j] = (TRAIN && live && r < n_in) ? a.eps[sb * n_in + r] : 0.f;
            z0dz0 = fmaf(uz[m][j], tu[m][j], z0dz0);
#pragma unroll
            for (int s = 0; s < 7; ++s) { kz[s][m][j] = 0.f; tk[s][m][j] = 0.f; }
        }
#pragma unroll
    for (int s = 0; s < 7; ++s) tks[s] = 0.f;
    if (a.sampling) z0dz0 = wv_quad_sum(z0dz0);

    // h = s(x), d = s', dd = s'' for the gradient form's tanh (the identity of an ID2 second layer compiled out)
    auto act3 = [&](const f32x4& pre, f32x4& h, f32x4& d, f32x4& dd, bool second) __attribute__((always_inline)) {
        if (ID2 && second) {
            h = pre; d = f32x4{1.f, 1.f, 1.f, 1.f}; dd = zero4;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) { h[j] = tanh_grad(pre[j]); d[j] = fmaf(-h[j], h[j], 1.f); dd[j] = -2.f * h[j] * d[j]; }
        }
    };
    // ---- one evaluation of augmented_f and of its tangent at (z, Dz) -> (zdot, Dzdot, this lane group's scalar tangent) ----
    auto rhs = [&](const f32x4 (&z)[NI], const f32x4 (&dz)[NI], f32x4 (&zd)[NI], f32x4 (&dzd)[NI], float& dsd) {
        f32x4 h1[NH], d1[NH], th1[NH], td1[NH];
#pragma unroll
        for (int m = 0; m < NH; ++m) {
            f32x4 acc = b1v[m], tac = gb1[m];
#pragma unroll
            for (int kt = 0; kt < NI; ++kt) {
                acc = mm4(fW1[m][kt], z[kt], acc);
                tac = mm4(fW1[m][kt], dz[kt], tac);
                tac = mm4(gW1[m][kt], z[kt], tac);
            }
            f32x4 dd;
            act3(acc, h1[m], d1[m], dd, false);
            th1[m] = d1[m] * tac; td1[m] = dd * tac;
        }
        f32x4 d2[NI], td2[NI];
        float e2 = 0.f, ze = 0.f;
#pragma unroll
        for (int m = 0; m < NI; ++m) {
            f32x4 acc = b2v[m], tac = gb2[m];
#pragma unroll
            for (int kt = 0; kt < NH; ++kt) {
                acc = mm4(fW2[m][kt], h1[kt], acc);
                tac = mm4(fW2[m][kt], th1[kt], tac);
                tac = mm4(gW2[m][kt], h1[kt], tac);
            }
            f32x4 h2, dv, dd;
            act3(acc, h2, dv, dd, true);
            zd[m] = h2 * rmask[m];
            d2[m] = dv * rmask[m];
            dzd[m] = dv * tac * rmask[m];
            td2[m] = dd * tac * rmask[m];
#pragma unroll
            for (int j = 0; j < 4; ++j) { e2 = fmaf(zd[m][j], zd[m][j], e2); ze = fmaf(zd[m][j], dzd[m][j], ze); }
        }
        float dl = 0.f, n2 = 0.f, ne = 0.f;
        if (MODE == TG_VJP) {
            f32x4 g2[NI], tg2[NI], pb1[NH], tpb1[NH];
#pragma unroll
            for (int m = 0; m < NI; ++m) { g2[m] = ep[m] * d2[m]; tg2[m] = ep[m] * td2[m]; }
#pragma unroll
            for (int m = 0; m < NH; ++m) {
                f32x4 acc = zero4, tac = zero4;
#pragma unroll
                for (int kt = 0; kt < NI; ++kt) {
                    acc = mm4(fW2T[m][kt], g2[kt], acc);
                    tac = mm4(fW2T[m][kt], tg2[kt], tac);
                    tac = mm4(gW2T[m][kt], g2[kt], tac);
                }
                pb1[m] = acc * d1[m];
                tpb1[m] = tac * d1[m] + acc * td1[m];
            }
#pragma unroll
            for (int m = 0; m < NI; ++m) {
                f32x4 eJ = zero4, teJ = zero4;
#pragma unroll
                for (int kt = 0; kt < NH; ++kt) {
                    eJ = mm4(fW1T[m][kt], pb1[kt], eJ);
                    teJ = mm4(fW1T[m][kt], tpb1[kt], teJ);
                    teJ = mm4(gW1T[m][kt], pb1[kt], teJ);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) { dl = fmaf(teJ[j], ep[m][j], dl); n2 = fmaf(eJ[j], eJ[j], n2); ne = fmaf(eJ[j], teJ[j], ne); }
            }
        } else if (MODE == TG_JVP) {
            f32x4 t1[NH], tt1[NH];
#pragma unroll
            for (int m = 0; m < NH; ++m) {
                f32x4 acc = zero4, tac = zero4;
#pragma unroll
                for (int kt = 0; kt < NI; ++kt) { acc = mm4(fW1[m][kt], ep[kt], acc); tac = mm4(gW1[m][kt], ep[kt], tac); }
                t1[m] = acc * d1[m];
                tt1[m] = tac * d1[m] + acc * td1[m];
            }
#pragma unroll
            for (int m = 0; m < NI; ++m) {
                f32x4 acc = zero4, tac = zero4;
#pragma unroll
                for (int kt = 0; kt < NH; ++kt) {
                    acc = mm4(fW2[m][kt], t1[kt], acc);
                    tac = mm4(fW2[m][kt], tt1[kt], tac);
                    tac = mm4(gW2[m][kt], t1[kt], tac);
                }
                const f32x4 t2 = acc * d2[m], tt2 = tac * d2[m] + acc * td2[m];
#pragma unroll
                for (int j = 0; j < 4; ++j) { dl = fmaf(tt2[j], ep[m][j], dl); n2 = fmaf(t2[j], t2[j], n2); ne = fmaf(t2[j], tt2[j], ne); }
            }
        } else {                                           // exact trace d1' (C d2)
#pragma unroll
            for (int m = 0; m < NH; ++m) {
                f32x4 acc = zero4, tac = zero4;
#pragma unroll
                for (int kt = 0; kt < NI; ++kt) {
                    acc = mm4(fC[m][kt], d2[kt], acc);
                    tac = mm4(fC[m][kt], td2[kt], tac);
                    tac = mm4(gC[m][kt], d2[kt], tac);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) { dl = fmaf(td1[m][j], acc[j], dl); dl = fmaf(d1[m][j], tac[j], dl); }
            }
        }
        dl = wv_quad_sum(dl);
        if (TRAIN) {
            e2 = wv_quad_sum(e2); ze = wv_quad_sum(ze); n2 = wv_quad_sum(n2); ne = wv_quad_sum(ne);
            const float num = q == 1 ? ze : ne, den2 = q == 1 ? (nd.norm_z ? e2 : 0.f) : (nd.norm_j ? n2 : 0.f);
            const float tn = den2 > 0.f ? num / __builtin_amdgcn_sqrtf(den2) : 0.f;
            dsd = q == 0 ? -dl : (q < 3 ? tn : 0.f);
        } else {
            dsd = q == 0 ? -dl : 0.f;
        }
    };

    // ---- k1 = f(u0), then the accepted steps in the solve's order with the solve's signed step sizes ----
    rhs(uz, tu, kz[0], tk[0], tks[0]);
    f32x4 zt[NI], tzt[NI];
#pragma unroll
    for (int m = 0; m < NI; ++m) { zt[m] = zero4; tzt[m] = zero4; }
    for (int it = 0; it < natt; ++it) {
        // (ENS: the member's rows are indexed here -- a trace pointer moved on in the prologue and held across the loop costs
        // the 64-hidden-unit VJP form a scratch frame)
        const float* tr = a.trace + 4 * ((size_t)it + (ENS ? (size_t)blockIdx.z * (size_t)a.trace_cap : (size_t)0));
        const float hstep = uni(tr[1]);
        if (uni(tr[3]) == 0.f) continue;                   // a rejected attempt changed nothing (wave-uniform)
        float sacc = 0.f;
#pragma unroll 1
        for (int s = 1; s <= 6; ++s) {
            float as[6];
#pragma unroll
            for (int j = 0; j < 6; ++j) as[j] = tab.a[s][j];
#pragma unroll
            for (int m = 0; m < NI; ++m) {
                f32x4 acc = as[0] * kz[0][m], tac = as[0] * tk[0][m];
#pragma unroll
                for (int j = 1; j < 6; ++j) { acc += as[j] * kz[j][m]; tac += as[j] * tk[j][m]; }
                zt[m] = uz[m] + hstep * acc;
                tzt[m] = tu[m] + hstep * tac;
            }
            if (s == 6) {                                  // a_7j = b_j: (zt, tzt) is the new solution and its tangent (FSAL)
                sacc = as[0] * tks[0];
#pragma unroll
                for (int j = 1; j < 6; ++j) sacc += as[j] * tks[j];
            }
            f32x4 zd[NI], dzd[NI];
            float dsd;
            rhs(zt, tzt, zd, dzd, dsd);
#pragma unroll
            for (int i = 1; i < 7; ++i) {
#pragma unroll
                for (int m = 0; m < NI; ++m) { kz[i][m] = s == i ? zd[m] : kz[i][m]; tk[i][m] = s == i ? dzd[m] : tk[i][m]; }
                tks[i] = s == i ? dsd : tks[i];
            }
        }
        tus += hstep * sacc;
#pragma unroll
        for (int m = 0; m < NI; ++m) { uz[m] = zt[m]; tu[m] = tzt[m]; kz[0][m] = kz[6][m]; tk[0][m] = tk[6][m]; }
        tks[0] = tks[6];
    }

    // ---- the tangent of the post-processing ----
    const float t1s = __shfl(tus, c + 16, 64), t2s = __shfl(tus, c + 32, 64);     // DE, Dn to lane group 0
    if constexpr (ENS) {
        // (the outputs move on to the member's copy here, not in the prologue: no more pointers held across the step loop)
        a.out += (size_t)blockIdx.z * en.out_stride;
        if (a.sampling) a.out_logq += (size_t)blockIdx.z * en.logq_stride;
    }
    if (a.sampling) {
        // Dx = the rows of Dz;  Dlogq = -z0 . Dz0 + D(dlogp)
        if (live) {
            float* o = a.out + ((size_t)dir * (size_t)a.B + (size_t)smp) * n_in;
#pragma unroll
            for (int m = 0; m < NI; ++m)
#pragma unroll
                for (int j = 0; j < 4; ++j) { const int r = 16 * m + 4 * q + j; if (r < n_in) o[r] = tu[m][j]; }
            if (q == 0) a.out_logq[(size_t)dir * (size_t)a.B + (size_t)smp] = tus - z0dz0;
        }
    } else {
        // Dlogpx = -z . Dz - D(dlogp);  DA = z_aug . Dz_aug / |z_aug|   (src/base_icnf.jl:167-189)
        float ss = 0.f, sa = 0.f, na = 0.f;
#pragma unroll
        for (int m = 0; m < NI; ++m)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = 16 * m + 4 * q + j;
                ss = fmaf(uz[m][j], tu[m][j], ss);
                if (r >= nd.nvars) { sa = fmaf(uz[m][j], tu[m][j], sa); na = fmaf(uz[m][j], uz[m][j], na); }
            }
        ss = wv_quad_sum(ss); sa = wv_quad_sum(sa); na = wv_quad_sum(na);
        if (live && q == 0) {
            const size_t Bz = (size_t)a.B;
            float* o = a.out + (size_t)dir * 4 * Bz + (size_t)smp;
            o[0] = -ss - tus;
            o[Bz] = TRAIN ? t1s : 0.f;
            o[2 * Bz] = TRAIN ? t2s : 0.f;
            o[3 * Bz] = (TRAIN && nd.norm_z_aug && nd.naugs > 0 && na > 0.f) ? sa / sqrtf(na) : 0.f;    // (TestMode: the loss has no A term)
        }
    }
}

typedef const void* tangent_fn;
template <int NH, bool ID2, bool ENS>
tangent_fn tangent_mode(int mode) {
    if (mode == TG_VJP) return (tangent_fn)k_tangent_wave<1, NH, TG_VJP, ID2, ENS>;
    if (mode == TG_JVP) return (tangent_fn)k_tangent_wave<1, NH, TG_JVP, ID2, ENS>;
    return (tangent_fn)k_tangent_wave<1, NH, TG_TEST, ID2, ENS>;
}
template <bool ENS>
tangent_fn tangent_kernel(const NetDesc& nd, bool train) {
    const int nh = (nd.dims[1] + 15) / 16, mode = !train ? TG_TEST : (nd.jvp ? TG_JVP : TG_VJP);
    if (nd.acts[1] == 0) return nh == 1 ? tangent_mode<1, true, ENS>(mode) : nullptr;
    switch (nh) {
        case 1: return tangent_mode<1, false, ENS>(mode);
        case 2: return tangent_mode<2, false, ENS>(mode);
        case 3: return tangent_mode<3, false, ENS>(mode);
        case 4: return tangent_mode<4, false, ENS>(mode);
    }
    return nullptr;
}

}  // namespace

bool tangent_supported(const NetDesc& nd) {
    if (nd.n_layers != 2 || nd.n_cond > 0 || nd.n_in < 1 || nd.n_in > 16 || nd.dims[1] < 1) return false;
    if (nd.acts[0] != 1 || !(nd.acts[1] == 1 || nd.acts[1] == 0)) return false;
    return nd.dims[1] <= (nd.acts[1] == 0 ? 16 : 64);
}

static bool tangent_args_ok(const TangentArgs& a, bool train) {
    return !(a.B < 1 || a.R < 1 || a.R > TG_MAX_R || !a.P || !a.x || !a.st || !a.trace || a.trace_cap < 1 || !a.out || (train && !a.eps) ||
             (a.sampling && !a.out_logq) || (a.dP && a.n_params < 1));
}

cnf_status tangent_launch(const TangentArgs& a, bool train, hipStream_t s) {
    if (!tangent_supported(a.nd)) return CNF_ERR_UNSUPPORTED;
    if (!tangent_args_ok(a, train)) return CNF_ERR_BAD_ARG;
    tangent_fn fn = tangent_kernel<false>(a.nd, train);
    if (!fn) return CNF_ERR_UNSUPPORTED;
    TangentArgs ka = a;
    WvTab tab = kWvTab;
    TangentNoEns none;
    void* args[] = {&ka, &tab, &none};
    if (hipLaunchKernel(fn, dim3((a.B + 15) / 16, a.R), dim3(64), args, 0, s) != hipSuccess) {
        (void)hipGetLastError();
        return CNF_ERR_HIP;
    }
    return CNF_OK;
}

cnf_status tangent_launch_many(const TangentArgs& a, const TangentEns& en, bool train, hipStream_t s) {
    if (!tangent_supported(a.nd)) return CNF_ERR_UNSUPPORTED;
    // (the members read their own StepState's attempt count: no route files rows for M members from the host)
    if (!tangent_args_ok(a, train) || en.M < 1 || en.M > TG_MAX_M || a.n_rows >= 0) return CNF_ERR_BAD_ARG;
    tangent_fn fn = tangent_kernel<true>(a.nd, train);
    if (!fn) return CNF_ERR_UNSUPPORTED;
    TangentArgs ka = a;
    WvTab tab = kWvTab;
    TangentEns ke = en;
    const size_t Bz = (size_t)a.B, Rz = (size_t)a.R, nz = (size_t)a.nd.n_in, xr = a.sampling ? nz : (size_t)a.nd.nvars;
    ke.dp_stride = Rz * (size_t)a.n_params; ke.eps_stride = Bz * nz; ke.dx_stride = Rz * Bz * xr;
    ke.out_stride = Rz * (a.sampling ? Bz * nz : 4 * Bz); ke.logq_stride = Rz * Bz;
    void* args[] = {&ka, &tab, &ke};
    if (hipLaunchKernel(fn, dim3((a.B + 15) / 16, a.R, en.M), dim3(64), args, 0, s) != hipSuccess) {
        (void)hipGetLastError();
        return CNF_ERR_HIP;
    }
    return CNF_OK;
}
