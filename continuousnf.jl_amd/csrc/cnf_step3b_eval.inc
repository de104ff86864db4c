// The six barrier intervals of ONE evaluation of the VJP compute mode on split-bf16 operands, looped over the stages of an
// attempt: the body shared by k_step3b (one step attempt per launch) and k_solve3b (the whole solve in one launch).
// Included INSIDE those kernels, after their definitions of the names used here (addresses, resident fragments, lambdas;
// S3B_RECORDS: a compile-time constant, with it `float* dmpw` and `size_t dmp_stride`).
        for (int stg = 1; stg <= nstg; ++stg) {
            f32x4 d2a, d2b;                                                  // sigma'_2 at this lane's h2 entries (interval 1 -> 3)
            S3bOp nA0;                                                       // narrow products: k-block 0 of the constant operand (s3b_narrow)
            // ---- interval 0: first layer, tile `wave`, both halves (K = 32: one k-block)
            {
                // conditional models (S3B_COND): the first layer's bias is a row per SAMPLE, W1[:, n_in:] ys + b1 (cnf_set_cond;
                // src/layers/cond_layer.jl:7-9) -- requested here, from L1 / L2, and consumed behind the products
                f32x4 bv1 = *(const f32x4*)(bias + 16 * wave + 4 * q), bv1b = bv1;
                if (S3B_COND) {
                    const int tb = b0 - 16 * hf;
                    bv1 = *(const f32x4*)(a.cond + (size_t)min(tb + s, a.B - 1) * a.cbs + 16 * wave + 4 * q);
                    bv1b = *(const f32x4*)(a.cond + (size_t)min(tb + 16 + s, a.B - 1) * a.cbs + 16 * wave + 4 * q);
                }
                S3bOp b[2];
                b[0] = s3b_load(ldsb + s3v::X0S + nb_rd, s3v::NP);
                b[1] = s3b_load(ldsb + s3v::X0S + nb_rd + HBN, s3v::NP);
                S3_SB();
                f32x4 acc[2] = {zero4, zero4};
                s3b_mm<2>(acc, wF1, b);
                s3b_store4(ldsb + s3v::H1G + wb_wr, s3v::WP, s3_tanh4(acc[0] + bv1));
                s3b_store4(ldsb + s3v::H1G + wb_wr + HBW, s3v::WP, s3_tanh4(acc[1] + bv1b));
            }
            S3T(0);
            s3_bar();
            S3T(1);                                                          // h1 visible
            // ---- interval 1: second layer, tile `wave`, both halves share the A fragments
            {
                const f32x4 bv2 = *(const f32x4*)(bias + 128 + 16 * wave + 4 * q);
                // scalar rows of the PREVIOUS evaluation from its RED partials (complete since the last barrier of it)
                if (stg > 1 && sown) sc_set(stg, read_scalars());              // slot j holds k_j
                f32x4 acc[2] = {zero4, zero4};
                // half a's epilogue, h2a = tanh(acc[0] + b2) -> sigma'_2, the split, the stores, in groups behind half b's
                // MFMAs (s3b_wide): per value j  A add the bias | E, R, O the three steps of tanh | D sigma'; then the steps
                // of the split of either pair.  Issue weight of the groups: 2 or 3, 61 over 23 groups; none behind half b's first MFMA,
                // where a read of acc[0] would still wait for half a's last one.
                float x[4] = {0.f, 0.f, 0.f, 0.f};
                float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
                S3bStore4s sa{};
                // (both halves' stores go through this ONE pointer value, h2w and h2w + HBW: the image base lies above the 16-bit
                // offset of ds_write_b64, and with half b's address written out on its own the compiler keeps an address register
                // per piece live across the stage loop -- profiles/wide_epilogue_kernel_resources.md)
                char* const h2w = ldsb + s3v::H2G + wb_wr;
#define S3W_A(j) { x[j] = acc[0][j] + bv2[j]; s3_hold(x[j]); }
#define S3W_E(j) { x[j] = s3_tanh_exp(x[j]); s3_hold(x[j]); }
#define S3W_R(j) { x[j] = s3_tanh_rcp(x[j]); s3_hold(x[j]); }
#define S3W_OD(j, d) { x[j] = s3_tanh_out(x[j]); d = fmaf(-x[j], x[j], 1.f); s3_hold(x[j]); s3_hold(d); }
                s3b_wide(acc, wF2, ldsb + s3v::H1G, ldsb + s3v::H1G + HBW, wb_rd, s3v::WP, [&](auto I) {
                    constexpr int i = decltype(I)::value;
                    if constexpr (i == -1) S3T(14);
                    if constexpr (i == 1) { S3W_A(0); S3W_A(1); }
                    if constexpr (i == 2) S3W_E(0);
                    if constexpr (i == 3) S3W_E(1);
                    if constexpr (i == 4) S3W_R(0);
                    if constexpr (i == 5) S3W_R(1);
                    if constexpr (i == 6) S3W_OD(0, d0);
                    if constexpr (i == 7) { S3W_OD(1, d1); s3b_store4s_step<0>(sa, x); }
                    if constexpr (i == 8) { S3W_A(2); S3W_A(3); }
                    if constexpr (i == 9) S3W_E(2);
                    if constexpr (i == 10) s3b_store4s_step<1>(sa, x);
                    if constexpr (i == 11) S3W_E(3);
                    if constexpr (i == 12) s3b_store4s_step<2>(sa, x);
                    if constexpr (i == 13) S3W_R(2);
                    if constexpr (i == 14) s3b_store4s_step<3>(sa, x);
                    if constexpr (i == 15) S3W_R(3);
                    if constexpr (i == 16) { s3b_store4s_step<4>(sa, x); s3b_store4s_step<5>(sa, x); }
                    if constexpr (i == 17) { S3W_OD(2, d2); x[3] = s3_tanh_out(x[3]); s3_hold(x[3]); }
                    if constexpr (i == 18) { d3 = fmaf(-x[3], x[3], 1.f); s3_hold(d3); s3b_store4s_step<6>(sa, x); }
                    if constexpr (i == 19) { s3b_store4s_step<7>(sa, x); s3b_store4s_put<0>(sa, h2w, s3v::WP); }
                    if constexpr (i == 20) s3b_store4s_step<8>(sa, x);
                    if constexpr (i == 21) s3b_store4s_step<9>(sa, x);
                    if constexpr (i == 22) { s3b_store4s_step<10>(sa, x); s3b_store4s_put<1>(sa, h2w, s3v::WP); }
                    if constexpr (i == 23) { s3b_store4s_step<11>(sa, x); s3b_store4s_put<2>(sa, h2w, s3v::WP); }
                    if constexpr (i == 24) S3T(15);
                });
#undef S3W_A
#undef S3W_E
#undef S3W_R
#undef S3W_OD
                d2a = f32x4{d0, d1, d2, d3};
                const f32x4 h2b = s3_tanh4(acc[1] + bv2);
                d2b = s3_dtanh4(h2b);
                s3b_store4(h2w + HBW, s3v::WP, h2b);
                // (W3 rows, k-block 0, for interval 2: nothing the barrier publishes; it lands while the stores drain)
                S3_SB();
                if (zown) nA0 = s3b_load(nrA + wb_rd, s3v::WP);
            }
            S3T(2);
            s3_bar();
            S3T(3);                                                          // h2 visible
            // ---- interval 2: last layer on waves 0-3 (one per SIMD): zdot rows r0..r0+3 of sample smp
            if (zown) {
                f32x4 z0 = zero4, z1 = zero4;                                  // two chains (terms 0-2 / 3-5)
                // what the epilogue reads that does not depend on the product is requested behind the last operands: the bias
                // and the Runge-Kutta rows u, k1..k4 (k5, the last of the stage sum, follows the loop: a seventh row in
                // flight there spills weight fragments in k_step3b and the several-tiles forms)
                f32x4 bv3, rku, rkk[5];
                s3b_narrow(z0, z1, nA0, nrA, nrB, wb_rd, s3v::WP, [&]() {
                    bv3 = *(const f32x4*)(bias + 256 + r0);
                    rku = *(const f32x4*)rkw; rkk[0] = *(const f32x4*)(rkw + 32);
#pragma unroll
                    for (int j = 1; j < 4; ++j) rkk[j] = *(const f32x4*)(kzw + 32 * (j - 1));
                });
                rkk[4] = *(const f32x4*)(kzw + 32 * 3);
                S3T(12);                                                     // (stamped builds: barrier exit -> last MFMA issued)
                // stage sum without the k this evaluation will produce: pre = u + h sum_{j<stg} a_{stg+1,j} k_j
                const float* A = tab.a[stg < 6 ? stg + 1 : 6];
                f32x4 pre = rku + (hstep * A[0]) * rkk[0];
#pragma unroll
                for (int j = 1; j < 5; ++j) pre += (hstep * A[j]) * rkk[j];
                const f32x4 zd = s3_tanh4(z0 + z1 + bv3);                      // padded rows: zero weights and bias -> 0
                s3b_store4(g3w, s3v::NP, epsr * s3_dtanh4(zd));               // g3 = eps .* sigma'_3
                const f32x4 xnext = pre + (hstep * A[stg]) * zd;
                if (stg < 6) s3b_store4(x0w, s3v::NP, xnext);                   // state of the next evaluation
                // (gradient path: U_{stg+2} filed behind u_n and U_2 of this step; the pointer is null when nothing is recorded)
                if (S3B_RECORDS && dmpw && stg < 5 && nv > 0) { if (nv >= 4) st4_wide(dmpw + (size_t)stg * dmp_stride, xnext); else st4(dmpw + (size_t)stg * dmp_stride, xnext, nv); }
                *(f32x4*)(kzw + 32 * (stg - 1)) = zd;                          // k_{stg+1}
                redw[0] = s3_dot4(zd, zd);
            }
            S3T(4);
            s3_bar();
            S3T(5);                                                          // g3 (and the next stage state) visible
            // ---- interval 3: reverse of the last layer, tile `wave` of W3^T, both halves (K = 32); g2 over h2 in place
            {
                S3bOp b[2];
                b[0] = s3b_load(ldsb + s3v::G3S + nb_rd, s3v::NP);
                b[1] = s3b_load(ldsb + s3v::G3S + nb_rd + HBN, s3v::NP);
                S3_SB();
                f32x4 acc[2] = {zero4, zero4};
                s3b_mm<2>(acc, wB3, b);
                s3b_store4(ldsb + s3v::H2G + wb_wr, s3v::WP, acc[0] * d2a);
                s3b_store4(ldsb + s3v::H2G + wb_wr + HBW, s3v::WP, acc[1] * d2b);
            }
            S3T(6);
            s3_bar();
            S3T(7);                                                          // g2 visible
            // ---- interval 4: reverse of the second layer, tile `wave` of W2^T; g1 over h1 in place
            {
                f32x4 acc[2] = {zero4, zero4};
                // half a's epilogue, g1a = acc[0] .* sigma'_1(h1a) -> the split, the stores, in groups behind half b's MFMAs
                // (s3b_wide): per value j  L, V h1a back from its three pieces | D sigma'_1 | G the product; then the steps of
                // the split of either pair, P for the first remainder of a product (s3b_store4s_rest_of_product).  h1a is requested in front of half a's last k-block, h1b -- needed only behind
                // the call -- once half a's stores are out.  Issue weight of the groups: 2 or 3, 56 over 20 groups.
                float x[4] = {0.f, 0.f, 0.f, 0.f}, dd[4] = {0.f, 0.f, 0.f, 0.f};
                S3bStore4s sa{};
                S3bPieces4 pa, pb;
                char* const g1w = ldsb + s3v::H1G + wb_wr;
#define S3W_L(j) { x[j] = s3b_load4_low(pa, j); s3_hold(x[j]); }
#define S3W_VD(j) { dd[j] = s3b_load4_value(pa, j, x[j]); dd[j] = fmaf(-dd[j], dd[j], 1.f); s3_hold(dd[j]); }
#define S3W_G(j) { x[j] = acc[0][j] * dd[j]; s3_hold(x[j]); }
#define S3W_P(j) s3b_store4s_rest_of_product<j>(sa, x, acc[0][j], dd[j])
                s3b_wide(acc, wB2, ldsb + s3v::H2G, ldsb + s3v::H2G + HBW, wb_rd, s3v::WP, [&](auto I) {
                    constexpr int i = decltype(I)::value;
                    if constexpr (i == -2) pa = s3b_load4_request(g1w, s3v::WP);
                    if constexpr (i == -1) S3T(16);
                    if constexpr (i == 0) S3W_L(0);
                    if constexpr (i == 1) S3W_VD(0);
                    if constexpr (i == 2) S3W_L(1);
                    if constexpr (i == 3) S3W_VD(1);
                    if constexpr (i == 4) { S3W_G(0); S3W_G(1); s3b_store4s_step<0>(sa, x); }
                    if constexpr (i == 5) S3W_L(2);
                    if constexpr (i == 6) S3W_P(0);
                    if constexpr (i == 7) S3W_VD(2);
                    if constexpr (i == 8) S3W_P(1);
                    if constexpr (i == 9) S3W_L(3);
                    if constexpr (i == 10) s3b_store4s_step<3>(sa, x);
                    if constexpr (i == 11) S3W_VD(3);
                    if constexpr (i == 12) { s3b_store4s_step<4>(sa, x); s3b_store4s_step<5>(sa, x); }
                    if constexpr (i == 13) { S3W_G(2); S3W_G(3); s3b_store4s_step<6>(sa, x); }
                    if constexpr (i == 14) { S3W_P(2); s3b_store4s_put<0>(sa, g1w, s3v::WP); }
                    if constexpr (i == 15) S3W_P(3);
                    if constexpr (i == 16) s3b_store4s_step<9>(sa, x);
                    if constexpr (i == 17) { s3b_store4s_step<10>(sa, x); s3b_store4s_put<1>(sa, g1w, s3v::WP); }
                    if constexpr (i == 18) { s3b_store4s_step<11>(sa, x); s3b_store4s_put<2>(sa, g1w, s3v::WP); }
                    if constexpr (i == 19) pb = s3b_load4_request(g1w + HBW, s3v::WP);
                    if constexpr (i == 24) S3T(17);
                });
#undef S3W_L
#undef S3W_VD
#undef S3W_G
#undef S3W_P
                s3b_store4(g1w + HBW, s3v::WP, acc[1] * s3_dtanh4(s3b_load4_values(pb)));
                // (W1^T rows, k-block 0, for interval 5: as W3's in front of interval 2)
                S3_SB();
                if (!zown) nA0 = s3b_load(nrA + wb_rd, s3v::WP);
            }
            S3T(8);
            s3_bar();
            S3T(9);                                                          // g1 visible
            // ---- interval 5: eJ = W1^T g1 on waves 4-7 (one per SIMD): trace and norm partials (src/icnf.jl:334, :343)
            if (!zown) {
                f32x4 j0 = zero4, j1 = zero4;
                s3b_narrow(j0, j1, nA0, nrA, nrB, wb_rd, s3v::WP, []() {});
                S3T(13);                                                     // (stamped builds: barrier exit -> last MFMA issued)
                const f32x4 ej = j0 + j1;
                redw[32 * 8] = -s3_dot4(ej, epsr);
                redw[2 * 32 * 8] = s3_dot4(ej, ej);
            }
            S3T(10);
            s3_bar();
            S3T(11);                                                          // RED complete; h1 / g1 free for the next evaluation
        }
