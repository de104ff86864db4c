/* The gradient w.r.t. the base distribution of the C ABI of libcnfhip.so.  Part of cnfhip.h, which includes it where its types
 * are declared (inside its extern "C" block): include cnfhip.h, not this file.  Like cnfhip_generate.h the two entry points
 * have a header and a binding table (`_lib.BASEGRAD_EXPORTS`) of their own, because the tests of the earlier entry points pin
 * the lists that cnfhip.h itself and cnfhip_generate.h declare; tests/test_base_grad_ref_host.py holds this header to the same
 * rule: every name declared here is exported by the library and bound. */
#ifndef CNFHIP_BASEGRAD_H
#define CNFHIP_BASEGRAD_H

/* ---- a learnable base distribution: gradients w.r.t. the `mean` and `chol` that cnf_set_basedist takes ----
 * The base is N(mean, L L'), W = inv(L), n_b = W (z_b - mean), and
 *     logpdf(z_b) = -sum_i log L_ii - n_in / 2 log(2 pi) - 1/2 |n_b|^2
 *     d/d mean sum_b w_b logpdf(z_b) = W' sum_b w_b n_b
 *     d/d L    sum_b w_b logpdf(z_b) = tril(W' sum_b w_b n_b n_b') - (sum_b w_b) diag(1 / L_ii)
 *                                      (diagonal kind: (sum_b w_b n_b[i]^2 - sum_b w_b) / sigma_i)
 * g_chol is laid out as cnf_set_basedist takes chol: n_in floats in the diagonal kind; ROW-major n_in x n_in in the dense kind,
 * the entries above the diagonal written as 0.  All pointers are DEVICE memory and the calls are stream-ordered: they return
 * once their launches are enqueued on `stream` (the first call of a larger problem grows a buffer of the handle behind a wait
 * for the device; a steady-state call allocates nothing).  The two calls share that buffer: calls on one handle that may overlap
 * in time must be enqueued on ONE stream, as everything else on a handle.  Sums run in a fixed order: the same bits from run to run.
 * CNF_ERR_BAD_ARG: a NULL pointer, B < 1, or a handle whose base is the default (kind 0: it has no mean and no chol).
 *
 * cnf_base_logpdf_pullback: g_mean[n_in], g_chol = sum_b w[b] d logpdf(base; s_b) / d (mean, chol), where s_b is
 *   - on an inference record (cnf_inference_record): the recorded final state z_b(t1).  logpx_b = logpdf(base, z_b(t1)) -
 *     dlogp_b and z_b(t1) does not depend on the base, so w = the cotangent of logpx gives the whole gradient;
 *   - on a sampling record (cnf_generate_record): the handle's copy of z0.  logq_b = logpdf(base, z0_b) + dlogp_b, so w = the
 *     cotangent of logq gives the partial derivative at FIXED z0 (a z0 that was itself drawn from the base adds
 *     cnf_base_sample_pullback of the grad_z0 that cnf_generate_pullback returns);
 *   - after cnf_loss_grad / cnf_loss_grad_test on a handle with a non-default base: the final state of that call's solve
 *     (the loss has w = -1/B), until the next call that would end a record.
 * May be called several times on one record, before or after the parameter pullback; it changes nothing of the record.
 * Also CNF_ERR_BAD_ARG when there is no such state or B differs from its batch.
 *
 * cnf_base_sample_pullback: the vector-Jacobian product of cnf_base_sample (z0[:, b] = mean + L normals[:, b]); stateless,
 * no record is needed.  normals and g_z0 are n_in x B:  g_mean = sum_b g_z0[:, b],  g_chol = tril(sum_b g_z0[:, b]
 * normals[:, b]')  (diagonal kind: its diagonal). */
cnf_status cnf_base_logpdf_pullback(cnf_handle h, const float* w, int B, float* g_mean, float* g_chol, void* stream);
cnf_status cnf_base_sample_pullback(cnf_handle h, const float* normals, const float* g_z0, int B, float* g_mean,
                                    float* g_chol, void* stream);

#endif /* CNFHIP_BASEGRAD_H */
