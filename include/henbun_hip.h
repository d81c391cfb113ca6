/*
 * henbun_hip.h -- C ABI of libhenbun_hip.so, the MI355X (gfx950) numeric
 * backend of henbun_amd.
 *
 * What this replaces.  The reference (fujii-team/Henbun) has NO native
 * boundary of its own: every numeric op on the ELBO path is a TensorFlow 1.x
 * graph node reached through `session.run` (reference Henbun/model.py:81,96,
 * 225-227,250,265) and the thin shim module Henbun/tf_wraps.py:26-48.  The
 * only native-op precedent is the disabled `tf.load_op_library('tfops/
 * matpackops.so')` hook (Henbun/tf_wraps.py:50-71).  This header is the
 * boundary the north star asks for in its place: a flat `extern "C"` surface,
 * plain device pointers and sizes, loaded from Python with ctypes
 * (henbun_amd/_lib.py).  Each entry cites the reference call site(s) whose TF
 * op(s) it stands in for.
 *
 * Conventions
 *   - every pointer is a caller-owned DEVICE pointer unless marked (host);
 *     the library allocates nothing persistent; scratch comes in through
 *     `ws`/`ws_elems` (elements of the op's dtype);
 *   - `stream` is a hipStream_t passed as void*; every call is asynchronous
 *     on it and never synchronises;
 *   - return 0 = ok, <0 = bad argument (message in hb_last_error_string()),
 *     >0 = hipError_t from the runtime;
 *   - numerical failure (non-positive-definite Cholesky) is reported through
 *     a device-side `int* info` (LAPACK convention: k+1 = leading minor k+1
 *     is not positive definite), since calls are asynchronous;
 *   - `_f32` / `_f64` suffix = arithmetic type; layouts are row-major,
 *     contiguous unless strides are given; extents are `long` (int64).
 *   - samplers accept injected noise (`u_in`, nullable) and export the noise
 *     they used (`u_out`), so parity tests never depend on the RNG stream.
 */
#ifndef HENBUN_HIP_H
#define HENBUN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history: 1 = rounds 1-3 (the round that removed hb_cholesky_inverse_sgp_f32 and hb_sgp_finish_* should have
 * bumped it and did not); 2 = round 4: hb_debug_set / hb_debug_clear, hb_cholesky_inverse_ws_elems and the workspace
 * contract of hb_cholesky_inverse_f32 (exchange + sync area, zero-filled once by its owner); added without changing an
 * existing signature: hb_cholesky_persistent_shape, hb_gram_cholesky_inverse_f32, hb_mlp2_sample_*, hb_matmul_gauss_*,
 * hb_matmul_gram_vjp_*, hb_gram_ell_fold_*, hb_sgp_rider_*, hb_fullrank_sample_kl_fwd1_* / hb_fullrank_one_launch_shape.
 * Still 2 after additions that change no existing signature: hb_sgp_predict_f32 / _f64, hb_sgp_predict_ws_elems and the
 * enum values HB_SGP_FULLRANK, HB_SGP_S_DIAG, HB_SGP_S_TRIL (closed-form predictive moments); hb_sgp_predict_cov_f32 /
 * _f64 and hb_sgp_predict_cov_ws_elems (full predictive covariance); hb_sgp_stats_f32 / _f64 and hb_sgp_stats_ws_elems
 * (sufficient statistics of the closed-form optimal q(u)); hb_sgp_select_f32 / _f64 and hb_sgp_select_ws_elems (greedy
 * conditional-variance selection of inducing points); hb_sgp_kgrad_f32 / _f64 and hb_sgp_kgrad_ws_elems (streamed part
 * of the gradient of the collapsed bound); hb_sgp_wstats_f32 / _f64, hb_sgp_wstats_ws_elems, hb_lik_sites_f32 / _f64,
 * hb_lik_sites_ws_elems, hb_lik_predict_f32 / _f64 and the enum values HB_LIK_* (natural-gradient fit of q(u) for
 * non-Gaussian likelihoods); hb_lik_param_grad_f32 / _f64, hb_lik_param_grad_ws_elems, hb_lik_logdens_f32 / _f64 and
 * HB_LIK_LAPLACE .. HB_LIK_BINOMIAL (likelihoods with a parameter of their own, its gradient, predictive log density); hb_sgp_wkgrad_f32 / _f64 (streamed part of the gradient of the ELBO at a fixed q(u));
 * hb_sgp_pathwise_f32 / _f64 (pathwise posterior function draws, linear in n); hb_gram_matvec_f32 / _f64 and hb_pcg_*
 * (matrix-free kernel product and the vector steps of lockstep preconditioned conjugate gradients: exact GP regression);
 * hb_gram_bilinear_grad_f32 / _f64 and hb_pcg_*_coef (the exact GP's log marginal likelihood and its gradient);
 * hb_sgp_bwd_phi_f32 and hb_sgp_bwd_phi_supported (the sparse-GP backward that writes the Cholesky VJP's operand
 * Phisym(-Abar A^T) where hb_sgp_bwd_f32 writes Lbar); hb_sgp_pathwise_grad_f32 / _f64, hb_sgp_pathwise_argmax_f32 / _f64
 * and hb_sgp_pathwise_argmax_ws_elems (input gradients and the per-draw extremum of pathwise function draws);
 * hb_sgp_predict_grad_f32 / _f64, hb_sgp_predict_grad_ws_elems, hb_sgp_acq_f32 / _f64, hb_sgp_acq_ws_elems and the enum
 * values HB_ACQ_* (input gradients of the closed-form predictive and closed-form acquisition functions);
 * hb_sgp_predict_fused, hb_sgp_frag_elems, hb_cholesky_frag_elems, hb_matmul_wgk_shape and the enum values HB_MATUTIL_*
 * (rules and sizes a planner asks for instead of restating them); hb_sgp_pathwise_acq_f32 / _f64,
 * hb_sgp_pathwise_acq_ws_elems and the enum values HB_PWACQ_* (batch acquisition from pathwise function draws);
 * hb_matmul_form and the enum values HB_MM_FORM_* (which kernel form, slab count and operand path hb_matmul_* takes for
 * a call: a host-side query that launches nothing); hb_gram_predict_f32 / _f64 and hb_gram_predict_ws_elems (exact GP:
 * predictive mean, cached upper bound of the predictive variance and closed-form acquisition from one kernel product);
 * hb_matmul_gram_vjp_tiles_ok / _tiles_f32 and hb_gram_tiles_fold_f32 (the Gram VJP's tile partials from the product that
 * computes Kbar, folded at the head of a serial chain); hb_gram_predict_grad_f32 / _f64 and hb_gram_predict_grad_ws_elems
 * (exact GP: input gradients of the cached predictive and of its closed-form acquisition); hb_lik_softmax_sites_f32 /
 * _f64, hb_lik_softmax_predict_f32 / _f64, hb_lik_softmax_ws_elems, HB_LIK_SOFTMAX, hb_sgp_mwstats_f32 / _f64 and
 * hb_sgp_mwstats_ws_elems (multi-class classification: softmax sites, weighted statistics of C weight sets from one A);
 * hb_lik_softmax_grad_f32 / _f64 (hyper-parameter gradient of the multi-class ELBO at fixed q(u_c): the exact weights of
 * the fixed-node value); hb_sgp_predict_multi_f32 / _f64, hb_sgp_predict_multi_ws_elems, hb_sgp_predict_multi_fused,
 * hb_lik_hetgauss_sites_f32 / _f64, hb_lik_hetgauss_predict_f32 / _f64, hb_lik_hetgauss_logdens_f32 / _f64,
 * hb_lik_hetgauss_ws_elems and HB_LIK_HETGAUSS (heteroscedastic regression: the marginals of C full-rank latent functions
 * from one pass, the two-latent Gaussian likelihood); hb_sgp_psi_stats_f32 / _f64, hb_sgp_psi_stats_ws_elems,
 * hb_sgp_psi_predict_f32 / _f64 and hb_sgp_psi_predict_ws_elems (psi statistics: the closed-form routes under uncertain
 * inputs); hb_sgp_psi_grad_f32 / _f64 and hb_sgp_psi_grad_ws_elems (their gradients: the Bayesian GP-LVM);
 * hb_sgp_kgrad_x_f32 / _f64 and hb_sgp_wkgrad_x_f32 / _f64 (hb_sgp_kgrad_* / hb_sgp_wkgrad_* with the input gradient
 * xbar [N, d] as a third output: deep kernel learning). */
#define HB_ABI_VERSION 2

/* ---- runtime ----------------------------------------------------------- */
int hb_version(void);
const char* hb_last_error_string(void);
/* Diagnostic switches (A/B forms of a dispatch rule, forced tile sizes; tests and tools/ use them): a process-wide
 * key -> value table.  The library never reads the environment; without a call here every dispatch rule is the
 * shipped one.  Keys: chol_persist (0: the launch-chain Cholesky), chol_no64, mm_no_wgk, mm_no_rowsreg, mm_no_rows,
 * mm_force_bt, mm_force_s, sgp_no_strip, sgp_force_strip, sgp_tiled_crossover, sgp_strip_form2, sgp_no_fused_finish,
 * lbar_force_s, lbar_no_lds, sgp_stats_no_A, sgp_stats_no_syrk (hb_sgp_stats_* without its first / second pass: timing
 * only, the outputs are then meaningless), sgp_stats_target_wg (tiles x K-splits aimed at; hb_sgp_stats_ws_elems follows), sgp_select_block (64 / 256: the workgroup
 * size of hb_sgp_select_*; the results do not depend on it), sgp_kgrad_plain (hb_sgp_kgrad_* in its plain-loop form for
 * every shape), sgp_phi_direct (0: hb_sgp_bwd_phi_supported answers 0, so a plan built then keeps hb_sgp_bwd and the
 * Cholesky VJP's first product), sgp_fwd_kbar (0: hb_sgp_fwd_kbar_supported answers 0, so a plan built then keeps the
 * forward and the Kbar strips as two launches), gram_vjp_tiles (0: hb_matmul_gram_vjp_tiles_ok answers 0, so a plan built then runs the
 * Gram VJP of K(z, z) as launches of its own).  hb_debug_clear() drops every entry. */
int hb_debug_set(const char* key, long value);
int hb_debug_clear(void);
/* device name / arch of the current device into (host) buf; returns 0 or hipError */
int hb_device_info(char* buf, int buflen, int* cu_count);

/* hipGraph capture of a launch sequence (replaces the per-op dispatch of
 * session.run, reference model.py:265-266).  exec is a (host) handle. */
int hb_graph_begin_capture(void* stream);
int hb_graph_end_capture(void* stream, void** exec_out);
int hb_graph_launch(void* exec, void* stream);
int hb_graph_destroy(void* exec);

/* ---- generic tensor plumbing (tf elementwise ops, reduce_sum, transpose,
 *      slice, tile; reference call sites listed in SURVEY.md 2.2) ---------- */
enum {
  /* unary */
  HB_EW_NEG = 1, HB_EW_EXP, HB_EW_LOG, HB_EW_SQRT, HB_EW_SQUARE, HB_EW_ABS, HB_EW_SIGN,
  HB_EW_SIGMOID, HB_EW_RELU, HB_EW_SOFTPLUS, HB_EW_TANH, HB_EW_RECIP, HB_EW_RSQRT,
  HB_EW_STEP, HB_EW_AFFINE /* p0*x+p1 */, HB_EW_CLIP /* [p0,p1] */, HB_EW_CLIPMASK,
  HB_EW_LGAMMA, HB_EW_POWC /* x^p0 */, HB_EW_LOG1P, HB_EW_COPY, HB_EW_DIGAMMA,
  /* binary */
  HB_EW_ADD = 32, HB_EW_SUB, HB_EW_MUL, HB_EW_DIV, HB_EW_MAX, HB_EW_MIN, HB_EW_POW,
  HB_EW_GT, HB_EW_GE, HB_EW_LT, HB_EW_LE, HB_EW_EQ,
  HB_EW_SIGMOID_GRAD /* (y,g) */, HB_EW_TANH_GRAD /* (y,g) */, HB_EW_RELU_GRAD /* (x,g) */,
  HB_EW_SOFTPLUS_GRAD /* (x,g) */, HB_EW_CLIP_GRAD /* (x,g) p0,p1 */,
  /* ternary */
  HB_EW_WHERE = 64 /* (c,a,b) */, HB_EW_FMA /* a*b+c */,
  HB_EW_GAUSS_LOGPDF /* (x,mu,var): reference densities.py:25-27 */,
  /* 4 in, 3 out */
  HB_EW_GAUSS_LOGPDF_GRAD = 80 /* (x,mu,var,g) -> (gx,gmu,gvar) */
};

/* out[k][i] = op(in[0][bcast(i)], ...); every output is contiguous with the
 * broadcast `shape[ndim]`; `istrides` is [nin][ndim] in elements (0 = broadcast).
 * in/out/istrides/shape/params are (host) arrays; params has 4 doubles or NULL. */
int hb_ewise_f32(int op, int nin, const void* const* in, const long* istrides, int nout,
                 void* const* out, int ndim, const long* shape, const double* params, void* stream);
int hb_ewise_f64(int op, int nin, const void* const* in, const long* istrides, int nout,
                 void* const* out, int ndim, const long* shape, const double* params, void* stream);

/* Fused Gaussian log-likelihood head (reference densities.py:25-27 under tf.reduce_sum, plus its TF gradients):
 *   ll = sum_j log N(x_j | f_j*scale, var)            -> ll[1]
 *   dmu_j = (x_j - f_j*scale)/var                      -> dmu[n]   (d ll / d mu_j)
 *   dscale = sum_j dmu_j f_j, dvar = sum_j (-1/(2var) + (x_j-mu_j)^2/(2var^2))   -> dscale[1], dvar[1]
 * x, f: n contiguous elements; scale (nullable = 1) and var: one element each, device.
 * ws >= 3*ceil(n/1024) elements.  Two launches; sums in a fixed order. */
int hb_gauss_ll_f32(const float* x, const float* f, const float* scale, const float* var, long n, float* ll,
                    float* dmu, float* dscale, float* dvar, float* ws, long ws_elems, void* stream);
int hb_gauss_ll_f64(const double* x, const double* f, const double* scale, const double* var, long n,
                    double* ll, double* dmu, double* dscale, double* dvar, double* ws, long ws_elems,
                    void* stream);
/* The same head with the gradient handed back to the producer of f written by the same launch:
 * fbar_j = scale * (post * dmu_j) = d(post * ll) / d f_j (post: the constant upstream factor of the likelihood term, N / n
 * in every notebook ELBO).  Replaces the two elementwise ops TF autodiff appends to the head (and their launch). */
int hb_gauss_ll_post_f32(const float* x, const float* f, const float* scale, const float* var, long n, float* ll,
                         float* dmu, float* dscale, float* dvar, double post, float* fbar, float* ws, long ws_elems,
                         void* stream);
int hb_gauss_ll_post_f64(const double* x, const double* f, const double* scale, const double* var, long n, double* ll,
                         double* dmu, double* dscale, double* dvar, double post, double* fbar, double* ws, long ws_elems,
                         void* stream);

/* A whole cluster of elementwise ops in one launch: a register program interpreted per element
 * of the broadcast iteration space `shape[ndim]` (ndim <= 4).  Registers 0..nin-1 hold the inputs
 * (read with `istrides`); instruction q = code[q] = {op, dst, a, b, c} (HB_EW_* op on registers a,b,c;
 * HB_EW_GAUSS_LOGPDF_GRAD takes the register number of its 4th operand in params[q][0] and writes
 * dst..dst+2) with params[q][2]; output k = register out_regs[k] stored with `ostrides` (a 0 stride on a dim of extent > 1
 * marks a broadcast dim: only index 0 writes); out_regs[k] + HB_EW_PROG_SUM instead writes the SUM of that
 * register over the whole space to out[k][0] (tf.reduce_sum of a chain's result; the program then runs as one
 * workgroup, space <= 65536 elements).  All array arguments are (host) arrays.  Replaces the
 * chains of tiny TF elementwise ops of the reference's graph at one launch per chain. */
enum { HB_EW_PROG_SUM = 256 };
int hb_ewise_prog_f32(int ninstr, const int* code, const double* params, int nin, const void* const* in,
                      const long* istrides, int nout, void* const* out, const int* out_regs,
                      const long* ostrides, int ndim, const long* shape, void* stream);
int hb_ewise_prog_f64(int ninstr, const int* code, const double* params, int nin, const void* const* in,
                      const long* istrides, int nout, void* const* out, const int* out_regs,
                      const long* ostrides, int ndim, const long* shape, void* stream);
/* Device-resident form for programs that are replayed (a captured plan): hb_ewise_prog_build validates the
 * same arguments and writes the launch descriptor (hb_ewise_prog_image_bytes() bytes, independent of the element
 * type) to HOST memory; the caller copies it to the device once (4-byte aligned) and every launch is
 * hb_ewise_prog_run_* with that pointer and the `n` / `reduces` build returned.  The kernel pulls the descriptor
 * into LDS with one parallel load; the by-value form above walks it with dependent scalar loads (~4 us slower). */
long hb_ewise_prog_image_bytes(void);
int hb_ewise_prog_build(int ninstr, const int* code, const double* params, int nin, const void* const* in,
                        const long* istrides, int nout, void* const* out, const int* out_regs,
                        const long* ostrides, int ndim, const long* shape, void* image_host, long* n_out,
                        int* reduces_out);
int hb_ewise_prog_run_f32(const void* image_dev, long n, int reduces, void* stream);
int hb_ewise_prog_run_f64(const void* image_dev, long n, int reduces, void* stream);
/* Compiled form (the one a plan uses when it can): the same program description is turned into HIP source --
 * shape, strides, op codes and constants as literals, every op the library's own definition with the op code known
 * at compile time -- and compiled for gfx950 at plan-build time by hiprtc (looked up with dlopen; where it is
 * absent hb_ewise_jit_available() returns 0 and callers keep the interpreted form above).  build returns an opaque
 * handle holding the loaded kernel and its pointer arguments (NULL for an empty iteration space); run launches it
 * on `stream` (capturable); identical programs share one compiled module.  source_out (nullable): receives the
 * generated kernel text, truncated to source_cap bytes, for inspection.  handle_out == NULL: dry run -- generate and
 * compile only (needs no device).  The interpreter took 8.8 us per launch at
 * cfg 2 for 7-11 scalar ops; replaces the same tf.* elementwise chains. */
int hb_ewise_jit_available(void);
int hb_ewise_jit_build_f32(int ninstr, const int* code, const double* params, int nin, const void* const* in,
                           const long* istrides, int nout, void* const* out, const int* out_regs,
                           const long* ostrides, int ndim, const long* shape, void** handle_out, long* n_out,
                           int* reduces_out, char* source_out, long source_cap);
int hb_ewise_jit_build_f64(int ninstr, const int* code, const double* params, int nin, const void* const* in,
                           const long* istrides, int nout, void* const* out, const int* out_regs,
                           const long* ostrides, int ndim, const long* shape, void** handle_out, long* n_out,
                           int* reduces_out, char* source_out, long source_cap);
int hb_ewise_jit_run(void* handle, void* stream);
int hb_ewise_jit_destroy(void* handle);
/* Column programs (round 3): a fused program over a SHORT-AND-WIDE space [R, n] (R <= 16 rows, e.g. the E experts of a
 * softmax gate over a minibatch of n points) in which reductions over the ROW axis are ordinary instructions.  One
 * thread owns one column: a register is R values (operands [R, n]) or one value (operands [1, n], scalars, and the
 * result of a row reduction), every row loop is unrolled in the thread, so the softmax gate of the expert mixture
 * (reference notebooks/Expert_GPR.ipynb:139-147: reduce_max, exp, reduce_sum, divide, weighted sum -- eight launches
 * op by op, three of them tf.reduce_* over axis 0) and its whole VJP are ONE launch each and every operand is read once.
 *   code[q] = {op, dst, a, b, c}: op is an HB_EW_* code (not HB_EW_GAUSS_LOGPDF_GRAD) or HB_COLPROG_SUM / HB_COLPROG_MAX
 *             (dst[0] = sum / max over the rows of register a, rows in order 0..R-1); registers 0..nin-1 are the inputs.
 *   istrides[k] = {row stride, column stride} of input k in elements: {ld, 1} an [R, n] operand (ld >= n: a row block of a
 *             taller matrix is passed by pointer offset, no copy), {0, 1} a row [1, n], {0, 0} a scalar.
 *   out_regs / ostrides likewise; an output with column stride 0 is written by the thread of column 0.
 * A register is R-high exactly when one of its operands is; handle_out / source_out / dry run as for
 * hb_ewise_jit_build; the handle is launched with hb_ewise_jit_run and released with hb_ewise_jit_destroy. */
enum { HB_COLPROG_SUM = -1, HB_COLPROG_MAX = -2 };
int hb_ewise_colprog_build_f32(int ninstr, const int* code, const double* params, int nin, const void* const* in,
                               const long* istrides, int nout, void* const* out, const int* out_regs,
                               const long* ostrides, long R, long n, void** handle_out, char* source_out,
                               long source_cap);
int hb_ewise_colprog_build_f64(int ninstr, const int* code, const double* params, int nin, const void* const* in,
                               const long* istrides, int nout, void* const* out, const int* out_regs,
                               const long* ostrides, long R, long n, void** handle_out, char* source_out,
                               long source_cap);

enum { HB_RED_SUM = 0, HB_RED_MAX = 1 };
/* out[K1,K2] = reduce over R of contiguous in[K1,R,K2]  (tf.reduce_sum / reduce_max) */
int hb_reduce_f32(int op, const float* in, float* out, long K1, long R, long K2, float* ws,
                  long ws_elems, void* stream);
int hb_reduce_f64(int op, const double* in, double* out, long K1, long R, long K2, double* ws,
                  long ws_elems, void* stream);

/* strided n-d copy, strides in elements (tf.transpose / slice / tile / concat) */
int hb_copy_nd_f32(const float* in, const long* istr, float* out, const long* ostr, int ndim,
                   const long* shape, void* stream);
int hb_copy_nd_f64(const double* in, const long* istr, double* out, const long* ostr, int ndim,
                   const long* shape, void* stream);

int hb_fill_f32(float* out, long n, double v, void* stream);
int hb_fill_f64(double* out, long n, double v, void* stream);

/* K0: dst[i,:] = src[perm[idx[i]],:]  (perm nullable).  Device-resident form
 * of MinibatchData.get_feed_dict's `self.data[minibatch_index]`, reference
 * param.py:733-739, with Indexer's train/test permutation (model.py:147-153)
 * applied on device.  *err is set to 1 on an out-of-range index. */
int hb_gather_rows_f32(const float* src, long nsrc, long row, const long* idx, const long* perm,
                       long n, float* dst, int* err, void* stream);
int hb_gather_rows_f64(const double* src, long nsrc, long row, const long* idx, const long* perm,
                       long n, double* dst, int* err, void* stream);
/* The same gather for up to 8 arrays that share the index vector (all with nsrc rows; rows[a] = row width of
 * array a), in one launch: a model's MinibatchData arrays (reference param.py:733-739 feeds them one by one). */
int hb_gather_rows_multi_f32(int narr, const float* const* srcs, const long* rows, float* const* dsts,
                             long nsrc, const long* idx, const long* perm, long n, int* err, void* stream);
int hb_gather_rows_multi_f64(int narr, const double* const* srcs, const long* rows, double* const* dsts,
                             long nsrc, const long* idx, const long* perm, long n, int* err, void* stream);

/* The minibatch draw and that gather in ONE launch: idx[i] ~ U{lo..hi-1} is drawn from RNG lane i exactly as
 * hb_rng_randint(state, nlanes, idx_out, n, lo, hi) would (same values, same state afterwards; n <= nlanes), written
 * to idx_out, and row perm[idx[i]] of every array is gathered.  Replaces Indexer.train_index + the feed of every
 * MinibatchData (reference param.py:715-739) per step. */
int hb_gather_rows_multi_draw_f32(int narr, const float* const* srcs, const long* rows, float* const* dsts,
                                  long nsrc, uint64_t* state, long nlanes, long lo, long hi, long* idx_out,
                                  const long* perm, long n, int* err, void* stream);
int hb_gather_rows_multi_draw_f64(int narr, const double* const* srcs, const long* rows, double* const* dsts,
                                  long nsrc, uint64_t* state, long nlanes, long lo, long hi, long* idx_out,
                                  const long* perm, long n, int* err, void* stream);

/* batched [B,R,C] matrix utilities.  mode BAND (0) = tf.matrix_band_part(lower,upper)
 * (reference variationals.py:145); ADD_EYE (1) = + alpha*I (kernels.py:100 jitter);
 * PHI (2) = Phi (lower triangle, halved diagonal) of the Cholesky gradient;
 * SYM (3) = 0.5*(A + A^T);
 * SYMLOW (4) = symmetric matrix built from HALF the lower triangle: out[i][j] = out[j][i] = 0.5*A[max(i,j)][min(i,j)]
 *     (= (Phi(A) + Phi(A)^T)/2, the operand that makes the Cholesky gradient's L^-T Phi(.) L^-1 symmetric by
 *     construction, so no symmetrising pass over the result is needed). */
enum { HB_MATUTIL_BAND = 0, HB_MATUTIL_ADD_EYE = 1, HB_MATUTIL_PHI = 2, HB_MATUTIL_SYM = 3, HB_MATUTIL_SYMLOW = 4 };
int hb_matutil_f32(const float* in, float* out, long B, long R, long C, int mode, long lower,
                   long upper, double alpha, void* stream);
int hb_matutil_f64(const double* in, double* out, long B, long R, long C, int mode, long lower,
                   long upper, double alpha, void* stream);

/* ---- RNG: xoroshiro128+ per lane (replaces tf.random_normal, reference
 *      variationals.py:107,127; gp/gp.py:132,138,142; and np.random.randint
 *      of model.py:147-153) ------------------------------------------------ */
/* state = 2*nlanes uint64 (s0[nlanes] then s1[nlanes]); seeded by splitmix64
 * from (seed, stream_id, lane). */
int hb_rng_init(uint64_t* state, long nlanes, uint64_t seed, uint64_t stream_id, void* stream);
int hb_rng_normal_f32(uint64_t* state, long nlanes, float* out, long n, void* stream);
int hb_rng_normal_f64(uint64_t* state, long nlanes, double* out, long n, void* stream);
/* uniform integers in [lo, hi), with replacement */
int hb_rng_randint(uint64_t* state, long nlanes, long* out, long n, long lo, long hi, void* stream);

/* ---- K1/K2: reparameterised Gaussian sampler fused with the Monte-Carlo KL
 *      (reference variationals.py:131-153 _sample, :178-186 logdet,
 *      :225-230 Normal._KL) ------------------------------------------------ */
/* diagonal q: x = mu + exp(s)*u ; kl = -0.5*sum(2 s + u^2 - x^2) over all n
 * elements.  u_in nullable (then drawn from rng, which must be non-null);
 * u_out, x: [n] dense; kl: 1 element; ws >= 2048 elements.
 * mu and s are n/L rows of L elements with row strides ld_mu, ld_s (>= L): L = n, ld = n is the flat case; an
 * encoder-fed (LOCAL) posterior passes the mean and log-std halves of the encoder's [rows, 2L] output in place
 * (reference variationals.py:70-80 slices them out of the fed tensor). */
int hb_diag_sample_kl_fwd_f32(const float* mu, const float* s, const float* u_in, uint64_t* rng,
                              long rng_lanes, float* u_out, float* x, float* kl, long n, long L,
                              long ld_mu, long ld_s, float* ws, void* stream);
int hb_diag_sample_kl_fwd_f64(const double* mu, const double* s, const double* u_in, uint64_t* rng,
                              long rng_lanes, double* u_out, double* x, double* kl, long n, long L,
                              long ld_mu, long ld_s, double* ws, void* stream);
/* VJP.  xbar nullable (= 0); klbar = d loss / d kl, one device scalar
 * (nullable = 0).  mubar = xbar + klbar*x ; sbar = mubar*exp(s)*u - klbar.
 * s has row stride ld_s; mubar and sbar are written with row stride ld_out (both halves of one [rows, 2L]
 * gradient of the encoder output, or dense with ld_out = L). */
int hb_diag_sample_kl_bwd_f32(const float* s, const float* u, const float* x, const float* xbar,
                              const float* klbar, float* mubar, float* sbar, long n, long L, long ld_s,
                              long ld_out, void* stream);
int hb_diag_sample_kl_bwd_f64(const double* s, const double* u, const double* x, const double* xbar,
                              const double* klbar, double* mubar, double* sbar, long n, long L, long ld_s,
                              long ld_out, void* stream);
/* full-rank q over `rows` independent blocks: x_r = mu_r + tril(S_r) u_r ;
 * kl = -0.5*sum(log S_kk^2 + u^2 - x^2).  mu/u/x: [rows,size].  S: packed == 0: dense
 * [rows,size,size] (upper part ignored); packed != 0: the lower triangle only,
 * [rows, size(size+1)/2] in numpy tril_indices (row-major) order -- half the bytes. */
int hb_fullrank_sample_kl_fwd_f32(const float* mu, const float* S, const float* u_in, uint64_t* rng,
                                  long rng_lanes, float* u_out, float* x, float* kl, long rows,
                                  long size, int packed, float* ws, void* stream);
int hb_fullrank_sample_kl_fwd_f64(const double* mu, const double* S, const double* u_in,
                                  uint64_t* rng, long rng_lanes, double* u_out, double* x,
                                  double* kl, long rows, long size, int packed, double* ws,
                                  void* stream);
/* The same in ONE launch for a block of up to 1024 dimensions (rows * size <= 8192; cfg 3's q(u)): every workgroup draws u
 * itself from the unchanged generator states, a wave owns rows k and size - 1 - k, the last workgroup to arrive folds the
 * KL partials and advances the generator.  `sync`: one zero 32-bit word owned by the caller for this stream (zero at
 * entry, left zero).  Shapes outside hb_fullrank_one_launch_shape, or sync == NULL: the three-launch form above.  Same
 * variates bit for bit; x and kl agree with the three-launch form to rounding. */
int hb_fullrank_one_launch_shape(long rows, long size);
int hb_fullrank_sample_kl_fwd1_f32(const float* mu, const float* S, const float* u_in, uint64_t* rng,
                                   long rng_lanes, float* u_out, float* x, float* kl, long rows, long size,
                                   int packed, float* ws, unsigned* sync, void* stream);
int hb_fullrank_sample_kl_fwd1_f64(const double* mu, const double* S, const double* u_in, uint64_t* rng,
                                   long rng_lanes, double* u_out, double* x, double* kl, long rows, long size,
                                   int packed, double* ws, unsigned* sync, void* stream);
/* mubar = xbar + klbar*x ; Sbar = tril(mubar u^T) - klbar*diag(1/S_kk) ; strictly upper = 0
 * (dense) or absent (packed: Sbar has S's packed layout) */
int hb_fullrank_sample_kl_bwd_f32(const float* S, const float* u, const float* x, const float* xbar,
                                  const float* klbar, float* mubar, float* Sbar, long rows,
                                  long size, int packed, void* stream);
int hb_fullrank_sample_kl_bwd_f64(const double* S, const double* u, const double* x,
                                  const double* xbar, const double* klbar, double* mubar,
                                  double* Sbar, long rows, long size, int packed, void* stream);
/* The reference's one (disabled) native-op pair, Henbun/tf_wraps.py:50-71: v [B, N(N+1)/2] <-> lower-
 * triangular tri [B,N,N] (zeros above the diagonal), entries in numpy tril_indices order
 * (transforms.py:225-244); each is the other's gradient (tf_wraps.py:56-58). */
int hb_vec_to_tri_f32(const float* v, float* tri, long B, long N, void* stream);
int hb_vec_to_tri_f64(const double* v, double* tri, long B, long N, void* stream);
int hb_tri_to_vec_f32(const float* tri, float* v, long B, long N, void* stream);
int hb_tri_to_vec_f64(const double* tri, double* v, long B, long N, void* stream);

/* ---- K3: stationary Gram matrices (reference gp/kernels.py:54-84
 *      square_dist, :110-111 UnitRBF.K, :122-131 UnitCsymRBF) -------------- */
enum { HB_KERN_RBF = 0, HB_KERN_CSYM_RBF = 1, HB_KERN_SQDIST = 2 /* the scaled squared distance itself */,
       HB_KERN_KBAR_SYMMETRIC = 256 /* hb_gram_bwd only, OR-ed into `kind`: Kbar is symmetric (the Cholesky VJP's output):
                                       the one-pass form need not read the transposed entries */ };
/* K[b,i,j] = k(X[b,i,:], X2[b,j,:]); sX/sX2 = batch strides in elements (0 =
 * shared); ell has dl = 1 (scalar) or d entries (ARD), post-transform; sEll = 0
 * (one kernel for the whole batch) or dl (a lengthscale vector per batch entry:
 * independent experts). */
/* diag_add is added to K[b,i,i] (the jitter of kern.Cholesky, gp/kernels.py:101; 0 otherwise). */
int hb_gram_fwd_f32(int kind, const float* X, long sX, const float* X2, long sX2, const float* ell,
                    long sEll, long dl, float* K, long B, long n, long n2, long d, double diag_add,
                    void* stream);
int hb_gram_fwd_f64(int kind, const double* X, long sX, const double* X2, long sX2,
                    const double* ell, long sEll, long dl, double* K, long B, long n, long n2, long d,
                    double diag_add, void* stream);
/* VJP: Xbar[B,n,d], X2bar[B,n2,d] (either nullable), ellbar[dl] or [B,dl] when sEll != 0
 * (nullable).  ws >= B*n*d elements when ellbar != NULL.  X2bar == Xbar (with X2 == X):
 * the total gradient w.r.t. the shared points is written once (kind | HB_KERN_KBAR_SYMMETRIC: for a symmetric Kbar,
 * without the strided reads of the transposed entries). */
int hb_gram_bwd_f32(int kind, const float* X, long sX, const float* X2, long sX2, const float* ell,
                    long sEll, long dl, const float* Kbar, float* Xbar, float* X2bar, float* ellbar,
                    long B, long n, long n2, long d, float* ws, void* stream);
int hb_gram_bwd_f64(int kind, const double* X, long sX, const double* X2, long sX2,
                    const double* ell, long sEll, long dl, const double* Kbar, double* Xbar,
                    double* X2bar, double* ellbar, long B, long n, long n2, long d, double* ws,
                    void* stream);

/* ---- dense linear algebra on MFMA (f32: v_mfma_f32_32x32x2_f32, f64:
 *      v_mfma_f64_16x16x4_f64) --------------------------------------------- */
enum {
  HB_MM_LOWER_OUT = 1, /* only tiles touching the lower triangle of C are computed; the rest of C is left alone */
  HB_MM_TRIL_OUT = 2,  /* C = tril(result): as LOWER_OUT, and the strict upper triangle is written as zero */
  HB_MM_PHI_OUT = 4,   /* C = Phi(result): strict lower kept, diagonal halved, strict upper zero (Cholesky VJP) */
  HB_MM_SYM_OUT = 8,   /* C = (R + R^T)/2 of the square result R (needs the workspace: ws_elems >= batch*M*N;
                          bias/act/beta are not applied) */
  HB_MM_ACTGRAD = 16   /* C = alpha * result * act'(Y): `bias` then points to Y = the activation OUTPUT of the layer
                          being differentiated, [batch, M, N] contiguous (sBias = M*N or 0), and `act` names the
                          activation: y(1-y), [y > 0], 1-y^2.  The MLP backward's "dx GEMM, then activation-gradient
                          pass" in one launch; beta must be 0 and no other flag may be set */,
  HB_MM_SYMLOW_OUT = 32, /* C[i][j] = C[j][i] = 0.5 * result[max(i,j)][min(i,j)] (hb_matutil mode 4 as an epilogue): only the
                          tiles touching the lower triangle are computed; square result, no bias / activation / beta */
  HB_MM_COLSUM_B = 64   /* (set by hb_matmul_colsum_*) the column sums of op(B) are produced next to C */
};
enum { HB_ACT_NONE = 0, HB_ACT_SIGMOID = 1, HB_ACT_RELU = 2, HB_ACT_TANH = 3 };
/* C[b] = act(alpha * op(A[b]) op(B[b]) + bias[b]) + beta * C[b], op = transpose if trans?.
 * A is M x K (after op), B is K x N, C is M x N; ld* = row strides, s* = batch
 * strides (0 = broadcast), bias nullable = per-column [N] (sBias batch stride).
 * Replaces tf.matmul (reference gp/gp.py:50,122,125,171; nn.py:32) and, with
 * bias/act, the fused MatBias layer clip(x@w+b) + activation (nn.py:31-32,79-84).
 * ws: split-K scratch (nullable -> no split). */
int hb_matmul_f32(const float* A, const float* B, float* C, long batch, long M, long N, long K,
                  long lda, long ldb, long ldc, long sA, long sB, long sC, int transA, int transB,
                  double alpha, double beta, const float* bias, long sBias, int act, int flags,
                  float* ws, long ws_elems, void* stream);
int hb_matmul_f64(const double* A, const double* B, double* C, long batch, long M, long N, long K,
                  long lda, long ldb, long ldc, long sA, long sB, long sC, int transA, int transB,
                  double alpha, double beta, const double* bias, long sBias, int act, int flags,
                  double* ws, long ws_elems, void* stream);

/* C = A^T B together with colsum[n] = sum_k B[k][n]: the weight gradient dW = X^T G of a MatBias layer AND its bias
 * gradient db = sum of the rows of G (reference nn.py:31-32 backward: tf.gradients of x @ w + b) from ONE pass over
 * G -- the workgroups of the first tile row fold the columns of B while it streams through them, the split-K finish
 * launch folds the slab partials; no stand-alone reduction launches.  A: [K, M] (lda), B: [K, N] (ldb), C: [M, N]; one
 * matrix; ws as in hb_matmul plus 64*N elements.  Shapes the fused form does not take (unaligned operands, K % 16 != 0)
 * fall back to hb_matmul followed by hb_reduce: same results up to summation order. */
int hb_matmul_colsum_f32(const float* A, const float* B, float* C, float* colsum, long M, long N, long K, long lda, long ldb,
                         long ldc, float* ws, long ws_elems, void* stream);
int hb_matmul_colsum_f64(const double* A, const double* B, double* C, double* colsum, long M, long N, long K, long lda,
                         long ldb, long ldc, double* ws, long ws_elems, void* stream);

/* Which form hb_matmul_f32 / _f64 (colsum != 0: hb_matmul_colsum_*) takes for a call, asked on the host: the launcher
 * and this query share one decision function, and nothing is launched.  elem_bytes: 4 / 8; the extents, strides, transposes,
 * beta and flags as the call passes them; a_aligned / b_aligned: the A / B base pointer is 16-byte aligned; ws_elems: as
 * passed (0: no workspace).  Returns HB_MM_FORM_*, or -1 for an empty product and for whatever the call rejects that
 * these arguments show: a leading dimension too small, batch > 65535, an operand past 32-bit indexing, a grid too
 * large, SYM_OUT / SYMLOW_OUT / ACTGRAD with M != N, beta != 0, another flag or (SYM_OUT) too small a workspace, and
 * with colsum != 0 anything but one A^T B product over contiguous B (the launcher tests through the same functions).
 * What the call rejects by `bias`, `act` or a NULL pointer the query does not see.  Where the pointers are not NULL,
 * for the two tile-engine forms: *S = contraction slabs (1: no split), *vec = the 16-byte operand
 * path, *finish = a finish launch follows (S > 1 or SYM_OUT), *bfast = the batch index is fastest in the grid
 * (batch % 8 == 0), *colsum_fused = the column sums ride in the product (0: a reduction launch of their own).  For the
 * other forms S = 1 and the rest are 0.  The mm_* switches of hb_debug_set are honoured. */
enum {
  HB_MM_FORM_TILE64 = 0,  /* matmul_kernel, 64 x 64 tiles */
  HB_MM_FORM_TILE128 = 1, /* matmul_kernel, 128 x 128 tiles */
  HB_MM_FORM_WGK = 2,     /* matmul_wgk_kernel: split-K inside the workgroup (fp32) */
  HB_MM_FORM_ROWS = 3,    /* matmul_rows_kernel: tall A, weights resident in LDS (fp32) */
  HB_MM_FORM_ROWSREG = 4  /* matmul_rowsreg_kernel: tall A, weights in registers (fp32) */
};
int hb_matmul_form(int elem_bytes, long batch, long M, long N, long K, long lda, long ldb, long ldc, long sA, long sB,
                   int transA, int transB, double beta, int flags, int a_aligned, int b_aligned, long ws_elems, int colsum,
                   int* S, int* vec, int* finish, int* bfast, int* colsum_fused);

/* ---- K7 fused: the amortised encoder in one launch per direction (csrc/mlp.hip; round 4).
 * o = act(y w0 + b0) w1 + b1   [n, 32] = [q_mu (16) | q_sqrt = log-std (16)]   (NeuralNet of two MatBias layers,
 * reference nn.py:31-32,73-84, fed to a LOCAL diagonal Normal, variationals.py:121-129), x = mu + exp(s) u and
 * kl = -0.5 sum(2 s + u^2 - x^2) (variationals.py:138-142,225-230); the hidden layer is never written.  The backward
 * recomputes it from y and returns the four weight gradients (no gradient for y: a data operand).
 * fp32; hb_mlp2_sample_supported(n, din, hid, nout, rng_lanes, has_u) == 1: din in {32, 64}, hid in {128, 256}, nout = 32,
 * n % 32 == 0 and, for in-kernel noise, rng_lanes >= 2 n (one generator lane per row and half: its draw differs from
 * hb_diag_sample_kl's lane assignment).  u_in nullable -> drawn from rng; u_out receives the noise used.
 * ws: hb_mlp2_sample_ws_elems(n, din, hid) elements (KL partials; the backward's per-chunk partial sums). */
int hb_mlp2_sample_supported(long n, long din, long hid, long nout, long rng_lanes, int has_u);
long hb_mlp2_sample_ws_elems(long n, long din, long hid);
int hb_mlp2_sample_fwd_f32(const float* y, const float* w0, const float* b0, const float* w1, const float* b1, int act,
                           const float* u_in, uint64_t* rng, long rng_lanes, float* x, float* kl, float* u_out, float* o,
                           long n, long din, long hid, float* ws, void* stream);
/* xbar [n,16] (nullable) and klbar [1] (nullable): gradients w.r.t. x and kl; o, u, x: the forward's outputs. */
int hb_mlp2_sample_bwd_f32(const float* y, const float* w0, const float* b0, const float* w1, int act, const float* o,
                           const float* u, const float* x, const float* xbar, const float* klbar, float* dw0, float* db0,
                           float* dw1, float* db1, long n, long din, long hid, float* ws, void* stream);

/* K4: L = chol(A), lower, batched [B,M,M]; the strict upper triangle of L is
 * zeroed; info[B] (device) receives 0 or k+1.  Replaces tf.cholesky
 * (reference gp/kernels.py:101; gp/gp.py:135).  A and L must NOT alias (workgroups
 * re-read diagonal tiles of A while L is being written); only the lower triangle
 * of A is significant beyond its diagonal tiles. */
int hb_cholesky_f32(const float* A, float* L, long B, long M, int* info, void* stream);
int hb_cholesky_f64(const double* A, double* L, long B, long M, int* info, void* stream);

/* K4+K6 fused: L = chol(A) and W = L^-1 from the same launches (the identity is
 * eliminated alongside A: the inverse costs extra width per launch, no extra
 * depth).  fp32 with M % 64 == 0 runs as ONE persistent launch (csrc/chol_persist.cuh): workgroups keep their tiles
 * in registers for the whole factorisation and hand finished 16-column chunks of a panel to each other through ws.
 * ws: hb_cholesky_inverse_ws_elems(B, M, sizeof element) elements (B*M*M, plus the persistent launch's sync words).
 * WORKSPACE CONTRACT (fp32, M % 64 == 0): the sync words behind the first B*M*M elements must be ZERO when a call
 * starts.  The caller zero-fills a workspace once, after allocating it (or whenever something else wrote into it);
 * every call leaves them zero again, so the same workspace serves call after call (graph replays included) as long
 * as it is used with the same (B, M) and by one stream at a time.  info[b] = -1 reports a synchronisation timeout
 * (dirty sync words, or a device that stopped making progress for 2 s): the outputs are then invalid.
 * Replaces the tf.cholesky +
 * tf.matrix_triangular_solve(Lm, .) pair of SparseGP.samples (reference
 * gp/gp.py:135,162,169).  A, L, W must not alias.
 * Wfrag (nullable; 2*B*M*M elements, needs M % 32 == 0): fragment-major copies of W and of W^T --
 * [B][M/32 row tiles t][M/32 k chunks Q][4 v][64 lanes (li + 32 h)][4 s] = W[32t+li][32Q+16h+4v+s] (then the
 * same for W^T) -- the order in which the MFMA operand loads of hb_sgp_fwd / hb_sgp_bwd consume them, so that
 * every load instruction reads one contiguous kilobyte.
 * frag_bf16x3 != 0 (fp32 only): Wfrag has 5*B*M*M elements and, behind the two fp32 images, receives the bf16x3
 * operand images of W and W^T (3 + 3 planes of B*M*M bf16: each fp32 entry split into hi + mid + lo bf16 terms;
 * [term][B][t][Q][k16-step q][64 lanes][8] = X[32t+li][32Q+16q+8h+j]) for the HB_PREC_BF16X3 contractions. */
long hb_cholesky_inverse_ws_elems(long B, long M, int elem_bytes);
/* elements of Wfrag for this (B, M): 2*B*M*M, or 5*B*M*M with the bf16x3 planes */
long hb_cholesky_frag_elems(long B, long M, int bf16x3);
/* 1 when hb_cholesky_inverse_f32 takes the persistent launch for this (B, M) (and the diagnostic switch leaves it on). */
int hb_cholesky_persistent_shape(long B, long M, int elem_bytes);
/* hb_gram_fwd with X2 = X and a diag_add, followed by hb_cholesky_inverse, as one launch: the persistent kernel synthesises its tiles of
 * K(X, X) + diag_add I from the points (the same per-entry function as hb_gram_fwd: the same bits), K itself is never
 * written.  kern.Cholesky(z) feeding SparseGP's whitening, reference gp/kernels.py:93-101 + gp/gp.py:159-162.
 * Only where hb_cholesky_persistent_shape(B, M, 4) is 1; X [B or 1][M, d] (sX = 0: shared), ell as in hb_gram_fwd. */
int hb_gram_cholesky_inverse_f32(int kind, const float* X, long sX, const float* ell, long sEll, long dl, long d,
                                 double diag_add, float* L, float* W, long B, long M, int* info, float* ws,
                                 float* Wfrag, int frag_bf16x3, void* stream);
int hb_cholesky_inverse_f32(const float* A, float* L, float* W, long B, long M, int* info, float* ws,
                            float* Wfrag, int frag_bf16x3, void* stream);
int hb_cholesky_inverse_f64(const double* A, double* L, double* W, long B, long M, int* info,
                            double* ws, double* Wfrag, int frag_bf16x3, void* stream);
/* W = L^{-1} (lower triangular inverse), batched.  Used in place of
 * tf.matrix_triangular_solve(Lm, .) (reference gp/gp.py:162,169): the
 * reference's own batched branch forms the explicit inverse the same way.
 * ws >= B*M*M elements (nullable when M <= 32); W must not alias L. */
int hb_trinv_f32(const float* L, float* W, long B, long M, float* ws, void* stream);
int hb_trinv_f64(const double* L, double* W, long B, long M, double* ws, void* stream);

/* ---- K5/K6: fused sparse-GP conditional (reference gp/gp.py:99-143 samples,
 *      :146-162 _effective_LT, :177-189 _additional_cov 'diagonal') -------- */
enum { HB_SGP_NEGLECTED = 0, HB_SGP_DIAGONAL = 1, HB_SGP_FULLRANK = 2 /* hb_sgp_predict_* only */ };
enum { HB_SGP_S_DIAG = 0, HB_SGP_S_TRIL = 1 };   /* the posterior factor S of hb_sgp_predict_* */
/* Operand precision of the M^2 n contraction.  NATIVE: the arithmetic type (fp32 / fp64 MFMA).  BF16X3 (fp32
 * only; BASELINE cfg 5's "fp16-with-fp32-accum" variant in a usable form): every fp32 operand is split into three
 * bf16 terms and the six significant cross products run on v_mfma_f32_32x32x16_bf16 with fp32 accumulation --
 * fp32-level accuracy (plain 16-bit operands leave a 27 % error in L^-1 K) at the bf16 matrix rate.  Needs the
 * bf16 images of hb_cholesky_inverse_f32 (frag_bf16x3 = 1) in Wfrag. */
enum { HB_PREC_NATIVE = 0, HB_PREC_BF16X3 = 1 };
/* Per expert e < E (all arrays carry a leading E; x may be shared: sx = 0):
 *   Kmn = k(z, x)            [M,n]   (never written to memory)
 *   A   = W Kmn              [M,n]   W = chol(Kmm + jitter I)^{-1}
 *   mean= u A                [P,n]
 *   v   = kdiag(x) - sum_m A^2        [n]
 *   f   = mean + sqrt(|v|) * eps      (DIAGONAL; eps [n] shared by the P rows,
 *                                      reference gp/gp.py:131-132)  or mean (NEGLECTED)
 * eps_in nullable -> drawn from rng; eps_out [E,n] receives the noise used.
 * Wfrag (nullable): the fragment-major copies hb_cholesky_inverse wrote for this W (faster operand loads).
 * ws >= hb_sgp_ws_elems(...) elements. */
long hb_sgp_ws_elems(long E, long n, long M, long d, long P);
/* Column-strip form and fragment-major exchange.  With Wfrag and hb_sgp_strip_path(...) == 1 the contraction runs
 * as column strips (one workgroup = 32 data columns x all M rows) and A may be left -- additionally (A_frag), or
 * only (A == NULL) -- in FRAGMENT-MAJOR layout for hb_sgp_bwd:
 *   A_frag [E][M/32 row tiles t][nS = ceil(n/32) strips s][4 v][64 lanes (li + 32 h)][4 s'] = A[32t+li][32s+16h+4v+s']
 * (zeros past column n): the MFMA operand fragments of the Lbar contraction over the data axis, in load order. */
int hb_sgp_strip_path(long E, long n, long M, long d, long P, int prec);
/* elements (of the arithmetic type) of a fragment-major [E, M, n] buffer -- A_frag, Kbar_frag, Abar_frag: E*M*32*ceil(n/32),
 * or for HB_PREC_BF16X3 three bf16 planes of that many entries (1.5 times the elements) */
long hb_sgp_frag_elems(long E, long n, long M, int prec);
int hb_sgp_fwd_f32(int kind, int mode, const float* x, long sx, const float* z, const float* ell,
                   long dl, const float* W, const float* Wfrag, int prec, const float* u,
                   const float* eps_in, uint64_t* rng, long rng_lanes, float* eps_out, float* A,
                   float* A_frag, float* f, float* v, long E, long n, long M, long d, long P, float* ws,
                   void* stream);
int hb_sgp_fwd_f64(int kind, int mode, const double* x, long sx, const double* z, const double* ell,
                   long dl, const double* W, const double* Wfrag, int prec, const double* u,
                   const double* eps_in, uint64_t* rng, long rng_lanes, double* eps_out, double* A,
                   double* A_frag, double* f, double* v, long E, long n, long M, long d, long P,
                   double* ws, void* stream);
/* The Gaussian likelihood head riding in the forward contraction (fp32, column-strip form, one latent function): where
 * hb_sgp_head_units(...) > 0 the strip kernel that finishes f_j also computes the per-point part of
 * hb_gauss_ll_post -- dmu_j, fbar_j = scale * (post * dmu_j) -- and leaves its strip's partial sums of
 * (ll, dscale, dvar) in head_part[3][units]; hb_gauss_ll_fold_* folds them (chain-aware: a job of the step's last serial
 * chain).  Replaces a launch of its own between the forward and the backward contraction (hb_gauss_ll: 5.6 us of the
 * cfg-2 step).  y [E, n] like f; draw = 1 when eps is drawn from rng (eps_in == NULL, DIAGONAL). */
long hb_sgp_head_units(long E, long n, long M, long d, long P, int prec, int has_wfrag, int draw, long rng_lanes);
int hb_sgp_fwd_gauss_f32(int kind, int mode, const float* x, long sx, const float* z, const float* ell, long dl,
                         const float* W, const float* Wfrag, int prec, const float* u, const float* eps_in,
                         uint64_t* rng, long rng_lanes, float* eps_out, float* A, float* A_frag, float* f, float* v,
                         long E, long n, long M, long d, long P, float* ws, const float* y, const float* scale,
                         const float* var, double post, float* dmu, float* fbar, float* head_part, long units,
                         void* stream);
/* Early-start forward (round 4): the forward contraction INSIDE the launch of the factorisation that feeds it.  Row block j
 * of W = L^-1 is final as soon as panel j of the persistent factorisation is done, so the strips of A = W K(z, x) can
 * take their row tiles while the factorisation is still running on a quarter of the chip (csrc/sgp.hip, early-start form).
 * Protocol, per thread:  hb_sgp_rider_begin();  ONE hb_sgp_fwd_f32 / hb_sgp_fwd_gauss_f32 call -- recorded, not launched
 * (its W / Wfrag are the buffers the factorisation is about to write; hb_sgp_rider_supported(...) must be 1 for its
 * arguments, otherwise the call fails);  then hb_cholesky_inverse_f32 / hb_gram_cholesky_inverse_f32 with the same
 * Wfrag: ONE launch runs the factorisation, this thread's pending side jobs and the recorded forward.  If the
 * factorisation cannot take it (other buffers, batch, size; bf16x3 images; more workgroups than two per CU) it launches
 * as usual and the recorded forward right behind it, so the results never depend on whether the ride happened (bits of A:
 * the last two row tiles are summed in three partial sums when it did).  hb_sgp_rider_flush launches a recorded
 * forward that no factorisation picked up.  Reference: gp/gp.py:159-172 (L^-1 K(z, x) behind tf.cholesky). */
int hb_sgp_rider_supported(long E, long n, long M, long d, long P, int prec, int has_wfrag, int draw, long rng_lanes);
int hb_sgp_rider_begin(void);
int hb_sgp_rider_pending(void);
int hb_sgp_rider_flush(void* stream);
/* The Gram VJP in the epilogue of the product that computes Kbar (round 4).  The Cholesky VJP ends in S = L^-T Phi L^-1
 * (reference: TF's _CholeskyGrad behind tf.cholesky gp/kernels.py:101), whose only reader is the VJP of K(X, X) + jitter I
 * (gp/kernels.py:54-101): C[batch, M, M] = op(A) op(B) as hb_matmul computes it (in-workgroup split-K form: fp32, M % 32 == 0,
 * K % 128 == 0, <= 1024 tiles -- hb_matmul_gram_vjp_ok) AND, from the same launch, Xbar[batch, M, d] and the lengthscale
 * row partials ell_partial[batch * M, d] of hb_gram_bwd's one-pass symmetric form (UnitRBF, Kbar symmetric).  `part`:
 * hb_matmul_gram_vjp_ws_elems(batch, M, d) scratch elements; `counters`: batch * M / 32 zero 32-bit words, left zero.
 * hb_gram_ell_fold_* folds the partials into ellbar (the last launch of hb_gram_bwd on its own; chain-aware). */
int hb_matmul_gram_vjp_ok(long M, long K, long batch, long d);
/* The shape part of the rule by which hb_matmul_f32 takes its in-workgroup split-K form (M % 32 == 0, N % 32 == 0,
 * K % 128 == 0, 128 <= K <= 4096, <= 1024 tiles): what a planner may ask before the operands exist.  Alignment, flags
 * and the diagnostic switch mm_no_wgk are NOT part of it -- a call may still take another form. */
int hb_matmul_wgk_shape(long M, long N, long K, long batch);
long hb_matmul_gram_vjp_ws_elems(long batch, long M, long d);
int hb_matmul_gram_vjp_f32(const float* A, const float* B, float* C, long batch, long M, long K, long lda, long ldb,
                           long ldc, long sA, long sB, long sC, int transA, int transB, const float* X, long sX,
                           const float* ell, long sEll, long dl, long d, float* Xbar, float* ell_partial,
                           float* part, unsigned* counters, void* stream);
int hb_gram_ell_fold_f32(const float* partial, long rows, long d, long dl, long groups, float* ellbar, void* stream);
int hb_gram_ell_fold_f64(const double* partial, long rows, long d, long dl, long groups, double* ellbar, void* stream);
/* The same product and epilogue VJP with the launch boundary as the hand-off ("tiles mode"): the launch leaves only the tile
 * partials part[batch][M/32][M/32][32][2 d] (hb_matmul_gram_vjp_ws_elems; plain stores, no counters), and
 * hb_gram_tiles_fold_f32 sums them, every sum in a fixed order, into Xbar[batch, M, d] and ellbar[dl] (lengthscales shared
 * by the batch).  The fold is chain-aware: at the head of a serial chain its loads join the chain's one load phase.
 * C may be NULL: S is then not stored (its only reader was the epilogue).  hb_matmul_gram_vjp_tiles_ok: the rule of
 * hb_matmul_gram_vjp_ok and at most 16384 partials (one chain workgroup, 16 per thread); 0 under
 * hb_debug_set("gram_vjp_tiles", 0). */
int hb_matmul_gram_vjp_tiles_ok(long M, long K, long batch, long d);
int hb_matmul_gram_vjp_tiles_f32(const float* A, const float* B, float* C, long batch, long M, long K, long lda, long ldb,
                                 long ldc, long sA, long sB, long sC, int transA, int transB, const float* X, long sX,
                                 const float* ell, long sEll, long dl, long d, float* part, void* stream);
int hb_gram_tiles_fold_f32(const float* part, long batch, long M, long d, long dl, float* Xbar, float* ellbar, void* stream);
/* The Gaussian likelihood head of a MatBias layer in the layer's own launch (round 4; reference nn.py:31-32 feeding
 * densities.py:25-27 under tf.reduce_sum): f = A[n, K] B[K, N] + bias[N] is consumed in the epilogue of the row-streaming
 * product and never written -- dmu[n, N] = (y - f s) / var, fbar = s (post dmu) when fbar != NULL, and one partial triple
 * of (ll, dscale, dvar) per wave in part[3][units] for hb_gauss_ll_fold.  units = hb_matmul_gauss_units(n, K, N); 0: this
 * shape takes the product and the head as two launches.  Supported: fp32, n >= 2048, 32 < N <= 256, K == 16 or K in {32, 64, 128}.  dmu / fbar agree
 * with hb_gauss_ll on the materialised f to fp32 rounding (the same per-point arithmetic on an f that was never rounded
 * through memory); the three sums are taken in another (fixed) order. */
long hb_matmul_gauss_units(long n, long K, long N);
int hb_matmul_gauss_f32(const float* A, long lda, const float* B, long ldb, const float* bias, const float* y,
                        const float* scale, const float* var, double post, float* dmu, float* fbar, float* part,
                        long units, long n, long K, long N, void* stream);
int hb_gauss_ll_fold_f32(const float* partial, long nb, float* ll, float* dscale, float* dvar, void* stream);
int hb_gauss_ll_fold_f64(const double* partial, long nb, double* ll, double* dscale, double* dvar, void* stream);
/* The contraction alone, A = W k(z,x) (posterior-prediction callers; isolated timing). */
int hb_sgp_A_f32(int kind, const float* x, long sx, const float* z, const float* ell, long dl,
                 const float* W, const float* Wfrag, int prec, float* A, long E, long n, long M, long d,
                 void* stream);
int hb_sgp_A_f64(int kind, const double* x, long sx, const double* z, const double* ell, long dl,
                 const double* W, const double* Wfrag, int prec, double* A, long E, long n, long M,
                 long d, void* stream);
/* Closed-form predictive moments of the sparse-GP conditional (csrc/sgp_predict.hip; not in the reference, whose only
 * route to a prediction is Monte-Carlo draws of gp/gp.py:99-143).  For the draw f = u^T A + residual of hb_sgp_fwd with
 * u ~ N(m, S S^T), per expert e, latent function p and column j:
 *   mean[e,p,j] = m_ep^T A_j
 *   var [e,p,j] = || S_ep^T A_j ||^2 + r_j,   r_j = |1 - sum_m A_mj^2|       (mode HB_SGP_DIAGONAL)
 *                                                  0                          (HB_SGP_NEGLECTED)
 *                                                  1 - sum_m A_mj^2 + jitter  (HB_SGP_FULLRANK: the diagonal of the
 *                                                  residual covariance whose Cholesky factor samples() draws with)
 * computed from A itself (never as a quadratic form in Kmm^-1, which cancels in fp32).  m [E, P, M].  s_kind
 * HB_SGP_S_DIAG: s [E, P, M] holds the standard deviations (diagonal S).  HB_SGP_S_TRIL: s is ONE lower-triangular
 * [R, R] matrix, R = E P M, its strict upper triangle zero; row (e P + p) M + i is the coefficient row of u[e, p, i],
 * so S_ep = s[(e P + p) M .. + M, 0 .. R].  x, sx, z, ell, dl, W, Wfrag as for hb_sgp_fwd.  Forward only.
 * With Wfrag, fp32, M % 32 == 0, 32 <= M <= 512, d <= 4, P <= 4 (HB_SGP_S_TRIL: E P == 1) ONE kernel per call: one
 * workgroup per 32-column strip forms A and (full rank) S^T A in registers / LDS and writes only mean and var.  Every other
 * shape runs chunked: columns in chunks of at most 32768, per chunk hb_sgp_A_*, (full rank) hb_matmul_*, one column-
 * statistics kernel.  ws >= hb_sgp_predict_ws_elems(E, n, M, d, P, s_kind, Wfrag != NULL, sizeof(T)) elements (16-byte
 * aligned; independent of n beyond one chunk). */
long hb_sgp_predict_ws_elems(long E, long n, long M, long d, long P, int s_kind, int has_wfrag, int dtype_bytes);
/* 1 when hb_sgp_predict_* runs its fused streaming kernel for these extents (else: column chunks) */
int hb_sgp_predict_fused(long E, long n, long M, long d, long P, int s_kind, int has_wfrag, int dtype_bytes);
int hb_sgp_predict_f32(int kind, const float* x, long sx, const float* z, const float* ell, long dl, const float* W,
                       const float* Wfrag, const float* m, const float* s, int s_kind, int mode, double jitter, float* mean,
                       float* var, long E, long n, long M, long d, long P, float* ws, void* stream);
int hb_sgp_predict_f64(int kind, const double* x, long sx, const double* z, const double* ell, long dl, const double* W,
                       const double* Wfrag, const double* m, const double* s, int s_kind, int mode, double jitter,
                       double* mean, double* var, long E, long n, long M, long d, long P, double* ws, void* stream);
/* The same moments for C latent functions of ONE expert with independent full-rank q(u_c) = N(m_c, S_c S_c^T) that share
 * x, z, ell, W and Wfrag (csrc/sgp_predict.hip; the marginals a multi-latent likelihood needs):
 *   mean[c, j] = m_c^T A_j,   var[c, j] = || S_c^T A_j ||^2 + r_j,   r_j as above for HB_SGP_DIAGONAL / HB_SGP_NEGLECTED
 * (any other mode is refused).  m [C, M], S [C, M, M] (the lower triangles are read), mean, var [C, n], 1 <= C <= 64.
 * With Wfrag, fp32, M % 32 == 0, 32 <= M <= 512, d <= 4: ONE strip kernel behind one pack launch (the C fragment-major
 * S_c^T images, C M^2 workspace elements).  A_strip = W K is formed once per strip; the means are taken in groups of 4 and
 * C_c = S_c^T A_strip once per latent function: C + 1 strip products where C calls of hb_sgp_predict_* take 2 C.  Every
 * other shape runs the one-latent chunked form once per latent function.  Either way mean and var hold the BITS of C calls
 * of hb_sgp_predict_*(m_c, S_c, HB_SGP_S_TRIL, E = P = 1) with the same Wfrag.  ws >= hb_sgp_predict_multi_ws_elems(n, M, d,
 * C, Wfrag != NULL, sizeof(T)) elements, 16-byte aligned.  Validated before any launch: the mode, C, the extents, NULL
 * pointers, kind (HB_KERN_RBF only), dl, Wfrag's alignment, the workspace. */
long hb_sgp_predict_multi_ws_elems(long n, long M, long d, long C, int has_wfrag, int dtype_bytes);
/* 1 when hb_sgp_predict_multi_* runs its fused strip kernel for these extents (else: the chunked form per latent function) */
int hb_sgp_predict_multi_fused(long n, long M, long d, long C, int has_wfrag, int dtype_bytes);
int hb_sgp_predict_multi_f32(int kind, const float* x, const float* z, const float* ell, long dl, const float* W,
                             const float* Wfrag, const float* m, const float* S, int mode, float* mean, float* var, long n,
                             long M, long d, long C, float* ws, void* stream);
int hb_sgp_predict_multi_f64(int kind, const double* x, const double* z, const double* ell, long dl, const double* W,
                             const double* Wfrag, const double* m, const double* S, int mode, double* mean, double* var, long n,
                             long M, long d, long C, double* ws, void* stream);
/* Full predictive covariance of the same draw (csrc/sgp_predict_cov.hip; not in the reference).  Per expert e and latent
 * function p, with A_e = L_e^-1 K(z_e, x):
 *   cov[e,p] = A^T S_ep S_ep^T A + K(x, x) - A^T A + jitter I   (mode HB_SGP_FULLRANK: what samples() factorises, plus u)
 *            = A^T S_ep S_ep^T A + diag(|1 - sum_m A_m^2|)        (HB_SGP_DIAGONAL: independent residuals)
 *            = A^T S_ep S_ep^T A                                  (HB_SGP_NEGLECTED)
 * so diag(cov) is hb_sgp_predict's var.  cov [E, P, n, n], written in full and bitwise symmetric (one triangle is computed
 * and mirrored).  x, sx, z, ell, dl, W, Wfrag, s, s_kind as for hb_sgp_predict_*; HB_SGP_S_TRIL needs E P == 1 (S is then
 * [M, M]).  Forward only.  Two passes: hb_sgp_A_* writes A into ws (from Wfrag when given), a full-rank S adds
 * C = S^T A (hb_matmul_*) and HB_SGP_DIAGONAL the column sums of A^2; then fp32 runs one MFMA launch, a workgroup per
 * 128 x 128 lower-triangle tile, the K-loop over the rows of A weighted by s_pk^2 - [FULLRANK] (diagonal S) or
 * -[FULLRANK] (full-rank S, then over the rows of C with weight 1), the RBF block and the diagonal term added in the
 * epilogue; fp64 runs a plain loop in the same order.  ws >= hb_sgp_predict_cov_ws_elems(E, n, M, P, s_kind, sizeof(T))
 * elements (16-byte aligned; O((E + 1) M n), linear in n). */
long hb_sgp_predict_cov_ws_elems(long E, long n, long M, long P, int s_kind, int dtype_bytes);
int hb_sgp_predict_cov_f32(int kind, const float* x, long sx, const float* z, const float* ell, long dl, const float* W,
                           const float* Wfrag, const float* s, int s_kind, int mode, double jitter, float* cov, long E, long n,
                           long M, long d, long P, float* ws, void* stream);
int hb_sgp_predict_cov_f64(int kind, const double* x, long sx, const double* z, const double* ell, long dl, const double* W,
                           const double* Wfrag, const double* s, int s_kind, int mode, double jitter, double* cov, long E,
                           long n, long M, long d, long P, double* ws, void* stream);
/* Sufficient statistics of the whole data set for the closed-form optimal q(u) and the collapsed bound of the whitened
 * sparse GP regression model (csrc/sgp_stats.hip; not in the reference).  With A = W k(z, X) [M, N], W = Lm^-1:
 *   Phi [M, M] = A A^T,   b [P, M] = (A Y)^T,   yy [P] = sum_j Y[j, p]^2,   a2sum [1] = tr Phi = sum_j sum_m A_mj^2
 * ALWAYS double, whatever the input type.  Phi is written in full and bitwise symmetric (the lower triangle is computed
 * and mirrored); a2sum is the fold of its diagonal.  X [N, d] and Y [N, P] row-major; z [M, d], ell [dl], W [M, M], Wfrag
 * (nullable) as for hb_sgp_A_* with E = 1.  kind must be HB_KERN_RBF; N >= 1, d >= 1, P >= 1.  One streaming pass in
 * column chunks of at most 32768: per chunk hb_sgp_A_* writes A_c into ws; fp32 with M % 32 == 0 and P <= 4 then runs a
 * split-K symmetric rank update on MFMA (128 x 128 lower-triangle tiles x K-splits, fp32 accumulation inside one split
 * only) whose partial tiles a second launch folds into Phi and b in double, in a fixed order (bitwise reproducible; no
 * atomics); every other shape runs plain loops in double.  The fp32 entry forms A in float32
 * (profiles/sgp_stats_errors.txt).  ws >= hb_sgp_stats_ws_elems(N, M, d, P, sizeof(T)) elements of T, 16-byte aligned;
 * the same for every N above one chunk. */
long hb_sgp_stats_ws_elems(long N, long M, long d, long P, int dtype_bytes);
int hb_sgp_stats_f32(int kind, const float* X, const float* Y, const float* z, const float* ell, long dl, const float* W,
                     const float* Wfrag, double* Phi, double* b, double* yy, double* a2sum, long N, long M, long d, long P,
                     float* ws, void* stream);
int hb_sgp_stats_f64(int kind, const double* X, const double* Y, const double* z, const double* ell, long dl, const double* W,
                     const double* Wfrag, double* Phi, double* b, double* yy, double* a2sum, long N, long M, long d, long P,
                     double* ws, void* stream);
/* Weighted form of hb_sgp_stats_* (csrc/sgp_stats.hip; not in the reference), the data pass of a natural-gradient step
 * on q(u) under any factorising likelihood (SparseGP.natgrad_q).  With A = W k(z, X) [M, N]:
 *   Phi [M, M] = A diag(w) A^T,   b [1, M] = (A r)^T,   tr [1] = tr Phi
 * ALWAYS double.  w [N] (16-byte aligned) and r [N] in the storage type; weights of either sign and zeros are taken as
 * they are: the weight multiplies the column operand of the rank update as it is staged (fp32 MFMA form: A_c diag(w)
 * rounded to float32 once; plain form: in double), A is never scaled by a root.  Chunking, K-splits, the fold in split
 * order and the final mirror are those of hb_sgp_stats_*: Phi is bitwise symmetric, two calls return the same bits, and
 * with w == 1, r = Y[:, 0] Phi and b have the bits of hb_sgp_stats_*.  Every other argument as for hb_sgp_stats_*;
 * ws >= hb_sgp_wstats_ws_elems(N, M, d, sizeof(T)) elements of T (= hb_sgp_stats_ws_elems with P = 1). */
long hb_sgp_wstats_ws_elems(long N, long M, long d, int dtype_bytes);
int hb_sgp_wstats_f32(int kind, const float* X, const float* w, const float* r, const float* z, const float* ell, long dl,
                      const float* W, const float* Wfrag, double* Phi, double* b, double* tr, long N, long M, long d, float* ws,
                      void* stream);
int hb_sgp_wstats_f64(int kind, const double* X, const double* w, const double* r, const double* z, const double* ell, long dl,
                      const double* W, const double* Wfrag, double* Phi, double* b, double* tr, long N, long M, long d,
                      double* ws, void* stream);
/* hb_sgp_wstats_* for C weight sets from ONE A (csrc/sgp_stats.hip; not in the reference): the data pass of a
 * natural-gradient step on C independent q(u_c) that share z, the lengthscales and W (SparseGP.natgrad_q with a
 * multi-latent likelihood).  Row c of w and r starts at w + c ldw, r + c ldw (ldw >= N; C = 1: ldw is not read):
 *   Phi [C, M, M]: Phi_c = A diag(w_c) A^T,   b [C, M]: b_c = (A r_c)^T,   tr [C]: tr Phi_c.
 * Per column chunk hb_sgp_A_* runs once; the rank update and its fold then run set by set over that A_c through one set
 * of partial tiles.  Chunk size, K-splits, fold order and mirror are those of hb_sgp_wstats_*: Phi_c, b_c, tr_c have the
 * BITS of hb_sgp_wstats_*(w_c, r_c).  Every row of w must start 16-byte aligned (fp32: ldw % 4 == 0 when C > 1); refused
 * before any launch otherwise.  ws >= hb_sgp_mwstats_ws_elems(N, M, d, C, sizeof(T)) elements of T -- those of
 * hb_sgp_wstats_ws_elems, whatever C. */
long hb_sgp_mwstats_ws_elems(long N, long M, long d, long C, int dtype_bytes);
int hb_sgp_mwstats_f32(int kind, const float* X, const float* w, const float* r, long ldw, const float* z, const float* ell,
                       long dl, const float* W, const float* Wfrag, double* Phi, double* b, double* tr, long N, long M, long d,
                       long C, float* ws, void* stream);
int hb_sgp_mwstats_f64(int kind, const double* X, const double* w, const double* r, long ldw, const double* z, const double* ell,
                       long dl, const double* W, const double* Wfrag, double* Phi, double* b, double* tr, long N, long M, long d,
                       long C, double* ws, void* stream);
/* Psi statistics: the data pass of the closed-form routes under UNCERTAIN inputs x_n ~ N(Xmean_n, diag(Xvar_n)), Xvar >= 0
 * (csrc/sgp_psi.hip; not in the reference).  For the unit RBF kernel with lengthscales l_k, a_k = 1 / (l_k^2 + 2 s_k):
 *   psi1_n(m)     = prod_k (1 + s_k / l_k^2)^-1/2 exp(-1/2 sum_k (mu_k - z_mk)^2 / (l_k^2 + s_k))                 = E k(x_n, z_m)
 *   psi2_n(m, m') = prod_k (1 + 2 s_k / l_k^2)^-1/2 exp(-1/2 sum_k a_k [(mu_k - z_mk)^2 + (mu_k - z_m'k)^2]
 *                                                      - 1/4 sum_k (z_mk - z_m'k)^2 (1 / l_k^2 - a_k))  = E k(x_n, z_m) k(x_n, z_m')
 *   Psi2 [M, M] = sum_n psi2_n,   C [P, M]: C[p, m] = sum_n psi1_n(m) Y[n, p],   yy [P] = sum_n Y[n, p]^2
 * ALWAYS double, and ALL ARITHMETIC is double whatever the storage type (Phi = W Psi2 W^T amplifies an error of Psi2 by
 * |W|^2 ~ 1 / jitter); the two entries differ in the type they load.  Xvar = 0 in any or all dimensions gives k(x, z_m) and
 * k(x, z_m) k(x, z_m'); a term whose exponent underflows is 0.  Xmean, Xvar [N, d], Y [N, P], z [M, d] row-major, ell [dl],
 * dl 1 or d; kind must be HB_KERN_RBF; N, M, P >= 1, 1 <= d <= 1535.  Cost: N M (M + 1) / 2 double exponentials on the vector
 * unit -- Psi2 is no rank update once the variances differ from point to point.  Workgroups own a 64 x 64 lower-triangle
 * tile of pairs times a split of N (a function of (N, M) alone), the splits' partial tiles go to ws and a second launch
 * folds them in split order: no atomics, two calls return the same bits; Psi2 is written in full and bitwise symmetric.
 * ws >= hb_sgp_psi_stats_ws_elems(N, M, d, P, sizeof(T)) elements of T, 16-byte aligned; the same for every N >= 1.
 * Refused before any launch: another kind, extents < 1, dl not 1 or d, a NULL pointer, M * M >= 2^31. */
long hb_sgp_psi_stats_ws_elems(long N, long M, long d, long P, int dtype_bytes);
int hb_sgp_psi_stats_f32(int kind, const float* Xmean, const float* Xvar, const float* Y, const float* z, const float* ell,
                         long dl, double* Psi2, double* C, double* yy, long N, long M, long d, long P, float* ws, void* stream);
int hb_sgp_psi_stats_f64(int kind, const double* Xmean, const double* Xvar, const double* Y, const double* z, const double* ell,
                         long dl, double* Psi2, double* C, double* yy, long N, long M, long d, long P, double* ws, void* stream);
/* The two contractions the predictive moments at Gaussian test inputs need (csrc/sgp_psi.hip), per point j of Xmean,
 * Xvar [n, d]:   e1[j] = sum_m beta[m] psi1_j(m),   e2[j] = sum_{m, m'} Q[m, m'] psi2_j(m, m')
 * with beta [M] and Q [M, M] in double; Q is taken as symmetric: its lower triangle is read and the off-diagonal terms
 * doubled.  psi1, psi2 are the functions of hb_sgp_psi_stats_*, evaluated by the same device code.  The pairs of one point
 * are spread over workgroups whose number depends on M alone and are summed in a fixed order: a point's result does not
 * depend on the other points of the call, bit for bit.  n = 0 returns 0 without a launch.
 * ws >= hb_sgp_psi_predict_ws_elems(n, M, d, sizeof(T)) elements of T, 16-byte aligned.  Refusals as above. */
long hb_sgp_psi_predict_ws_elems(long n, long M, long d, int dtype_bytes);
int hb_sgp_psi_predict_f32(int kind, const float* Xmean, const float* Xvar, const float* z, const float* ell, long dl,
                           const double* beta, const double* Q, double* e1, double* e2, long n, long M, long d, float* ws,
                           void* stream);
int hb_sgp_psi_predict_f64(int kind, const double* Xmean, const double* Xvar, const double* z, const double* ell, long dl,
                           const double* beta, const double* Q, double* e1, double* e2, long n, long M, long d, double* ws,
                           void* stream);
/* Gradients of the psi statistics (csrc/sgp_psi_grad.hip; not in the reference).  For a bound that depends on the per-point
 * statistics of hb_sgp_psi_stats_* as
 *   F = 1/2 sum_n sum_{m, m'} Q[m, m'] psi2_n(m, m') + sum_n sum_m rho_nm psi1_n(m),   rho_nm = sum_p R[m, p] Y[n, p]
 * (Q [M, M] symmetric -- its lower triangle is read -- and R [M, P] in double: Q = 2 W^T G W, R = W^T g^T of the collapsed
 * bound), the four gradients, all double and overwritten:
 *   mubar [N, d] = dF/dXmean,  sbar [N, d] = dF/dXvar,  zbar [M, d] = dF/dz,  ellbar [dl] = dF/dell (dl = 1: summed over d)
 * through psi1 and psi2 only (the part through K(z, z) is the caller's).  ALL ARITHMETIC is double whatever the storage
 * type.  Xvar = 0 is exact (no log s is taken); a point whose exponents underflow contributes exact zeros.  Two passes of
 * one exponential per (point, pair of the lower triangle) each: a point-major one for mubar, sbar (one thread per point,
 * the rows of the triangle split over workgroups by a rule of M alone: a point's result does not depend on the other points
 * of the call, bit for bit) and a pair-major one for zbar, ellbar (the tiles and register blocks of hb_sgp_psi_stats_*).
 * Partials go to ws and are folded in a fixed order by further launches: no atomics, two calls return the same bits.
 * ws >= hb_sgp_psi_grad_ws_elems(N, M, d, P, sizeof(T)) elements of T, 16-byte aligned; the same for every N >= 1 (N is
 * walked in chunks).  Refusals, before any launch, as hb_sgp_psi_stats_*. */
long hb_sgp_psi_grad_ws_elems(long N, long M, long d, long P, int dtype_bytes);
int hb_sgp_psi_grad_f32(int kind, const float* Xmean, const float* Xvar, const float* Y, const float* z, const float* ell,
                        long dl, const double* Q, const double* R, double* mubar, double* sbar, double* zbar, double* ellbar,
                        long N, long M, long d, long P, float* ws, void* stream);
int hb_sgp_psi_grad_f64(int kind, const double* Xmean, const double* Xvar, const double* Y, const double* z, const double* ell,
                        long dl, const double* Q, const double* R, double* mubar, double* sbar, double* zbar, double* ellbar,
                        long N, long M, long d, long P, double* ws, void* stream);
/* Sites of a factorising likelihood under Gaussian marginals (csrc/lik_sites.hip; not in the reference).  For
 * f_j ~ N(mu_j, v_j), mu_j = mscale mean[j], v_j = vscale var[j] (the scales take the unit-variance moments of
 * hb_sgp_predict_* to those of f = sqrt(k_var) (..): mscale = sqrt(k_var), vscale = k_var):
 *   l_j = E[log p(y_j | f)],  lam[j] = E[-d2 log p / df2],  beta[j] = E[d log p / df] + lam[j] mu_j,  ell_sum[0] = sum_j l_j.
 *   HB_LIK_GAUSSIAN   y ~ N(f, param), param = the variance > 0: l = -log(2 pi param) / 2 - ((y - mu)^2 + v) / (2 param),
 *                     lam = 1 / param, beta = y / param
 *   HB_LIK_BERNOULLI  y in {0, 1}, log p = y f - softplus(f): 20-node Gauss-Hermite, f_i = mu + sqrt(2 v) x_i
 *   HB_LIK_POISSON    log p = y f - exp(f) - lgamma(y + 1): with e = exp(mu + v / 2), l = y mu - e - lgamma(y + 1), lam = e,
 *                     beta = y - e + e mu
 * y, mean, var, lam, beta [N] in the storage type; all arithmetic is double, rounded once on output and saturated to the
 * largest finite value of the storage type.  ell_sum: per-block partials (ws) folded in block order by a second launch,
 * no atomics -- two calls return the same bits.  ws >= hb_lik_sites_ws_elems(N) doubles (at most 1024).  Validated before
 * any launch: the id, N >= 0, param > 0 for HB_LIK_GAUSSIAN, vscale >= 0.
 * hb_lik_predict_*: mean and variance of a new y given f ~ N(mean[j], var[j]): (mean, var + param); (p, p (1 - p)) with
 * p = E sigmoid(f) by the same rule; (e, e + (exp(var) - 1) e^2).
 *
 * Likelihoods with a parameter of their own (ids from 16; all log-concave in f, so lam >= 0).  delta = mu - y:
 *   HB_LIK_LAPLACE      param = the scale b > 0, log p = -log 2b - |y - f| / b.  Closed form (the kink defeats the rule):
 *                       A = E|y - f| = sqrt(2 v / pi) exp(-delta^2 / 2v) + delta erf(delta / sqrt(2 v)),
 *                       l = -log 2b - A / b, g = erf((y - mu) / sqrt(2 v)) / b, lam = (2 / b) exp(-delta^2 / 2v) / sqrt(2 pi v)
 *                       (v = 0: A = |delta|, g = sign(y - mu) / b, lam = 0).  Predictive (mu, v + 2 b^2)
 *   HB_LIK_GAMMA        param = the shape a > 0, mean exp(f), y > 0 IS THE CALLER'S DUTY (log y is taken as it comes):
 *                       log p = a log a - lgamma(a) + (a - 1) log y - a f - a y exp(-f).  Closed form with
 *                       E = exp(-mu + v / 2): l = a log a - lgamma(a) + (a - 1) log y - a mu - a y E, g = -a + a y E,
 *                       lam = a y E.  Predictive, e = exp(mu + v / 2): (e, e^2 (expm1(v) + exp(v) / a)).  a = 1: exponential
 *   HB_LIK_NEGBINOMIAL  param = the dispersion r > 0, mean exp(f), variance mean + mean^2 / r.  With t = f - log r:
 *                       log p = lgamma(y + r) - lgamma(r) - lgamma(y + 1) + y t - (y + r) softplus(t); 20-node rule,
 *                       g = E[y sigmoid(-t) - r sigmoid(t)], lam = (y + r) E[sigmoid(t) sigmoid(-t)].
 *                       Predictive (e, e + e^2 (expm1(v) + exp(v) / r))
 *   HB_LIK_BINOMIAL     param = the total count n >= 1, integer-valued; logit link, y in {0, .., n}:
 *                       log p = lgamma(n + 1) - lgamma(y + 1) - lgamma(n - y + 1) + y f - n softplus(f); 20-node rule,
 *                       g = E[y sigmoid(-f) - (n - y) sigmoid(f)], lam = n E[sigmoid(f) sigmoid(-f)].  Predictive with
 *                       p = E sigmoid: (n p, n E[sigmoid(f) sigmoid(-f)] + n^2 E[(sigmoid(f) - p)^2]), the second
 *                       expectation taken over the nodes once p is known (no E sigmoid^2 - p^2)
 * Validated before any launch as well: param > 0 for the first three, param >= 1 and integer-valued for HB_LIK_BINOMIAL.
 *
 * hb_lik_param_grad_*: out[0] = sum_j l_j and out[1] = sum_j dl_j / dparam at fixed mu_j, v_j, for the likelihoods whose
 * parameter is continuous; any other known id returns < 0 ("no continuous parameter").  Same scales, grid, per-block
 * partials and fold as hb_lik_sites_* (two calls return the same bits); ws >= hb_lik_param_grad_ws_elems(N) doubles.
 *   HB_LIK_GAUSSIAN     d/dvar:  -1 / (2 s2) + ((y - mu)^2 + v) / (2 s2^2)
 *   HB_LIK_LAPLACE      d/db:    -1 / b + A / b^2
 *   HB_LIK_GAMMA        d/da:    log a + 1 - psi(a) + log y - mu - y E
 *   HB_LIK_NEGBINOMIAL  d/dr:    psi(y + r) - psi(r) - y / r - E[softplus(t)] + (y + r) / r E[sigmoid(t)]   (20-node rule)
 * psi is evaluated in double on the device: the recurrence up to x >= 10, then the asymptotic series through x^-14 (the
 * first term left out is below 5e-17 there; the elementwise table's HB_EW_DIGAMMA stops at 1e-11 and is not used).
 *
 * hb_lik_logdens_*: out[j] = log integral p(y_j | f) N(f; mu_j, v_j) df (out may be NULL) and sum[0] = sum_j out[j] in
 * double by the same fold, for all seven ids; ws >= hb_lik_sites_ws_elems(N) doubles.  Gaussian: the density of
 * N(mu, v + param).  Laplace: closed form, p = e^(v / 2b^2) [e^(-d/b) erfc((v/b - d) / sqrt(2v)) + e^(d/b) erfc((v/b + d) /
 * sqrt(2v))] / 4b with d = y - mu, evaluated in log space through erfcx (a term whose erfc argument z is >= 0 is
 * -d^2 / 2v + log erfcx(z)), so neither |d| / b large nor v small overflows or loses the tail.  The others: the 20-node
 * rule over p(y | f_i), combined by log-sum-exp. */
enum {
  HB_LIK_GAUSSIAN = 0,
  HB_LIK_BERNOULLI = 1,
  HB_LIK_POISSON = 2,
  HB_LIK_LAPLACE = 16,
  HB_LIK_GAMMA = 17,
  HB_LIK_NEGBINOMIAL = 18,
  HB_LIK_BINOMIAL = 19,
  HB_LIK_SOFTMAX = 32,  /* C latent functions: served by hb_lik_softmax_*, refused by the entries above */
  HB_LIK_HETGAUSS = 33  /* two latent functions: served by hb_lik_hetgauss_*, refused by the entries above */
};
long hb_lik_sites_ws_elems(long N);
int hb_lik_sites_f32(int lik, const float* y, const float* mean, const float* var, double mscale, double vscale, double param,
                     float* lam, float* beta, double* ell_sum, long N, double* ws, void* stream);
int hb_lik_sites_f64(int lik, const double* y, const double* mean, const double* var, double mscale, double vscale,
                     double param, double* lam, double* beta, double* ell_sum, long N, double* ws, void* stream);
int hb_lik_predict_f32(int lik, const float* mean, const float* var, double param, float* ymean, float* yvar, long N,
                       void* stream);
int hb_lik_predict_f64(int lik, const double* mean, const double* var, double param, double* ymean, double* yvar, long N,
                       void* stream);
long hb_lik_param_grad_ws_elems(long N);
int hb_lik_param_grad_f32(int lik, const float* y, const float* mean, const float* var, double mscale, double vscale,
                          double param, double* out, long N, double* ws, void* stream);
int hb_lik_param_grad_f64(int lik, const double* y, const double* mean, const double* var, double mscale, double vscale,
                          double param, double* out, long N, double* ws, void* stream);
int hb_lik_logdens_f32(int lik, const float* y, const float* mean, const float* var, double mscale, double vscale, double param,
                       float* out, double* sum, long N, double* ws, void* stream);
int hb_lik_logdens_f64(int lik, const double* y, const double* mean, const double* var, double mscale, double vscale,
                       double param, double* out, double* sum, long N, double* ws, void* stream);
/* Softmax (multi-class) likelihood under C independent Gaussian marginals (csrc/lik_softmax.hip; not in the reference).
 * y [N] holds the labels 0 .. C-1 as numbers of the storage type (labels outside that range ARE THE CALLER'S DUTY: such a
 * point gets g = -mean_s p and contributes nothing to the sums); mean, var [C, N] row-major; mu = mscale mean, v = vscale
 * var as for hb_lik_sites_*.  nodes [S, C]: standard-normal draws shared by all points (double).  With
 * f_sc = mu_jc + sqrt(max(v_jc, 0)) nodes[s, c] and p_s = softmax_c(f_s) (shifted by the maximum):
 *   l_j = mean_s log p_{s, y_j},  g_jc = mean_s ([c = y_j] - p_sc),  lam[c, j] = mean_s p_sc (1 - p_sc)  (Price's form of
 *   -2 dE l / dv_c: never negative),  beta[c, j] = g_jc + lam[c, j] mu_jc,  lsum[0] = sum_j l_j.
 * hb_lik_softmax_predict_*: prob[c, j] = mean_s p_sc (NULL: not written); with y given, logdens[j] = log mean_s p_{s, y_j},
 * combined by log-sum-exp over the nodes -- as log1p(-mean_s (1 - p_{s, y_j})) where that mean of p is above 1/2, so a
 * density near 1 keeps its digits too -- (NULL: not written), and total[0] = sum_j logdens[j] (NULL: not formed).  y NULL
 * with logdens or total asked for is refused.
 * Arithmetic is double in both entries; one rounding on output.  1 - p of the class that carries the maximum is formed
 * from the sum of the OTHER classes' terms, so lam and g keep their relative digits where p is near 1.  lsum and total are
 * per-workgroup partials (ws) folded by a second launch in block order, no atomics: two calls return the same bits.
 * ws >= hb_lik_softmax_ws_elems(N, C) doubles (at most 1024).  Validated before any launch: 2 <= C <= 64, 1 <= S <= 1024,
 * N >= 0 (N = 0 writes lsum = 0 / total = 0 and returns), vscale >= 0. */
long hb_lik_softmax_ws_elems(long N, long C);
int hb_lik_softmax_sites_f32(const float* y, const float* mean, const float* var, double mscale, double vscale,
                             const double* nodes, long S, float* lam, float* beta, double* lsum, long N, long C, double* ws,
                             void* stream);
int hb_lik_softmax_sites_f64(const double* y, const double* mean, const double* var, double mscale, double vscale,
                             const double* nodes, long S, double* lam, double* beta, double* lsum, long N, long C, double* ws,
                             void* stream);
/* Weights of the hyper-parameter gradient of the softmax ELBO at fixed q(u_c) (same file; not in the reference;
 * SparseGP.elbo_and_grad_multi).  Inputs, layout, node tiles, softmax, grid, fold and validation are those of
 * hb_lik_softmax_sites_*; the outputs are the EXACT partial derivatives of the fixed-node value l_j with respect to the
 * marginals, ALWAYS double whatever the storage type, rows ldo >= N apart.  With d_sc = [c = y_j] - p_sc (1 - p on the
 * label lane from the sum of the other classes' terms, never 1 - p with p near 1):
 *   r[c ldo + j] = g_jc = mean_s d_sc                                   (= d l_j / d mu_jc)
 *   w[c ldo + j] = -mean_s(d_sc nodes[s, c]) / sqrt(v_jc)   for v_jc > 0  (= -2 d l_j / d v_jc: signed, unlike lam)
 *   w[c ldo + j] = mean_s p_sc (1 - p_sc)                   for v_jc <= 0 (the node sum has no derivative there; this is
 *                                                           Price's form, the exact expectation's: p (1 - p) at mu where every
 *                                                           class of the point has v = 0)
 *   lsum[0] = sum_j l_j with the BITS of hb_lik_softmax_sites_*'s lsum on the same inputs (the same terms, accumulation
 *   and fold order), so the gradient belongs to the value SparseGP.natgrad_q reports.
 * Two calls return the same bits.  ws >= hb_lik_softmax_ws_elems(N, C) doubles. */
int hb_lik_softmax_grad_f32(const float* y, const float* mean, const float* var, double mscale, double vscale,
                            const double* nodes, long S, double* w, double* r, long ldo, double* lsum, long N, long C,
                            double* ws, void* stream);
int hb_lik_softmax_grad_f64(const double* y, const double* mean, const double* var, double mscale, double vscale,
                            const double* nodes, long S, double* w, double* r, long ldo, double* lsum, long N, long C,
                            double* ws, void* stream);
int hb_lik_softmax_predict_f32(const float* y, const float* mean, const float* var, double mscale, double vscale,
                               const double* nodes, long S, float* prob, float* logdens, double* total, long n, long C,
                               double* ws, void* stream);
int hb_lik_softmax_predict_f64(const double* y, const double* mean, const double* var, double mscale, double vscale,
                               const double* nodes, long S, double* prob, double* logdens, double* total, long n, long C,
                               double* ws, void* stream);
/* Heteroscedastic Gaussian likelihood over TWO latent functions (csrc/lik_sites.hip; not in the reference):
 *   y ~ N(f, exp(g + c)),   param = c, the prior mean of the log noise variance (any finite number).
 * mean, var [2, ld]: row 0 the unit-variance marginals of f, row 1 (ld elements on) those of g; mu = mscale mean, v =
 * vscale var as for hb_lik_sites_*.  With s = (y - mu_f)^2 + v_f and e = exp(-mu_g - c + v_g / 2) the expected log density
 * and its derivatives are closed forms (no quadrature):
 *   l = -1/2 log 2 pi - 1/2 (mu_g + c) - 1/2 s e
 *   dl/dmu_f = (y - mu_f) e,   lam_f = e            dl/dmu_g = -1/2 + 1/2 s e,   lam_g = 1/2 s e
 *   beta = dl/dmu + lam mu;   both lam >= 0, and lam = -2 dl/dv exactly;   dl/dc = dl/dmu_g.
 * hb_lik_hetgauss_sites_*: lam, beta [2, ld] and, when r is not NULL, r [2, ld] = dl/dmu (the weights of the hyper-parameter
 * gradient at fixed q together with w = lam; sum_j r[1, j] = d sum_j l_j / dc), and ell_sum[0] = sum_j l_j.  y [N]; ld >= N
 * (the padding hb_sgp_mwstats_* asks of its weights; elements N .. ld of a row are not touched).  Double arithmetic, rounded
 * once on output and saturated to the largest finite value of the storage type; per-block partials (ws) folded in block
 * order by a second launch, no atomics: two calls return the same bits.
 * hb_lik_hetgauss_predict_*: mean and variance of a new y given f ~ N(mean[0, j], var[0, j]), g ~ N(mean[1, j], var[1, j])
 * (already scaled): ymean = mu_f, yvar = v_f + exp(mu_g + c + v_g / 2); ymean, yvar [n].
 * hb_lik_hetgauss_logdens_*: out[j] = log sum_i w_i N(y_j; mu_f, v_f + exp(mu_g + c + sqrt(2 v_g) x_i)) over the 20-node
 * Gauss-Hermite rule in g (f is integrated in closed form), combined by log-sum-exp (out may be NULL), and sum[0] = sum_j
 * out[j] by the same fold.  ws >= hb_lik_hetgauss_ws_elems(N) doubles (at most 1024) for the two entries that sum.
 * Validated before any launch: N >= 0, ld >= N, a finite c, vscale >= 0, NULL pointers. */
long hb_lik_hetgauss_ws_elems(long N);
int hb_lik_hetgauss_sites_f32(const float* y, const float* mean, const float* var, long ld, double mscale, double vscale,
                              double param, float* lam, float* beta, float* r, double* ell_sum, long N, double* ws,
                              void* stream);
int hb_lik_hetgauss_sites_f64(const double* y, const double* mean, const double* var, long ld, double mscale, double vscale,
                              double param, double* lam, double* beta, double* r, double* ell_sum, long N, double* ws,
                              void* stream);
int hb_lik_hetgauss_predict_f32(const float* mean, const float* var, long ld, double param, float* ymean, float* yvar, long n,
                                void* stream);
int hb_lik_hetgauss_predict_f64(const double* mean, const double* var, long ld, double param, double* ymean, double* yvar,
                                long n, void* stream);
int hb_lik_hetgauss_logdens_f32(const float* y, const float* mean, const float* var, long ld, double mscale, double vscale,
                                double param, float* out, double* sum, long N, double* ws, void* stream);
int hb_lik_hetgauss_logdens_f64(const double* y, const double* mean, const double* var, long ld, double mscale, double vscale,
                                double param, double* out, double* sum, long N, double* ws, void* stream);
/* Pathwise posterior function draws (csrc/sgp_pathwise.hip; not in the reference; Wilson et al. 2020).  S function draws,
 * each a coefficient row coef[s] = [ w_s / sqrt(L) | v_s ] over 2L random Fourier features of the unit RBF kernel and the M
 * canonical basis functions K(z_m, .), evaluated at n points:
 *   out[s, j] = scale ( sum_{l<L} [ coef[s, 2l] cos(p_lj) + coef[s, 2l+1] sin(p_lj) ]
 *                       + sum_{m<M} coef[s, 2L+m] exp(-1/2 sum_k ((z_mk - x_jk) / ell_k)^2) ),   p_lj = sum_k omega_lk x_jk / ell_k.
 * x [n, d], omega [L, d], z [M, d], coef [S, 2L + M], out [S, n], row-major and contiguous; ell [dl], dl in {1, d}.  kind
 * must be HB_KERN_RBF.  L >= 1, S >= 1, d >= 1; M = 0 is legal (the prior path alone; z may then be NULL); n = 0 returns
 * without a launch; n, S (2L + M) and S n below 2^31.  No workspace: ONE launch, the basis is synthesised in LDS (one sincos
 * per (l, j), phases reduced in double in revolutions: exact to the rounding of the result for |p| in the hundreds) and
 * contracted on the 16 x 16 x 4 MFMA of the dtype, once for up to 64 draws.  The order of the sum over the 2L + M rows is
 * fixed and the value of a column does not depend on the other columns of the call: two calls, or x evaluated in pieces,
 * return the same bits.  Validated before any launch. */
int hb_sgp_pathwise_f32(int kind, const float* x, const float* omega, const float* z, const float* ell, long dl,
                        const float* coef, double scale, float* out, long n, long L, long M, long d, long S, void* stream);
int hb_sgp_pathwise_f64(int kind, const double* x, const double* omega, const double* z, const double* ell, long dl,
                        const double* coef, double scale, double* out, long n, long L, long M, long d, long S, void* stream);
/* Maximising pathwise function draws (csrc/sgp_pathwise_grad.hip; not in the reference).  Arguments, limits and validation
 * are those of hb_sgp_pathwise_* unless stated; both share its synthesis, coef staging and K order (csrc/sgp_pathwise.cuh).
 *
 * hb_sgp_pathwise_grad: values and input gradients in ONE launch,
 *   grad[s, j, k] = d out[s, j] / d x_jk
 *                 = scale ( sum_{l<L} (omega_lk / ell_k) [ -coef[s, 2l] sin(p_lj) + coef[s, 2l+1] cos(p_lj) ]
 *                           + sum_{m<M} coef[s, 2L+m] K(z_m, x_j) (z_mk - x_jk) / ell_k^2 ),
 * grad [S, n, d] row-major, non-NULL; out [S, n] or NULL (the values are then not stored).  The derivative operands are
 * formed in registers from the value tile (trig rows swapped and scaled by the signed omega_lk / ell_k, RBF rows scaled by
 * (z_mk - x_jk) / ell_k^2): no transcendental beyond those of the value.  32 draws per workgroup (16 for double at d >= 3);
 * d <= 4 in one workgroup, larger d in groups of 4 dimensions on the grid's z.  n = 0 returns without a launch; additionally S n d must be below
 * 2^31.  `out` is bit-identical to hb_sgp_pathwise on the same inputs; every out[s, j] and grad[s, j, :] is independent of
 * the other columns and of the other draws: two calls, x in pieces, or a subset of the draws return the same bits.
 *
 * hb_sgp_pathwise_argmax: best[s] = max_j out[s, j] (largest != 0) or min_j (largest == 0) and idx[s] its first column,
 * out[s, j] being exactly the number hb_sgp_pathwise stores -- and [S, n] is never written.  Each workgroup reduces its
 * strip of 128 columns per draw (registers, lanes, the four waves through LDS) into ws; a second launch, a workgroup per
 * draw, folds the strips.  No atomics; comparisons are strict and ties go to the lowest column, so a NaN is never chosen:
 * a draw with no comparable value reports idx = -1 and best = -inf (largest) or +inf.  best [S], idx [S] (long), non-NULL;
 * n = 0 is rejected (bad extents); ws >= hb_sgp_pathwise_argmax_ws_elems(n, S) = 2 S ceil(n / 128) elements of T, NULL
 * rejected.  Two calls return the same bits.  Both entries are validated before any launch. */
int hb_sgp_pathwise_grad_f32(int kind, const float* x, const float* omega, const float* z, const float* ell, long dl,
                             const float* coef, double scale, float* out, float* grad, long n, long L, long M, long d, long S,
                             void* stream);
int hb_sgp_pathwise_grad_f64(int kind, const double* x, const double* omega, const double* z, const double* ell, long dl,
                             const double* coef, double scale, double* out, double* grad, long n, long L, long M, long d, long S,
                             void* stream);
long hb_sgp_pathwise_argmax_ws_elems(long n, long S);
int hb_sgp_pathwise_argmax_f32(int kind, const float* x, const float* omega, const float* z, const float* ell, long dl,
                               const float* coef, double scale, int largest, float* best, long* idx, long n, long L, long M,
                               long d, long S, float* ws, void* stream);
int hb_sgp_pathwise_argmax_f64(int kind, const double* x, const double* omega, const double* z, const double* ell, long dl,
                               const double* coef, double scale, int largest, double* best, long* idx, long n, long L, long M,
                               long d, long S, double* ws, void* stream);
/* Batch acquisition from pathwise function draws (csrc/sgp_pathwise_acq.hip; not in the reference; Wilson et al. 2020,
 * section 5): the Monte-Carlo acquisition of S coherent function draws over PER-DRAW incumbents, reduced over the draws
 * inside the pathwise kernel -- [S, n] is never written.  Arguments, limits and validation are those of
 * hb_sgp_pathwise_argmax_* (n >= 1, kind must be HB_KERN_RBF).  With v_sj the number hb_sgp_pathwise stores for draw s and
 * column j (those bits), sigma = +1 (largest != 0) or -1, t_sj = sigma ((double) v_sj - (double) incumbent[s]):
 *   HB_PWACQ_EI   u_sj = max(t_sj, 0)         (expected improvement: greedy q-EI with incumbent[s] <- max(., f_s(x*)))
 *   HB_PWACQ_PI   u_sj = t_sj > 0 ? 1 : 0     (probability of improvement)
 *   value[j] = (T) ( (sum_s u_sj) / S ),
 * the sum over all S draws in double in an order fixed by S alone (a lane's registers, the four lane groups of a wave, the
 * row tiles, then the tiles of 64 draws in tile order); a NaN v_sj makes value[j] NaN.  idx [1] (long) = the first j with
 * the largest value[j] among the comparable ones and best [1] = value[idx]: comparisons strict, ties to the lowest
 * column, a NaN never chosen, no comparable value: idx = -1 and best = -inf.  incumbent [S] non-NULL; value [n] nullable;
 * best and idx are given together or not at all; at least one of value / (best, idx) must be given.  acq must be one
 * of the two ids.  value[j] depends neither on the other columns nor on n: two calls, or x in pieces, return the same
 * bits.  No atomics.  One launch of the pathwise kernel with the reducing epilogue, for S > 64 a second that adds the
 * tiles of draws, and one workgroup that folds the strips' arg-max pairs.  ws >= hb_sgp_pathwise_acq_ws_elems(n, S)
 * DOUBLES (whatever the dtype), NULL rejected: 2 ceil(n / 128) for S <= 64 -- with value == NULL nothing of size n is
 * written anywhere -- and ceil(S / 64) n more for S > 64.  Validated before any launch. */
enum { HB_PWACQ_EI = 0, HB_PWACQ_PI = 1 };
long hb_sgp_pathwise_acq_ws_elems(long n, long S);
int hb_sgp_pathwise_acq_f32(int kind, const float* x, const float* omega, const float* z, const float* ell, long dl,
                            const float* coef, double scale, int acq, int largest, const float* incumbent, float* value,
                            float* best, long* idx, long n, long L, long M, long d, long S, double* ws, void* stream);
int hb_sgp_pathwise_acq_f64(int kind, const double* x, const double* omega, const double* z, const double* ell, long dl,
                            const double* coef, double scale, int acq, int largest, const double* incumbent, double* value,
                            double* best, long* idx, long n, long L, long M, long d, long S, double* ws, void* stream);
/* Input gradients of hb_sgp_predict's moments and closed-form acquisition functions (csrc/sgp_predict_grad.hip; not in
 * the reference).  One expert, one latent function (E = P = 1 of hb_sgp_predict_*), kind must be HB_KERN_RBF; x [n, d],
 * z [M, d], ell [dl], W, Wfrag, m [M], s ([M] standard deviations or [M, M] lower), s_kind, mode, jitter as there.  With
 * K_kj = k(z_k, x_j), t_kjd = (z_kd - x_jd) / ell_d^2, A = W K, C = S^T A:
 *   dmean[j, d] = sum_k alpha_k K_kj t_kjd,     alpha = W^T m^T
 *   dvar [j, d] = 2 sum_k G_kj K_kj t_kjd,      G = W^T (S C - A diag rho),
 *   rho_j = sign(1 - sum_m A_mj^2) (HB_SGP_DIAGONAL), 0 (HB_SGP_NEGLECTED), 1 (HB_SGP_FULLRANK)
 * -- formed from A itself, like the variance, never as a quadratic form in Kmm^-1.
 *
 * hb_sgp_predict_grad: mean [n], var [n] (each nullable: then not stored), dmean [n, d], dvar [n, d] row-major, non-NULL.
 * mean and var are bit-identical to hb_sgp_predict's (the same code).  n = 0 returns without a launch.
 *
 * hb_sgp_acq: the acquisition `acq` of the scaled model f = scale * (..) at every row of x, its tail evaluated per point in
 * double whatever the storage type.  With k_var = scale^2, s = +1 (largest != 0) or -1, mu' = s scale mean,
 * v = max(k_var var, var_floor), sigma = sqrt(v), u = (mu' - s best - param) / sigma, Phi(u) = erfc(-u / sqrt 2) / 2:
 *   HB_ACQ_EI   sigma (u Phi + phi)    (param = xi)
 *   HB_ACQ_PI   Phi                    (param = xi)
 *   HB_ACQ_UCB  mu' + param sigma      (param = beta; best unused)
 * val [n], grad [n, d] = d val / d x (zero through v where it was clamped), best_val [1] = max_j val[j] -- those bits --
 * and best_idx [1] (long) its first row: every output is nullable, at least one must be given; when only best_val /
 * best_idx are asked for nothing of size n is written.  The arg-max follows hb_sgp_pathwise_argmax: workgroup partials
 * in ws, a second launch folds them, comparisons strict, ties to the lowest row, a NaN never chosen, no comparable value:
 * idx = -1 and best_val = -inf; n = 0 is rejected for an arg-max and returns without a launch otherwise.
 *
 * Fused form under the conditions of hb_sgp_predict's fused form: fp32, Wfrag, M % 32 == 0, 32 <= M <= 512, d <= 4.  One
 * workgroup per 32-column strip, A, C, V = S C - A diag rho and G on MFMA in LDS, no [M, n] intermediate in memory.
 * V, G and the fold are formed only when a gradient output (dmean / dvar, grad) is given: values or the arg-max alone cost
 * what hb_sgp_predict costs and carry the same bits.  Everything else runs in column chunks over hb_sgp_A_* and hb_matmul_*.  No atomics: two calls return the same bits, and
 * a column's results do not depend on the other columns of the call.  ws >= hb_sgp_predict_grad_ws_elems /
 * hb_sgp_acq_ws_elems(n, M, d, s_kind, Wfrag != NULL, sizeof(T)) elements (16-byte aligned, bounded by one chunk of
 * columns, not by n).  Validated before any launch. */
enum { HB_ACQ_EI = 0, HB_ACQ_PI = 1, HB_ACQ_UCB = 2 };
long hb_sgp_predict_grad_ws_elems(long n, long M, long d, int s_kind, int has_wfrag, int dtype_bytes);
int hb_sgp_predict_grad_f32(int kind, const float* x, const float* z, const float* ell, long dl, const float* W,
                            const float* Wfrag, const float* m, const float* s, int s_kind, int mode, double jitter,
                            float* mean, float* var, float* dmean, float* dvar, long n, long M, long d, float* ws,
                            void* stream);
int hb_sgp_predict_grad_f64(int kind, const double* x, const double* z, const double* ell, long dl, const double* W,
                            const double* Wfrag, const double* m, const double* s, int s_kind, int mode, double jitter,
                            double* mean, double* var, double* dmean, double* dvar, long n, long M, long d, double* ws,
                            void* stream);
long hb_sgp_acq_ws_elems(long n, long M, long d, int s_kind, int has_wfrag, int dtype_bytes);
int hb_sgp_acq_f32(int kind, const float* x, const float* z, const float* ell, long dl, const float* W, const float* Wfrag,
                   const float* m, const float* s, int s_kind, int mode, double jitter, int acq, double best, double param,
                   double scale, int largest, double var_floor, float* val, float* grad, float* best_val, long* best_idx,
                   long n, long M, long d, float* ws, void* stream);
int hb_sgp_acq_f64(int kind, const double* x, const double* z, const double* ell, long dl, const double* W,
                   const double* Wfrag, const double* m, const double* s, int s_kind, int mode, double jitter, int acq,
                   double best, double param, double scale, int largest, double var_floor, double* val, double* grad,
                   double* best_val, long* best_idx, long n, long M, long d, double* ws, void* stream);
/* Matrix-free kernel product (csrc/gram_matvec.hip; not in the reference; Gardner et al. 2018, Wang et al. 2019):
 *   out[s, j] = scale * sum_{i<N} V[s, i] k(x2_i, x_j) + shift * V[s, j],     s < S, j < n,
 * the product a conjugate-gradient solve with K(X, X) + sigma^2 I asks for, and the exact posterior mean at new points.
 * x [n, d], x2 [N, d], V [S, N], out [S, n], row-major and contiguous; ell [dl], dl in {1, d}; kind must be HB_KERN_RBF.
 * x2 == NULL is the symmetric form x2 = x (N must equal n); only then may shift be non-zero.  S >= 1, d >= 1; n = 0 or
 * N = 0 returns without a kernel launch (N = 0: out is zero-filled).  k is the difference-then-scale exp2 form of the strip
 * kernels (csrc/sgp_strip.cuh) and is never written to memory.  The rows i are cut into chunks of hb_gram_matvec_chunk()
 * (a compile-time constant: it depends on nothing); the grid is column strips x row chunks x tiles of 64 right-hand
 * sides, each workgroup contracts its block on the 16 x 16 x 4 MFMA of the dtype, and with more than one chunk a second
 * launch adds the chunks' partials in chunk order IN DOUBLE (both dtypes), applies scale and shift and writes out; one
 * chunk: the same finish in the first launch's epilogue, the workspace untouched.  No atomics.  The order of every sum is
 * fixed by N alone: an output element depends neither on the other columns nor on S nor on n -- two calls, x evaluated in
 * pieces, or a subset of the right-hand sides return the same bits.  n, N up to 2^31 - 1 (strips of 128 x chunks below
 * 2^31); S N and S n are indexed in long.  More than 16 chunks are launched 16 at a time, the fold carrying its running
 * double sum between the groups (the same additions in the same order), so the workspace is O(S n) whatever N:
 * ws >= hb_gram_matvec_ws_elems(n, N, S, sizeof(T)) elements of T, 16-byte aligned -- 0 for one chunk (NULL allowed),
 * chunks x S x n up to 16 chunks, beyond that 16 S n plus S n doubles.  Validated before any launch. */
long hb_gram_matvec_chunk(void);
long hb_gram_matvec_ws_elems(long n, long N, long S, int dtype_bytes);
int hb_gram_matvec_f32(int kind, const float* x, const float* x2, const float* ell, long dl, const float* V, double scale,
                       double shift, float* out, long n, long N, long d, long S, float* ws, void* stream);
int hb_gram_matvec_f64(int kind, const double* x, const double* x2, const double* ell, long dl, const double* V, double scale,
                       double shift, double* out, long n, long N, long d, long S, double* ws, void* stream);
/* Predictive mean, cached predictive variance and closed-form acquisition of an exact GP from ONE kernel product
 * (csrc/gram_matvec.hip; not in the reference).  V [S, N] holds P mean rows first (1 <= P <= S), then S - P cache rows.
 * With t[s, j] the DOUBLE that hb_gram_matvec holds for the same x, x2, V and scale (no shift) before its final rounding -- the chunks' partials
 * added in chunk order, or the one chunk's accumulator, times scale:
 *   mean[p, j] = (T) t[p, j], p < P              -- the bits of hb_gram_matvec on those rows;
 *   q_j = sum_{s >= P} t[s, j]^2                  -- in double, s ascending, each square and each sum rounded once;
 *   var[j] = (T) max(prior - q_j, 0);
 *   val[j] = (T) the tail of hb_sgp_acq -- HB_ACQ_EI / _PI / _UCB with best, param, largest, var_floor as there, scale = 1 --
 *            evaluated in double at (t[0, j], prior - q_j); needs P == 1.  acq = -1: no acquisition (val, best_val and
 *            best_idx must then be NULL).
 * With V = [alpha; R_c], scale = prior = k_var, R_c = L_T^-1 C and T = C K^ C^T = L_T L_T^T for any full-row-rank C [r, N],
 * var is k_var - k*^T C^T (C K^ C^T)^-1 C k* >= k_var - k*^T K^^-1 k*: an UPPER bound of the exact predictive variance
 * (the Galerkin restriction of K^^-1 to span(C^T); henbun_amd/gp/exact.py: VarianceCache).
 * Outputs, each nullable, at least one given: mean [P, n], var [n], val [n] in the storage type, best_val [1] DOUBLE =
 * max_j val[j] (those bits, widened) and best_idx [1] (long) its first column, by the rule of hb_sgp_acq: comparisons
 * strict, ties to the lowest column, a NaN never chosen, no comparable value: -1 and -inf.  With only best_val / best_idx
 * asked for nothing of size n is written except the workspace.  n = 0 returns without a launch (rejected for an arg-max).
 * Phase 1 is the kernel of hb_gram_matvec, every chunk's partial left in the workspace (a single chunk's too); phase 2,
 * one thread per column, adds the chunks in chunk order in double (16 chunks at a time, the running sum carried between
 * the groups) and finishes the column; a one-workgroup launch folds the per-workgroup arg-max partials.  No atomics: two
 * calls return the same bits, and a column's outputs depend neither on n nor on the other columns nor on how x is cut
 * into pieces.  x [n, d], x2 [N, d] (non-NULL, N >= 1), ell [dl], dl in {1, d}; kind must be HB_KERN_RBF.
 * ws >= hb_gram_predict_ws_elems(n, N, S, sizeof(T)) elements of T, 16-byte aligned: min(chunks, 16) S n partials, S n
 * doubles beyond 16 chunks, a double and a long per 256 columns.  Validated before any launch. */
long hb_gram_predict_ws_elems(long n, long N, long S, int dtype_bytes);
int hb_gram_predict_f32(int kind, const float* x, const float* x2, const float* ell, long dl, const float* V, long P,
                        double scale, double prior, int acq, double best, double param, int largest, double var_floor,
                        float* mean, float* var, float* val, double* best_val, long* best_idx, long n, long N, long d, long S,
                        float* ws, void* stream);
int hb_gram_predict_f64(int kind, const double* x, const double* x2, const double* ell, long dl, const double* V, long P,
                        double scale, double prior, int acq, double best, double param, int largest, double var_floor,
                        double* mean, double* var, double* val, double* best_val, long* best_idx, long n, long N, long d,
                        long S, double* ws, void* stream);
/* Input gradients of hb_gram_predict's outputs from ONE kernel product (csrc/gram_predict_grad.hip; not in the reference).
 * Arguments as for hb_gram_predict, without the arg-max.  With t[s, j] as there and
 *   u[s, j, k] = d t[s, j] / d x_jk = scale * sum_{i<N} V[s, i] k(x2_i, x_j) (x2_ik - x_jk) / ell_k^2
 * held in DOUBLE the same way (the chunks' partials added in chunk order, times scale):
 *   dmean[p, j, k] = (T) u[p, j, k], p < P;
 *   dvar[j, k]     = (T) (-2 sum_{s >= P} t[s, j] u[s, j, k])   -- in double, s ascending, each product and each sum rounded
 *                    once; exactly 0 where prior - q_j < 0 (var was clamped to 0) and without cache rows (S == P);
 *   dval[j, k]     = (T) (sgn a_mu u[0, j, k] + a_v (-2 sum ..)) -- sgn = +1 (largest) / -1, a_mu and a_v the derivatives of
 *                    the tail of hb_sgp_acq at (t[0, j], prior - q_j); a_v is 0 where var_floor clamps.  Needs P == 1.
 * Outputs, each nullable, at least one given: mean [P, n], var [n], val [n] -- the BITS of hb_gram_predict -- and
 * dmean [P, n, d], dvar [n, d], dval [n, d]; val and dval need an acquisition (acq != -1).
 * Phase 1 is the loop of hb_gram_matvec's kernel with 1 + min(d, 4) accumulator sets: the operand of dimension k is the
 * value tile times (x2_rk - x_ck) (1 / ell_k^2), formed in registers as the MFMA loop reads the tile (no second exp2);
 * 32 right-hand sides per workgroup (16 for double at d >= 3), d > 4 in groups of 4 dimensions on the grid's z.  Every
 * workgroup leaves its value partial and its derivative partials in the workspace; phase 2, one thread per column and
 * dimension (each folds the value rows itself; the thread of dimension 0 also writes mean, var and val), adds the chunks
 * in chunk order in double (16 chunks at a time, running sums [1 + d, S, n] carried between the groups) and finishes the
 * column's outputs of that dimension.  No atomics: two calls return the same bits, and a column's outputs depend neither on n nor on
 * the other columns nor on how x is cut into pieces.  n = 0 returns without a launch.
 * ws >= hb_gram_predict_grad_ws_elems(n, N, d, S, sizeof(T)) elements of T, 16-byte aligned: 1 + d times the partials
 * (min(chunks, 16) S n, rounded up to 8 bytes) and, beyond 16 chunks, 1 + d times S n doubles.  Validated before any launch. */
long hb_gram_predict_grad_ws_elems(long n, long N, long d, long S, int dtype_bytes);
int hb_gram_predict_grad_f32(int kind, const float* x, const float* x2, const float* ell, long dl, const float* V, long P,
                             double scale, double prior, int acq, double best, double param, int largest, double var_floor,
                             float* mean, float* var, float* val, float* dmean, float* dvar, float* dval, long n, long N,
                             long d, long S, float* ws, void* stream);
int hb_gram_predict_grad_f64(int kind, const double* x, const double* x2, const double* ell, long dl, const double* V, long P,
                             double scale, double prior, int acq, double best, double param, int largest, double var_floor,
                             double* mean, double* var, double* val, double* dmean, double* dvar, double* dval, long n, long N,
                             long d, long S, double* ws, void* stream);
/* Vector steps of S preconditioned conjugate-gradient iterations run in lockstep on rows of length N (csrc/gram_matvec.hip;
 * henbun_amd/gp/exact.py).  x, r, p, Ap, w [S, N] in the storage type; rz, rr, thr, out [S] DOUBLE: every dot product and
 * scalar is double.  One workgroup per row, sums in a fixed order: two solves return the same bits.  A row with
 * rr[s] <= thr[s] has converged and is left untouched by update and direction (its alpha is 0).
 *   hb_pcg_dot:        out[s] = sum_i a_si b_si;
 *   hb_pcg_update:     alpha_s = rz_s / (p_s . Ap_s) (0 when the curvature is not positive);  x_s += alpha_s p_s;
 *                      r_s -= alpha_s Ap_s;  rr_s = |r_s|^2;
 *   hb_pcg_direction:  z_s = (r_s - wscale w_s) zscale (w == NULL: z_s = r_s);  beta_s = (r_s . z_s) / rz_s (first != 0:
 *                      0, p is not read);  p_s = z_s + beta_s p_s;  rz_s = r_s . z_s. */
int hb_pcg_dot_f32(const float* a, const float* b, double* out, long S, long N, void* stream);
int hb_pcg_dot_f64(const double* a, const double* b, double* out, long S, long N, void* stream);
int hb_pcg_update_f32(float* x, float* r, const float* p, const float* Ap, const double* rz, double* rr, const double* thr,
                      long S, long N, void* stream);
int hb_pcg_update_f64(double* x, double* r, const double* p, const double* Ap, const double* rz, double* rr, const double* thr,
                      long S, long N, void* stream);
int hb_pcg_direction_f32(const float* r, const float* w, float* p, double* rz, const double* rr, const double* thr,
                         double wscale, double zscale, int first, long S, long N, void* stream);
int hb_pcg_direction_f64(const double* r, const double* w, double* p, double* rz, const double* rr, const double* thr,
                         double wscale, double zscale, int first, long S, long N, void* stream);
/* hb_pcg_update / hb_pcg_direction with the recurrence coefficients logged: coef [2 iterations, S] DOUBLE or NULL.  With
 * coef != NULL the update of iteration `it` stores alpha_s at coef[(2 it) S + s] and the direction after it beta_s at
 * coef[(2 it + 1) S + s]; a converged row (skipped) stores nothing, so a log the host pre-filled with NaN marks where a
 * row's recurrence ended.  From these the host builds the Lanczos tridiagonal of the preconditioned matrix (stochastic
 * Lanczos quadrature of log det, henbun_amd/gp/exact.py).  x, r, p, rz, rr are the bits of the entries above; coef ==
 * NULL is exactly those entries. */
int hb_pcg_update_coef_f32(float* x, float* r, const float* p, const float* Ap, const double* rz, double* rr,
                           const double* thr, long S, long N, double* coef, long it, void* stream);
int hb_pcg_update_coef_f64(double* x, double* r, const double* p, const double* Ap, const double* rz, double* rr,
                           const double* thr, long S, long N, double* coef, long it, void* stream);
int hb_pcg_direction_coef_f32(const float* r, const float* w, float* p, double* rz, const double* rr, const double* thr,
                              double wscale, double zscale, int first, long S, long N, double* coef, long it, void* stream);
int hb_pcg_direction_coef_f64(const double* r, const double* w, double* p, double* rz, const double* rr, const double* thr,
                              double wscale, double zscale, int first, long S, long N, double* coef, long it, void* stream);
/* Bilinear contraction of K = K(x, x) and of its lengthscale derivative against S weighted pairs of vectors
 * (csrc/gram_grad.hip; not in the reference): the traces of the gradient of the exact GP's log marginal likelihood.
 *   g[0]     = sum_s w_s sum_ij A_si B_sj K_ij
 *   g[1 + k] = sum_s w_s sum_ij A_si B_sj K_ij (x_ik - x_jk)^2 / ell_k^3,   k < dl  (dl = 1: summed over k, ell_0^3)
 * x [N, d], A, B [S, N] row-major and contiguous in the storage type; ell [dl], dl in {1, d}; w [S] and g [1 + dl] DOUBLE;
 * kind must be HB_KERN_RBF.  Neither K nor W = sum_s w_s A_s (x) B_s is written to memory: workgroups of column strips x
 * row chunks (the decomposition of hb_gram_matvec) form 32 x 32 tiles of W on the 16 x 16 x 4 MFMA with the pair index
 * contracted, evaluate K and the squared differences at the accumulator positions and add into per-lane DOUBLE sums.  No
 * atomics: one partial per workgroup, folded in a fixed order in double by a second launch; more than 16 chunks or 64
 * pairs are taken 16 / 64 at a time with the fold carrying its sum in g.  Two calls return the same bits.  ARD
 * lengthscales with d > 4 run four dimensions per grid z-slice.  ws >= hb_gram_bilinear_grad_ws_elems(N, dl) DOUBLES =
 * min(chunks, 16) x strips x (1 + dl), whatever S.  N = 0: g is zero-filled, no kernel of the contraction runs.
 * Validated before any launch. */
long hb_gram_bilinear_grad_ws_elems(long N, long dl);
int hb_gram_bilinear_grad_f32(int kind, const float* x, const float* ell, long dl, const float* A, const float* B,
                              const double* w, double* g, long N, long d, long S, double* ws, void* stream);
int hb_gram_bilinear_grad_f64(int kind, const double* x, const double* ell, long dl, const double* A, const double* B,
                              const double* w, double* g, long N, long d, long S, double* ws, void* stream);
/* Greedy conditional-variance selection of M inducing points out of X [N, d] (csrc/sgp_select.hip; not in the reference;
 * Burt, Rasmussen, van der Wilk 2020): a pivoted incomplete Cholesky of K(X, X).  With dvar [N] = kdiag = 1 and the
 * history C [M, N], for j = 0 .. M - 1:
 *   i_j = argmax_i dvar_i, exact ties to the LOWEST index (i_0 = 0);  if dvar_{i_j} <= threshold: stop, count = j;
 *   pivots[j] = dvar_{i_j};  idx[j] = i_j;
 *   C[j, i] = (k(x_i, x_{i_j}) - sum_{t < j} C[t, i] C[t, i_j]) / sqrt(pivots[j])     (the sum in t order);
 *   dvar_i <- max(dvar_i - C[j, i]^2, 0);  dvar_{i_j} <- 0.
 * Outputs, all DEVICE memory: idx [M] and pivots [M] (entries from count on: -1 and 0), count [1] (M when the threshold
 * never stopped it), trace [1] = sum_i dvar_i at the end = tr(K_XX - K_XZ K_ZZ^-1 K_ZX), summed in double in a fixed order.
 * k is the library's one definition of the kernel value (csrc/gram_value.cuh); kind must be HB_KERN_RBF; ell [dl],
 * dl in {1, d}; 1 <= M <= N, M <= 8192, d >= 1, threshold >= 0.  The _f32 entry keeps C and dvar in float, the _f64 entry
 * runs the same code in double.  M + 1 launches, one per chosen point plus a fold, no host synchronisation, no atomics:
 * two calls on the same inputs return the same bits.  ws >= hb_sgp_select_ws_elems(N, M, d, sizeof(T)) elements of T,
 * 16-byte aligned: the history, dvar and the arg-max partials -- O(M N): (M + 1) x (N rounded up to 64) + 12288 (float) /
 * 8192 (double).  Row j streams j rows of the history: N M^2 / 2 elements read in all.
 * WORKSPACE LAYOUT (part of the contract: the preconditioner of henbun_amd/gp/exact.py reads it): the history C starts at
 * ws[0], row j at ws + j ld with ld = N rounded up to 64 and zeros in the pad columns; after the call rows 0 .. count - 1
 * hold the pivoted incomplete Cholesky factor, C^T C ~ K(X, X). */
long hb_sgp_select_ws_elems(long N, long M, long d, int dtype_bytes);
int hb_sgp_select_f32(int kind, const float* X, const float* ell, long dl, long N, long M, long d, double threshold, long* idx,
                      float* pivots, long* count, double* trace, float* ws, void* stream);
int hb_sgp_select_f64(int kind, const double* X, const double* ell, long dl, long N, long M, long d, double threshold,
                      long* idx, double* pivots, long* count, double* trace, double* ws, void* stream);
/* Streamed part of the gradient of the collapsed bound (csrc/sgp_cbgrad.hip; not in the reference).  With K = k(z, X)
 * [M, N] and the weights Q [M, M], R [M, P] of the M^3 tail (SparseGP.collapsed_bound_and_grad):
 *   Kbar = Q K + R Y^T,  E = Kbar o K,
 *   zbar[i, k] = -sum_j E_ij (z_ik - x_jk) / ell_k^2,   ellbar[k] = sum_ij E_ij (z_ik - x_jk)^2 / ell_k^3
 * (dl == 1: ellbar [1], summed over k).  Kbar is never written.  The suffix is the STORAGE type of X [N, d] and Y [N, P]
 * only: z, ell, Q, R, zbar [M, d], ellbar [dl], the workspace and all arithmetic are double (the z gradient of the bound
 * is a difference of two terms about 1000 times its size).  kind must be HB_KERN_RBF; N, M, d, P >= 1,
 * d <= 256, P <= 256, M + d + P <= 8000.  M % 16 == 0, M <= 512, d <= 4, P <= 4: column strips of 32 on
 * v_mfma_f64_16x16x4_f64 with K synthesised in LDS, at most 256 strips; every other shape: plain double loops.  A second
 * launch folds the strips' partials in strip order (no atomics, no flags): two calls on the same inputs return the same
 * bits.  Outputs are overwritten.  ws >= hb_sgp_kgrad_ws_elems(N, M, d, P) doubles, 16-byte aligned; independent of N. */
long hb_sgp_kgrad_ws_elems(long N, long M, long d, long P);
int hb_sgp_kgrad_f32(int kind, const float* X, const float* Y, const double* z, const double* ell, long dl, const double* Q,
                     const double* R, double* zbar, double* ellbar, long N, long M, long d, long P, double* ws, void* stream);
int hb_sgp_kgrad_f64(int kind, const double* X, const double* Y, const double* z, const double* ell, long dl, const double* Q,
                     const double* R, double* zbar, double* ellbar, long N, long M, long d, long P, double* ws, void* stream);
/* Column-weighted form of hb_sgp_kgrad_* (same file; not in the reference), the streamed part of the gradient of the ELBO
 * of a factorising likelihood at a fixed q(u) (SparseGP.elbo_and_grad): one latent function (P = 1) and
 *   Kbar_ij = w_j (Q K)_ij + R_i r_j,  E = Kbar o K,  zbar and ellbar as above
 * with per-point weights w [N], r [N] in DOUBLE whatever the storage type of X (any sign, zeros included; in the model
 * w_j = E[-d2 log p_j], r_j = E[d log p_j]), R [M, 1].  The same kernels with one template flag: w is staged next to r
 * and multiplies the accumulator of Q K before + R r, so w == 1, r = Y[:, 0] returns the bits of hb_sgp_kgrad_* at P = 1.
 * Same shapes for the two forms, the same diagnostic switch, the same fold launch, two calls return the same bits;
 * ws >= hb_sgp_kgrad_ws_elems(N, M, d, 1) doubles. */
int hb_sgp_wkgrad_f32(int kind, const float* X, const double* w, const double* r, const double* z, const double* ell, long dl,
                      const double* Q, const double* R, double* zbar, double* ellbar, long N, long M, long d, double* ws,
                      void* stream);
int hb_sgp_wkgrad_f64(int kind, const double* X, const double* w, const double* r, const double* z, const double* ell, long dl,
                      const double* Q, const double* R, double* zbar, double* ellbar, long N, long M, long d, double* ws,
                      void* stream);
/* hb_sgp_kgrad_* / hb_sgp_wkgrad_* with the INPUT gradient as a third output (same file, the template flag XG of the same
 * kernels; not in the reference): the products E_ij (z_ik - x_jk) whose row sums are zbar have as their column sums
 *   xbar[j, k] = +sum_i E_ij (z_ik - x_jk) / ell_k^2          [N, d], double, row-major, overwritten
 * -- the complete derivative of the collapsed bound (of the ELBO at a fixed q(u) for the weighted form, where E already
 * carries w_j and r_j) with respect to X at fixed weights Q, R, because k(x, x) == 1 and every dependence on X goes
 * through K(z, X).  The arguments are those of the entry without _x with xbar after ellbar; the same checks, shapes,
 * forms, diagnostic switch and workspace (hb_sgp_kgrad_ws_elems: xbar needs none).  zbar and ellbar are the bits of the
 * entry without _x.  Strip form: per step of 32 columns the lanes' sums over their rows are folded over the four lane
 * groups by two shuffles and over the 8 waves through LDS in wave order, and every column is written by the one
 * workgroup that owns its step -- no atomics, no fold launch; the order depends on M alone, so two calls return the same
 * bits and the bits of a column do not depend on N or on the other columns.  LDS: 8 x 32 x d doubles more, 158 208 B of
 * the CU's 160 KB at M = 512, d = 4, weighted.  Plain form: per column and dimension a sum per thread over its strided
 * rows, per wave by shuffles, over the 4 waves in wave order.  sum_j xbar_j = -zbar_streamed summed over i (translation
 * invariance). */
int hb_sgp_kgrad_x_f32(int kind, const float* X, const float* Y, const double* z, const double* ell, long dl, const double* Q,
                       const double* R, double* zbar, double* ellbar, double* xbar, long N, long M, long d, long P, double* ws,
                       void* stream);
int hb_sgp_kgrad_x_f64(int kind, const double* X, const double* Y, const double* z, const double* ell, long dl, const double* Q,
                       const double* R, double* zbar, double* ellbar, double* xbar, long N, long M, long d, long P, double* ws,
                       void* stream);
int hb_sgp_wkgrad_x_f32(int kind, const float* X, const double* w, const double* r, const double* z, const double* ell, long dl,
                        const double* Q, const double* R, double* zbar, double* ellbar, double* xbar, long N, long M, long d,
                        double* ws, void* stream);
int hb_sgp_wkgrad_x_f64(int kind, const double* X, const double* w, const double* r, const double* z, const double* ell, long dl,
                        const double* Q, const double* R, double* zbar, double* ellbar, double* xbar, long N, long M, long d,
                        double* ws, void* stream);
/* VJP given fbar [E,P,n]:
 *   Abar = u^T fbar + A diag(c),  c = -eps sign(v)/sqrt|v| * sum_p fbar_p
 *   Kbar = W^T Abar            [E,M,n]  (scratch output, kept for Lbar)
 *   Lbar = -tril(Kbar A^T)     [E,M,M]
 *   ubar = fbar A^T            [E,P,M]
 * Wfrag (nullable) / prec: as for hb_sgp_fwd; with Wfrag (fp32, M %% 32 == 0, M <= 512, d <= 4, P <= 4, no xbar) Kbar
 * and the row gradients come from ONE column-strip kernel (no second pass over Kbar and A).
 * A_frag / Kbar_frag (both or neither; need hb_sgp_strip_path): A is read, and Kbar written, in the fragment-major
 * layout of hb_sgp_fwd's A_frag (A / Kbar may then be NULL), and Lbar comes from a contraction whose every operand
 * load is one contiguous kilobyte (E*M*32*ceil(n/32) elements each).
 *   zbar, ellbar (and xbar, nullable) through Kmn = k(z,x). */
int hb_sgp_bwd_f32(int kind, int mode, const float* x, long sx, const float* z, const float* ell,
                   long dl, const float* W, const float* Wfrag, int prec, const float* u, const float* eps,
                   const float* A, const float* A_frag, const float* v, const float* fbar, float* Kbar,
                   float* Kbar_frag, float* Lbar, float* ubar, float* zbar, float* ellbar, float* xbar,
                   long E, long n, long M, long d, long P, float* ws, void* stream);
/* hb_sgp_bwd_f32 for a caller whose only use of Lbar is the Cholesky VJP's first product Phisym(L^T tril(Lbar))
 * (Phisym(Q)_ij = Q_{max(i,j),min(i,j)} / 2, hb_matutil mode 4): with W = L^-1 that product equals Phisym(-Abar A^T),
 * Abar = u^T fbar + A diag(c), so W^T never multiplies the M x M result and L^T never multiplies it back.
 *   Phi [E,M,M] (both triangles written) replaces Lbar; Abar_frag (E*M*32*ceil(n/32) elements, the layout of A_frag)
 *   is scratch: the strip kernel leaves Abar there, where hb_sgp_bwd_f32 leaves Kbar in Kbar_frag.
 * ubar, zbar and ellbar are those of hb_sgp_bwd_f32, bit for bit.  fp32, native precision, fragment-major A only, and
 * only where hb_sgp_bwd_phi_supported(...) == 1: hb_sgp_strip_path for HB_PREC_NATIVE, and the diagnostic switch
 * sgp_phi_direct not set to 0 (the switch is read by _supported alone: ask once, when the call sequence is planned). */
int hb_sgp_bwd_phi_supported(long E, long n, long M, long d, long P);
int hb_sgp_bwd_phi_f32(int kind, int mode, const float* x, long sx, const float* z, const float* ell, long dl,
                       const float* W, const float* Wfrag, const float* u, const float* eps, const float* A_frag,
                       const float* v, const float* fbar, float* Abar_frag, float* Phi, float* ubar, float* zbar,
                       float* ellbar, long E, long n, long M, long d, long P, float* ws, void* stream);
/* Forward and Kbar column strips in ONE launch.  hb_sgp_fwd_gauss_f32 and the strip kernel of hb_sgp_bwd_phi_f32 give one
 * workgroup the same 32 data columns, and with the head in the forward everything the backward strip reads is in that
 * workgroup when the forward's epilogue ends.  Where hb_sgp_fwd_kbar_supported(...) == 1 -- hb_sgp_head_units(...) > 0,
 * hb_sgp_bwd_phi_supported(...) == 1, d <= 2, E * ceil(n / 32) <= 512 strips (beyond that the two launches measured
 * faster), and hb_debug_set("sgp_fwd_kbar", 0) not set (read by _supported alone) --
 *   hb_sgp_fwd_gauss_kbar_f32: the arguments of hb_sgp_fwd_gauss_f32 (fbar and A_frag required, HB_PREC_NATIVE), then
 *     Abar_frag (as hb_sgp_bwd_phi_f32's) and bws, a workspace of hb_sgp_ws_elems(E, n, M, d, P) elements that receives the
 *     backward's strip partials and that nothing else may write until hb_sgp_bwd_phi_rest_f32 has run.  The backward's
 *     fbar IS the head's fbar, its eps and v the forward's.  Never recorded as a rider (hb_sgp_rider_begin).
 *   hb_sgp_bwd_phi_rest_f32: the rest of hb_sgp_bwd_phi_f32 -- the Abar A^T contraction over A_frag / Abar_frag and the
 *     finish launch -- on the same bws: writes Phi, ubar, zbar, ellbar.
 * Every output of the pair has the bits of hb_sgp_fwd_gauss_f32 followed by hb_sgp_bwd_phi_f32. */
int hb_sgp_fwd_kbar_supported(long E, long n, long M, long d, long P, int prec, int has_wfrag, int draw, long rng_lanes);
int hb_sgp_fwd_gauss_kbar_f32(int kind, int mode, const float* x, long sx, const float* z, const float* ell, long dl,
                              const float* W, const float* Wfrag, int prec, const float* u, const float* eps_in,
                              uint64_t* rng, long rng_lanes, float* eps_out, float* A, float* A_frag, float* f, float* v,
                              long E, long n, long M, long d, long P, float* ws, const float* y, const float* scale,
                              const float* var, double post, float* dmu, float* fbar, float* head_part, long units,
                              float* Abar_frag, float* bws, void* stream);
int hb_sgp_bwd_phi_rest_f32(const float* A_frag, const float* Abar_frag, float* Phi, float* ubar, float* zbar,
                            float* ellbar, long dl, long E, long n, long M, long d, long P, float* bws, void* stream);
int hb_sgp_bwd_f64(int kind, int mode, const double* x, long sx, const double* z, const double* ell,
                   long dl, const double* W, const double* Wfrag, int prec, const double* u,
                   const double* eps, const double* A, const double* A_frag, const double* v,
                   const double* fbar, double* Kbar, double* Kbar_frag, double* Lbar, double* ubar,
                   double* zbar, double* ellbar, double* xbar, long E, long n, long M, long d, long P,
                   double* ws, void* stream);

/* ---- K9: flat-buffer Adam, TensorFlow-1 formula (reference model.py:206,220
 *      tf.train.AdamOptimizer via optimizer.minimize) --------
 *   t <- t+1 ; lr_t = lr*sqrt(1-b2^t)/(1-b1^t)
 *   m <- b1 m + (1-b1) g ; v <- b2 v + (1-b2) g^2 ; theta <- theta - lr_t m/(sqrt(v)+eps)
 * g is read as gscale*g (gscale = 1/world_size for data-parallel means).
 * t is a device-side step counter (one int64), incremented by the call when `tick` != 0 (several
 * calls on disjoint segments of one parameter set share a step: only the last one ticks).
 * Failure containment: tf.cholesky raises inside session.run BEFORE apply_gradients (reference
 * model.py:265-266), leaving the parameters at the last good step.  Calls here are asynchronous,
 * so the update reads this step's factorisation status words `info[n_info]` (nullable, LAPACK
 * convention), the other ranks' all-reduced failure flag `dpflag` (nullable, one element) and the
 * sticky record `fail[2]` (nullable): when any is non-zero the call changes nothing (theta, m, v,
 * t) and `fail` keeps {step number t+1, status} of the FIRST blocked step until the host clears it. */
int hb_adam_step_f32(float* theta, const float* g, float* m, float* v, long n, double lr, double b1,
                     double b2, double eps, double gscale, long* t, int tick, const int* info,
                     long n_info, const float* dpflag, long* fail, void* stream);
int hb_adam_step_f64(double* theta, const double* g, double* m, double* v, long n, double lr,
                     double b1, double b2, double eps, double gscale, long* t, int tick,
                     const int* info, long n_info, const double* dpflag, long* fail, void* stream);

/* ---- side jobs: small independent launches riding on another kernel's launch (csrc/side_jobs.cuh) --------------
 * hb_side_push_* take the arguments of their stand-alone twins (hb_gather_rows_multi_draw_f32,
 * hb_diag_sample_kl_fwd_f32, hb_diag_sample_kl_bwd_f32) but RECORD the job in a per-thread list instead of launching
 * it (a job that does not fit the side form -- more than one workgroup for the sampler, fp64 -- is launched at
 * once, as the twin would).  The next host launch issued by the same thread -- launch 0 of hb_cholesky /
 * hb_cholesky_inverse on the 64-column fp32 path, hb_matmul on its in-workgroup split-K path -- appends the recorded
 * jobs' workgroups to its own grid.  hb_side_flush launches whatever is still pending as one kernel of its own, so
 * push ... host ... flush is always equivalent to the stand-alone calls provided nobody reads the jobs' outputs
 * before the host launch has run.  hb_side_pending: number of recorded jobs (at most 3; a fourth push flushes). */
int hb_side_push_gather_draw_f32(int narr, const float* const* srcs, const long* rows, float* const* dsts, long nsrc,
                                 uint64_t* state, long nlanes, long lo, long hi, long* idx_out, const long* perm,
                                 long n, int* err, void* stream);
int hb_side_push_diag_fwd_f32(const float* mu, const float* s, const float* u_in, uint64_t* rng, long rng_lanes,
                              float* u_out, float* x, float* kl, long n, long L, long ld_mu, long ld_s, float* ws,
                              void* stream);
int hb_side_push_diag_bwd_f32(const float* s, const float* u, const float* x, const float* xbar, const float* klbar,
                              float* mubar, float* sbar, long n, long L, long ld_s, long ld_out, void* stream);
int hb_side_pending(void);
int hb_side_flush(void* stream);
/* Drops the calling thread's recorded jobs without running them (returns how many): for a caller whose launch sequence
 * was abandoned between a push and its host launch; the recorded raw pointers must not ride on a later, unrelated
 * launch.  henbun_amd's Plan calls it before and after every execution / capture of a plan. */
int hb_side_discard(void);

/* ---- serial chains: several small DEPENDENT launches run as one generated kernel (csrc/chain.cuh, csrc/jit.hip) ----
 * Between hb_chain_begin() and hb_chain_end(stream) the calling thread records the small launches that the chain-aware
 * entry points would issue (each up to a few thousand elements: a chain is one workgroup, csrc/chain.cuh has the limits) --
 * hb_ewise_jit_run, hb_gauss_ll_*, hb_adam_step_*, the finishing pass of hb_sgp_fwd_*, the lengthscale fold of hb_gram_bwd_* --
 * and runs them, in
 * call order, as ONE hiprtc-compiled kernel: one workgroup of 1024 threads, a barrier between jobs.  A launch that cannot
 * be recorded first runs what is recorded, so the order of the calls is the order of execution; ONLY the entry points
 * named above may be called between begin and end.  A kernel boundary inside a captured step costs ~4.5 us, more than
 * any of these bodies takes: at BASELINE cfg 2 the lengthscale fold, the last gradient cluster and Adam are one launch.  Without hiprtc in the process
 * (hb_ewise_jit_available() == 0) nothing is recorded and every call launches as usual.
 * hb_chain_discard: drop what is recorded without running it and stop recording (returns the number of jobs dropped).
 * hb_chain_source: the generated part of the source the recorded jobs would compile to (diagnostics; launches nothing). */
int hb_chain_begin(void);
int hb_chain_end(void* stream);
int hb_chain_discard(void);
int hb_chain_source(char* out, long cap);
/* hb_chain_compile_dry: compile the kernel of the recorded jobs for gfx950 without loading or launching it (no device
 * needed), drop the jobs and stop recording: the build / CPU check of the generated chains. */
int hb_chain_compile_dry(void);
/* hb_chain_stamps: diagnostics of a chain generated under hb_debug_set("chain_stamps", 1): thread 0 of the chain kernel
 * keeps clock stamps (kernel entry, end of the load phase, end of every job) and stores them when it ends; out[0] = their
 * number, out[1..] the stamps of the chain that ran last.  Synchronises the device; the first call allocates the buffer
 * (call it once before capturing a stream). */
int hb_chain_stamps(unsigned long long* out, long cap);

/* ---- data-parallel exchange step (no reference counterpart: the reference is one tf.Session on one
 *      device, model.py:57,255-269) --------------------------------------------------
 * One process per GPU; the ranks exchange ONE all-reduce (sum) of the flat gradient buffer per Adam
 * step, over RCCL (xGMI inside a node), issued on the caller's stream -- capturable into the step's
 * hipGraph between the backward kernels and hb_adam_step.
 *   hb_comm_available   1 when RCCL could be resolved in this process (it is looked up among the already
 *                       loaded libraries first, then dlopen'ed: the library has no link-time dependency).
 *   hb_comm_unique_id   (host) 128-byte rendezvous token, created on rank 0 and handed to the other ranks
 *                       by the launcher's own channel (henbun_amd.parallel uses torch.distributed for that).
 *   hb_comm_init        collective over all ranks; *comm_out is a (host) handle.
 *   hb_allreduce_sum    in place over `n` elements, asynchronous on `stream`.
 *   hb_dp_pack          tail[0] = objective[0] (nullable -> 0), tail[1] = any(info != 0): the two words that
 *                       ride behind the gradient so that every rank sees the mean objective and a failed
 *                       factorisation on ANY rank blocks the update on EVERY rank (hb_adam_step's dpflag). */
#define HB_COMM_ID_BYTES 128
int hb_comm_available(void);
int hb_comm_unique_id(char* id128);
int hb_comm_init(const char* id128, int rank, int world, void** comm_out);
int hb_comm_destroy(void* comm);
int hb_allreduce_sum_f32(float* buf, long n, void* comm, void* stream);
int hb_allreduce_sum_f64(double* buf, long n, void* comm, void* stream);
int hb_dp_pack_f32(float* tail, const float* objective, const int* info, long n_info, void* stream);
int hb_dp_pack_f64(double* tail, const double* objective, const int* info, long n_info, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HENBUN_HIP_H */
