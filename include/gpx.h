/*
 * gpx.h — C ABI of the MI355X exact-GP regression engine (libgpx.so, gfx950).
 *
 * This is the drop-in boundary for the reference's GP hot path. The reference has no FFI of
 * its own: its seam is the duck-typed GPflow model it calls from Python
 * (SURVEY.md §8b). Each entry point below replaces one piece of GPflow 2.9.1 arithmetic at a
 * reference call site:
 *
 *   gpx_batch_lml_grad  <- model.training_loss + its gradient inside
 *                          gpflow.optimizers.Scipy().minimize(...)   GPR/model_trainer.py:18-19
 *                          (also Multi-Input_GPR/models/model_trainer.py:20-21, 36-37)
 *   gpx_batch_predict   <- model.predict_f(X, full_cov=False)        GPR/model_trainer.py:20,
 *                          GPR/predictor.py:6;  model.predict_y(X)   GPR/predictor.py:7
 *   gpx_batch_predict_full_cov <- model.predict_f(X, full_cov=True)  test_scripts/GPR_Entropy.py:373
 *   gpx_kernel_spec     <- the kernel objects of GPR/main.py:105-114 and the composite
 *                          Exponential*Exponential of Multi-Input_GPR/main.py:118-135
 *
 * Evaluation paths (chosen per problem and per call, results agree to rounding): the dense
 * recursive Cholesky-and-inverse, or — when K and every ∂K/∂θ are exactly zero in fp64 beyond a
 * band of 64-blocks (SE / Matern / Exponential with a lengthscale small against the spacing of
 * sorted inputs, e.g. GPflow's default ℓ = 1 on the reference's integer day offsets) — a
 * block-banded Cholesky, banded solves and selected inversion of K⁻¹ on the band, O(N·bw²).
 * Every banded evaluation checks itself: max_j |Σ_i K_ji Z_ij − 1| over the band (Z the selected
 * inverse) must be <= GPX_BAND_TOL (default 1e-6), else that problem is re-evaluated densely in
 * the same call (selected inversion loses accuracy for very smooth kernels with wide bands).
 * GPX_BAND=0 in the environment forces the dense path.
 *
 * Conventions
 *  - All arithmetic is fp64. X, Y, Xnew and the predict outputs are caller-owned DEVICE
 *    pointers (e.g. torch tensors' data_ptr()); the library never frees them.
 *  - theta / lml / grad / info of gpx_batch_lml_grad are HOST arrays; the call returns when
 *    they are filled (the L-BFGS-B driver on the host needs them immediately).
 *  - theta is in constrained space (θ > 0), row stride GPX_THETA_STRIDE per problem:
 *    theta[b*GPX_THETA_STRIDE + p] for the kernel parameters p < spec.n_params, followed by the
 *    Gaussian noise variance σn² at p = spec.n_params (and, for a slot with a mean function, its
 *    coefficients behind that: gpx_batch_set_mean). grad has the same layout and holds
 *    ∂logML/∂θ (the chain rule to the unconstrained variables is the caller's job).
 *  - Per-term parameter order follows GPflow's tf.Module flattening (sorted attribute names):
 *      SE/Matern12/Matern32/Matern52/Exponential : [lengthscales, variance]
 *      RationalQuadratic                         : [alpha, lengthscales, variance]
 *      Periodic(SquaredExponential)              : [base.lengthscales, base.variance, period]
 *      Linear                                    : [variance]
 *      Coregion (GPX_COREGION)                   : [W row-major (P*R), kappa (P)]
 *    With GPX_TERM_ARD in a stationary term's kind (one lengthscale per active dimension, GPflow's
 *    vector `lengthscales`; see gpx_term below) its dim_count lengthscales take the scalar's place:
 *      SE/Matern/Exponential | GPX_TERM_ARD      : [l_0 .. l_{dim_count-1}, variance]
 *      RationalQuadratic | GPX_TERM_ARD          : [alpha, l_0 .. l_{dim_count-1}, variance]
 *    Such problems always take the dense path, in the same batches and calls as the others.
 *    Signed slots: the W entries of a Coregion term may be any finite value (negative and zero
 *    too). Every other kernel parameter, kappa included, and the noise variance must be finite
 *    and > 0; anything else is GPX_BAD_ARG.
 *  - Return codes: GPX_OK, GPX_NOT_PD (some problem's K+σn²I is not positive definite; its
 *    info[b] holds the 1-based index of the first failing pivot, like LAPACK potrf),
 *    GPX_BAD_ARG, GPX_HIP_ERROR. No C++ exception crosses this boundary.
 *  - A context is bound to one device. Several threads may use one context at the same time
 *    as long as each thread works on its own batch / svgp object (all per-evaluation streams,
 *    events and workspace belong to the batch); a single batch is NOT thread-safe.
 *    gpx_last_error returns the calling thread's most recent failure message (errno-like).
 *    A NULL stream means the context's own stream, which concurrent threads then share
 *    (correct, but their evaluations serialise): pass one stream per thread instead.
 */
#ifndef GPX_H_
#define GPX_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPX_OK 0
#define GPX_NOT_PD 1
#define GPX_BAD_ARG 2
#define GPX_HIP_ERROR 3
/* info[b] of a problem whose evaluation was deferred (gpx_batch_set_deferred): its result comes
 * with a later gpx_batch_lml_grad_complete or gpx_batch_deferred_wait */
#define GPX_INFO_DEFERRED (-1000)

#define GPX_MAX_TERMS 4
#define GPX_THETA_STRIDE 16 /* kernel params + 1 noise slot (+ mean coefficients), per problem */
#define GPX_MAX_DIM 16      /* input dimension D limit */

typedef enum {
  GPX_SE = 1,          /* σ² exp(-r²/2)                         gpflow.kernels.SquaredExponential */
  GPX_MATERN12 = 2,    /* σ² exp(-r)                            gpflow.kernels.Matern12 */
  GPX_MATERN32 = 3,    /* σ² (1+√3r) exp(-√3r)                  gpflow.kernels.Matern32 */
  GPX_MATERN52 = 4,    /* σ² (1+√5r+5r²/3) exp(-√5r)            gpflow.kernels.Matern52 */
  GPX_EXPONENTIAL = 5, /* σ² exp(-r/2)                          gpflow.kernels.Exponential */
  GPX_RQ = 6,          /* σ² (1+r²/(2α))^(-α)                   gpflow.kernels.RationalQuadratic */
  GPX_PERIODIC_SE = 7, /* σ² exp(-½Σ(sin(πΔ/p)/ℓ)²)             gpflow.kernels.Periodic(SE) */
  GPX_LINEAR = 8,      /* σ² x·x'                               gpflow.kernels.Linear */
  GPX_COREGION = 9     /* B[a, b], B = W Wᵀ + diag(κ)           gpflow.kernels.Coregion */
} gpx_term_kind;

typedef enum { GPX_SUM = 0, GPX_PRODUCT = 1 } gpx_combine;

/*
 * ARD (one lengthscale per active dimension, GPflow's vector `lengthscales`): OR this flag into
 * gpx_term.kind. Valid with SE, Matern12/32/52, Exponential and RationalQuadratic and
 * dim_count >= 2 only (anything else: GPX_BAD_ARG). The term then takes dim_count lengthscale
 * slots in place of one, flattened where the scalar sits:
 *      SE/Matern/Exponential | GPX_TERM_ARD : [l_0 .. l_{dim_count-1}, variance]
 *      RationalQuadratic     | GPX_TERM_ARD : [alpha, l_0 .. l_{dim_count-1}, variance]
 * with r² formed from x_d / l_d. A spec with an ARD term always takes the dense route (never band
 * storage's sweeps: gpx_batch_band_width / _band_class report it as dense), its stationary terms
 * may cover at most GPX_MAX_DIM input columns in total (plus D when a Linear or Periodic term is
 * present), it leaves the theta row's last column free (n_params + 1 <= GPX_THETA_STRIDE - 1: up to
 * 13 lengthscales for a single term), and it is accepted by the gpx_batch_* entry points only
 * (gpx_svgp / gpx_sgpr / gpx_vgp refuse it). grad carries dlogML/dl_d in each l_d's column.
 */
#define GPX_TERM_ARD 0x100
#define GPX_TERM_KIND_MASK 0xff

/*
 * Coregion (gpflow.kernels.Coregion, the intrinsic coregionalisation model): a term of kind
 * GPX_COREGION acts on exactly one input column (dim_count == 1) that holds each row's output
 * index a in [0, P). K(x, x') = B[a, a'] with B = W Wᵀ + diag(kappa), W of shape [P, R] (signed)
 * and kappa of shape [P] (> 0). P (output_dim) and R (rank) sit in gpx_kernel_spec.reserved as
 * P | R << 8; the term's theta slots are [W row-major (P*R), kappa (P)] at param_offset, and grad
 * carries dlogML/dW_pr and dlogML/dkappa_p in the same columns. The index is read as an integer
 * and clamped to [0, P - 1] on the device: callers validate it (the Python surface refuses any
 * value that is not an exact integer in [0, P)).
 * A spec holds at most one Coregion term, alone or as one factor of a GPX_PRODUCT spec with any
 * other term kinds (GPX_TERM_ARD ones included). Such a spec always takes the dense route
 * (gpx_batch_band_width / _band_class report -1; band storage runs it on the fallback slots),
 * leaves the theta row's last column free like an ARD spec (n_params + 1 <= GPX_THETA_STRIDE - 1),
 * and is accepted by the gpx_batch_* entry points only (gpx_svgp / gpx_sgpr / gpx_vgp and their
 * *_small_* creators refuse it). Refused with GPX_BAD_ARG and these gpx_last_error texts:
 *   "a Coregion term acts on exactly one input column (dim_count == 1)"
 *   "a Coregion spec needs P >= 1 and R >= 1 in reserved (P | R << 8)"
 *   "a spec may hold one Coregion term"
 *   "a Coregion term is valid alone or in a GPX_PRODUCT spec, not in a GPX_SUM"
 *   "a Coregion spec may use GPX_THETA_STRIDE - 1 columns of the theta row (kernel parameters + noise)"
 *   "reserved must be 0 in a spec without a Coregion term"
 */
typedef struct {
  int32_t kind;         /* gpx_term_kind, optionally | GPX_TERM_ARD */
  int32_t dim_start;    /* active_dims = slice(dim_start, dim_start + dim_count) */
  int32_t dim_count;
  int32_t param_offset; /* index of this term's first parameter in the theta row */
} gpx_term;

typedef struct {
  int32_t n_terms;      /* 1..GPX_MAX_TERMS */
  int32_t combine;      /* gpx_combine (ignored when n_terms == 1) */
  int32_t n_params;     /* kernel parameters; the noise variance sits at theta[n_params] */
  int32_t reserved;     /* P | R << 8 of the spec's Coregion term; 0 without one */
  gpx_term terms[GPX_MAX_TERMS];
} gpx_kernel_spec;

/* Parametric mean function of a GPR problem (gpflow.functions Constant / Linear / Polynomial, one
 * output column). Its coefficients β sit in the θ row behind the noise slot, theta[n_params + 1 + k]
 * for k < n_coef, in the order
 *   CONSTANT   [c]                        m(x) = c                          n_coef = 1
 *   LINEAR     [A_0 .. A_{D-1}, b]        m(x) = Σ_d x_d A_d + b            n_coef = D + 1
 *   POLYNOMIAL [w_0 .. w_degree]          m(x) = Σ_k w_k x^k  (D = 1)       n_coef = degree + 1 <= 5
 * and grad carries ∂logML/∂β_k in the same columns. Coefficients are unconstrained (any finite
 * value); the row must hold them: n_params + 1 + n_coef <= GPX_THETA_STRIDE. */
typedef enum { GPX_MEAN_ZERO = 0, GPX_MEAN_CONSTANT = 1, GPX_MEAN_LINEAR = 2, GPX_MEAN_POLYNOMIAL = 3 } gpx_mean_kind;
typedef struct { int32_t kind, degree, n_coef, reserved; } gpx_mean_spec;

typedef struct gpx_ctx gpx_ctx;
typedef struct gpx_batch gpx_batch;

const char* gpx_version(void);

/* One context per device. */
int gpx_create(int device, gpx_ctx** out);
int gpx_destroy(gpx_ctx* ctx);
const char* gpx_last_error(const gpx_ctx* ctx);

/* The signed theta slots of a spec for inputs of D columns: bit p of *mask_out is set when slot p
 * may hold any finite value (the W entries of a Coregion term); every other kernel parameter and
 * the noise variance must be finite and > 0. Pure host logic, no device needed. GPX_BAD_ARG for a
 * spec that gpx_batch_create would refuse. */
int gpx_spec_signed_mask(const gpx_kernel_spec* spec, int D, uint32_t* mask_out);

/*
 * A batch of B independent GPR problems (the per-asset / per-kernel fits of
 * GPR/main.py:23-37 x GPR/model_trainer.py:14). Problem b has n[b] <= N_max points.
 *   X : device fp64 [B, N_max, D] row-major;  Y : device fp64 [B, N_max].
 *   n : host int32 [B];  specs : host [B].
 * The batch keeps pointers to X and Y (they must outlive it) and owns its HBM workspace
 * (about 4 * B * Np^2 * 8 bytes, Np = N_max rounded up to 64).
 */
int gpx_batch_create(gpx_ctx* ctx, int B, int N_max, int D, const double* X, const double* Y,
                     const int32_t* n, const gpx_kernel_spec* specs, gpx_batch** out);
/*
 * gpx_batch_create with BAND STORAGE, for many resident slots of banded problems (the
 * continuous-batching fits of configuration C2: SE / Matern / Exponential kernels on sorted
 * day offsets, GPR/data_handler.py:42-44 + GPR/model_trainer.py:15, whose K is exactly zero in
 * fp64 beyond one or two 64-blocks off the diagonal). The workspace keeps only the band of two
 * 64-blocks: 3 * Np * 257 * 8 bytes per slot (25 MiB at N = 4096 instead of 384 MiB), so ~10x
 * more slots fit in HBM. Same calls and results as a gpx_batch_create batch; evaluations the
 * fused banded sweeps cannot take (a wider band, another kernel family, a failed band check)
 * and predictions that need a fresh factor run densely on 4 internal fallback slots in the
 * same call. 449 <= N_max <= 8192.
 */
int gpx_batch_create_banded(gpx_ctx* ctx, int B, int N_max, int D, const double* X, const double* Y,
                            const int32_t* n, const gpx_kernel_spec* specs, gpx_batch** out);
int gpx_batch_destroy(gpx_batch* batch);

/*
 * Rebind slot b to a new problem: the caller has already written its inputs into row b of
 * the X / Y arrays given at creation (n <= N_max valid points); this updates n[b] and the
 * kernel spec and invalidates the slot's cached factor. Used to stream many fits through a
 * fixed set of device slots (continuous batching).
 */
int gpx_batch_rebind(gpx_batch* batch, int b, int n, const gpx_kernel_spec* spec);

/*
 * gpx_batch_rebind with the problem's inputs given on the HOST (X [n, D], Y [n], fp64): they are
 * copied into the slot's pinned staging region at once (the host buffers may be reused on
 * return) and reach slot b of the batch's X / Y arrays by DMA at the start of the next device
 * call on the batch, on that call's stream. Rows n .. N_max-1 of the slot are zeroed.
 * `stream` is unused (kept for the ABI).
 */
int gpx_batch_rebind_host(gpx_batch* batch, int b, int n, const double* X, const double* Y,
                          const gpx_kernel_spec* spec, void* stream);
/* The same with the inputs in DEVICE memory (X [n, D], Y [n], e.g. a model's resident tensors):
 * only recorded; the next device call on the batch gathers every pending slot in one kernel on
 * its stream (which also returns the per-16-row-block boxes of X for the band tables), so X and Y
 * must stay valid and unchanged until that call has been issued and completed. `stream` (may be
 * NULL) is the stream in whose order X and Y are ready (their producer's): an event recorded on
 * it here is waited on by the gather when that runs on another stream. */
int gpx_batch_rebind_device(gpx_batch* batch, int b, int n, const double* X, const double* Y,
                            const gpx_kernel_spec* spec, void* stream);
/* gpx_batch_rebind_device with the per-16-row-block bounding boxes of X supplied by the caller
 * (host array, for each of the ceil(n/16) blocks and each of the D columns the pair (min, max)
 * of that column over the block's rows: [ceil(n/16)][D][2]), as gpx_batch_slot_boxes returned
 * them for the same X earlier: the band tables are computed here and the next call's gather
 * needs no box download (and no stream synchronise) for this slot. */
int gpx_batch_rebind_device_boxed(gpx_batch* batch, int b, int n, const double* X, const double* Y,
                                  const gpx_kernel_spec* spec, const double* boxes, void* stream);
/*
 * The mean function of slot b (NULL or kind GPX_MEAN_ZERO: zero mean, the state of every slot after
 * creation and after ANY gpx_batch_rebind* of it). With r = y − m(X; β) every evaluation runs on r:
 * logML and the kernel / noise gradients are the zero-mean formulas on r, ∂logML/∂β_k =
 * Σ_j α_j ∂m(x_j)/∂β_k, predictions at new inputs gain m(X*), variances do not change. A slot with
 * kind CONSTANT and c = 0 gives the zero-mean bits. Refused (GPX_BAD_ARG) on band-storage batches,
 * while deferred completion is on, while an evaluation is submitted, and when the θ row is too short.
 */
int gpx_batch_set_mean(gpx_batch* batch, int b, const gpx_mean_spec* mean);
/* The boxes of slot b's X (layout as above) as computed when its inputs were last gathered;
 * GPX_BAD_ARG if unknown (not gathered yet, host-staged, or no band tables for this batch's
 * shape). For a caller that caches them per series. */
int gpx_batch_slot_boxes(const gpx_batch* batch, int b, double* boxes);

/*
 * logML and ∂logML/∂θ at theta for the n_active problems listed in active (host int32).
 * Outputs are written at each active problem's row: lml[b], grad[b*GPX_THETA_STRIDE + p],
 * info[b]. stream may be NULL (library stream). Returns after the outputs are on the host.
 */
int gpx_batch_lml_grad(gpx_batch* batch, int n_active, const int32_t* active, const double* theta,
                       double* lml, double* grad, int32_t* info, void* stream);

/*
 * gpx_batch_lml_grad in two halves, so one host thread can keep several batches in flight:
 * _submit validates, routes and enqueues the whole evaluation (uploads, kernels and the
 * download of the results into pinned memory) on `stream` and returns without waiting;
 * _complete waits for it, writes lml / grad / info exactly as gpx_batch_lml_grad does (and
 * re-evaluates densely, synchronously, any banded problem whose check failed). One submitted
 * evaluation per batch at a time; the batch must not be used in between (other batches may).
 * theta is copied by _submit. gpx_batch_lml_grad = _submit + _complete.
 */
int gpx_batch_lml_grad_submit(gpx_batch* batch, int n_active, const int32_t* active, const double* theta,
                              void* stream);
int gpx_batch_lml_grad_complete(gpx_batch* batch, double* lml, double* grad, int32_t* info);
/* 1 when the submitted evaluation (if any) has finished on the device (complete will not
 * wait), 0 while it runs; < 0 on error. */
int gpx_batch_lml_grad_query(gpx_batch* batch);
/*
 * Host-side routing query: for rows[i] at theta (the gpx_batch_lml_grad layout), the band
 * width in 64-blocks the evaluation would take (>= 0: the block-banded path), -1 for the
 * dense path, -2 when the row's band tables are not known yet (a device rebind still waiting
 * for the next call's gather). No device work.
 */
int gpx_batch_band_width(gpx_batch* batch, int n_rows, const int32_t* rows, const double* theta, int32_t* p_out);
/* The path an evaluation of each row at theta would take, host-side (no device work), as
 * gpx_batch_lml_grad_submit routes it: 1..15 = the band16 sweeps with a band of that many 16-row
 * blocks; 16 + p = the 64-row banded path with p 64-blocks in a batch without band16 tables;
 * 32 + p = the 64-row banded path although the batch has band16 tables (the band is wider than
 * the band16 sweeps take); -1 = dense (or, band storage, the fallback slots); -2 = not known yet
 * (a rebind whose gather runs with the next call). Callers that keep several batches use it to
 * evaluate the slow classes apart from the fast ones (Scipy.minimize_stream wide_group). */
int gpx_batch_band_class(gpx_batch* batch, int n_rows, const int32_t* rows, const double* theta, int32_t* cls_out);
/* Deferred completion of the slow evaluation classes. With q >= 0, the problems of a call whose
 * evaluation takes the band16 sweeps wider than q 16-row blocks, or the 64-row banded sweeps,
 * run on a stream of their own and gpx_batch_lml_grad_complete returns without waiting for them:
 * it reports info[b] = GPX_INFO_DEFERRED for those rows, and delivers (lml, grad, info) of
 * deferred rows of earlier calls whose work has finished by then (rows of neither kind are not
 * written). A deferred row may not be evaluated, predicted or rebound until it is delivered;
 * gpx_batch_deferred_wait blocks until every deferred row is delivered (into its arrays; it is
 * refused, GPX_BAD_ARG, while an evaluation is submitted on the batch and not completed). The
 * call's other problems never wait for the slow classes, whose sweeps (one wavefront per SIMD,
 * or 73 KiB of LDS per workgroup) start late under a full band16 load. Same results, bit for
 * bit, as without deferral. q < 0 turns it off (the default). */
/* Which banded route the batch's band16 problems take (GPX_BAND_ROUTE_*), a property of the batch,
 * never of a call: a problem's arithmetic then depends on its own data, θ and this setting only —
 * not on how many problems share its call — so a fit reproduces bit for bit whichever fits run
 * beside it (the solo GPR of GPR/model_trainer.py:15-19 and the same series inside a batch of
 * thousands give the same trajectory).
 *   SWEEPS (0, the default): the one-wavefront band16 sweeps (throughput: thousands of problems
 *     in flight fill the chip);
 *   BCR (1): block cyclic reduction for the widths it covers (Q <= 5; log-depth latency for calls
 *     of a few problems, ~4x the sweeps' work), wider problems on the 64-row sweeps;
 *   AUTO (2): BCR for calls of at most GPX_BCR_MAX (default 32) band16 problems, else the sweeps —
 *     the round-5 rule, whose results depend on the call's size (the two routes agree to ~1e-9
 *     relative, not bit for bit).
 * The environment variable GPX_BCR_MAX, when set, overrides the setting for every batch of the
 * process (0: sweeps, a large value: BCR; the A/B knob of the tests and tools). */
#define GPX_BAND_ROUTE_SWEEPS 0
#define GPX_BAND_ROUTE_BCR 1
#define GPX_BAND_ROUTE_AUTO 2
int gpx_batch_set_band_route(gpx_batch* batch, int route);
int gpx_batch_set_deferred(gpx_batch* batch, int q);
int gpx_batch_deferred_wait(gpx_batch* batch, double* lml, double* grad, int32_t* info);
/* rows with a deferred evaluation in flight: writes up to cap slot indices, returns the count */
int gpx_batch_deferred_rows(const gpx_batch* batch, int32_t* rows, int cap);

/*
 * Posterior marginals at Xnew for the active problems: GPflow GPR.predict_f(full_cov=False)
 * (add_noise = 0) or predict_y (add_noise = 1: variance + σn²).
 *   Xnew : device fp64 [B, M, D];  mean, var : device fp64 [B, M] (caller-owned).
 * theta/info are host arrays as above. Re-factorises K+σn²I at theta like GPflow (no caching
 * across calls unless theta is bit-identical to the last factorisation of that problem).
 */
int gpx_batch_predict(gpx_batch* batch, int n_active, const int32_t* active, const double* theta,
                      const double* Xnew, int M, int add_noise, double* mean, double* var,
                      int32_t* info, void* stream);

/*
 * gpx_batch_predict at each problem's own training inputs (GPR/model_trainer.py:20,
 * predict_f(X_train)) in O(N²) from the factor: with Kxs = K_y − σn²I, GPflow's
 * Kxsᵀα = y − σn²α and k_jj − colsum((L⁻¹Kxs)²)_j = σn² − σn⁴ [K_y⁻¹]_jj exactly.
 *   mean, var : device fp64 [B, N_max] (rows < n[b] written).
 */
int gpx_batch_predict_train(gpx_batch* batch, int n_active, const int32_t* active,
                            const double* theta, int add_noise, double* mean, double* var,
                            int32_t* info, void* stream);

/*
 * gpx_batch_predict_train with the outputs packed by position: mean, var : device fp64
 * [n_active, N_max], row i for problem active[i] (rows < n[active[i]] written). A caller that
 * keeps each fit's prediction (the stepped drivers: a few dozen finished fits per round of a
 * 1024-slot batch) allocates only those rows. Same values as gpx_batch_predict_train.
 */
int gpx_batch_predict_train_rows(gpx_batch* batch, int n_active, const int32_t* active,
                                 const double* theta, int add_noise, double* mean, double* var,
                                 int32_t* info, void* stream);

/*
 * Posterior mean and FULL covariance at Xnew: GPflow GPR.predict_f(Xnew, full_cov=True)
 * (GPflow returns the covariance as [1, M, M]; predict_y has no full_cov form in GPflow).
 *   Xnew : device fp64 [B, M, D];  mean : device fp64 [B, M];  cov : device fp64 [B, M, M].
 * cov[b] = k(X*,X*) − Kxsᵀ (K+σn²I)⁻¹ Kxs, formed as k(X*,X*) − AᵀA with A = L⁻¹·Kxs (MFMA).
 */
int gpx_batch_predict_full_cov(gpx_batch* batch, int n_active, const int32_t* active,
                               const double* theta, const double* Xnew, int M, double* mean,
                               double* cov, int32_t* info, void* stream);

/*
 * Joint draws from Gaussians on the device (GPflow's sample_mvn(full_cov=True) arithmetic), fp64:
 * for problem b with M points and S samples
 *   A = cov[b] + jitter*I   (one add per diagonal entry; only the lower triangle of cov is read)
 *   L = chol(A), lower
 *   out[b, s, i] = mean[b, i] + sum_{k <= i} L[i, k] * white[b, s, k]
 * One algorithm for every M (right-looking, blocks of 64: diagonal block and panel per step in one
 * kernel, trailing update and L*white^T on the batched fp64 MFMA GEMM). A problem's output bits are
 * the same alone and inside any batch, and sample s does not depend on S.
 * gpx_sample_mvn: every buffer is the caller's (device, fp64, contiguous): mean [B, M], cov
 * [B, M, M], white [B, S, M] (standard normal draws, or any vectors), out [B, S, M]. info (host,
 * [B]) gets the 1-based index of the first pivot of A that is not > 0 and finite (as LAPACK potrf),
 * else 0; with some info[b] != 0 the call returns GPX_NOT_PD, that problem's out rows are NOT
 * written and the other problems' are correct. The call returns when out is filled; calls on one
 * context take turns (they share its workspace). Limits: 1 <= M <= the value of gpx_sample_limits
 * (8192; needs no device), S >= 1, jitter finite and >= 0.
 * gpx_batch_predict_samples: the posterior of gpx_batch_predict_full_cov at Xnew (device
 * [B, M, D]) followed by the sampler, in one call with one synchronise: the covariance stays in the
 * batch's workspace (no [M, M] copy-out, no host round trip). mean (device [B, M]) and out (device
 * [B, S, M]) are written for the active rows; white is device [B, S, M], indexed by slot like them.
 * Works on every batch gpx_batch_predict_full_cov works on (band storage, ARD, Coregion and mean
 * function specs included). info[b] != 0 if either factorisation failed (GPX_NOT_PD);
 * gpx_last_error names which: "K + noise*I ..." or "the posterior covariance + jitter*I ...".
 * GPX_BAD_ARG (with a message): null pointers, M <= 0, S <= 0, M over the limit, a negative or
 * non-finite jitter, a problem with a deferred evaluation in flight. A NULL ctx / batch is
 * GPX_BAD_ARG without touching a device.
 */
int gpx_sample_limits(int* m_max);
int gpx_sample_mvn(gpx_ctx* ctx, int B, int M, int S, const double* mean, const double* cov,
                   const double* white, double jitter, double* out, int32_t* info, void* stream);
int gpx_batch_predict_samples(gpx_batch* batch, int n_active, const int32_t* active, const double* theta,
                              const double* Xnew, int M, int S, const double* white, double jitter,
                              double* mean, double* out, int32_t* info, void* stream);

/* Timing hooks for bench.py: total device time (ms) of the last call's kernels, measured with
 * HIP events on the stream they ran on, split by phase. */
typedef struct {
  double factor_ms;   /* K build + recursive Cholesky-and-inverse */
  double alpha_ms;    /* the two triangular matrix-vector products */
  double grad_ms;     /* fused K^-1 = W^T W formation + gradient contraction + reduce */
  double predict_ms;  /* predict-only kernels */
  double total_ms;
  double gemm_flops;  /* MFMA flops issued by the GEMM kernels of the last call */
  /* cumulative since the last gpx_batch_reset_timing, profiling enabled only: the fused
   * K^-1 = W^T W + gradient-contraction kernel (one launch per gpx_batch_lml_grad call) */
  double contract_ms_total;
  double contract_launches;
  double contract_alg_flops;  /* algorithmic flops of those launches: n_active * sum_i 2(i+1)(Np-i) */
  double eval_ms_total;       /* whole gpx_batch_lml_grad device time */
  double evals;               /* problem-evaluations (sum of n_active) */
  /* block-banded path (cumulative, profiling enabled only): device time of its part of the
   * calls, calls that had banded problems, banded problem-evaluations, Σ band width p (64-blocks)
   * over those evaluations */
  double band_ms_total;
  double band_calls;
  double band_evals;
  double band_p_sum;
  /* fused banded kernels (p <= 2), each launch timestamped at its actual start and end:
   * summed durations, launches, and block-product flops issued (2·64³ per 64³ product, the
   * leaf counted as 2/3 of one) */
  double band_fwd_ms_total;
  double band_bwd_ms_total;
  double band_fused_launches;
  double band_fwd_flops;
  double band_bwd_flops;
  double band_fallbacks;      /* banded evaluations whose check failed, redone densely */
  double shadow_evals;        /* band storage: evaluations run on the dense fallback slots */
  double shadow_predicts;     /* band storage: predictions run on the dense fallback slots */
  /* 16-row-block banded sweeps (one wavefront per problem, band of Q <= 4 16-blocks): summed
   * launch durations, launch pairs, problem-evaluations, Σ Q, and the MFMA flops they issue
   * (2·16³ per tile product) */
  double band16_fwd_ms_total;
  double band16_bwd_ms_total;
  double band16_launches;
  double band16_evals;
  double band16_q_sum;
  double band16_fwd_flops;
  double band16_bwd_flops;
  /* Σ over band16 launches of (problems in the launch) × (its duration, ms): the wave-ms the
   * sweeps held (one wavefront per problem); ÷ (wave slots × wall ms) = their occupancy */
  double band16_wave_ms;
  /* the deferred part's wide launches (band16_wide_kernel: the Q = 4 and 5 classes of a call, both
   * sweeps per wavefront): their durations, count, MFMA flops and problems — kept out of the
   * band16 forward/backward launch figures above (which count the per-class launches only) */
  double band16_wide_ms_total, band16_wide_launches, band16_wide_flops, band16_wide_evals;
  /* block cyclic reduction (calls with at most GPX_BCR_MAX band16 problems): the device time of
   * the reduction chains (forward and backward levels, contraction), chains, problem-evaluations */
  double bcr_ms_total, bcr_calls, bcr_evals;
  /* of band_fused_launches: the timed 64-row launch pairs that were the p = 2 class's
   * (band_fwd_kernel / band_bwd_kernel) rather than the p <= 1 class's (band_fwd1_kernel / band_bwd1_kernel) */
  double band_fused_p2_launches;
  /* band16 problem-evaluations of widths Q = 6..8 taken by the block-cyclic-reduction chain of block
   * size 128 (whatever the batch's route; they no longer run as one-wavefront sweeps) */
  double bcr_wide_evals;
} gpx_timing;
int gpx_batch_last_timing(const gpx_batch* batch, gpx_timing* out);
int gpx_batch_reset_timing(gpx_batch* batch);
/* Diagnostic: per-wavefront residency records of the band16 sweeps (one wavefront walks one
 * problem), for occupancy timelines across processes sharing a GPU. cap > 0 allocates room for
 * cap records and turns recording on; 0 frees it and turns it off (both synchronise the device).
 * Each record is three uint64: start and end in the device's constant 100 MHz clock
 * (s_memrealtime, one clock for every process on the GPU) and kind = Q (forward sweep) or
 * 16 + Q (backward sweep). _read synchronises the device, copies up to cap records into out,
 * sets *n_out and restarts the recording. */
int gpx_batch_wave_trace(gpx_batch* batch, unsigned int cap);
int gpx_batch_wave_trace_read(gpx_batch* batch, unsigned long long* out, unsigned int cap, unsigned int* n_out);
int gpx_set_profiling(gpx_ctx* ctx, int enabled);

/* ---------------------------------------------------------------------------------------
 * SVGP: gpflow.models.SVGP(kernel, Gaussian(σn²), inducing_variable=Z, num_data=...) with
 * GPflow's defaults (whiten=True, full lower-triangular q_sqrt, zero mean, one latent GP) —
 * test_scripts/SVGP.py:461-478 (M=120), :515-540 (M=20), test_scripts/GPR.py:118-138.
 *   gpx_svgp_elbo_grad  <- training_loss_closure((X, Y)) value + gradient, fed to
 *                          gpflow.optimizers.Scipy().minimize (test_scripts/SVGP.py:471-474)
 *   gpx_svgp_predict    <- model.predict_f(X_test) / predict_y          (SVGP.py:478)
 *
 * One gpx_svgp holds one shard of the data: X [N, D] and Y [N] (device, fp64, caller-owned).
 * n_total = rows over all shards (= N on one GPU); the ELBO's data term is scaled by
 * num_data / n_total like GPflow's minibatch scaling. Per evaluation:
 *   theta  host [16]: kernel params (gpx_kernel_spec layout) then σn² at theta[n_params]
 *   Z      host [M, D]   inducing inputs;   q_mu host [M];   q_sqrt host [M, M] row-major,
 *          lower triangle used (the FillTriangular-constrained value)
 * Outputs (host): elbo; grad_theta [16] (∂ELBO/∂θ constrained, σn² at n_params);
 *   grad_Z [M, D]; grad_qmu [M]; grad_qsqrt [M, M] (lower triangle, upper zero).
 * Sharded use: gpx_svgp_eval_local on every shard, sum the gpx_svgp_partials() device
 * buffers over shards (one all-reduce), then gpx_svgp_eval_finish. gpx_svgp_elbo_grad is
 * local + finish for the unsharded case (n_total == N).
 */
typedef struct gpx_svgp gpx_svgp;
int gpx_svgp_create(gpx_ctx* ctx, int N, int M, int D, const double* X, const double* Y,
                    const gpx_kernel_spec* spec, double num_data, long long n_total,
                    gpx_svgp** out);
/* The same model with a Gaussian or StudentT likelihood (GPX_LIK_*, below), evaluated by the
 * per-point route: the marginal (μ_n, v_n) of every data row, GPflow's variational expectation of
 * it (closed form for the Gaussian, the 20-point Gauss–Hermite rule for StudentT, the arithmetic of
 * gpx_vgp) and per-row weights through the same M x M algebra — three M²N GEMM passes plus element
 * passes over M x N; one more M x N buffer than gpx_svgp_create. An object from here takes this
 * route for BOTH likelihoods: with GPX_LIK_GAUSSIAN it computes the ELBO of gpx_svgp_create by the
 * general route (equal up to summation order; gpx_svgp_create keeps its closed-form path and its
 * bits). theta[n_params] is the likelihood parameter, finite and > 0: the Gaussian variance or the
 * StudentT scale; grad_theta[n_params] is its gradient. df (StudentT only; fixed) must be finite and
 * > 0 at create; predict with add_noise adds scale²·df/(df − 2) and needs df > 2 (GPX_BAD_ARG
 * otherwise). The partials / bind_partials / eval_local / eval_finish / elbo_grad / predict /
 * destroy calls below serve both kinds of object; the partial buffer has the same length and layout
 * except its scalars, which are Σ ve, Σ ∂ve/∂φ, n_local here. Shards of one model must all come
 * from the same create call. */
int gpx_svgp_create_lik(gpx_ctx* ctx, int N, int M, int D, const double* X, const double* Y,
                        const gpx_kernel_spec* spec, double num_data, long long n_total,
                        int likelihood /* GPX_LIK_* */, double df, gpx_svgp** out);
int gpx_svgp_destroy(gpx_svgp* svgp);
/* the partial-sum buffer (device, fp64, len doubles) and a way to substitute a caller-owned
 * one (e.g. a torch tensor that torch.distributed all-reduces in place) */
int gpx_svgp_partials(gpx_svgp* svgp, double** dev_ptr, long long* len);
int gpx_svgp_bind_partials(gpx_svgp* svgp, double* dev_ptr, long long len);
int gpx_svgp_eval_local(gpx_svgp* svgp, const double* theta, const double* Z, const double* q_mu,
                        const double* q_sqrt, int32_t* info, void* stream);
int gpx_svgp_eval_finish(gpx_svgp* svgp, double* elbo, double* grad_theta, double* grad_Z,
                         double* grad_qmu, double* grad_qsqrt, void* stream);
int gpx_svgp_elbo_grad(gpx_svgp* svgp, const double* theta, const double* Z, const double* q_mu,
                       const double* q_sqrt, double* elbo, double* grad_theta, double* grad_Z,
                       double* grad_qmu, double* grad_qsqrt, int32_t* info, void* stream);
/* predict_f (add_noise = 0) / predict_y (1) at Xnew (device [Mn, D]) -> mean, var (device [Mn]) */
int gpx_svgp_predict(gpx_svgp* svgp, const double* theta, const double* Z, const double* q_mu,
                     const double* q_sqrt, const double* Xnew, int Mn, int add_noise, double* mean,
                     double* var, int32_t* info, void* stream);

/* ---------------------------------------------------------------------------------------
 * A batch of small SVGP models, one fused launch per call: the sweep of the reference's
 * train_svgp_model (test_scripts/GPR.py:118-138, GPR_Entropy.py:137-157, SVGP.py:459-545: per
 * kernel one SVGP(kernel, Gaussian(1e-4), inducing_variable=X[:20]), N = 5..~800). The model and
 * its arithmetic are gpx_svgp_create's (whitened, Gaussian likelihood by the closed form, jitter
 * 1e-6, num_data scaling with n_total = n); each model is evaluated whole by one workgroup.
 * Limits (gpx_svgp_small_limits; over them GPX_BAD_ARG): M <= 32, N <= 4096, D <= GPX_MAX_DIM;
 * specs with GPX_TERM_ARD are refused as by gpx_svgp_create.
 *
 * An object has B slots for models of one input dimension D with n <= N_max rows and m <= M_max
 * inducing points. gpx_svgp_small_bind copies a model's X [n, D] and Y [n] (host, fp64) into slot b.
 * Per call, all host fp64 arrays indexed by SLOT, of which only the rows of the active slots are
 * read / written, and of a row only the model's own leading entries (its tail is never read):
 *   theta   [B][16]           kernel params then σn² at theta[n_params], as gpx_svgp_elbo_grad
 *   Z       [B][M_max·D]      the slot's [m, D] inducing inputs, row-major, at the row's start
 *   q_mu    [B][M_max]        its m entries
 *   q_sqrt  [B][M_max·M_max]  its [m, m] row-major matrix (row stride m), lower triangle read
 * Outputs: elbo [B]; grad_theta [B][16]; grad_Z, grad_q_mu, grad_q_sqrt in the layouts of Z, q_mu,
 * q_sqrt (grad_q_sqrt: zeros above the diagonal); info [B]: the 1-based index of the first pivot of
 * Kmm + 1e-6 I that is not > 0, else 0. GPX_NOT_PD when some active slot's info != 0 — that slot's
 * outputs are then unspecified, the other slots' stay valid. theta not finite or <= 0, a non-finite
 * Z and a zero diagonal of q_sqrt return GPX_BAD_ARG before anything is launched.
 * A model's outputs are a function of its own inputs alone, bit for bit: they do not depend on B,
 * on its slot, on its place in `active`, or on what else the call evaluates.
 * gpx_svgp_small_predict: predict_f (add_noise = 0) / predict_y (1) of slot b at Xnew (HOST
 * [Mn, D]) -> mean, var (HOST [Mn]); theta [16], Z [m, D], q_mu [m], q_sqrt [m, m] of that one model.
 * Calls return when the outputs are filled; one object serves one thread at a time.
 */
typedef struct gpx_svgp_small gpx_svgp_small;
int gpx_svgp_small_limits(int* m_max, int* n_max); /* 32, 4096; needs no device */
int gpx_svgp_small_create(gpx_ctx* ctx, int B, int N_max, int M_max, int D, gpx_svgp_small** out);
int gpx_svgp_small_bind(gpx_svgp_small* small, int b, int n, int m, const double* X, const double* Y,
                        const gpx_kernel_spec* spec, double num_data);
int gpx_svgp_small_elbo_grad(gpx_svgp_small* small, int n_active, const int32_t* active,
                             const double* theta, const double* Z, const double* q_mu,
                             const double* q_sqrt, double* elbo, double* grad_theta, double* grad_Z,
                             double* grad_q_mu, double* grad_q_sqrt, int32_t* info, void* stream);
int gpx_svgp_small_predict(gpx_svgp_small* small, int b, const double* theta, const double* Z,
                           const double* q_mu, const double* q_sqrt, const double* Xnew, int Mn,
                           int add_noise, double* mean, double* var, int32_t* info, void* stream);
int gpx_svgp_small_destroy(gpx_svgp_small* small);

/* ---------------------------------------------------------------------------------------
 * SGPR: gpflow.models.SGPR((X, Y), kernel, inducing_variable=Z, noise_variance=...) — the
 * collapsed (Titsias) bound of sparse GP regression with a Gaussian likelihood, zero mean, one
 * output; test_scripts/SVGP.py:395-412 (SE kernel, M = 10, N ≈ 113).
 *   gpx_sgpr_elbo_grad  <- model.training_loss value + gradient, fed to
 *                          gpflow.optimizers.Scipy().minimize(model.training_loss, ...)
 *   gpx_sgpr_predict    <- model.predict_f(X_test) / predict_y
 * X [N, D] and Y [N] are device-resident fp64 and caller-owned; they must outlive the object.
 * Per evaluation (host): theta [16] = kernel params (gpx_kernel_spec layout) then σn² at
 * theta[n_params]; Z [M, D] row-major. Outputs (host): elbo; grad_theta [16] (∂F/∂θ constrained,
 * σn² at n_params); grad_Z [M, D].
 * Two M x M factorisations run per call, so info points to TWO int32: info[0] the first failing
 * pivot (1-based, 0 = ok) of Kmm = k(Z,Z) + 1e-6 I, info[1] that of B = I + L⁻¹ Kmn Kmnᵀ L⁻ᵀ/σn²
 * (I + PSD: a failure there means a non-finite input). Either one returns GPX_NOT_PD.
 * Not provided: mean functions, multi-output Y, full_cov, upper_bound, other likelihoods (those
 * are gpx_vgp's), and row-sharding over GPUs — K̄mn depends on the all-reduced B, so shards would
 * need a two-pass protocol that gpx_svgp_partials does not give.
 */
typedef struct gpx_sgpr gpx_sgpr;
int gpx_sgpr_create(gpx_ctx* ctx, int N, int M, int D, const double* X, const double* Y,
                    const gpx_kernel_spec* spec, gpx_sgpr** out);
int gpx_sgpr_destroy(gpx_sgpr* sgpr);
int gpx_sgpr_elbo_grad(gpx_sgpr* sgpr, const double* theta, const double* Z, double* elbo,
                       double* grad_theta, double* grad_Z, int32_t* info, void* stream);
/* predict_f (add_noise = 0) / predict_y (1) at Xnew (device [Mn, D]) -> mean, var (device [Mn]) */
int gpx_sgpr_predict(gpx_sgpr* sgpr, const double* theta, const double* Z, const double* Xnew, int Mn,
                     int add_noise, double* mean, double* var, int32_t* info, void* stream);

/* ---------------------------------------------------------------------------------------
 * A batch of small SGPR models, one fused launch per call: a sweep of the reference's SGPR cell
 * (test_scripts/SVGP.py:393-400: SGPR((X, Y), SquaredExponential(), inducing_variable =
 * np.linspace(0, 360, 10)[:, None]), N ≈ 113, M = 10) over kernels, inducing counts and series. The
 * model and its arithmetic are gpx_sgpr_create's (collapsed bound, Gaussian likelihood, zero mean,
 * jitter 1e-6, explicit W = L⁻¹ and WB = LB⁻¹); each model is evaluated whole by one workgroup, in
 * two passes over its data. Limits (gpx_sgpr_small_limits; over them GPX_BAD_ARG): M <= 32,
 * N <= 4096, D <= GPX_MAX_DIM; specs with GPX_TERM_ARD are refused as by gpx_sgpr_create.
 *
 * An object has B slots for models of one input dimension D with n <= N_max rows and m <= M_max
 * inducing points. gpx_sgpr_small_bind copies a model's X [n, D] and Y [n] (host, fp64) into slot b.
 * Per call, all host fp64 arrays indexed by SLOT, of which only the rows of the active slots are
 * read / written, and of a row only the model's own leading entries (its tail is never read):
 *   theta   [B][16]           kernel params then σn² at theta[n_params], as gpx_sgpr_elbo_grad
 *   Z       [B][M_max·D]      the slot's [m, D] inducing inputs, row-major, at the row's start
 * Outputs: elbo [B]; grad_theta [B][16]; grad_Z in the layout of Z; info [B][2]: the 1-based index of
 * the first pivot that is not > 0 of Kmm + 1e-6 I (info[b][0]) and of B = I + L⁻¹ Kmn Kmnᵀ L⁻ᵀ/σn²
 * (info[b][1]), else 0. GPX_NOT_PD when some active slot's info != 0 — that slot's outputs are then
 * unspecified, the other slots' stay valid. theta not finite or <= 0 and a non-finite Z return
 * GPX_BAD_ARG before anything is launched.
 * A model's outputs are a function of its own inputs alone, bit for bit: they do not depend on B,
 * on its slot, on its place in `active`, or on what else the call evaluates.
 * gpx_sgpr_small_predict: predict_f (add_noise = 0) / predict_y (1) of slot b at Xnew (HOST
 * [Mn, D]) -> mean, var (HOST [Mn]); theta [16] and Z [m, D] of that one model; info points to two
 * int32. Mn = 0 is allowed and writes nothing.
 * Calls return when the outputs are filled; one object serves one thread at a time.
 */
typedef struct gpx_sgpr_small gpx_sgpr_small;
int gpx_sgpr_small_limits(int* m_max, int* n_max); /* 32, 4096; needs no device */
int gpx_sgpr_small_create(gpx_ctx* ctx, int B, int N_max, int M_max, int D, gpx_sgpr_small** out);
int gpx_sgpr_small_bind(gpx_sgpr_small* small, int b, int n, int m, const double* X, const double* Y,
                        const gpx_kernel_spec* spec);
int gpx_sgpr_small_elbo_grad(gpx_sgpr_small* small, int n_active, const int32_t* active,
                             const double* theta, const double* Z, double* elbo, double* grad_theta,
                             double* grad_Z, int32_t* info, void* stream);
int gpx_sgpr_small_predict(gpx_sgpr_small* small, int b, const double* theta, const double* Z,
                           const double* Xnew, int Mn, int add_noise, double* mean, double* var,
                           int32_t* info, void* stream);
int gpx_sgpr_small_destroy(gpx_sgpr_small* small);

/* ---------------------------------------------------------------------------------------
 * VGP: gpflow.models.VGP((X, Y), kernel, likelihood) with GPflow's defaults — whitened
 * q(f) = N(L q_mu, L q_sqrt q_sqrtᵀ Lᵀ), L = chol(k(X,X) + 1e-6 I), full q_sqrt, zero mean, one
 * output; test_scripts/SVGP.py:402-437 (SE kernel, StudentT likelihood, N ≈ 113).
 *   gpx_vgp_elbo_grad  <- model.training_loss value + gradient, fed to
 *                         gpflow.optimizers.Scipy().minimize(model.training_loss, ...)
 *   gpx_vgp_predict    <- model.predict_f(X_test) (predict_y = 0) / model.predict_y (1)
 * likelihood: GPX_LIK_GAUSSIAN (closed-form variational expectation) or GPX_LIK_STUDENT_T
 * (GPflow's 20-point Gauss–Hermite rule; df is fixed at create and must be > 0, predict_y
 * needs df > 2).
 * X [N, D] and Y [N] are device-resident fp64 and caller-owned; they must outlive the object.
 * Per evaluation (host): theta [16] = kernel params (gpx_kernel_spec layout) then the likelihood
 * parameter at theta[n_params] (Gaussian variance / StudentT scale); q_mu [N]; q_sqrt [N][N]
 * row-major, its lower triangle is read. Outputs (host): elbo; grad_theta [16] (constrained,
 * likelihood parameter at n_params); grad_qmu [N]; grad_qsqrt [N][N] (lower, zeros above).
 * X is data: no input gradient. info: first failing pivot (1-based, 0 = ok) of k(X,X) + 1e-6 I
 * (GPX_NOT_PD). theta not finite or <= 0, non-finite q_mu / q_sqrt and a zero diagonal of q_sqrt
 * return GPX_BAD_ARG. The workspace is thirteen N x N fp64 matrices.
 * predict: Xnew device [Mn, D] -> mean, var device [Mn]; predict_y adds the likelihood's
 * variance (σn², or scale²·df/(df − 2)).
 * Not provided: mean functions, multi-output Y, full_cov, sharding, several VGPs per call.
 */
enum { GPX_LIK_GAUSSIAN = 0, GPX_LIK_STUDENT_T = 1 };
typedef struct gpx_vgp gpx_vgp;
int gpx_vgp_create(gpx_ctx* ctx, int N, int D, const double* X, const double* Y,
                   const gpx_kernel_spec* spec, int likelihood, double df, gpx_vgp** out);
int gpx_vgp_destroy(gpx_vgp* vgp);
int gpx_vgp_elbo_grad(gpx_vgp* vgp, const double* theta, const double* q_mu, const double* q_sqrt,
                      double* elbo, double* grad_theta, double* grad_qmu, double* grad_qsqrt,
                      int32_t* info, void* stream);
int gpx_vgp_predict(gpx_vgp* vgp, const double* theta, const double* q_mu, const double* q_sqrt,
                    const double* Xnew, int Mn, int predict_y, double* mean, double* var,
                    int32_t* info, void* stream);

/* ---------------------------------------------------------------------------------------
 * Host helpers of the batched L-BFGS-B driver (no device work): for the n_fits fits of one
 * round, u [n_fits, n_vars] are the unconstrained variables (gpflow.optimizers.Scipy's x,
 * GPR/model_trainer.py:18-19), rows [n_fits] their batch slots, cols [n_vars] the θ index of each
 * variable, lower [n_vars] its Shift (1e-6 for the Gaussian likelihood variance, else 0).
 *   gpx_host_theta_rows   theta[rows[k]][cols[v]] = lower[v] + softplus(u[k][v])
 *   gpx_host_loss_grad_u  loss[k] = −lml[rows[k]];
 *                         grad_u[k][v] = −grad[rows[k]][cols[v]] · sigmoid(u[k][v])
 * theta / grad rows have GPX_THETA_STRIDE entries (gpx_batch_lml_grad's layout).
 */
int gpx_host_theta_rows(int n_fits, int n_vars, const double* u, const int32_t* rows,
                        const int32_t* cols, const double* lower, double* theta);
int gpx_host_loss_grad_u(int n_fits, int n_vars, const double* u, const int32_t* rows,
                         const int32_t* cols, const double* lml, const double* grad, double* loss,
                         double* grad_u);
/* The same with a transform code per variable, tcode [n_vars]: 0 = softplus + Shift as above,
 * 1 = identity (θ = u, ∂θ/∂u = 1: the mean-function coefficients; lower[v] is ignored). */
int gpx_host_theta_rows_t(int n_fits, int n_vars, const double* u, const int32_t* rows,
                          const int32_t* cols, const double* lower, const int32_t* tcode, double* theta);
int gpx_host_loss_grad_u_t(int n_fits, int n_vars, const double* u, const int32_t* rows,
                           const int32_t* cols, const int32_t* tcode, const double* lml, const double* grad,
                           double* loss, double* grad_u);

#ifdef __cplusplus
}
#endif
#endif /* GPX_H_ */
