/*
 * nnest_hip.h -- C ABI of libnnest_hip.so: the MI355X (gfx950) implementation of the nnest
 * flow-transform + batched-proposal + likelihood + flow-training hot path.
 *
 * The reference (adammoss/nnest v0.4.2) is pure Python and has no FFI; the seam it offers is
 * constructor injection of a Trainer-shaped object (nnest/sampler.py:50, :196-212;
 * nnest/nested.py:44, :83).  Each entry point below names the reference function it replaces
 * (paths relative to the reference root).  INTEGRATION.md shows the ctypes binding a reference
 * maintainer would add.
 *
 * Conventions
 *   - all pointers named *_dev are DEVICE pointers (e.g. torch tensor .data_ptr()); the caller owns
 *     every buffer; rows are row-major [N, D] float32 unless stated
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every call is asynchronous
 *     on that stream unless documented otherwise; nothing here calls hipDeviceSynchronize
 *   - return value: 0 = ok, non-zero = error (NNEST_E_*); message via nnest_hip_last_error();
 *     nothing throws across the ABI
 *   - packed weights are float32 in torch state_dict order: per block,
 *     scale_net {W[H,D] b[H] (W[H,H] b[H])xL W[D,H] b[D]} then translate_net (same shapes)
 */
#ifndef NNEST_HIP_H
#define NNEST_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NNEST_HIP_ABI_VERSION 15

enum {
    NNEST_OK = 0,
    NNEST_E_ARG = 1,         /* bad argument / unsupported configuration */
    NNEST_E_HIP = 2,         /* HIP runtime error */
    NNEST_E_UNSUPPORTED = 3, /* shape outside what the kernels are instantiated for */
};

/* likelihood ids for the fused kernels (nnest/likelihoods.py) */
enum {
    NNEST_LIKE_ROSENBROCK = 0, /* Rosenbrock.loglike   likelihoods.py:51 */
    NNEST_LIKE_GAUSSMIX = 1,   /* GaussianMix.loglike  likelihoods.py:165-189 (sep 4, sigma 1, w .4 .3 .2 .1) */
    NNEST_LIKE_HIMMELBLAU = 2, /* Himmelblau.loglike   likelihoods.py:70 (D>2: sum over consecutive pairs) */
    NNEST_LIKE_GAUSSIAN = 3,   /* Gaussian.loglike     likelihoods.py:77-94  params[0] = corr (equicorrelated covariance) */
    NNEST_LIKE_EGGBOX = 4,     /* Eggbox.loglike       likelihoods.py:97-110 (x_dim = 2) */
    NNEST_LIKE_SHELL = 5,      /* GaussianShell        likelihoods.py:113-132 params = sigma, rshell, center */
    NNEST_LIKE_DOUBLE_SHELL = 6, /* DoubleGaussianShell likelihoods.py:135-150 params = sigma1, rshell1, center1,
                                    sigma2, rshell2, center2 (weights 1, 1) */
    NNEST_LIKE_COUNT = 7
};

/* which analytic likelihood the fused kernels evaluate, and on what: logl = loglike(scale * x)
 * (the reference's transform = lambda x: scale * x, examples/nested/run.py:25-42).  Host struct. */
typedef struct {
    int id;          /* NNEST_LIKE_* */
    float scale;
    float params[6]; /* per-likelihood parameters, see the enum; unused entries ignored */
} nnest_like_t;

/* flags for nnest_mh_constrained_steps */
enum {
    NNEST_MH_DYNAMIC_STEP = 1, /* sampler.py:422-431 step-size adaptation applied per group of 16 walkers (one wave): equals
                                * the reference's rule for batches of <= 16 chains, shard-invariant, no cross-workgroup
                                * traffic */
    NNEST_MH_UNCONSTRAINED = 2, /* loglstar = None (sampler.py:371-410): plain Metropolis with the likelihood and the box
                                 * prior in the ratio, min(1, exp(dlogdet + dlogl)); `loglstar` is ignored and every
                                 * proposal counts as one likelihood call */
    NNEST_MH_DYNAMIC_BATCH = 4, /* sampler.py:422-431 over ALL C walkers of the launch, as the reference applies it: every
                                 * workgroup posts its accepted count per step to `sync_dev`; the scale used from step
                                 * s + 1 + lag on reflects the batch-wide count of step s.  lag = flags bits 8..11
                                 * (NNEST_MH_LAG): 0 is the reference's rule exactly (a grid-wide wait per step), lag >= 1
                                 * takes the wait off the step's critical path (the counts are requested one step ahead).
                                 * Needs every workgroup resident: NNEST_E_UNSUPPORTED beyond ~16 walkers x 8 x CUs */
};
#define NNEST_MH_LAG(n) (((n) & 15) << 8)
/* flags bits 29 / 30: sync_dev is one half of a double buffer whose other half lies BEHIND it (bit 29) / IN FRONT of it (bit 30),
 * nnest_mh_sync_words(steps) words away, and the launch zeroes that other half for the next launch (see sync_dev below) */
#define NNEST_MH_SYNC_ZERO_NEXT (1 << 29)
#define NNEST_MH_SYNC_ZERO_PREV (1 << 30)
/* flags bits 20..27, with NNEST_MH_DYNAMIC_BATCH and lag >= 1: the first n steps of the launch apply the rule EXACTLY (lag 0, a
 * grid-wide wait on each of them) and only the steps after them run `lag` behind: votes 1..n are applied as the reference
 * applies them, the votes of the steps s > n from step s + 1 + lag on.  The rule's gain is 1 / (1 + votes) and every launch
 * starts from the caller's step_size, so the early votes are the ones that move the scale.  Kernel forms that do not implement
 * it return NNEST_E_UNSUPPORTED (nnest_mh_form_for tells). */
#define NNEST_MH_WARM(n) (((n) & 255) << 20)
/* flags bits 16..19: pin the kernel form (0 = by population).  A caller that shards ONE batch over ranks pins the form the
 * whole batch would get, so that a shard reproduces the slice of the unsharded run bit for bit. */
enum { NNEST_MH_FORM_AUTO = 0, NNEST_MH_FORM_IMAGE = 1, NNEST_MH_FORM_REG = 2, NNEST_MH_FORM_TEAM = 3, NNEST_MH_FORM_QUAD = 4,
       NNEST_MH_FORM_QUAD1 = 5, /* the quad tile with both nets on one wave (same bits as QUAD; A/B diagnostic) */
       NNEST_MH_FORM_SOLO = 6   /* one walker per wave, layers as v_fmac_f32 + DPP row rotations (nnest_solo.hip): <= 4 walkers per CU,
                                 * x_dim <= 128 (beyond 64 with the weights in LDS), fixed step or the batch-wide rule at lag >= 3 or at lag 0
                                 * (round 5: the reference's rule itself, every step an exact step) */ };
#define NNEST_MH_FORM(f) (((f) & 15) << 16)

typedef struct nnest_nvp nnest_nvp_t; /* opaque: RealNVP coupling stack + Adam state on one device */

int nnest_hip_version(void);
const char *nnest_hip_last_error(void);
/* number of compute units / device name of the current device (diagnostics for bench.py) */
int nnest_hip_device_info(int *num_cu, int *clock_khz, char *name, int name_len);

/* SingleSpeedNVP(num_inputs=D, num_hidden=H, num_blocks=B, num_layers=L) -- networks.py:328-347.
 * Allocates device storage for the packed weights, Adam moments and the MFMA-fragment image. */
int nnest_nvp_create(int D, int H, int B, int L, nnest_nvp_t **out);
/* SingleSpeedNVP(..., scale=) -- networks.py:328-347: '' (full affine coupling), 'translate'
 * (CouplingLayer(translate_only=True), networks.py:293-294, :304-305) or 'constant' (translate-only couplings, each
 * followed by a ScaleLayer, networks.py:312-325: y = x e^s, logdet += s).
 * Packed layout for every mode: the B blocks as for '' (scale_net then translate_net); with 'translate' and
 * 'constant' the scale_net slots are unused -- forced to zero on load, never given a gradient -- and with
 * 'constant' the B ScaleLayer scalars follow the blocks (nnest_nvp_num_params counts them). */
enum { NNEST_SCALE_AFFINE = 0, NNEST_SCALE_TRANSLATE = 1, NNEST_SCALE_CONSTANT = 2 };
int nnest_nvp_create_scaled(int D, int H, int B, int L, int scale_mode, nnest_nvp_t **out);
/* Masked autoregressive flow (named by BASELINE config 5).  ABSENT FROM THE REFERENCE (nnest/trainer.py:83-100
 * dispatches 'choleksy' / 'nvp' / 'spline' only): build-defined, DESIGN.md 3c -- B blocks of two MADE-masked nets with the
 * shapes of the coupling nets (so the packed vector has the SingleSpeedNVP layout and size), dimension order reversed between
 * blocks; forward (x -> z, the density / training direction) is one pass, inverse (z -> x, sampling and the Metropolis
 * proposals) runs group by group (nnest_maf_num_groups passes per block, at most hidden_dim + 1).  The handle is an
 * nnest_nvp_t: every nnest_nvp_* entry point (weights, Adam state, forward / inverse / log_probs / inverse_loglike, loss_grad,
 * adam_step) and nnest_mh_constrained_steps accept it; nnest_nvp_train and nnest_nvp_vjp return NNEST_E_UNSUPPORTED (the epoch
 * loop of this flow is driven from the host).  hidden_dim 16, x_dim 2..128. */
int nnest_maf_create(int D, int H, int B, int L, nnest_nvp_t **out);
int nnest_maf_num_groups(const nnest_nvp_t *maf);
int nnest_nvp_destroy(nnest_nvp_t *nvp);
int nnest_nvp_num_params(const nnest_nvp_t *nvp);
/* Base distribution of the flow (NormalizingFlowModel(prior=...), networks.py:47-59; Trainer(base_dist=...), trainer.py:41):
 * beta = 0 (default) is MultivariateNormal(0, I); beta > 0 is the reference's GeneralisedNormal(loc 0, scale 1, beta)
 * (nnest/distributions/generalised_normal.py:66-71; examples/nested/run.py --base_dist gen_normal --beta 8).  It enters
 * log_probs and therefore the training loss; forward / inverse and the proposal kernel do not depend on it. */
int nnest_nvp_set_base(nnest_nvp_t *nvp, float beta);
/* netG.load_state_dict / state_dict (trainer.py:102-106, :241): host<->device copy of the packed
 * weights.  These two synchronise `stream` before returning. */
int nnest_nvp_load_weights(nnest_nvp_t *nvp, const float *packed_host, void *stream);
int nnest_nvp_store_weights(nnest_nvp_t *nvp, float *packed_host, void *stream);
/* device pointer of the packed weights / Adam exp_avg / exp_avg_sq (read-only views for tests) */
int nnest_nvp_device_ptrs(nnest_nvp_t *nvp, float **w_dev, float **m_dev, float **v_dev);
/* host copies of Adam's exp_avg / exp_avg_sq (torch.optim.Adam state, trainer.py:121-122); synchronises `stream` */
int nnest_nvp_store_adam(nnest_nvp_t *nvp, float *exp_avg_host, float *exp_avg_sq_host, void *stream);
int nnest_nvp_load_adam(nnest_nvp_t *nvp, const float *exp_avg_host, const float *exp_avg_sq_host, void *stream);
/* Adam step counter and optimiser reset (torch.optim.Adam state, trainer.py:121-122) */
int nnest_nvp_adam_state(nnest_nvp_t *nvp, int *step_count, int set_step, int reset_moments, void *stream);

/* NormalizingFlow.forward (networks.py:24-32) via Trainer.forward (trainer.py:247-257): x -> z, logdet */
int nnest_nvp_forward(nnest_nvp_t *nvp, const float *x_dev, float *z_dev, float *logdet_dev, int N, void *stream);
/* NormalizingFlow.inverse (networks.py:34-42) via Trainer.inverse (trainer.py:259-269): z -> x, logdet */
int nnest_nvp_inverse(nnest_nvp_t *nvp, const float *z_dev, float *x_dev, float *logdet_dev, int N, void *stream);
/* NormalizingFlowModel.log_probs (networks.py:71-76), N(0,I) base (networks.py:51-57) */
int nnest_nvp_log_probs(nnest_nvp_t *nvp, const float *x_dev, float *logp_dev, int N, void *stream);

/* Fused "one eval": x = f^-1(z), logdet; box prior UniformPrior(-1,1) (priors.py:39-43);
 * logl = loglike(like->scale * x) as safe_loglike (sampler.py:110-133) incl. non-finite -> -1e100.
 * logl_dev is float64 [N]; inbox_dev int32 [N] (1 = inside the box).  x_dev/logdet_dev may be NULL. */
int nnest_nvp_inverse_loglike(nnest_nvp_t *nvp, const nnest_like_t *like, const float *z_dev, float *x_dev,
                              float *logdet_dev, double *logl_dev, int *inbox_dev, int N, void *stream);

/* Likelihood.__call__ over rows (likelihoods.py:14-22) through safe_loglike: logl[n] = loglike(like->scale*x[n]).
 * x_unit_dev float32 [N,D]; logl_dev float64 [N]. */
int nnest_loglike(const nnest_like_t *like, const float *x_unit_dev, double *logl_dev, int N, int D,
                  void *stream);

/* Sampler._mcmc_sample, hard-constraint branch (sampler.py:229-463), `steps` Metropolis steps for C
 * walkers inside ONE launch.
 *   z_dev [C,D]        in: latent start (= forward(init_samples), sampler.py:264); out: final latent
 *   x_dev [C,D]        out: final x = f^-1(z) (sampler.py:266, :439)
 *   logl_dev [C] f64   in: init_loglikes; out: final log-likelihoods
 *   loglstar           hard constraint logl > loglstar (sampler.py:361)
 *   step_size          initial proposal scale (sampler.py:255)
 *   noise_dz_dev       NULL -> in-kernel noise: every (walker, lane group) and every walker's uniform draw runs a
 *                      xoshiro128++ stream (add / xor / rotate: full-rate VALU) SEEDED by one Philox4x32-10 block keyed by
 *                      (seed; walker_offset + walker, lane group, stream), the normals by Box-Muller -- so a walker's draws
 *                      depend on (seed, its global index) only and a sharded batch draws what the unsharded one draws
 *                      (csrc/flow_tile.h "proposal stream of the persistent MH kernel"; nnest_mh_fill_noise replays them);
 *                      else recorded noise [steps, C, D] (torch.randn_like(z), sampler.py:310)
 *   noise_u_dev        recorded uniforms [steps, C] (torch.rand, sampler.py:334); required iff noise_dz_dev
 *   hist_x_dev         optional [C, steps+1, D] history of x (reference return layout, sampler.py:455);
 *   hist_logl_dev      optional [C, steps+1] f64
 *   n_accept_dev [C]   out int32: accepted moves per walker  (sampler.py:418-420) in bits 0..29; bit 30 (NNEST_MH_ALL_MOVED) is set
 *                      when EVERY coordinate of the chain's last x differs from its first x = f^-1(z_0) -- the reference's test
 *                      of a chain before its end may replace a live point (nested.py:432: np.all(samples[:,0] != samples[:,-1]));
 *                      evaluated against the first x the launch computed -- in-kernel by the solo and quad forms (the first x
 *                      parked in x_dev meanwhile), by a follow-up kernel on the launch's stream for the 16-walker-tile forms
 *                      and the spline / MAF flows (the first x in a side buffer of the library); x_dev NULL: the bit says
 *                      "accepted at least once"
 *   n_call_dev [C]     out int32: likelihood calls per walker (rows that passed the prior/Jacobian test,
 *                      sampler.py:358-363)
 *   scale_out_dev      optional float32 [ngroups]: final scale per adaptation group (sampler.py:422-431)
 *   sync_dev           NNEST_MH_DYNAMIC_BATCH only (else NULL): nnest_mh_sync_words(steps) 8-byte words, ZERO at the launch;
 *                      the last word is an error flag (non-zero: a bounded wait ran out).  Either the caller zeroes them in
 *                      front of every launch, or it keeps a double buffer of 2 x nnest_mh_sync_words(steps) words, zeroes it
 *                      once, passes the halves alternately and sets NNEST_MH_SYNC_ZERO_NEXT (the other half lies behind
 *                      sync_dev) or NNEST_MH_SYNC_ZERO_PREV (in front of it): the launch then zeroes the other half for the
 *                      next one (the solo form in-kernel, on spare waves: no fill launch in front of a K4 launch)
 */
int nnest_mh_constrained_steps(nnest_nvp_t *nvp, const nnest_like_t *like, float *z_dev, float *x_dev,
                               double *logl_dev, double loglstar, float step_size, int steps, int C, int flags,
                               const float *noise_dz_dev, const float *noise_u_dev, uint64_t seed,
                               uint64_t walker_offset, float *hist_x_dev, double *hist_logl_dev, int *n_accept_dev,
                               int *n_call_dev, float *scale_out_dev, void *sync_dev, void *stream);
/* The kernel form (NNEST_MH_FORM_*, never AUTO) nnest_mh_constrained_steps runs for C walkers under `flags` (in-kernel noise, no
 * history): the pinned form of flags bits 16..19 if it applies to this flow shape, population and step rule, the form chosen
 * by population otherwise; -1 if the launch would be refused (NNEST_E_UNSUPPORTED).  A caller that shards one batch of C_total
 * walkers over ranks asks with C = C_total and pins the answer on every shard (reference: the MPI scatter of one batch,
 * nnest/nested.py:405-427, has no such choice -- every rank runs the same Python). */
int nnest_mh_form_for(const nnest_nvp_t *nvp, int C, int flags);

/* SLICE proposal in latent space (BASELINE.json north_star: "the slice/MH proposal step in latent space").
 * ABSENT FROM THE REFERENCE: Sampler._mcmc_sample proposes Gaussian random-walk Metropolis moves only (nnest/sampler.py:310-316), so
 * this step is build-defined and its parity UNPINNED; it is held to a CPU restatement of the same definition
 * (oracle/oracle.py::slice_sample).  `steps` slice-sampling updates (Neal 2003: stepping out, shrinkage) of every walker along a
 * fresh random direction of latent space, of the target the reference's constrained Metropolis step leaves invariant
 * (sampler.py:326-361): density |det dx/dz| on {x(z) in the unit box, logL(x(z)) > loglstar}.  Per step: eps ~ N(0, I),
 * candidates z + t * width * eps; log y = log|det|(z) + log u1; bracket [-u0, 1 - u0], stepped out by 1 while the end lies in the
 * slice, left then right, within a budget of B = 2 max_stepout expansions in all.  If the slice's ends need more than B, the bracket
 * restarts at [-u0, 1 - u0] and B is split at random between the sides (Neal 2003, sec. 4.1): at most J = min(B, floor(u63 (B + 1)))
 * to the left, then at most B - J to the right.  (Separate caps per side are not reversible once they bind.)  max_stepout = 0: no
 * stepping out; 0..2^24.  Then up to max_shrink (1..60) shrinkage draws t = t_l + (t_r - t_l) u_k, k = 2, 3, ...
 * z_dev [C,D] and logl_dev [C]
 * are updated in place, x_dev [C,D] receives the chains' ends; n_call_dev [C]: candidates whose likelihood decided (inside the box and
 * above the slice level), n_move_dev [C]: steps that moved, with NNEST_MH_ALL_MOVED as in nnest_mh_constrained_steps, n_eval_dev [C]
 * (or NULL): evaluations of the flow.  noise_dz_dev [steps,C,D] replays recorded directions (NULL: in-kernel Philox, the draws
 * nnest_slice_fill_noise exports); the uniforms are Philox4x32-10 words of (seed, walker, 64 step + k), exact in float32.
 * hist_x_dev [C, steps + 1, D] or NULL.  One walker per wave, no cross-workgroup wait: any C.  Shapes: the reference's defaults
 * (hidden 16, 3 blocks, 1 layer, scale ''), x_dim <= 128; NNEST_E_UNSUPPORTED otherwise.  (Added within ABI 15.)
 * Every other flow (MAF, Cholesky, fast/slow, other NVP shapes) and every likelihood the kernels do not know (a host callable,
 * derived parameters, another prior) run the same definition through nnest_slice_rounds_* below; the spline flow has
 * nnest_spline_slice_steps. */
int nnest_slice_steps(nnest_nvp_t *nvp, const nnest_like_t *like, float *z_dev, float *x_dev, double *logl_dev, double loglstar,
                      float width, int steps, int C, int max_stepout, int max_shrink, const float *noise_dz_dev, uint64_t seed,
                      uint64_t walker_offset, float *hist_x_dev, int *n_call_dev, int *n_move_dev, int *n_eval_dev, void *stream);

/* SLICE proposal in ROUNDS, for any flow and any likelihood: the definition of nnest_slice_steps (directions, Philox uniforms, slice
 * level, bracket, step-out within the budget of 2 max_stepout expansions, shrinkage, counters, NNEST_MH_ALL_MOVED), with
 * each walker's state machine kept in a handle on the device
 * and the flow's inverse and the likelihood evaluated by the CALLER between the launches.  One round:
 *   z_cand --(caller: the flow's inverse entry point)--> x_cand, ld_cand
 *   nnest_slice_rounds_screen: box test (or the caller's prior flags) and slice level; the x_cand rows whose likelihood decides are
 *       packed into rows_dev in ascending walker order (their walkers in idx_dev); counts_dev = {packed rows, walkers whose candidate
 *       was live}.  counts[1] == 0: every walker has finished, nothing further is to be evaluated.
 *   caller: logl_rows[r] = logL(rows[r]) for r < counts[0] (float64, non-finite values as -1e100)
 *   nnest_slice_rounds_advance: consumes the decisions, steps every walker, writes the next candidates into z_cand_dev.
 * Walkers do not wait for each other: one that finishes an update starts its next in the next round, so a batch takes as many rounds
 * as its busiest walker has evaluations (+ one that finds none live).  Device pointers, one stream, return codes.
 *   create: state for C walkers of x_dim D and `steps` updates (device memory of the current device).
 *   begin: z_dev [C,D] and its x_dev = f^-1(z), ld_dev = log|det dx/dz| (float32), logl_dev [C] (float64) start the chains (read only);
 *       noise_dz_dev [steps,C,D] replays recorded directions (NULL: in-kernel Philox, what nnest_slice_fill_noise exports);
 *       hist_x_dev / hist_z_dev [C, steps + 1, D], hist_logl_dev [C, steps + 1]: the state after every update, or NULL;
 *       move_ref_dev [C, steps] or NULL: per update the packed row the walker moved to, counted over the rows of all rounds since
 *       begin (the row of round r is  rows before round r + its row), -1 if it stayed -- what a caller needs to pick the derived
 *       parameters it computed with a row; z_cand_dev [C,D] receives the first candidates.
 *   screen: x_cand_dev [C,D], ld_cand_dev [C]; inbox_dev [C] int or NULL (NULL: UniformPrior(D, -1, 1), NaN inside); rows_dev
 *       [C,D], idx_dev [C], counts_dev [2] int out.
 *   advance: rows_dev and logl_rows_dev [>= counts[0]] of this round; z_cand_dev [C,D] out.
 *   finish: z_dev, x_dev [C,D], logl_dev [C], n_call_dev, n_move_dev (with NNEST_MH_ALL_MOVED), n_eval_dev [C] out (each may be
 *       NULL); n_call counts the packed rows of the walker, n_eval its candidates.
 * (Added within ABI 15.) */
typedef struct nnest_slice_rounds nnest_slice_rounds_t;
int nnest_slice_rounds_create(int C, int D, int steps, nnest_slice_rounds_t **out);
int nnest_slice_rounds_destroy(nnest_slice_rounds_t *h);
int nnest_slice_rounds_begin(nnest_slice_rounds_t *h, const float *z_dev, const float *x_dev, const float *ld_dev, const double *logl_dev,
                             double loglstar, float width, int max_stepout, int max_shrink, const float *noise_dz_dev, uint64_t seed,
                             uint64_t walker_offset, float *hist_x_dev, float *hist_z_dev, double *hist_logl_dev, int *move_ref_dev,
                             float *z_cand_dev, void *stream);
int nnest_slice_rounds_screen(nnest_slice_rounds_t *h, const float *x_cand_dev, const float *ld_cand_dev, const int *inbox_dev,
                              float *rows_dev, int *idx_dev, int *counts_dev, void *stream);
int nnest_slice_rounds_advance(nnest_slice_rounds_t *h, const float *rows_dev, const double *logl_rows_dev, float *z_cand_dev, void *stream);
int nnest_slice_rounds_finish(nnest_slice_rounds_t *h, float *z_dev, float *x_dev, double *logl_dev, int *n_call_dev, int *n_move_dev,
                              int *n_eval_dev, void *stream);
int nnest_slice_fill_noise(float *dz_dev, int steps, int C, int D, uint64_t seed, uint64_t walker_offset, void *stream);

/* ENSEMBLE sampler: emcee 3's EnsembleSampler with its default StretchMove (RedBlueMove, a = 2, nsplits = 2, randomize_split = True)
 * in the latent space of the flow, as Sampler._ensemble_sample runs it through emcee (nnest/sampler.py:632-724).  BUILD-DEFINED
 * STREAM, EMCEE'S MOVE: the draws are this library's Philox4x32-10 words, so parity with emcee is statistical.  N = C walkers z_k in
 * R^D; step t (global index, 0-based; `step0` is the index of a launch's first step):
 *   1. split: inds = arange(N) % 2 shuffled by Fisher-Yates, i = N - 1 down to 1: swap inds[i], inds[j], j = (m (i + 1)) >> 24, m = the
 *      top 24 bits of word (i & 3) of Philox(key seed; counter (i >> 2, t, 0, 4 << 28)).  Set 0 = {k : inds[k] = 0}, set 1 the rest,
 *      each listed in ascending walker index.
 *   2. set 0 moves against the current positions of set 1, then set 1 against the updated set 0.  Walker k of the moving set:
 *      u1, u2, u3 = the top 24 bits of words 0, 1, 2 of Philox(key seed; counter (0, k, t, 3 << 28 | k >> 32)) / 2^24;
 *      zz = ((a - 1) u1 + 1)^2 / a;  j = member floor(u2 Nc) of the other set (Nc its size);  q = z_j - (z_j - z_k) zz  (float32,
 *      each operation rounded);  lnpdiff = (D - 1) log zz + lp(q) - lp(z_k) (float64);  the walker moves to q iff lnpdiff > log u3.
 *   lp(z) (transformed_loglike, sampler.py:674-689): x = f^-1(z), ld = log|det dx/dz|, T(x) = x * t_std + t_mean per dimension
 *      (float32), logL = safe_loglike(T(x)) (non-finite -> -1e100), prior = 0 if T(x) lies in the box [lo, hi] (NaN inside; no box:
 *      lo = hi = NULL), else -inf.  constrained = 0: lp = (logL + ld) + prior;  constrained = 1: lp = -inf if logL < loglstar, else
 *      ld + prior.
 * A run is a function of the seed: the split of step t depends on (seed, t) only, the uniforms on (seed, walker, t), so neither the
 * cut into launches nor the route changes it.  Callers refuse N < 2 D, as emcee does.  (All added within ABI 15.)
 *
 * work_dev: int32 scratch of nnest_ensemble_work_words(C, steps) words per launch (an error word, one step count per walker, the
 * split tables of the launch's steps); -1 if the size does not fit an int.
 * nnest_ensemble_fill_noise: writes the split of steps step0 .. step0 + steps - 1 into work_dev: inds [steps, C] int32 at word
 * offset nnest_ensemble_work_words(C, 0), then the sets' member lists [steps, C] (set 0 then set 1); u_dev [steps, C, 3] float32
 * (or NULL) receives u1, u2, u3.  The fused entry builds its own split; the round route calls this first.
 * nnest_ensemble_max_walkers: the population nnest_ensemble_steps takes for this flow and likelihood id: 4 walkers per workgroup
 * times the resident workgroups, min(occupancy API, 8, floor(800 / (SGPR granules + 16))) per CU; -1 if the flow's shape is not
 * the fused route's.
 * nnest_ensemble_steps: the FUSED route, `steps` steps in one launch, one walker per wave; the default NVP shape (hidden 16,
 *   3 blocks, 1 layer, scale ''), x_dim <= 128, a known likelihood id (like->scale is ignored: the likelihood sees T(x)).  Walkers
 *   hand positions to each other inside the launch, so every workgroup must be resident: C > nnest_ensemble_max_walkers is refused
 *   with NNEST_E_UNSUPPORTED.  z_in_dev [C,D] (read only; not z_out_dev), lp_in_dev [C] or NULL (evaluate lp(z_in)); z_out_dev,
 *   x_out_dev [C,D], lp_out_dev [C] the last state; hist_z_dev, hist_x_dev [C, steps, D], hist_lp_dev [C, steps] the state after
 *   every step (required: the hand-off channel); n_accept_dev [C] or NULL.  t_std_dev, t_mean_dev [D].  The call waits for the
 *   launch: a hand-off wait that runs out (~2 s) ends every wave and returns NNEST_E_HIP.
 * nnest_ensemble_rounds_propose / _accept: the ROUND route, any flow and any likelihood.  Per half-step (half 0 / 1) of chunk step i
 *   (global step step0 + i) the moving set has n0 = ceil(C/2) (half 0) or C - n0 (half 1) walkers; its rows are listed in ascending
 *   walker order.  propose: q_dev [rows, D] = the moving walkers' proposals from z_cur_dev [C,D].  The caller maps them: x, ld =
 *   f^-1(q) (any flow), logl = safe logL(T(x)) float64, and optionally lprior_dev [rows] float64 (the log prior of T(x); NULL: the box
 *   on T(x) from lo/hi, no prior if those are NULL too).  accept: the rule; z_cur_dev, x_cur_dev, lp_cur_dev [C] and the history
 *   rows of step i (hist_* as above) are updated, n_accept_dev [C] counts, acc_rows_dev [rows] (or NULL) flags the rows taken.
 *   half = -1 in accept is the initial evaluation: rows = all C walkers in order, q = their z; it sets z_cur, x_cur, lp_cur and
 *   zeroes n_accept. */
int nnest_ensemble_work_words(int C, int steps);
int nnest_ensemble_fill_noise(int *work_dev, float *u_dev, int C, int steps, uint64_t step0, uint64_t seed, void *stream);
int nnest_ensemble_max_walkers(nnest_nvp_t *nvp, int like_id);
int nnest_ensemble_steps(nnest_nvp_t *nvp, const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev, const float *lo_dev,
                         const float *hi_dev, const float *z_in_dev, const double *lp_in_dev, float *z_out_dev, float *x_out_dev,
                         double *lp_out_dev, float *hist_z_dev, float *hist_x_dev, double *hist_lp_dev, int *n_accept_dev, int *work_dev,
                         int C, int steps, uint64_t step0, uint64_t seed, int constrained, double loglstar, void *stream);
int nnest_ensemble_rounds_propose(const int *work_dev, int C, int steps, int D, int i, int half, uint64_t step0, uint64_t seed,
                                  const float *z_cur_dev, float *q_dev, void *stream);
int nnest_ensemble_rounds_accept(const int *work_dev, int C, int steps, int D, int i, int half, uint64_t step0, uint64_t seed,
                                 const float *q_dev, const float *x_dev, const float *ld_dev, const double *logl_dev,
                                 const double *lprior_dev, const float *t_std_dev, const float *t_mean_dev, const float *lo_dev,
                                 const float *hi_dev, float *z_cur_dev, float *x_cur_dev, double *lp_cur_dev, float *hist_z_dev,
                                 float *hist_x_dev, double *hist_lp_dev, int *n_accept_dev, int *acc_rows_dev, int constrained,
                                 double loglstar, void *stream);

/* The FUSED route through the NEURAL-SPLINE flow: the run above with f the spline flow (the split table, the Philox streams 3 and 4,
 * zz, the partner, q, lnpdiff, lp, T and the box are the ones above), `steps` steps in one launch.  (Added within ABI 15.)
 * Layout: 16 walkers per workgroup, four waves per tile (the team form of nnest_spline_mh_constrained_steps, and its shapes); a step
 * is two half-steps, each one evaluation of the tile: in half h the walkers of set h propose, the others evaluate their own point
 * and the result is discarded.
 * THE TWO-PUBLISH RULE: a tile holds walkers of both sets, so it publishes TWICE per step -- after half 0 the history rows and the
 * step counts (t + 1) of its set-0 walkers, after half 1 those of its set-1 walkers.  Half 1 of step t waits for set-0 partners at
 * count t + 1; with one publish at the end of a step two tiles could wait for each other.  With two, every wait points to an
 * earlier (step, half), partners in the same tile included, so the launch completes whenever every workgroup is resident.
 * nnest_spline_ensemble_max_walkers: the population nnest_spline_ensemble_steps takes: 16 walkers per workgroup times the resident
 *   workgroups by the formula of nnest_ensemble_max_walkers; -1 for a NULL handle, an unknown likelihood id or a shape the kernel
 *   is not instantiated for.
 * nnest_spline_ensemble_steps: the argument list, the argument checks, the residency refusal (C > max_walkers:
 *   NNEST_E_UNSUPPORTED; a grid that is not proven resident is never launched) and the bounded hand-off wait (NNEST_E_HIP) of
 *   nnest_ensemble_steps.  work_dev: nnest_ensemble_work_words; the draws: nnest_ensemble_fill_noise. */
struct nnest_spline;
int nnest_spline_ensemble_max_walkers(struct nnest_spline *spl, int like_id);
int nnest_spline_ensemble_steps(struct nnest_spline *spl, const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev,
                                const float *lo_dev, const float *hi_dev, const float *z_in_dev, const double *lp_in_dev, float *z_out_dev,
                                float *x_out_dev, double *lp_out_dev, float *hist_z_dev, float *hist_x_dev, double *hist_lp_dev,
                                int *n_accept_dev, int *work_dev, int C, int steps, uint64_t step0, uint64_t seed, int constrained,
                                double loglstar, void *stream);

/* The stretch move in X SPACE: the run above with f = identity and ld = 0, so the walkers are x_k and
 *   lp(x) = safe_loglike(T(x)) + prior (constrained = 1: -inf if logL < loglstar, else prior),
 * T the identity (t_std_dev = t_mean_dev = NULL) or x * t_std + t_mean, the prior the box on T(x) or none.  The split table, the
 * uniforms, zz, the partner, lnpdiff and the accept rule are the ones above on the same Philox streams, so the run is the one
 * the round entries compute with an identity map for the flow, and is a function of (seed, step) only.  It is the emcee run
 * EnsembleSampler.bootstrap starts from (nnest/ensemble.py:111-147).  (Added within ABI 15.)
 * nnest_ensemble_x_max_walkers: the resident population of nnest_ensemble_x_steps for x_dim D and this likelihood id, by the
 *   formula of nnest_ensemble_max_walkers applied to the x-space kernel (which has no LDS and few registers: 24 walkers per CU,
 *   the SGPR term); -1 for D outside 1..128, an unknown id or no device.
 * nnest_ensemble_x_steps: `steps` steps in one launch, one walker per wave, D <= 128 (NNEST_E_UNSUPPORTED beyond) and a known
 *   likelihood id.  x_in_dev [C,D] (read only; not x_out_dev), lp_in_dev [C] or NULL; x_out_dev [C,D], lp_out_dev [C] the last
 *   state, tx_out_dev [C,D] or NULL its T(x); hist_x_dev [C, steps, D], hist_lp_dev [C, steps] the state after every step
 *   (required: the hand-off channel); n_accept_dev [C] or NULL; work_dev as above.  The argument checks, the residency refusal
 *   (NNEST_E_UNSUPPORTED) and the bounded hand-off wait are those of nnest_ensemble_steps. */
int nnest_ensemble_x_max_walkers(int D, int like_id);
int nnest_ensemble_x_steps(const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev, const float *lo_dev, const float *hi_dev,
                           const float *x_in_dev, const double *lp_in_dev, float *x_out_dev, float *tx_out_dev, double *lp_out_dev,
                           float *hist_x_dev, double *hist_lp_dev, int *n_accept_dev, int *work_dev, int C, int D, int steps, uint64_t step0,
                           uint64_t seed, int constrained, double loglstar, void *stream);
/* MOVE MIXTURES: emcee's differential-evolution (DE) move beside the stretch move, one move chosen per step by weight, as
 * emcee 3.1's EnsembleSampler.sample does with a weighted list of moves (RedBlueMove, DEMove).  BUILD-DEFINED STREAM, EMCEE'S MOVE:
 * the definition below is RESTATED FROM EMCEE'S DOCUMENTED BEHAVIOUR (emcee is not available to check against); parity with emcee
 * is statistical.  (All added within ABI 15.)  The split, the halves, lp, u1 u2 u3 and the 24-bit conventions are those of
 * nnest_ensemble_steps above; in addition, at global step t:
 *   move of step t: every walker takes the same move in both halves.  m_t = the top 24 bits of word 0 of Philox(key seed; counter
 *      (0, t, 1, 4 << 28)) (the split draws from counter word 2 = 0 of that stream).  The step is a stretch step iff m_t < thr,
 *      thr = floor(p_stretch 2^24) in float64 from the normalised weights, p_stretch = w_stretch / (w_stretch + w_de): thr = 2^24
 *      is always the stretch move, 0 always the DE move.
 *   stretch step: as above, bit for bit.
 *   DE step, walker k of the moving set, Nc walkers in the other set (Nc >= 2, hence C >= 4: NNEST_E_ARG below):
 *      partner a = member ja = (m2 Nc) >> 24, the stretch partner's draw and rule;
 *      partner b = member jb = (mw (Nc - 1)) >> 24, then jb += (jb >= ja), mw the top 24 bits of word 3 of the walker's block: an
 *        ordered pair of distinct members;
 *      n = sqrt(-2 ln((mx + 1) / 2^24)) cos(2 pi my / 2^24) (float64), mx, my the top 24 bits of words 0, 1 of
 *        Philox(key seed; counter (1, k, t, 3 << 28 | k >> 32));
 *      gamma = (float)(g0 (1 + sigma n)) (float64 inside), g0 = de_gamma0 or 2.38 / sqrt(2 D) for 0, sigma = de_sigma or 1e-5 for 0
 *        (emcee's defaults);
 *      q = z_k + (z_b - z_a) gamma (float32, each operation rounded);  lnpdiff = lp(q) - lp(z_k) (float64, no factor);  the
 *        walker moves to q iff lnpdiff > log u3.
 * A run stays a function of the seed and the weights, not of its cut into launches or its route.  The snooker and KDE moves are not
 * built.
 * nnest_ens_moves_t: the weights (non-negative, finite, not both 0: NNEST_E_ARG otherwise) and the DE scale.  A NULL `moves` is the
 *   stretch move alone: nnest_ensemble_steps, _x_steps, _max_walkers, _x_max_walkers and _rounds_propose / _accept ARE the entries
 *   below with NULL.
 * nnest_ensemble_moves_threshold: thr of these weights; -1 if they are refused.
 * nnest_ensemble_moves_steps, nnest_ensemble_x_moves_steps: the fused entries above with one trailing `moves`.  A run with a DE step
 *   in it (thr < 2^24) launches a kernel instantiation of its own, which waits for two partners per DE step through the same
 *   hand-off, at the same step counts; its resident population is nnest_ensemble_moves_max_walkers / _x_moves_max_walkers (the same
 *   formula on that instantiation), beyond which the call is refused with NNEST_E_UNSUPPORTED.  thr = 2^24 runs the stretch move's
 *   own instantiation.
 * nnest_ensemble_rounds_moves_propose / _accept: the round entries above with one trailing `moves` (the same for both calls).
 * nnest_ensemble_fill_moves: the moves' draws of steps step0 .. step0 + steps - 1, through the kernels' own functions, for tests:
 *   move_dev [steps] int32 (0 stretch, 1 DE), b_dev [steps, C] int32 (jb after the shift: an index into the other set's member
 *   list) and gamma_dev [steps, C] float32, each or NULL.  work_dev: as nnest_ensemble_fill_noise wrote it for the same C, steps,
 *   step0 and seed (jb depends on the size of the walker's other set).  moves NULL: every step a stretch step, the default scale. */
typedef struct nnest_ens_moves {
    float w_stretch, w_de;        /* the weights of the stretch and the DE move */
    float de_gamma0, de_sigma;    /* the DE scale g0 and its relative spread sigma; 0: emcee's defaults */
} nnest_ens_moves_t;
int nnest_ensemble_moves_threshold(const nnest_ens_moves_t *moves);
int nnest_ensemble_moves_max_walkers(nnest_nvp_t *nvp, int like_id, const nnest_ens_moves_t *moves);
int nnest_ensemble_x_moves_max_walkers(int D, int like_id, const nnest_ens_moves_t *moves);
int nnest_ensemble_moves_steps(nnest_nvp_t *nvp, const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev,
                               const float *lo_dev, const float *hi_dev, const float *z_in_dev, const double *lp_in_dev, float *z_out_dev,
                               float *x_out_dev, double *lp_out_dev, float *hist_z_dev, float *hist_x_dev, double *hist_lp_dev,
                               int *n_accept_dev, int *work_dev, int C, int steps, uint64_t step0, uint64_t seed, int constrained,
                               double loglstar, void *stream, const nnest_ens_moves_t *moves);
int nnest_ensemble_x_moves_steps(const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev, const float *lo_dev,
                                 const float *hi_dev, const float *x_in_dev, const double *lp_in_dev, float *x_out_dev, float *tx_out_dev,
                                 double *lp_out_dev, float *hist_x_dev, double *hist_lp_dev, int *n_accept_dev, int *work_dev, int C, int D,
                                 int steps, uint64_t step0, uint64_t seed, int constrained, double loglstar, void *stream,
                                 const nnest_ens_moves_t *moves);
int nnest_ensemble_rounds_moves_propose(const int *work_dev, int C, int steps, int D, int i, int half, uint64_t step0, uint64_t seed,
                                        const float *z_cur_dev, float *q_dev, void *stream, const nnest_ens_moves_t *moves);
int nnest_ensemble_rounds_moves_accept(const int *work_dev, int C, int steps, int D, int i, int half, uint64_t step0, uint64_t seed,
                                       const float *q_dev, const float *x_dev, const float *ld_dev, const double *logl_dev,
                                       const double *lprior_dev, const float *t_std_dev, const float *t_mean_dev, const float *lo_dev,
                                       const float *hi_dev, float *z_cur_dev, float *x_cur_dev, double *lp_cur_dev, float *hist_z_dev,
                                       float *hist_x_dev, double *hist_lp_dev, int *n_accept_dev, int *acc_rows_dev, int constrained,
                                       double loglstar, void *stream, const nnest_ens_moves_t *moves);
int nnest_ensemble_fill_moves(const int *work_dev, int *move_dev, int *b_dev, float *gamma_dev, int C, int D, int steps, uint64_t step0,
                              uint64_t seed, const nnest_ens_moves_t *moves, void *stream);

/* RANDOM-WALK METROPOLIS in the latent space of the flow with the likelihood, the prior and the Jacobian in the ratio: MCMCSampler's
 * run, Sampler._mcmc_sample with loglstar = None (nnest/mcmc.py:79-126, nnest/sampler.py:372-416), every step of a launch inside the
 * kernel.  BUILD-DEFINED STREAM, THE REFERENCE'S MOVE: the draws are this library's Philox4x32-10 words, so parity with torch's
 * stream is statistical.  C walkers z_k in R^D; step t (global index, 0-based; `step0` is the index of a launch's first step); the
 * global walker index is w = walker_offset + k:
 *   normals:  eps[4g .. 4g+3] = the four Box-Muller normals of Philox(key seed; counter (g, w, t, 5 << 28 | w >> 32)), with the
 *             arithmetic of the slice proposal's directions (float32: u = r 2^-32 + 2^-33, sqrt(-2 ln u), sin / cos in revolutions);
 *   uniform:  u = the top 24 bits of word 0 of Philox(key seed; counter (0, w, t, 6 << 28 | w >> 32)) / 2^24;
 *   proposal: q = z_k + step_size * eps (float32, each operation rounded);
 *   accept:   the walker moves to q iff lp(q) - lp(z_k) > log u (float64), lp the target of nnest_ensemble_steps at constrained = 0:
 *             x = f^-1(z), T(x) = x * t_std + t_mean, logL = safe_loglike(T(x)), lp = (logL + log|det dx/dz|) + prior, the prior 0 in
 *             the box [lo, hi] on T(x) (NaN inside) and -inf outside;
 *   logged:   the walker carries logL(T(x)) (float64) beside lp: the reference returns logL in `loglikes`.
 * A run is a function of (seed, global walker index, global step) only: neither the cut into launches, nor the kernel layout, nor
 * a shard of the population (walker_offset) changes it.  Walkers are independent: there is no hand-off, no residency limit and no
 * work buffer, and the calls are asynchronous on `stream`.  Only this unconstrained target is built (the hard constraint is
 * nnest_mh_constrained_steps's); the step is fixed.  (All added within ABI 15.)
 * nnest_mcmc_steps: the default NVP shape (hidden 16, 3 blocks, 1 layer, scale ''), x_dim <= 128, a known likelihood id
 *   (like->scale is ignored: the likelihood sees T(x)); other shapes: NNEST_E_UNSUPPORTED.  Any C >= 1: one walker per wave,
 *   ceil(C / 4) workgroups.  z_in_dev [C,D]; lp_in_dev, logl_in_dev [C]: both (the start's lp and logL, as a previous launch returned
 *   them) or both NULL (evaluated); z_out_dev, x_out_dev [C,D], lp_out_dev, logl_out_dev [C]: the last state (z_out_dev may be
 *   z_in_dev); hist_z_dev, hist_x_dev [C, steps, D], hist_logl_dev [C, steps]: the state after every step, all three or all NULL
 *   (the ends only); n_accept_dev [C] or NULL.  t_std_dev, t_mean_dev [D], both or both NULL (T = identity); lo_dev, hi_dev [D], both
 *   or both NULL (no prior).  steps = 0 evaluates the start: x_out_dev, lp_out_dev and logl_out_dev are written, nothing else is
 *   (z_out_dev may then be NULL).
 * nnest_spline_mcmc_steps: the same run through the neural-spline flow, on the team tile of nnest_spline_ensemble_steps and its
 *   shapes: 16 walkers per workgroup, four waves; a step is ONE evaluation of the tile in which every live row proposes (rows >= C
 *   evaluate their own point, and the result is discarded); the four waves take bit-identical decisions.
 * nnest_mcmc_fill_noise: the draws above as arrays, through the kernels' own functions: dz_dev [steps, C, D] float32 (eps) and u_dev
 *   [steps, C] float32, either or NULL, for steps step0 .. step0 + steps - 1 and walkers walker_offset .. walker_offset + C - 1. */
int nnest_mcmc_steps(nnest_nvp_t *nvp, const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev, const float *lo_dev,
                     const float *hi_dev, const float *z_in_dev, const double *lp_in_dev, const double *logl_in_dev, float *z_out_dev,
                     float *x_out_dev, double *lp_out_dev, double *logl_out_dev, float *hist_z_dev, float *hist_x_dev,
                     double *hist_logl_dev, int *n_accept_dev, int C, int steps, float step_size, uint64_t step0, uint64_t seed,
                     uint64_t walker_offset, void *stream);
int nnest_spline_mcmc_steps(struct nnest_spline *spl, const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev,
                            const float *lo_dev, const float *hi_dev, const float *z_in_dev, const double *lp_in_dev,
                            const double *logl_in_dev, float *z_out_dev, float *x_out_dev, double *lp_out_dev, double *logl_out_dev,
                            float *hist_z_dev, float *hist_x_dev, double *hist_logl_dev, int *n_accept_dev, int C, int steps,
                            float step_size, uint64_t step0, uint64_t seed, uint64_t walker_offset, void *stream);
int nnest_mcmc_fill_noise(float *dz_dev, float *u_dev, int steps, int C, int D, uint64_t step0, uint64_t seed, uint64_t walker_offset,
                          void *stream);
/* THE TEMPERED TARGET of the same run, and the two service kernels of a SEQUENTIAL MONTE CARLO sampler built on it (SMCSampler,
 * nnest_amd/smc.py).  BUILD-DEFINED: the reference has no such sampler.  The sampler anneals L^beta pi from beta = 0
 * (the prior, sampled exactly) to beta = 1; between two temperatures it reweights, resamples, retrains the flow and moves the
 * particles with Metropolis steps in the flow's latent space.  (All added within ABI 15.)
 * nnest_mcmc_tempered_steps, nnest_spline_mcmc_tempered_steps: nnest_mcmc_steps / nnest_spline_mcmc_steps with the likelihood to the
 *   power `beta` -- the arguments of their siblings plus `double beta` before `stream`.  Everything said of nnest_mcmc_steps holds, with
 *     lp_beta(z) = ((beta * logL) + log|det dx/dz|) + prior,
 *   float64, each operation rounded; logL is the safe value (-1e100 for non-finite).  lp_in_dev, lp_out_dev and the accept rule use
 *   lp_beta; the walker still carries and logs the UNTEMPERED logL (logl_in_dev, logl_out_dev, hist_logl_dev).  The draws are the
 *   same (streams 5 and 6), and so are the invariances: the cut into launches, a shard by walker_offset; steps = 0 evaluates the
 *   start.  beta must be finite and >= 0, else NNEST_E_ARG before any launch, the outputs untouched; beta = 0 is valid: the prior and
 *   the Jacobian alone.  beta = 1.0 is bit-identical to the untempered entry (1.0 * logL is exact) on every output.  The tempering is
 *   a compile-time variant of the two kernels: the untempered entries run the code they ran before.
 * nnest_smc_reweight: the next temperature and the weights that lead there.  logl_dev [N] float64 (safe values), 1 <= N <= 2^20;
 *   beta in [0, 1): the population's temperature; ess_fraction in (0, 1).  With w_i(b) = exp((b - beta) (logL_i - max logL)) and
 *   ESS(b) = (sum w)^2 / sum w^2:  if ESS(1) >= ess_fraction * N then beta' = 1;  otherwise 64 bisection steps on [lo, hi] = [beta, 1]:
 *   mid = 0.5 * (lo + hi); ESS(mid) < ess_fraction * N ? hi = mid : lo = mid; beta' = hi, and where that does not exceed beta in
 *   float64, beta' = 1: the ladder always advances.  out_dev [4] float64 = {beta', log((1/N) sum_i exp((beta' - beta) logL_i))
 *   computed as (beta' - beta) max logL + log(sum w / N), ESS(beta'), max logL}.  m_dev [N] int64: m_i = floor(w_i(beta') * 2^31),
 *   INTEGER weights (0 .. 2^31): their sums do not depend on the order of a scan.  One workgroup; every reduction float64 in a fixed
 *   order, no floating-point atomics: the same call twice returns the same bits.  Asynchronous on `stream`.  NNEST_E_ARG before any
 *   launch: N outside 1 .. 2^20, ess_fraction outside (0, 1) (NaN included), beta outside [0, 1), a NULL buffer.
 * nnest_smc_resample: systematic resampling on the integer weights m_dev [N] int64 (>= 0).  T = sum m;
 *     u = the top 24 bits of word 0 of Philox(key seed; counter (0, stage, 0, 8 << 28)) / 2^24 (stream 8; streams 0-7 are taken);
 *     p_j = floor(((j + u) * (double)T) / N), float64, each operation rounded (every operand is exact);
 *     anc_j = the smallest i whose inclusive prefix sum of m exceeds p_j;
 *   row j of theta_out_dev [N, D] float32 and of logl_out_dev [N] float64 is row anc_j of theta_in_dev and logl_in_dev, and
 *   anc_out_dev [N] int32 holds anc_j (non-decreasing in j).  The outputs must not be the inputs.  stage >= 0, D >= 1.  One workgroup.
 *   The call returns after the kernel has finished (it reads the kernel's verdict back): T = 0, or a negative weight, is NNEST_E_ARG
 *   with theta_out_dev and logl_out_dev unwritten (anc_out_dev[0] = -1). */
int nnest_mcmc_tempered_steps(nnest_nvp_t *nvp, const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev, const float *lo_dev,
                              const float *hi_dev, const float *z_in_dev, const double *lp_in_dev, const double *logl_in_dev,
                              float *z_out_dev, float *x_out_dev, double *lp_out_dev, double *logl_out_dev, float *hist_z_dev,
                              float *hist_x_dev, double *hist_logl_dev, int *n_accept_dev, int C, int steps, float step_size,
                              uint64_t step0, uint64_t seed, uint64_t walker_offset, double beta, void *stream);
int nnest_spline_mcmc_tempered_steps(struct nnest_spline *spl, const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev,
                                     const float *lo_dev, const float *hi_dev, const float *z_in_dev, const double *lp_in_dev,
                                     const double *logl_in_dev, float *z_out_dev, float *x_out_dev, double *lp_out_dev,
                                     double *logl_out_dev, float *hist_z_dev, float *hist_x_dev, double *hist_logl_dev, int *n_accept_dev,
                                     int C, int steps, float step_size, uint64_t step0, uint64_t seed, uint64_t walker_offset, double beta,
                                     void *stream);
int nnest_smc_reweight(const double *logl_dev, int N, double beta, double ess_fraction, double *out_dev, long long *m_dev, void *stream);
int nnest_smc_resample(const long long *m_dev, int N, int D, uint64_t seed, int stage, const float *theta_in_dev, const double *logl_in_dev,
                       int *anc_out_dev, float *theta_out_dev, double *logl_out_dev, void *stream);
/* THE MIXED WALK: the tempered random-walk Metropolis run above with a flow-INDEPENDENCE ("global") step at every global_every-th
 * step, in kernels of their own (nnest_mcmc_mixed.hip, nnest_spline_mcmc_mixed.hip).  BUILD-DEFINED: the reference
 * has no such step.  A global step proposes a draw of the flow's base mapped through the flow -- the trained flow as a PROPOSAL, not
 * only as a preconditioner -- and accepts on the ratio of importance weights: it lets a chain jump between modes the flow has learnt
 * and decorrelates the duplicated particles behind an SMC resampling.  (All added within ABI 15.)
 * nnest_mcmc_mixed_steps, nnest_spline_mcmc_mixed_steps: the arguments of nnest_mcmc_tempered_steps / nnest_spline_mcmc_tempered_steps
 *   plus `int global_every` and `int *n_accept_global_dev` before `stream`.  A launch advances C walkers by `steps` steps; step t is a
 *   global index (step0 + the step's number within the launch, as the 32-bit index the draws use); w = walker_offset + row.  With
 *   k = global_every:
 *     kind:    step t is GLOBAL iff k > 0 and (t + 1) % k == 0, for all walkers alike (k = 1: every step; k = 10: steps 9, 19, ...);
 *              LOCAL otherwise.
 *     draws:   eps = the normals and u = the uniform of nnest_mcmc_steps at (seed, w, t) (streams 5 and 6): a draw at (w, t) is used
 *              by exactly one kind, so no new stream exists and nnest_mcmc_fill_noise exports the draws of either kind.
 *     target:  lp(z) = lp_beta(z) of nnest_mcmc_tempered_steps = ((beta * logL) + log|det dx/dz|) + prior; beta is always an argument,
 *              beta = 1.0 is the untempered target bit for bit.  The walker carries and logs the UNTEMPERED logL.
 *     local:   q = z + step_size * eps (float32, each operation rounded); the walker moves iff lp(q) - lp(z) > log u (float64):
 *              exactly nnest_mcmc_tempered_steps's step.
 *     global:  q = eps on the live dims (padded dims 0).  With zz(z) = the float64 sum of the squares of the float32 row, summed in the
 *              order the layout's importance kernel uses, b(z) = -1/2 zz(z) - D * log sqrt(2 pi) (the N(0, I) density of
 *              nnest_importance_evidence) and lw(z) = lp(z) - b(z) (float64, one rounded subtraction, no contraction), the walker
 *              moves iff lw(q) - lw(z) > log u (float64, the same comparison).  b and lw are functions of the row and its lp alone:
 *              nothing but (z, lp, logL) is carried between launches, so a run cut into launches stays the same run.  A walker
 *              whose lp and the proposal's lp are both -inf refuses (NaN compares false), as in the local rule.
 *   ONE loop and ONE target evaluation per step: the kind selects q and the two sides of the accept rule.  global_every = 0 is
 *   nnest_mcmc_tempered_steps's run bit for bit on every output (and at beta = 1.0 nnest_mcmc_steps's).  Everything said of
 *   nnest_mcmc_steps holds: the buffers, the invariances (the cut into launches, a shard by walker_offset, history or not), steps = 0
 *   evaluates the start and writes x_out_dev, lp_out_dev and logl_out_dev only.  n_accept_dev [C] or NULL counts the accepted steps
 *   of BOTH kinds; n_accept_global_dev [C] or NULL the accepted global steps.  NNEST_E_ARG before any launch, the outputs untouched:
 *   beta not finite or < 0, global_every < 0, and nnest_mcmc_steps's argument errors.  NNEST_E_UNSUPPORTED before any launch: what
 *   the _check entry below refuses.  The base must be N(0, I).
 * nnest_mcmc_mixed_check, nnest_spline_mcmc_mixed_check: NNEST_OK where the entry takes this handle (its shape and base) and this
 *   likelihood id, else NNEST_E_UNSUPPORTED with the reason in nnest_hip_last_error() -- a GeneralisedNormal base in the words of
 *   nnest_importance_check --, as the entry itself would answer; nothing is launched. */
int nnest_mcmc_mixed_check(nnest_nvp_t *nvp, int like_id);
int nnest_spline_mcmc_mixed_check(struct nnest_spline *spl, int like_id);
int nnest_mcmc_mixed_steps(nnest_nvp_t *nvp, const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev, const float *lo_dev,
                           const float *hi_dev, const float *z_in_dev, const double *lp_in_dev, const double *logl_in_dev, float *z_out_dev,
                           float *x_out_dev, double *lp_out_dev, double *logl_out_dev, float *hist_z_dev, float *hist_x_dev,
                           double *hist_logl_dev, int *n_accept_dev, int C, int steps, float step_size, uint64_t step0, uint64_t seed,
                           uint64_t walker_offset, double beta, int global_every, int *n_accept_global_dev, void *stream);
int nnest_spline_mcmc_mixed_steps(struct nnest_spline *spl, const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev,
                                  const float *lo_dev, const float *hi_dev, const float *z_in_dev, const double *lp_in_dev,
                                  const double *logl_in_dev, float *z_out_dev, float *x_out_dev, double *lp_out_dev, double *logl_out_dev,
                                  float *hist_z_dev, float *hist_x_dev, double *hist_logl_dev, int *n_accept_dev, int C, int steps,
                                  float step_size, uint64_t step0, uint64_t seed, uint64_t walker_offset, double beta, int global_every,
                                  int *n_accept_global_dev, void *stream);
/* THE ADAPTIVE WALK: the mixed walk above with the step of the local proposal adapted PER WALKER, in kernels of their own
 * (nnest_mcmc_adapt.hip, nnest_spline_mcmc_adapt.hip).  BUILD-DEFINED: the reference's mcmc_dynamic_step_size is a
 * batch-wide rule, and its MCMCSampler never forwards it.  (All added within ABI 15.)
 * nnest_mcmc_adapt_steps, nnest_spline_mcmc_adapt_steps: the arguments of nnest_mcmc_mixed_steps / nnest_spline_mcmc_mixed_steps up to
 *   n_accept_global_dev, then `const double *step_in_dev, double *step_out_dev, double *hist_step_dev, uint32_t adapt_steps,
 *   double adapt_rate, double target_accept` before `stream`.  Kind, draws, target and the accept rule of a step are the mixed
 *   walk's.  Every walker carries a float64 `sigma`:
 *     start:   sigma = min(max(step_in_dev[row], NNEST_ADAPT_STEP_MIN), NNEST_ADAPT_STEP_MAX) with step_in_dev given (the max and
 *              the min each keep their second operand where the comparison is false: a NaN loads as NNEST_ADAPT_STEP_MIN), else
 *              (double)step_size.
 *     local:   q = z + (float)sigma * eps (float32, each operation rounded: the mixed walk's proposal at the float32 rounding of the
 *              walker's own sigma); the walker moves iff lp(q) - lp(z) > log u.  After the decision acc, iff t < adapt_steps:
 *                g     = adapt_rate / sqrt((double)t + 1.0)
 *                sigma = sigma * (1.0 + g * ((acc ? 1.0 : 0.0) - target_accept))
 *                sigma = min(max(sigma, NNEST_ADAPT_STEP_MIN), NNEST_ADAPT_STEP_MAX)
 *              in float64, each operation rounded, no contraction; division and square root are correctly rounded.  The update
 *              uses the BINARY decision, not the acceptance probability: no transcendental enters, and the rule replayed from the
 *              decisions reproduces sigma to the bit.  A refusal because both sides are -inf counts as a rejection.
 *     global:  the mixed walk's step; it uses no step and leaves sigma alone.
 *     frozen:  a step with t >= adapt_steps leaves sigma alone: from there on each chain is a Metropolis chain at a fixed step.
 *   The run stays a function of (seed, w, t) and the start alone; the state carried between launches is (z, lp, logL, sigma), so a
 *   run cut into launches with step_out_dev handed to step_in_dev is the same run, and the invariances of nnest_mcmc_steps hold.
 *   adapt_steps = 0 with step_in_dev NULL is nnest_mcmc_mixed_steps's run bit for bit; adapt_steps = 0 with step_in_dev given runs
 *   every walker at its own fixed step.  step_in_dev [C] or NULL; step_out_dev [C] or NULL, written iff steps > 0, as z_out_dev is;
 *   hist_step_dev [C, steps] or NULL, independent of the history trio: sigma after each step, global steps included.  The other
 *   buffers and counters are the mixed entry's.  NNEST_E_ARG before any launch, the outputs untouched: adapt_rate not finite or
 *   outside [0, 1], target_accept not strictly inside (0, 1) -- with these the factor stays inside (0, 2) --, and the mixed entry's
 *   argument errors.  NNEST_E_UNSUPPORTED before any launch: what the _check entry below refuses.
 * nnest_mcmc_adapt_check, nnest_spline_mcmc_adapt_check: as nnest_mcmc_mixed_check / nnest_spline_mcmc_mixed_check answer; nothing is
 *   launched. */
#define NNEST_ADAPT_STEP_MIN 1e-8
#define NNEST_ADAPT_STEP_MAX 1e2
int nnest_mcmc_adapt_check(nnest_nvp_t *nvp, int like_id);
int nnest_spline_mcmc_adapt_check(struct nnest_spline *spl, int like_id);
int nnest_mcmc_adapt_steps(nnest_nvp_t *nvp, const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev, const float *lo_dev,
                           const float *hi_dev, const float *z_in_dev, const double *lp_in_dev, const double *logl_in_dev, float *z_out_dev,
                           float *x_out_dev, double *lp_out_dev, double *logl_out_dev, float *hist_z_dev, float *hist_x_dev,
                           double *hist_logl_dev, int *n_accept_dev, int C, int steps, float step_size, uint64_t step0, uint64_t seed,
                           uint64_t walker_offset, double beta, int global_every, int *n_accept_global_dev, const double *step_in_dev,
                           double *step_out_dev, double *hist_step_dev, uint32_t adapt_steps, double adapt_rate, double target_accept,
                           void *stream);
int nnest_spline_mcmc_adapt_steps(struct nnest_spline *spl, const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev,
                                  const float *lo_dev, const float *hi_dev, const float *z_in_dev, const double *lp_in_dev,
                                  const double *logl_in_dev, float *z_out_dev, float *x_out_dev, double *lp_out_dev, double *logl_out_dev,
                                  float *hist_z_dev, float *hist_x_dev, double *hist_logl_dev, int *n_accept_dev, int C, int steps,
                                  float step_size, uint64_t step0, uint64_t seed, uint64_t walker_offset, double beta, int global_every,
                                  int *n_accept_global_dev, const double *step_in_dev, double *step_out_dev, double *hist_step_dev,
                                  uint32_t adapt_steps, double adapt_rate, double target_accept, void *stream);
/* A GAUSSIAN LIKELIHOOD FROM USER DATA in the adaptive walk above, in kernels of their own (nnest_mcmc_gdata.hip,
 * nnest_spline_mcmc_gdata.hip).  BUILD-DEFINED.  No NNEST_LIKE_* id stands for it: the likelihood is compiled into
 * these kernels and described by nnest_gdata_t.  (All added within ABI 15.)
 *   logL(theta) = logl0 - 1/2 (theta - mu)^T P (theta - mu),   P = R^T R symmetric positive definite.
 * nnest_gdata_t: mu_dev [D] float32; r_dev [D, D] float32, row-major, UPPER triangular (the float32 rounding of L^T, P = L L^T in
 *   float64; the strictly lower triangle holds zeros and is never read); logl0 finite; 1 <= D <= 128.
 * The arithmetic, with t = T(x) the float32 row the existing evaluators produce (or a row of t_dev):
 *     d_c  = t_c - mu_c                       float32, one rounding
 *     y_r  = sum_{c >= r} R[r, c] * d_c       float32; the order of the sum is the kernel's own, fused multiply-adds allowed
 *     q    = sum_r (double)y_r * (double)y_r  float64, in a fixed order: the same bits on every lane that holds the walker
 *     logL = logl0 - 0.5 * q                  float64; -1e100 where that is not finite (the rule of the known likelihoods)
 *   So logL <= logl0 always, a row equal to mu gives logl0 exactly, and the same row gives the same bits in any position of any
 *   launch of one entry.  (The two walks order the sum of y_r differently: their values agree to float32 rounding, not to the bit.)
 * nnest_loglike_gdata: the likelihood alone on N rows t_dev [N, D] float32 that are already T(x); logl_dev [N] float64.  D must be
 *   the descriptor's.  N = 0 launches nothing.
 * nnest_mcmc_gdata_steps, nnest_spline_mcmc_gdata_steps: the arguments of nnest_mcmc_adapt_steps / nnest_spline_mcmc_adapt_steps with
 *   `const nnest_gdata_t *gdata` in place of `const nnest_like_t *like`.  The run is the adaptive walk's in every respect -- draws,
 *   schedule, weight, accept rule, step rule, beta, lp_in_dev / logl_in_dev, histories, counters, steps = 0, the cut into launches,
 *   a shard by walker_offset --; only logL differs.  With adapt_steps = 0 and step_in_dev NULL it is the mixed walk on this
 *   likelihood, with global_every = 0 besides the tempered random walk, at beta = 1.0 the plain one.
 * NNEST_E_ARG before any launch, the outputs untouched: gdata NULL, a NULL mu_dev or r_dev, D outside 1 .. 128 or not the flow's
 *   x_dim (not the D argument of nnest_loglike_gdata), logl0 not finite, and every argument error of the adaptive entries.
 *   NNEST_E_UNSUPPORTED before any launch: what the _check entry refuses.
 * nnest_mcmc_gdata_check, nnest_spline_mcmc_gdata_check: NNEST_OK where the entry takes this handle (its shape and base: what
 *   nnest_mcmc_adapt_check / nnest_spline_mcmc_adapt_check take) and a descriptor of dimension D, else NNEST_E_UNSUPPORTED -- or
 *   NNEST_E_ARG for a D that is not the flow's x_dim -- with the reason in nnest_hip_last_error(); nothing is launched. */
typedef struct nnest_gdata {
    const float *mu_dev;
    const float *r_dev;
    double logl0;
    int D;
} nnest_gdata_t;
int nnest_loglike_gdata(const nnest_gdata_t *gdata, const float *t_dev, double *logl_dev, int N, int D, void *stream);
int nnest_mcmc_gdata_check(nnest_nvp_t *nvp, int D);
int nnest_spline_mcmc_gdata_check(struct nnest_spline *spl, int D);
int nnest_mcmc_gdata_steps(nnest_nvp_t *nvp, const nnest_gdata_t *gdata, const float *t_std_dev, const float *t_mean_dev, const float *lo_dev,
                           const float *hi_dev, const float *z_in_dev, const double *lp_in_dev, const double *logl_in_dev, float *z_out_dev,
                           float *x_out_dev, double *lp_out_dev, double *logl_out_dev, float *hist_z_dev, float *hist_x_dev,
                           double *hist_logl_dev, int *n_accept_dev, int C, int steps, float step_size, uint64_t step0, uint64_t seed,
                           uint64_t walker_offset, double beta, int global_every, int *n_accept_global_dev, const double *step_in_dev,
                           double *step_out_dev, double *hist_step_dev, uint32_t adapt_steps, double adapt_rate, double target_accept,
                           void *stream);
int nnest_spline_mcmc_gdata_steps(struct nnest_spline *spl, const nnest_gdata_t *gdata, const float *t_std_dev, const float *t_mean_dev,
                                  const float *lo_dev, const float *hi_dev, const float *z_in_dev, const double *lp_in_dev,
                                  const double *logl_in_dev, float *z_out_dev, float *x_out_dev, double *lp_out_dev, double *logl_out_dev,
                                  float *hist_z_dev, float *hist_x_dev, double *hist_logl_dev, int *n_accept_dev, int C, int steps,
                                  float step_size, uint64_t step0, uint64_t seed, uint64_t walker_offset, double beta, int global_every,
                                  int *n_accept_global_dev, const double *step_in_dev, double *step_out_dev, double *hist_step_dev,
                                  uint32_t adapt_steps, double adapt_rate, double target_accept, void *stream);
/* A GENERALISED LINEAR MODEL OF USER DATA -- logistic or Poisson (log-link) regression -- in the adaptive walk above, in kernels of
 * their own (nnest_mcmc_glm.hip, nnest_spline_mcmc_glm.hip, glm_data.h).  BUILD-DEFINED.  No NNEST_LIKE_* id stands
 * for it: the likelihood is compiled into these kernels, one per family, and described by nnest_glm_t.  (All added within ABI 15.)
 *   eta_i = o_i + sum_c A[i, c] theta_c,   logL(theta) = logl0 + sum_{i < n} l_i,
 *   NNEST_GLM_LOGISTIC: y_i in {0, 1},  l_i = -softplus((1 - 2 y_i) eta_i),  softplus(s) = max(s, 0) + log1p(exp(-|s|));
 *   NNEST_GLM_POISSON:  y_i >= 0,       l_i = y_i eta_i - exp(eta_i)   (the caller puts -sum lgamma(y_i + 1) into logl0).
 * nnest_glm_t: at_dev [D, ld] float32 = A^T with leading dimension ld (rows of A along the fast axis), y_dev [ld] and o_dev [ld]
 *   float32 (o the offset: zeros for none); 1 <= n <= 65536 rows, ld >= n a multiple of 64, 1 <= D <= 128; logl0 finite.  What the
 *   arrays hold at rows n .. ld - 1 does not matter: those rows are masked (softplus(0) is not 0).  The values of y are the
 *   caller's business (likelihoods.GLMData checks them on the host).
 * The arithmetic, with t = T(x) the float32 row the existing evaluators produce (or a row of t_dev):
 *     eta_i = o_i + sum_c A[i, c] * t_c       float32; fused multiply-adds, in the kernel's own order
 *     l_i                                     float64 from (double)eta_i, as written above; NaN where eta_i is not finite
 *     logL  = logl0 + sum_{i < n} l_i         float64, in a fixed order per entry; -1e100 where that is not finite
 *   So a logistic logL <= logl0 always, a row with a non-finite coordinate gives -1e100, and the same row gives the same bits in
 *   any position of any launch of one entry.  (The two walks order the sums differently: their values agree to rounding.)
 * nnest_loglike_glm: the likelihood alone on N rows t_dev [N, D] float32 that are already T(x); logl_dev [N] float64.  D must be
 *   the descriptor's.  N = 0 launches nothing.
 * nnest_mcmc_glm_steps, nnest_spline_mcmc_glm_steps: the arguments of nnest_mcmc_adapt_steps / nnest_spline_mcmc_adapt_steps with
 *   `const nnest_glm_t *glm` in place of `const nnest_like_t *like`.  The run is the adaptive walk's in every respect -- draws,
 *   schedule, weight, accept rule, step rule, beta, lp_in_dev / logl_in_dev, histories, counters, steps = 0, the cut into launches,
 *   a shard by walker_offset --; only logL differs.  With adapt_steps = 0 and step_in_dev NULL it is the mixed walk on this
 *   likelihood, with global_every = 0 besides the tempered random walk, at beta = 1.0 the plain one.
 * NNEST_E_ARG before any launch, the outputs untouched: glm NULL, a NULL at_dev, y_dev or o_dev, D outside 1 .. 128 or not the
 *   flow's x_dim (not the D argument of nnest_loglike_glm), n outside 1 .. 65536, ld < n or not a multiple of 64 or above 65536, a
 *   family that is neither of the two, logl0 not finite, and every argument error of the adaptive entries.
 *   NNEST_E_UNSUPPORTED before any launch: what the _check entry refuses.
 * nnest_mcmc_glm_check, nnest_spline_mcmc_glm_check: NNEST_OK where the entry takes this handle (its shape and base: what
 *   nnest_mcmc_adapt_check / nnest_spline_mcmc_adapt_check take) and a descriptor of dimension D, else NNEST_E_UNSUPPORTED -- or
 *   NNEST_E_ARG for a D that is not the flow's x_dim -- with the reason in nnest_hip_last_error(); nothing is launched. */
#define NNEST_GLM_LOGISTIC 0
#define NNEST_GLM_POISSON 1
typedef struct nnest_glm {
    const float *at_dev;
    const float *y_dev;
    const float *o_dev;
    double logl0;
    int n;
    int ld;
    int D;
    int family;
} nnest_glm_t;
int nnest_loglike_glm(const nnest_glm_t *glm, const float *t_dev, double *logl_dev, int N, int D, void *stream);
int nnest_mcmc_glm_check(nnest_nvp_t *nvp, int D);
int nnest_spline_mcmc_glm_check(struct nnest_spline *spl, int D);
int nnest_mcmc_glm_steps(nnest_nvp_t *nvp, const nnest_glm_t *glm, const float *t_std_dev, const float *t_mean_dev, const float *lo_dev,
                         const float *hi_dev, const float *z_in_dev, const double *lp_in_dev, const double *logl_in_dev, float *z_out_dev,
                         float *x_out_dev, double *lp_out_dev, double *logl_out_dev, float *hist_z_dev, float *hist_x_dev,
                         double *hist_logl_dev, int *n_accept_dev, int C, int steps, float step_size, uint64_t step0, uint64_t seed,
                         uint64_t walker_offset, double beta, int global_every, int *n_accept_global_dev, const double *step_in_dev,
                         double *step_out_dev, double *hist_step_dev, uint32_t adapt_steps, double adapt_rate, double target_accept,
                         void *stream);
int nnest_spline_mcmc_glm_steps(struct nnest_spline *spl, const nnest_glm_t *glm, const float *t_std_dev, const float *t_mean_dev,
                                const float *lo_dev, const float *hi_dev, const float *z_in_dev, const double *lp_in_dev,
                                const double *logl_in_dev, float *z_out_dev, float *x_out_dev, double *lp_out_dev, double *logl_out_dev,
                                float *hist_z_dev, float *hist_x_dev, double *hist_logl_dev, int *n_accept_dev, int C, int steps,
                                float step_size, uint64_t step0, uint64_t seed, uint64_t walker_offset, double beta, int global_every,
                                int *n_accept_global_dev, const double *step_in_dev, double *step_out_dev, double *hist_step_dev,
                                uint32_t adapt_steps, double adapt_rate, double target_accept, void *stream);
/* INDEPENDENT NORMAL PRIORS beside the regression likelihoods above, in kernels of their own (nnest_mcmc_glm_prior.hip,
 * nnest_spline_mcmc_glm_prior.hip, gauss_prior.h).  BUILD-DEFINED.  (All added within ABI 15.)
 *   log pi(theta) = logc - 1/2 sum_c ((theta_c - m_c) / sigma_c)^2,   logc = -sum_c log sigma_c - (D / 2) log 2 pi.
 * nnest_gauss_prior_t: m_dev [D] float32 the means, r_dev [D] float32 = float32(1 / sigma_c), logc as above (any finite constant is
 *   taken: the walk does not depend on it), 1 <= D <= 128.  r = 0 is an infinitely wide prior in that coordinate.
 * The arithmetic, with t = T(x) the float32 row the likelihood sees (or a row of t_dev):
 *     u_c    = (t_c - m_c) * r_c                 float32, each operation rounded (no fused multiply-add)
 *     ss     = sum_c (double)u_c * (double)u_c   float64, in the kernel's own fixed order (the order of the walk's sum of z^2)
 *     log pi = logc - 0.5 * ss                   float64; -inf where ss is not finite: a non-finite coordinate is refused, never NaN
 *     lp_beta = ((beta * logL) + log|det|) + log pi   each operation rounded: the tempered target with log pi in place of its 0.0
 *   A row outside the box lo_dev / hi_dev has lp = -inf, as in every sibling.  The same row gives the same bits of log pi at any
 *   position of any launch of one entry.  (The two walks order the sum differently: their values agree to rounding.)
 * nnest_logprior_gauss: log pi alone on N rows t_dev [N, D] float32 that are already T(x); logp_dev [N] float64.  D must be the
 *   descriptor's.  N = 0 launches nothing.
 * nnest_mcmc_glm_prior_steps, nnest_spline_mcmc_glm_prior_steps: the arguments of nnest_mcmc_glm_steps / nnest_spline_mcmc_glm_steps
 *   with `const nnest_gauss_prior_t *prior` after `glm`.  The run is theirs in every respect -- draws, mixed schedule, the global
 *   step's weight (on this lp), accept rule, step rule, beta, lp_in_dev / logl_in_dev, histories, counters, steps = 0, the cut into
 *   launches, a shard by walker_offset --; only the target's prior term differs.  With r = 0 and logc = 0.0 every lp of a row whose
 *   coordinates are finite is nnest_mcmc_glm_steps's to the bit.
 * NNEST_E_ARG before any launch, the outputs untouched: prior NULL, a NULL m_dev or r_dev, D outside 1 .. 128 or not the flow's
 *   x_dim, logc not finite, and every argument error of the glm entries.  NNEST_E_UNSUPPORTED before any launch: what the _check
 *   entry refuses.
 * nnest_mcmc_glm_prior_check, nnest_spline_mcmc_glm_prior_check: the verdict of nnest_mcmc_glm_check / nnest_spline_mcmc_glm_check
 *   (the same shapes and base) for these entries; nothing is launched. */
typedef struct nnest_gauss_prior {
    const float *m_dev;
    const float *r_dev;
    double logc;
    int D;
} nnest_gauss_prior_t;
int nnest_logprior_gauss(const nnest_gauss_prior_t *prior, const float *t_dev, double *logp_dev, int N, int D, void *stream);
int nnest_mcmc_glm_prior_check(nnest_nvp_t *nvp, int D);
int nnest_spline_mcmc_glm_prior_check(struct nnest_spline *spl, int D);
int nnest_mcmc_glm_prior_steps(nnest_nvp_t *nvp, const nnest_glm_t *glm, const nnest_gauss_prior_t *prior, const float *t_std_dev,
                               const float *t_mean_dev, const float *lo_dev, const float *hi_dev, const float *z_in_dev,
                               const double *lp_in_dev, const double *logl_in_dev, float *z_out_dev, float *x_out_dev, double *lp_out_dev,
                               double *logl_out_dev, float *hist_z_dev, float *hist_x_dev, double *hist_logl_dev, int *n_accept_dev, int C,
                               int steps, float step_size, uint64_t step0, uint64_t seed, uint64_t walker_offset, double beta,
                               int global_every, int *n_accept_global_dev, const double *step_in_dev, double *step_out_dev,
                               double *hist_step_dev, uint32_t adapt_steps, double adapt_rate, double target_accept, void *stream);
int nnest_spline_mcmc_glm_prior_steps(struct nnest_spline *spl, const nnest_glm_t *glm, const nnest_gauss_prior_t *prior,
                                      const float *t_std_dev, const float *t_mean_dev, const float *lo_dev, const float *hi_dev,
                                      const float *z_in_dev, const double *lp_in_dev, const double *logl_in_dev, float *z_out_dev,
                                      float *x_out_dev, double *lp_out_dev, double *logl_out_dev, float *hist_z_dev, float *hist_x_dev,
                                      double *hist_logl_dev, int *n_accept_dev, int C, int steps, float step_size, uint64_t step0,
                                      uint64_t seed, uint64_t walker_offset, double beta, int global_every, int *n_accept_global_dev,
                                      const double *step_in_dev, double *step_out_dev, double *hist_step_dev, uint32_t adapt_steps,
                                      double adapt_rate, double target_accept, void *stream);
/* POINTWISE PREDICTIVE STATISTICS of the regression likelihoods above over a set of posterior draws: per data row, what lppd, WAIC
 * and importance-sampled leave-one-out are made of, and per new design row the posterior predictive mean (nnest_glm_pointwise.hip,
 * glm_pointwise.h).  BUILD-DEFINED: the reference has no such estimator.  (All added within ABI 15.)
 * The [S draws x n rows] matrix of terms is never stored: the product runs on the matrix cores, the float64 term behind it, and a
 * running reduction over the draws per data row.  t_dev [S, D] float32: rows that are already theta = T(x).  For nnest_glm_t:
 *     eta_is = o_i + sum_c A[i, c] * t_sc     float32, exactly nnest_loglike_glm's definition: fused multiply-adds, in the kernel's
 *                                             own order
 *     l_is   = the family's term              float64 from (double)eta_is, as written above (NaN where eta_is is not finite).
 *                                             logl0 plays no part: a constant belongs to no row
 *   A pair (i, s) is LIVE when l_is is finite; NaN and +-inf are dead and are not counted.  A draw with a non-finite coordinate is
 *   dead for every row.
 * nnest_glm_pointwise writes eight doubles per data row i < n, stats_dev[i][0 .. 7], all sums over the live s:
 *     0, 1      a_i = max_s l_is,          P_i = sum_s exp(l_is - a_i)
 *     2, 3, 4   b_i = max_s (-l_is),       Q_i = sum_s exp(-l_is - b_i),   Q2_i = sum_s exp(2 (-l_is - b_i))
 *     5         cnt_i, the live draws
 *     6, 7      mean_i = the mean of l_is, M2_i = sum_s (l_is - mean_i)^2; carried as (count, mean, M2), merged by Chan's rule
 *   A row with no live draw gives {-inf, 0, -inf, 0, 0, 0, 0, 0}.  (lppd_i = a + log P - log cnt; the WAIC penalty is
 *   M2 / (cnt - 1); the importance-sampled leave-one-out density is -(b + log Q - log cnt), its effective sample size Q^2 / Q2.)
 * nnest_glm_predict is the same stream over NEW design rows: the descriptor holds A_new and offset_new (y_dev is ignored but must
 *   not be NULL), and row j < n gets three doubles stats_dev[j][0 .. 2] = {cnt_j, mean_j, M2_j} of the inverse link
 *     NNEST_GLM_LOGISTIC: mu_js = 1 / (1 + exp(-eta_js));   NNEST_GLM_POISSON: mu_js = exp(eta_js)
 *   in float64 from the float32 eta_js.  A pair is live when eta_js and mu_js are finite.
 * The reduction is deterministic and uses no floating-point atomics: the draws are dealt in tiles of 16 to G = nnest_glm_pointwise_groups
 *   (S, n) draw groups, each workgroup writes its rows' partial statistics into partials_dev ([G, n, 8] doubles; [G, n, 3] for
 *   nnest_glm_predict), and a second kernel merges the G partials of a row in index order.  The same call made twice returns the
 *   same bits.  G depends on (S, n) alone, not on the device.  S = 0 is valid (G = 0) and writes the empty statistics.  The
 *   statistics of a run cut into launches and merged on the host (a = max a_k, P = sum P_k e^(a_k - a), ...; Chan's rule for slots
 *   5 - 7: _lib.merge_glm_pointwise) are the single launch's up to reordered float64 addition.  Rows n .. ld - 1 of the descriptor's
 *   arrays are masked, whatever they hold.  The calls are asynchronous on `stream`.
 * nnest_glm_pointwise_groups: G for S draws and n rows (0 for S = 0); -1 for S outside 0 .. 2^30 or n outside 1 .. 65536.
 * NNEST_E_ARG before any launch, the outputs untouched: a NULL glm, t_dev, stats_dev or partials_dev, a D that is not the
 *   descriptor's, every descriptor nnest_loglike_glm refuses, S outside 0 .. 2^30. */
int nnest_glm_pointwise_groups(int S, int n);
int nnest_glm_pointwise(const nnest_glm_t *glm, const float *t_dev, double *stats_dev, double *partials_dev, int S, int D, void *stream);
int nnest_glm_predict(const nnest_glm_t *glm, const float *t_dev, double *stats_dev, double *partials_dev, int S, int D, void *stream);
/* PARETO-SMOOTHED LEAVE-ONE-OUT (PSIS-LOO) of the same likelihoods over the same draws, and the matrix of their terms
 * (nnest_glm_psis.hip, glm_psis.h).  BUILD-DEFINED, to the operation: the reference has no such estimator.  (All
 * added within ABI 15.)  eta_is and l_is are nnest_glm_pointwise's, to the bit: the kernels stream the draws in its layout.
 * nnest_glm_terms writes the matrix itself: out_dev [S, n] float64, out[s][i] = l_is, NaN for a dead pair.  S = 0 writes nothing.
 *   NNEST_E_ARG before any launch: what nnest_glm_pointwise refuses, a NULL out_dev, S n above 2^30.
 * nnest_glm_psis: per data row i, over its live draws, with b_i and cnt_i the slots 2 and 5 of stats_dev [n, 8] = what
 *   nnest_glm_pointwise wrote FOR THE SAME t_dev AND S (read only),
 *     d_s   = b_i - (-l_is) >= 0                       float64
 *     M*    = min(cnt / 5, ceil(3 sqrt(cnt)))          integers; ceil(3 sqrt(cnt)) the smallest m with m^2 >= 9 cnt
 *     c_i   = the largest double whose low 40 bits are zero with #{s : d_s < c_i} <= M*  (a bin edge of key(d) = the top 24 bits of
 *             the pattern of d, so that tied draws go in or out together); 0 for a row with no live draw
 *     tail  = {s : d_s < c_i}, M_i its size (0 when the bin of d = 0 alone holds more than M* draws)
 *     body  = the others: N_body their number, B = sum e^(-d), B2 = sum (e^(-d))^2
 *   and, where M_i >= 5, Zhang & Stephens' (2009) fit of a generalised Pareto distribution to the tail's exceedances, with the
 *   prior of loo::gpdfit: u = e^(-c_i); x_(1) <= .. <= x_(M) the sorted e^(-d) - u; m = 30 + floor(sqrt(M));
 *   x* = x_(floor(M / 4 + 0.5)); theta_j = 1 / x_(M) + (1 - sqrt(m / (j - 1/2))) / (3 x*), j = 1 .. m; k_j = mean log1p(-theta_j x);
 *   L_j = M (log(-theta_j / k_j) - k_j - 1); w_j = 1 / sum_i exp(L_i - L_j) (an overflow to +inf: 0); theta^ = sum theta_j w_j;
 *   k = mean log1p(-theta^ x); sigma = -k / theta^; k^ = (k M + 5) / (M + 10).  The smoothed tail: p_j = (j - 1/2) / M,
 *   q_j = min(1, u + sigma expm1(-k^ log1p(-p_j)) / k^) (for |k^| < 2^-40: u - sigma log1p(-p_j)), beside d_(j), the d of x_(j).
 *     log numerator   = log(N_body + sum_j q_j e^(d_(j)))
 *     log denominator = log(B + sum_j q_j)
 *     elpd_psis       = (-b_i + log numerator) - log denominator
 *     psis_ess        = (B + sum q)^2 / (B2 + sum q^2)
 *   Where M_i < 5 there is no fit: k^ = +inf, sigma = NaN, and q_j = e^(-d_(j)), the raw weights, with the numerator N_body + M_i:
 *   the plain importance-sampling estimate.  A k that is not finite: k^ = NaN, sigma = NaN, and the plain estimate likewise.
 *   out_dev [n, 16] float64, row i: {0 c_i, 1 M_i, 2 N_body, 3 B, 4 B2, 5 sigma, 6 k^, 7 log numerator, 8 log denominator,
 *   9 elpd_psis (NaN for a row with no live draw), 10 psis_ess (0 then), 11 flag, 12 M*, 13 theta^ (NaN without a fit), 14, 15 zero}.
 *   flag: 1 = a tail value found no slot and was dropped (never with a stats_dev of these draws), 2 = no fit (M_i < 5), 4 = k not
 *   finite.  (The Poisson -lgamma(y_i + 1) is the caller's to add to elpd_psis.)
 *   work_dev: nnest_glm_psis_work_bytes(S, n) bytes.  Its first n Mcap doubles, Mcap = nnest_glm_psis_tail_cap(S) = ceil(3 sqrt(S))
 *   (1 for S = 0), are the tail buffer [n, Mcap]: behind the call, row i holds its M_i tail values d sorted ascending in its first
 *   M_i slots; the other slots are not written.  The rest -- the draw groups' body sums, the digit counts, the prefixes and the slot
 *   counters -- is scratch.  Nothing is written past the stated sizes nor to rows i >= n; rows n .. ld - 1 of the descriptor are masked.
 *   The cutoff comes from three streaming passes that count one 8-bit digit of the key each (integer atomics), a fourth pass
 *   collects the tail and the body sums, a fit kernel sorts the tail and does the rest in a fixed order: no floating-point atomics,
 *   the same call twice returns the same bits.  All S draws are resident in one call: S <= 2^20 (thin a longer run), and the work
 *   buffer at most 2^30 bytes.  S = 0 is valid and writes the empty result {0, 0, 0, 0, 0, NaN, +inf, -inf, -inf, NaN, 0, 2, 0, NaN,
 *   0, 0}.  Asynchronous on `stream`.
 * nnest_glm_psis_work_bytes: the bytes of work_dev; -1 for S outside 0 .. 2^20, n outside 1 .. 65536 or more than 2^30 bytes.
 * nnest_glm_psis_tail_cap: Mcap; -1 for S outside 0 .. 2^20.
 * NNEST_E_ARG before any launch, the outputs untouched: everything nnest_glm_pointwise refuses, a NULL stats_dev, out_dev or
 *   work_dev, S above 2^20, a work size above 2^30 bytes. */
int nnest_glm_terms(const nnest_glm_t *glm, const float *t_dev, double *out_dev, int S, int D, void *stream);
int nnest_glm_psis_tail_cap(int S);
long long nnest_glm_psis_work_bytes(int S, int n);
int nnest_glm_psis(const nnest_glm_t *glm, const float *t_dev, const double *stats_dev, double *out_dev, void *work_dev, int S, int D,
                   void *stream);
/* GRADIENT, CURVATURE AND NEWTON STEP of the same likelihoods at ONE theta: what a posterior mode, the Laplace approximation and the
 * Laplace evidence are made of (nnest_glm_newton.hip, glm_newton.h).  BUILD-DEFINED: the reference has none.  (All
 * added within ABI 15.)  Everything is float64; the float32 descriptor is read as it is and converted exactly.
 * nnest_glm_curv, at theta_dev [D] float64, writes out_dev [1 + D + D D] float64:
 *     eta_i = o_i + sum_c A[i, c] * theta_c    float64; fused multiply-adds, in the kernel's own fixed order
 *     l_i                                      the family's term as written above, from the double eta_i (NaN where it is not finite)
 *     NNEST_GLM_LOGISTIC: mu_i = 1 / (1 + exp(-eta_i)), w_i = mu_i (1 - mu_i), both from exp(-|eta_i|): no overflow at either end
 *     NNEST_GLM_POISSON:  mu_i = w_i = exp(eta_i)
 *     out[0]               = logl0 + sum_{i < n} l_i              -1e100 where that is not finite
 *     out[1 + c]           = sum_i (y_i - mu_i) A[i, c]           the gradient of log L
 *     out[1 + D + c D + d] = sum_i w_i A[i, c] A[i, d]            the NEGATIVE Hessian of log L: a full matrix, the lower triangle a
 *                                                                 bit copy of the upper
 *   A non-finite theta_c or a non-finite sum leaves out[0] = -1e100; the gradient and the matrix then hold whatever they hold: read
 *   out[0] first.  Rows n .. ld - 1 of the descriptor's arrays are masked, whatever they hold.  The rows are dealt in blocks of 64 to
 *   G = nnest_glm_curv_groups(n, D) workgroups, which write their sums into partials_dev ([G][1 + D + D (D + 1) / 2] doubles), and a
 *   second kernel adds the G partials of each entry in index order: no floating-point atomics, the same call twice returns the same
 *   bits, and G depends on (n, D) alone, not on the device.  The matrix is accumulated on the float64 matrix cores.
 * nnest_glm_curv_groups: G for n rows and D columns; -1 for n outside 1 .. 65536 or D outside 1 .. 128.
 * nnest_glm_newton_solve, in one workgroup, from curv_dev (nnest_glm_curv's out) and theta_dev [D]: with the prior's m, r =
 *   float32(1 / sigma) and logc converted to double (prior NULL: no prior, log pi = 0),
 *     g_c = out[1 + c] - (theta_c - m_c) r_c^2,   H = the matrix + diag(r_c^2),   log pi = logc - 1/2 sum_c ((theta_c - m_c) r_c)^2
 *     H = L L^T (float64 Cholesky, a fixed order),   H delta = g by the two triangular solves
 *   step_dev [D] = delta; chol_dev [D D] = L, row-major, the part above the diagonal zero; info_dev [4] =
 *     {log L + log pi,  the Newton decrement lambda^2 = g^T delta,  log det H = 2 sum_c log L_cc,  status}
 *   status 0: ok; 1: a pivot was <= 0 or not finite (H is not positive definite: the data do not determine theta) -- pivot j counts
 *   as <= 0 when it is not above (j + 2) 2^-52 H_jj, the bound on its own rounding error, so that an exactly singular H is refused
 *   whichever way its last pivots round --; 2: curv_dev[0]
 *   was the safe value -1e100, or log pi is not finite.  For a status other than 0 step_dev and chol_dev are zeros (never NaN) and
 *   info[1] = info[2] = 0.
 * Both are asynchronous on `stream`.  NNEST_E_ARG before any launch, the outputs untouched: everything nnest_loglike_glm refuses, a
 *   D that is not the descriptor's (the solve: D outside 1 .. 128), a NULL pointer (but prior), a prior descriptor that
 *   nnest_logprior_gauss refuses. */
int nnest_glm_curv_groups(int n, int D);
int nnest_glm_curv(const nnest_glm_t *glm, const double *theta_dev /*[D]*/, double *out_dev /*[1 + D + D*D]*/,
                   double *partials_dev /*[G][1 + D + D(D+1)/2]*/, int D, void *stream);
int nnest_glm_newton_solve(const double *curv_dev /* nnest_glm_curv's out */, const nnest_gauss_prior_t *prior /* NULL: none */,
                           const double *theta_dev, double *step_dev /*[D]*/, double *chol_dev /*[D*D]*/, double *info_dev /*[4]*/, int D,
                           void *stream);
/* IMPORTANCE-SAMPLED EVIDENCE with the trained flow as the proposal: Z = E_q[L(T(x)) pi(T(x)) / q(x)], drawn, evaluated and reduced
 * inside one kernel.  BUILD-DEFINED: the reference has no such estimator.  Sample m is a global 64-bit index; row k of a launch of M
 * samples is m = sample_offset + k:
 *   draws:   z_m[4g .. 4g+3] = the four Box-Muller normals of Philox(key seed; counter (g, m, 0, 7 << 28 | m >> 32)), with the
 *            arithmetic of nnest_mcmc_steps's normals (stream 7; streams 0-6 are taken);
 *   target:  lp(z_m), exactly the target of nnest_mcmc_steps: x = f^-1(z), ld = log|det dx/dz|, T(x) = x * t_std + t_mean in float32,
 *            logL = safe_loglike(T(x)), lp = (logL + ld) + prior, the prior 0 in the box [lo, hi] on T(x) (NaN inside), -inf outside;
 *   base:    N(0, I) only: logb(z) = -1/2 sum z_d^2 - (D / 2) log 2 pi, in float64 from the float32 z;
 *   weight:  logw_m = lp(z_m) - logb(z_m), float64.  A sample is LIVE when logw is neither NaN nor -inf; a dead one has weight 0;
 *   sums:    a = max logw over the live samples (-inf: none), S1 = sum exp(logw - a), S2 = sum exp(2 (logw - a)), n_live; float64,
 *            written as double sums_dev[4] = {a, S1, S2, n_live}.  (log Z over x is a + log S1 - log M; the ESS is S1^2 / S2.)
 * The reduction is deterministic and uses no floating-point atomics: each wave keeps a running (a, S1, S2), each workgroup writes one
 * partial into partials_dev, and a second, one-workgroup kernel combines the partials in index order; the live count is added up as
 * an integer.  The same call made twice returns bit-identical sums.  A sample's z, x, logL and logw are functions of (seed, m) only:
 * not of M, sample_offset, the grid, or whether the per-sample outputs were asked for; the sums of a run cut into launches and merged
 * on the host (a = max a_i, S1 = sum S1_i e^(a_i - a), S2 = sum S2_i e^(2 (a_i - a))) agree with the single launch's up to reordered
 * float64 addition.  The calls are asynchronous on `stream`.  (All added within ABI 15.)
 * nnest_importance_groups: the workgroups a launch of M samples uses (a persistent grid: ceil(M / tile), capped by a multiple of the
 *   CU count of the current device); tile = 4 (nnest_importance_evidence) or 16 (nnest_spline_importance_evidence); partials_dev
 *   holds 3 * groups doubles.  -1: a bad argument or no device.
 * nnest_importance_evidence: the shapes of nnest_mcmc_steps (hidden 16, 3 blocks, 1 layer, scale '', x_dim <= 128; like->scale is
 *   ignored); one sample per wave, four waves per workgroup, the weights loaded once per workgroup.  z_out_dev, x_out_dev [M,D],
 *   logl_out_dev, logw_out_dev [M]: the per-sample z, x = f^-1(z) (NOT T(x)), logL and logw, all four or all NULL (the sums only).
 *   t_std_dev, t_mean_dev [D], both or both NULL (T = identity); lo_dev, hi_dev [D], both or both NULL (no prior).  M = 0 .. 2^30;
 *   M = 0 is valid: the sums are {-inf, 0, 0, 0} and nothing else is written.  NNEST_E_UNSUPPORTED, before any launch: a
 *   GeneralisedNormal base (nnest_nvp_set_base with beta != 0), an unknown likelihood id, another shape.
 * nnest_spline_importance_evidence: the same through the neural-spline flow, on the team tile of nnest_spline_mcmc_steps and its
 *   shapes: 16 samples per workgroup and pass, four waves; rows >= M of the last tile evaluate their point and are neither counted nor
 *   written; the four waves hold identical sums and one of them publishes.
 * nnest_importance_fill_noise: the draws above as an array, through the kernels' own function: z_dev [M, D] float32.
 * nnest_importance_check, nnest_spline_importance_check: NNEST_OK where the entry takes this handle (its shape and base) and this
 *   likelihood id, else NNEST_E_UNSUPPORTED with the reason in nnest_hip_last_error(), as the entry itself would answer; nothing is
 *   launched: a front end asks before it chooses its route. */
int nnest_importance_groups(int M, int tile);
int nnest_importance_check(nnest_nvp_t *nvp, int like_id);
int nnest_spline_importance_check(struct nnest_spline *spl, int like_id);
int nnest_importance_evidence(nnest_nvp_t *nvp, const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev, const float *lo_dev,
                              const float *hi_dev, float *z_out_dev, float *x_out_dev, double *logl_out_dev, double *logw_out_dev,
                              double *partials_dev, double *sums_dev, int M, uint64_t seed, uint64_t sample_offset, void *stream);
int nnest_spline_importance_evidence(struct nnest_spline *spl, const nnest_like_t *like, const float *t_std_dev, const float *t_mean_dev,
                                     const float *lo_dev, const float *hi_dev, float *z_out_dev, float *x_out_dev, double *logl_out_dev,
                                     double *logw_out_dev, double *partials_dev, double *sums_dev, int M, uint64_t seed,
                                     uint64_t sample_offset, void *stream);
int nnest_importance_fill_noise(float *z_dev, int M, int D, uint64_t seed, uint64_t sample_offset, void *stream);
/* IMPORTANCE-SAMPLED EVIDENCE OF A REGRESSION: nnest_importance_evidence's estimate with the likelihood of a nnest_glm_t (logistic,
 * Poisson) in place of the analytic ones and, optionally, the normal priors of a nnest_gauss_prior_t in place of the box
 * (nnest_importance_glm.hip, nnest_spline_importance_glm.hip).  BUILD-DEFINED.  A sample is the importance sample above in every
 * respect but the target: the draws (stream 7, m = sample_offset + k: z_out_dev is bit-equal to nnest_importance_fill_noise), the
 * flow's inverse and T, the base, the weight logw = lp - logb, the sums, the partials (3 * nnest_importance_groups(M, tile) doubles,
 * tile 4 / 16), the two-stage reduction without floating-point atomics and the determinism are those stated there.
 *   logL:    the likelihood of nnest_mcmc_glm_steps on T(x), float64 terms from the float32 linear predictor in the layout's fixed
 *            order, rows >= n masked, -1e100 where the sum is not finite;
 *   prior:   prior NULL: 0 inside the box lo_dev / hi_dev on T(x) (NaN inside), -inf outside, or no box; prior given: log pi(T(x)) =
 *            logc - 1/2 ss of nnest_mcmc_glm_prior_steps, float64 in the layout's fixed order, -inf where ss is not finite; no box;
 *   lp:      (logL + ld) + prior, each operation rounded (nnest_mcmc_glm_prior_steps's target at beta = 1).
 * (Without a box and without a prior the sums are those of the likelihood's integral over R^D, which is no evidence and is infinite
 * for separable classes: a front end asks for a proper prior.)  Asynchronous on `stream`.  (All added within ABI 15.)
 * nnest_importance_glm_evidence: the shapes of nnest_importance_evidence; one sample per wave, the wave's 64 lanes take 64 data rows
 *   a pass; the prior's m and r in registers, loaded once a launch.
 * nnest_spline_importance_glm_evidence: the same through the neural-spline flow on the team tile: the four waves share the row
 *   blocks of the matrix-core product, rows >= M of the last tile evaluate their point and are neither counted nor written; the
 *   prior's m and r are staged once per workgroup in LDS; one wave publishes.
 * NNEST_E_ARG before any launch, the outputs untouched: everything nnest_importance_evidence refuses (M outside 0 .. 2^30; the
 *   per-sample outputs not all four or all NULL; NULL partials_dev or sums_dev; t_std_dev / t_mean_dev or lo_dev / hi_dev not both or
 *   neither), everything nnest_mcmc_glm_steps refuses of the descriptor, everything nnest_mcmc_glm_prior_steps refuses of the prior, a
 *   prior together with a box.  M = 0 is valid: the sums are {-inf, 0, 0, 0}.  NNEST_E_UNSUPPORTED: what the _check says.
 * nnest_importance_glm_check, nnest_spline_importance_glm_check: the verdict of nnest_importance_check /
 *   nnest_spline_importance_check on the handle's shape and base, and D == x_dim (NNEST_E_ARG otherwise); nothing is launched. */
int nnest_importance_glm_check(nnest_nvp_t *nvp, int D);
int nnest_spline_importance_glm_check(struct nnest_spline *spl, int D);
int nnest_importance_glm_evidence(nnest_nvp_t *nvp, const nnest_glm_t *glm, const nnest_gauss_prior_t *prior /* NULL: none */,
                                  const float *t_std_dev, const float *t_mean_dev, const float *lo_dev, const float *hi_dev,
                                  float *z_out_dev, float *x_out_dev, double *logl_out_dev, double *logw_out_dev, double *partials_dev,
                                  double *sums_dev, int M, uint64_t seed, uint64_t sample_offset, void *stream);
int nnest_spline_importance_glm_evidence(struct nnest_spline *spl, const nnest_glm_t *glm, const nnest_gauss_prior_t *prior /* NULL: none */,
                                         const float *t_std_dev, const float *t_mean_dev, const float *lo_dev, const float *hi_dev,
                                         float *z_out_dev, float *x_out_dev, double *logl_out_dev, double *logw_out_dev,
                                         double *partials_dev, double *sums_dev, int M, uint64_t seed, uint64_t sample_offset,
                                         void *stream);

/* SLICE PROPOSAL ON A REGRESSION: nnest_slice_steps's update -- directions, Philox uniforms noise_uniform(seed, walker, 64 step + k),
 * log y = log|det| + log u1, the bracket, the step-out budget with the random split, shrinkage, the counters and NNEST_MH_ALL_MOVED,
 * word for word -- with the likelihood of a nnest_glm_t (above: float32 eta in the layout's own order, float64 terms, rows >= n
 * masked, the safe rule -1e100) compiled in, one kernel per flow and family.  BUILD-DEFINED.  Two differences:
 *   logL(x) := GLM(T(x)), T(x)_d = x_d * t_std[d] + t_mean[d] in float32 without contraction (t_std_dev / t_mean_dev [D], both or
 *     neither; NULL: the identity);
 *   the likelihood is not evaluated where no decision depends on it: a candidate outside the box or below the slice level cannot be
 *     moved to and its logL is read by nothing (the spline tile skips only where none of its 16 walkers needs one).  No output shows it:
 *     n_eval_dev counts every candidate, n_call_dev those that passed the box and the slice level.
 * The box is on x (!(x < -1 || x > 1), a NaN coordinate inside), as in nnest_slice_steps -- not on T(x).  The other arguments are
 * nnest_slice_steps's (max_stepout 0..2^24, max_shrink 1..60, width > 0; the counters may each be NULL); the descriptor is checked
 * as everywhere (its D against the flow's x_dim, family, n <= 65536: NNEST_E_ARG).  The NVP runs one walker per wave, the spline flow
 * its team tile (four waves per 16 walkers, the only form); no cross-workgroup wait: any C.
 * nnest_slice_glm_check, nnest_spline_slice_glm_check: NNEST_OK where the entry takes this handle's shape (the NVP: hidden 16, 3
 * blocks, 1 layer, scale '', x_dim <= 128; the spline flow: the team tile's shapes) and a descriptor of dimension D, else
 * NNEST_E_UNSUPPORTED / NNEST_E_ARG with the reason in nnest_hip_last_error; nothing is launched.  Other flows and shapes run the
 * same definition through nnest_slice_rounds_* with nnest_loglike_glm between the launches.  (All added within ABI 15.) */
int nnest_slice_glm_check(nnest_nvp_t *nvp, int D);
int nnest_spline_slice_glm_check(struct nnest_spline *spl, int D);
int nnest_slice_glm_steps(nnest_nvp_t *nvp, const nnest_glm_t *glm, const float *t_std_dev, const float *t_mean_dev, float *z_dev,
                          float *x_dev, double *logl_dev, double loglstar, float width, int steps, int C, int max_stepout, int max_shrink,
                          const float *noise_dz_dev, uint64_t seed, uint64_t walker_offset, float *hist_x_dev, int *n_call_dev,
                          int *n_move_dev, int *n_eval_dev, void *stream);
int nnest_spline_slice_glm_steps(struct nnest_spline *spl, const nnest_glm_t *glm, const float *t_std_dev, const float *t_mean_dev,
                                 float *z_dev, float *x_dev, double *logl_dev, double loglstar, float width, int steps, int C,
                                 int max_stepout, int max_shrink, const float *noise_dz_dev, uint64_t seed, uint64_t walker_offset,
                                 float *hist_x_dev, int *n_call_dev, int *n_move_dev, int *n_eval_dev, void *stream);

/* METROPOLIS PROPOSAL ON A REGRESSION: nnest_mh_constrained_steps's hard-constraint step (sampler.py:229-463) -- fs = (float)scale,
 * z' = z + eps * fs in float32 (a product and a sum), x' = f^-1(z'), log_ratio = inbox(x') ? ld' - ld : -inf, ratio =
 * min(exp(log_ratio), 1) with a NaN kept, pre = u < ratio, acc = pre && logL' > loglstar; n_call_dev counts pre, n_accept_dev counts acc
 * with NNEST_MH_ALL_MOVED in bit 30 -- with the likelihood of a nnest_glm_t (above: float32 eta in the layout's own order, float64
 * terms, rows >= n masked, the safe rule -1e100) compiled in, one kernel per flow and family.  BUILD-DEFINED.
 *   logL(x) := GLM(T(x)), T(x)_d = x_d * t_std[d] + t_mean[d] in float32 without contraction (t_std_dev / t_mean_dev [D], both or
 *     neither; NULL: the identity).  The box is on x (!(x < -1 || x > 1), a NaN coordinate inside) -- not on T(x).
 *   Draws: eps[4g .. 4g+3] = Philox normals of (seed, walker_offset + row, step 1.., g) on stream DZ (what nnest_slice_fill_noise
 *     exports), padded dimensions exactly 0; u = the Philox uniform of (seed, walker, step) on stream U (24 bits).  A chain is a
 *     function of seed, walker and step (and of the votes under a step rule).  noise_dz_dev [steps, C, D] and noise_u_dev [steps, C],
 *     both or neither, replace them.  hist_x_dev [C, steps + 1, D], hist_logl_dev [C, steps + 1]: optional.
 *   The likelihood is not evaluated where nothing reads it: a proposal with pre false is rejected whatever its logL (the spline tile
 *     skips only where none of its 16 walkers has pre).  No output shows it.
 *   flags: 0 (fixed step) | NNEST_MH_DYNAMIC_BATCH | NNEST_MH_LAG(0..15) (the reference's rule over all C walkers; the vote of step s
 *     applies from step s + 1 + lag on; sync_dev: nnest_mh_sync_words(steps) words, ZERO at the launch, the last one the error word
 *     of a bounded wait that ran out) | NNEST_MH_DYNAMIC_STEP, the spline entry only (the rule per 16-walker tile, any C).  Anything
 *     else -- NNEST_MH_UNCONSTRAINED (that walk is nnest_mcmc_glm_steps), NNEST_MH_WARM, form bits, the sync halves -- is NNEST_E_ARG.
 *   The batch rule needs every workgroup resident: a grid beyond the kernel's occupancy times the device's CUs is refused with
 *     NNEST_E_UNSUPPORTED and nothing is launched.  scale_out_dev: one float per workgroup (4 walkers: the NVP; 16: the spline flow).
 * The descriptor is checked as everywhere (NNEST_E_ARG).  The NVP runs one walker per wave (hidden 16, 3 blocks, 1 layer, scale '',
 * x_dim <= 128), the spline flow its team tile.  nnest_mh_glm_check, nnest_spline_mh_glm_check: NNEST_OK where the entry takes this
 * handle's shape, a descriptor of dimension D, C walkers and this flags word (the residency verdict included), else the code and
 * the reason in nnest_hip_last_error; nothing is launched.  (All added within ABI 15.) */
int nnest_mh_glm_check(nnest_nvp_t *nvp, int D, int C, int flags);
int nnest_spline_mh_glm_check(struct nnest_spline *spl, int D, int C, int flags);
int nnest_mh_glm_steps(nnest_nvp_t *nvp, const nnest_glm_t *glm, const float *t_std_dev, const float *t_mean_dev, float *z_dev,
                       float *x_dev, double *logl_dev, double loglstar, float step_size, int steps, int C, int flags,
                       const float *noise_dz_dev, const float *noise_u_dev, uint64_t seed, uint64_t walker_offset, float *hist_x_dev,
                       double *hist_logl_dev, int *n_accept_dev, int *n_call_dev, float *scale_out_dev, void *sync_dev, void *stream);
int nnest_spline_mh_glm_steps(struct nnest_spline *spl, const nnest_glm_t *glm, const float *t_std_dev, const float *t_mean_dev,
                              float *z_dev, float *x_dev, double *logl_dev, double loglstar, float step_size, int steps, int C,
                              int flags, const float *noise_dz_dev, const float *noise_u_dev, uint64_t seed, uint64_t walker_offset,
                              float *hist_x_dev, double *hist_logl_dev, int *n_accept_dev, int *n_call_dev, float *scale_out_dev,
                              void *sync_dev, void *stream);
/* size of sync_dev in 8-byte words for a launch of `steps` steps */
int nnest_mh_sync_words(int steps);
/* number of adaptation groups nnest_mh_constrained_steps uses for C walkers (size of scale_out_dev) */
int nnest_mh_num_groups(const nnest_nvp_t *nvp, int C);

/* The in-kernel proposal noise as arrays, for tests: dz[steps,C,D] ~ N(0,1), u[steps,C] ~ U[0,1),
 * bit-identical to what nnest_mh_constrained_steps draws for (seed, walker_offset). */
int nnest_mh_fill_noise(float *dz_dev, float *u_dev, int steps, int C, int D, uint64_t seed, uint64_t walker_offset,
                        void *stream);

/* Trainer.train's epoch loop (trainer.py:198-232) inside one launch: for each epoch, Trainer._train
 * (trainer.py:384-403: minibatches of `batch` rows in the order perm_dev[epoch], data + jitter*noise,
 * loss = -mean(log_probs), backward, Adam with coupled weight decay) then Trainer._validate
 * (trainer.py:405-418), early stopping with `patience` and best-model restore (trainer.py:205-209, :241).
 *   xtrain_dev [n_train,D], xvalid_dev [n_valid,D] float32
 *   perm_dev [max_epochs, n_train] int32 (DataLoader shuffle order per epoch, trainer.py:185)
 *   noise_dev  NULL -> in-kernel normals, one Philox4x32-10 block + Box-Muller per (seed; position of the row in the epoch's
 *              order, epoch_offset + epoch, group of four dims) -- no stream state: any kernel form draws the same jitter;
 *              else [max_epochs, n_train, D]
 *              in perm order (torch.randn_like(data), trainer.py:392)
 *   losses_dev optional float32 [max_epochs, 2]: (train, validation) loss per epoch, normalised as the
 *              reference logs them (/len(dataset), trainer.py:403, :418)
 *   result_dev see nnest_train_result_t (device memory; in/out when NNEST_TRAIN_RESUME is set)
 *   epoch_offset, flags: a long train() may be issued as several launches ("chunks") so that the shuffle
 *              table stays small: chunk k passes epoch_offset = epochs already run and NNEST_TRAIN_RESUME,
 *              which continues the early-stopping state held in result_dev and the best-weights snapshot;
 *              NNEST_TRAIN_FINALIZE (last chunk) restores the best-validation weights (trainer.py:241); that
 *              restore also happens whenever patience runs out.  A single-launch train() passes
 *              epoch_offset 0 and flags = NNEST_TRAIN_FINALIZE.
 * Adam moments and step count persist in the handle across calls (optimizer is created once,
 * trainer.py:121-122).
 * Returns NNEST_E_UNSUPPORTED for batch > 128, for a MAF handle, and where min(batch, n_train) is more rows than one workgroup can
 * stage: 96 at hidden_dim 64 with two hidden layers, 64 with three, 112 at hidden_dim 32 with three and x_dim > 32.  Such an epoch
 * loop is driven from the host: nnest_nvp_loss_grad, which splits a batch over launches, and nnest_nvp_adam_step per minibatch.
 */
typedef struct {
    int epochs_run;             /* total epochs run so far (including previous chunks) */
    int best_epoch;             /* 1-based epoch of the best validation loss (trainer.py:206) */
    float best_validation_loss;
    float last_train_loss;
    int counter;                /* epochs since the last improvement (trainer.py:209, :223) */
    int stopped;                /* 1 when counter > patience ended the run (trainer.py:225); 2: internal error (a bounded grid
                                 * barrier of the multi-CU kernel ran out: results invalid) */
} nnest_train_result_t;

enum { NNEST_TRAIN_RESUME = 1, NNEST_TRAIN_FINALIZE = 2,
       NNEST_TRAIN_ONE_CU = 4 /* keep the epoch loop on ONE workgroup (the round-1 kernel) instead of one workgroup per 16-row tile
                               * of the minibatch on eight compute units; both produce the same bits (A/B and test switch) */ };

int nnest_nvp_train(nnest_nvp_t *nvp, const float *xtrain_dev, int n_train, const float *xvalid_dev, int n_valid,
                    const int *perm_dev, const float *noise_dev, uint64_t seed, float jitter, int batch,
                    int max_epochs, int patience, float lr, float weight_decay, int epoch_offset, int flags,
                    float *losses_dev, nnest_train_result_t *result_dev, void *stream);
/* nnest_nvp_train_form (added within ABI 15): the kernel nnest_nvp_train runs the epoch loop in for minibatches of `batch` rows and
 * these `flags`, from the predicates of the launch itself -- 0: train_kernel, one workgroup (*detail = how many of its two fragment
 * images live in LDS: 2, 1 or 0); 1: train_kernel_grid, eight workgroups (*detail = 10 NT + L, NT = ceil(x_dim / 32), L = num_layers);
 * 2: train_kernel_rows, one workgroup per four rows (*detail = U = NT).  -1: nnest_nvp_train refuses the call (batch outside
 * [1, 128], a MAF handle, or more rows than one workgroup can stage, as stated above: nnest_nvp_loss_grad and nnest_nvp_vjp split
 * such a batch over launches, the one-launch epoch loop cannot).  detail may be NULL. */
int nnest_nvp_train_form(const nnest_nvp_t *nvp, int batch, int flags, int *detail);

/* One minibatch: loss and dloss/dw (before weight decay) into grad_dev [num_params], no update.
 * For tests (reference: loss.backward(), trainer.py:400). x_dev [M,D]. loss_dev float32[1]. */
int nnest_nvp_loss_grad(nnest_nvp_t *nvp, const float *x_dev, int M, float *grad_dev, float *loss_dev, void *stream);

/* The flow as one stage of a composite model (FastSlowNormalizingFlowModel, networks.py:86-150): vector-Jacobian product
 * of one batch (M <= 128 rows).  With L = sum_rows gz . f(x) + gld * sum_rows logdet(x):  grad_dev = dL/dw (packed order),
 * gx_dev = dL/dx [M,D]. */
int nnest_nvp_vjp(nnest_nvp_t *nvp, const float *x_dev, const float *gz_dev, float gld, int M, float *grad_dev, float *gx_dev,
                  void *stream);
/* one torch.optim.Adam step (coupled weight decay, trainer.py:121-122) from a gradient computed outside nnest_nvp_train;
 * uses and advances the handle's Adam state (the step counter lives on the device: asynchronous on `stream`, like the passes) */
int nnest_nvp_adam_step(nnest_nvp_t *nvp, const float *grad_dev, float lr, float weight_decay, void *stream);
/* MAF handles (nnest_maf_create): one epoch of Trainer._train (trainer.py:384-403) queued by ONE call -- per minibatch of `batch`
 * (<= 128) consecutive rows of rows_dev [n_train, D] (the caller has applied the epoch's permutation and jitter): loss + gradient,
 * one Adam step (coupled weight decay), image rebuild; *loss_sum_dev += the minibatch's loss (the reference's running sum of
 * loss.item(), trainer.py:402).  Asynchronous on `stream`; nothing is read back. */
int nnest_maf_train_epoch(nnest_nvp_t *nvp, const float *rows_dev, int n_train, int batch, float lr, float weight_decay,
                          float *loss_sum_dev, void *stream);

/* training jitter when jitter < 0 (trainer.py:168-171): 0.2 * mean of the 2-nearest-neighbour distance
 * table (self distance 0 included) of samples_dev [N,D] float64; result to out_dev float64[1]. */
int nnest_training_jitter(const double *samples_dev, int N, int D, double *out_dev, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Neural-spline flow: SingleSpeedSpline(num_inputs=D, hidden_dim=H, num_blocks=B, num_bins=K, tail_bound)
 * (networks.py:708-715) = [ActNorm (:661-705), Invertible1x1Conv (:625-658), NSF_CL (:559-622)] x B.
 * Packed weights = the concatenated state_dict: per block  s[D] t[D] | L[D,D] S[D] U[D,D] |
 *   f1.net.{0,2,4,6}.{weight,bias} | f2.net.{0,2,4,6}.{weight,bias}.
 * perm = the B fixed permutation matrices P [B,D,D] of the 1x1 convolutions (networks.py:634-635: a plain attribute
 * of the reference module, NOT in its state_dict); identity until loaded.
 * Same calling conventions as the nnest_nvp_* functions they parallel.  num_bins must be 8 (the reference's value).
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct nnest_spline nnest_spline_t;
int nnest_spline_create(int D, int H, int B, int K, float tail_bound, nnest_spline_t **out);
int nnest_spline_destroy(nnest_spline_t *spl);
int nnest_spline_num_params(const nnest_spline_t *spl);
int nnest_spline_set_base(nnest_spline_t *spl, float beta);   /* as nnest_nvp_set_base */
int nnest_spline_load_weights(nnest_spline_t *spl, const float *packed_host, const float *perm_host, void *stream);
int nnest_spline_store_weights(nnest_spline_t *spl, float *packed_host, float *perm_host, void *stream);
/* NormalizingFlow.forward / .inverse (networks.py:24-42), NormalizingFlowModel.log_probs (networks.py:71-76) */
int nnest_spline_forward(nnest_spline_t *spl, const float *x_dev, float *z_dev, float *logdet_dev, int N, void *stream);
int nnest_spline_inverse(nnest_spline_t *spl, const float *z_dev, float *x_dev, float *logdet_dev, int N, void *stream);
int nnest_spline_log_probs(nnest_spline_t *spl, const float *x_dev, float *logp_dev, int N, void *stream);
int nnest_spline_inverse_loglike(nnest_spline_t *spl, const nnest_like_t *like, const float *z_dev, float *x_dev,
                                 float *logdet_dev, double *logl_dev, int *inbox_dev, int N, void *stream);
/* Sampler._mcmc_sample (sampler.py:229-463) with the spline inverse: arguments as nnest_mh_constrained_steps.  Kernel forms (chosen
 * by the library; the walkers' results do not depend on the form beyond float32 rounding): one wave per 16 walkers at large
 * populations; four waves per 16-walker tile while the tiles fit two per CU; four waves per EIGHT walkers (each held in both
 * halves of the matrix-core columns: one spline evaluation per lane serves two groups of four dimensions) at x_dim > 32 under a
 * fixed step or NNEST_MH_DYNAMIC_BATCH while those tiles fit one per CU.  scale_out_dev has one entry per 16 walkers in every form. */
int nnest_spline_mh_constrained_steps(nnest_spline_t *spl, const nnest_like_t *like, float *z_dev, float *x_dev,
                                      double *logl_dev, double loglstar, float step_size, int steps, int C, int flags,
                                      const float *noise_dz_dev, const float *noise_u_dev, uint64_t seed,
                                      uint64_t walker_offset, float *hist_x_dev, double *hist_logl_dev, int *n_accept_dev,
                                      int *n_call_dev, float *scale_out_dev, void *sync_dev, void *stream);

/* The form of the proposal kernel nnest_spline_mh_constrained_steps runs for C walkers under `flags` (the three above), -1 if the
 * launch would be refused (the batch-wide rule on a grid that is not resident).  (Added within ABI 15.) */
enum { NNEST_SPLINE_MH_WAVE = 0, NNEST_SPLINE_MH_TEAM = 1, NNEST_SPLINE_MH_PAIR = 2 };
int nnest_spline_mh_form_for(const nnest_spline_t *spl, int C, int flags);

/* SLICE proposal in latent space with the spline flow: the definition, streams and counters of nnest_slice_steps (BUILD-DEFINED,
 * parity unpinned: the reference has no slice proposal; held to oracle/oracle.py::slice_sample) with the spline's inverse and
 * log-det in place of the NVP's -- the stepping-out budget of 2 max_stepout expansions and its random split included.
 * Arguments as nnest_slice_steps; n_call_dev, n_move_dev, n_eval_dev may each be NULL.  The
 * directions are the ones nnest_slice_fill_noise exports.  Kernel forms as the spline proposal kernel's: 16 walkers per wave,
 * four waves per 16 walkers, four waves per 8 walkers held twice (x_dim > 32); walkers are not held in step (each evaluates its
 * own next candidate in every round of the tile; one that has finished idles), so any C, no resident-grid requirement.  flags:
 * bits 0..3 pin a form, NNEST_SPLINE_SLICE_FORM(NNEST_SPLINE_MH_WAVE / _TEAM / _PAIR), 0 = NNEST_SPLINE_SLICE_AUTO lets the
 * library choose; the forms agree to float32 rounding.  Shapes: those of nnest_spline_mh_constrained_steps (hidden 16 up to
 * x_dim 128, hidden 32 up to x_dim 64); NNEST_E_UNSUPPORTED for a pinned form the shape lacks.  (Added within ABI 15.) */
enum { NNEST_SPLINE_SLICE_AUTO = 0 };
#define NNEST_SPLINE_SLICE_FORM(f) (((f) + 1) & 15)
int nnest_spline_slice_steps(nnest_spline_t *spl, const nnest_like_t *like, float *z_dev, float *x_dev, double *logl_dev,
                             double loglstar, float width, int steps, int C, int max_stepout, int max_shrink, int flags,
                             const float *noise_dz_dev, uint64_t seed, uint64_t walker_offset, float *hist_x_dev, int *n_call_dev,
                             int *n_move_dev, int *n_eval_dev, void *stream);
/* The form (NNEST_SPLINE_MH_WAVE / _TEAM / _PAIR) nnest_spline_slice_steps runs for C walkers under `flags`, -1 if it would refuse
 * the launch.  (Added within ABI 15.) */
int nnest_spline_slice_form_for(const nnest_spline_t *spl, int C, int flags);

/* Training.  ActNorm's data-dependent initialisation (networks.py:698-705): s = -log std(x) (unbiased), t = -mean(x e^s)
 * block after block from the batch x_dev [N,D] -- in the reference this happens inside the first forward pass of a
 * fresh model, which under Trainer.train is the first (jittered) minibatch. */
int nnest_spline_actnorm_init(nnest_spline_t *spl, const float *x_dev, int N, void *stream);
/* loss = -mean(log_probs(x)) and its gradient wrt the packed weights (loss.backward(), trainer.py:394-400) */
int nnest_spline_loss_grad(nnest_spline_t *spl, const float *x_dev, int M, float *grad_dev, float *loss_dev, void *stream);
/* Trainer.train's epoch loop (trainer.py:198-241) as nnest_nvp_train, except that the loop is driven from the host
 * (two launches per minibatch, the epoch's books kept on the device): losses_host [max_epochs,2] and result_host are HOST
 * pointers, the best-validation weights are restored on return and the call synchronises `stream`.  The Adam moments
 * persist across calls like torch.optim.Adam's state.
 * nnest_spline_train_form (added within ABI 15): the form a minibatch of `batch` rows runs in -- 1: one row per workgroup, the
 * evaluation on eight lanes per item, weight gradients contracted over the rows (nnest_spline_rows.hip: hidden_dim 16, x_dim <= 64,
 * batch <= 128); 0: sixteen / eight rows per workgroup of four waves (nnest_spline_train.hip).  Both follow the same reference
 * arithmetic; they agree to rounding, not to the bit.  NNEST_SPL_ROWS=0 in the environment pins form 0. */
int nnest_spline_train_form(const nnest_spline_t *spl, int batch);
/* the spline flow as one stage of a composite model (FastSlowSpline, networks.py:718-731): as nnest_nvp_vjp / nnest_nvp_adam_step */
int nnest_spline_vjp(nnest_spline_t *spl, const float *x_dev, const float *gz_dev, float gld, int M, float *grad_dev, float *gx_dev,
                     void *stream);
int nnest_spline_adam_step(nnest_spline_t *spl, const float *grad_dev, float lr, float weight_decay, void *stream);
int nnest_spline_train(nnest_spline_t *spl, const float *xtrain_dev, int n_train, const float *xvalid_dev, int n_valid,
                       const int *perm_dev, const float *noise_dev, uint64_t seed, float jitter, int batch, int max_epochs,
                       int patience, float lr, float weight_decay, float *losses_host, nnest_train_result_t *result_host,
                       void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Chain statistics of a batch of MCMC histories x[C, T, D] (float32; element (i, j, d) at x_dev[i * chain_stride + j * step_stride
 * + d], so a prefix [:, :t] of a longer history and the [C, steps + 1, D] history of nnest_mh_constrained_steps are read in place)
 * -- nnest/utils/evaluation.py and Sampler._chain_stats, nnest/sampler.py:474-492, with the reference's definitions (float64
 * sums; f32 products in the lag sums):
 *   v = x, or x * a + b per dimension when affine_dev [2, D] float64 = (a, b) is given (the reference's T(x) = x * std + mean)
 *   acceptance   #{(i, j): j = 1..T-1, v[i,j] != v[i,j-1] in at least one coordinate} / (C (T - 1))   (an exact count)
 *   jump         sum_i sum_j ||v[i,j] - v[i,j-1]||_2 / (C (T - 1))
 *   mu, sd       mean_dev / std_dev when given, else the mean and population std (ddof 0) over all C T rows
 *   p_s[d]       (1 / C) sum_i mean_{j<T-s} (v[i,j,d] - mu_d)(v[i,j+s,d] - mu_d) / sd_d       -- divided by the STANDARD DEVIATION,
 *                as the reference (sampler.py:480 passes std into evaluation.py:17's `var`)
 *   ESS          e_d = 1; for s = 1 .. T-1: stop if no d has p_s[d] > 0.05, else e_d += 2 p_s[d] (1 - s / T) for every d with
 *                p_s[d] > 0.05 (the stop is global over d); ESS_d = T / e_d
 *   R-hat        (C > 1; NaN for C = 1) theta_i / sigma2_i = mean / variance of chain i over the steps, theta_bar = mean_i theta_i
 *                (mu with NNEST_CHAIN_STATS_RHAT_AT_MEAN), B = T / (C - 1) sum_i sum_d (theta_i - theta_bar)^2 (ONE number: the
 *                reference's np.sum has no axis, evaluation.py:88),
 *                W = 1 / (C sum_i sigma2_i + 1e-5), V = (T - 1) / T W + (C + 1) / (C T) B, R-hat = sqrt(V / W)   (evaluation.py:77-93)
 * Any C >= 1, T >= 2, D >= 1.  Every call is asynchronous on `stream` and bitwise repeatable (fixed-order sums, no float atomics).
 * work_dev: float64 scratch of nnest_chain_stats_work_words(C, T, D) words (-1: bad shape), reused across the calls of one batch.
 *
 * nnest_chain_stats: all of it.  out_dev [4 + 4 D] float64 = acceptance, jump, stop lag (the s at which the ESS sum stopped; T if it
 *   never did), C, then ESS[D], R-hat[D], mu[D], sd[D].  p_dev (optional) [T - 1, D]: p_s in row s - 1 for every lag computed.
 *   Lags are computed in blocks of 256, 256, 512, 1024, 2048, 2048, ...; a block after the stop lag costs its launches only.
 *   flags: NNEST_CHAIN_STATS_ALL_LAGS computes (and writes to p_dev) every lag; NO_ESS skips the lags (ESS and stop lag NaN).
 * The stages, for a batch sharded over devices: the chain sums [3 + 3 D] (accepted pairs, jump sum, C, sum_i (theta_i - c)[D],
 *   sum_i (theta_i - c)^2[D], sum_i sigma2_i[D]) and the lag sums [nlags, D] (sum_i sum_{j<T-s} y y) are ADDITIVE over shards:
 *   all-reduce them between the stages.  c = center_dev [D] of nnest_chain_stats_chains -- the same on every shard (the mean passed
 *   to prepare will do) -- or, when NULL, the first chain's theta of the call (one shard only); the centring keeps the moments
 *   exact when the chain means are large compared with their spread.  chains -> (all-reduce) -> prepare (with the global C) -> for each lag block: lags -> (all-reduce) ->
 *   advance -> finish.  nlags: a multiple of 256 up to 2048. */
enum { NNEST_CHAIN_STATS_ALL_LAGS = 1, NNEST_CHAIN_STATS_NO_ESS = 2, NNEST_CHAIN_STATS_RHAT_AT_MEAN = 4 };
int nnest_chain_stats_work_words(int C, int T, int D);
/* emcee's normalised autocorrelation function of walkers x[C, T, D] (emcee 3 autocorr.integrated_time with has_walkers; read in
 * place through the strides, as above): f_dev [T, D] float64, f(s, d) = SUM_k acf_k(s) / acf_k(0) over the walkers -- the caller
 * divides by C -- with acf_k(s) = sum_{t < T - s} (x_kt - m_k)(x_k,t+s - m_k), m_k the walker's OWN mean over T, not divided by
 * T - s.  A direct float64 sum over every lag 0 .. T - 1.  tau = 2 cumsum(f / C) - 1 at Sokal's window is the caller's
 * (nnest_amd.evaluation.integrated_autocorr_time).  This is NOT the estimator of nnest_chain_stats (global mean, divided by the
 * standard deviation, global stop).  work_dev: float64 scratch of nnest_chain_autocorr_work_words(C, T, D) words (-1: bad
 * shape).  (Added within ABI 15.) */
int nnest_chain_autocorr_work_words(int C, int T, int D);
int nnest_chain_autocorr(const float *x_dev, int C, int T, int D, long long chain_stride, long long step_stride, double *work_dev,
                         double *f_dev, void *stream);
int nnest_chain_stats(const float *x_dev, int C, int T, int D, long long chain_stride, long long step_stride, const double *affine_dev,
                      const double *mean_dev, const double *std_dev, int flags, double *work_dev, double *p_dev, double *out_dev,
                      void *stream);
int nnest_chain_stats_chains(const float *x_dev, int C, int T, int D, long long chain_stride, long long step_stride,
                             const double *affine_dev, const double *center_dev, double *work_dev, double *chain_sums_dev,
                             void *stream);
int nnest_chain_stats_prepare(const double *chain_sums_dev, int C, int T, int D, const double *mean_dev, const double *std_dev,
                              double *work_dev, void *stream);
int nnest_chain_stats_lags(const float *x_dev, int C, int T, int D, long long chain_stride, long long step_stride,
                           const double *affine_dev, int lag0, int nlags, int flags, double *work_dev, double *lag_sums_dev,
                           void *stream);
int nnest_chain_stats_advance(const double *chain_sums_dev, const double *lag_sums_dev, int C, int T, int D, int lag0, int nlags,
                              int flags, double *work_dev, double *p_dev, void *stream);
int nnest_chain_stats_finish(const double *chain_sums_dev, int C, int T, int D, int flags, double *work_dev, double *out_dev,
                             void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * 'choleksy' flow: SingleSpeedCholeksy(num_inputs=D) (networks.py:162-239): y = L x + b, L lower triangular with
 * diag = softplus(unconstrained_diag) + 1e-3.  Packed weights = state_dict order: bias[D], lower_entries[D(D-1)/2]
 * (np.tril_indices(D, -1) order), unconstrained_diag[D].  Conventions as the nnest_nvp_* functions.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct nnest_chol nnest_chol_t;
int nnest_chol_create(int D, nnest_chol_t **out);
int nnest_chol_destroy(nnest_chol_t *chol);
int nnest_chol_num_params(const nnest_chol_t *chol);
int nnest_chol_set_base(nnest_chol_t *chol, float beta);
int nnest_chol_load_weights(nnest_chol_t *chol, const float *packed_host, void *stream);
int nnest_chol_store_weights(nnest_chol_t *chol, float *packed_host, void *stream);
int nnest_chol_forward(nnest_chol_t *chol, const float *x_dev, float *z_dev, float *logdet_dev, int N, void *stream);
int nnest_chol_inverse(nnest_chol_t *chol, const float *z_dev, float *x_dev, float *logdet_dev, int N, void *stream);
int nnest_chol_log_probs(nnest_chol_t *chol, const float *x_dev, float *logp_dev, int N, void *stream);
int nnest_chol_loss_grad(nnest_chol_t *chol, const float *x_dev, int M, float *grad_dev, float *loss_dev, void *stream);
int nnest_chol_adam_step(nnest_chol_t *chol, const float *grad_dev, float lr, float weight_decay, void *stream);

/* Host-side (no GPU involved): the rows of a chain file in the reference's text format -- Sampler._save_samples,
 * nnest/sampler.py:494-511: np.savetxt(fmt='%.5E'): '%.5E' numbers separated by one space, '\n' after every row -- into out_host
 * (capacity >= 14 * n_rows * n_cols + 1 bytes); formatted on `threads` host threads.  Returns the number of bytes written, -1 on
 * a bad argument. */
long nnest_format_rows_e5(const double *rows_host, long n_rows, int n_cols, char *out_host, long out_cap, int threads);

/* Host-side (no GPU involved): the rows "<tag>,<step>,<value>\n" of the scalar log (utils.ScalarWriter, which stands where the
 * reference keeps trainer.writer.add_scalar, nnest/nested.py:467) for a run of steps, the value written as Python's repr(float)
 * writes it (the shortest digits that read back to the same double, ".0" after an integral value, exponent form below 1e-4 and
 * from 1e16, "nan" / "inf").  out_host: capacity >= n * (strlen(tag) + 48) + 1 bytes.  Returns the number of bytes written, -1 on
 * a bad argument.  (Added within ABI 15: host-only, nothing else changed.) */
long nnest_format_scalar_rows(const char *tag, const long long *steps_host, const double *values_host, long n, char *out_host,
                              long out_cap);

/* Host-side (no GPU involved): the per-iteration body of the nested-sampling loop while the MCMC strategy is in force --
 * NestedSampler.run, nnest/nested.py:269-293 (worst live point, evidence update, dead-point append), :429-437 (consume the next
 * usable chain of the batch), :458-471 (volume shell, remaining-evidence test) -- as ONE call per event instead of ~7 us of
 * interpreter per iteration (2e5 iterations in a BASELINE config-2 run).  The loop returns to the caller whenever the reference
 * does something that is not this arithmetic, with the reason:
 *   NNEST_HOST_FINISHED      fraction_remain <= dlogz or it > max_iters (nested.py:269)
 *   NNEST_HOST_RETRAIN       first pass, or it % update_interval == 0 at the top of a pass (nested.py:311-314): train, then call
 *                            again with resume = NNEST_HOST_AFTER_TRAIN
 *   NNEST_HOST_NEED_SAMPLES  the batch is used up (nested.py:399): run the chains from loglstar (state.loglstar), hand over the new
 *                            endpoints, nb = 0, resume = NNEST_HOST_AFTER_SAMPLES
 *   NNEST_HOST_LOG           a point was accepted at it > 0, it % log_interval == 0 (nested.py:439-456, before `it` advances):
 *                            log, then resume = NNEST_HOST_AFTER_LOG
 *   NNEST_HOST_CHECKPOINT    `it` has just advanced to a multiple of log_interval (nested.py:473-485); resume = NNEST_HOST_TOP
 *   NNEST_HOST_DEAD_FULL     the dead-point buffers are full: grow them, resume = NNEST_HOST_TOP (nothing was changed)
 * Arithmetic: float64, the reference's operations in the reference's order; log Z by logaddexp as numpy computes it (libm exp /
 * log1p).  The information H is NOT updated here (numpy's vectorised exp is not libm's): per dead point the loop records log Z
 * before the update (dead_logz_prev), the caller forms the two exponentials with numpy and nnest_host_h_update runs the recurrence.
 * Dead point k: row dead_v[k] = [v (D) | derived (nd)], dead_logl[k], dead_logwt[k], dead_logz_prev[k]. */
enum { NNEST_HOST_FINISHED = 0, NNEST_HOST_RETRAIN = 1, NNEST_HOST_NEED_SAMPLES = 2, NNEST_HOST_LOG = 3, NNEST_HOST_CHECKPOINT = 4,
       NNEST_HOST_DEAD_FULL = 5 };
enum { NNEST_HOST_TOP = 0, NNEST_HOST_AFTER_TRAIN = 1, NNEST_HOST_AFTER_SAMPLES = 2, NNEST_HOST_AFTER_LOG = 3 };
typedef struct {
    double logz, logvol, fraction_remain, max_logl, loglstar;
    long long it, n_dead;
    int accept_point, nb, first_time, resume, worst, pad_;
} nnest_host_state_t;
int nnest_host_mcmc_consume(nnest_host_state_t *state, int N, int D, int nd, double *active_u, double *active_v, double *active_logl,
                            double *active_derived, const double *end_u, const double *end_v, const double *end_logl,
                            const unsigned char *moved, const double *end_derived, int C, double *dead_v, double *dead_logl,
                            double *dead_logwt, double *dead_logz_prev, long long dead_cap, double dlogz, long long max_iters,
                            long long update_interval, long long log_interval);
/* The same loop while 'rejection_prior' is the strategy in force (nnest/nested.py:322-334, :362-373 over
 * Sampler._rejection_prior_sample, nnest/sampler.py:529-543): the reference draws one prior sample per likelihood call until one lies
 * above loglstar; the draws are independent, so the caller evaluates them a block per launch and hands over the block's candidates
 * -- the indices (ascending) that were above the threshold when the block was made, cand_logl32 (the kernel's likelihood of
 * float32(x)) and cand_logl64 (the reference's float64 one) per candidate, their rows cand_u / transformed rows cand_v [n_cand, D],
 * derived [n_cand, nd].  Candidates are examined in order, each once; an iteration's call count is the number examined up to and
 * including the accepted one (blocks used up without a hit carry over in pending_calls).  Returns as nnest_host_mcmc_consume, plus
 *   NNEST_HOST_NEED_SAMPLES  no block / block used up: make one of prior.block_next draws, set prior.n / n_cand / pos = k = hits = 0,
 *                            resume = NNEST_HOST_AFTER_SAMPLES
 *   NNEST_HOST_EXPIRED       the strategy expired in the pass before (volume_switch, or the last 20 call counts average more than
 *                            mcmc_steps and MCMC is available: nested.py:328-334); nothing of the next pass has been done.
 * NNEST_HOST_LOG here is nested.py:374-378 ((it + 1) % log_interval == 0).  (Added within ABI 15: host-only.) */
enum { NNEST_HOST_EXPIRED = 6 };
typedef struct {
    long long pos, k, hits, n, n_cand;   /* the walk through the current block */
    long long pending_calls;             /* candidates examined since the last accepted one, in blocks used up */
    long long total_calls;               /* Sampler.total_calls (sampler.py:119) */
    long long block_next;                /* size of the next block */
    double ncs[20];                      /* the last 20 call counts (nested.py:325-326) */
    double mean_calls;
    int ncs_len, expired;
} nnest_host_prior_t;
int nnest_host_prior_consume(nnest_host_state_t *state, nnest_host_prior_t *prior, int N, int D, int nd, double *active_u,
                             double *active_v, double *active_logl, double *active_derived, const long long *cand_idx,
                             const double *cand_logl32, const double *cand_logl64, const double *cand_u, const double *cand_v,
                             const double *cand_derived, double *dead_v, double *dead_logl, double *dead_logwt,
                             double *dead_logz_prev, long long dead_cap, double dlogz, long long max_iters, long long log_interval,
                             double volume_switch, double mcmc_steps, int mcmc_valid);
/* h <- exp(logwt - total) * logl + exp(logz_prev - total) * (h + logz_prev) - total  over n dead points (nested.py:281-283), the two
 * exponentials supplied by the caller (e1, e2); every operation rounded by itself.  Returns the new h. */
double nnest_host_h_update(double h, const double *e1, const double *e2, const double *logl, const double *logz_prev,
                           const double *total, long long n);

#ifdef __cplusplus
}
#endif
#endif /* NNEST_HIP_H */
