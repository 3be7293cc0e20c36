/* bmm_mcmc.h -- C ABI of the MI355X-native cluster-allocation path of bmm-mcmc.
 *
 * This is the drop-in boundary: the three *_run entry points take exactly what the
 * reference's .Call glue hands its C++ samplers and fill caller-owned buffers laid
 * out like the R objects it returns.  Plain pointers and sizes only; no R, Rcpp,
 * torch or HIP types.  Every function returns 0 on success or a BMM_E_* code, and
 * bmm_last_error() then describes the failure (thread-local).  Nothing here aborts.
 *
 * Layouts (all as R stores them):
 *   X          N x P int32, column-major: element (i,d) at X[i + d*N]   (IntegerMatrix,
 *              /root/reference/src/RcppExports.cpp:15)
 *   z_out      S x N int32, column-major, labels 1-based, S = nsamples - burnin
 *              (arma::Mat<int>::tail_rows, src/collapsed_gibbs.cpp:240)
 *   theta_out  K x P x S double, column-major                (src/collapsed_gibbs.cpp:241)
 *   alpha_out  S doubles (an S x 1 matrix in R)              (src/collapsed_gibbs.cpp:231)
 *   pi_out     S x maxK double, column-major                 (src/stickbreaking.cpp:240)
 * Rows the reference never writes (trace row 0 when burnin = 0) come back as
 * NA_integer_ (INT_MIN) / NaN / the initial values, see DESIGN.md "Quirks".
 *
 * `batch`: observations are resampled in consecutive batches of this many against
 * sufficient statistics frozen at batch start, each with its own contribution
 * removed exactly.  batch = 1 is the reference's sequential scan (src/collapsed_gibbs.cpp:86-182
 * updates the member lists after every draw); batch <= 0 picks bmm_default_batch(sampler, N), a
 * function of the sampler and N only.  `seed` keys the Philox streams; same seed + same batch
 * (given or defaulted) => same chain, bit for bit, on any device and with either X layout.
 *
 * TOLERANCE of a batch > 1 against the sequential scan (the north star's "stated floating-point
 * tolerance on posterior cluster proportions").  Quantity: the posterior-mean cluster
 * proportions, sorted descending (label-switching invariant), averaged over the kept sweeps.
 *   BMM_TOL_PROPORTIONS 0.015  |default-batch chain - batch-1 chain| per component, both averaged
 *                              over >= 3 seeds, on each of the reference's bundled data sets
 *                              (measured, 3 seeds x 400 kept sweeps: 0.0002 on K2_N100_P5, 0.0001 on
 *                              K2_N1000_P5, 0.005 on K3_N1000_P5, whose two 0.2 components overlap)
 *   BMM_TOL_THETA       0.05   the same comparison for theta-hat, per cell, clusters ordered by size
 *                              within each sweep (measured 0.0004, 0.0001, 0.037).  Against the
 *                              generating values the reference documents (R/bmm-mcmc.R:16-17, 34-35,
 *                              49-50) theta-hat of K2_N1000_P5 is within the same 0.05 (measured
 *                              0.035); on K3_N1000_P5 the posterior itself, at batch 1 as at the
 *                              default, sits up to 0.16 from them (finite sample, overlapping
 *                              components), so there the pin is the batch-1 chain, not the truth.
 * The DP sampler at its default batch (N/16): the two dominant components of K2_N1000_P5 within 0.05
 * of the batch-1 chain over 6 seeds (measured 0.038; noise-limited -- an unbounded-K chain wanders,
 * seed s.d. 0.08).
 * tests/test_gpu_tolerance.py holds the HIP path to all of it on the GPU, default batch against the
 * batch-1 oracle chain.  At the shapes the benchmark numbers are quoted on the batch-1 chain is a committed
 * fixture (tests/golden/tolerance_*.json: K = 20 with N = 1e6, P = 50 and N = 1e7, P = 100; K = 3, N = 1e5; five
 * DP shapes up to N = 1e6) and tests/test_gpu_tolerance_fixtures.py holds the default batch to the same two
 * numbers against it, per component including the 1/210 one: measured at most 2e-5 and 1e-3 from the generating
 * allocation (the bias of a batch shrinks with N; the bundled N <= 1000 sets above are the hard case).  For the
 * DP sampler there the quantity is the share of the observations per generating component (the sequential
 * scan itself seats a generating component as two clusters at N >= 1e5).  The tests run at exactly what
 * bmm_default_batch returns (N/8 and N/16 below 2^16 observations, N/4 for both samplers from there on), including a
 * K = 20 fixture at N = 2^16, the smallest N that gets the larger batch.
 * The stick-breaking and full samplers have no batch and no tolerance:
 * their z-step is exactly parallel (src/stickbreaking.cpp:69-92 reads only sweep j-1).
 */
#ifndef BMM_MCMC_H
#define BMM_MCMC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BMM_OK 0
#define BMM_E_ARG 1         /* invalid argument (message says which) */
#define BMM_E_UNSUPPORTED 2 /* more than 1024 categories */
#define BMM_E_HIP 3         /* a HIP runtime call failed */
#define BMM_E_NODEVICE 4    /* no usable gfx950 device */
#define BMM_E_STATE 5       /* call sequence error on a resident chain */
#define BMM_E_RCCL 6        /* RCCL could not be opened, or a collective failed */
#define BMM_E_CALLBACK 7    /* a relabel hook returned non-zero */

#define BMM_TOL_PROPORTIONS 0.015
#define BMM_TOL_THETA 0.05

#define BMM_SAMPLER_COLLAPSED 0
#define BMM_SAMPLER_DP 1
#define BMM_SAMPLER_SB 2
#define BMM_SAMPLER_FULL 3

#define BMM_NA_INTEGER (-2147483647 - 1)

const char* bmm_last_error(void);
/* features per lookup group of the spec arithmetic (DESIGN.md "Numerics"): of the tables against the full
 * statistics (preferred width; _for: the width the shape runs at -- narrower when its table image would not
 * fit in LDS otherwise; a pure function of its arguments, -1 for invalid ones), and of the own-cluster
 * ("minus self") tables */
int bmm_spec_group_width(void);
int bmm_spec_group_width_own(void);
int bmm_spec_group_width_for(int sampler, int K, int P);
/* LDS bytes a workgroup of the packed resample kernel needs at (sampler, K, P) with lookup groups of W features
 * (W one of the two widths above): both binary32 images, Nk, E, the histogram and the queue; -1 where P or K is
 * beyond the resident kernels or W is neither width */
int64_t bmm_spec_pk_image_bytes(int sampler, int K, int P, int W);
/* library default batch size for N observations (used when batch <= 0): below 2^16 observations floor(N/8)
 * for the finite sampler and floor(N/16) for the DP sampler (at least 1); from 2^16 on floor(N/4) for
 * both -- the bias of a batch shrinks with N and is not measurable there (TOLERANCE above; DESIGN.md
 * section 2); N for stick-breaking and full.  Depends on nothing else. */
int64_t bmm_default_batch(int sampler, int64_t N);

/* ---- progress of the *_run entry points ---------------------------------------------------
 * The reference prints "Sample j" at every sweep (src/collapsed_gibbs.cpp:85, stickbreaking.cpp:67; the DP
 * sampler adds the current number of clusters, collapsed_gibbs_dp.cpp:99).  Here a run is silent unless the
 * caller installs a hook: after every `every`-th sweep the calling thread calls fn(user, sample, nsamples,
 * k_used) with sample = the reference's printed index of the sweep just finished (2 .. nsamples), k_used =
 * the DP sampler's clusters in use after it (-1 for the other samplers).  A non-zero return stops the run
 * (BMM_E_CALLBACK).  Per calling thread; applies to the single-chain *_run calls made afterwards; fn = NULL
 * or every <= 0 turns it off.  The sweeps stay enqueued ahead of the device: the hook follows events. */
typedef int (*bmm_progress_fn)(void* user, int sample, int nsamples, int k_used);
int bmm_set_progress(bmm_progress_fn fn, void* user, int every);
/* Wall-clock milliseconds the last single-chain *_run call of this thread spent in: [1] creating the chain,
 * its buffers and the starting state (the host's other cores validate and pack X meanwhile), [0] what was
 * left of the packing after that, plus the upload of the planes, [2] enqueueing the sweeps, [3] waiting for
 * the device to finish them, [4] the label trace on its way out (device transpose, PCIe, host copy into the
 * caller's matrix), [5] releasing the chain. */
#define BMM_RUN_PHASES 6
int bmm_last_run_phases(double* ms /* BMM_RUN_PHASES doubles */);
/* host threads the two ends of a run use (affinity mask, cgroup CPU quota, at most 16) */
int bmm_host_threads(void);
/* Between calls the library keeps up to eight 4 MiB pieces of pinned host staging and, per device, up to four
 * idle plain streams and up to six device blocks of at most 512 MiB in all (creating and destroying a stream
 * costs about 2 ms each on this runtime, pinning 4 MiB about 1 ms, and a device allocation now and then 10 ms:
 * together more than a 220-sweep drop-in call at N = 1e6 spends outside its sweeps).  This releases them; they
 * come back with the next call. */
int bmm_release_pools(void);

/* ---- beta, gamma: the Beta(beta, gamma) prior of every theta_kd ------------------------------
 * Any beta, gamma > 0 is accepted.  Every Beta variate the samplers draw (theta, the sticks, the imputation step's
 * phi, the eject move's p_E, the eta of the concentration's update) is X / (X + Y) of two gamma variates and is a
 * number in [0, 1] for every pair of positive shapes, never NaN.  A gamma variate of shape below 0.052 can lie below
 * the binary64 range and is then exactly 0, as R's rgamma returns it; a Beta draw one of whose gammas did so is
 * decided from the logarithms of the same two variates, 1 / (1 + exp(log Y - log X)), which continues the same
 * random variable and keeps the law Beta(p, q) (csrc/bmm_spec.h, rbeta_join_; DESIGN.md "Variates").  With small
 * beta and gamma most of a Beta(beta + s, gamma + n - s) draw's mass of an empty or one-sided cell rounds to
 * exactly 0 or 1: such theta cells appear in the trace from beta = gamma of about 0.05 down, and their table entries
 * are -inf (a category whose weight is exactly 0 for a row that contradicts the cell).
 *
 * ---- drop-in entry points --------------------------------------------------------
 * Replaces collapsed_gibbs_cpp (src/collapsed_gibbs.cpp:24-36; .Call symbol
 * _bmmmcmc_collapsed_gibbs_cpp, src/RcppExports.cpp:11-31) with relabel = FALSE. */
int bmm_collapsed_run(const int32_t* X, int64_t N, int P, const int32_t* initialK, int nsamples,
                      int K, double alpha, double beta, double gamma, double a, double b, int burnin,
                      int64_t batch, uint64_t seed, int device, int32_t* z_out, double* theta_out,
                      double* alpha_out);
/* Replaces collapsed_gibbs_dp_cpp (src/collapsed_gibbs_dp.cpp:27-38; .Call symbol
 * _bmmmcmc_collapsed_gibbs_dp_cpp, src/RcppExports.cpp:34-53).  theta_out is maxK x P x S. */
int bmm_dp_run(const int32_t* X, int64_t N, int P, int nsamples, double alpha, double beta,
               double gamma, double a, double b, int burnin, int maxK, int64_t batch, uint64_t seed,
               int device, int32_t* z_out, double* theta_out, double* alpha_out);
/* Replaces gibbs_stickbreaking_cpp (src/stickbreaking.cpp:10-23; .Call symbol
 * _bmmmcmc_gibbs_stickbreaking_cpp, src/RcppExports.cpp:114-135).  initialTheta is
 * maxK x P column-major.  The z-step is exactly parallel, so there is no batch. */
int bmm_sb_run(const int32_t* X, int64_t N, int P, const double* initialPi,
               const double* initialTheta, int nsamples, int maxK, double alpha, double beta,
               double gamma, double a, double b, int burnin, uint64_t seed, int device,
               double* pi_out, int32_t* z_out, double* theta_out, double* alpha_out);

/* Replaces gibbs_cpp, the uncollapsed finite sampler (src/full_gibbs.cpp:32-45; .Call symbol
 * _bmmmcmc_gibbs_cpp, src/RcppExports.cpp:66-88): the z-step of the stick-breaking sampler with
 * pi ~ Dirichlet(alpha/K + counts) (full_gibbs.cpp:203-210).  SURVEY.md section 8 row f1. */
int bmm_full_run(const int32_t* X, int64_t N, int P, const double* initialPi,
                 const double* initialTheta, int nsamples, int K, double alpha, double beta,
                 double gamma, double a, double b, int burnin, uint64_t seed, int device,
                 double* pi_out, int32_t* z_out, double* theta_out, double* alpha_out);

/* ---- relabel = TRUE: the per-sweep allocation probabilities for the host's Stephens code ----
 * The reference stores, per observation, the normalised conditional it drew z_i from: for the last
 * `burnrelabel` burn-in sweeps into the cube probs_out (N x K x burnrelabel,
 * src/collapsed_gibbs.cpp:76,162-167) that my_stephens_batch consumes once at j = burnin - 1
 * (:187-190), then every kept sweep's N x K matrix probs_sample for my_stephens_online (:168-172,
 * :191-192).  Stephens' algorithm and lp_solve stay host code of the reference, unchanged; the
 * *_run_probs entry points produce exactly those matrices on the device (from the resident
 * resample kernel's own weights) and hand them over through these hooks, called on the calling
 * thread.  Matrices are column-major, by label; the DP's new-cluster mass is filed under the label
 * it would open (src/collapsed_gibbs_dp.cpp:193).  A hook returning non-zero stops the run
 * (BMM_E_CALLBACK).  The chain itself does not depend on the relabelling, so sweep j + 1 already runs
 * while on_sample works on sweep j.  hooks == NULL: exactly the plain *_run. */
typedef int (*bmm_probs_fn)(void* user, int j /* sweep index, 1-based as the reference's loop */,
                            const double* probs /* host, valid during the call */);
typedef struct bmm_relabel_hooks {
    int burnrelabel;         /* sweeps of the batch window (clamped to burnin) */
    double* probs_batch;     /* N x K x burnrelabel doubles, filled before batch_done; caller-owned */
    bmm_probs_fn batch_done; /* once, after sweep burnin - 1; probs = probs_batch; may be NULL */
    bmm_probs_fn on_sample;  /* after every sweep j >= burnin; probs = that sweep's N x K; may be NULL */
    void* user;
} bmm_relabel_hooks;
int bmm_collapsed_run_probs(const int32_t* X, int64_t N, int P, const int32_t* initialK, int nsamples,
                            int K, double alpha, double beta, double gamma, double a, double b,
                            int burnin, int64_t batch, uint64_t seed, int device, int32_t* z_out,
                            double* theta_out, double* alpha_out, const bmm_relabel_hooks* hooks);
int bmm_dp_run_probs(const int32_t* X, int64_t N, int P, int nsamples, double alpha, double beta,
                     double gamma, double a, double b, int burnin, int maxK, int64_t batch,
                     uint64_t seed, int device, int32_t* z_out, double* theta_out, double* alpha_out,
                     const bmm_relabel_hooks* hooks);
int bmm_sb_run_probs(const int32_t* X, int64_t N, int P, const double* initialPi,
                     const double* initialTheta, int nsamples, int maxK, double alpha, double beta,
                     double gamma, double a, double b, int burnin, uint64_t seed, int device,
                     double* pi_out, int32_t* z_out, double* theta_out, double* alpha_out,
                     const bmm_relabel_hooks* hooks);
int bmm_full_run_probs(const int32_t* X, int64_t N, int P, const double* initialPi,
                       const double* initialTheta, int nsamples, int K, double alpha, double beta,
                       double gamma, double a, double b, int burnin, uint64_t seed, int device,
                       double* pi_out, int32_t* z_out, double* theta_out, double* alpha_out,
                       const bmm_relabel_hooks* hooks);

/* ---- relabel = TRUE with Stephens' relabelling on the device ----------------
 * The reference's online relabelling (src/stephens.cpp, lp_solve underneath) as it executes, resident on the
 * device: the batch window's matrices stay in HBM, my_stephens_batch runs once after sweep burnin - 1
 * (collapsed_gibbs.cpp:187-190; always maxiter = 100 iterations: its threshold 10^(-6) is an integer XOR,
 * stephens.cpp:24), my_stephens_online after every kept sweep (:191-199), all stream-ordered behind the sweeps
 * with no host round trip.  The assignment lp_solve solves is solved exactly by the Hungarian method with a fixed
 * tie rule (lowest column index wins; DESIGN.md lists the choice among equal-cost optima as a deviation).
 * Arguments are those of the *_run_probs entry points with the hooks replaced by `rel`; z_out / theta_out
 * receive the relabelled traces (z = perm[z - 1] + 1, theta_relab(perm(k), d, s) = theta(k, d, s):
 * collapsed_gibbs.cpp:197-199, 215-217), rel the rest of the reference's list.  BMM_E_ARG when the reference
 * would have no Q (burnin < 2 or burnrelabel < 1), for K (maxK) above BMM_STEPHENS_MAX_K, and -- before the first
 * sweep, naming the bytes -- when the window (burnrelabel x N x K doubles) and its workspace do not fit in device
 * memory.  Progress hooks and bmm_last_run_phases behave as in a plain run. */
#define BMM_STEPHENS_MAX_K 128
typedef struct bmm_relabel_out {
    int burnrelabel;          /* sweeps of the batch window (>= 1; clamped as the R wrappers do) */
    int32_t* permutations;    /* S x K int32 column-major, 0-based (arma::Mat<int>, collapsed_gibbs.cpp:194) */
    int32_t* z_original;      /* S x N as z_out: the labels as sampled */
    double* theta_original;   /* K x P x S as theta_out: theta as sampled */
} bmm_relabel_out;
int bmm_collapsed_run_relabel(const int32_t* X, int64_t N, int P, const int32_t* initialK, int nsamples,
                              int K, double alpha, double beta, double gamma, double a, double b,
                              int burnin, int64_t batch, uint64_t seed, int device, int32_t* z_out,
                              double* theta_out, double* alpha_out, const bmm_relabel_out* rel);
int bmm_dp_run_relabel(const int32_t* X, int64_t N, int P, int nsamples, double alpha, double beta,
                       double gamma, double a, double b, int burnin, int maxK, int64_t batch,
                       uint64_t seed, int device, int32_t* z_out, double* theta_out, double* alpha_out,
                       const bmm_relabel_out* rel);
int bmm_sb_run_relabel(const int32_t* X, int64_t N, int P, const double* initialPi,
                       const double* initialTheta, int nsamples, int maxK, double alpha, double beta,
                       double gamma, double a, double b, int burnin, uint64_t seed, int device,
                       double* pi_out, int32_t* z_out, double* theta_out, double* alpha_out,
                       const bmm_relabel_out* rel);
int bmm_full_run_relabel(const int32_t* X, int64_t N, int P, const double* initialPi,
                         const double* initialTheta, int nsamples, int K, double alpha, double beta,
                         double gamma, double a, double b, int burnin, uint64_t seed, int device,
                         double* pi_out, int32_t* z_out, double* theta_out, double* alpha_out,
                         const bmm_relabel_out* rel);
/* The two functions of src/stephens.h on the device, for arbitrary host inputs (what the runs above execute):
 *   batch:  p N x K x M (column-major cube, finite, >= 0) -> Q_out N x K (the Q computed at the start of the last
 *           of the 100 iterations, stephens.cpp:36-43, 64) and perm_out M x K int32 (that iteration's
 *           permutations, 0-based, not inverted: :54-56)
 *   online: Q, p N x K and the sweep index j -> perm_out K (0-based), Q_out = (j * (Q + p[:, perm])) / (j + 1)
 *           (:77-92), and, unless NULL, cost_out K x K column-major: the cost matrix the assignment was solved on,
 *           C[k,l] = sum_n p(n,l) * (p(n,l) - log Q(n,k)) with terms of p(n,l) == 0 counting 0 (:79). */
int bmm_device_stephens_batch(int device, const double* p, int64_t N, int K, int M, double* Q_out,
                              int32_t* perm_out);
int bmm_device_stephens_online(int device, const double* Q, const double* p, int64_t N, int K, int j,
                               int32_t* perm_out, double* Q_out, double* cost_out);
/* Which form of the relabelling kernels a shape runs, as pure bookkeeping -- no device is touched, and the values
 * come from the functions the launches themselves call.  N rows, K categories, M slices of a batch window (M = 0:
 * the online step only).  out:
 *   [0] workgroups of the cost pass over one slice (the online step)   [1] the same per slice of an M-slice batch
 *   [2] rows of p per workgroup for [0]                                [3] for [1]       ([1], [3]: 0 when M = 0)
 *   [4] 4 x 4 blocks of the cost matrix per thread (1..4)              [5] rows staged in LDS per tile (64 or 16)
 *   [6] 4 x 4 blocks in all, ceil(K/4)^2                               [7] thread groups sharing a tile's rows
 *   [8] 1 when the assignment holds the cost matrix in LDS, else 0     [9] columns per lane of the assignment (1..3)
 *   [10], [11] unused, 0.
 * BMM_E_ARG unless N >= 1, M >= 0 and 1 <= K <= BMM_STEPHENS_MAX_K. */
int bmm_device_stephens_plan(int64_t N, int K, int M, int64_t out[12]);

/* ---- several independent chains in one call (SURVEY.md section 8 rows b and e) ---------------
 * n_chains chains of one sampler over the same data, chain c keyed seed + c and resident on
 * devices[c] (all on device 0 when devices is NULL; a device may appear several times: its chains
 * share one copy of the data and overlap on streams with hardware queues of their own -- about four
 * chains per device is where that pays).  X is uploaded and packed into bit
 * planes once, on devices[0]; when the run spans several devices the planes -- 4 * ceil(P/32) bytes
 * per observation, not the int32 matrix -- are broadcast once with RCCL over xGMI inside this
 * process (ncclCommInitAll over the distinct devices, one ncclBroadcast; librccl is opened on
 * demand, BMM_E_RCCL if that fails).  That is the only collective: chains never communicate.
 * One host thread per chain drives it; nothing of R's API is touched off the calling thread.
 * Per-chain inputs and outputs are tables of n_chains pointers, each laid out as in the
 * single-chain entry point of the sampler (initialK for collapsed; initialPi/initialTheta and pi_out
 * for stick-breaking and full; unused tables may be NULL).  relabel is not offered here. */
int bmm_multi_run(int sampler, int n_chains, const int* devices, const int32_t* X, int64_t N, int P,
                  const int32_t* const* initialK, const double* const* initialPi,
                  const double* const* initialTheta, int nsamples, int K /* K or maxK */, double alpha,
                  double beta, double gamma, double a, double b, int burnin, int64_t batch, uint64_t seed,
                  double* const* pi_out, int32_t* const* z_out, double* const* theta_out,
                  double* const* alpha_out);
/* Where bmm_multi_run puts things for a device table (NULL: every chain on device 0), as pure bookkeeping --
 * no device is touched: devices_out[0 .. *n_devices_out) = the distinct devices in first-use order (the
 * broadcast list of the one ncclBroadcast, root first: devices_out[0] packs the data), holder_of_chain[c] =
 * the chain that holds the copy of the bit planes chain c reads (the first chain on c's device; a holder
 * names itself, every other chain shares with bmm_chain_share_data).  Both outputs have room for n_chains. */
int bmm_multi_plan(int n_chains, const int* devices, int* n_devices_out, int* devices_out, int* holder_of_chain);
/* The broadcast of bmm_multi_run on a test pattern of `words` 32-bit words over the listed distinct
 * devices, compared afterwards on every one of them.  With one device the collective still runs
 * (library opened, communicator of one rank, ncclBroadcast): what a one-GPU box can check. */
int bmm_multi_selfcheck(int n_devices, const int* devices, int64_t words);

/* ---- resident chains --------------------------------------------------------------
 * The same samplers with the data matrix and the chain state kept in HBM between
 * calls: what the benchmark and the one-chain-per-GPU driver use.  A chain is bound
 * to one device and one HIP stream; calls on one chain must not overlap. */
typedef struct bmm_chain bmm_chain;

int bmm_chain_create(bmm_chain** out, int sampler, int64_t N, int P, int K /* K or maxK */,
                     double alpha, double beta, double gamma, double a, double b, int64_t batch,
                     uint64_t seed, int device);
void bmm_chain_destroy(bmm_chain* c);
/* How the sweeps read X.  X is constant over the chain, so by default it is packed once, when
 * it is handed over, into bit planes (ceil(P/32) 32-bit words per observation: 24 instead of 408
 * bytes per observation and sweep at P = 100) and the int32 matrix is not kept: host data pass
 * through a staging buffer in slabs of rows, a matrix already on the device is read once and not
 * again after bmm_chain_set_data_device returns.  BMM_X_INT32 streams the IntegerMatrix layout R
 * hands over in place instead (no packing pass; a device matrix stays borrowed for the life of
 * the chain).  Same chain either way.  To be chosen before the data are set. */
#define BMM_X_BITPLANES 0
#define BMM_X_INT32 1
int bmm_chain_set_x_layout(bmm_chain* c, int layout);
int bmm_chain_get_x_layout(const bmm_chain* c, int* layout);
/* X from host memory or already on this device (see the layouts above for what is kept).
 * set_data_device reads dX on the chain's own stream: it first waits for the whole device
 * (hipDeviceSynchronize), so a matrix a kernel or a collective of the caller's is still writing
 * is complete before it is validated and packed. */
int bmm_chain_set_data_host(bmm_chain* c, const int32_t* X);
int bmm_chain_set_data_device(bmm_chain* c, const void* dX);
/* Several chains on one device over the same data: `c` shares the bit planes `from` holds (same
 * device, N and P), before either has run a sweep.  The planes are reference-counted: chains may be
 * destroyed in any order, the last one frees them.  Both chains move to streams with hardware queues of
 * their own, so that their launches overlap (up to about four chains per device pay off).  What
 * bmm_multi_run does for chains that share a device. */
int bmm_chain_share_data(bmm_chain* c, bmm_chain* from);
/* The chain's bit planes on its device: ceil(P/32) planes of N 32-bit words (allocated on first
 * call).  A rank that received them from a broadcast (160 MB instead of the 4 GB int32 matrix at
 * K=20, N=1e7, P=100) declares them complete with bmm_chain_planes_filled, which waits for the device. */
int bmm_chain_planes(bmm_chain* c, void** dXb, int64_t* n_words);
int bmm_chain_planes_filled(bmm_chain* c);
/* Resident chains on different devices, one per device, in one process: chains[0] holds the data; the
 * others receive its bit planes with one RCCL broadcast (ncclCommInitAll + ncclBroadcast, as
 * bmm_multi_run does).  Then bmm_chains_sweeps drives them, one host thread each. */
int bmm_chains_broadcast_planes(bmm_chain* const* chains, int n_chains);
/* starting state: collapsed needs 1-based labels; stick-breaking needs pi and theta;
 * dp starts from zero clusters and needs neither */
int bmm_chain_set_initial_labels(bmm_chain* c, const int32_t* z1);
int bmm_chain_set_initial_params(bmm_chain* c, const double* pi, const double* theta);
/* enqueue n more sweeps on the chain's stream (returns without waiting) */
int bmm_chain_sweeps(bmm_chain* c, int n);
/* the same for several chains at once, one host thread per chain (chains on one device overlap) */
int bmm_chains_sweeps(bmm_chain* const* chains, int n_chains, int n);
int bmm_chain_sync(bmm_chain* c);
/* n more sweeps, returning the cluster sizes after each one (nk_out is n x K, row-major: sweep,
 * label) -- the per-sweep summary plot_gibbs derives from z (R/utils.R:146-173) without moving
 * the 4*N-byte label row off the device each sweep.  Waits. */
int bmm_chain_sweeps_counts(bmm_chain* c, int n, int32_t* nk_out);
int bmm_chain_sweep_index(const bmm_chain* c); /* sweeps done so far */
/* current state, copied to host: labels 1-based (NA where unassigned) */
int bmm_chain_get_labels(bmm_chain* c, int32_t* z1);
int bmm_chain_get_counts(bmm_chain* c, int32_t* Nk /*K*/, int32_t* S /*K*P, S[k*P+d]*/);
int bmm_chain_get_alpha(bmm_chain* c, double* alpha);
int bmm_chain_get_params(bmm_chain* c, double* pi /*K*/, double* theta /*K x P colmajor*/);
/* One more sweep, also returning that sweep's allocation probabilities: probs_out is N x K
 * column-major (host), row i = the normalised conditional observation i was drawn from, by label
 * (the DP's new-cluster mass under the label it would open).  This is the matrix the reference
 * stores for Stephens' relabelling (src/collapsed_gibbs.cpp:162-172, collapsed_gibbs_dp.cpp:190-200,
 * stickbreaking.cpp:129-139) -- one sweep of what the *_run_probs entry points stream (SURVEY.md section 8
 * row f2): the weights come out of the resident resample kernel itself.  Waits. */
int bmm_chain_sweep_probs(bmm_chain* c, double* probs_out);

/* ---- one chain sharded over several ranks --------------------
 * Exact for the stick-breaking and full samplers, whose z-step is independent across
 * observations given (pi, theta): each rank holds rows [first_row, first_row + N) of the N_total
 * and resamples them; the K*(P+1) integer statistic deltas are summed over ranks (one RCCL
 * all-reduce, done by the caller on the device pointers below); every rank then draws the same
 * pi, theta, alpha, because the Philox streams are keyed by (seed, global index) only.
 *   set_shard once before the first sweep; per sweep: shard_resample (returns with the deltas
 *   complete), all-reduce *dNk (K int32) and *dS (K*P int32) in place, shard_finish.
 *   The _async form of shard_resample returns without waiting: the caller then orders its collective
 *   behind the chain's own HIP stream (bmm_chain_stream) and the finish behind the collective -- no
 *   host round trip inside a sweep (multi.ShardedChain does it with a torch ExternalStream). */
int bmm_chain_set_shard(bmm_chain* c, int64_t N_total, int64_t first_row);
int bmm_chain_shard_resample(bmm_chain* c);
int bmm_chain_shard_resample_async(bmm_chain* c);
int bmm_chain_stream(bmm_chain* c, void** hip_stream);
int bmm_chain_shard_deltas(bmm_chain* c, void** dNk, void** dS);
int bmm_chain_shard_finish(bmm_chain* c);

/* HIP-event timing of the z-resample kernel on the chain's own stream (start / stop events attached to
 * the launches): turn on, run sweeps, sync, read total milliseconds and launch count since it was turned on.
 * every = 0 off, 1 every sweep, n the launches of every n-th sweep only (an event pair costs
 * a few us of stream time per launch, which a sampled measurement keeps out of the total) */
int bmm_chain_profile(bmm_chain* c, int every);
int bmm_chain_profile_read(bmm_chain* c, double* resample_ms, int64_t* resample_launches);
/* batch size in effect */
int64_t bmm_chain_batch(const bmm_chain* c);
/* bytes of dynamic LDS and threads per workgroup the resample kernel uses for this shape */
int bmm_chain_kernel_shape(const bmm_chain* c, int* lds_bytes, int* threads, int* grid_max);
/* ... and its form: lanes of a wave per observation (1, or 2: two lanes share an observation, each scoring half
 * of the categories -- above 32 accumulators, and for launches too short to fill the chip otherwise), and whether
 * the resample workgroups build the table image themselves (small finite-sampler shapes: no table kernel between
 * batches).  Which form runs never changes a chain's values. */
int bmm_chain_kernel_form(const bmm_chain* c, int* lanes_per_observation, int* builds_own_tables);

/* ---- posterior predictive density of new observations ------------------------------
 * For a state s of the chain (the state after a sweep) and a new binary row x of P features, the per-state
 * predictive density p(x | s) is the model's posterior predictive given that state:
 *   collapsed  (counts Nk, S; concentration alpha_s; N fitted observations), over all K labels:
 *              sum_k (Nk + alpha/K)/(N + alpha) * prod_d (beta + S_kd)^x_d (gamma + Nk - S_kd)^(1-x_d) / (beta + gamma + Nk)
 *              -- an empty label keeps its prior weight (alpha/K)/(N + alpha) and the prior Bernoulli terms;
 *   dp         sum over used labels of Nk/(N + alpha) * (the same product), plus the new-cluster term
 *              alpha/(N + alpha) * prod_d beta^x_d gamma^(1-x_d) / (beta + gamma);
 *   sb, full   (pi_s, theta_s as returned for that sweep): sum_k pi_k prod_d theta_kd^x_d (1 - theta_kd)^(1-x_d).
 * alpha_s is the value the next sweep's conditional would use.  These are proper densities (over all 2^P rows they
 * sum to 1) and the samplers' own allocation conditionals for an (N+1)-th observation in all but two places, where
 * the predictive uses the model's terms: the finite collapsed sampler gives an emptied label probability 0 for ever,
 * and the DP sampler's new-cluster term is P * (log beta - log(beta + gamma)) whatever x is (equal to the term above
 * only when beta == gamma).  The quantity does not depend on how the labels are numbered: it needs no relabelling.
 *
 * For M new rows and the S folded states:
 *   lppd[m]       log((1/S) sum_s p(x_m | s)), the log pointwise predictive density;
 *   logdens[s, m] log p(x_m | s), S x M column-major like the label trace;
 *   resp[m, k]    the mean over the folded states of the normalised category weights, M x Kc column-major, Kc = K,
 *                 for the DP sampler maxK labels and then the new-cluster column.  It is in the sampler's label
 *                 order of each sweep, so it means something only for a chain that does not switch labels.
 * Xnew is M x P int32 column-major (element (m, d) at Xnew[m + d*M]); it is validated (0/1) and packed into bit
 * planes on the device.  Everything is enqueued on the chain's stream behind the sweep's last kernel: a folded
 * sweep adds no synchronisation and no host-device copy.  Not offered on a sharded chain (bmm_chain_set_shard). */
/* resident chains: the new rows; replaces any earlier set and empties the accumulators; M = 0 drops it */
int bmm_chain_set_newdata_host(bmm_chain* c, const int32_t* Xnew, int64_t M);
/* whether the folds also accumulate resp (off by default: Kc more doubles per row and fold); empties the accumulators */
int bmm_chain_predict_responsibilities(bmm_chain* c, int on);
/* the new rows against the current state, once: no sweep, accumulators untouched.  logdens_out M doubles, resp_out
 * M x Kc or NULL.  Waits. */
int bmm_chain_predict_state(bmm_chain* c, double* logdens_out, double* resp_out);
/* n more sweeps, each folded into the accumulators; logdens_trace n x M column-major (then the call waits) or NULL
 * (then it returns without waiting, as bmm_chain_sweeps).  BMM_E_ARG, naming the bytes, when the trace does not fit
 * in device memory. */
int bmm_chain_sweeps_predict(bmm_chain* c, int n, double* logdens_trace);
/* lppd (M doubles) and resp (M x Kc, or NULL) over the states folded so far, and their number; the accumulators
 * stay, so more sweeps may follow */
int bmm_chain_get_predictive(bmm_chain* c, double* lppd, double* resp, int* n_folded);
int bmm_chain_predict_reset(bmm_chain* c);

/* One call: the *_run entry points plus Xnew, M and the outputs; only kept sweeps (j >= burnin) are folded.  Without
 * burn-in the first kept row of the traces is the starting state, not a sweep: that row of logdens is NaN and
 * lppd averages over the S - 1 sweeps.  relabel / hooks: NULL, or what the *_run_relabel / *_run_probs entry points
 * take in their last argument -- the predictive does not depend on the labels, so it combines with either. */
typedef struct bmm_predict_out {
    double* lppd;                     /* M doubles */
    double* logdens;                  /* S x M doubles column-major, or NULL */
    double* resp;                     /* M x Kc doubles column-major, or NULL */
    const bmm_relabel_out* relabel;   /* or NULL */
    const bmm_relabel_hooks* hooks;   /* or NULL (ignored when relabel is set) */
} bmm_predict_out;
int bmm_collapsed_run_predict(const int32_t* X, int64_t N, int P, const int32_t* initialK, int nsamples, int K,
                              double alpha, double beta, double gamma, double a, double b, int burnin,
                              int64_t batch, uint64_t seed, int device, int32_t* z_out, double* theta_out,
                              double* alpha_out, const int32_t* Xnew, int64_t M, const bmm_predict_out* pred);
int bmm_dp_run_predict(const int32_t* X, int64_t N, int P, int nsamples, double alpha, double beta, double gamma,
                       double a, double b, int burnin, int maxK, int64_t batch, uint64_t seed, int device,
                       int32_t* z_out, double* theta_out, double* alpha_out, const int32_t* Xnew, int64_t M,
                       const bmm_predict_out* pred);
int bmm_sb_run_predict(const int32_t* X, int64_t N, int P, const double* initialPi, const double* initialTheta,
                       int nsamples, int maxK, double alpha, double beta, double gamma, double a, double b,
                       int burnin, uint64_t seed, int device, double* pi_out, int32_t* z_out, double* theta_out,
                       double* alpha_out, const int32_t* Xnew, int64_t M, const bmm_predict_out* pred);
int bmm_full_run_predict(const int32_t* X, int64_t N, int P, const double* initialPi, const double* initialTheta,
                         int nsamples, int K, double alpha, double beta, double gamma, double a, double b,
                         int burnin, uint64_t seed, int device, double* pi_out, int32_t* z_out,
                         double* theta_out, double* alpha_out, const int32_t* Xnew, int64_t M,
                         const bmm_predict_out* pred);

/* ---- incomplete new rows: density of the observed cells, missing cells predicted ------
 * A new row x may have missing cells: observed cells O, missing cells U.  The row is not in the fit, so nothing is
 * imputed or approximated: a missing cell marginalises out exactly (its Bernoulli term sums to 1), and the category
 * terms are those of the section above with the product running over d in O only,
 *   p(x_O | s) = sum_k w_k(s) prod_{d in O} t_kd(x_d),
 * w_k the category weights and t_kd the Bernoulli terms of the three formulas above (for the DP the new-cluster column
 * included, an unused label at weight 0).  A row with O empty has p = sum_k w_k: 1 for the finite and the DP sampler,
 * sum_k pi_k for the explicit ones.  For a missing cell (m, d) the per-state joint with a 1 in it is
 *   q_md(s) = p(x_O, x_d = 1 | s) = sum_k w_k prod_{O} t_k.(x.) * t_kd(1).
 * Over the S folded states:
 *   lppd[m]          log((1/S) sum_s p(x_O | s)), on the observed cells;
 *   resp[m, k]       the mean of the normalised category weights from the observed cells;
 *   cell_mean[m, d]  sum_s q_md(s) / sum_s p(x_O | s) = P(x_d = 1 | x_O, X), the posterior predictive probability of a 1
 *                    in the missing cell given the row's observed cells and the fitted data;
 *   cell_state[m, d] q_md(s) / p(x_O | s) = P(x_d = 1 | x_O, s), the per-state value;
 *   logdens[s, m]    log p(x_O | s).
 * cell_mean is NOT the plain mean over the states of cell_state: the chain samples s | X, not s | X, x_O, so the states
 * are weighted by p(x_O | s) (self-normalised importance weights).  Both sums are kept as streaming log-sum-exp pairs,
 * one lane per row and per cell: no atomics, a fixed order, the same bits twice.
 * The cells are given as bmm_set_missing takes them: strictly ascending in (row, column), rows int64 in 0 .. M-1,
 * columns int32 in 0 .. P-1; Xnew holds 0 in them (any 0/1 value is ignored).  Per-cell outputs are in the order of the
 * list.  A set without missing cells takes the kernels of the section above and gives their results byte for byte.
 * Refused, leaving the chain as it was: unsorted or repeated cells, a cell outside M x P (BMM_E_ARG), and whatever
 * the predictive itself refuses. */
/* resident chains: after bmm_chain_set_newdata_host; replaces any earlier mask and empties the accumulators;
 * n = 0 drops the mask.  A later bmm_chain_set_newdata_host drops it with the set it belonged to. */
int bmm_chain_set_newdata_missing(bmm_chain* c, const int64_t* rows, const int32_t* cols, int64_t n);
/* bmm_chain_predict_state with the per-state P(x_d = 1 | x_O, s) of every missing cell: cell_out n doubles or NULL
 * (non-NULL needs a mask); resp_out M x Kc or NULL.  Waits. */
int bmm_chain_predict_state_cells(bmm_chain* c, double* logdens_out, double* resp_out, double* cell_out);
/* cell_mean (n doubles) over the states folded so far, and their number; the accumulators stay */
int bmm_chain_get_predictive_cells(bmm_chain* c, double* cell_mean, int* n_folded);
/* One call: armed for the next *_run_predict call of the calling thread and disarmed when that call returns, whatever
 * it returns, exactly as bmm_set_missing; the cells index the Xnew of that call, cell_mean_out receives n_cells doubles
 * (NaN when no sweep was folded).  cell_mean_out = NULL disarms.  The list must stay valid until the run returns. */
int bmm_set_newdata_missing(const int64_t* rows, const int32_t* cols, int64_t n_cells, double* cell_mean_out);
/* Which form of the masked scorer a shape takes -- a pure function of (sampler, K, P), no device is touched; the
 * launches read the same function.  LDS: the split table image (two tables per group, by bit value, the constants and
 * the exp table) staged in LDS, lds_bytes of it, `threads` lanes per workgroup; GLOBAL: the image does not fit or the
 * shape has no resident kernel: tables read from global memory, scores in scratch columns, lds_bytes = 0.  table_bytes:
 * the image in device memory.  K: the labels (maxK for the DP and stick-breaking samplers). */
enum { BMM_PREDICT_NA_LDS = 0, BMM_PREDICT_NA_GLOBAL = 1 };
typedef struct bmm_predict_na_plan_out {
    int form;             /* BMM_PREDICT_NA_* */
    int threads;
    int64_t lds_bytes;
    int64_t table_bytes;
} bmm_predict_na_plan_out;
int bmm_predict_na_plan(int sampler, int K, int P, bmm_predict_na_plan_out* out);

/* ---- clustering point estimate and posterior similarity ------------------------------
 * Label-invariant summaries of a label trace, computed where the trace is.  A row z of N labels in 0 .. Kc-1 is a
 * partition.  For two rows c, z let n_ab = #{i : c_i = a, z_i = b}, n_a. = sum_b n_ab, n_.b = sum_a n_ab.
 *   Binder distance   B(c, z) = (sum_a n_a.^2 + sum_b n_.b^2 - 2 sum_ab n_ab^2) / 2: the pairs i < j on which the two
 *                     partitions disagree, an exact integer;
 *   VI distance       VI(c, z) = (sum_a f(n_a.) + sum_b f(n_.b) - 2 sum_ab f(n_ab)) / N in nats, f(n) = n log n, f(0) = 0,
 *                     with the spec's log_ (DESIGN.md "Numerics").  Every sum runs in an order fixed by the shape (256
 *                     partial sums, cell k in partial k mod 256, ascending; then a binary tree), d(z, z) = 0 by
 *                     construction (the diagonal is not computed), and VI is exactly 0 wherever B is 0;
 *   expected loss     of candidate row c over the S draws: L(c) = (1/S) sum_t d(c, z_t); binder2 = sum_t 2 B(c, z_t) is
 *                     the exact integer behind it (for Binder L = binder2 / (2 S));
 *   point estimate    the candidate with the smallest L (Binder: the smallest binder2), lowest index on ties.
 *                     Candidates are rows 0, stride, 2 stride, ... (C = ceil(S / stride) of them; stride = 1: every row);
 *                     the draws are always all S rows;
 *   similarity        of chosen observations idx[0 .. M): cnt[u, v] = #{t : z_t[idx_u] = z_t[idx_v]}, uint32, M x M,
 *                     symmetric, diagonal S.
 * With delta_ij = [c_i = c_j]: sum_{i<j} (S delta_ij - cnt_ij)^2 = S sum_t B(c, z_t) + sum_{i<j} cnt_ij^2 - S sum_{i<j} cnt_ij,
 * so Dahl's least-squares criterion against the full N x N similarity matrix orders the candidates as the expected
 * Binder loss does, and that matrix is never needed.
 * A row with a label below 1 (1-based, as z_out) or above Kc is not a partition: the stand-alone entry points refuse
 * it, naming the row and the observation, before a device is touched. */
#define BMM_PARTITION_BINDER 0
#define BMM_PARTITION_VI 1
#define BMM_PARTITION_MAX_K 1024
#define BMM_PARTITION_MAX_ROWS 65535 /* rows of one call (a grid dimension of the launches) */
/* z: S x N int32 column-major, 1-based, as z_out -- any stack of rows over the same observations, so traces of several
 * chains can be pooled by the caller.  loss_out C doubles; binder2_out C uint64 or NULL (filled under either
 * criterion); best_out the row of z (0-based, a multiple of stride) of the point estimate; dist_out C x S doubles
 * column-major or NULL: B (exact below 2^53) or VI of candidate c against row t.  BMM_E_ARG unless 1 <= S <=
 * BMM_PARTITION_MAX_ROWS, N >= 1,
 * stride >= 1, 1 <= Kc <= BMM_PARTITION_MAX_K and S * N^2 < 2^63 (the integer totals would overflow). */
int bmm_device_partition_distances(int device, const int32_t* z, int S, int64_t N, int Kc, int criterion, int stride,
                                   double* loss_out, uint64_t* binder2_out, int* best_out, double* dist_out);
/* idx: M observations, 0-based, in any order, repeats allowed; cnt_out M x M uint32.  Labels may be any values >= 1.
 * S at most BMM_PARTITION_MAX_ROWS.  BMM_E_ARG, naming the bytes, when the M^2 counts and the S x M block of gathered labels do not fit in device memory. */
int bmm_device_psm(int device, const int32_t* z, int S, int64_t N, const int64_t* idx, int64_t M, uint32_t* cnt_out);
/* Which form of the kernels a shape runs, as pure bookkeeping -- no device is touched, and the values come from the
 * functions the launches themselves call.  out:
 *   [0] bytes per label on the device (1 up to 256 categories, else 4)
 *   [1] 1: contingency tables in LDS (Kc <= 64); 0: the generic form, tables in global memory
 *   [2] draws per workgroup, T                    [3] copies of each table, R (4 while a table is at most 1 KiB)
 *   [4] blocks of draws, ceil(S / T)              [5] workgroups launched ([4] x candidates; generic: its grid)
 *   [6] threads per workgroup                     [7] bytes of dynamic LDS (0: generic)
 *   [8] 1 when only t > c is counted and mirrored (every row a candidate)
 *   [9] 1 when the VI sums are computed           [10] bytes of tables in global memory (0: LDS form)
 *   [11] labels per row of the device block (N rounded up to 16).
 * BMM_E_ARG as bmm_device_partition_distances, and unless n_candidates = ceil(S / stride) for some stride >= 1. */
int bmm_device_partition_plan(int S, int64_t N, int Kc, int n_candidates, int criterion, int64_t out[12]);
/* For a run: armed per calling thread, like bmm_set_progress, for the NEXT single-chain *_run* call of that thread
 * (plain, _probs, _relabel, _predict) and disarmed when that call returns, whatever it returns; NULL disarms.  The
 * struct is copied; its buffers must stay valid through that call.  With it armed the run computes the summary from
 * the resident trace after the last sweep and before the trace leaves, on the labels as sampled (the quantities do
 * not depend on the numbering, so a relabelling run gives the same).  Trace row 0 of a run without burn-in is the
 * starting state; where that is no partition (every sampler but the finite collapsed one leaves it unassigned) the
 * row is left out of candidates and draws alike: n_used = S - 1, candidates are rows first, first + stride, ...
 * with first = S - n_used, and loss, binder2 and dist have ceil(n_used / stride) rows and n_used columns.  Not armed:
 * nothing changes, no allocation, no launch.  bmm_multi_run does not take it (pool chains through the stand-alone
 * call): a bmm_multi_run call of the arming thread disarms it like any other run and computes no summary.  The summary's time is counted in phases [3] and [4] of bmm_last_run_phases (it sits between the last sweep
 * and the trace on its way out). */
typedef struct bmm_partition_out {
    int criterion;           /* BMM_PARTITION_BINDER or BMM_PARTITION_VI */
    int stride;              /* >= 1 */
    double* loss;            /* room for ceil(S / stride) doubles */
    uint64_t* binder2;       /* the same count, or NULL */
    int* best;               /* row of the trace (0-based) of the point estimate; -1 when no row was usable */
    int32_t* z_best;         /* N int32, 1-based: that row, the labels as sampled; or NULL */
    int* n_used;             /* rows used */
    double* dist;            /* room for ceil(S / stride) x S doubles, or NULL */
    const int64_t* psm_idx;  /* psm_M observations, 0-based, or NULL */
    int64_t psm_M;
    uint32_t* psm_cnt;       /* psm_M x psm_M, counts over the rows used */
} bmm_partition_out;
int bmm_set_partition_summary(const bmm_partition_out* out);

/* ---- greedy search for the clustering point estimate ----------------------------------
 * The summary above answers with a visited state.  The search moves single rows of a candidate partition to whichever
 * cluster lowers the posterior expected loss most, until no row wants to move (the greedy searches of Wade &
 * Ghahramani 2018, Rastelli & Friel 2018, the sweeps of SALSO, Dahl, Johnson & Mueller 2022), on the device.
 *   z_t (t < S)    the draws, labels in 0 .. Kc-1;
 *   c              the candidate, labels in 0 .. Ka-1: Ka slots, of which any may be empty;
 *   n_a            the size of slot a;  T_t[a][b] = #{i : c_i = a, z_t,i = b};  n_t,b the size of label b of draw t;
 *   binder2(c)     = S sum_a n_a^2 + sum_t sum_b n_t,b^2 - 2 sum_t sum_ab T_t[a][b]^2 = sum_t 2 B(c, z_t), uint64, exact;
 *   vi_tot(c)      = S sum_a f(n_a) + sum_t sum_b f(n_t,b) - 2 sum_t sum_ab f(T_t[a][b]), f(n) = n log_(n), f(0) = 0: the
 *                  device adds it draw by draw, w_t = F_c + F_t - 2 G_t in the fixed order of the section above and
 *                  exactly 0 where B(c, z_t) = 0, then over t (draw t in partial t mod 256, ascending, then a binary
 *                  tree).  The expected VI is vi_tot / (S N);
 *   score          of row i for slot a, the row taken out of the state: with a0 = c_i, own = [a = a0], m_a = n_a - own
 *                  and U_t,a = T_t[a][z_t,i] - own,
 *                    Binder  g_a = S m_a - 2 sum_t U_t,a                                  (int64)
 *                    VI      g_a = S phi(m_a) - 2 sum_t phi(U_t,a),  phi(n) = f(n + 1) - f(n), phi(0) = 0, the sum over
 *                            t ascending in binary64.
 *                  g_a - g_a0 is the change of the total when the row moves from a0 to a.  An empty slot scores 0 by
 *                  this very formula, and so does the row's own cluster when the row is alone in it: opening a new
 *                  cluster is no case of its own;
 *   move           the row goes to the slot with the smallest g; on exact ties its current slot wins, then the lowest;
 *   pass           the rows are cut into contiguous batches [k B, (k + 1) B); every row of a batch is scored against
 *                  the tables as they stood at the start of the batch, then the batch's moves are applied (n, T brought
 *                  up to date with integer adds, -1 / +1 per draw and moved row).  B = 1 is the sequential greedy;
 *   search         best = start; best_tot = total(start); B = batch
 *                  repeat up to max_passes times:
 *                      moved = one pass over c with batch B;  tot = total(c)
 *                      if moved == 0: converged; stop                            (c == best here)
 *                      if tot < best_tot: best, best_tot = c, tot               (strict)
 *                      else: c = best; if B == min_batch: stop; B = max(min_batch, B / 2)
 *                  total is binder2 under Binder and vi_tot under VI.  The result is never worse than the start;
 *                  converged means that no single-row move to any of the Ka slots lowers the loss.
 * Limits: 1 <= Kc <= BMM_PARTITION_SEARCH_MAX_K and the same for Ka (the tables of a draw live in LDS), S and N as
 * bmm_device_partition_distances (S N^2 < 2^63). */
#define BMM_PARTITION_SEARCH_MAX_K 64
typedef struct bmm_partition_search_opts {
    int64_t batch;     /* B of the first pass, >= 1 (above N: N) */
    int64_t min_batch; /* >= 1 (above batch: batch) */
    int max_passes;    /* >= 1 */
    int max_clusters;  /* Ka, 1 .. BMM_PARTITION_SEARCH_MAX_K */
} bmm_partition_search_opts;
/* NULL options mean batch = ceil(N / 8), min_batch = ceil(N / 256), max_passes = 50, Ka = Kc. */
typedef struct bmm_partition_search_out {
    int32_t* z_hat;          /* N int32, 1-based: the searched partition, in the slots' numbering */
    uint64_t* binder2;       /* its exact total sum_t 2 B(z_hat, z_t), under either criterion */
    double* loss;            /* its expected loss: binder2 / (2 S), or vi_tot / (S N) */
    double* start_loss;      /* the same two of the start */
    uint64_t* start_binder2;
    int* passes;             /* passes run, at most max_passes */
    int64_t* pass_batch;     /* per pass, room for max_passes each: its B, */
    int64_t* pass_moved;     /*   the rows it moved, */
    uint64_t* pass_binder2;  /*   binder2 of the state it left (before a restore), */
    double* pass_total;      /*   and that state's total as a double: binder2 converted, or vi_tot */
    int* converged;          /* 1: the last pass moved no row */
    int* n_clusters;         /* non-empty slots of z_hat */
} bmm_partition_search_out;
/* z as bmm_device_partition_distances takes it.  start: N int32 in 1 .. Ka, or NULL: the draws' minimiser of the
 * criterion at stride 1 (then Ka >= Kc).  BMM_E_ARG before a device is touched: the limits above, a start label outside
 * 1 .. Ka (the observation is named), batch, min_batch or max_passes below 1, a null z or out or a null buffer in out. */
int bmm_device_partition_search(int device, const int32_t* z, int S, int64_t N, int Kc, int criterion,
                                const int32_t* start, const bmm_partition_search_opts* opts,
                                const bmm_partition_search_out* out);
/* Which form of the k_ps_* kernels a shape runs, as pure bookkeeping -- no device is touched, and the values come from
 * the function the launches themselves call.  out:
 *   [0] bytes per label of the draws (1)          [1] cells from one label's run of slots to the next, KaP
 *   [2] threads per row, ceil(Ka / 8)             [3] rows per workgroup of k_ps_score
 *   [4] draws per LDS block, D                    [5] blocks of draws, ceil(S / D)
 *   [6] what bounds D: 0 S, 1 the LDS budget, 2 the 32-bit sums of a block (D N < 2^32)
 *   [7] bytes of dynamic LDS of k_ps_score        [8] workgroups of one k_ps_score launch, ceil(batch / [3])
 *   [9] batches of a pass, ceil(N / batch)        [10] 1: VI (binary64 tables and sums), 0: Binder (uint32, 32-bit sums
 *   within a block, 64-bit across)                [11] bytes of tables in global memory.
 * BMM_E_ARG as bmm_device_partition_search. */
int bmm_partition_search_plan(int S, int64_t N, int Kc, int Ka, int criterion, int64_t batch, int64_t out[12]);
/* For a run: armed per calling thread for the NEXT single-chain *_run* call, as bmm_set_partition_summary, and
 * disarmed when that call returns; out = NULL disarms, opts = NULL means the defaults.  Needs the partition summary
 * armed (its z_best may be NULL): the search takes the summary's criterion and starts from the row it chose, device to
 * device, after the summary and before the trace leaves, over the rows the summary used (n_used; with none usable
 * nothing is searched and out is left as it was).  BMM_E_ARG, before a device is touched, when no partition summary is
 * armed, the run's K is above BMM_PARTITION_SEARCH_MAX_K or max_clusters is below it.  Not armed: no allocation, no
 * launch.  The structs are copied; the buffers must stay valid through the call.  bmm_partition_out is not touched. */
int bmm_set_partition_search(const bmm_partition_search_opts* opts, const bmm_partition_search_out* out);

/* ---- credible ball and row-to-cluster similarity of the point estimate -----------------
 * How sure the estimate is: the credible ball of Wade & Ghahramani (2018) around one centre partition c under the
 * criterion, and how often every row sat with the members of every cluster of c.  In the notation of the block above:
 *   z_t (t < S)    the draws, labels in 0 .. Kc-1;
 *   c              the centre, labels in 0 .. Ka-1: Ka slots, of which any may be empty;
 *   n_a            the size of slot a;  T_t[a][b] = #{i : c_i = a, z_t,i = b};  n_t,b the size of label b of draw t;
 *   d2_t           = 2 B(c, z_t), uint64, exact;
 *   w_t            = N VI(c, z_t), binary64, F_c + F_t - 2 G_t in the order the search's totals fix, and exactly 0
 *                  where d2_t = 0;
 *   D_t            d2_t under Binder, w_t under VI.  Every comparison below is made on these values as the device
 *                  produced them: integer compares under Binder, binary64 compares under VI;
 *   k_t            the non-empty labels of draw t, #{b : n_t,b > 0};
 *   ball           the draws ordered by (D_t, t), m = min(S, max(1, ceil(level S))): the radius is the D of the m-th
 *                  draw in that order, the ball is {t : D_t <= radius}.  Ties at the radius are all inside: n_in >= m;
 *   horizontal     bound: the draws of the ball with the largest D_t (the radius, by construction): the lowest such t
 *                  and how many there are;
 *   upper          vertical upper bound: among the ball's draws with the smallest k_t those with the largest D_t: the
 *                  lowest such t, how many, k_t and D_t;
 *   lower          vertical lower bound: the same with the largest k_t;
 *   similarity     of a chosen row i to slot a: sim[i][a] = sum_t T_t[a][z_t,i], uint64, exact, a < Ka.  It equals
 *                  sum_{j : c_j = a} cnt[i, j] with cnt the similarity counts of bmm_device_psm; for a = c_i it
 *                  includes the row itself S times.
 * Derived by the caller: with own = [a = c_i], membership[i][a] = (sim[i][a] - S own) / (S (n_a - own)), the posterior
 * mean similarity of the row to the other members of the slot -- a soft membership that does not depend on how the
 * draws number their clusters (undefined for an empty slot and for a row alone in its cluster).
 * The radius and the three bounds are chosen on the host from the 24 S bytes of d2, w and k read back, O(S log S); the
 * three bounding rows leave the device as three rows.  The similarity is the device's one large pass, N Ka S table
 * reads for all rows.  Limits as the search: 1 <= Kc, Ka <= BMM_PARTITION_SEARCH_MAX_K, S N^2 < 2^63. */
typedef struct bmm_credible_bound {
    int* sweep;           /* the lowest draw (row of z, 0-based) attaining the bound */
    int* ties;            /* the draws attaining it */
    int* n_clusters;      /* k_t of those draws */
    double* dist;         /* their distance in the criterion's natural unit: B = d2 / 2, or VI = w / N */
    uint64_t* d2;         /* d2 of draw `sweep` */
    int32_t* z;           /* N int32, 1-based: draw `sweep` */
} bmm_credible_bound;     /* any pointer may be NULL */
typedef struct bmm_credible_ball_out {
    uint64_t* d2;              /* S: d2_t, under either criterion */
    double* dist;              /* S: d2_t / 2 under Binder, w_t / N under VI */
    int32_t* n_clusters;       /* S: k_t */
    double* radius;            /* the radius in the unit of dist */
    uint64_t* radius2;         /* d2 of the m-th draw in the order (D_t, t) */
    int* n_in;                 /* draws in the ball */
    bmm_credible_bound horizontal, upper, lower;
    uint64_t* sim;             /* member_M x Ka uint64, row-major ([u][a]); NULL: the similarity pass is not launched */
    const int64_t* member_idx; /* member_M observations, 0-based, any order, repeats allowed; NULL: all N rows in order
                                  (member_M is then taken as N) */
    int64_t member_M;
    int64_t* sizes;            /* Ka: n_a */
} bmm_credible_ball_out;       /* any output pointer may be NULL */
/* z as bmm_device_partition_distances takes it; centre: N int32 in 1 .. Ka.  BMM_E_ARG before a device is touched: Kc
 * or Ka outside 1 .. BMM_PARTITION_SEARCH_MAX_K, a centre label outside 1 .. Ka (the observation is named), level
 * outside (0, 1] or NaN, a member index outside 0 .. N-1, S N^2 >= 2^63, a null z, centre or out. */
int bmm_device_credible_ball(int device, const int32_t* z, int S, int64_t N, int Kc, int criterion,
                             const int32_t* centre, int Ka, double level, const bmm_credible_ball_out* out);
/* Which form of the k_cb_* kernels a shape runs, as pure bookkeeping -- no device is touched, and the values come from
 * the function the launches themselves call.  M: the chosen rows (N: all rows, read from the label block; fewer: a
 * gathered subset).  out:
 *   [0] bytes per label of the draws (1)          [1] cells from one label's run of slots to the next, KaP
 *   [2] threads per row, ceil(Ka / 8)             [3] rows per workgroup of k_cb_member
 *   [4] draws per LDS block, D                    [5] blocks of draws, ceil(S / D)
 *   [6] what bounds D: 0 S, 1 the LDS budget, 2 the 32-bit sums of a block (D N < 2^32)
 *   [7] bytes of dynamic LDS of k_cb_member       [8] workgroups of k_cb_member, ceil(M / [3])
 *   [9] 1: the labels of a subset are gathered first, 0: all rows, the label block is read directly
 *   [10] 1: VI (w_t computed), 0: Binder          [11] bytes of tables in global memory.
 * BMM_E_ARG as bmm_device_credible_ball, and unless 1 <= M. */
int bmm_credible_ball_plan(int S, int64_t N, int Kc, int Ka, int criterion, int64_t M, int64_t out[12]);
/* For a run: armed per calling thread for the NEXT single-chain *_run* call, as bmm_set_partition_search, and disarmed
 * when that call returns; out = NULL disarms.  Needs the partition summary armed: the ball takes the summary's
 * criterion, and its centre is the searched partition when a search is armed too, else the row the summary chose,
 * device to device; it runs over the rows the summary used (n_used; with none usable out is left as it was), after the
 * search and before the trace leaves.  The bounds' `sweep` are rows of the run's trace.  BMM_E_ARG, before a device is
 * touched, when no partition summary is armed, the run's K is above BMM_PARTITION_SEARCH_MAX_K, level is outside
 * (0, 1] or a member index is outside 0 .. N-1.  Not armed: no allocation, no launch.  The struct is copied; its
 * buffers must stay valid through the call (sizes and a row of sim hold Ka = the search's max_clusters, or K). */
int bmm_set_credible_ball(double level, const bmm_credible_ball_out* out);

/* ---- leave-one-out predictive of the fitted rows: LPML, WAIC ---------------------------
 * For the state s after a kept sweep and a fitted row i with label z_i, ell[s, i] is the log density of x_i given
 * everything else in the state:
 *   collapsed, dp  row i is taken out of the statistics, Nk' = Nk - [k = z_i], S'_kd = S_kd - x_id [k = z_i], N - 1 fitted
 *                  rows remain, and ell is the per-state predictive above of x_i for a chain fitted to those N - 1 rows:
 *                    collapsed  log sum_k (Nk' + alpha/K)/(N - 1 + alpha) prod_d (beta + S'_kd)^x (gamma + Nk' - S'_kd)^(1-x) / (beta + gamma + Nk')
 *                    dp         the same over the labels with Nk' > 0, weight Nk'/(N - 1 + alpha), plus the new cluster
 *                               alpha/(N - 1 + alpha) prod_d beta^x gamma^(1-x) / (beta + gamma)
 *                  with alpha_s the value the next sweep's conditional would use.  So a finite label that removing i has
 *                  emptied, or that was empty, keeps its prior weight (alpha/K)/(N - 1 + alpha) and the prior Bernoulli
 *                  terms (the model's term, not the sampler's "probability 0 for ever"); a DP row that sat alone has its
 *                  own label unused and is scored by the other used labels and the new cluster; away from those cases
 *                  ell is the log normaliser of the allocation conditional the sampler computes for row i at batch 1.
 *   sb, full       ell = log sum_k pi_k prod_d theta_kd^x (1 - theta_kd)^(1-x): the predictive above with the fitted rows
 *                  as the new rows.  The labels do not enter.
 * Only the states of the other rows enter ell for the collapsed model, and
 *   CPO_i^-1 = 1 / p(x_i | X_-i) = E[ 1 / p(x_i | X_-i, z_-i) | X ]      exactly:
 *     p(z_-i | X) = p(z_-i | X_-i) p(x_i | X_-i, z_-i) / p(x_i | X_-i)                           (Bayes, x_i as the datum)
 *     so sum_{z_-i} p(z_-i | X) / p(x_i | X_-i, z_-i) = sum_{z_-i} p(z_-i | X_-i) / p(x_i | X_-i)  (the factor cancels)
 *     = 1 / p(x_i | X_-i)                                                                          (p(z_-i | X_-i) sums to 1),
 * and z_-i of a draw of z | X is a draw of z_-i | X: the harmonic mean of exp(ell[s, i]) over the chain estimates CPO_i.
 * (For the explicit samplers the same identity holds with (pi, theta) in the place of z_-i.)
 * A state in which some row has no label -- a DP, stick-breaking or full chain before its first sweep -- is refused with
 * BMM_E_STATE and the chain stays usable.  Per row, over the S' folded states:
 *   log_cpo[i]  log S' - logsumexp_s(-ell)          ess[i]   exp(2 logsumexp(-ell) - logsumexp(-2 ell)), the effective
 *   lppd[i]     logsumexp_s(ell) - log S'                    sample size of the harmonic-mean weights, in [1, S']
 *   mean[i], var[i]  mean and sample variance (denominator S' - 1; NaN when S' = 1) of ell
 * and the scalars lpml = sum_i log_cpo, min_ess, n_folded, and -- for the two explicit samplers only, where ell is a log
 * likelihood -- p_waic = sum_i var, elpd_waic = sum_i lppd - p_waic (NaN for the counting samplers).  The sums over rows
 * run in an order fixed by N: 1024 partial sums, row i in partial i mod 1024, ascending; then a binary tree.  A row is
 * owned by one lane and nothing is atomic, so one seed gives the same bits twice.  Everything is enqueued on the chain's
 * stream behind the sweep's last kernel: a folded sweep adds no synchronisation and no host-device copy, an armed chain
 * that is not folding enqueues what an unarmed one does.  Not offered on a sharded chain, nor on the int32 layout of a
 * shape the resident kernels take (it reads the bit planes). */
typedef struct bmm_loo_out {
    double* log_cpo;    /* N doubles each; any may be NULL */
    double* ess;
    double* lppd;
    double* mean;
    double* var;
    double* lpml;       /* scalars; any may be NULL */
    double* min_ess;
    double* p_waic;
    double* elpd_waic;
    int* n_folded;
    double* ell;        /* whole runs only: S x N doubles column-major like logdens, or NULL */
} bmm_loo_out;
/* resident chains: arm (allocates 12 doubles per fitted row and, for the counting samplers, the two table sets; arming an
 * armed chain empties the accumulators) or disarm; needs the data */
int bmm_chain_set_loo(bmm_chain* c, int on);
/* ell of the current state, once: no sweep, accumulators untouched.  ell_out N doubles.  Waits. */
int bmm_chain_loo_state(bmm_chain* c, double* ell_out);
/* n more sweeps, each folded; ell_trace n x N column-major (then the call waits) or NULL (then it returns without
 * waiting, as bmm_chain_sweeps).  BMM_E_ARG, naming the bytes, when the trace does not fit in device memory. */
int bmm_chain_sweeps_loo(bmm_chain* c, int n, double* ell_trace);
/* the summary over the states folded so far (out->ell is ignored); the accumulators stay, so more sweeps may follow */
int bmm_chain_get_loo(bmm_chain* c, const bmm_loo_out* out);
int bmm_chain_loo_reset(bmm_chain* c);
/* For a run: armed per calling thread for the NEXT single-chain *_run* call of that thread (plain, _probs, _relabel,
 * _predict) and disarmed when that call returns, whatever it returns, exactly as bmm_set_partition_summary; NULL
 * disarms.  The struct is copied; its buffers must stay valid through that call.  Only kept sweeps (j >= burnin) are
 * folded; without burn-in the first kept row of the traces is the starting state, not a sweep: that row of ell is NaN
 * and is not folded.  bmm_multi_run does not take it and disarms it. */
int bmm_set_loo_summary(const bmm_loo_out* out);

/* ---- split-merge moves of the DP chain --------------------------------------------------
 * One-row-at-a-time Gibbs cannot move a block of rows between clusters; the split-merge Metropolis-Hastings move of
 * Jain & Neal (2004) can, and its accept step makes it exact whatever the parallelism of the proposal.  The model is
 * the DP Beta-Bernoulli mixture of the predictive section above, alpha the value the next sweep would use.  The move
 * applies to a DP chain whose rows are all seated, between sweeps (then no statistic deltas are pending: the end of a
 * sweep folds them).  THE MOVE, number m ahead of sweep j (tests/split_merge_ref.py restates it in NumPy):
 *   1. two distinct rows i, j uniformly; a = z_i, b = z_j.
 *   2. a == b: a split candidate; the second label is f, the smallest label with Nk = 0 below maxK; with none the
 *      move is SKIPPED (and counted).           3. a != b: a merge candidate; the two labels are a and b.
 *   4. members: the rows carrying either label, minus the two anchors.
 *   5. launch state: i on side 0 (the first label), j on side 1 (the second); every member on either side with
 *      probability 1/2 from its own uniform (side 0 iff u < 1/2), whatever its current label.
 *   6. `scans` >= 0 intermediate restricted scans: every member is redrawn between the two sides AT ONCE, scored
 *      against the two sides' statistics frozen at the start of that scan with its own contribution removed exactly,
 *      w_c = (n_c - [own]) prod_d (Beta-Bernoulli predictive of side c without the row) -- the terms k_resample uses
 *      for a used label; n_c - [own] >= 1 because of the anchors.  Side 0 iff u < w_0 / (w_0 + w_1).
 *   7. final scan: for a split of the same form, and drawn; log q = the sum over members of the log probability of
 *      the side drawn.  For a merge nothing is drawn; log q = the sum over members of the log probability, from the
 *      launch state (after the intermediate scans), of the side that is the member's current label.
 *   8. L(c) = sum_d [lgamma(beta + S_cd) + lgamma(gamma + n_c - S_cd) - lgamma(beta + gamma + n_c)]
 *             + P [lgamma(beta + gamma) - lgamma(beta) - lgamma(gamma)];
 *      split: log_prior = log alpha + lgamma(n_a') + lgamma(n_f') - lgamma(n_a), log_lik = L(a') + L(f') - L(a),
 *             log r = log_prior + log_lik - log q;
 *      merge: log_prior = -log alpha + lgamma(n_a + n_b) - lgamma(n_a) - lgamma(n_b), log_lik = L(a u b) - L(a) - L(b),
 *             log r = log_prior + log_lik + log q.
 *   9. accept iff log u < log r.
 *  10. commit: a split writes the proposed labels; a merge gives every row of the larger label the smaller one; Nk
 *      and S of the two labels are replaced by their exact integer values.  (The DP bookkeeping keeps nothing else
 *      derived from Nk on the device: the sweep finds its free label in the table image it builds per batch.)
 * Random streams, a pure function of (seed, sweep j, move m, row): the pair, u and a 32-bit salt from two
 * Philox4x32 blocks of stream 8 (c0 = m, c2 = j); a member's uniform of scan t (0 = launch) is Philox2x32 at counter
 * (row, 2^31 + t) keyed by the salt.  The sweeps' own row uniforms have a second counter word below 2^31, so none of
 * their (key, counter) pairs is reused.  Moves enqueued between sweeps j - 1 and j count on from the armed ones.
 * Determinism: log q is summed in an order fixed by N (1024 partial sums, row i in partial i mod 1024, ascending,
 * then a binary tree); the integer statistics use atomics; one seed gives the same bits twice.  lgamma is the
 * spec's lgamma_ (bmm_spec.h), the same bits on host and device.
 * The reference's DP sweep uses, for beta != gamma, a new-cluster term that is not the model's (see the predictive
 * section); the move targets the model.  A DP chain is created with beta == gamma only, where the two agree.
 * Refused: a sampler other than DP with BMM_E_UNSUPPORTED (the finite collapsed sampler gives an emptied label
 * probability 0 for ever, so its chain targets a different model from the one this ratio is for; the explicit
 * samplers carry pi and theta, which the move does not update), the int32 layout and P above 1024 with
 * BMM_E_UNSUPPORTED, an unseated or sharded chain with BMM_E_STATE. */
#define BMM_SM_SPLIT 0
#define BMM_SM_MERGE 1
#define BMM_SM_SKIPPED 2
#define BMM_SM_OUTSIDE 255 /* side byte of a row outside the two labels; 0 / 1 a member's side, 2 / 3 anchors i / j */
typedef struct bmm_split_merge_step {
    int64_t row_i, row_j;      /* 0-based */
    int32_t label_a, label_b;  /* 1-based: the first and the second label */
    int32_t kind;              /* BMM_SM_* */
    int32_t accepted;
    int64_t members;
    int64_t n_before[2];       /* sizes of the two labels before the move (split: n_a, 0) */
    int64_t n_after[2];        /* ... as proposed (split: n_a', n_f'; merge: n_a + n_b, 0) */
    double log_prior, log_lik, log_q, log_u, log_r;
    uint32_t sweep, move;      /* what keyed the move's streams */
    uint8_t* launch_side;      /* in: room for N side bytes, or NULL; the launch state */
    uint8_t* proposal_side;    /* in: the same; the state the final scan drew (split) or scored from (merge) */
} bmm_split_merge_step;
/* moves_per_sweep moves at the start of every sweep from the second, before its first table build (so the theta-hat
 * and the label row a sweep records belong together); 0 turns them off.  An unarmed chain enqueues what it always did. */
int bmm_chain_set_split_merge(bmm_chain* c, int moves_per_sweep, int scans);
/* n moves now, with the scans last set (returns without waiting) */
int bmm_chain_split_merge(bmm_chain* c, int n);
/* one move, then waits; fills *out (set launch_side / proposal_side first) */
int bmm_chain_split_merge_step(bmm_chain* c, bmm_split_merge_step* out);
/* proposed splits, accepted splits, proposed merges, accepted merges, skipped.  Waits. */
int bmm_chain_split_merge_stats(bmm_chain* c, int64_t out[5]);
/* Replaces the allocation of a seated DP chain between sweeps (1-based labels, validated on the device, BMM_E_ARG
 * naming the first bad row and the chain unchanged) and recounts Nk and S: warm starts.  Waits. */
int bmm_chain_set_labels(bmm_chain* c, const int32_t* z1);
/* For a run: armed per calling thread for the NEXT single-chain *_run* call of that thread and disarmed when it
 * returns, as bmm_set_loo_summary; moves_per_sweep = 0 disarms.  The run's five counts are read afterwards with
 * bmm_last_split_merge_stats.  bmm_multi_run does not take it and disarms it. */
int bmm_set_split_merge(int moves_per_sweep, int scans);
int bmm_last_split_merge_stats(int64_t out[5]);

/* ---- feature selection for the counting samplers ------------------------------------------
 * In questionnaire or clinical data many of the P binary features say nothing about the clusters.  The variable-selection
 * collapsed Gibbs sampler of White, Wyse & Murphy (2016) gives every feature an inclusion indicator and samples it with
 * the allocation.  THE MODEL: gamma_d ~ Bernoulli(rho), independently, for every feature d;
 *   gamma_d = 1  feature d clusters: theta_kd ~ Beta(beta, gamma) per cluster -- the model of the rest of this header;
 *   gamma_d = 0  feature d is noise: one rate theta_0d ~ Beta(beta, gamma) shared by every row.
 * theta is integrated out throughout.  Offered for BMM_SAMPLER_COLLAPSED and BMM_SAMPLER_DP.
 *   z-step      the sampler's own conditional with the product over d running over gamma_d = 1 only: a noise
 *               feature's predictive term is the same for every category and cancels.  The tables the resample
 *               kernels read hold 0 for an excluded feature -- both terms, full and own-cluster tables -- and the DP's
 *               new-cluster term counts the included features, P_in (log beta - log(beta + gamma)); the resample kernels
 *               themselves are the ones every chain runs.
 *   gamma-step  with lB(x, y) = lgamma(x) + lgamma(y) - lgamma(x + y), T_d = sum_k S_kd and the counts as the end of
 *               the sweep folded them,
 *                 Lambda_d = log rho - log(1 - rho)
 *                            + sum_{k : N_k > 0} [ lB(beta + S_kd, gamma + N_k - S_kd) - lB(beta, gamma) ]
 *                            - [ lB(beta + T_d, gamma + N - T_d) - lB(beta, gamma) ],
 *                 p_d = 1 / (1 + exp(-Lambda_d)),   gamma_d = [u_d < p_d].
 *               Given the labels the P indicators are independent, so one launch redraws them all exactly.  An empty
 *               cluster is skipped, not added as a zero; the sum runs in an order fixed by K (lane l of a wave adds
 *               the terms of clusters l, l + 64, ... in ascending order, the all-rows term counting as entry K of
 *               that walk, subtracted; the 64 partial sums are added by a butterfly; log rho - log(1 - rho) last).
 *               u_d is the 53-bit uniform of the first Philox4x32 block of stream 9 at counter (c0 = d, block 0,
 *               c2 = sweep j) under the chain's key: no (key, counter) pair of any other stream.  lgamma, log and exp
 *               are the spec's (bmm_spec.h), the same bits on host and device.
 *   order       inside sweep j: z is resampled against the mask of sweep j - 1, the sweep end folds the counts (theta-hat
 *               and alpha as ever), then gamma is drawn from those counts; trace row j records that gamma.  The initial
 *               mask is all ones.  The step is stream-ordered behind the sweep end: no host wait.
 * inclusion[d] is the mean of the draws over the folded steps, inclusion_rb[d] the mean of p_d (the Rao-Blackwellised
 * estimate of the same probability; one binary64 add per step, so one seed gives the same bits twice).
 * A chain that was never given a mask enqueues exactly what it always did.  A chain with a mask builds its tables with
 * the masked flavour of the table kernel and never takes the form whose workgroups build their own tables
 * (bmm_chain_kernel_form reports what runs); its values with the all-ones mask are those of a chain without one.
 * Refused: the stick-breaking and full samplers (they carry theta) and a run of the DP sampler with beta != gamma (its
 * new-cluster term is the model's only when they are equal; a resident DP chain is created with beta == gamma only)
 * with BMM_E_UNSUPPORTED; a chain with a mask combined with newdata,
 * the leave-one-out summary or split-merge moves, in either order, with BMM_E_UNSUPPORTED -- their tables and ratios
 * are written for the all-features model; the selection model's versions are a follow-up; a sharded chain, a chain
 * without data and a finite chain without initial labels (rows that cannot be seated yet) with BMM_E_STATE; rho
 * outside (0, 1) with BMM_E_ARG. */
typedef struct bmm_feature_step {
    double* lambda;   /* in: room for P doubles each, or NULL: Lambda_d, p_d, u_d of the last step */
    double* p;
    double* u;
    uint8_t* gamma;   /* in: room for P bytes, or NULL: the indicators it drew */
    uint32_t sweep;   /* out: the sweep it followed (what keyed its uniforms) */
} bmm_feature_step;
/* on != 0: a gamma-step behind every sweep from now on, every step folded; arming empties the accumulators.  on = 0:
 * no more steps; the mask stays as it is. */
int bmm_chain_set_feature_select(bmm_chain* c, int on, double rho);
/* the mask, between sweeps: gamma[d] in {0, 1}, P bytes.  set waits; get waits and gives all ones for a chain that
 * never had a mask. */
int bmm_chain_set_features(bmm_chain* c, const uint8_t* gamma);
int bmm_chain_get_features(bmm_chain* c, uint8_t* gamma);
/* the last step's record.  Waits. */
int bmm_chain_feature_step(bmm_chain* c, bmm_feature_step* out);
/* n more sweeps of an armed chain, returning the indicators after each: gamma_trace is n x P bytes, row-major (sweep,
 * feature).  Waits. */
int bmm_chain_sweeps_features(bmm_chain* c, int n, uint8_t* gamma_trace);
/* inclusion, inclusion_rb (P doubles each, either may be NULL; NaN while nothing is folded) and the number of folded
 * steps; the accumulators stay, so more sweeps may follow */
int bmm_chain_get_feature_summary(bmm_chain* c, double* inclusion, double* inclusion_rb, int* n_folded);
int bmm_chain_feature_reset(bmm_chain* c);
/* For a run: armed per calling thread for the NEXT single-chain collapsed or DP *_run* call of that thread and
 * disarmed when that call returns, whatever it returns, as bmm_set_split_merge and bmm_set_loo_summary; NULL disarms.
 * The struct is copied; its buffers must stay valid through that call.  Only kept sweeps (j >= burnin) are recorded
 * and folded; without burn-in the first kept row is the starting state: its indicators are the initial mask (all
 * ones) and it is not folded.  bmm_multi_run does not take it and disarms it. */
typedef struct bmm_feature_out {
    double rho;
    uint8_t* gamma;        /* S x P bytes, row-major (kept sweep, feature) */
    double* inclusion;     /* P doubles */
    double* inclusion_rb;  /* P doubles */
    int32_t* n_selected;   /* S ints: the included features per kept sweep */
    int* n_folded;         /* or NULL */
} bmm_feature_out;
int bmm_set_feature_select(const bmm_feature_out* out);

/* ---- k-modes++ initial allocation of the counting samplers ------------------------------------
 * A data-driven start computed on the device from the resident bit planes: k-means++ seeding under Hamming distance
 * (for 0/1 data the squared Euclidean distance, so D^2 sampling is Hamming-weighted sampling), then a few k-modes
 * rounds.  Integer arithmetic throughout but for one product per centre, so the result does not depend on the launch
 * geometry and is the same on host and device (tests/init_ref.py restates it in NumPy).  THE DEFINITION.  Inputs: the
 * planes Xb[w][N], W = ceil(P/32) words per row, the last word masked to its P valid bits on both sides of every
 * comparison; Kc centres, 1 <= Kc <= K; seed; iters >= 0.
 *   draws       init_uniform(seed, j) = u01(x, y) of the first Philox4x32 block of stream 10 (bmm_spec.h kStreamInit) at
 *               counter (c0 = j, block 0, c2 = 0), j = 0 .. Kc - 1: no (key, counter) pair of any other draw.
 *   seeding     r_0 = min(N - 1, (int64)(u_0 * (double)N)); centre 0 is row r_0.  Per row dist[i] (int32, initially
 *               P + 1) and near[i].  After centre m is fixed, h = sum over words of popcount(x_i[w] ^ c_m[w]); if
 *               h < dist[i] (strict: ties go to the lowest label) then dist[i] = h, near[i] = m.  For j = 1 .. Kc - 1:
 *               T = sum_i dist[i] (int64; N P < 2^53, so (double)T is exact); T == 0: every row coincides with a centre,
 *               stop with k_eff = j; otherwise t = min(T - 1, (int64)(u_j * (double)T)), r_j = the smallest i whose
 *               inclusive prefix sum of dist exceeds t, centre j is row r_j.  Without a stop k_eff = Kc.
 *   refinement  at most `iters` rounds of k-modes from the labels `near`.  (a) Nk and S of the current labels; bit d of
 *               centre k becomes 1 if 2 S_kd > Nk, 0 if 2 S_kd < Nk, and keeps its value on a tie or when Nk == 0.
 *               (b) every row takes the nearest centre among 0 .. k_eff - 1, ties to the lowest label; `changed` = the
 *               rows whose label differs from before.  A round with changed == 0 ends the refinement.
 *   result      0-based labels in [0, k_eff); the centres (k_eff x W words); the picked rows; the final Nk; and
 *               {k_eff, rounds_run, changed_last, cost}: rounds_run counts the rounds executed (the one that found
 *               changed == 0 included), changed_last is the last of them's `changed` (0 when iters = 0), cost the sum
 *               over rows of the Hamming distance to the row's own centre (after seeding: the sum of dist).  With this
 *               tie rule the cost never increases from one round to the next.
 * One initialisation is 2 Kc - 1 seeding launches, one seating launch (nearest seeded centre per row, which is `near`,
 * and the counts of those labels) and two launches per round, all enqueued at once on the chain's stream; flags on the
 * device make the launches left over after a stop or after convergence return at once, and the record is read after one
 * final wait.  Kc * W * 4 above BMM_INIT_MAX_CENTRE_BYTES is refused with BMM_E_UNSUPPORTED, the chain stays usable. */
#define BMM_INIT_KMODES 1
#define BMM_INIT_MAX_CENTRE_BYTES 65536
typedef struct bmm_init_info {
    int32_t k_eff, rounds_run;
    int64_t changed_last, cost;
    double device_ms;  /* HIP-event time of the launches of this initialisation */
} bmm_init_info;
/* n_centres = 0: K for the collapsed sampler; must be given for the DP sampler.  A collapsed chain that has its data
 * and has not started gets its initial labels on the device and is left exactly as bmm_chain_set_initial_labels leaves
 * it: no label crosses PCIe.  A seated DP chain between sweeps and outside a run gets a new allocation and the recount
 * of Nk and S, as bmm_chain_set_labels.  Waits.  Refused: a sharded chain, a collapsed chain already started, an
 * unseated DP chain, a chain inside a run with BMM_E_STATE; the stick-breaking and full samplers (they start from pi
 * and theta) and the int32 layout with BMM_E_UNSUPPORTED; n_centres outside 1..K and iters < 0 with BMM_E_ARG. */
int bmm_chain_init_labels(bmm_chain* c, int kind, int n_centres, int iters, bmm_init_info* info);
/* of the last initialisation of this chain: the centres, k_eff x ceil(P/32) words; the picked rows (k_eff, 0-based)
 * and, unless NULL, the final cluster sizes (k_eff) */
int bmm_chain_get_init_centres(bmm_chain* c, uint32_t* words);
int bmm_chain_get_init_rows(bmm_chain* c, int64_t* rows, int32_t* Nk);
/* For a run: armed per calling thread for the NEXT single-chain bmm_collapsed_run* call of that thread and disarmed
 * when it returns, as bmm_set_split_merge; kind = 0 disarms.  The run initialises on the device once the planes have
 * arrived and ignores the initialK it is handed (which must still be there); its record is read afterwards with
 * bmm_last_init_info.  A run of another sampler made while armed returns BMM_E_UNSUPPORTED (and disarms);
 * bmm_multi_run does not take it and disarms it. */
int bmm_set_init(int kind, int iters);
int bmm_last_init_info(bmm_init_info* info);

/* ---- the allocation sampler: unknown K for the finite chain ----------------------------------
 * The finite collapsed sampler fixes K; the DP sampler frees it but puts no prior on it.  The allocation sampler of Nobile
 * & Fearnside (2007) runs the finite model with K in the state and a prior on it, and gives a posterior p(K | x).
 * THE MODEL AND THE CHAIN (tests/alloc_ref.py restates them in NumPy).  State (K, z), 1 <= K <= maxK, z in {0..K-1}^N.
 * K ~ p(K), a caller-supplied vector of maxK log probabilities; weights ~ Dirichlet(a, ..., a) with a fixed a > 0 PER
 * COMPONENT (not alpha / K); theta_kd ~ Beta(beta, gamma).  With the weights and theta integrated out,
 *   log pi(K, z) = log p(K) + lgamma(K a) - lgamma(K a + N) + sum_k [lgamma(a + n_k) - lgamma(a)] + sum_k L(k),
 * L the L(c) of the split-merge section, 0 for an empty label.
 *   sweep   the finite sampler's sweep with the table build k_count_tables<TAB_ALLOC>: label k < K scores log(n + a) - log(N - 1
 *           + K a) plus the Beta-Bernoulli terms of its statistics -- the prior terms when it is empty, so an emptied
 *           label can be taken again; the row's own label with the row removed, log(n - 1 + a) - ..., so a row that
 *           sits alone keeps its label at prior weight; labels from K on are closed.  K is read from the device: no
 *           host wait.  The resample kernels are the ones every chain runs (they draw from the table image alone);
 *           the form whose workgroups build their own tables is never chosen, and above 128 features the sweeps run on
 *           the generic kernel, which reads the same image.
 *   move    eject / absorb (section 3.2 of the paper, p_E integrated out of the proposal density), number m ahead of
 *           sweep j.  Eject with probability pe_K (pe_1 = 1, pe_maxK = 0, else 1/2), otherwise absorb.
 *           eject   j1 uniform over the K labels, j2 = K the appended label, p_E ~ Beta(e, e); every row of j1 moves to
 *                   j2 iff its own uniform is < p_E; n1', n2' the proposed sizes (either may be 0);
 *                   log q = lbeta(e + n1', e + n2') - lbeta(e, e);
 *                   log_prior = log p(K+1) - log p(K) + [lgamma((K+1)a) - lgamma((K+1)a + N)] - [lgamma(K a) - lgamma(K a + N)]
 *                               + lgamma(a + n1') + lgamma(a + n2') - lgamma(a + n) - lgamma(a),
 *                   log_lik = L(j1') + L(j2') - L(j1), log_move = log(1 - pe_{K+1}) - log pe_K,
 *                   log r = log_prior + log_lik + log_move - log q.
 *           absorb  an ordered pair (j1, j2), j1 != j2, uniform over the K (K - 1) pairs; every row of j2 takes j1, then
 *                   the rows of label K - 1 take j2 (when j2 != K - 1), K falls by one.  log r is the negative of the
 *                   eject's with n1' = n_j1, n2' = n_j2 and K - 1 in the eject's role; log_prior and log_lik are
 *                   reported negated, log_q and log_move as the eject's: log r = log_prior + log_lik - log_move + log q.
 *           accept iff log u < log r; the commit writes the labels, the exact integer Nk and S of the labels touched
 *           (the swapped label included) and K.
 * The labelled chain is valid on the lumped state (K, partition): tests/test_alloc_ref.py builds the exact transition
 * matrices of the move and of a batch-1 sweep on a small data set and holds them to detailed balance.
 * Random streams, a pure function of (seed, sweep j, move m, row): kind, j1, u, the salt and an absorb's j2 from three
 * Philox4x32 blocks of stream 11 (c0 = m, c2 = j), p_E from streams 12 and 13 (the spec's rbeta_); a row's uniform is
 * Philox2x32 at counter (row, 2^31) under the salt, as a split-merge member's.  The sums over features run in an order
 * fixed by P (feature d in partial d mod 1024, ascending, then a binary tree); lgamma is the spec's lgamma_.
 * A chain is the finite collapsed one created with K = maxK and alpha = a (the per-component parameter); arming it is
 * for good.  K starts at maxK; bmm_chain_set_k changes it between sweeps.
 * Refused with BMM_E_UNSUPPORTED: a sampler other than the finite collapsed one, alpha = 0 (the concentration's update
 * does not apply: a is fixed), a chain with a feature mask, newdata or the leave-one-out summary, and those on an armed
 * chain, as the probability hand-off of the relabelling (their tables assume a fixed K), the int32 layout, P above 1024,
 * maxK above 64; a sharded chain or one without data or initial labels with BMM_E_STATE.  bmm_multi_run does not take it. */
#define BMM_EA_EJECT 0
#define BMM_EA_ABSORB 1
#define BMM_EA_OUTSIDE 255 /* side byte of a row the move does not touch.  Eject: 0 a row of j1 that stays, 1 one that
                            * moves to j2.  Absorb: 0 a row of j1, 1 a row of j2, 2 a row of label K - 1 that takes j2
                            * (j2 != K - 1; with j1 == K - 1 the rows of j1 carry 2) */
typedef struct bmm_alloc_step {
    int32_t kind, accepted;    /* BMM_EA_* */
    int32_t j1, j2;            /* 1-based */
    int32_t k_before, k_after;
    uint64_t pe_bits;          /* the bits of p_E (a NaN for an absorb, which draws none) */
    int64_t members;           /* rows moved: n2' */
    int64_t n_before[2];       /* sizes of j1 and j2 before the move (eject: n_j1, 0) */
    int64_t n_after[2];        /* ... as proposed (eject: n1', n2'; absorb: n_j1 + n_j2, 0) */
    double log_prior, log_lik, log_q, log_move, log_u, log_r;
    uint32_t sweep, move;      /* what keyed the move's streams */
    uint8_t* side;             /* in: room for N side bytes, or NULL */
} bmm_alloc_step;
/* arms the chain (for good) and sets log p(K), K = 1..maxK, every one finite, the moves at the start of every sweep from
 * the second, before its first table build (0: sweeps with open empty labels only), and e of p_E ~ Beta(e, e) */
int bmm_chain_set_alloc(bmm_chain* c, const double* log_prior_k, int moves_per_sweep, double eject_a);
/* K between sweeps: every label above it must be empty (BMM_E_ARG otherwise).  Waits. */
int bmm_chain_set_k(bmm_chain* c, int K);
int bmm_chain_get_k(bmm_chain* c, int* K);
/* n moves now (returns without waiting) */
int bmm_chain_alloc(bmm_chain* c, int n);
/* one move, then waits; fills *out (set side first) */
int bmm_chain_alloc_step(bmm_chain* c, bmm_alloc_step* out);
/* proposed ejects, accepted ejects, proposed absorbs, accepted absorbs.  Waits. */
int bmm_chain_alloc_stats(bmm_chain* c, int64_t out[4]);
/* One call, shaped like bmm_collapsed_run: initialK holds 1-based labels in 1..K0, theta_out is maxK x P x S with NaN
 * where a label is empty, k_out S int32: K after every kept sweep (row 0 of a run without burn-in: K0), moves_out the four
 * counts or NULL.  bmm_set_partition_summary combines with it; relabelling, feature selection, split-merge moves, the
 * leave-one-out summary, newdata and a device start armed for the call make it return BMM_E_UNSUPPORTED. */
int bmm_alloc_run(const int32_t* X, int64_t N, int P, const int32_t* initialK, int nsamples, int maxK, double a,
                  double beta, double gamma, const double* log_prior_k, int K0, int moves_per_sweep, double eject_a,
                  int burnin, int64_t batch, uint64_t seed, int device, int32_t* z_out, double* theta_out,
                  int32_t* k_out, int64_t moves_out[4]);

/* ---- split-merge moves of the allocation sampler ---------------------------------------------
 * Eject / absorb cuts a component by a coin per row; at large N such a cut is never accepted (section 18).  These moves
 * propose the cut along the data, by the restricted scans of the DP chain's split-merge move above, under the allocation
 * sampler's target.  A split opens component K + 1, a merge closes one; the number of empty open components does not
 * change.  The state is (K, z) as above; on the lumped state (K, partition rho with t non-empty blocks) the target is
 *   pi(K, rho) = p(K) K! / (K - t)! Gamma(K a) / Gamma(K a + N) prod_c Gamma(a + n_c) / Gamma(a) prod_c m(x_c).
 * THE MOVE, number m ahead of sweep j (tests/alloc_split_ref.py restates it in NumPy):
 *   1. an ordered pair of distinct rows (i, j), the accept uniform and a salt as the DP move draws them, from stream 18.
 *   2. z_i == z_j: a split of that block, la = z_i, lb = K, the first closed label; SKIPPED (and counted) when K == maxK.
 *      z_i != z_j: a merge of la = z_i and lb = z_j.
 *   3. launch state, `scans` intermediate restricted scans and the final scan as steps 4 to 7 of the DP move, with the
 *      prior of the allocation model between the two sides: w_c = (n_c - [own] + a) prod_d (predictive of side c without
 *      the row).  log q as there.
 *   4. split of n into n0 (stays la, holds i) and n1 (takes label K, holds j), K -> K + 1:
 *        log_prior = log p(K+1) - log p(K) + log(K + 1)
 *                    + [lgamma((K+1)a) - lgamma((K+1)a + N)] - [lgamma(K a) - lgamma(K a + N)]
 *                    + lgamma(a + n0) + lgamma(a + n1) - lgamma(a + n) - lgamma(a)      (as_log_prior of bmm_spec.h),
 *        log_lik the DP move's, log r = log_prior + log_lik - log q.  log(K + 1) is the lumping factor
 *        (K+1)! / (K-t)! over K! / (K-t)!: it is not in the labelled log pi(K, z).
 *      merge at K -> K - 1: the exact negative of the split from K - 1 with the roles swapped,
 *        log r = log_prior + log_lik + log q.
 *   5. accept iff log u < log r.  A split gives the rows of side 1 label K and sets Nk, S of both labels to their exact
 *      integer values; a merge gives the rows of lb label la, adds the statistics and then, as an absorb, moves label
 *      K - 1 into lb (rows, Nk, S) unless lb == K - 1.  K is written on the device.
 * The moves sit behind the sweep's eject / absorb moves and ahead of its first table build.  One seed gives the same bits
 * twice; the sums run in the DP move's fixed orders.  Refused: whatever bmm_chain_set_alloc refuses, a chain that is not
 * armed with BMM_E_STATE, N < 2 with BMM_E_ARG.  bmm_chain_set_split_merge stays refused on an armed chain, and
 * bmm_set_split_merge ahead of bmm_alloc_run. */
typedef struct bmm_alloc_split_step {
    int64_t row_i, row_j;      /* 0-based */
    int32_t label_a, label_b;  /* 1-based: la and lb (a split: lb = K + 1, the label opened) */
    int32_t kind;              /* BMM_SM_* */
    int32_t accepted;
    int32_t k_before, k_after;
    int32_t moved, pad;        /* 1-based: the label a committed merge moved into the gap, or -1 */
    int64_t members;
    int64_t n_before[2];       /* sizes of the two labels before the move (split: n, 0) */
    int64_t n_after[2];        /* ... as proposed (split: n0, n1; merge: n_a + n_b, 0) */
    double log_prior, log_lik, log_q, log_u, log_r;
    uint32_t sweep, move;      /* what keyed the move's streams */
    uint8_t* launch_side;      /* in: room for N side bytes (BMM_SM_OUTSIDE ...), or NULL; the launch state */
    uint8_t* proposal_side;    /* in: the same; the state the final scan drew (split) or scored from (merge) */
} bmm_alloc_split_step;
/* moves_per_sweep moves at the start of every sweep from the second, behind its eject / absorb moves; 0 turns them off
 * (and still sets the scans of the moves below).  A chain with none armed enqueues what it always did. */
int bmm_chain_set_alloc_split_merge(bmm_chain* c, int moves_per_sweep, int scans);
/* n moves now, with the scans last set (returns without waiting) */
int bmm_chain_alloc_split_merge(bmm_chain* c, int n);
/* one move, then waits; fills *out (set launch_side / proposal_side first) */
int bmm_chain_alloc_split_merge_step(bmm_chain* c, bmm_alloc_split_step* out);
/* proposed splits, accepted splits, proposed merges, accepted merges, skipped.  Waits. */
int bmm_chain_alloc_split_merge_stats(bmm_chain* c, int64_t out[5]);
/* For a run: armed per calling thread for the NEXT bmm_alloc_run of that thread and disarmed when it returns; any other
 * run answers it with BMM_E_UNSUPPORTED.  The run's five counts are read with bmm_last_alloc_split_merge_stats. */
int bmm_set_alloc_split_merge(int moves_per_sweep, int scans);
int bmm_last_alloc_split_merge_stats(int64_t out[5]);

/* ---- label-switching correction from the label trace alone: ECR ------------------------------
 * Equivalence Classes Representatives (Papastamoulis & Iliopoulos 2010) and its pivot-free iterative form
 * ECR-ITERATIVE-1 (Rodriguez & Walker 2014; Papastamoulis 2016): every kept sweep gets the permutation of its labels
 * that agrees with a pivot allocation on as many observations as possible.  No probability matrix is needed, any
 * burn-in will do.  Labels are 0-based in these definitions (1-based at the interfaces, as z_out); z_t is row t of an
 * S x N trace with labels in 0 .. K-1, c a pivot of N labels in 0 .. K-1.
 *   table        n_t[a, b] = #{i : z_t[i] = a, c[i] = b}, an exact integer (uint32; N < 2^32);
 *   permutation  perm_t maximises agree_t = sum_a n_t[a, perm_t[a]]: the min-cost assignment on the K x K column-major
 *                matrix C[b + a K] = -(double) n_t[a, b] (rows: pivot labels, columns: draw labels) by the Hungarian
 *                method of the Stephens path, unchanged (rows enter in index order, the lowest column index wins a
 *                tie).  Its "perm[l] = the row assigned to column l" reads "draw label l leaves as pivot label
 *                perm[l]": the convention of bmm_relabel_out.permutations, z = perm[z], theta_relab[perm[k]] =
 *                theta[k].  The costs are integers below 2^53, so the potentials stay exact;
 *   iterative    (no pivot given) perm_t = identity; iteration it = 1, 2, ...: c[i] = the label with the most votes
 *                among perm_t[z_t[i]] over the rows used, the lowest label on a tie; tables and permutations as above;
 *                total_it = sum_t agree_t, an exact int64, which never decreases.  The loop stops after the first
 *                iteration with total_it == total_(it-1) (converged = 1) or after max_iter iterations (converged = 0),
 *                and returns the permutations, agreements and pivot of the last iteration run.  With a pivot given:
 *                one pass, iterations = 1, converged = 1;
 *   unused rows  trace row 0 of a run without burn-in is unassigned for every sampler but the finite collapsed one:
 *                it is left out of votes and totals, its permutation is the identity, its agree 0, and n_used = S - 1.
 * Nothing is floating point but the cost handed to the assignment; all counting is integer adds, so two calls give
 * the same bits.  One synchronising copy of 8 bytes (total_it) per iteration is the loop's only host round trip. */
#define BMM_ECR_MAX_K BMM_STEPHENS_MAX_K
#define BMM_ECR_PIVOT_GIVEN 0
#define BMM_ECR_PIVOT_PARTITION 1
#define BMM_ECR_PIVOT_ITERATIVE 2
/* Any stack of rows over the same observations (traces of several chains can be stacked by the caller).  z: S x N int32
 * column-major, 1-based; pivot: N labels, 1-based, or NULL for the iterative form (max_iter >= 1 then).  perm_out S x K
 * int32 column-major, 0-based; agree_out S int64; pivot_out N int32, 1-based, or NULL: the pivot of the last iteration;
 * z_out S x N as z, relabelled (z_out = perm[z - 1] + 1, applied by the host's cores), or NULL; tables_out S x K x K
 * uint32 or NULL, n_t[a, b] at [(t K + a) K + b]; iterations, converged as above.  BMM_E_ARG, before a device is
 * touched, unless 1 <= S <= BMM_PARTITION_MAX_ROWS, N >= 1, 1 <= K <= BMM_ECR_MAX_K, and for a label of z or of the
 * pivot outside 1 .. K (the row and the observation are named). */
int bmm_device_ecr(int device, const int32_t* z, int S, int64_t N, int K, const int32_t* pivot, int max_iter,
                   int32_t* perm_out, int64_t* agree_out, int32_t* pivot_out, int32_t* z_out, uint32_t* tables_out,
                   int* iterations, int* converged);
/* Which form of the k_ecr_* kernels a shape runs, as pure bookkeeping -- no device is touched, and the values come from
 * the function the launches themselves read.  out:
 *   [0] bytes per label of the stand-alone call's device block (1; a run reads its resident int32 trace: 4)
 *   [1] 1: tables in LDS; 0: the generic form, adds straight to the global tables (a table above 48 KiB, K > 110)
 *   [2] label rows per workgroup, T               [3] copies of each table in LDS, R (across the lanes of a wave)
 *   [4] blocks of rows, ceil(S / T)               [5] slices of observations (the grid is [5] x [4] workgroups)
 *   [6] observations per slice                    [7] bytes of dynamic LDS of the tables pass (0: generic)
 *   [8] 1: vote counters in LDS; 0: the generic form, counters in global memory (K > 96)
 *   [9] workgroups of the votes pass              [10] its bytes of dynamic LDS, or of global counters (generic)
 *   [11] labels per row of the stand-alone call's device block (N rounded up to 16).
 * BMM_E_ARG unless 1 <= S <= BMM_PARTITION_MAX_ROWS, N >= 1 and 1 <= K <= BMM_ECR_MAX_K. */
int bmm_device_ecr_plan(int S, int64_t N, int K, int64_t out[12]);
/* For a run: armed per calling thread for the NEXT single-chain *_run* call of that thread and disarmed when that call
 * returns, whatever it returns, like bmm_set_partition_summary; NULL disarms.  The struct is copied; its buffers must
 * stay valid through that call.  After the last sweep (and after the partition summary, when one is armed) the run
 * computes the permutations from the resident trace, and then z_out / theta_out receive the relabelled traces (z =
 * perm[z - 1] + 1, theta_relab(perm(k), d, s) = theta(k, d, s)) and z_original / theta_original the traces as sampled,
 * as a *_run_relabel call leaves them.  Any burnin >= 0; combines with the partition and leave-one-out summaries,
 * newdata, feature selection, split-merge moves and a device start.  BMM_ECR_PIVOT_PARTITION takes the row the armed
 * partition summary chose, straight from the device: BMM_E_ARG, before a device is touched, when none is armed.
 * BMM_E_ARG together with a *_run_relabel call or *_run_probs hooks (two relabellings), BMM_E_UNSUPPORTED for
 * bmm_alloc_run; bmm_multi_run disarms it like any other run.  Its time is counted in phases [3] and [4] of
 * bmm_last_run_phases. */
typedef struct bmm_ecr_out {
    int pivot_kind;          /* BMM_ECR_PIVOT_GIVEN, _PARTITION or _ITERATIVE */
    const int32_t* pivot;    /* _GIVEN: N labels, 1-based; else ignored */
    int max_iter;            /* _ITERATIVE: >= 1; else ignored */
    int32_t* permutations;   /* S x K int32 column-major, 0-based */
    int32_t* z_original;     /* S x N as z_out: the labels as sampled */
    double* theta_original;  /* K x P x S as theta_out: theta as sampled */
    int64_t* agree;          /* S */
    int32_t* pivot_out;      /* N int32, 1-based (0 when no row was usable), or NULL */
    int* iterations;
    int* converged;
    int* n_used;             /* rows used */
} bmm_ecr_out;
int bmm_set_ecr_relabel(const bmm_ecr_out* out);

/* ---- log joint trace and keep-best (MAP) allocation ------------------------------------------
 * The number every MCMC user plots first: log p(x, z, alpha, mask) of the state after a kept sweep, from the integer
 * statistics the sweep end has folded -- no pass over X.  n_k, s_kd: the folded counts of the state after kept sweep j;
 * alpha_j: the concentration after that sweep's update (the value in the alpha trace row); lgamma, log: the spec's lgamma_
 * and log_ (bmm_spec.h), the same bits on host and device; lB0 = lgamma(beta) + lgamma(gamma) - lgamma(beta + gamma).
 *   log_lik    log p(x | z), theta integrated out -- for all five samplers, the explicit ones included, from the counts:
 *              the sum over the labels k with n_k > 0 and the features d of
 *                ((lgamma(beta + s_kd) + lgamma((gamma + n_k) - s_kd)) - lgamma(beta + gamma + n_k)) - lB0.
 *              An empty label is skipped, not added as a zero (the per-cell term of the feature-selection step).  With a
 *              feature mask an excluded feature contributes, once instead of per label, the pooled term of that section:
 *              the same expression with (N, T_d), T_d = sum_k s_kd.
 *   log_prior  log p(z | alpha_j):
 *                collapsed, full  lgamma(alpha) - lgamma(alpha + N) + sum_{k: n_k > 0} [lgamma(alpha/K + n_k) - lgamma(alpha/K)]
 *                                 -- the Dirichlet-multinomial MODEL, as the predictive and leave-one-out sections use it,
 *                                 not the finite sampler's quirk that an emptied label stays empty for ever;
 *                dp               K+ log(alpha) + sum_{n_k > 0} lgamma(n_k) + lgamma(alpha) - lgamma(alpha + N), K+ the labels in use;
 *                                 the probability of the PARTITION (over the 877 partitions of 7 rows it sums to 1): every
 *                                 numbering of its blocks within the maxK labels has this same value;
 *                stick-breaking   sum_{k < K-1} [lbeta(1 + n_k, alpha + n_{>k}) - lbeta(1, alpha)], n_{>k} the rows of the labels
 *                                 above k: the sticks integrated out.  It DEPENDS ON THE ORDER OF THE LABELS;
 *                allocation       log p(K) + lgamma(K a) - lgamma(K a + N) + sum_{k < K, n_k > 0} [lgamma(a + n_k) - lgamma(a)],
 *                                 K the open label count on the device, a the chain's per-component parameter.
 *   log_hyper  a log(b) - lgamma(a) + (a - 1) log(alpha) - b alpha when the chain samples alpha (created with alpha = 0), else 0;
 *              with a feature mask plus sum_d [gamma_d log rho + (1 - gamma_d) log(1 - rho)] = P_in log rho + (P - P_in) log(1 - rho),
 *              rho as last given to bmm_chain_set_feature_select (1/2 for a mask that was only ever set by hand).
 *   log_joint  (log_lik + log_prior) + log_hyper.
 * A row of output is these four doubles, in this order.
 * THE ORDER OF THE SUMS is a pure function of (K, P, mask); bmm_spec.h carries it once for host and device (the pieces
 * lj_cell, lj_prior_term, lj_finish; log_joint_spec is the whole statement for the host).  One workgroup per label: lane t
 * of 256 adds the cells of the included features t, t + 256, ... in ascending order from 0, and the 256 partial sums are
 * folded by a binary tree in LDS (partial t takes partial t + o, o = 128 .. 1); lgamma(beta + gamma + n_k) is computed once
 * per label and subtracted per cell; with a mask one more workgroup sums the pooled terms of the excluded features the
 * same way.  One lane then adds, from 0 and ascending in k, the totals of the labels that hold a row and last the pooled
 * term; the labels' prior terms the same way, and the model's head to that sum: (lgamma(alpha) - lgamma(alpha + N)) + sum;
 * (K+ log(alpha) + sum) + (lgamma(alpha) - lgamma(alpha + N)); (log p(K) + (lgamma(K a) - lgamma(K a + N))) + sum.
 * log_hyper is ((a log(b) - lgamma(a)) + (a - 1) log(alpha)) - b alpha, then plus the mask's term.  Nothing is atomic
 * in global memory: one state gives the same bits twice.  The statistics are read as they stand, pending deltas added
 * and nothing cleared, so a finite chain is scored before its first sweep too; no X is read, so both layouts, the
 * generic path, any P and up to 1024 labels are served.
 * KEEP-BEST: a cell on the device holds {best_total, best_sweep, improved}.  The lane that writes a folded row sets
 * improved = total > best_total -- strict, so the earliest sweep wins a tie and a NaN never wins -- and a second launch
 * copies the N labels of that sweep into the chain's best-state row only when improved is set.  Stream-ordered: a folded
 * sweep adds no synchronisation and no host-device copy, an armed chain that is not folding enqueues what an unarmed
 * one does.  The best state is the maximum a posteriori allocation among the folded states, the standard ECR pivot.
 * Refused: a sharded chain with BMM_E_UNSUPPORTED; a DP, stick-breaking or full chain before its first sweep (rows
 * without a label) with BMM_E_STATE, and the chain stays usable. */
/* arm (allocates N int32 and a few doubles per label; arming an armed chain empties the best state) or disarm (the
 * best state stays readable) */
int bmm_chain_set_logpost(bmm_chain* c, int on);
/* the row of the current state, once: no sweep, the best state untouched; needs no arming.  Waits. */
int bmm_chain_logpost_state(bmm_chain* c, double out[4]);
/* n more sweeps of an armed chain, each folded; trace n x 4 column-major (then the call waits) or NULL (then it returns
 * without waiting, as bmm_chain_sweeps) */
int bmm_chain_sweeps_logpost(bmm_chain* c, int n, double* trace);
/* the best folded state: its labels (N int32, 1-based, or NULL), its log_joint and the sweep it followed.  Waits. */
int bmm_chain_get_best(bmm_chain* c, int32_t* z1, double* total, int* sweep);
int bmm_chain_logpost_reset(bmm_chain* c);
/* For a run: armed per calling thread for the NEXT single-chain *_run* call of that thread, bmm_alloc_run included, and
 * disarmed when that call returns, whatever it returns, as bmm_set_loo_summary; NULL disarms.  The struct is copied;
 * its buffers must stay valid through that call; any field may be NULL.  Only kept sweeps (j >= burnin) are folded;
 * without burn-in the first kept row is the starting state, not a sweep: row 0 of rows is NaN and cannot be best.  It
 * combines with every other option; under a relabelling the values are those of the state as sampled and z_best is a
 * row of z_original.  bmm_multi_run does not take it and disarms it. */
typedef struct bmm_logpost_out {
    double* rows;        /* S x 4 doubles column-major like logdens: log_lik, log_prior, log_hyper, log_joint */
    int32_t* z_best;     /* N int32, 1-based: the labels of the best kept state, as sampled */
    double* best_total;  /* its log_joint (NaN when no state was folded) */
    int* best_row;       /* its row of the trace, 0-based: the first maximum of log_joint (-1 when no state was folded) */
} bmm_logpost_out;
int bmm_set_logpost(const bmm_logpost_out* out);
/* The rows of any stack of label rows over the same data (traces of several chains can be stacked by the caller), on a
 * transient chain: X is packed once, then per state the labels are uploaded, the statistics recounted and the state
 * scored by the launches above, so a run's own z and alpha give the run's rows bit for bit.  z: S x N int32 column-major,
 * 1-based; alpha: S values (> 0; the allocation sampler: a); sample_alpha: whether alpha's Gamma(a, b) prior enters
 * log_hyper; log_prior_k (K = maxK values) and k_open (S values) go together and select the allocation model, NULL
 * otherwise; mask: P bytes in {0, 1} with rho, or NULL; out: S x 4 column-major.  BMM_E_ARG, before a device is touched,
 * for a label outside 1 .. K (1 .. k_open[s]), naming the first bad cell. */
int bmm_device_log_joint(int device, const int32_t* X, int64_t N, int P, int sampler, int K, double beta, double gamma,
                         int sample_alpha, double a, double b, const double* log_prior_k, const int32_t* z, int S,
                         const double* alpha, const int32_t* k_open, const uint8_t* mask, double rho, double* out);

/* ---- parallel tempering: a replica ladder on the device ----------------------------------------
 * Metropolis-coupled MCMC for the two counting samplers (collapsed, dp).  A ladder has R <= 8 rungs with inverse
 * temperatures 1 = b_0 > b_1 > ... > b_{R-1} > 0; rung r holds a whole chain state (z, the counts, alpha) and targets
 *     pi_r(z, alpha)  proportional to  p(alpha) p(z | alpha) p(x | z)^{b_r}.
 * Only the marginal likelihood is tempered.  THE ONE-ROW CONDITIONAL of a tempered chain is the usual one with every
 * per-feature log-predictive term multiplied once by b after its denominator is subtracted, t = b * (log(.) - log(beta +
 * gamma + n)), in the table of the full statistics and in the one with the scored row removed alike; the category's
 * constant, log(n_k + alpha/K) - log(N - 1 + alpha) (collapsed) or log n_k - log(N - 1 + alpha) (dp), is untouched, and
 * the DP's new-cluster option is (log alpha - log(N - 1 + alpha)) + b * (P * (log beta - log(beta + gamma))).  With b = 1
 * every table entry has the bits of an unarmed chain's (x * 1.0 is x).  A tempered chain runs the kernel forms of a
 * chain with a feature mask: none that builds its own tables, no packed form; its draws are the same function of the
 * tables as every chain's.
 * THE EXCHANGE.  The priors are untempered, so they cancel: for neighbouring rungs r and r + 1, with L = log_lik of each
 * rung's current state (column 0 of its log joint row, the section above: the same order of sums, the same bits),
 *     d = (b_r - b_{r+1}) * (L_{r+1} - L_r),
 * the exchange is accepted iff d >= 0 or u < expw(d) (the draw's weight exponential, bmm_spec.h); a NaN d rejects.
 * u is the 52-bit uniform of the first two words of Philox4x32-10 at counter (r, 0, t, kStreamTemper = 14) under the
 * LADDER's seed, t the exchange point, counted from 0 over the life of the ladder.  Point t proposes the pairs with
 * r = t (mod 2); they are disjoint, so all are decided (one wave, one lane per pair, plain stores) and carried out
 * (one grid slice per pair, stream-ordered behind the decision) at once.
 * STATES MOVE, TEMPERATURES STAY: an accepted exchange swaps, in place on the device, the two chains' current label
 * rows, Nk, S, every replica of the pending count deltas as they stand (no fold) and alpha.  Each chain keeps its rung,
 * its seed, its streams and its kernels; rung 0 is always chains[0], an ordinary chain at b = 1 with every option and
 * recorder it has otherwise.  walker[r] names the state at rung r: it starts as r and is swapped with the state.
 * Refused with BMM_E_UNSUPPORTED, before anything is touched: stick-breaking, full and allocation chains, a chain with
 * a feature mask, split-merge moves on any rung, a sharded chain, rungs on different devices.  Armed chains refuse
 * those options in turn. */
/* on: the chain's table builds run the tempered flavour at inv_temp (0 < inv_temp <= 1; on with 1.0 runs that kernel
 * and gives an unarmed chain's bits); off: the chain is as it was.  Between sweeps, any time. */
int bmm_chain_set_temper(bmm_chain* c, int on, double inv_temp);
int bmm_chain_get_temper(const bmm_chain* c, int* on, double* inv_temp);
typedef struct bmm_ladder bmm_ladder;
typedef struct bmm_exchange_step {
    double d, u;        /* NaN for a pair that was not proposed at this point */
    int32_t proposed;   /* 1 for the pairs with r = t (mod 2) */
    int32_t accepted;
    int32_t point;      /* t */
    int32_t pad;
} bmm_exchange_step;
/* chains[0] unarmed or at 1.0, the others armed with strictly decreasing powers; one device, one sampler, equal N, P, K,
 * beta, gamma, a, b, batch and sweep index; the data shared (bmm_chain_share_data; the int32 layout: one device matrix);
 * nothing armed that the list above refuses.  BMM_E_ARG, or BMM_E_STATE where a chain's state is at fault, naming the
 * rung.  The chains stay the caller's and must outlive the ladder. */
int bmm_ladder_create(bmm_ladder** out, bmm_chain* const* chains, int R, uint64_t seed);
void bmm_ladder_destroy(bmm_ladder* l);
/* n sweeps of every rung, each on its own stream, an exchange point after every swap_every-th (>= 1) of them: every
 * rung scores its state on its stream, chains[0]'s stream waits for them, decides and exchanges, the others wait for
 * that.  One host thread; it never blocks, and the call returns without waiting.  A chains[0] armed for the log joint
 * trace folds its rows after the exchange. */
int bmm_ladder_sweeps(bmm_ladder* l, int n, int swap_every);
/* one exchange point now; out: R - 1 records (or NULL).  Waits.  BMM_E_STATE for a DP ladder before its first sweep. */
int bmm_ladder_exchange_step(bmm_ladder* l, bmm_exchange_step* out);
/* proposed, accepted: R - 1 each; walker: R; any may be NULL.  Waits. */
int bmm_ladder_stats(bmm_ladder* l, int64_t* proposed, int64_t* accepted, int32_t* walker);
/* For a run: armed per calling thread for the NEXT bmm_collapsed_run / bmm_dp_run of that thread and disarmed when that
 * call returns, as bmm_set_logpost; NULL disarms.  The run creates R - 1 helper chains with seed + r (mod 2^64) over the
 * run's planes, gives them the run's initialK (collapsed), and drives the ladder under the run's seed; everything the
 * call returns comes from chains[0], whose trace rows are the states after the exchange.  R = 1 is the run without it,
 * byte for byte.  Refused with BMM_E_UNSUPPORTED together with a relabelling run, a probability hand-off, split-merge
 * moves, feature selection, the allocation sampler or bmm_multi_run (which disarms it). */
typedef struct bmm_temper_out {
    int R;
    const double* inv_temp;  /* R values, inv_temp[0] = 1 */
    int swap_every;          /* >= 1 */
    int64_t* proposed;       /* R - 1, or NULL */
    int64_t* accepted;       /* R - 1, or NULL */
    int32_t* walker_cold;    /* S, or NULL: the walker at rung 0 after each kept sweep (row 0 without burn-in: 0) */
    double* loglik;          /* S x R column-major, or NULL: every rung's log_lik after the exchange point of a kept sweep, NaN elsewhere */
} bmm_temper_out;
int bmm_set_temper(const bmm_temper_out* out);

/* ---- pairwise local-dependence check ---------------------------------------------------------
 * The model check of a Bernoulli mixture: within a cluster the features are independent.  Condition on the labels and
 * on each label's margins (n_k rows, s_kd ones of feature d, s_ke ones of feature e): under the model -- for the
 * collapsed samplers too, theta integrates out of a statement conditional on sufficient statistics -- the co-occurrence
 *   c_k(d, e) = #{i : z_i = k, x_id = 1, x_ie = 1}    is Hypergeometric(n_k, s_kd, s_ke), so
 *   E_k = s_kd s_ke / n_k,    V_k = s_kd s_ke (n_k - s_kd)(n_k - s_ke) / (n_k^2 (n_k - 1)).
 * Two realised discrepancies per pair and state, each with a reference distribution known under the model:
 *   Z  = sum_k (c_k - E_k) / sqrt(sum_k V_k)            approximately N(0, 1), signed (Cochran-Mantel-Haenszel)
 *   X2 = sum_{k: V_k > 0} (c_k - E_k)^2 / V_k           approximately chi-square with df = #{k : V_k > 0}
 * Z is blind to dependence whose sign differs between clusters; X2 is not.
 * CHOSEN FEATURES AND PAIRS: feat[0 .. M), 2 <= M <= 128, distinct, any order, any P.  The pairs (i < j) of positions
 * in feat are numbered as numpy.triu_indices(M, 1) numbers them; npairs = M (M - 1) / 2.
 * COUNTS: c[k][pair], uint32, over the labels k = 0 .. Kc - 1 (Kc = K, or the DP's maxK).  The margins are counted in
 * the same pass over the same rows, so everything here is a function of (X, z) alone.
 * FIXED ARITHMETIC per pair (bmm_spec.h pc_label, pc_z; no fused operation): the labels in ascending order, labels with
 * n_k < 2 skipped; in int64 num = c n - s_d s_e, pd = s_d (n - s_d), pe = s_e (n - s_e), nn = n n, each converted to
 * binary64 once; a_k = num / n; v_k = (pd pe) / (nn (n - 1)); A += a_k; V += v_k; if v_k > 0: X2 += (a_k a_k) / v_k and
 * df += 1.  Z = A / sqrt(V) when V > 0, else the pair has no Z for that state (NaN in a row, not folded).
 * THE FOLD over the evaluated states, one add per pair per state, in sweep order: doubles sum_z, sum_z2 (of Z Z),
 * sum_x2; int64 sum_df; int32 n_z (the states with V > 0); n_folded; n11[pair] = sum_k c_k of the last evaluated state.
 * No floating-point atomic is used anywhere (integer atomics build the counts): one state gives the same bits twice.
 * Everything is enqueued on the chain's stream behind the sweep's last kernel: no host wait, no copy; an armed chain
 * that is not folding enqueues exactly what an unarmed one does, and the check reads state only, so it changes no chain.
 * Arming costs M N / 8 bytes (the chosen features as column slices of 64 rows per word, X being constant over a
 * chain's life) plus Kc (npairs + M + 1) uint32 and 6 npairs values of fold; disarming frees them.
 * REFUSED: BMM_E_UNSUPPORTED for a chain with a feature mask (the pooled model's reference distribution is another
 * one), a sharded chain, a chain on the int32 layout (no bit planes); BMM_E_STATE for a state with unseated rows (a DP,
 * stick-breaking or full chain before its first sweep); BMM_E_ARG for M outside 2 .. 128, a feature outside 0 .. P - 1
 * or repeated, stride < 1, counts above BMM_PAIR_CHECK_MAX_COUNT_BYTES, or more than 8 * 65535 labels.  While the check is
 * armed bmm_chain_set_data_host / _device and bmm_chain_planes_filled answer BMM_E_STATE: the slices were cut from the
 * data the chain held at arming; disarm, set the data, arm again. */
#define BMM_PAIR_CHECK_MAX_M 128
#define BMM_PAIR_CHECK_MAX_COUNT_BYTES (16u << 20) /* Kc * npairs * 4 */
typedef struct bmm_pair_check_out {
    const int32_t* feat; /* bmm_set_pair_check: the M chosen features, 0-based (bmm_chain_get_pair_check ignores it) */
    int M;
    int stride;          /* bmm_set_pair_check: every stride-th kept sweep is evaluated, from the first kept row on */
    double* z_rows;      /* a run: S x npairs column-major, or NULL; NaN where not evaluated or V = 0 */
    double* x2_rows;     /* a run: S x npairs column-major, or NULL; NaN where not evaluated */
    double* sum_z;       /* npairs each, any may be NULL */
    double* sum_z2;
    double* sum_x2;
    int64_t* sum_df;
    int32_t* n_z;
    uint32_t* n11;
    int* n_folded;
} bmm_pair_check_out;
/* arm (feat, M, stride as above; arming an armed chain empties the fold and takes the new features) or, with feat NULL
 * or M = 0, disarm and free */
int bmm_chain_set_pair_check(bmm_chain* c, const int32_t* feat, int M, int stride);
/* the current state, once: no sweep, the fold untouched; npairs values each, any may be NULL.  Waits. */
int bmm_chain_pair_check_state(bmm_chain* c, double* z_out, double* x2_out, int32_t* df_out);
/* n more sweeps of an armed chain, sweeps 0, stride, 2 stride, ... of them evaluated and folded; trace n x (2 npairs)
 * column-major, Z then X2, NaN where not evaluated (then the call waits) or NULL (then it does not wait) */
int bmm_chain_sweeps_pair_check(bmm_chain* c, int n, double* trace);
/* reads the fold (the sums, n_folded); z_rows, x2_rows, feat, M, stride are ignored.  Waits. */
int bmm_chain_get_pair_check(bmm_chain* c, bmm_pair_check_out* out);
int bmm_chain_pair_check_reset(bmm_chain* c);
/* the Kc x npairs uint32 of the current state, counts[k * npairs + pair]; margins (Kc x M, or NULL) and rows (Kc, or
 * NULL) are the s_kd and n_k counted in the same pass.  Waits. */
int bmm_chain_pair_counts(bmm_chain* c, uint32_t* counts, uint32_t* margins, uint32_t* rows);
/* For a run: armed per calling thread for the NEXT single-chain *_run* call of that thread and disarmed when that call
 * returns, as bmm_set_logpost; NULL disarms.  The struct and feat are copied.  Only kept sweeps are folded, every
 * stride-th of them counted from kept row 0 (without burn-in row 0 is the starting state and stays NaN).  Under
 * bmm_set_temper the check sees rung 0 after the exchange point.  bmm_multi_run does not take it and disarms it. */
int bmm_set_pair_check(const bmm_pair_check_out* out);
/* Any stack of label rows over the same data on a transient chain, as bmm_device_log_joint: z S x N int32 column-major,
 * 1-based in 1 .. Kc; counts: S x Kc x npairs uint32 (state s at counts + s Kc npairs) or NULL; rows: S x (2 npairs)
 * column-major, Z then X2, or NULL; out: the fold over the S states in order (its z_rows, x2_rows, feat, M, stride
 * are ignored), or NULL.  A run's own z gives the run's rows bit for bit. */
int bmm_device_pair_check(int device, const int32_t* X, int64_t N, int P, int Kc, const int32_t* z, int S,
                          const int32_t* feat, int M, uint32_t* counts, double* rows, const bmm_pair_check_out* out);
/* pure bookkeeping: the bytes the check needs on the device and the grid of k_pc_counts */
typedef struct bmm_pair_check_plan_out {
    int64_t bytes_slices, bytes_counts, bytes_fold;
    int64_t chunks;            /* ceil(N / 64) */
    int64_t chunks_per_slice;  /* a multiple of chunks_per_round */
    int chunks_per_round;      /* chunks a workgroup stages at a time, one per wave */
    int tiles, row_slices, label_blocks;  /* the grid: x, y, z */
    int ka;                    /* labels per workgroup: accumulators per pair */
    int pairs_per_lane;        /* pairs of the tile a lane owns */
    int threads;
} bmm_pair_check_plan_out;
int bmm_pair_check_plan(int64_t N, int Kc, int M, bmm_pair_check_plan_out* out);

/* ---- missing data: NA cells imputed on the device ------------------------------------------------
 * Cells missing at random, handled by data augmentation.  The chain lives on (z, x_mis, ...): the sampler's own sweep
 * runs on the completed matrix, unchanged, and behind every sweep end the missing cells are redrawn jointly and exactly
 * given everything else.  Both steps leave p(z, x_mis, ... | x_obs) invariant, so the labels are draws from the posterior
 * of the model with the missing cells integrated out.
 *   Counting chains (collapsed, DP): for every label k and feature j with a missing cell among k's rows, with n the
 * label's rows that have the feature observed and s of them holding a 1, phi_kj ~ Beta(beta + s, gamma + n - s) (n = 0:
 * the prior; bmm_spec.h na_phi), thrown away after the step.  Explicit chains (stick-breaking, full): phi is the theta
 * the sweep has just drawn.  Then every missing cell (i, j) becomes  u_ij < phi_{z_i, j},  u_ij = na_uniform(seed,
 * i * P + j, sweep) (bmm_spec.h): keyed by the cell and the sweep alone.  phi first and the cells independently given it
 * is the composition form of the Polya-urn joint of the cells of one (k, j); drawing them in parallel from the plug-in
 * rate (beta + s) / (beta + gamma + n) would not be exact.
 *   The step runs behind everything sweep t does today, so the theta row recorded for sweep t belongs to (z_t, X_{t-1}):
 * the labels of sweep t with the cells as they stood before its step.  Whenever the chain is idle, bmm_chain_get_counts
 * equals a recount of the completed matrix under the current labels.  The log joint (bmm_set_logpost) of an armed chain
 * is the joint of the completed state.
 *
 * bmm_chain_set_missing: after the data is set, before or after the rows have labels.  rows / cols: the n_cells missing
 * cells, 0-based, strictly ascending in (row, column); their values in the matrix that was handed over are ignored.
 * Every cell is filled with  na_uniform(seed, cell, 0) < beta / (beta + gamma)  and, where the rows have labels, the
 * counts follow.  n_cells = 0 withdraws the declaration (the planes keep the cells' last values).  From then on every
 * sweep of bmm_chain_sweeps* is followed by the step, and every step is folded into the summary.
 *   BMM_E_ARG: a cell out of range or out of order.  BMM_E_UNSUPPORTED: the int32 layout; a sharded chain; a chain
 * whose planes other chains read (bmm_chain_share_data, a ladder); together, in either order, with the leave-one-out
 * summary and parallel tempering (wrong on a completed or shared matrix), the pair check (its slices are cut once),
 * feature selection, split-merge moves, the allocation sampler, bmm_chain_init_labels and bmm_chain_sweep_probs (not in
 * this change).  BMM_E_STATE: no data yet, cells already declared, new data under declared cells.  All of these are
 * answered before a device is touched. */
int bmm_chain_set_missing(bmm_chain* c, const int64_t* rows, const int32_t* cols, int64_t n_cells);
/* one imputation step now, under the index of the last sweep (the keys of that sweep's own step: meant for a chain
 * inspected by hand, not for sampling).  Folded like any other step. */
int bmm_chain_impute_step(bmm_chain* c);
/* bits[n_cells]: the cells' current values, in the order they were declared */
int bmm_chain_get_missing_state(bmm_chain* c, uint8_t* bits);
/* over the folded steps, per cell (any may be NULL): mean_rb, the mean of phi_{z_i, j} (Rao-Blackwellised: the posterior
 * probability that the cell is a 1), mean_draw, the share of ones drawn; NaN before the first fold.  Each cell's sums
 * have one owner and the steps add in order: one seed gives the same bits twice. */
int bmm_chain_get_missing_summary(bmm_chain* c, double* mean_rb, double* mean_draw, int64_t* n_folded);
int bmm_chain_missing_reset(bmm_chain* c);
/* For a run: armed per calling thread for the NEXT bmm_collapsed_run / bmm_dp_run / bmm_sb_run / bmm_full_run (and their
 * _probs form without hooks, and _predict) of that thread and disarmed when that call returns; out = NULL disarms.
 * rows, cols and the buffers of out must live until the run returns; the X of the run holds any 0 / 1 value in the
 * missing cells.  Kept sweeps are folded; last[n_cells] receives the cells after the last sweep.  BMM_E_ARG and
 * BMM_E_UNSUPPORTED as above, also for bmm_set_init and a *_run_relabel / hooked *_run_probs hand-off; bmm_multi_run
 * and bmm_alloc_run answer an armed declaration with BMM_E_UNSUPPORTED.  n_cells = 0 is the run without it, byte for
 * byte.  Allowed, and unchanged because they read labels or folded counts only: the partition summary, ECR, the
 * predictive of new rows (complete, or incomplete: the section "incomplete new rows") and the log joint trace. */
typedef struct bmm_missing_out {
    double* mean_rb;    /* [n_cells] */
    double* mean_draw;  /* [n_cells] */
    uint8_t* last;      /* [n_cells] */
    int64_t* n_folded;
} bmm_missing_out;
int bmm_set_missing(const int64_t* rows, const int32_t* cols, int64_t n_cells, const bmm_missing_out* out);

/* ---- constraints: known labels and allowed-label sets ---------------------------------------------
 * Partial knowledge of the rows' classes.  A constrained row i has a non-empty set A_i of labels it may take, given as a
 * 64-bit mask (bit k: label k, 0-based); a known label is the singleton set.  Rows that are not listed are free.
 *   The move.  The sweep draws a listed row as it draws every row, a proposal k' from its full conditional.  If k' is in
 * A_i the draw stands; if not, the row keeps the label it had.  The target is the conditional restricted to A_i, the
 * proposal is the unrestricted conditional, so the Metropolis-Hastings ratio is 1 inside A_i and 0 outside: the move is
 * exact and carries no weight; under a batch it is exact to the degree the unconstrained sweep is.  A row with a
 * singleton set never moves.  The revert (k_constrain, behind every resample launch whose range holds a listed row)
 * also undoes the row's move in the pending count deltas, so no table and no statistic ever sees the row moved.
 *   Starting labels.  A listed row of the finite collapsed chain whose starting label z0 (0-based) lies outside A_i
 * starts at its (z0 mod |A_i|)-th allowed label, counted from the lowest, projected on the device before the labels
 * are counted.  The same rule puts the rows of a chain that is armed between sweeps inside their sets, and the counts
 * follow.  A row of a DP, stick-breaking or full chain that is seated by the chain's first sweep and drawn outside A_i
 * there takes its lowest allowed label.
 *   Labels.  Masks name the chain's own labels.  On the finite and the full sampler label k is a class.  On the DP and
 * the stick-breaking sampler (K = maxK) a label is whatever cluster holds it: singleton masks, which pin a cluster to a
 * label by the rows held there, are the intended use; a DP label that no held row occupies is an ordinary free label,
 * and free rows may open new clusters as they always do.
 *
 * bmm_chain_set_constraints: rows[n] 0-based and strictly ascending, masks[n] non-zero with no bit at or above K.  Before
 * the chain has started or between sweeps.  n = 0 withdraws the constraints: the rows are free from the next sweep on.
 * From then on every sweep of bmm_chain_sweeps* reverts; a sweep of a chain without constraints enqueues exactly what it
 * always did.  The draws of held rows are still computed (the resample kernels are untouched).
 *   BMM_E_ARG: a row out of range or out of order, an empty set, a label at or above K.  BMM_E_UNSUPPORTED: a sharded
 * chain; together, in either order, with split-merge moves, parallel tempering (a ladder), the leave-one-out summary,
 * the allocation sampler, bmm_chain_init_labels, bmm_chain_set_labels and bmm_chain_sweep_probs (the emitted rows would
 * be those of reverted draws).  BMM_E_STATE: constraints already set, inside a run.  All of these are answered before a
 * device is touched.  Unchanged beside it: the predictive of new rows, the partition summary, ECR, the log joint (of
 * the whole state, held rows included), the pair check, feature selection and missing cells. */
int bmm_chain_set_constraints(bmm_chain* c, int64_t n, const int64_t* rows, const uint64_t* masks);
/* since the constraints were last set: proposed, the listed rows drawn (listed rows x sweeps); reverted, those drawn
 * outside their set.  Integer counts: one seed gives the same values twice.  Readable after a withdrawal. */
int bmm_chain_constraint_stats(bmm_chain* c, int64_t* proposed, int64_t* reverted);
/* For a run: armed per calling thread for the NEXT bmm_collapsed_run / bmm_dp_run / bmm_sb_run / bmm_full_run (and their
 * _probs form without hooks, and _predict) of that thread and disarmed when that call returns; n = 0 disarms and is the
 * run without it, byte for byte.  rows and masks must live until the run returns.  BMM_E_ARG and BMM_E_UNSUPPORTED as
 * above, also for bmm_set_init and a *_run_relabel / hooked *_run_probs hand-off; bmm_multi_run and bmm_alloc_run
 * answer armed constraints with BMM_E_UNSUPPORTED.  bmm_last_constraint_stats: the counters of the thread's last run. */
int bmm_set_constraints(int64_t n, const int64_t* rows, const uint64_t* masks);
int bmm_last_constraint_stats(int64_t* proposed, int64_t* reverted);

/* ---- posterior summary: online pivot relabelling, memberships folded on the device ----------
 * What a latent-class user takes out of a chain -- each row's class and how sure it is, each class's size and item
 * profile, under one labelling -- folded behind the kept sweeps on the live label row, so that the S x N label trace
 * need not exist.  Labels are 0-based in these definitions (1-based at the interfaces); z_s is the state after kept
 * sweep s, theta_s and alpha_s its rows of the theta and alpha traces, c the pivot.
 *   folded sweeps  kept sweep j is folded when it is a sweep (trace row 0 of a run without burn-in is the starting
 *                state and never folded) and (j - first kept sweep index) is a multiple of `stride`: the rule of the
 *                pair check's stride.  n_folded counts them.
 *   permutation  BMM_SUMMARY_PIVOT_FIRST / _GIVEN: perm_s and agree_s of z_s against c exactly as "ECR" above defines
 *                them with a pivot given (table, min-cost assignment, its tie rule, agree): one pass per folded sweep,
 *                enqueued behind it, no host wait.  BMM_SUMMARY_PIVOT_NONE: the identity and agree_s = 0, no launch.
 *                perm_s[l] keeps its meaning: draw label l leaves as pivot label perm_s[l].
 *   pivot        _FIRST: the first kept state that is assigned -- trace row 0, or row 1 for the DP, stick-breaking and
 *                full samplers in a run without burn-in -- copied device to device behind that sweep, whether or not the
 *                stride folds it.  _GIVEN: N labels in 1 .. K.  _NONE: none; the state is folded as sampled (the choice
 *                with constraints, where a few held rows per class pin the labelling).
 *   counts       cnt[k][i] = #{folded s : perm_s[z_s[i]] = k}, uint32; an unassigned label is skipped.
 *   z_hat, n_max z_hat[i] = the k with the largest cnt[k][i], the lowest on a tie (1-based on the way out); n_max[i]
 *                that count.  A row never assigned has z_hat 1 and n_max 0.
 *   size_sum     size_sum[k] = sum_i cnt[k][i], int64: the cluster sizes under perm_s added over the folded sweeps.
 *   profiles     theta_sum[perm_s[l], d] += theta_s[l, d]; theta_sq[perm_s[l], d] += theta_s[l, d] * theta_s[l, d],
 *                the product rounded before the add, no contraction; one add per folded sweep in sweep order, so two
 *                runs give the same bits.  A NaN cell (the finite sampler's empty label) is left out; theta_n[perm_s[l]]
 *                counts the folded sweeps whose theta_s[l, 0] is not NaN.  alpha_sum[0] += alpha_s and alpha_sum[1] +=
 *                alpha_s * alpha_s likewise.
 *   per sweep    agree[s] (int64) and permutations (S x K int32 column-major, 0-based) for every kept sweep; -1 and the
 *                identity where the sweep was not folded.
 * Nothing per row is floating point; probabilities, entropies, means and deviations are the caller's to derive from
 * the integers and the sums.  The summary reads state only: an armed chain's labels, theta and alpha are those of an
 * unarmed one, byte for byte. */
#define BMM_SUMMARY_PIVOT_NONE 0
#define BMM_SUMMARY_PIVOT_FIRST 1
#define BMM_SUMMARY_PIVOT_GIVEN 2
typedef struct bmm_summary_opts {
    int pivot_kind;       /* BMM_SUMMARY_PIVOT_NONE, _FIRST or _GIVEN */
    const int32_t* pivot; /* _GIVEN: N labels, 1-based, in 1 .. K; else ignored */
    int stride;           /* >= 1 */
    int keep_trace;       /* bmm_set_summary: 0 drops the label trace of the run (below); else 1 */
} bmm_summary_opts;
typedef struct bmm_summary_out { /* any pointer may be NULL */
    int32_t* pivot;        /* N int32, 1-based: the pivot used (0 for _NONE, or when no kept state was assigned) */
    int32_t* z_hat;        /* N int32, 1-based */
    uint32_t* n_max;       /* N */
    int* n_folded;
    int64_t* size_sum;     /* K */
    double* theta_sum;     /* K x P column-major */
    double* theta_sq;      /* K x P column-major */
    int32_t* theta_n;      /* K */
    double* alpha_sum;     /* 2: the sum and the sum of squares */
    int64_t* agree;        /* a run: S */
    int32_t* permutations; /* a run: S x K int32 column-major, 0-based */
    uint32_t* counts;      /* N x K uint32 column-major (cnt[k][i] at [i + k N]): 4 N K bytes, so only on request */
} bmm_summary_out;
/* For a run: armed per calling thread for the NEXT single-chain bmm_collapsed_run / bmm_dp_run / bmm_sb_run /
 * bmm_full_run (and their _probs form without hooks, and _predict) of that thread and disarmed when that call returns,
 * whatever it returns; opts NULL disarms.  Both structs are copied; their buffers must stay valid through that call.
 * keep_trace = 0: the run carves no label trace on the device, writes no z_out (z_out may then be NULL, and only then)
 * and skips the trace's way out; the theta, alpha and pi traces stay.  Refused before a device is touched: BMM_E_ARG for
 * stride < 1, N >= 2^32, K > BMM_ECR_MAX_K unless the pivot is _NONE, a pivot label outside 1 .. K, together with a
 * relabelling of the same run (bmm_set_ecr_relabel, a *_run_relabel call, *_run_probs hooks), and for keep_trace = 0
 * together with anything that reads the trace (the partition summary, ECR, Stephens' relabelling);
 * BMM_E_UNSUPPORTED for bmm_alloc_run and together with parallel tempering; bmm_multi_run disarms it like any other
 * option.  Composes with what only reads state or acts between sweeps (constraints, a device start, the log joint
 * trace, the pair check, the predictive summaries, split-merge moves, feature selection, missing cells). */
int bmm_set_summary(const bmm_summary_opts* opts, const bmm_summary_out* out);
/* The bytes a run's device buffers take -- the traces, and with keep_trace the label trace and the two staging blocks
 * of its way out -- plus, with summary != 0, the summary's own block.  A pure function, read by the run itself; no
 * device is touched.  With keep_trace = 0 no term grows with S N.  -1 for an argument out of range. */
int64_t bmm_run_bytes(int sampler, int64_t N, int P, int K, int S, int keep_trace, int summary);
/* The launch shapes of the summary's kernels, from the function the launches read (no device is touched).  out:
 *   [0] threads per workgroup                     [1] workgroups of k_sum_fold (its grid cap: [2])
 *   [2] the cap                                   [3] words per plane of the counts (N rounded up to 64)
 *   [4] bytes of dynamic LDS of k_sum_fold        [5] workgroups of k_sum_profiles
 *   [6] workgroups of k_sum_finish                [7] its bytes of dynamic LDS
 *   [8] bytes of the counts                       [9] bytes of the summary's whole block
 *   [10] launches per folded sweep with a pivot (memsets included)   [11] ... and without one.
 * BMM_E_ARG unless N, P, K >= 1 and N < 2^32. */
int bmm_summary_plan(int64_t N, int P, int K, int64_t out[12]);
/* Resident chains.  bmm_chain_set_summary arms (opts->keep_trace is ignored) or, with opts NULL, disarms and frees;
 * BMM_E_UNSUPPORTED on a sharded chain, a chain of the allocation sampler and a tempered chain, BMM_E_STATE inside a
 * run, BMM_E_ARG as above.  Armed, bmm_chain_sweeps_summary(c, n) runs n sweeps and folds every stride-th of them from
 * its first on (agree n int64 and permutations n x K column-major, or NULL); plain bmm_chain_sweeps folds nothing.  The
 * _FIRST pivot is the state after the first sweep a bmm_chain_sweeps_summary call runs.  bmm_chain_summary_state folds
 * nothing: it relabels the present state against the pivot and returns its permutation (K) and agreement; BMM_E_STATE
 * before a pivot exists.  bmm_chain_get_summary finishes (z_hat, n_max, size_sum) and copies out; it waits, and may
 * be called again after more sweeps.  bmm_chain_summary_reset zeroes the folds and forgets a _FIRST pivot. */
int bmm_chain_set_summary(bmm_chain* c, const bmm_summary_opts* opts);
int bmm_chain_summary_state(bmm_chain* c, int32_t* perm_out, int64_t* agree_out);
int bmm_chain_sweeps_summary(bmm_chain* c, int n, int64_t* agree, int32_t* permutations);
int bmm_chain_get_summary(bmm_chain* c, bmm_summary_out* out);
int bmm_chain_summary_reset(bmm_chain* c);

/* ---- categorical features: polytomous items for the collapsed and the DP sampler ------------
 * A feature j has L_j levels, levels[j].  L_j = 1 is a binary feature in one column under the chain's Beta(beta, gamma)
 * prior, exactly the cell every chain has.  L_j >= 2 is a block of L_j neighbouring one-hot columns -- column l of the
 * block is 1 in the rows at level l -- under a symmetric Dirichlet(beta, ..., beta) prior on the level probabilities,
 * beta being the chain's beta.  The columns of the features, in order, are the chain's P columns.  For a cluster of n
 * rows with c_l at level l the predictive of level l is (beta + c_l) / (L beta + n), with the scored row removed
 * (beta + c_l - 1) / (L beta + n - 1); the DP's new cluster gives every level 1 / L.  (One-hot columns run through the
 * Bernoulli model are a different model: it scores a row's L - 1 zeros, divides by beta + gamma + n per column and gives
 * the new cluster (beta / (beta + gamma))^L per item.)  A block of 2 levels is Dirichlet(beta, beta): the Bernoulli
 * column with gamma = beta.  The counts of ones per cluster are the level counts, so Nk, S, theta = S / Nk (the level
 * proportions), the resample kernels and everything that reads labels and counts are unchanged; the sweep's table
 * build alone (k_count_tables<TAB_CAT>) reads which columns form a block.
 *
 * bmm_chain_set_categorical: before or after the data, before the chain has started or between sweeps.  F = 0 withdraws
 * the levels.  When levels and data first meet, and whenever either changes, the device checks that every row has
 * exactly one bit set in every block (k_cat_check): BMM_E_ARG otherwise, and bmm_last_error names the first bad row and
 * its feature; data that fail are not taken.  Levels of all 1 are the plain chain, byte for byte.
 *   BMM_E_ARG: a level below 1 (or above 255); the levels' columns do not add up to P.  BMM_E_UNSUPPORTED, in either
 * order of arming: the int32 layout; a sharded chain; the stick-breaking and the full sampler; the allocation sampler;
 * parallel tempering (a ladder); feature selection; split-merge moves; missing cells; newdata, the leave-one-out
 * summary, the log joint trace and the pair check (their scorers know the Bernoulli cell only); bmm_chain_init_labels.
 * BMM_E_STATE: inside a run.  Unchanged beside it: the partition summary with its search and credible ball, ECR,
 * constraints, the posterior summary, bmm_chain_sweep_probs, bmm_chain_get_counts / _get_params.  A categorical chain
 * runs every resample form but those that build their own tables, the packed one (k_resample_pk) included. */
int bmm_chain_set_categorical(bmm_chain* c, const int32_t* levels, int F);
/* the levels a chain carries: *F (0: none), and levels[*F] when levels is not NULL */
int bmm_chain_get_categorical(const bmm_chain* c, int32_t* levels, int* F);
/* For a run: armed per calling thread for the NEXT bmm_collapsed_run / bmm_dp_run (and their _probs form without hooks)
 * of that thread and disarmed when that call returns; F = 0 disarms.  The vector is copied.  BMM_E_ARG and
 * BMM_E_UNSUPPORTED as above, before a device is touched, also for bmm_set_init, a *_run_relabel / hooked *_run_probs
 * hand-off (relabel = TRUE), bmm_sb_run / bmm_full_run, bmm_alloc_run and bmm_multi_run. */
int bmm_set_categorical(const int32_t* levels, int F);
/* Pure bookkeeping, no device: the column map of a levels vector -- first_column[F] (or NULL), lev[P] (or NULL): 0 for a
 * Bernoulli column, else the L of the column's block, the bytes the table build reads -- and the kernel form a chain of
 * that shape gets on num_cus compute units (batch <= 0: the default batch).  P is the levels' sum. */
typedef struct bmm_categorical_plan_out {
    int32_t n_columns, n_blocks;
    int32_t generic;            /* the shape runs the generic kernels */
    int32_t threads, lanes;     /* of a resample workgroup; lanes per observation */
    int32_t packed;             /* k_resample_pk: k_count_tables<TAB_CAT> writes the packed image */
    int32_t builds_own_tables;  /* always 0: not offered to a categorical chain */
    int64_t batch;
} bmm_categorical_plan_out;
int bmm_categorical_plan(int sampler, int64_t N, int K, int64_t batch, int num_cus, const int32_t* levels, int F,
                         int32_t* first_column, uint8_t* lev, bmm_categorical_plan_out* out);

/* ---- ensemble of exact chains.  `chains` independent batch = 1 chains of the collapsed
 * (BMM_SAMPLER_COLLAPSED) or the DP sampler (BMM_SAMPLER_DP; K is maxK) over one data set, one wavefront per chain, every
 * chain advanced by one launch per sweep (k_ens_sweep; a sweep over more than 2048 / ceil(P / 8) rows, rounded down to a multiple of 64, is several launches).  Chain c
 * draws under seed + c and is, bit for bit, the chain bmm_collapsed_run / bmm_dp_run run at batch = 1 under that seed: the
 * arithmetic is bmm_spec.h's in the same order.  alpha = 0: sampled (a, b), as everywhere.
 *   z0         collapsed: one start per chain, N labels in 1..K each; dp: NULL (the rows are seated in sweep 1)
 *   z_out      per chain an S x N column-major label trace, S = nsamples - burnin; or NULL: no label trace at all
 *   nk_out     per chain S x K cluster sizes, row s at nk_out[c] + s * K
 *   theta_out  per chain K x P x S;  alpha_out per chain S;  z_last per chain the N labels after the last sweep
 * Row 0 of a run without burn-in is the start, as in the single-chain runs: z0 (dp: NA_integer_), theta NaN (dp: 0), the
 * first alpha, the sizes of the start.
 * Limits, refused with BMM_E_UNSUPPORTED before a device is touched: at most 64 categories (K, or maxK + 1), P <= 128,
 * N < 65536, the terms of one chain within the 160 KiB of LDS of a workgroup ((4 P Kc + 256) * 8 + 4 K P bytes), a sampler
 * other than the two, any armed run option (bmm_set_*: an ensemble runs plain chains), the int32 layout of the test
 * variant.  BMM_E_ARG: chains < 1, beta != gamma for the DP, a start label outside 1..K, a null buffer.
 * bmm_ensemble_plan is pure bookkeeping, no device: out = {group width of the scores (bmm_spec_group_width_for), LDS
 * bytes per chain, chains per workgroup, workgroups per launch, launches per sweep, device bytes of the chains' state,
 * device bytes per kept sweep without the label trace, device bytes per kept sweep of the label trace}; the same
 * refusals of a shape. */
int bmm_ensemble_plan(int sampler, int64_t N, int P, int K, int chains, int64_t out[8]);
int bmm_ensemble_run(int sampler, const int32_t* X, int64_t N, int P, int chains, const int32_t* const* z0, int nsamples, int K,
                     double alpha, double beta, double gamma, double a, double b, int burnin, uint64_t seed, int device,
                     int32_t* const* z_out, int32_t* const* nk_out, double* const* theta_out, double* const* alpha_out,
                     int32_t* const* z_last);

/* ---- leave-one-out and held-out predictive on every chain of an ensemble.  bmm_ensemble_run_ex
 * is bmm_ensemble_run with a last argument, the folds asked for; NULL: bmm_ensemble_run itself.  After every kept sweep
 * (every sweep from `burnin` on; row 0 of a run without burn-in is the start and is not folded) the state of each chain
 * is scored by its own wavefront (k_ens_score, one launch per fold asked for, all chains) and folded into accumulators
 * of the chain's own:
 *   newdata, M   M new rows x P, column-major, every cell 0 or 1 (BMM_E_ARG otherwise; incomplete new rows are not
 *                offered here): the posterior predictive of "posterior predictive density" above, per chain.
 *                M = 0: none
 *   loo          nonzero: the leave-one-out predictive of the fitted rows ("leave-one-out predictive"), per chain
 * The quantities, their arithmetic and its order are those of bmm_collapsed_run / bmm_dp_run at batch = 1 with the same
 * option, so chain c's outputs equal, bit for bit, those of the single run under seed + c.  alpha is the chain's value
 * after the sweep's update.  Outputs, a table of `chains` pointers each (a table that is not asked for may be NULL):
 *   pred_lppd     [M]                       pred_logdens  S x M column-major, when predictive_trace is nonzero
 *   loo_log_cpo, loo_ess, loo_lppd, loo_mean, loo_var   [N] each
 *   loo_ell       S x N column-major, when loo_trace is nonzero
 *   loo_lpml, loo_min_ess   [chains] doubles;  n_folded: one int, the states folded (the same for every chain and fold)
 * A trace row that was not folded is NaN; with no state folded every output is NaN and n_folded 0.  The mean
 * responsibilities are not offered: labels switch between chains.  An armed bmm_set_* option is refused by both entries.
 * bmm_ensemble_fold_plan is pure bookkeeping, no device: out = {LDS bytes per chain of the scorer (the sweep's slice),
 * chains per workgroup, device bytes of the accumulators and the finish kernels' outputs (loo: chains * (12 N + 8)
 * doubles; newdata: chains * 3 M doubles and ceil(P / 32) * M plane words), device bytes per kept sweep of the ell trace
 * (chains * N doubles) and of the logdens trace (chains * M doubles), launches added per kept sweep}; bmm_ensemble_plan's
 * refusals of a shape, and BMM_E_ARG for M < 0. */
typedef struct {
    const int32_t* newdata;
    int64_t M;
    int32_t loo, loo_trace, predictive_trace;
    double* const* pred_lppd;
    double* const* pred_logdens;
    double* const* loo_log_cpo;
    double* const* loo_ess;
    double* const* loo_lppd;
    double* const* loo_mean;
    double* const* loo_var;
    double* const* loo_ell;
    double* loo_lpml;
    double* loo_min_ess;
    int32_t* n_folded;
} bmm_ensemble_folds;
int bmm_ensemble_fold_plan(int sampler, int64_t N, int P, int K, int chains, int64_t M, int loo, int64_t out[6]);
int bmm_ensemble_run_ex(int sampler, const int32_t* X, int64_t N, int P, int chains, const int32_t* const* z0, int nsamples, int K,
                        double alpha, double beta, double gamma, double a, double b, int burnin, uint64_t seed, int device,
                        int32_t* const* z_out, int32_t* const* nk_out, double* const* theta_out, double* const* alpha_out,
                        int32_t* const* z_last, const bmm_ensemble_folds* folds);

/* ---- device self-checks used by the parity tests (op: 0 log, 1 exp, 2 div by in2, 3 sqrt,
 * 4 the draw's weight exponential expw, 5 lgamma_; elementwise over n doubles, evaluated on the GPU with the
 * spec arithmetic) */
int bmm_device_math(int device, int op, const double* in, const double* in2, double* out, int64_t n);
/* out[i] = the spec's variate number `kind` (0 gamma(shape p), 1 beta(p,q), 2 update_alpha
 * with alpha_old p, K = (int)q, N = 1000, a = b = 1) for stream index i, on the GPU */
int bmm_device_variates(int device, int kind, double p, double q, uint64_t seed, uint32_t sweep,
                        double* out, int64_t n);
/* The same with parameters per element: out[i] from p[i], q[i] and the scalars a, b, N, for stream index i
 * (kinds 0 and 1: streams 3 and 4 of counter word i; kinds 2 and 3: seed + i).
 *   0  gamma(shape p[i])                                   (q may be NULL)
 *   1  beta(p[i], q[i]), the spec's rbeta_
 *   2  update_alpha_ from alpha_old = p[i] with K = (int)q[i], under (a, b, N)
 *   3  the same through update_alpha_wave, the form the kernels run: one wave per element, lane 0's value
 *   4  beta(p[i], q[i]) with X and Y drawn by two threads 128 apart and joined through LDS, by the device functions
 *      k_sb_theta_tables draws theta with
 * Kinds 3 and 4 equal kinds 2 and 1 bit for bit. */
int bmm_device_variates_ex(int device, int kind, const double* p, const double* q, double a, double b, double N,
                           uint64_t seed, uint32_t sweep, double* out, int64_t n);
int bmm_device_count(int* n);

#ifdef __cplusplus
}
#endif
#endif
