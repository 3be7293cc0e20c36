/* bmm_oracle.h -- CPU oracle for the cluster-allocation path of stulacy/bmm-mcmc.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing under bmm-mcmc_amd/ may include, link or call
 * this; only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg do.
 *
 * PARITY UNPINNED for every RNG-dependent output: the reference (R + Rcpp +
 * RcppArmadillo + R nmath) cannot be built or run in this image, ships no tests and
 * no golden vectors, and draws through R's Mersenne-Twister, which a counter-based
 * device generator cannot reproduce.  What pins this file instead:
 *   - the RNG-free conditionals are checked against closed-form known answers
 *     recomputed from the cited reference lines with NumPy (tests/golden/make_kats.py);
 *   - the bundled datasets' documented generating parameters (R/bmm-mcmc.R:13-17,
 *     31-35, 46-50) as statistical acceptance bounds;
 *   - Philox4x32-10 and Philox2x32-10 against the Random123 known-answer vectors;
 *   - the stationary law of the batch-1 chains against the exact posterior by enumeration of every
 *     allocation of seven observations (scipy log-beta / log-gamma; tests/test_oracle_posterior.py): DP,
 *     stick-breaking, full sampler, and the alpha update against quadrature.
 *
 * Two restatements per sampler:
 *   *_literal : the reference algorithm as written -- per-cluster member lists,
 *               sums recomputed for every (i,k,d), glibc log/exp, one observation at
 *               a time (collapsed_gibbs.cpp:84-225, collapsed_gibbs_dp.cpp:98-283,
 *               stickbreaking.cpp:66-236).  O(N^2 P) per sweep: small N only.
 *   *_run     : the same chain from cached sufficient statistics, observations
 *               resampled in batches of `batch` against statistics frozen at batch
 *               start (own contribution removed exactly), in the build's fixed
 *               binary64 arithmetic.  batch == 1 is the reference's sequential scan.
 *               This is what the HIP path must match bit for bit.
 *
 * Layouts follow the R objects: X is N x P column-major int32 (element (i,d) at
 * i + d*N); z_out is S x N column-major, labels 1-based; theta_out is K x P x S
 * column-major; alpha_out has S entries; S = nsamples - burnin.
 */
#ifndef BMM_ORACLE_H
#define BMM_ORACLE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ORACLE_NA_INT (-2147483647 - 1) /* R's NA_integer_ */

/* ---- numerics (restated; must equal bmm-mcmc_amd/csrc/bmm_spec.h bit for bit) ---- */
void oracle_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
void oracle_philox2x32_10(const uint32_t ctr[2], uint32_t key, uint32_t out[2]);
double oracle_u01(uint32_t a, uint32_t b);
double oracle_u52(uint32_t a, uint32_t b);
double oracle_expw(double x);
void oracle_expw_array(const double* x, double* y, int64_t n);
double oracle_z_uniform(uint64_t seed, uint64_t i, uint32_t sweep);
double oracle_log(double x);
double oracle_exp(double x);
double oracle_rgamma(double shape, uint64_t seed, uint32_t c0, uint32_t sweep, uint32_t stream);
double oracle_rbeta(double p, double q, uint64_t seed, uint32_t c0a, uint32_t c0b, uint32_t sweep,
                    uint32_t stream_a, uint32_t stream_b);
double oracle_update_alpha(double alpha_old, double a, double b, double N, int K, uint64_t seed,
                           uint32_t sweep);
/* array forms: element i is the scalar call at stream index c0 = i (gamma, beta) or seed + i (update_alpha, K[i]
 * truncated to int) */
void oracle_rgamma_array(const double* shape, uint64_t seed, uint32_t sweep, uint32_t stream, double* out, int64_t n);
void oracle_rbeta_array(const double* p, const double* q, uint64_t seed, uint32_t sweep, uint32_t stream_a,
                        uint32_t stream_b, double* out, int64_t n);
void oracle_update_alpha_array(const double* alpha_old, const double* K, double a, double b, double N, uint64_t seed,
                               uint32_t sweep, double* out, int64_t n);
void oracle_log_array(const double* x, double* y, int64_t n);
void oracle_exp_array(const double* x, double* y, int64_t n);
int oracle_group_width(void);
int oracle_group_width_own(void);
int oracle_group_width_for(int sampler, int K, int P); /* the spec's per-shape rule: 5, or 4 for big table images */

/* ---- RNG-free conditionals of one observation (z is 1-based, i 0-based) ---- */
/* literal = reference formula with glibc; spec = the build's table arithmetic. */
void oracle_collapsed_cond_literal(const int32_t* X, int64_t N, int P, const int32_t* z, int64_t i,
                                   int K, double alpha, double beta, double gamma,
                                   double* raw /*K*/, double* norm /*K*/);
void oracle_collapsed_cond_spec(const int32_t* X, int64_t N, int P, const int32_t* z, int64_t i,
                                int K, double alpha, double beta, double gamma,
                                double* score /*K*/, double* norm /*K*/);
/* The allocation sampler's sweep (include/bmm_mcmc.h "allocation sampler"): maxK labels, the first K_open open at
 * weight log(n + a) - log(N - 1 + K_open a) with the prior terms where empty, the rest closed (-inf, norm exactly 0). */
void oracle_alloc_cond_spec(const int32_t* X, int64_t N, int P, const int32_t* z, int64_t i, int maxK,
                            int K_open, double a, double beta, double gamma, double* score /*maxK*/,
                            double* norm /*maxK*/);
/* DP: existing clusters in label order 1..K then the new-cluster option (K+1 values). */
void oracle_dp_cond_literal(const int32_t* X, int64_t N, int P, const int32_t* z, int64_t i, int K,
                            double alpha, double beta, double gamma, double* logw /*K+1*/,
                            double* norm /*K+1*/);
void oracle_dp_cond_spec(const int32_t* X, int64_t N, int P, const int32_t* z, int64_t i, int K,
                         double alpha, double beta, double gamma, double* logw, double* norm);
void oracle_sb_cond_literal(const int32_t* X, int64_t N, int P, int64_t i, int K, const double* pi,
                            const double* theta /*K x P colmajor*/, double* raw, double* norm);
void oracle_sb_cond_spec(const int32_t* X, int64_t N, int P, int64_t i, int K, const double* pi,
                         const double* theta, double* score, double* norm);

/* ---- samplers ---- */
int oracle_collapsed_literal(const int32_t* X, int64_t N, int P, const int32_t* z0, int nsamples,
                             int K, double alpha, double beta, double gamma, double a, double b,
                             int burnin, uint64_t seed, int32_t* z_out, double* theta_out,
                             double* alpha_out);
int oracle_collapsed_run(const int32_t* X, int64_t N, int P, const int32_t* z0, int nsamples, int K,
                         double alpha, double beta, double gamma, double a, double b, int burnin,
                         int64_t batch, uint64_t seed, int32_t* z_out, double* theta_out,
                         double* alpha_out);
/* The allocation sampler's sweeps, moves off, as a third mode of the counts chain: rows as oracle_collapsed_run's
 * (row 0 of a run without burn-in: z0, theta NaN), the sweeps numbered first_sweep, first_sweep + 1, ...; theta_out
 * is S / Nk with NaN where a label is empty. */
int oracle_alloc_run(const int32_t* X, int64_t N, int P, const int32_t* z0, int nsamples, int maxK, int K_open,
                     double a, double beta, double gamma, int burnin, int64_t batch, uint64_t seed,
                     uint32_t first_sweep, int32_t* z_out, double* theta_out);
int oracle_dp_literal(const int32_t* X, int64_t N, int P, int nsamples, double alpha, double beta,
                      double gamma, double a, double b, int burnin, int maxK, uint64_t seed,
                      int32_t* z_out, double* theta_out, double* alpha_out);
int oracle_dp_run(const int32_t* X, int64_t N, int P, int nsamples, double alpha, double beta,
                  double gamma, double a, double b, int burnin, int maxK, int64_t batch,
                  uint64_t seed, int32_t* z_out, double* theta_out, double* alpha_out);
/* The same chains with the probability matrix of chosen sweeps beside the trace -- the N x K column-major
 * matrix the reference stores for Stephens' relabelling, filed by label, every row under the state its batch
 * saw (for the DP's first sweep that includes the doubling batch schedule).  probs_out: nprobs such matrices,
 * zero-filled by the caller; the q-th is that of sweep probs_sweeps[q] (the chain's sweep number j >= 1). */
int oracle_collapsed_run_probs(const int32_t* X, int64_t N, int P, const int32_t* z0, int nsamples, int K,
                               double alpha, double beta, double gamma, double a, double b, int burnin,
                               int64_t batch, uint64_t seed, int32_t* z_out, double* theta_out,
                               double* alpha_out, int nprobs, const int32_t* probs_sweeps, double* probs_out);
int oracle_dp_run_probs(const int32_t* X, int64_t N, int P, int nsamples, double alpha, double beta,
                        double gamma, double a, double b, int burnin, int maxK, int64_t batch,
                        uint64_t seed, int32_t* z_out, double* theta_out, double* alpha_out, int nprobs,
                        const int32_t* probs_sweeps, double* probs_out);
/* the explicit samplers (variant 0 stick-breaking, 1 full; literal 0 = the *_run form, 1 = *_literal) */
int oracle_explicit_probs(int variant, int literal, const int32_t* X, int64_t N, int P, const double* pi0,
                          const double* theta0, int nsamples, int maxK, double alpha, double beta, double gamma,
                          double a, double b, int burnin, uint64_t seed, double* pi_out, int32_t* z_out,
                          double* theta_out, double* alpha_out, int nprobs, const int32_t* probs_sweeps,
                          double* probs_out);
/* the *_run chains of the two counting samplers without the S x N label trace: cluster sizes per kept
 * sweep (S x K, row-major by sweep), theta-hat, alpha, labels after the last sweep (1-based) */
int oracle_counts_summary(int sampler, const int32_t* X, int64_t N, int P, const int32_t* z0, int nsamples,
                          int K, double alpha, double beta, double gamma, double a, double b, int burnin,
                          int64_t batch, uint64_t seed, int32_t* nk_out, double* theta_out,
                          double* alpha_out, int32_t* z_last);
int oracle_sb_literal(const int32_t* X, int64_t N, int P, const double* pi0, const double* theta0,
                      int nsamples, int maxK, double alpha, double beta, double gamma, double a,
                      double b, int burnin, uint64_t seed, double* pi_out, int32_t* z_out,
                      double* theta_out, double* alpha_out);
int oracle_sb_run(const int32_t* X, int64_t N, int P, const double* pi0, const double* theta0,
                  int nsamples, int maxK, double alpha, double beta, double gamma, double a, double b,
                  int burnin, uint64_t seed, double* pi_out, int32_t* z_out, double* theta_out,
                  double* alpha_out);

int oracle_full_literal(const int32_t* X, int64_t N, int P, const double* pi0, const double* theta0,
                        int nsamples, int K, double alpha, double beta, double gamma, double a, double b,
                        int burnin, uint64_t seed, double* pi_out, int32_t* z_out, double* theta_out,
                        double* alpha_out);
int oracle_full_run(const int32_t* X, int64_t N, int P, const double* pi0, const double* theta0,
                    int nsamples, int K, double alpha, double beta, double gamma, double a, double b,
                    int burnin, uint64_t seed, double* pi_out, int32_t* z_out, double* theta_out,
                    double* alpha_out);

/* ---- CPU baseline timing: `nthreads` independent chains (seed+t), one per thread,
 * each running `sweeps` sweeps of the *_run form; returns wall seconds (sweep loop only,
 * set-up excluded), or a negative value on error.  sampler: 0 collapsed, 1 dp, 2 sb. ---- */
double oracle_time_sweeps(int sampler, const int32_t* X, int64_t N, int P, int K, int sweeps,
                          int64_t batch, uint64_t seed, int nthreads);

const char* oracle_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
