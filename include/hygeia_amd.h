/*
 * hygeia_amd.h -- C ABI of the MI355X-native Hygeia change-point inference path.
 *
 * Drop-in boundary for the two-group (case/control) inference engine of
 * ucl-medical-genomics/hygeia. The reference exposes this path as
 *
 *   filter_and_smoother_algorithm.run(observations, initial_state_prior,
 *       initial_proposal, transition_fn, observation_fn, num_particles,
 *       proposal_fn, num_resampled_ancestors, optimal_resampling,
 *       multinomial_resampling, num_simulations)
 *     -> (BackwardSimulationResults(particle={merged_state [T,B],
 *          control_state [T,B,2], case_state [T,B,2]}),
 *         final_unnormalized_log_weights [N_max])
 *   (src/two_group/hygeia/filter_and_smoother_algorithm.py:38-138)
 *
 * with the model (CaseControlRegimeModel, case_control_regime_model.py:41-244)
 * and the proposal (CaseControlProposal, case_control_proposal_mappings.py:3-216)
 * passed in as Python callables, driven by
 * src/two_group/run_inference_two_groups.py:92-322 ("hygeia infer"). Here the
 * model is fixed (it is the only one the CLI builds) and given by its
 * parameters; everything else is plain pointers and sizes.
 *
 * Conventions: every entry point returns HYG_OK (0) or a negative HYG_E* code
 * and never throws; hyg_last_error() gives a thread-local message. The caller
 * owns every buffer. Functions taking a `stream` argument enqueue work on that
 * hipStream_t (NULL = the default stream) and take DEVICE pointers; functions
 * named *_host take host pointers and synchronise. There is no CPU fallback:
 * without a HIP device every compute entry point returns HYG_EDEVICE.
 *
 * Threading: a model handle (hyg_tg_model / hyg_sg_model) is read-only after
 * creation except for its per-stream pinned staging buffers, which are
 * mutex-guarded; several host threads may launch with one model, each on its
 * own stream, without waiting for each other's kernels. hyg_set_kernel_timing /
 * hyg_tg_last_kernel_ms are a process-wide diagnostic and are not thread-safe.
 * The single-group chain launches need two workgroups per chain resident at
 * once; they stay correct on a shared GPU (a chain's pair then waits for a
 * free CU) but are sized for a GPU they have to themselves.
 */
#ifndef HYGEIA_AMD_H
#define HYGEIA_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HYG_KMAX 16

#define HYG_OK 0
#define HYG_EINVAL (-1)
#define HYG_ENUMERIC (-2) /* all particle weights became -inf */
#define HYG_EDEVICE (-3)
#define HYG_ENOMEM (-4)
#define HYG_EUNSUPPORTED (-5)

/* Parameters of the two-group model as "hygeia infer" receives them
 * (absl flags at run_inference_two_groups.py:19-72, theta file at :76-89,
 * fixed kappa at :158-161). */
typedef struct hyg_tg_params {
  int32_t n_regimes;               /* K = len(--mu) (:126)                        */
  int32_t minimum_duration;        /* u, --minimum_duration, default 3 (:25-27)   */
  int32_t num_resampled_ancestors; /* M, --num_resampled_particles, default 50     */
  int32_t num_samples_backward;    /* B, --num_samples_backward, default 25       */
  int32_t optimal_resampling;      /* 1 on the CLI path (:274)                    */
  int32_t multinomial;             /* --multinomial; used only when optimal == 0  */
  int32_t theta_len;               /* number of values in theta (K^2 on the CLI)  */
  int32_t _pad;
  double mu[HYG_KMAX];             /* --mu (float32 in the reference)             */
  double sigma[HYG_KMAX];          /* --sigma                                     */
  double theta[HYG_KMAX * HYG_KMAX]; /* theta_{chrom}.csv.gz 'data': K(K-1) log-p
                                        blocks, then K logit-omega (:76-89)       */
  double omega_case;               /* --omega_case, default 0.8 (:28-30)          */
  double merge_log_prob;           /* --merge_log_prob, default log(0.1) (:31-33) */
  double split_prob;               /* --split_prob, default 0.01 (:34-36)         */
  double kappa_control;            /* 2 (:158-159)                                */
  double kappa_case;               /* 2 (:160-161)                                */
} hyg_tg_params;

/* Fills p with the reference's flag defaults (K = 6, uniform theta). */
void hyg_tg_params_default(hyg_tg_params* p);

/* One chain = one (chromosome, segment, seed) task of modules/two_group/4_infer.nf,
 * i.e. one run_inference_two_groups.py process. */
typedef struct hyg_tg_chain {
  int64_t site_begin; /* first site of the chain in the site-major input arrays  */
  int32_t n_sites;    /* T (segment + buffers, run_inference_two_groups.py:199-200) */
  int32_t _pad;
  uint64_t seed;      /* --seed                                                  */
  uint64_t chain_id;  /* RNG stream id of the chain (e.g. chrom*2^32 + batch)    */
  int64_t out_begin;  /* first output row of the chain in the output arrays      */
} hyg_tg_chain;

typedef struct hyg_tg_model hyg_tg_model; /* opaque: derived constants + tables */

/* Builds the model: derived constants (T2/T4 of SURVEY 8a), Beta-Binomial
 * log-gamma tables for read counts <= max_total_reads, and the hazard tables
 * (case_control_regime_model.py:111-168) for durations <= max_duration.
 * Uploads the tables to the current HIP device when one is present. */
int hyg_tg_model_create(const hyg_tg_params* params, int32_t max_total_reads,
                        int32_t max_duration, hyg_tg_model** out);
void hyg_tg_model_destroy(hyg_tg_model* model);

/* Derived sizes: I = 2K + K^2 proposal slots, N_max = M * I particles
 * (run_inference_two_groups.py:263,285). */
int32_t hyg_tg_num_particles(const hyg_tg_model* model);

/* 1 when the model's chains keep their particle arrays (the N_max log-weights
 * and sort keys, 16 B per particle) in global memory, else 0. That is the case
 * exactly when the forward kernel's LDS layout at 256 threads exceeds the
 * 160 KiB of a CU: from K = 13 at M = 50, or e.g. K = 6 at M = 200. Such a
 * shape runs both kernels at 256 threads whatever width is forced, with a
 * per-chain scratch in the workspace (hyg_tg_workspace_bytes). Every shape
 * with M <= 256 runs; M > 256 is HYG_EUNSUPPORTED. No device needed.
 * Diagnostic. No reference counterpart. */
int32_t hyg_tg_global_weights(const hyg_tg_model* model);

/* Threads per chain workgroup of the forward kernel for a launch of n_chains
 * chains on the current device: 256 (up to three chains per CU) or, at most
 * one chain per CU, the low-occupancy width 512, whose extra waves shorten the
 * parallel phases of each step of the sequential chain (512 also for the
 * K = 12 stress shape, one chain per CU by its LDS). Always 256 for a shape
 * with hyg_tg_global_weights, forced or not. Diagnostic: the launch
 * functions choose it themselves. No reference counterpart (the reference
 * runs one chain per CPU process, modules/two_group/4_infer.nf:28). */
int32_t hyg_tg_threads_per_chain(const hyg_tg_model* model, int32_t n_chains);

/* The same for the backward kernel (256, or 768 at most one chain per CU).
 * Either width is the automatic or forced one where its kernel can run the
 * shape (LDS layout within 160 KiB, at least M threads), else 256: a shape just
 * under the hyg_tg_global_weights limit fits at 256 threads only (K = 12,
 * M = 54: 163 392 B, 164 000 B at 512), so no choice or override of the width
 * makes a shape with M <= 256 fail. Diagnostic. */
int32_t hyg_tg_backward_threads_per_chain(const hyg_tg_model* model, int32_t n_chains);

/* Forward-kernel workgroups (chains) one CU holds at the width a launch of
 * n_chains uses (the HIP occupancy query with the kernel's LDS): 3 for the
 * pipeline shape at 256 threads, 1 at the low-occupancy width. 0 without a
 * device. Diagnostic. */
int32_t hyg_tg_chains_per_cu(const hyg_tg_model* model, int32_t n_chains);

/* LDS bytes of one chain workgroup of the forward (backward = 0) or backward
 * kernel at `threads` (64, 128, 256, 512 or 768; 0 for another width). A shape
 * with hyg_tg_global_weights has the one width 256, whose layout leaves the
 * particle arrays out; every other width reports 0 for it. No
 * device needed. Diagnostic: C3 on one GPU needs three 256-thread forward
 * chains per CU, and the hardware's LDS allocation leaves the pipeline shape
 * little room (53 520 B holds three per CU; 53 776 B held two while the
 * occupancy query still reported three); tests pin it. */
size_t hyg_tg_lds_bytes(const hyg_tg_model* model, int32_t threads, int32_t backward);

/* The kernel instantiation a launch of n_chains chains runs on the current
 * device, forward (backward = 0) or backward, as a NUL-terminated name of the
 * form kernel<threads,K,M,B,phase timers,global arrays>, e.g.
 * "tg_backward_kernel<256,12,50,25,false,true>" (K, M, B = 0: the build for any
 * shape). Writes at most len bytes, the NUL included; returns the bytes needed
 * (call with buf = NULL to size the buffer) or a negative HYG_E* code:
 * HYG_EUNSUPPORTED for a shape no kernel runs (M > 256). No device needed.
 * Diagnostic: it is the launcher's own choice, so a test can pin it. */
int32_t hyg_tg_kernel_name(const hyg_tg_model* model, int32_t n_chains, int32_t backward, char* buf, int32_t len);

/* Test / tuning override of the chain workgroup sizes for every later launch
 * in the process: forward and backward threads (64, 128, 256, 512 or 768;
 * 0 = the automatic choice above). Not thread-safe. The results do not depend
 * on it: every width computes the same bits. A shape with
 * hyg_tg_global_weights ignores it and runs at 256 threads. */
int hyg_tg_force_threads(int32_t forward, int32_t backward);

/* Tail overlap of hyg_tg_run_chains (on = 1, the default; 0 = off) for every
 * later launch in the process. When the forward holds one chain per CU and
 * the chains fill more than one round of CUs with a partial last round (the
 * K = 12 stress shape: 1 164 chains on 256 CUs), the launch runs the forward
 * of the full rounds, then the rest's forward on the launch stream while the
 * full rounds' backward runs on a second stream of the library's, on the CUs
 * the last round leaves idle; the call's stream waits for both. The results
 * do not depend on it (GPU test). Not thread-safe. No reference counterpart. */
int hyg_tg_set_tail_overlap(int32_t on);

/* Gather window of the forward kernels for every later launch in the process:
 * on a step that resamples through the top set, the waves that would wait for
 * wave 0's serial section (the K loop and the systematic search) compute
 * meanwhile, for the first `positions` sorted positions of the set, the
 * ancestor a parent at that position becomes (state, weight, hazards), and the
 * gather copies it for every parent inside the window instead of computing it
 * after the search. 0 = off (the gather computes every ancestor); -1 = the
 * default; at most 256, the largest top set. A kernel takes what its waves
 * and its scratch hold of the window (192 positions at 256 threads). The
 * results do not depend on it: the parked values are the gather's own
 * arithmetic (GPU test). Tests use small windows to mix parents inside and
 * outside it. Not thread-safe. No reference counterpart. */
int hyg_tg_set_gather_window(int32_t positions);

/* Rotating wave priorities of the 256-thread forward kernels (the width that
 * shares a CU between up to three chains; full, forward-only and traced
 * launches) for every later launch in the process: 1 = on (the default), 0 = off. A SIMD issues by
 * priority, then by age, so with every chain at one priority the chains of a CU
 * advance at fixed, unequal rates for the whole launch and the launch waits for
 * the youngest. With rotation each wave takes a base priority 0 .. 2 from its
 * wave slot in the SIMD and the epoch of the device's constant clock, the six
 * orders of three priorities in turn, so the chains of a CU advance alike on
 * average. The backward kernels keep one priority (rotation measured slower
 * there). The results do not depend on it: a priority changes when a wave
 * issues, never what it computes (GPU test). Not thread-safe. No reference
 * counterpart. */
int hyg_tg_set_priority_rotation(int32_t on);

/* The base priority (0 .. 2) a wave in SIMD wave slot `slot` (>= 0) holds at the
 * clock value `ticks` (10 ns each) while rotation is on, from the table the
 * kernels use; -1 for a negative slot. hyg_tg_priority_epoch_ticks: the ticks
 * one order of priorities lasts. Diagnostics; no GPU needed. */
int32_t hyg_tg_priority_base(uint64_t ticks, int32_t slot);
int32_t hyg_tg_priority_epoch_ticks(void);

/* How the 256-thread forward kernels that keep their weights in LDS (full,
 * forward-only, traced and resuming launches) walk a wave's candidate list in
 * the step's log-sum-exp and in the gather of the top set, for every later
 * launch in the process: 1 = per 64 entries (the default), 0 = in whole chunks
 * of 256 as before. Both loops are unrolled four entries per lane, so a list
 * of 230 entries used to pay for 256 slots and one of 260 for 512; walked per
 * 64 entries, the rest of a list takes a two-entry and a one-entry pass
 * instead of one more whole chunk. The results do not depend on it: per entry
 * the operations are the same, and the sums are exact integer sums (GPU
 * test). hyg_tg_fine_list_walk: the current setting. Not thread-safe. No
 * reference counterpart. */
int hyg_tg_set_fine_list_walk(int32_t on);
int32_t hyg_tg_fine_list_walk(void);

/* The forward of a full launch (hyg_tg_run_chains[_multi]) in rounds, for every
 * later launch in the process. When a launch leaves some CUs one chain more
 * than the others for its whole length (n chains on C CUs, n % C != 0), the
 * forward can be cut in time: round 1 runs every chain to a cut of its own,
 * the kernel ends, and round 2 resumes every chain from its last history
 * record in another block order, in which the chains of the heavier CUs sit on
 * lighter ones. 0 = one launch; 1 = automatic (the default: two rounds where
 * the schedule expects a gain, see hyg_tg_forward_schedule); 2 = two rounds
 * whatever the lengths and loads, where the kernel allows it (tests). Other
 * values are HYG_EINVAL. Only 256-thread forwards that record history and keep
 * their arrays in LDS are cut; forward-only and traced launches never. The
 * results do not depend on it: a chain is a function of its record (GPU test).
 * A launch in rounds stays asynchronous on its stream; its round tables live in
 * a buffer the library keeps per device, so the forward of such a launch
 * starts on the device after the forward of the one before it on that device,
 * whatever their streams. Where the buffer cannot be had the launch runs as
 * one launch. Not thread-safe. No reference counterpart. */
int hyg_tg_set_forward_rounds(int32_t mode);

/* The schedule such a launch of n_chains chains of n_sites[i] sites would run
 * on a device of `cus` CUs (0: the current device's count as the launcher sees
 * it, hyg_tg_device_cus; 256 on a host without a device), as data; no GPU
 * needed. The kernel is planned as the launch's (current device, forced
 * widths). `resident`: forward workgroups one CU holds (hyg_tg_chains_per_cu).
 * Arrays of max_rounds (>= 2) x n_chains entries, round r at r * n_chains:
 * blocks[r] is the grid of round r (0: no such round), order[r n + p] the chain
 * block p runs (-1 behind the grid), and chain i runs steps [begin[r n + i],
 * end[r n + i]) in round r (empty: not in the round). A round's block p sits
 * on CU p % CUs. Cuts are 64 q + 1. Returns the number of rounds (1 or 2) or a
 * negative HYG_E* code. The automatic mode cuts a launch when k = n / C >= 1,
 * e = n % C > 0, k + 1 <= resident, the e (k + 1) chains of the heavier CUs
 * fit the (C - e) k blocks of the lighter ones, the step rates of both loads
 * were measured, and the longest chain has at least 4 096 steps. */
int32_t hyg_tg_forward_schedule(const hyg_tg_model* model, const int32_t* n_sites, int32_t n_chains, int32_t multi,
                                int32_t forward_only, int32_t cus, int32_t resident, int32_t max_rounds,
                                int32_t* blocks, int32_t* order, int32_t* begin, int32_t* end);

/* Compute units of `device` as the two-group launcher sees them: the width
 * choice (one chain per CU or more) and the tail overlap depend on it. Cached
 * per device, so a process that switches devices (hyg_set_device) uses each
 * device's own count. 0 if unknown (no such device, no HIP). No reference
 * counterpart. */
int32_t hyg_tg_device_cus(int32_t device);

/* Test override of that count for device (0 <= device < 64); cus = 0 drops
 * the override (the next use queries the device). The results do not depend
 * on it (every width computes the same bits); launches after it are shaped as
 * on a device with that many CUs. */
int hyg_tg_set_device_cus(int32_t device, int32_t cus);

/* Test override of the single-group chain's log-weight sort for every later
 * launch in the process. The sort orders one 64-bit word per particle: the
 * order key's top 64 - bits bits and the particle index (bits = 8, or 0 for
 * the default). Wherever keys that agree on those bits disagree below them,
 * the kernel detects it and re-sorts exactly, so the results do not depend on
 * it; larger values (up to 60) make that path run often. Not thread-safe. */
int hyg_sg_force_key_drop(int32_t bits);

/* Per-site emission table E[t][g*K + r] = log g_t for group g (0 control,
 * 1 case) and regime r: sum over samples of BetaBinomial(meth | total,
 * alpha_r, beta_r) (case_control_regime_model.py:197-231). Counts are
 * site-major uint16 [T][S]. Device pointers. */
int hyg_tg_emission(const hyg_tg_model* model, const uint16_t* meth_ctrl, const uint16_t* tot_ctrl,
                    int32_t s_ctrl, const uint16_t* meth_case, const uint16_t* tot_case, int32_t s_case,
                    int64_t n_sites, double* emission, void* stream);

/* Workspace bytes for the forward->backward ancestor history of `n_chains`
 * chains totalling `total_steps` filter steps. For the K = 12 stress shape the
 * bound also holds a full-N weight scratch per chain (Nmax f64, 67 KB), which
 * only the 256-thread backward of a launch with more chains than CUs uses; it
 * is charged whatever the width, so the size does not depend on the launch
 * width or hyg_tg_force_threads (a conservative bound: under 0.04 % of a
 * full-length chain's history). For a shape with hyg_tg_global_weights it holds
 * a 256-byte-aligned scratch per chain for the forward's log-weights and sort
 * keys (16 B x N_max; 1.2 MB at K = 16, M = 256), whose weight part the
 * backward reuses. hyg_tg_run_chains places the scratches behind the records
 * and returns HYG_EINVAL when the workspace does not hold them. */
size_t hyg_tg_workspace_bytes(const hyg_tg_model* model, int32_t n_chains, int64_t total_steps);

/* Outputs of hyg_tg_run_chains, all device pointers indexed by out_begin + t:
 * trajectories as the reference saves them (run_inference_two_groups.py:299-314):
 *   merged [T][B] int16, control [T][B][2] int16 (d, r), case [T][B][2] int16,
 *   split_probs [T] f32, regime_probs [T][2K] f32 (test_function means, :233-240,294-296),
 * per chain: log_z [n_chains] f64 (logsumexp of the final weights, :289-290) and
 * optionally final_log_weights [n_chains][N_max] f64 (the second return value
 * of run(), -inf padded; may be NULL), status [n_chains] int32 (HYG_OK or
 * HYG_ENUMERIC per chain; may be NULL).
 *
 * A chain whose particle weights all become -inf at some site has status
 * HYG_ENUMERIC, log_z -inf and all N_max entries of its final_log_weights row
 * -inf, the same bytes in full, forward-only and traced launches. None of its
 * rows [out_begin, out_begin + n_sites) of the five trajectory arrays is
 * written: they hold what they held before the launch. The other chains of the
 * launch are what they are without it (GPU test: tests/test_gpu_tg_enumeric.py). */
typedef struct hyg_tg_outputs {
  int16_t* merged;
  int16_t* control;
  int16_t* kase;
  float* split_probs;
  float* regime_probs;
  double* log_z;
  double* final_log_weights;
  int32_t* status;
} hyg_tg_outputs;

/* Runs the particle filter with optimal finite-state resampling followed by
 * backward simulation (filter_and_smoother_algorithm.py:38-138, 141-288,
 * 368-447) for `n_chains` independent chains, one workgroup per chain.
 * `chains` is a HOST array; `emission` is the device table of
 * hyg_tg_emission; `workspace` has hyg_tg_workspace_bytes bytes. Returns HYG_OK
 * when the launch was enqueued, whatever becomes of its chains: a chain whose
 * weights all become -inf (a table with -inf entries; counts give finite ones)
 * reports HYG_ENUMERIC in outputs->status, -inf in log_z and its
 * final_log_weights row, and leaves its trajectory rows unwritten
 * (hyg_tg_outputs); the backward simulation of that chain does not run. */
int hyg_tg_run_chains(const hyg_tg_model* model, const hyg_tg_chain* chains, int32_t n_chains,
                      const double* emission, void* workspace, size_t workspace_bytes,
                      const hyg_tg_outputs* outputs, void* stream);

/* Host-pointer convenience: one chain of T sites (the whole of one
 * run_inference_two_groups.py invocation). Outputs are host arrays sized as
 * above for one chain; final_log_weights may be NULL. */
int hyg_tg_run_chain_host(const hyg_tg_model* model, const uint16_t* meth_ctrl, const uint16_t* tot_ctrl,
                          int32_t s_ctrl, const uint16_t* meth_case, const uint16_t* tot_case, int32_t s_case,
                          int32_t n_sites, uint64_t seed, uint64_t chain_id, int16_t* merged, int16_t* control,
                          int16_t* kase, float* split_probs, float* regime_probs, double* log_z,
                          double* final_log_weights);

/* Host-pointer form of hyg_tg_run_chains (round 4): the counts of n_sites
 * sites (host, site-major) are copied in, the emission table is formed, the
 * n_chains chains (host array: site_begin into the counts, out_begin into the
 * output rows) run in one launch, and the outputs come back into host arrays
 * of out_rows rows (layouts as above), log_z and status [n_chains]
 * (final_log_weights [n_chains][N_max], may be NULL). Returns HYG_OK when the
 * launch ran; a chain whose weights all became -inf has HYG_ENUMERIC in its
 * status, -inf in log_z and final_log_weights, and its rows of the five
 * trajectory arrays are unspecified (the device does not write them, and the
 * staging buffers they are copied from are not initialised). The same holds
 * for hyg_tg_run_chains_host_multi, and for hyg_tg_run_chain_host, which
 * returns HYG_ENUMERIC itself for its one chain. `hygeia infer_many` (every task that modules/two_group/4_infer.nf:42-48
 * fans out, in one launch) runs through it without torch. */
int hyg_tg_run_chains_host(const hyg_tg_model* model, const uint16_t* meth_ctrl, const uint16_t* tot_ctrl,
                           int32_t s_ctrl, const uint16_t* meth_case, const uint16_t* tot_case, int32_t s_case,
                           int64_t n_sites, const hyg_tg_chain* chains, int32_t n_chains, int64_t out_rows,
                           int16_t* merged, int16_t* control, int16_t* kase, float* split_probs,
                           float* regime_probs, double* log_z, double* final_log_weights, int32_t* status);

/* ------------------------------------------------ multi-model launches
 * One launch whose chains each name their model: the pipeline's model is per
 * chromosome (theta_{chrom}.csv.gz, step 2's estimate of P and omega for the
 * control group, sets the control transitions, the hazard tables and their
 * length), so the tasks of a whole genome share a launch only this way
 * (`hygeia infer_genome`). Each chain computes exactly what it computes alone
 * with its own model through hyg_tg_run_chains: the chain kernels of such a
 * launch differ from the single-model ones by one load of the chain's model
 * from a device table at entry. None of the entry points below has a
 * reference counterpart: the reference runs one process per task
 * (modules/two_group/4_infer.nf:28). The conventions above apply. */

/* HYG_OK when the n_models models can share a launch: they agree on n_regimes,
 * minimum_duration, num_resampled_ancestors, num_samples_backward,
 * optimal_resampling, max_total_reads and, bit for bit, on mu and sigma as
 * given, so that one shape, one LDS layout and one emission table serve all of
 * them. theta, omega_case, merge_log_prob, split_prob, the kappa values and
 * max_duration may differ. Otherwise HYG_EINVAL, hyg_last_error() naming the
 * first field that differs; also HYG_EINVAL for n_models < 1 or a null entry.
 * No device needed. */
int hyg_tg_models_compatible(const hyg_tg_model* const* models, int32_t n_models);

/* Workspace bytes of a multi-model launch: hyg_tg_workspace_bytes of models[0]
 * (the bound depends on the shared shape only) plus the device table of the
 * models, which the launch keeps in the workspace header. Like that bound it
 * does not depend on the launch width or hyg_tg_force_threads. 0 for a bad
 * argument. */
size_t hyg_tg_workspace_bytes_multi(const hyg_tg_model* const* models, int32_t n_models, int32_t n_chains,
                                    int64_t total_steps);

/* hyg_tg_run_chains with chain i run under models[chain_model[i]].
 * `models` and `chain_model` (int32 [n_chains]) are HOST arrays; `emission` is
 * the table of hyg_tg_emission with any of the models (they share it);
 * `workspace` has hyg_tg_workspace_bytes_multi bytes. The launch is planned
 * from the shared shape and n_chains exactly as a single-model launch of
 * n_chains chains (width, global arrays, tail overlap, hyg_tg_force_threads,
 * hyg_tg_set_device_cus) and runs the multi-model build of the same kernel
 * (hyg_tg_kernel_name_multi). A chain may be as long as its own model's
 * max_duration. Incompatible models (hyg_tg_models_compatible) or an index out
 * of [0, n_models) give HYG_EINVAL before anything is enqueued. n_models = 1
 * is allowed and gives the bits of hyg_tg_run_chains. Every model must live on
 * the current device. The descriptor upload goes through models[0]'s staging
 * buffers (see Threading above). */
int hyg_tg_run_chains_multi(const hyg_tg_model* const* models, int32_t n_models, const hyg_tg_chain* chains,
                            const int32_t* chain_model, int32_t n_chains, const double* emission,
                            void* workspace, size_t workspace_bytes, const hyg_tg_outputs* outputs, void* stream);

/* Host-pointer form of hyg_tg_run_chains_multi, as hyg_tg_run_chains_host is
 * to hyg_tg_run_chains: the counts of every chain's sites in one site-major
 * array (a genome: the chromosomes one after another), the emission table
 * formed once with models[0], one launch, host outputs. `hygeia infer_genome`
 * runs through it without torch. */
int hyg_tg_run_chains_host_multi(const hyg_tg_model* const* models, int32_t n_models, const uint16_t* meth_ctrl,
                                 const uint16_t* tot_ctrl, int32_t s_ctrl, const uint16_t* meth_case,
                                 const uint16_t* tot_case, int32_t s_case, int64_t n_sites,
                                 const hyg_tg_chain* chains, const int32_t* chain_model, int32_t n_chains,
                                 int64_t out_rows, int16_t* merged, int16_t* control, int16_t* kase,
                                 float* split_probs, float* regime_probs, double* log_z,
                                 double* final_log_weights, int32_t* status);

/* hyg_tg_kernel_name for a multi-model launch of n_chains chains: the same
 * width and global-arrays flag, and a seventh template argument, true, e.g.
 * "tg_forward_kernel<256,6,50,25,false,false,true>". The multi-model builds
 * have no phase timers: a phase-timer request (the tuning build) runs the
 * plain build. HYG_EINVAL for incompatible models. No device needed. */
int32_t hyg_tg_kernel_name_multi(const hyg_tg_model* const* models, int32_t n_models, int32_t n_chains,
                                 int32_t backward, char* buf, int32_t len);

/* ------------------------------------------------- forward-only launches
 * The particle filter alone: log Z (the estimate of the marginal likelihood
 * that `infer` writes to log_normalizing_constants_optimal_{seed}.txt), the
 * final log-weights and the status of every chain, bit for bit those of
 * hyg_tg_run_chains on the same chains, from builds of the forward kernel that
 * record no ancestor history (an eighth template argument, false). No backward
 * kernel runs and no trajectory is written. The launch is planned exactly as
 * the forward of hyg_tg_run_chains of n_chains chains (width, global-arrays
 * flag, forced and tuned widths, CU count).
 *
 * The workspace holds the header (the chain descriptors and, for _multi, the
 * model table) and, for a hyg_tg_global_weights shape, each chain's forward
 * scratch; it holds no history and does not depend on the chains' lengths. */
size_t hyg_tg_filter_workspace_bytes(const hyg_tg_model* model, int32_t n_chains);
size_t hyg_tg_filter_workspace_bytes_multi(const hyg_tg_model* const* models, int32_t n_models, int32_t n_chains);

/* Conventions as hyg_tg_run_chains / hyg_tg_run_chains_multi: `chains` is a
 * host array (its out_begin is ignored), `emission`, `workspace`, `log_z`
 * [n_chains], `final_log_weights` [n_chains x hyg_tg_num_particles] and
 * `status` [n_chains] are device pointers; the last two may be NULL. The
 * launch is enqueued on `stream`. Errors as the full entries': HYG_EINVAL for
 * incompatible models, a model index out of range, a workspace that is too
 * small ("workspace too small") or a chain longer than its model's
 * max_duration; HYG_EUNSUPPORTED for optimal_resampling = 0 and for
 * num_resampled_ancestors > 256; HYG_EDEVICE without a device. With kernel
 * timing on, hyg_tg_last_kernel_ms reports the forward and -1 for the
 * backward. */
int hyg_tg_filter_chains(const hyg_tg_model* model, const hyg_tg_chain* chains, int32_t n_chains,
                         const double* emission, void* workspace, size_t workspace_bytes, double* log_z,
                         double* final_log_weights, int32_t* status, void* stream);
int hyg_tg_filter_chains_multi(const hyg_tg_model* const* models, int32_t n_models, const hyg_tg_chain* chains,
                               const int32_t* chain_model, int32_t n_chains, const double* emission, void* workspace,
                               size_t workspace_bytes, double* log_z, double* final_log_weights, int32_t* status,
                               void* stream);

/* Host-pointer forms, as hyg_tg_run_chains_host[_multi]: the counts of n_sites
 * sites in (site-major uint16), host `log_z`, `final_log_weights` (may be
 * NULL) and `status` out; the emission table is formed once, then one launch. */
int hyg_tg_filter_chains_host(const hyg_tg_model* model, const uint16_t* meth_ctrl, const uint16_t* tot_ctrl,
                              int32_t s_ctrl, const uint16_t* meth_case, const uint16_t* tot_case, int32_t s_case,
                              int64_t n_sites, const hyg_tg_chain* chains, int32_t n_chains, double* log_z,
                              double* final_log_weights, int32_t* status);
int hyg_tg_filter_chains_host_multi(const hyg_tg_model* const* models, int32_t n_models, const uint16_t* meth_ctrl,
                                    const uint16_t* tot_ctrl, int32_t s_ctrl, const uint16_t* meth_case,
                                    const uint16_t* tot_case, int32_t s_case, int64_t n_sites,
                                    const hyg_tg_chain* chains, const int32_t* chain_model, int32_t n_chains,
                                    double* log_z, double* final_log_weights, int32_t* status);

/* The instantiation a forward-only launch of n_chains chains runs, as
 * hyg_tg_kernel_name[_multi] report the full launch's: the name carries all
 * eight template arguments, the last one false, e.g.
 * "tg_forward_kernel<256,6,50,25,false,false,false,false>". There are no
 * phase-timer builds. No device needed. */
int32_t hyg_tg_filter_kernel_name(const hyg_tg_model* model, int32_t n_chains, char* buf, int32_t len);
int32_t hyg_tg_filter_kernel_name_multi(const hyg_tg_model* const* models, int32_t n_models, int32_t n_chains,
                                        char* buf, int32_t len);

/* ------------------------------------------- traced forward-only launches
 * A forward-only launch that also returns what the filter knows at every site.
 * For a chain of T sites the launch writes row out_begin + t, t in [0, T), of
 * up to three arrays (any of the pointers may be NULL, not all three):
 *
 *   log_z_t      f64 [rows]      the log Z the same chain (seed, chain id) would
 *                                report if it ended at site t, bit for bit; row
 *                                T - 1 is the launch's log_z
 *   split_probs  f32 [rows]      P(merged_t = 0 | y_0..t)
 *   regime_probs f32 [rows][2K]  P(regime_t = r | y_0..t), column g*K + r,
 *                                control (g = 0) first
 *
 * the filtering marginals of the particle set the chain ending at t would
 * report (its final_log_weights w_n and their states): with mx = max w_n,
 * m_n = hyg_fix100(hyg_exp(w_n - mx)) (the u128 images at 2^-100 of the step's
 * log-sum-exp), S their integer sum and S_c the integer sum over the particles
 * of a class (merged == 0; control regime r; case regime r), the output is
 * (float)(hyg_u128_to_f64(S_c, 100) / hyg_u128_to_f64(S, 100)): one IEEE f64
 * division rounded to f32, whatever the reduction order. With both probability
 * pointers NULL the class sums are skipped. If a chain's status is
 * HYG_ENUMERIC, the rows from the first site whose weights are all -inf hold
 * -inf in log_z_t and NaN in the probabilities. log_z, final_log_weights and
 * status are those of hyg_tg_filter_chains, bit for bit. No reference
 * counterpart as a launch (the reference's filter-only module,
 * hygeia/particle_filter_deterministic_proposal.py, runs one chain). */
typedef struct hyg_tg_trace {
  double* log_z_t;
  float* split_probs;
  float* regime_probs;
} hyg_tg_trace;

/* hyg_tg_filter_chains[_multi] with a trace: the same arguments, the same
 * workspace (hyg_tg_filter_workspace_bytes[_multi]: no history) and the same
 * errors; `trace` holds device pointers, and chains[i].out_begin is honoured
 * as hyg_tg_run_chains honours it. A NULL trace or one whose three pointers
 * are NULL is HYG_EINVAL (that caller wants hyg_tg_filter_chains). The launch
 * is planned as the forward-only launch of n_chains chains and runs the
 * traced build of its kernel (a ninth template argument, true). */
int hyg_tg_trace_chains(const hyg_tg_model* model, const hyg_tg_chain* chains, int32_t n_chains,
                        const double* emission, void* workspace, size_t workspace_bytes, const hyg_tg_trace* trace,
                        double* log_z, double* final_log_weights, int32_t* status, void* stream);
int hyg_tg_trace_chains_multi(const hyg_tg_model* const* models, int32_t n_models, const hyg_tg_chain* chains,
                              const int32_t* chain_model, int32_t n_chains, const double* emission, void* workspace,
                              size_t workspace_bytes, const hyg_tg_trace* trace, double* log_z,
                              double* final_log_weights, int32_t* status, void* stream);

/* Host-pointer forms, as hyg_tg_filter_chains_host[_multi]: the trace arrays
 * are host arrays of out_rows rows (any of them NULL, not all three); every
 * chain must have out_begin >= 0 and out_begin + n_sites <= out_rows, else
 * HYG_EINVAL before anything runs. Rows no chain owns are left as they are. */
int hyg_tg_trace_chains_host(const hyg_tg_model* model, const uint16_t* meth_ctrl, const uint16_t* tot_ctrl,
                             int32_t s_ctrl, const uint16_t* meth_case, const uint16_t* tot_case, int32_t s_case,
                             int64_t n_sites, const hyg_tg_chain* chains, int32_t n_chains, int64_t out_rows,
                             double* log_z_t, float* split_probs, float* regime_probs, double* log_z,
                             double* final_log_weights, int32_t* status);
int hyg_tg_trace_chains_host_multi(const hyg_tg_model* const* models, int32_t n_models, const uint16_t* meth_ctrl,
                                   const uint16_t* tot_ctrl, int32_t s_ctrl, const uint16_t* meth_case,
                                   const uint16_t* tot_case, int32_t s_case, int64_t n_sites,
                                   const hyg_tg_chain* chains, const int32_t* chain_model, int32_t n_chains,
                                   int64_t out_rows, double* log_z_t, float* split_probs, float* regime_probs,
                                   double* log_z, double* final_log_weights, int32_t* status);

/* The instantiation a traced launch of n_chains chains runs: the forward-only
 * launch's with a ninth template argument, true, e.g.
 * "tg_forward_kernel<256,6,50,25,false,false,false,false,true>". No device
 * needed. */
int32_t hyg_tg_trace_kernel_name(const hyg_tg_model* model, int32_t n_chains, char* buf, int32_t len);
int32_t hyg_tg_trace_kernel_name_multi(const hyg_tg_model* const* models, int32_t n_models, int32_t n_chains,
                                       char* buf, int32_t len);

/* Kernel timing for benchmarks: when enabled, HIP events are recorded on the
 * launch stream around the emission, forward and backward kernels;
 * hyg_tg_last_kernel_ms waits for the last ones and returns their durations
 * in ms (-1 for a kernel not launched since timing was enabled). */
void hyg_set_kernel_timing(int enable);
int hyg_tg_last_kernel_ms(float* ms3);

/* ======================================================== single group
 * The single-group engine (src/single_group/src/cpp): SMC over the semi-Markov
 * state (d, r) with up to N_max particles, optimal finite-state resampling and
 * online marginal smoothing of the regime indicators (Alenlov & Olsson 2019),
 * as exported to R by
 *   runOnlineCombinedInferenceCpp(vartheta, thetaInit, genomicPositions,
 *       nTotalReads [S x T], nMethylatedReads [S x T], nParticlesMax,
 *       smcProposalType = 1, smcResampleType = 2, useOnlineMarginalSmoothing,
 *       epsilon, useOnlineParameterEstimation = false, ...)
 *     -> regimeProbabilityEstimates [T][1 + K] (position, P(r = 1..K))
 *   (singleGroup.cpp:76-189; called by bin/estimate_parameters_and_regimes:303-322).
 * Online parameter estimation (useOnlineParameterEstimation = TRUE, the
 * pipeline's --estimate_parameters) is the hyg_sg_*_pe family below. */
typedef struct hyg_sg_params {
  int32_t n_regimes;          /* K = vartheta[1] (model_functions.R:36-59)          */
  int32_t minimum_duration;   /* u = vartheta[0]                                    */
  int32_t num_particles_max;  /* nParticlesMax, 250 in the pipeline                 */
  int32_t resample_type;      /* smcResampleType: 2 = optimal finite state (only)    */
  int32_t is_kappa_fixed;     /* vartheta[2K+2]                                     */
  int32_t theta_len;          /* K(K-1) + K (+ K if kappa is estimated)             */
  double alpha[HYG_KMAX];     /* vartheta[2 .. K+1]                                  */
  double beta[HYG_KMAX];      /* vartheta[K+2 .. 2K+1]                               */
  double kappa[HYG_KMAX];     /* vartheta[2K+3 ..] when fixed                        */
  double theta[HYG_KMAX * (HYG_KMAX + 1)]; /* K rows of K-1 log-weights of P, K logit(omega), (K log kappa) */
  double epsilon;             /* smoothing variance threshold, 0.01                  */
} hyg_sg_params;

typedef struct hyg_sg_model hyg_sg_model;

/* One chain: the sites [site_begin, site_begin + n_sites) of the site-major
 * count arrays (one sample group on one chromosome). */
typedef struct hyg_sg_chain {
  int64_t site_begin;
  int32_t n_sites;
  int32_t _pad;
  uint64_t seed;
  uint64_t chain_id;
  int64_t out_begin;
} hyg_sg_chain;

void hyg_sg_params_default(hyg_sg_params* p);
/* Derived quantities of ModelParameters::setKnownParameters/setUnknownParameters
 * (singleGroup.h:173-335): P, omega, kappa and the hazard tables rho(d, r)
 * with the exit status, Beta-Binomial lgamma tables for counts <= max_total_reads. */
int hyg_sg_model_create(const hyg_sg_params* params, int32_t max_total_reads, int32_t max_duration,
                        hyg_sg_model** out);
void hyg_sg_model_destroy(hyg_sg_model* model);
/* E[t][r] = sum_s log BetaBinomial(meth_ts | tot_ts, alpha_r, beta_r)
 * (Model::evaluateLogObservationDensity, singleGroup.h:611-627). Device pointers, [T][S]. */
int hyg_sg_emission(const hyg_sg_model* model, const uint16_t* meth, const uint16_t* tot, int32_t n_samples,
                    int64_t n_sites, double* emission, void* stream);
/* Workspace for n_chains chains with room for `psi_capacity` pending smoothing
 * times per chain (the online-smoothing state; 0 = default 4096). */
size_t hyg_sg_workspace_bytes(const hyg_sg_model* model, int32_t n_chains, int32_t psi_capacity);
/* Runs SMC + online marginal smoothing for n_chains chains (one workgroup
 * each). regime_probs [rows][K] f64 receives the smoothed P(r_t = r) of every
 * site (OnlineCombinedInference.h:106-117), status [n_chains] HYG_OK /
 * HYG_ENUMERIC / HYG_ENOMEM (pending smoothing times exceeded psi_capacity). */
int hyg_sg_run_chains(const hyg_sg_model* model, const hyg_sg_chain* chains, int32_t n_chains,
                      const double* emission, void* workspace, size_t workspace_bytes, int32_t psi_capacity,
                      double* regime_probs, int32_t* status, void* stream);
/* Host-pointer convenience for one chain: counts [T][S]. */
int hyg_sg_run_chain_host(const hyg_sg_model* model, const uint16_t* meth, const uint16_t* tot,
                          int32_t n_samples, int32_t n_sites, uint64_t seed, uint64_t chain_id,
                          double* regime_probs);

/* ---- online parameter estimation
 * runOnlineCombinedInferenceCpp(..., useOnlineParameterEstimation = TRUE,
 *     normaliseGradients, useAdam, nStepsWithoutParameterUpdate,
 *     learningRateExponent, learningRateFactor, ...) -> thetaEstimates
 * (singleGroup.cpp:76-189, OnlineCombinedInference.h:48-118,
 * OnlineParameterEstimation.h:42-176, GradientAscent.h:62-155), run by the
 * two-group pipeline's `hygeia estimate_parameters_and_regimes ...
 * --estimate_regime_probabilities --estimate_parameters`
 * (modules/two_group/2_estimate_parameters_and_regimes.nf:38-52). The
 * regime probabilities are smoothed under the moving theta, as the reference.
 * With is_kappa_fixed = 0 theta holds K more entries log kappa_r and the
 * gradient is the reference's as written (singleGroup.h:664-692: the omega
 * coordinate takes d log rho / d theta_kappa, the kappa coordinates stay put;
 * include/hyg_sg_pe.h). */
typedef struct hyg_sg_pe_params {
  int32_t use_adam;               /* --use_adam, TRUE                          */
  int32_t normalise_gradients;    /* --normalise_gradients, FALSE              */
  int32_t n_steps_without_update; /* --n_steps_without_parameter_update, 200   */
  int32_t _pad;
  double learning_rate_exponent;  /* --learning_rate_exponent, 0.1             */
  double learning_rate_factor;    /* --learning_rate_factor, 0.01              */
} hyg_sg_pe_params;

void hyg_sg_pe_params_default(hyg_sg_pe_params* pe);
/* Rows of theta the chains report: per chain 1 + (n_sites - 1) / every (the
 * initial theta, then theta after each update at t = every, 2 every, ...);
 * chain i's rows follow chain i-1's. The reference's thetaEstimates row t
 * (t = 0 .. T-1) is row t / every of its chain. */
int64_t hyg_sg_pe_theta_rows(const hyg_sg_chain* chains, int32_t n_chains, int32_t every);
size_t hyg_sg_pe_workspace_bytes(const hyg_sg_model* model, const hyg_sg_chain* chains, int32_t n_chains,
                                 int32_t psi_capacity);
/* As hyg_sg_run_chains, with theta updated online; theta_out [rows][theta_len]
 * f64 (device; theta_len = K^2, or K (K + 1) with kappa estimated). status may also be HYG_ENOMEM when a sojourn outgrows the
 * hazard table (HYG_SGPE_DCAP rows) before the hazard's exit. */
int hyg_sg_run_chains_pe(const hyg_sg_model* model, const hyg_sg_pe_params* pe, const hyg_sg_chain* chains,
                         int32_t n_chains, const double* emission, void* workspace, size_t workspace_bytes,
                         int32_t psi_capacity, double* regime_probs, double* theta_out, int32_t* status,
                         void* stream);
/* Host-pointer convenience for one chain: regime_probs [T][K], theta_out
 * [1 + (T - 1) / every][K^2]. */
int hyg_sg_run_chain_host_pe(const hyg_sg_model* model, const hyg_sg_pe_params* pe, const uint16_t* meth,
                             const uint16_t* tot, int32_t n_samples, int32_t n_sites, uint64_t seed,
                             uint64_t chain_id, double* regime_probs, double* theta_out);

/* ---- multi-model launches: every chain of a launch names its own model
 * (a genome's chromosomes, each with its own theta_0 or its own estimated
 * p / kappa / omega, in one launch). No reference counterpart: the pipeline
 * starts one process per chromosome
 * (modules/single_group/2_estimate_parameters.nf, 3_estimate_regimes.nf).
 *
 * HYG_OK when the n_models models can share a launch: they agree on n_regimes,
 * minimum_duration, num_particles_max, is_kappa_fixed, max_total_reads and,
 * bit for bit, on alpha and beta as given, so that one shape, one LDS layout
 * and one emission table serve all of them. theta, kappa, epsilon and
 * max_duration (and with it the hazard tables' length) may differ. Otherwise
 * HYG_EINVAL, hyg_last_error() naming the first field that differs; also
 * HYG_EINVAL for n_models < 1 or a null entry. No device needed. */
int hyg_sg_models_compatible(const hyg_sg_model* const* models, int32_t n_models);

/* Workspace bytes of a multi-model launch: hyg_sg_workspace_bytes /
 * hyg_sg_pe_workspace_bytes of models[0] (the bound depends on the shared
 * shape only) plus the chain -> model indices and the device tables of the
 * models, which the launch keeps in the workspace header. The estimation
 * inputs (theta_0 per model, one lgk / dgk table per distinct kappa vector)
 * live in a stream-ordered side allocation, as in hyg_sg_run_chains_pe. 0 for
 * a bad argument. */
size_t hyg_sg_workspace_bytes_multi(const hyg_sg_model* const* models, int32_t n_models, int32_t n_chains,
                                    int32_t psi_capacity);
size_t hyg_sg_pe_workspace_bytes_multi(const hyg_sg_model* const* models, int32_t n_models,
                                       const hyg_sg_chain* chains, int32_t n_chains, int32_t psi_capacity);

/* hyg_sg_run_chains / hyg_sg_run_chains_pe with chain i run under
 * models[chain_model[i]]: each chain computes the bits it computes alone with
 * its model. `models` and `chain_model` (int32 [n_chains]) are HOST arrays;
 * `emission` is the table of hyg_sg_emission with any of the models (they
 * share it); `workspace` has hyg_sg_[pe_]workspace_bytes_multi bytes. The
 * launch is planned from the shared shape exactly as a single-model launch
 * (LDS layout, chains per batch) and runs the multi-model build of the same
 * kernel; those builds have no phase timers. With estimation chain i starts
 * from its model's theta and reads the lgk / dgk table of its model's kappa;
 * the step sizes are one table per launch, theta_out's rows stay chain after
 * chain. A chain may be as long as its own model's max_duration. Incompatible
 * models (hyg_sg_models_compatible) or an index out of [0, n_models) give
 * HYG_EINVAL before anything is enqueued. n_models = 1 is allowed and gives
 * the bits of the single-model entry. Every model must live on the current
 * device. The descriptor upload goes through models[0]'s staging buffers (see
 * Threading above). */
int hyg_sg_run_chains_multi(const hyg_sg_model* const* models, int32_t n_models, const hyg_sg_chain* chains,
                            const int32_t* chain_model, int32_t n_chains, const double* emission,
                            void* workspace, size_t workspace_bytes, int32_t psi_capacity, double* regime_probs,
                            int32_t* status, void* stream);
int hyg_sg_run_chains_pe_multi(const hyg_sg_model* const* models, int32_t n_models, const hyg_sg_pe_params* pe,
                               const hyg_sg_chain* chains, const int32_t* chain_model, int32_t n_chains,
                               const double* emission, void* workspace, size_t workspace_bytes,
                               int32_t psi_capacity, double* regime_probs, double* theta_out, int32_t* status,
                               void* stream);

/* Host-pointer form of the two above (pe may be NULL: no estimation, theta_out
 * unused): the counts of every chain's sites in one site-major [n_sites][n_samples]
 * array (a genome: the chromosomes one after another), the emission table
 * formed once with models[0], one launch, then host regime_probs
 * [out_rows][K], theta_out [hyg_sg_pe_theta_rows][theta_len] and status
 * [n_chains] (per chain, as hyg_sg_run_chains; the return value is that of the
 * launch). `hygeia estimate_genome` runs through it without torch. */
int hyg_sg_run_chains_host_multi(const hyg_sg_model* const* models, int32_t n_models, const hyg_sg_pe_params* pe,
                                 const uint16_t* meth, const uint16_t* tot, int32_t n_samples, int64_t n_sites,
                                 const hyg_sg_chain* chains, const int32_t* chain_model, int32_t n_chains,
                                 int64_t out_rows, double* regime_probs, double* theta_out, int32_t* status);

/* ---- forward-only launches: log Z, the final particle set, a filter trace
 * The single-group counterpart of hyg_tg_filter_chains / hyg_tg_trace_chains:
 * the SMC of every chain alone, in builds of the chain kernel (template flags
 * FO, TRC) that run one workgroup per chain, with no smoothing partner, no
 * ring and no backward-kernel rows. Every decision of a step (the sorts, the
 * K loop, the systematic draw keyed by (seed, chain_id, t), keep-top) is the
 * full launch's bit for bit, so the particle sets are those behind
 * hyg_sg_run_chains' smoothed probabilities. Per chain the launch returns
 *
 *   log_z             f64 [n_chains]           the SMC estimate of log p(y_0..T-1):
 *                                              the log-sum-exp of the last step's
 *                                              unnormalised log-weights
 *   final_log_weights f64 [n_chains][N_max]    those log-weights, -inf beyond N
 *   final_states      i32 [n_chains][N_max][2] the particles (d, r), -1 beyond N
 *   n_particles       i32 [n_chains]           N
 *   status            i32 [n_chains]           HYG_OK / HYG_ENUMERIC
 *
 * (the last four may be NULL). After HYG_ENUMERIC log_z and every final
 * log-weight are -inf, the states -1 and n_particles 0.
 *
 * The workspace holds the chain descriptors and, for _multi, the model table
 * and the chain -> model indices: no ring, no smoothing slots, nothing that
 * depends on the chains' lengths. 0 for a bad argument. */
size_t hyg_sg_filter_workspace_bytes(const hyg_sg_model* model, int32_t n_chains);
size_t hyg_sg_filter_workspace_bytes_multi(const hyg_sg_model* const* models, int32_t n_models, int32_t n_chains);

/* Conventions as hyg_sg_run_chains[_multi]: `chains`, `models` and
 * `chain_model` are host arrays (out_begin is ignored), the other pointers
 * device pointers; the launch is enqueued on `stream`. Errors as the full
 * entries', all raised before anything is enqueued: HYG_EINVAL for incompatible
 * models, a model index out of range, a chain longer than its model's
 * max_duration or a workspace that is too small ("workspace too small");
 * HYG_EUNSUPPORTED for a layout past the LDS of a CU (resample_type != 2 and
 * num_particles_max > 256 are refused by hyg_sg_model_create); HYG_EDEVICE
 * without a device. Like the full single-group launches they take no part in
 * hyg_tg_last_kernel_ms. */
int hyg_sg_filter_chains(const hyg_sg_model* model, const hyg_sg_chain* chains, int32_t n_chains,
                         const double* emission, void* workspace, size_t workspace_bytes, double* log_z,
                         double* final_log_weights, int32_t* final_states, int32_t* n_particles, int32_t* status,
                         void* stream);
int hyg_sg_filter_chains_multi(const hyg_sg_model* const* models, int32_t n_models, const hyg_sg_chain* chains,
                               const int32_t* chain_model, int32_t n_chains, const double* emission, void* workspace,
                               size_t workspace_bytes, double* log_z, double* final_log_weights,
                               int32_t* final_states, int32_t* n_particles, int32_t* status, void* stream);

/* The filter trace: for a chain of T sites the traced launch also writes row
 * out_begin + t, t in [0, T), of up to three arrays (any pointer may be NULL,
 * not all three). With w_n = hyg_exp(lw_n - log Z_t), the self-normalised
 * weights of step t as the kernel forms them,
 *
 *   log_z_t      f64 [rows]     log Z_t: bit for bit the log_z of the same chain
 *                               (seed, chain id) cut after site t
 *   regime_probs f64 [rows][K]  hyg_u128_to_f64(sum_{n: r_n = r} hyg_fix100(w_n), 100):
 *                               P(r_t = r | y_0..t), the sum the full launch
 *                               stores for the last site of a chain
 *   cp_probs     f64 [rows]     the same sum over d_n = 1:
 *                               P(a segment starts at t | y_0..t)
 *
 * The sums are exact integer sums, so they do not depend on the reduction
 * order; with both probability pointers NULL they are skipped. After
 * HYG_ENUMERIC the rows from the first site whose weights are all -inf hold
 * -inf in log_z_t and NaN in the probabilities. */
typedef struct hyg_sg_trace {
  double* log_z_t;
  double* regime_probs;
  double* cp_probs;
} hyg_sg_trace;

/* hyg_sg_filter_chains[_multi] with a trace: the same workspace and errors;
 * `trace` holds device pointers and chains[i].out_begin is honoured as
 * hyg_sg_run_chains honours it. A NULL trace or one whose three pointers are
 * NULL is HYG_EINVAL. All other outputs are the untraced launch's bit for bit. */
int hyg_sg_trace_chains(const hyg_sg_model* model, const hyg_sg_chain* chains, int32_t n_chains,
                        const double* emission, void* workspace, size_t workspace_bytes, const hyg_sg_trace* trace,
                        double* log_z, double* final_log_weights, int32_t* final_states, int32_t* n_particles,
                        int32_t* status, void* stream);
int hyg_sg_trace_chains_multi(const hyg_sg_model* const* models, int32_t n_models, const hyg_sg_chain* chains,
                              const int32_t* chain_model, int32_t n_chains, const double* emission, void* workspace,
                              size_t workspace_bytes, const hyg_sg_trace* trace, double* log_z,
                              double* final_log_weights, int32_t* final_states, int32_t* n_particles,
                              int32_t* status, void* stream);

/* Host-pointer forms, as hyg_sg_run_chains_host_multi: the counts of every
 * chain's sites in one site-major [n_sites][n_samples] array, the emission
 * table formed once with models[0], one launch, host outputs (`log_z` and
 * `status` required). The trace arrays are host arrays of out_rows rows (any
 * of them NULL, not all three); every chain must have out_begin >= 0 and
 * out_begin + n_sites <= out_rows, else HYG_EINVAL before anything runs. Rows
 * no chain owns are left as they are. */
int hyg_sg_filter_chains_host_multi(const hyg_sg_model* const* models, int32_t n_models, const uint16_t* meth,
                                    const uint16_t* tot, int32_t n_samples, int64_t n_sites,
                                    const hyg_sg_chain* chains, const int32_t* chain_model, int32_t n_chains,
                                    double* log_z, double* final_log_weights, int32_t* final_states,
                                    int32_t* n_particles, int32_t* status);
int hyg_sg_trace_chains_host_multi(const hyg_sg_model* const* models, int32_t n_models, const uint16_t* meth,
                                   const uint16_t* tot, int32_t n_samples, int64_t n_sites,
                                   const hyg_sg_chain* chains, const int32_t* chain_model, int32_t n_chains,
                                   int64_t out_rows, double* log_z_t, double* regime_probs, double* cp_probs,
                                   double* log_z, double* final_log_weights, int32_t* final_states,
                                   int32_t* n_particles, int32_t* status);

/* The instantiation a forward-only / traced launch runs: the chain kernel's
 * name with all seven template arguments (K, threads, PE, PHS, MM, FO, TRC),
 * e.g. "sg_chain_kernel<6,512,false,false,true,true,false>" for a multi-model
 * forward-only launch at K = 6. Returns the bytes needed including the
 * terminator, as hyg_tg_kernel_name. No device needed. */
int32_t hyg_sg_filter_kernel_name(const hyg_sg_model* model, char* buf, int32_t len);
int32_t hyg_sg_filter_kernel_name_multi(const hyg_sg_model* const* models, int32_t n_models, char* buf, int32_t len);
int32_t hyg_sg_trace_kernel_name(const hyg_sg_model* model, char* buf, int32_t len);
int32_t hyg_sg_trace_kernel_name_multi(const hyg_sg_model* const* models, int32_t n_models, char* buf, int32_t len);

/* ---- joint segmentations by backward simulation
 * The marginals above say nothing about where a sample's change points are or
 * how sure each one is; joint draws of the whole path (d_t, r_t), t < T, do.
 * Two stages. hyg_sg_history_chains_multi is hyg_sg_filter_chains_multi that
 * also keeps the particle set of every site (the history builds of the chain
 * kernel, template flag HST); hyg_sg_sample_paths_multi draws n_trajectories
 * paths per chain from a history, any number of times.
 *
 * History row out_begin + t of a chain (12 N_max + 4 bytes per site):
 *
 *   log_weights f64 [rows][N_max]  the unnormalised log-weights lw_n of step t
 *                                  (what final_log_weights holds for the last step)
 *   states      u32 [rows][N_max]  d | r << 24
 *   n_particles i32 [rows]         N_t
 *
 * Entries n >= N_t are not written. After HYG_ENUMERIC the rows from the first
 * site whose weights are all -inf hold n_particles = 0. */
typedef struct hyg_sg_history {
  double* log_weights;
  uint32_t* states;
  int32_t* n_particles;
} hyg_sg_history; /* device pointers */

/* Workspace (hyg_sg_filter_workspace_bytes_multi), conventions and refusals as
 * hyg_sg_trace_chains_multi, in the same order and before anything is
 * enqueued; a NULL history or a NULL pointer in it is HYG_EINVAL.
 * chains[i].out_begin is honoured. Every other output is the untraced
 * launch's bit for bit. n_models = 1 is allowed. */
int hyg_sg_history_chains_multi(const hyg_sg_model* const* models, int32_t n_models, const hyg_sg_chain* chains,
                                const int32_t* chain_model, int32_t n_chains, const double* emission,
                                void* workspace, size_t workspace_bytes, const hyg_sg_history* history,
                                double* log_z, double* final_log_weights, int32_t* final_states,
                                int32_t* n_particles, int32_t* status, void* stream);

/* n_trajectories in [1, 1024] paths per chain, one wave each. A draw from the
 * set of site s with logits l_n, n < N_s: m = max l_n, i_n =
 * hyg_exp_fix100(l_n - m), C_n = i_0 + .. + i_n, uu = (hyg_rand64(seed,
 * chain_id, 6, s, b) >> 11) 2^-53, thr = max(1, ceil(uu C_{N-1})), n* = the
 * smallest n with C_n >= thr (integers only: no dependence on the reduction
 * order). Trajectory b draws its last particle from site T - 1 with l_n =
 * lw_n; a particle (d, r) at site t fixes the sites t - d + 1 .. t, and the
 * particle before the segment is drawn from site s - 1, s = t - d + 1, with
 * l_n = (lw_n + base(d_n, r_n)) + log P[r_n][r].
 *
 * paths int16 [rows][n_trajectories][2] = ((int16)(d & 0xffff), r) at row
 * out_begin + t: hyg_tg_outputs' state layout, durations modulo 2^16 as
 * hyg_cp_* document. forward_status (device [n_chains], NULL = all HYG_OK): a
 * chain whose status is not HYG_OK gets -1 in all its rows and that status in
 * sample_status. sample_status (device [n_chains], may be NULL) is otherwise
 * HYG_OK, or HYG_ENUMERIC when a draw met no finite logit, a sojourn longer
 * than the sites before it or a regime >= K (impossible on a forward's
 * history); the rest of that trajectory is then -1. The chain descriptors go
 * to a stream-ordered side allocation. */
int hyg_sg_sample_paths_multi(const hyg_sg_model* const* models, int32_t n_models, const hyg_sg_chain* chains,
                              const int32_t* chain_model, int32_t n_chains, const hyg_sg_history* history,
                              const int32_t* forward_status, int32_t n_trajectories, int16_t* paths,
                              int32_t* sample_status, void* stream);

/* Host-pointer form of the two: emission table, history and paths on the
 * device, both stages on one stream, then host paths [out_rows][B][2] (rows no
 * chain owns keep the caller's values), log_z and status (the forward's; a
 * chain that is not HYG_OK has -1 in its rows). Every chain must have
 * out_begin >= 0 and out_begin + n_sites <= out_rows. HYG_ENOMEM when the
 * device allocation fails; the message names the bytes asked for. */
int hyg_sg_sample_chains_host_multi(const hyg_sg_model* const* models, int32_t n_models, const uint16_t* meth,
                                    const uint16_t* tot, int32_t n_samples, int64_t n_sites,
                                    const hyg_sg_chain* chains, const int32_t* chain_model, int32_t n_chains,
                                    int32_t n_trajectories, int64_t out_rows, int16_t* paths, double* log_z,
                                    int32_t* status);

/* ================================================ aggregation and DMPs
 * The consumers of the two-group trajectories:
 *   aggregate_results.py:71-206  per-site means over every seed's trajectories
 *                                (split_probs = mean(merged == 0), regimes)
 *   get_dmps.py:46-180           test statistics 1 - #(r_ctrl != r_case) / P
 *                                (and 1 - #(r_ctrl = i, r_case = j) / P), FDR
 *                                and weighted-FDR selection, regime frequencies
 *   multiple_testing.py:3-22     FDR_procedure, weighted_FDR_procedure
 * on trajectories resident in HBM (the outputs of hyg_tg_run_chains). */

/* The job's gather of per-site posterior counts over trajectories and seeds
 * (what aggregate_results.py:129,181 averages; bench.py's step ends with it):
 * for every segment (out_row, site, n_rows) of the device array segments
 * [n_segments][3] int64 and every i < n_rows,
 *   counts[site + i][0]     += round(B * split[out_row + i])
 *   counts[site + i][1 + j] += round(B * regime[out_row + i][j]),  j < 2K,
 * round half to even (torch.round). split / regime are hyg_tg_outputs'
 * split_probs / regime_probs, means over the B trajectories, so B p is an
 * integer. counts [n_sites][1 + 2K] int32 (device) is added to, not cleared.
 * exclusive = 1: the caller guarantees that the call's segments cover disjoint
 * sites (e.g. the chains of one seed), and each count is a plain read-add-write
 * (coalesced; the C3 job's 56 M rows in about 2 ms per seed); exclusive = 0:
 * segments may share sites (several seeds in one call) and every add is an
 * integer atomic (the same sums, about 22 ms for the C3 job). The caller keeps
 * every row and site in range; max_rows (>= every n_rows) sizes the grid.
 * Asynchronous on stream. Replaces a torch gather / round / index_add chain
 * (parallel.posterior_counts, kept as the tests' reference). */
int hyg_tg_posterior_counts(const float* split, const float* regime, int32_t K, int32_t B,
                            const int64_t* segments, int32_t n_segments, int64_t max_rows, int32_t exclusive,
                            int32_t* counts, void* stream);

/* One chromosome segment: the same reported (trimmed) rows in every seed's
 * trajectory block. */
typedef struct hyg_dmp_group {
  int64_t site_begin; /* global site index of the first reported row */
  int64_t n_rows;     /* reported rows */
} hyg_dmp_group;

/* Per-site counts over the P = B * n_seeds trajectories of a site (device
 * pointers; host arrays `groups` [n_groups] and `block_rows`
 * [n_groups][n_seeds] = output row, in merged/control/kase, of the first
 * reported row of each seed's block):
 *   counts [n_sites][2 + 2K] int32 = (#(merged == 0), #(r_ctrl != r_case),
 *                                     #(r_ctrl == r) for r < K, #(r_case == r) for r < K)
 *   pairs  [n_sites][K][K]   int32 = #(r_ctrl == i and r_case == j), or NULL.
 * merged [rows][B], control/kase [rows][B][2] (d, r) int16 as hyg_tg_outputs.
 * Rows of sites outside every group are not written. */
int hyg_dmp_site_counts(const int16_t* merged, const int16_t* control, const int16_t* kase, int32_t B,
                        int32_t K, const hyg_dmp_group* groups, const int64_t* block_rows, int32_t n_groups,
                        int32_t n_seeds, int64_t n_sites, int32_t* counts, int32_t* pairs, void* stream);

/* FDR_procedure(t, fdr_threshold) (multiple_testing.py:3-12) for the
 * statistics t_i = 1 - c_i / P, c_i = counts[i * stride + column] (device),
 * 0 <= c_i <= P: the ascending sort is a counting sort by c (device), the
 * float64 running means np.cumsum(sorted) / (i + 1) are replayed exactly in
 * numpy's sequential order on the host. Outputs the reference's (k, Q_k,
 * threshold): (0, 0, 0) when fdr_threshold < min t; (n, Q_n, 1.01) when every
 * Q_i <= fdr_threshold (the reference's `s == shape` branch). Synchronises. */
int hyg_dmp_fdr(const int32_t* counts, int32_t stride, int32_t column, int64_t n, int32_t n_particles,
                double fdr_threshold, int64_t* k, double* q_k, double* threshold, void* stream);

/* weighted_FDR_procedure(t, fdr_threshold, w_fp, w_fn) (multiple_testing.py:14-22)
 * for the same statistics: ranking computed and sorted on the device (stable
 * LSD radix sort; the reference's np.argsort is not stable, so ties of the
 * ranking keep ascending site order here), Nsums = np.cumsum of the ranked
 * excess error rates replayed exactly on the host. ranked [n] (device,
 * int64) receives ranking_indices; *s the number selected (ranked[0:s]),
 * *n_sum = Nsums[s - 1] (Python indexing: the last sum when s = 0).
 * Synchronises. */
int hyg_dmp_weighted_fdr(const int32_t* counts, int32_t stride, int32_t column, int64_t n, int32_t n_particles,
                         double fdr_threshold, const double* w_fp, const double* w_fn, int64_t* ranked,
                         int64_t* s, double* n_sum, void* stream);

/* ================================================ regions
 * Differentially methylated regions from the joint trajectories (no
 * counterpart in the reference pipeline, which stops at single sites). For a
 * chromosome of n_sites sites and P = B * n_seeds trajectories,
 *   D[t][p] = (r_ctrl[t][p] != r_case[t][p]),  c_t = sum_p D[t][p]
 * (c_t is column 1 of hyg_dmp_site_counts). A seed site has c_t >= min_count;
 * seed sites t, t + 1 are linked iff 0 < positions[t + 1] - positions[t] <=
 * max_gap; a candidate region is a maximal run [begin, end) of linked seed
 * sites with end - begin >= min_sites. Device pointers unless said. */

/* The candidate regions of counts[t * stride + column] (int32) and positions
 * (int64), in ascending order, to regions [capacity][2] int64 (begin, end).
 * *n_regions (host) is always set to the number found; regions == NULL with
 * capacity == 0 only counts; more regions than capacity is HYG_EINVAL and
 * nothing is written. The prefix sums run as separate launches (tile sums, a
 * scan of the sums, apply) without atomics, so the result is the same from run
 * to run. n_sites <= 2^31. Synchronises. */
int hyg_dmr_find_regions(const int32_t* counts, int32_t stride, int32_t column, int64_t n_sites,
                         int32_t min_count, const int64_t* positions, int64_t max_gap, int32_t min_sites,
                         int64_t* regions, int64_t capacity, int64_t* n_regions, void* stream);

/* Per region [a, b) of regions [n_regions][2], with n = b - a and
 * s_p = sum_{t in [a, b)} D[t][p] for trajectory p = seed block * B + b:
 *   region_counts[r][0] = n_all  = #{p : s_p == n}
 *   region_counts[r][1] = n_frac = #{p : s_p * frac_den >= frac_num * n}
 * (0 <= frac_num <= frac_den, 1 <= frac_den <= 1000; compared in int64).
 * control / kase [rows][B][2] (d, r) int16 as hyg_tg_outputs, addressed through
 * the host arrays `groups` (sorted by site, disjoint, inside [0, n_sites)) and
 * `block_rows` [n_groups][n_seeds] as in hyg_dmp_site_counts; a region may run
 * over several groups. A site inside no group counts as not differential for
 * every trajectory and is not read. B * n_seeds <= 16384. Synchronises (the
 * group descriptors are uploaded per call). */
int hyg_dmr_region_counts(const int16_t* control, const int16_t* kase, int32_t B, const hyg_dmp_group* groups,
                          const int64_t* block_rows, int32_t n_groups, int32_t n_seeds, int64_t n_sites,
                          const int64_t* regions, int64_t n_regions, int32_t frac_num, int32_t frac_den,
                          int32_t* region_counts, void* stream);

/* sums[r][c] (int64) = sum over the sites of region r of counts[t][c], for
 * every column of the int32 matrix counts [n_sites][stride], stride <= 4096:
 * from hyg_dmp_site_counts' matrix, sum c_t and the regime histograms of both
 * groups over a region. Asynchronous on stream. */
int hyg_dmr_region_sums(const int32_t* counts, int32_t stride, int64_t n_sites, const int64_t* regions,
                        int64_t n_regions, int64_t* sums, void* stream);

/* ================================================ change points
 * Change points with credible intervals from the joint trajectories (no
 * counterpart in the reference pipeline). Trajectories are in the
 * hyg_tg_outputs layout: merged [rows][B] int16, control / kase [rows][B][2]
 * (d, r) int16, addressed through `groups` (sorted, disjoint site ranges) and
 * `block_rows` [n_groups][n_seeds] exactly as in hyg_dmp_site_counts.
 * Trajectory p = seed block * B + b. A group is one chain's reported rows;
 * trajectories of different groups are independent draws, so the first
 * reported row of a group has no predecessor and no event of any kind. A site
 * inside no group has none either.
 *
 * For a site t that is not its group's first row, compared with row t - 1 of
 * the same seed block, a group's state *continues* when r_t == r_{t-1} and
 * (uint16)d_t == (uint16)(d_{t-1} + 1): the outputs store the 24-bit duration
 * modulo 2^16, so 32767 -> -32768 and -1 -> 0 are continuations, not events.
 * In the packed 32-bit (d, r) word this is one compare:
 *   w_t == (w_{t-1} & 0xffff0000) | ((w_{t-1} + 1) & 0xffff).
 * Event kinds, also the column order of the event matrix:
 *   0 control  the control state does not continue
 *   1 case     the case state does not continue
 *   2 any      kind 0 or kind 1
 *   3 split    merged[t-1] != 0 and merged[t] == 0
 *   4 merge    merged[t-1] == 0 and merged[t] != 0
 * "Does not continue" is wider than "d reset": a merge gives the case group
 * the control's (d + 1, r) without a reset, and a merged state proposing the
 * merge slot sets both durations to 0; both are events of the group whose
 * state jumped.
 *
 * With E[t][p] the indicator of one kind, c_t = sum_p E[t][p]. For a window
 * [a, b): s_p = sum_{t in [a,b)} E[t][p], E_tot = sum_t c_t,
 *   n_any = #{p : s_p >= 1},  n_one = #{p : s_p == 1},
 *   mode  = the smallest t in [a, b) with c_t = max c,
 *   C(t)  = sum_{a <= u <= t} c_u, C(a - 1) = 0,
 *   tail  = level_den - level_num, 0 < level_num <= level_den <= 1000,
 *   lo    = min{t : 2 level_den C(t) > tail E_tot},
 *   hi    = max{t : 2 level_den (E_tot - C(t - 1)) > tail E_tot},
 *   E_tot = 0: mode = lo = a, hi = b - 1.
 * lo, hi and mode are absolute site indices; all comparisons are in int64
 * (2000 * 16384 * 2^31 fits); lo <= hi follows from level_num > 0; at level
 * 1/1 lo and hi are the first and last site of the window that has an event.
 * Windows are found by hyg_dmr_find_regions on the event matrix (stride 5,
 * column = kind, min_sites 1): with min_count >= 1 no window holds a group's
 * first row, so none spans two groups; the entries below are also correct for
 * windows given by the caller that do. Device pointers unless said;
 * B * n_seeds <= 16384. */

/* events [n_sites][5] int32 = c_t of the five kinds. Rows of sites outside
 * every group are not written; a group's first row is written as zeros.
 * merged may be NULL: columns 3 and 4 are then written as 0. One workgroup per
 * 64 sites; its lanes read consecutive words of a seed block's rows, and the
 * row before is the same range one row back. Integer sums only. n_sites <=
 * 2^31. Synchronises (the group descriptors are uploaded per call). */
int hyg_cp_site_events(const int16_t* merged, const int16_t* control, const int16_t* kase, int32_t B,
                       const hyg_dmp_group* groups, const int64_t* block_rows, int32_t n_groups, int32_t n_seeds,
                       int64_t n_sites, int32_t* events, void* stream);

/* counts [n_windows][2] int32 = (n_any, n_one) of the windows [n_windows][2]
 * int64 (begin, end) for one kind in [0, 4]. Kinds 0 to 2 read control / kase
 * only (merged may be NULL), kinds 3 and 4 read merged only (control / kase
 * may be NULL; merged == NULL is HYG_EINVAL). A window's first site that is a
 * group's first row contributes no event; a site in no group is skipped, not
 * read. One workgroup per window, the lane layout of hyg_dmr_region_counts.
 * Synchronises. */
int hyg_cp_window_counts(const int16_t* merged, const int16_t* control, const int16_t* kase, int32_t B,
                         const hyg_dmp_group* groups, const int64_t* block_rows, int32_t n_groups, int32_t n_seeds,
                         int64_t n_sites, int32_t kind, const int64_t* windows, int64_t n_windows, int32_t* counts,
                         void* stream);

/* out [n_windows][4] int64 = (n_events = E_tot, mode, lo, hi) from
 * c_t = events[t * stride + column] (int32, non-negative), usually the event
 * matrix. One workgroup per window; a window longer than the workgroup is
 * walked in chunks of 256 sites with a carried running sum, so no window
 * length is unsupported. Windows are clipped to [0, n_sites). Asynchronous on
 * stream. */
int hyg_cp_window_intervals(const int32_t* events, int32_t stride, int32_t column, int64_t n_sites,
                            const int64_t* windows, int64_t n_windows, int32_t level_num, int32_t level_den,
                            int64_t* out, void* stream);

/* ================================================ transition statistics
 * Sufficient statistics of omega_case, merge_log_prob and split_prob from the
 * joint trajectories (no counterpart in the reference pipeline): under the
 * model's transition law the three settings enter the complete-data likelihood
 * of a path only through these integer counts, so a Monte-Carlo EM step over a
 * launch's draws is one pass over its outputs (hygeia_amd/em.py).
 *
 * Trajectories and their addressing (`groups`, `block_rows`, trajectory p =
 * seed block * B + b) are exactly hyg_cp_site_events'. For every (site t that
 * is not its group's first row, trajectory p), with x = row t - 1 and y = row
 * t, m = (merged != 0), and the durations d_c, d_k read as uint16 of the
 * stored words (a true duration >= 65536 aliases: not handled):
 *
 *   merged trial (case_control_regime_model.py:80-87): if
 *     min(d_c(x), d_k(x)) >= minimum_duration then stats[2 m(x) + m(y)] += 1;
 *   case-hazard trial (the fourth branch of case_control_distributions.py:
 *     246-291): if m(y) == 0 and not (m(x) == 1 and d_c(y) != 1) and not
 *     (m(x) == 0 and r_c(y) == r_k(x)) then, with j = min(d_k(x), dcap),
 *     trials[j] += 1 and, if d_k(y) == 1, events[j] += 1,
 *
 * trials = stats + 4, events = stats + 4 + dcap + 1. The words are classified
 * as they are; nothing assumes the path is legal under the model.
 *
 * stats [4 + 2 (dcap + 1)] int64 (device) is ADDED to: the caller zeroes it,
 * and calls over parts of the groups sum to the call over all of them. One
 * workgroup per 256 sites; LDS int32 bins flushed once per workgroup with
 * 64-bit integer atomic adds, nonzero bins only: integer sums, so equal from
 * run to run. 1 <= dcap <= 4096, minimum_duration >= 0, B * n_seeds <= 16384,
 * n_sites <= 2^31, all three trajectory arrays required; otherwise HYG_EINVAL
 * before the device is touched. Synchronises (the group descriptors are
 * uploaded per call). */
int hyg_tg_transition_stats(const int16_t* merged, const int16_t* control, const int16_t* kase, int32_t B,
                            const hyg_dmp_group* groups, const int64_t* block_rows, int32_t n_groups, int32_t n_seeds,
                            int64_t n_sites, int32_t minimum_duration, int32_t dcap,
                            int64_t* stats /* device, [4 + 2 * (dcap + 1)] */, void* stream);

/* ================================================ regime BED tracks
 * make_bed_file (src/single_group/bin/make_bed_file:19-66)
 * on regime probabilities resident in HBM. */

/* Per site of regime_probs [n_sites][K] f64 (device): score = the largest
 * probability, label = the first regime attaining it, or -1 ("equiprobable")
 * when more than one does (data.table pmax / rowSums(.SD == score) / max.col
 * ties.method "first"). label [n_sites] int8, score [n_sites] f64 (device). */
int hyg_bed_labels(const double* regime_probs, int32_t K, int64_t n_sites, int8_t* label, double* score,
                   void* stream);
/* Host: the BED lines of fwrite(bed, sep = "\t", col.names = FALSE, scipen = 999)
 *   chrom  pos-1  pos+1  name  score  .  pos-1  pos+1  itemRgb
 * for sites already in output order (setkey(bed, chr, start)); names[K + 1]
 * = the regime column names then "equiprobable", rgb[K + 1] likewise; score
 * with at most 15 significant digits, trailing zeros dropped. Writes at most
 * out_bytes bytes; returns the bytes needed (call with out = NULL to size the
 * buffer) or a negative HYG_E* code. */
int64_t hyg_bed_format(const char* chrom, const int64_t* positions, const int8_t* label, const double* score,
                       int64_t n_sites, int32_t K, const char* const* names, const char* const* rgb, char* out,
                       int64_t out_bytes);

/* ================================================ preprocess (BED -> counts)
 * `hygeia preprocess` (src/two_group/preprocess_bed.py), the
 * device part for one sample on one chromosome: the strand collapse
 * (collapse_strands :183-259: "+" rows joined to "-" rows on end == start,
 * missing strand 0, key = start+ or start- - 1, rows with coverage > 0) and its
 * counts on the CpG grid (:298-336: meth = round(total avg / 100), unmeth =
 * round(total (100 - avg) / 100), half away from zero as polars; sites without
 * a collapsed row NaN, the reference's null). Device pointers; each strand's records sorted by start
 * with unique starts (the caller checks); coverage and percent as f64.
 * Writes counts[t * stride + column] = meth, [.. + 1] = unmeth for every site
 * (stride 2: one sample's contiguous [n_sites][2] block, the fastest layout);
 * plus_single_base != 0 promises end = start + 1 for every "+" record (the
 * pairing then needs no marking pass and no scratch); else scratch [n_minus]
 * bytes; *conflicts (device int, caller-zeroed) counts sites
 * that two collapsed rows claim (records longer than one base): a "+" record
 * starting at the site that does not end one base later, and a "-" record
 * starting one base after the site that no "+" record ends at; a site listed
 * twice in cpg_pos0 counts twice. The count is conservative: such a site
 * counts even when one of the two rows has coverage 0 and the reference's
 * coverage filter would have dropped it before its joins. The values written
 * at a counted site are unspecified. */
int hyg_pre_collapse(const int64_t* cpg_pos0, int64_t n_sites, const int64_t* plus_start, const int64_t* plus_end,
                     const double* plus_coverage, const double* plus_percent, int64_t n_plus,
                     const int64_t* minus_start, const double* minus_coverage, const double* minus_percent,
                     int64_t n_minus, int32_t plus_single_base, uint8_t* scratch, double* counts, int32_t stride,
                     int32_t column, int32_t* conflicts, void* stream);

/* Number of visible HIP devices (0 when none: compute calls then fail). */
int hyg_device_count(void);

/* Device policy of concurrent task processes. The reference runs one CPU
 * process per (chrom, batch, seed) task (modules/two_group/4_infer.nf:28,42-48),
 * all at once under Nextflow's local executor (nextflow.config:17-21), and a
 * task never names a device; without a policy every task of an 8-GPU node
 * would land on device 0.
 *
 * hyg_device_slot_acquire takes the first free slot in the order
 * (slot 0 of device 0, 1, ..., n_devices - 1, slot 1 of device 0, ...), a slot
 * being an exclusive flock(2) on `<lock_dir>/hygeia_amd.gpu<d>.slot<j>.lock`
 * held until hyg_device_slot_release or the process exits (a crashed task
 * frees its slot), so concurrent tasks spread evenly over the devices: 16
 * tasks on 8 devices hold two slots each. No HIP call (n_devices is the
 * caller's: tests fake it). HYG_EINVAL when lock_dir is not usable or all
 * max_per_device slots of every device are held; one slot per process (a
 * second call returns the held one). hyg_set_device makes `device` the
 * calling thread's current HIP device (hipSetDevice): models created and
 * chains launched after it use that device. */
int hyg_device_slot_acquire(const char* lock_dir, int32_t n_devices, int32_t max_per_device, int32_t* device,
                            int32_t* slot);
int hyg_device_slot_release(void);
int hyg_set_device(int32_t device);
int hyg_get_device(void);
const char* hyg_last_error(void);
const char* hyg_version(void);

#ifdef __cplusplus
}
#endif
#endif /* HYGEIA_AMD_H */
