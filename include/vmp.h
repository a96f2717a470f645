/*
 * vmp.h — C ABI of libvmp.so, the MI355X-native batched VM placement/migration
 * environment (drop-in for the reference's `VmEnv` gym plugin path).
 *
 * The reference boundary is a Python gymnasium plugin, not an FFI:
 *   register("VmEnv-v1", entry_point="vmenv.envs.env:VmEnv")   vmenv/__init__.py:3-6
 *   env = gym.make("VmEnv-v1", config=Config(**env_cfg))        main.py:47
 * Every entry point below replaces one method of that class (or of the
 * FirstFit/BestFit agents) for N independent env instances at once; the
 * Python layer (vmp/env.py, vmp/batched.py) binds them with ctypes and keeps
 * the reference's reset()/step()/get_invalid_action_mask() surface.
 *
 * Conventions
 *  - All array pointers passed to a handle created on a GPU are DEVICE
 *    pointers (e.g. torch.Tensor.data_ptr() on that device); sizes are in
 *    elements. Layouts are env-major: x[env][...].
 *  - Every call returns 0 on success or a negative VMP_E* code; the message of
 *    the last failure on this thread is vmp_last_error().
 *  - Invalid actions are never errors: they are no-ops reported in `valid`
 *    (env.py:71-72).
 *  - A handle is bound to one HIP stream (vmp_set_stream) and is not
 *    thread-safe; different handles may be used from different threads.
 */
#ifndef VMP_H
#define VMP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VMP_ABI_VERSION 14

#define VMP_OK 0
#define VMP_EINVAL (-1)
#define VMP_EDEVICE (-2)
#define VMP_EOOM (-3)
#define VMP_ESTATE (-4)

/* reward_function (env.py:123-156) */
#define VMP_REWARD_WR 0
#define VMP_REWARD_UT 1
#define VMP_REWARD_KL 2
/* sequence (env.py:211-219) */
#define VMP_SEQ_UNIFORM 0
#define VMP_SEQ_LOWUNIFORM 1
#define VMP_SEQ_HIGHUNIFORM 2
/* eval-mode Record metrics (vmp_record_read): per-env sums, VMP_NREC doubles */
#define VMP_REC_STEPS 0     /* recorded steps */
#define VMP_REC_REWARD 1    /* sum of rewards */
#define VMP_REC_CPU 2       /* sum over steps and PMs of cpu, and of cpu^2 */
#define VMP_REC_CPU2 3
#define VMP_REC_MEM 4       /* same for memory */
#define VMP_REC_MEM2 5
#define VMP_REC_RANK 6      /* sum of _get_rank (PMs hosting >= 1 VM) */
#define VMP_REC_DROP 7      /* sum of dropped / total_requests (0 if none) */
#define VMP_REC_TCM 8       /* sum of target_cpu_mean, target_memory_mean */
#define VMP_REC_TMM 9
#define VMP_REC_WAITING 10  /* sum of waiting_ratio */
#define VMP_REC_LIFE_SUM 11 /* sum of VM lifetimes (record.py vm_lifetime) */
#define VMP_REC_LIVES 12    /* number of VM lives (len(unique_vms_placement)) */
#define VMP_REC_REWARD_OK 13 /* sum and count of rewards > -1e7, count of rewards < -1e7 */
#define VMP_REC_N_OK 14
#define VMP_REC_N_BAD 15
#define VMP_REC_CPUVAR 16   /* sum over steps of var over PMs of cpu, of memory */
#define VMP_REC_MEMVAR 17   /*   (exp_performance.py:109-113, exp_vm_size.py:78-83) */
#define VMP_REC_XMEM 18     /* sum over steps and PMs of mem[e][p] * sum_s mem[s][p] over the
                               handle's envs: their sum over e is the cross-env square
                               exp_performance.py:114 (np.var(memory, axis=0)) needs; 0 when
                               n_env > VMP_REC_XMAX */
#define VMP_NREC 19
#define VMP_REC_XMAX 64
#define VMP_REC_BINS 1001   /* pending / slowdown rates x1000: 0 .. 1000 */
/* per-request outcome log (vmp_reqlog_read): one int32[VMP_RQ_NF] row per request id */
#define VMP_RQ_SLOT 0       /* -2 not observed, -1 dropped, >= 0 the slot it took */
#define VMP_RQ_ARRIVED 1    /* timestep of the step that offered it (dropped ones too) */
#define VMP_RQ_PLACED 2     /* timestep of its first valid placement, 0 = not yet */
#define VMP_RQ_FINISHED 3   /* timestep of the step whose _run_vms finished it, 0 = not yet */
#define VMP_RQ_SUSPENDS 4   /* valid suspend actions on it */
#define VMP_RQ_WAIT_STEPS 5 /* steps that left it at WAIT, the arrival step included */
#define VMP_RQ_NF 6
/* ... and its per-env meta, int64[VMP_RQ_NMETA] */
#define VMP_RQ_FIRST 0      /* total_requests when the env's log started */
#define VMP_RQ_NEXT 1       /* total_requests now: the ids observed are [FIRST, NEXT) */
#define VMP_RQ_LOST 2       /* requests whose id was >= capacity: not logged */
#define VMP_RQ_NMETA 3
/* per-step time series (vmp_series_read): one f64[VMP_SR_NF] row per window of `stride` steps.
 * Fields 1..12 are sums over the window's steps (divide by STEPS for the window mean), fields
 * 13..18 the env's int64 counters after the window's last step, stored as f64: exact below 2^53 */
#define VMP_SR_STEPS 0            /* steps folded into the row; 0 = never written */
#define VMP_SR_REWARD 1           /* the step's reward */
#define VMP_SR_WAITING_RATIO 2    /* waiting_ratio (VMP_ST_WAITING_RATIO) */
#define VMP_SR_CPU_SUM 3          /* np.sum(cpu) over the PMs, numpy's pairwise order */
#define VMP_SR_MEM_SUM 4          /* np.sum(memory) */
#define VMP_SR_CPU_VAR 5          /* np.var(cpu): two-pass, the mean from the pairwise sum */
#define VMP_SR_MEM_VAR 6          /* np.var(memory) */
#define VMP_SR_TARGET_CPU_MEAN 7  /* env.py:116-121 with cap_target_util applied */
#define VMP_SR_TARGET_MEM_MEAN 8
#define VMP_SR_USED_PM 9          /* _get_rank: PMs hosting at least one VM */
#define VMP_SR_EMPTY_PM 10        /* P - count_nonzero(cpu): base.py:134's `used_pm` */
#define VMP_SR_WAITING 11         /* slots with placement == WAIT */
#define VMP_SR_RUNNING 12         /* slots with placement < P */
#define VMP_SR_TIMESTEP 13        /* ... and the counters, as vmp_get_counters returns them */
#define VMP_SR_TOTAL_REQUESTS 14
#define VMP_SR_SERVED 15
#define VMP_SR_SUSPEND 16
#define VMP_SR_PLACE 17
#define VMP_SR_DROPPED 18
#define VMP_SR_NF 19
/* ... and its per-env meta, int64[VMP_SR_NMETA] */
#define VMP_SR_FIRST 0      /* the env's timestep when its series started */
#define VMP_SR_COUNT 1      /* steps observed since then: the next step folds into row COUNT / stride */
#define VMP_SR_LOST 2       /* steps whose row index was >= capacity: counted, not stored */
#define VMP_SR_NMETA 3
/* actor-head modes (vmp_policy_head) */
#define VMP_HEAD_SAMPLE 0 /* Network.get_action(obs, action=None, mask) (ppo.py:115-126) */
#define VMP_HEAD_GIVEN 1  /* Network.get_action(obs, action, mask): log_prob/entropy only */
#define VMP_HEAD_ARGMAX 2 /* Network.get_det_action (ppo.py:128-131): unmasked argmax */
#define VMP_HEAD_MAX_A 1024 /* action_dim limit of the register-resident row */
#define VMP_ACTOR_HEAD_MAX_A 128 /* action_dim limit of the fused GEMM + head (vmp_actor_head) */
/* heuristic policies (src/agents/firstfit.py:21-38, bestfit.py:21-40) */
#define VMP_POLICY_FIRSTFIT 0
#define VMP_POLICY_BESTFIT 1

/* Mirrors vmenv/envs/config.py:4-15 field for field. */
typedef struct vmp_config {
  double arrival_rate;      /* Poisson lambda per step */
  double service_length;    /* Poisson mean; runtime = poisson(L) + 1 */
  int32_t pms;              /* P */
  int32_t vms;              /* V (slots) */
  int64_t training_steps;
  int64_t eval_steps;
  int64_t seed;
  int32_t reward_function;  /* VMP_REWARD_* */
  int32_t sequence;         /* VMP_SEQ_* */
  int32_t cap_target_util;  /* bool */
  int32_t allow_null_action;/* bool: A = P+2 if true else P+1 (env.py:26) */
  double beta;
} vmp_config;

/* Per-env counters, vmp_get_counters() row layout (env.py:196-205, 299-318). */
#define VMP_CTR_TOTAL_REQUESTS 0
#define VMP_CTR_SERVED 1
#define VMP_CTR_SUSPEND 2
#define VMP_CTR_PLACE 3
#define VMP_CTR_DROPPED 4
#define VMP_CTR_TIMESTEP 5
#define VMP_NCTR 6
/* Per-env float stats, vmp_get_stats() row layout. */
#define VMP_ST_WAITING_RATIO 0
#define VMP_ST_TARGET_CPU_MEAN 1
#define VMP_ST_TARGET_MEM_MEAN 2
#define VMP_ST_TOTAL_CPU_REQ 3
#define VMP_ST_TOTAL_MEM_REQ 4
#define VMP_NST 5

typedef struct vmp_handle vmp_handle;

int vmp_abi_version(void);
const char *vmp_last_error(void);

/* VmEnv.__init__ (env.py:23-33) for n_env instances on HIP device `device`.
 * Every env is reset with seeds[i] (host array, n_env entries), i.e.
 * reset(seed=seeds[i]) -> four numpy PCG64 streams seeded seeds[i]+k
 * (env.py:172-178). eval_mode starts false (env.py:25). */
int vmp_create(const vmp_config *cfg, int32_t n_env, const int64_t *seeds, int32_t device,
               vmp_handle **out);
int vmp_destroy(vmp_handle *h);
int vmp_set_stream(vmp_handle *h, void *hip_stream);
/* VmEnv.eval (env.py:105-106). */
int vmp_set_eval(vmp_handle *h, int32_t eval_mode);
/* Shape helpers: A = action_dim (env.py:26), D = obs dim (env.py:27). */
int vmp_dims(const vmp_handle *h, int32_t *n_env, int32_t *P, int32_t *V, int32_t *A,
             int32_t *D);

/* Per-env workload: env i draws arrivals ~ Poisson(arrival_rate[i]) (env.py:272) and planned
 * runtimes ~ Poisson(service_length[i]) + 1 (env.py:289) from its next step on. HOST arrays of
 * n_env doubles; either may be NULL = keep that quantity as it is. Values must be finite and
 * >= 0 (VMP_EINVAL otherwise); on any failure the handle keeps its previous workload and stays
 * usable. Env i then behaves bit for bit as a handle created with its pair in the config: the
 * state, the RNG streams and the step hints are untouched, only the Poisson constants the
 * step kernels read change (the three samplers, lam == 0 / < 10 / >= 10, may be mixed within
 * one launch). Stream-ordered behind the launches already queued on the handle's stream; the
 * call synchronises that stream before it returns, so it must not be made while the stream
 * is capturing.
 * Graphs: the first call moves the kernels' constants from the handle's single pair to a
 * per-env array, so a graph captured BEFORE the first vmp_set_workload keeps reading the
 * config's values and must be recaptured. Later calls rewrite that array in place: graphs
 * captured after the first call stay valid across them and replay with the new values.
 * (ABI 12) */
int vmp_set_workload(vmp_handle *h, const double *arrival_rate, const double *service_length);
/* Current per-env values (the config's for a handle never given a workload); HOST arrays, nullable. */
int vmp_get_workload(const vmp_handle *h, double *arrival_rate, double *service_length);

/* Trace-driven workload: envs replay the caller's requests instead of drawing them.
 * A trace is `steps` steps of requests: offs int64[steps + 1] (offs[0] = 0, non-decreasing,
 * offs[steps] < 2^31) and per request cpu, mem (hundredths, 1..100) and runtime (1..2^30).
 * The requests of step index s are [offs[s], offs[s+1]), in order. On a traced env the step
 * run at timestep s + 1 (reset leaves timestep 1) runs _accept_vm_requests (env.py:271-293)
 * with a = offs[s+1] - offs[s] arrivals (0 from step `steps` on): the k = min(a, #NULL) lowest
 * NULL slots take the step's first k requests in order (vm_cpu = cpu/100, vm_mem = mem/100,
 * planned = remaining = runtime), total_requests += a, dropped += a - k. A DROPPED REQUEST IS
 * CONSUMED: it is never offered again and the next step starts at offs[s+1]. (The draw-based
 * env draws sizes and runtimes per accepted VM, so there a drop consumes no draw; this is the
 * one deliberate difference, and what makes the request sequence independent of the policy.)
 * RNG streams 1-4 are neither read nor advanced; everything else of the step is unchanged.
 * vmp_reset rewinds an env to step 0 of its trace (its seeds still reseed the idle streams).
 *
 * vmp_set_trace: HOST arrays, copied by the call. trace_of_env int32[n_env] maps each env to
 * a trace (NULL: every env replays trace 0). Null pointers, offs[0] != 0, a decreasing offs,
 * a size of 0 or above 100, a runtime of 0 or above 2^30 and a map entry out of range return
 * VMP_EINVAL, a failed device allocation VMP_EOOM; both leave the handle exactly as it was,
 * usable with its previous trace or its RNG workload. Stream-ordered behind the launches
 * already queued; synchronises the stream, so it must not be made during capture. A handle
 * with a per-env workload may be given a trace: the workload is dormant until
 * vmp_clear_trace. On a traced handle vmp_set_workload returns VMP_ESTATE.
 * Graphs: the first vmp_set_trace (and vmp_clear_trace) switches the handle's step kernels,
 * so graphs captured before it must be recaptured. Later calls rewrite the device-side
 * descriptor table in place: a graph captured on a traced handle stays valid across them and
 * replays the new traces.
 * Snapshots of a traced handle carry a flag and a 64-bit hash of (traces, map); vmp_restore
 * needs the same hash on the target and refuses traced into plain and the reverse
 * (VMP_EINVAL). The snapshot size does not change. (ABI 13) */
typedef struct vmp_trace {
  int64_t steps;
  const int64_t *offs;     /* [steps + 1] */
  const uint8_t *cpu;      /* [offs[steps]] */
  const uint8_t *mem;      /* [offs[steps]] */
  const uint32_t *runtime; /* [offs[steps]] */
} vmp_trace;
int vmp_set_trace(vmp_handle *h, int32_t n_traces, const vmp_trace *traces,
                  const int32_t *trace_of_env);
/* Back to the RNG workload (per-env if the handle had one), the streams where they stood. */
int vmp_clear_trace(vmp_handle *h);
/* n_traces (0: no trace); then, all HOST and nullable: trace_of_env int32[n_env],
 * steps / requests int64[n_traces] of every trace. */
int vmp_trace_info(const vmp_handle *h, int32_t *n_traces, int32_t *trace_of_env, int64_t *steps,
                   int64_t *requests);

/* VmEnv.reset (env.py:180-226) for the envs whose env_mask byte is non-zero
 * (env_mask may be NULL = all). seeds: device int64[n_env] or NULL; a NULL
 * seeds array is reset(seed=None): streams continue and the VM-size
 * sequences restart 2*max(training_steps, eval_steps) draws further
 * (env.py:181-182, 211-219). obs (nullable): device f32[n_env][D]. */
int vmp_reset(vmp_handle *h, const int64_t *seeds, const uint8_t *env_mask, float *obs);

/* VmEnv.step (env.py:66-103) for every env.
 *  actions: device int32[n_env][V]
 *  obs:     device f32[n_env][D]  (nullable)     env.py:295-296
 *  reward:  device f64[n_env]     (nullable)     env.py:123-156
 *  done:    device u8[n_env]      (nullable)     env.py:160-163
 *  valid:   device u8[n_env][V]   (nullable)     env.py:68-72 */
int vmp_step(vmp_handle *h, const int32_t *actions, float *obs, double *reward,
             uint8_t *done, uint8_t *valid);
/* vmp_step that also writes the invalid-action mask of the state it leaves
 * (get_invalid_action_mask, env.py:45-53, as vmp_mask lays it out) into
 * next_mask_bits (nullable): the mask the next PPOAgent.act reads
 * (ppo.py:151-153), without a separate vmp_mask launch per step. (ABI 11) */
int vmp_step_mask(vmp_handle *h, const int32_t *actions, float *obs, double *reward,
                  uint8_t *done, uint8_t *valid, uint32_t *next_mask_bits);

/* FirstFitAgent.act / BestFitAgent.act (firstfit.py:21-38, bestfit.py:21-40)
 * on the current observation of every env -> device int32[n_env][V]. */
int vmp_heuristic_act(vmp_handle *h, int32_t policy, int32_t *actions);

/* The same agents on a CALLER's observation, device f32[n_env][3V+2P]
 * (firstfit.py:21-38 / bestfit.py:21-40 read only the obs they are passed,
 * utils.py:37-47): f32 fit tests on the obs values, FirstFit updating cpu
 * only, BestFit in flip(argsort(cpu+memory)) order with numpy's scalar
 * introsort ties; no env state is read. -> device int32[n_env][V]. P <= 3583. */
int vmp_heuristic_act_obs(vmp_handle *h, int32_t policy, const float *obs, int32_t *actions);

/* act + step fused in one launch: the action the heuristic takes on the
 * pre-step observation is applied by step() in the same kernel (the
 * Base.test loop body, base.py:71-86). actions_out (nullable) receives it. */
int vmp_heuristic_step(vmp_handle *h, int32_t policy, int32_t *actions_out, float *obs,
                       double *reward, uint8_t *done, uint8_t *valid);

/* K fused heuristic steps per env in one launch, state resident on chip.
 * rewards: device f64[k_steps][n_env] (nullable); done_count: device
 * int64[n_env] (nullable) accumulates the steps whose `terminated` was true. */
int vmp_rollout_heuristic(vmp_handle *h, int32_t policy, int32_t k_steps, double *rewards,
                          int64_t *done_count);

/* VmEnv.get_invalid_action_mask(masked=True) (env.py:45-53), bit-packed:
 * device u32[n_env][V][W], W = ceil(A/32); bit a of row v set = invalid. */
int vmp_mask(vmp_handle *h, uint32_t *bits);
/* Same mask expanded to the reference's bool layout: device u8[n_env][V][A]. */
int vmp_mask_bool(vmp_handle *h, uint8_t *mask);

/* Observation of the current state (env.py:295-296): device f32[n_env][D]. */
int vmp_get_obs(vmp_handle *h, float *obs);
/* Counters (VMP_CTR_*): device int64[n_env][VMP_NCTR]. */
int vmp_get_counters(vmp_handle *h, int64_t *counters);
/* Stats (VMP_ST_*): device f64[n_env][VMP_NST]. */
int vmp_get_stats(vmp_handle *h, double *stats);
/* Full reference-dtype state (info / parity): device arrays, each nullable.
 * placement, remaining: int64[n_env][V]; vm_cpu, vm_mem: f64[n_env][V];
 * cpu, mem: f64[n_env][P]. */
int vmp_get_state(vmp_handle *h, int64_t *placement, double *vm_cpu, double *vm_mem,
                  double *cpu, double *mem, int64_t *remaining);
/* _get_rank (env.py:320-325) = number of PMs hosting >= 1 VM: int64[n_env]. */
int vmp_get_rank(vmp_handle *h, int64_t *rank);

/* Checkpoint / resume of the batched env state (the reference only
 * saves the policy weights, ppo.py:163-170). vmp_snapshot copies everything a
 * later reset/step reads — the four PCG64 streams and sequence bases, counters,
 * step hints, PM resources and VM words with their finish keys — into a
 * device buffer of vmp_snapshot_bytes() bytes (16-byte aligned); vmp_restore
 * writes it into a handle of the same env count and config (the config's seed
 * field may differ), which then continues bit-exactly where the snapshotted
 * handle stood. Stream-ordered on the handle's stream (vmp_snapshot returns
 * after the copy; vmp_restore synchronises the stream once to check the
 * snapshot's descriptor). Not included: eval mode (vmp_set_eval) and the
 * Record recorder (re-enable it after a restore, as after a reset).
 * A handle given a per-env workload (vmp_set_workload) appends it to its
 * snapshots (16 * n_env bytes more, counted by vmp_snapshot_bytes);
 * vmp_restore then needs a handle whose current workload is bitwise the same,
 * and refuses (VMP_EINVAL) a snapshot with a workload on a handle without one
 * and the reverse. Handles never given one keep the earlier layout and size. */
int vmp_snapshot_bytes(const vmp_handle *h, int64_t *bytes);
int vmp_snapshot(vmp_handle *h, void *dst);
int vmp_restore(vmp_handle *h, const void *src);

/* Branch env states between handles on the device: "what would happen from THIS state if ...".
 * For every dst env i with 0 <= src_of_dst[i] < src.n_env, dst env i receives the complete state
 * of that src env: its header (streams, sequence bases, timestep, counters, stats and the step
 * hint word, verbatim: the hints describe the state they travel with), its PM row and its whole
 * VM row, the padded words behind slot V included, so the env's rows of a vmp_snapshot are equal
 * byte for byte. -1, and any other value outside the range, keeps dst env i untouched; such a
 * value is never used as an index (the map lives on the device: the host does not see it).
 *  src_of_dst: device int32[dst.n_env]
 *  seeds:      device int64[dst.n_env], nullable. Where seeds[i] >= 0 on a copied env, its four
 *              streams become what vmp_reset writes for reset(seed = seeds[i]) (stream k = PCG64
 *              of seeds[i] + k, the sequence bases the fresh states of streams 1 and 2) and
 *              everything else stays the copied state; seeds[i] < 0 keeps the copied streams.
 * Not copied: eval mode, the per-env workload, the trace and its map, the launch-order flags
 * (stale flags cost speed only). A dst env continues under dst's own workload or trace at the
 * copied timestep. The env counts may differ.
 * VMP_EINVAL: a null handle or map; handles of different pms, vms or action count, of configs
 * that differ in anything but the seed (the check of vmp_restore), or on different devices.
 * VMP_ESTATE: one handle has a trace and the other has none. Both handles stay usable.
 * dst == src is allowed and correct for any map (overlaps, swaps, one env to all): the call then
 * reads a staging copy owned by the handle, allocated on the first such call (VMP_EOOM if that
 * fails, the handle unchanged) and freed by vmp_destroy.
 * Stream-ordered on dst's stream; ordering against work queued on src's stream is the caller's
 * job (the Python layer binds both to one stream). With dst != src the call allocates nothing
 * and never synchronises, so it may be captured in a graph; the map and seeds are read on the
 * device at replay. The one exception: on a dst with the recorder, the request log or the time
 * series on, the first call allocates an n_env-byte mask, so make one call before capturing.
 * Those observers restart for exactly the overwritten dst envs, from the new state, as after
 * vmp_reset with their mask; the observers of kept envs continue. (ABI 14, additive) */
int vmp_branch(vmp_handle *dst, vmp_handle *src, const int32_t *src_of_dst, const int64_t *seeds);

/* Set env states from the caller's arrays on the device: the inverse of vmp_get_state /
 * vmp_get_counters. All pointers are DEVICE pointers, in those calls' shapes and dtypes:
 *  env_mask   u8[n_env], nullable = every env; a zero byte keeps the env
 *  placement, remaining  int64[n_env][V]; vm_cpu, vm_mem f64[n_env][V]       (required)
 *  cpu, mem   f64[n_env][P], both given or both NULL
 *  counters   int64[n_env][VMP_NCTR] (VMP_CTR_*, the timestep included), nullable = kept
 *  totals     f64[n_env][2]: VMP_ST_TOTAL_CPU_REQ, VMP_ST_TOTAL_MEM_REQ, nullable = kept
 *  seeds      int64[n_env], nullable; seeds[e] >= 0 gives env e the four streams and sequence
 *             bases of reset(seed = seeds[e]), seeds[e] < 0 keeps its streams
 *  status     u8[n_env], nullable: a VMP_SS_* code per env
 * A selected env is validated as a whole on the device. If every rule holds, all of it is
 * written (status VMP_SS_IMPORTED); otherwise NOTHING of it is written and status names the
 * lowest-numbered failing rule. P = pms: placement P is WAIT, P + 1 is NULL (an empty slot).
 *  VMP_SS_PLACEMENT   a placement outside [0, P + 1]
 *  VMP_SS_NULL_SLOT   a NULL slot whose sizes or remaining are not 0
 *  VMP_SS_VM_SIZE     an existing VM whose size is not bitwise (double)k / 100.0, k in 1..100
 *  VMP_SS_RUNTIME     an existing VM whose remaining is outside [1, 2^30]
 *  VMP_SS_TIMESTEP    the timestep (counters' if given, else the env's own) outside [1, 2^31)
 *  VMP_SS_COUNTER     one of the other five counters negative
 *  VMP_SS_CAPACITY    a PM whose running VMs sum to more than 100 hundredths of cpu or memory
 *  VMP_SS_LOAD_FLOOR  a given load x that is neither 0 nor >= 1e-7 (NaN included)
 *  VMP_SS_LOAD_MAX    a given load above 1.0
 *  VMP_SS_LOAD_SUM    a given load with |x - sum k / 100| >= 1e-7 (env.py:267's threshold)
 * Written: the VM words of slots 0..V-1 (a running VM's time word is its finish key timestep +
 * remaining; the words behind slot V stay); the PM row: the given loads verbatim (they carry a
 * run's rounding history), else (double)(sum of k) / 100.0 per PM, which does not depend on any
 * order; the six counters and the two totals where given; waiting_ratio = #waiting / #existing
 * (0 without a VM, env.py:112-115); the step hint word as 0 (the next step takes the general
 * path); the streams where seeds say so. The target means are derived by vmp_get_stats and by
 * the steps that need them. Not touched: eval mode, the per-env workload, the trace and its map
 * (a traced env continues on its own trace at the imported timestep), the launch-order flags.
 * VMP_EINVAL, the handle unchanged: a null handle, a missing required array, exactly one of
 * cpu / mem, or more PMs than the kernel's per-PM sums hold in LDS (8190).
 * Stream-ordered on the handle's stream; allocates nothing and never synchronises, so it may be
 * captured in a graph and replayed with rewritten arrays. The one exception, as in vmp_branch:
 * with the recorder, the request log or the time series on, the first call allocates an
 * n_env-byte mask, so make one call before capturing. Those observers restart for exactly the
 * imported envs; refused and unselected envs keep theirs. (ABI 14, additive) */
#define VMP_SS_SKIPPED 0
#define VMP_SS_IMPORTED 1
#define VMP_SS_PLACEMENT 2
#define VMP_SS_NULL_SLOT 3
#define VMP_SS_VM_SIZE 4
#define VMP_SS_RUNTIME 5
#define VMP_SS_TIMESTEP 6
#define VMP_SS_COUNTER 7
#define VMP_SS_CAPACITY 8
#define VMP_SS_LOAD_FLOOR 9
#define VMP_SS_LOAD_MAX 10
#define VMP_SS_LOAD_SUM 11
int vmp_set_state(vmp_handle *h, const uint8_t *env_mask,
                  const int64_t *placement, const double *vm_cpu, const double *vm_mem,
                  const int64_t *remaining,
                  const double *cpu, const double *mem,
                  const int64_t *counters, const double *totals,
                  const int64_t *seeds, uint8_t *status);

/* PPOAgent.update GAE (ppo.py:232-243) over T steps x N envs, reverse scan:
 *  delta = r + (1-d)*gamma*v' - v;  g = delta + (1-d)*gamma*lambda*g.
 * All device f32 [T][N] (done as f32 0/1); adv and ret are outputs. */
int vmp_gae(int32_t T, int32_t N, const float *reward, const float *done, const float *value,
            const float *next_value, float gamma, float lam, float *adv, float *ret,
            void *hip_stream);

/* Network.get_action head (ppo.py:115-126) on the actor's logits f32[B][V*A]
 * (row-major, as nn.Linear writes them): rows flagged in mask_bits u32[B][V][W]
 * (W = ceil(A/32), nullable = get_action(..., invalid_mask=None)) are set to
 * -1e7 as ppo.py:119 does, then per (b, v) a Categorical over A.
 *  - VMP_HEAD_SAMPLE: action[b][v] drawn (inverse CDF, counter-based uniforms
 *    from (seed, offset + b*V + v)); VMP_HEAD_GIVEN: action read.
 *    logprob[b] = sum_v log p(action), entropy[b] = sum_v H (ppo.py:123-126),
 *    both nullable.
 *  - VMP_HEAD_ARGMAX: get_det_action (ppo.py:128-131), argmax of the unmasked
 *    row, first index on ties; logprob/entropy untouched.
 *  - rng_counter (nullable): a device u64 whose current value is mixed into the
 *    seed, so a captured graph that advances it between replays draws fresh
 *    actions; workspace (nullable): 2*B*V floats of row scratch (else the call
 *    allocates stream-ordered memory, which graph capture may not support).
 *  - wait_ratio >= 0 applies PPOAgent.act's WAIT coin flips first (ppo.py:154-156):
 *    a row with > 1 invalid entries whose column wait_index (= P) is valid
 *    gets it forbidden when a uniform draw exceeds wait_ratio
 *    (migration_ratio). wait_ratio < 0: no flips (PPOAgent.learn, ppo.py:197).
 * Replaces the torch Categorical / multinomial calls of ppo.py:117-126.
 * All pointers are device pointers; A <= VMP_HEAD_MAX_A. */
int vmp_policy_head(int32_t B, int32_t V, int32_t A, int32_t mode, const float *logits,
                    const uint32_t *mask_bits, float wait_ratio, int32_t wait_index,
                    uint64_t seed, uint64_t offset, const uint64_t *rng_counter, int32_t *action,
                    float *logprob, float *entropy, float *workspace, void *hip_stream);

/* Backward of vmp_policy_head (VMP_HEAD_SAMPLE/GIVEN, no coin flips) for the
 * PPO loss (ppo.py:258-277): given dL/dlogprob[B] and dL/dentropy[B]
 * (nullable = 0), writes dL/dlogits f32[B][V*A]; masked entries get 0 (the
 * in-place mask assignment of ppo.py:119 passes no gradient). dlogits may
 * alias logits (the rows are read before they are written). */
int vmp_policy_head_backward(int32_t B, int32_t V, int32_t A, const float *logits,
                             const uint32_t *mask_bits, const int32_t *action,
                             const float *g_logprob, const float *g_entropy, float *dlogits,
                             void *hip_stream);

/* vmp_policy_head_backward with bf16 dlogits (round to nearest even), for the
 * bf16-GEMM training leg whose dW / dh GEMMs take bf16 inputs: the cast pass
 * over the [B, V*A] gradient is folded into the head's store. Tiled path only:
 * A <= 128, logits 16-byte and dlogits 8-byte aligned; dlogits must not alias
 * logits. Not a parity path (the reference trains in f32). */
int vmp_policy_head_backward_bf16(int32_t B, int32_t V, int32_t A, const float *logits,
                                  const uint32_t *mask_bits, const int32_t *action,
                                  const float *g_logprob, const float *g_entropy,
                                  uint16_t *dlogits_bf16, void *hip_stream);

/* The actor's last Linear fused with the head above (ppo.py:115-131, SURVEY
 * §8(f)1): logits = h W^T + bias (h f32[B][K], weight f32[V*A][K] as nn.Linear
 * stores it, bias f32[V*A]) computed on the f32 matrix cores and consumed by
 * the head inside the same workgroup, so the [B, V*A] logits are never written
 * unless logits_out (nullable, f32[B][V*A]) asks for them (the training
 * forward keeps them for vmp_policy_head_backward). Modes, mask, coin flips,
 * rng and outputs as vmp_policy_head (the same per-row uniforms: equal logits
 * draw equal actions). Needs K % 32 == 0, A <= VMP_ACTOR_HEAD_MAX_A and
 * 16-byte aligned h / weight. */
int vmp_actor_head(int32_t B, int32_t K, int32_t V, int32_t A, int32_t mode, const float *h,
                   const float *weight, const float *bias, const uint32_t *mask_bits,
                   float wait_ratio, int32_t wait_index, uint64_t seed, uint64_t offset,
                   const uint64_t *rng_counter, int32_t *action, float *logprob, float *entropy,
                   float *logits_out, float *workspace, void *hip_stream);

/* The actor MLP forward (ppo.py:98-109: Linear(D, H), Tanh, Linear(H, H),
 * Tanh, Linear(H, N)) in f32 for rollouts and eval, one launch: x f32[B][D]
 * (the observations), b1, b2 f32[H] and b3 f32[N] the biases, `packed` the
 * three weight matrices (nn.Linear's w1 f32[H][D], w2 f32[H][H], w3 f32[N][H])
 * in the kernel's MFMA-fragment order, written by vmp_actor_mlp_pack into
 * vmp_actor_mlp_packed_floats(D, H, N, layers) floats (16-byte aligned); the
 * caller re-packs whenever a weight changes. layers = 3: out = the logits
 * f32[B][N]; layers = 2: out = self.actor[:-1](x), the last hidden layer
 * after its Tanh, f32[B][H] (the big heads of config/100.yml go on to
 * vmp_actor_head; w3 / b3 unused). 16 rows per workgroup on the f32 matrix
 * cores, activations kept in LDS between layers. Needs H % 32 == 0, H <= 512,
 * N <= 512, D <= VMP_ACTOR_MLP_MAX_D. Forward only (no autograd). (ABI 11) */
#define VMP_ACTOR_MLP_MAX_D 1536
int64_t vmp_actor_mlp_packed_floats(int32_t D, int32_t H, int32_t N, int32_t layers);
int vmp_actor_mlp_pack(int32_t D, int32_t H, int32_t N, int32_t layers, const float *w1,
                       const float *w2, const float *w3, float *packed, void *hip_stream);
int vmp_actor_mlp_f32(int32_t B, int32_t D, int32_t H, int32_t N, int32_t layers, const float *x,
                      const float *packed, const float *b1, const float *b2, const float *b3,
                      float *out, void *hip_stream);
/* The same MLP with the masked head of vmp_policy_head on its logits in one
 * launch (ppo.py:98-131 Network.get_action / get_det_action with the
 * PPOAgent.act WAIT coin, ppo.py:151-156): N = V * A <= 512, A <= 128; modes,
 * mask bits, coin, rng stream and outputs exactly as vmp_policy_head (the
 * per-row code is shared, so equal logits draw equal actions and give equal
 * logprob / entropy, bit for bit); logits_out (nullable, f32[B][V*A]) keeps a
 * copy of the logits. The logits otherwise never leave the workgroup: one
 * launch per batched step of the eval loop (base.py:71-86). advance_counter
 * (with rng_counter u64[2]): the launch itself adds 1 to rng_counter[0] once
 * every workgroup has read it (rng_counter[1] is the arrival ticket, 0
 * between launches), instead of a separate increment launch. (ABI 11) */
int vmp_actor_mlp_head_f32(int32_t B, int32_t D, int32_t H, int32_t V, int32_t A, int32_t mode,
                           const float *x, const float *packed, const float *b1, const float *b2,
                           const float *b3, const uint32_t *mask_bits, float wait_ratio,
                           int32_t wait_index, uint64_t seed, uint64_t offset,
                           const uint64_t *rng_counter, int32_t advance_counter,
                           int32_t *action, float *logprob, float *entropy, float *logits_out,
                           void *hip_stream);

/* Training side of the fused actor head in bf16: the update's
 * get_action(obs, action, mask) (ppo.py:115-126, called at ppo.py:258) and its
 * backward, for the bf16 training leg (not the parity path: the reference
 * trains in f32). h bf16[B][K] (the actor's last hidden layer rounded to
 * bf16), weight bf16[V*A][K], bias f32[V*A], mask_bits as vmp_policy_head
 * (nullable), action i32[B][V] (GIVEN). Needs K % 64 == 0, A <= 128, 16-byte
 * aligned h / weight / mask_bits (a row's mask words are read as one vector)
 * and, for the backward, 4-byte aligned dlogits (stored as bf16 pairs).
 * Forward: logprob / entropy f32[B] of the given actions; logits formed tile
 * by tile on the bf16 matrix cores (f32 accumulate) and consumed in
 * registers, never written. workspace: nullable, 2*B*V floats. */
int vmp_actor_head_bf16_fwd(int32_t B, int32_t K, int32_t V, int32_t A, const uint16_t *h,
                            const uint16_t *weight, const float *bias, const uint32_t *mask_bits,
                            const int32_t *action, float *logprob, float *entropy,
                            float *workspace, void *hip_stream);
/* Rollout sampling on the same kernel (the bf16 leg's collect: get_action(obs,
 * mask) ppo.py:115-126 and PPOAgent.act's WAIT coin ppo.py:151-156, as
 * vmp_policy_head / vmp_actor_head in VMP_HEAD_SAMPLE mode): action
 * i32[B][V] is the OUTPUT, drawn per (sample, VM row) by inverse CDF over
 * the masked softmax in action order with the counter-based uniform of
 * vmp_policy_head's stream (seed, offset + b*V + v; rng_counter nullable,
 * mixed into the seed as there); wait_ratio >= 0 applies the WAIT coin at
 * column wait_index (needs mask_bits). logprob / entropy f32[B] of the drawn
 * actions. The logits never reach memory. (ABI 10) */
int vmp_actor_head_bf16_sample(int32_t B, int32_t K, int32_t V, int32_t A, const uint16_t *h,
                               const uint16_t *weight, const float *bias,
                               const uint32_t *mask_bits, float wait_ratio, int32_t wait_index,
                               uint64_t seed, uint64_t offset, const uint64_t *rng_counter,
                               int32_t *action, float *logprob, float *entropy, float *workspace,
                               void *hip_stream);
/* Backward: recomputes the logits tiles and writes
 *   dlogits[b][ld] = bf16(d logprob/entropy loss / d logits)  (ld >= V*A)
 * with g_logprob / g_entropy f32[B] (nullable: 0), masked entries 0, as
 * vmp_policy_head_backward_bf16 computes from stored logits. The caller runs
 * it over row chunks (pointers offset to the chunk) and feeds each chunk's
 * dlogits to the dW / dh GEMMs, so no [B, V*A] tensor is ever allocated.
 * dbias (nullable): f32[V*A], ADDED to: the bias gradient of the chunk, the
 * column sums of its dlogits in f32 before the bf16 rounding, formed inside
 * the kernel (per-wave sums in LDS, one partial per M group, reduced in a
 * fixed order: run-to-run identical), so no pass over the dlogits computes
 * it. workspace (nullable): vmp_actor_head_bf16_bwd_workspace(B, V, A) floats
 * for the partials (else stream-ordered memory is allocated). */
int vmp_actor_head_bf16_bwd(int32_t B, int32_t K, int32_t V, int32_t A, const uint16_t *h,
                            const uint16_t *weight, const float *bias, const uint32_t *mask_bits,
                            const int32_t *action, const float *g_logprob,
                            const float *g_entropy, uint16_t *dlogits, int32_t ld, float *dbias,
                            float *workspace, void *hip_stream);
int64_t vmp_actor_head_bf16_bwd_workspace(int32_t B, int32_t V, int32_t A);

/* Eval-mode Record metrics on the device (record.py:34-134, base.py:131-148):
 * on = 1 allocates the recorder and starts it from the current state (call it
 * right after reset, as Base.test records from reset); every later vmp_step /
 * vmp_heuristic_step / vmp_rollout_heuristic step is recorded for every env.
 * While it is on, vmp_reset restarts the recorder of exactly the envs it
 * resets (previous placement from the reset state, no open lives, zero hist
 * and sums; the other envs' records go on), and vmp_restore restarts every
 * env's recorder from the restored state (a recorder is no part of a
 * snapshot): what the request log and the time series do. A VM present when a
 * recorder (re)starts has no arrival on record: its life starts with length 0
 * and grows from the next recorded step. on = 0 frees it. */
int vmp_record_enable(vmp_handle *h, int32_t on);
/* Read the metrics so far (non-destructive): hist u32[n_env][2][VMP_REC_BINS]
 * = counts of the pending and slowdown rates rounded to 3 decimals (x1000),
 * over every VM life incl. the open ones; sums f64[n_env][VMP_NREC]. The
 * Record.get_summary values follow from these (vmp/record.py). */
int vmp_record_read(vmp_handle *h, uint32_t *hist, double *sums);

/* Per-request outcome log on the device: what happened to request j of an env, for paired
 * comparisons of policies on one trace (vmp_set_trace), or on any workload. The id of a
 * request is its ordinal among the requests offered to the env since its last reset: the
 * value of total_requests before it is counted (on a traced env reset at step 0, its index
 * in the trace: drops are consumed). Per env the log holds `capacity` rows
 * int32[VMP_RQ_NF] indexed by id, updated by one more kernel after every vmp_step /
 * vmp_step_mask / vmp_heuristic_step; vmp_rollout_heuristic runs one step per launch while
 * the log is on, as it does for the recorder. t below is the env's timestep when the step
 * starts (reset leaves 1; a traced step t offers trace step t - 1).
 *   SLOT      -2: not observed (never offered, or offered before the log started);
 *             -1: dropped; >= 0: the slot it took
 *   ARRIVED   t of the step that offered it, set for dropped requests too
 *   PLACED    t of the step whose action phase first placed it validly (0: not yet), so
 *             PLACED - ARRIVED steps passed before its first placement
 *   FINISHED  t of the step whose _run_vms finished it (0: not yet)
 *   SUSPENDS  valid suspend actions on it
 *   WAIT_STEPS steps that left it at WAIT, the arrival step included, so
 *             WAIT_STEPS - (PLACED - ARRIVED) steps were spent suspended after placement
 * Meta int64[VMP_RQ_NMETA] per env: FIRST = total_requests when the env's log started, NEXT =
 * total_requests now, LOST = requests whose id was >= capacity (not logged; their VMs stay
 * untracked).
 *
 * vmp_reqlog_enable: capacity = rows per env; 0 frees the log. Otherwise the log is
 * (re)allocated and started from the current state: VMs already in the system are not
 * tracked and ids below FIRST stay unobserved. capacity < 0, above 2^31 - 1 or of a byte
 * size that does not fit returns VMP_EINVAL; a failed allocation VMP_EOOM, the handle (and
 * an earlier log) exactly as before. With the recorder on as well, the two share the
 * handle's scratch action / validity buffers. Stream-ordered behind the queued launches; it
 * allocates, so it must not be made during capture, and a graph captured before it does not
 * log and must be recaptured.
 * With the log on, vmp_reset restarts the log of exactly the envs it resets, vmp_restore
 * restarts every env's log (the log is not part of a snapshot), vmp_destroy frees it. (ABI 14) */
int vmp_reqlog_enable(vmp_handle *h, int64_t capacity);
/* Rows per env of the handle's log, 0 = off. */
int vmp_reqlog_info(const vmp_handle *h, int64_t *capacity);
/* Copy the log so far (non-destructive, stream-ordered): rows device
 * int32[n_env][capacity][VMP_RQ_NF], meta device int64[n_env][VMP_RQ_NMETA], each nullable.
 * VMP_ESTATE while the log is off. (On the device WAIT_STEPS of a VM that is waiting now is an
 * open count, written at events only; the read closes it in the caller's copy with one small
 * kernel, so the rows read are always the counts up to the last step.) */
int vmp_reqlog_read(vmp_handle *h, int32_t *rows, int64_t *meta);

/* Per-step time series on the device: how reward, waiting ratio, PM utilisation, target means,
 * used PMs and the counters develop over the steps of every env (the per-step lists of the
 * reference's Record, src/record.py:13-32), without a host copy per step. A third observer
 * behind the step, beside the recorder and the request log: one more kernel after every
 * vmp_step / vmp_step_mask / vmp_heuristic_step (vmp_rollout_heuristic runs one step per launch
 * while it is on) reads the post-step state and the step's reward and changes no env state.
 * Per env the series holds `capacity` rows f64[VMP_SR_NF]; row r covers the observed steps
 * [r stride, (r + 1) stride) counted from the env's series start. The first step of a window
 * stores fields 0..12, each later step adds its values to them with one f64 add in step order
 * (at stride 1 a row is the step's own values bit for bit); fields 13..18 are overwritten by
 * every step, so they are those of the window's latest step. Only the last, open row can have
 * STEPS < stride. CPU_SUM / MEM_SUM are the sums the `ut` reward is made of; the target means
 * are recomputed from the state under every reward function (EnvHdr's own are left alone).
 * With pm_rows, a second array f32[capacity][2 pms] per env keeps the PM part of the
 * observation (cpu then memory, as vmp_get_obs emits them) of each window's latest step: the
 * data of Base.test's utilisation timeline.
 * Meta int64[VMP_SR_NMETA] per env: FIRST = the timestep when the env's series started, COUNT =
 * steps observed since, LOST = steps whose row was >= capacity (counted, not stored). The
 * row index is read from COUNT on the device, so a replayed graph advances through the rows.
 *
 * vmp_series_enable: capacity = rows per env, 0 frees the series; stride >= 1 steps per row;
 * pm_rows 0 / 1. Otherwise the series is (re)allocated and started at row 0 from the current
 * state (FIRST = the current timestep). An invalid argument or a byte size that does not fit
 * returns VMP_EINVAL, a failed allocation VMP_EOOM; both leave the handle (and an earlier
 * series) exactly as before. The series asks the step for its reward only (a scratch f64[n_env]
 * where the caller passes none), never for actions or validity flags. Stream-ordered behind the
 * queued launches; it allocates, so it must not be made during capture, and a graph captured
 * before it does not observe and must be recaptured.
 * With the series on, vmp_reset restarts the series of exactly the envs it resets, vmp_restore
 * restarts every env's (the series is not part of a snapshot), vmp_destroy frees it. */
int vmp_series_enable(vmp_handle *h, int64_t capacity, int32_t stride, int32_t pm_rows);
/* Rows per env (0 = off), steps per row and whether PM rows are kept; each nullable. */
int vmp_series_info(const vmp_handle *h, int64_t *capacity, int32_t *stride, int32_t *pm_rows);
/* Copy the series so far (non-destructive, stream-ordered): rows device
 * f64[n_env][capacity][VMP_SR_NF], pm device f32[n_env][capacity][2 pms] (only with pm_rows),
 * meta device int64[n_env][VMP_SR_NMETA], each nullable. VMP_ESTATE while the series is off, or
 * for a pm buffer on a series without PM rows. */
int vmp_series_read(vmp_handle *h, double *rows, float *pm, int64_t *meta);

/* Fault injection (tests only): the n-th device allocation made by the
 * library from now on fails as out of memory (n = 0: off). Drives the
 * failure and cleanup paths of vmp_create / vmp_record_enable / vmp_mask_bool
 * under the host sanitizers (tests/native/capi_faults.cpp). */
int vmp_debug_fail_alloc(int32_t n);
/* Number of device allocations the library currently holds (all handles):
 * back to its previous value after a failed call or a vmp_destroy. */
int64_t vmp_debug_live_allocs(void);

/* Diagnostics: per-env shader-clock cycles per kernel phase, accumulated since
 * the previous call, device u64[n_env][24] (see tools/stamps.py for the phase names).
 * Only a library built with -DVMP_STAMPS records them; otherwise
 * returns VMP_EINVAL. */
int vmp_debug_stamps(vmp_handle *h, uint64_t *out);

/* Diagnostics (-DVMP_CHECK_QUIET check build, `make check-quiet`): the number
 * of per-step launches, since the previous call, that skipped the heuristic
 * on the header's quiet bit (EnvHdr::pad bit 62) although some pending VM
 * fitted a PM — always 0 unless an entry point that writes env state left the
 * bit stale. The check build evaluates the fit test on quiet steps too.
 * Returns VMP_EINVAL in a normal build. */
int vmp_debug_quiet_violations(int64_t *count);

/* Diagnostics: workgroups per CU the runtime reports for the per-step env
 * kernel of this handle (hipOccupancyMaxActiveBlocksPerMultiprocessor) and
 * the LDS bytes it is launched with (dynamic + static). */
int vmp_debug_occupancy(vmp_handle *h, int32_t *blocks_per_cu, int32_t *lds_bytes);

/* Diagnostics: the order in which the workgroups of the per-step launches of
 * the wave kernels (V <= 1024) take the envs. 0: index order; 1: every other
 * launch walks the envs downwards; 2: as 1, and the heuristic per-step launch
 * hands the envs that were not idle after the previous launch to workgroups
 * dispatched early. Results do not depend on the mode. A new handle starts in
 * mode 2; for measurements VMP_LAUNCH_ORDER=<mode>[:<tail divisor>] in the
 * environment of vmp_create overrides that. */
int vmp_debug_launch_order(vmp_handle *h, int32_t mode);
/* What the next heuristic per-step launch would do: env_of_block device
 * int32[n_env], the env each workgroup takes; flags_read device
 * uint8[64 * ceil(n_env / 64)], the flag bytes [chunk][rank] it decides on
 * (non-zero: not idle). Stream-ordered; counts as no launch. */
int vmp_debug_launch_map(vmp_handle *h, int32_t *env_of_block, uint8_t *flags_read);

#ifdef __cplusplus
}
#endif
#endif /* VMP_H */
