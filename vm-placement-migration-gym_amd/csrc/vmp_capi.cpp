// vmp_capi.cpp — extern "C" entry points of libvmp.so (declared in include/vmp.h).
// Argument checks, device allocation and kernel dispatch on the handle's stream
// (error text, counted allocations, Poisson setup: vmp_host.h; LDS carve: vmp_carve.h;
// the recorder, request log and time series behind a step: vmp_observers.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vmp.h"
#include "vmp_branch.h"
#include "vmp_carve.h"
#include "vmp_host.h"
#include "vmp_kernels.h"
#include "vmp_launch_order.h"
#include "vmp_layout.h"
#include "vmp_observers.h"
#include "vmp_state.h"
#include "vmp_trace.h"

using namespace vmp;

namespace vmp {
// error reporting for the policy kernels (vmp_policy.hip) through vmp_last_error()
int policy_fail(int code, const char *msg) { return fail(code, msg); }
}  // namespace vmp

struct vmp_handle {
  vmp_config cfg;
  int32_t N, P, V, A, D, W32;
  int32_t device;
  int32_t eval_mode;
  hipStream_t stream;
  uint32_t *vmw;  // [N][vm_pitch(V)]
  double *pm;
  EnvHdr *hdr;
  double *lg_arr, *lg_svc;
  PoisConst arr, svc;
  EnvParams prm;
  uint32_t *scratch_bits;  // for vmp_mask_bool
  PoisConst *pois_dev;
  uint64_t *stamps;
  uint64_t *jump_dev;
  uint8_t *bigscr;  // k_env_big's HBM spill of the accepted / existing VM sizes
  bool big;  // k_env_big (V > 1024, or VMP_BIG_KERNEL=1)
  Observers ob;  // recorder, request log, time series (vmp_observers.h)
  // per-env workload (vmp_set_workload); all null / 0 for a handle never given one
  double *wl;           // host f64 [N][2]: arrival_rate, service_length of every env
  PoisConst *wl_rec;    // host mirror of pois_env
  PoisConst *pois_env;  // device [N][2], prm.pois once set (address stable from then on);
                        // non-null selects the WL = true kernels (launch_env)
  double *lg_shared;    // device loggam table shared by all PTRS records of pois_env
  int32_t lg_shared_n;
  // trace-driven workload (vmp_set_trace); all null / 0 without one
  TraceDesc *tr_tab;    // device [N], prm.pois while set (address stable until vmp_clear_trace);
                        // non-null selects the trace kernels (launch_env)
  uint64_t *tr_data;    // device: every trace's offs and packed requests (vmp_trace.h)
  TraceDesc *tr_host;   // host mirror of tr_tab
  int32_t tr_n;         // traces
  int32_t *tr_map;      // host [N]
  int64_t *tr_info;     // host [tr_n][2]: steps, requests
  uint64_t tr_hash;     // content hash of (traces, map), carried by snapshots
  // launch order of the per-step wave launches (vmp_launch_order.h): their count
  // (its low bit is the next launch's parity), the mode and the tail divisor; the
  // two flag buffers lie behind hdr. None of it is part of a snapshot.
  uint32_t lo_count;
  int32_t lo_mode, lo_div;
  // vmp_branch: the staging copy of hdr | pm | vmw for dst == src, allocated on first use
  uint8_t *br_stage;
};

namespace {

// The wave step kernel of VPT slot rows per lane: external actions, the
// per-step launch or the fused rollout; wl: the handle has a per-env workload
// (p.pois is [N][2]: the kernels of vmp_kernels_wl.hip)
using EnvKernel = void (*)(EnvParams, StepOut);
template <int VPT>
EnvKernel env_kernel_tr(bool ext, bool one) {  // the handle has a trace: vmp_kernels_tr.hip
  if (ext) return k_env_ext_tr<VPT>;
  return one ? k_env_tr<VPT, true> : k_env_tr<VPT, false>;
}
template <int VPT>
EnvKernel env_kernel(bool ext, bool one, bool wl, bool tr) {
  if (tr) return env_kernel_tr<VPT>(ext, one);
  if (ext) return wl ? k_env_ext<VPT, true> : k_env_ext<VPT, false>;
  if (one) return wl ? k_env<VPT, true, true> : k_env<VPT, true, false>;
  return wl ? k_env<VPT, false, true> : k_env<VPT, false, false>;
}

// EnvParams::pad0 of the next per-step wave launch
uint32_t launch_order_word(const vmp_handle *h) {
  return lo_word(h->lo_mode, (int)(h->lo_count & 1u), h->N, lo_tail(h->N, h->lo_div));
}

int launch_env(vmp_handle *h, const StepOut &o) {
  dim3 grid((h->N + kEnvWavesPerBlock - 1) / kEnvWavesPerBlock), block(64 * kEnvWavesPerBlock);
  EnvParams p = h->prm;
  const bool wl = h->pois_env != nullptr, tr = h->tr_tab != nullptr;
  const int spt = big_spt(h->V);
  p.scap = kSpecDraws;
  p.lds_wave_bytes = launch_wave_bytes(p, o.k_steps);
  const size_t lds = launch_lds(p, o.k_steps, h->big, spt);
  if (!lds_fits(lds, h->big)) return fail(VMP_EINVAL, "config too large for the LDS carve");
  if (h->big) {  // one workgroup per env
    if (tr) launch_big_env_tr(spt, o.k_steps == 1, h->N, lds, h->stream, p, o);
    else if (wl) launch_big_env_wl(spt, o.k_steps == 1, h->N, lds, h->stream, p, o);
    else launch_big_env(spt, o.k_steps == 1, h->N, lds, h->stream, p, o);
    return launched();
  }
  // external actions: vmp_step, one step
  if (o.actions && o.k_steps != 1) return fail(VMP_EINVAL, "external actions take one step per launch");
  if (o.k_steps == 1) {  // per-step launches alternate their direction (vmp_launch_order.h)
    p.pad0 = (int32_t)launch_order_word(h);
    h->lo_count++;
  }
  const int need = (h->V + 63) / 64;  // the fewest of 1 / 2 / 4 / 8 / 16 rows that hold V
  const auto pick = need <= 1 ? env_kernel<1> : need <= 2 ? env_kernel<2> : need <= 4 ? env_kernel<4>
                    : need <= 8 ? env_kernel<8> : env_kernel<16>;
  hipLaunchKernelGGL(pick(o.actions != nullptr, o.k_steps == 1, wl, tr), grid, block, lds, h->stream, p, o);
  return launched();
}

StepOut empty_out() {
  StepOut o;
  std::memset(&o, 0, sizeof(o));
  o.policy = -1;
  return o;
}

void refresh_params(vmp_handle *h) {
  h->prm.eval_mode = h->eval_mode;
  h->prm.limit = h->eval_mode ? h->cfg.eval_steps : h->cfg.training_steps;
}

// One step and the observers that are on behind it (Observers::step)
int step_observed(vmp_handle *h, const StepOut &o) {
  return h->ob.step(h->prm, h->stream, o, [h](const StepOut &x) { return launch_env(h, x); });
}

int check_policy(int32_t policy) {
  if (policy == VMP_POLICY_FIRSTFIT || policy == VMP_POLICY_BESTFIT) return VMP_OK;
  return fail(VMP_EINVAL, "unknown policy");
}

}  // namespace

extern "C" {

int vmp_abi_version(void) { return VMP_ABI_VERSION; }
const char *vmp_last_error(void) { return g_err.c_str(); }

static int create_rest(vmp_handle *h, const vmp_config *cfg, int32_t n_env, const int64_t *seeds);

int vmp_create(const vmp_config *cfg, int32_t n_env, const int64_t *seeds, int32_t device,
               vmp_handle **out) {
  if (!cfg || !out || n_env <= 0 || !seeds) return fail(VMP_EINVAL, "null argument or n_env <= 0");
  if (cfg->pms < 1 || cfg->pms > 65533) return fail(VMP_EINVAL, "pms must be in [1, 65533]");
  if (cfg->vms < 1 || cfg->vms > kBigNT * kBigMaxSPT)
    return fail(VMP_EINVAL, "vms must be in [1, 10240] on this build");
  if (cfg->reward_function < 0 || cfg->reward_function > 2)
    return fail(VMP_EINVAL, "Function does not exist: reward_function");  // env.py:156
  if (cfg->sequence < 0 || cfg->sequence > 2) return fail(VMP_EINVAL, "unknown sequence");
  if (!(cfg->arrival_rate >= 0) || !(cfg->service_length >= 0))
    return fail(VMP_EINVAL, "arrival_rate and service_length must be >= 0");
  for (int32_t i = 0; i < n_env; i++)
    if (seeds[i] < 0) return fail(VMP_EINVAL, "seeds must be non-negative");
  HIP_TRY(hipSetDevice(device));
  vmp_handle *h = new vmp_handle();
  std::memset(h, 0, sizeof(*h));
  h->cfg = *cfg;
  h->N = n_env;
  h->P = cfg->pms;
  h->V = cfg->vms;
  h->A = cfg->allow_null_action ? cfg->pms + 2 : cfg->pms + 1;
  h->D = 3 * cfg->vms + 2 * cfg->pms;
  h->W32 = (h->A + 31) / 32;
  const char *force = getenv("VMP_BIG_KERNEL");
  h->big = cfg->vms > kMaxVPT * kWaveSize || (force && force[0] == '1');
  h->device = device;
  h->stream = nullptr;
  int rc = setup_pois(cfg->arrival_rate, h->arr, &h->lg_arr);
  if (rc == VMP_OK) rc = setup_pois(cfg->service_length, h->svc, &h->lg_svc);
  if (rc == VMP_OK) rc = create_rest(h, cfg, n_env, seeds);
  if (rc != VMP_OK) return fail_after(rc, [&] { vmp_destroy(h); });  // frees what was allocated
  *out = h;
  return VMP_OK;
}

// vmp_create after the handle exists: every failure returns a code and the
// caller destroys the handle (vmp_destroy tolerates what was not allocated).
static int create_rest(vmp_handle *h, const vmp_config *cfg, int32_t n_env, const int64_t *seeds) {
  hipError_t e1 = dev_malloc(&h->vmw, sizeof(uint32_t) * (size_t)n_env * vm_pitch(h->V));
  hipError_t e2 = dev_malloc(&h->pm, sizeof(double) * (size_t)n_env * 2 * h->P);
  // the headers, then the two flag buffers of the launch order (zero: every env idle)
  const size_t hdr_bytes = sizeof(EnvHdr) * (size_t)n_env + 2 * (size_t)lo_flag_bytes(n_env);
  hipError_t e3 = dev_malloc(&h->hdr, hdr_bytes);
  if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess)
    return fail(VMP_EOOM, "device allocation failed");
  HIP_TRY(hipMemset(h->hdr, 0, hdr_bytes));
  h->lo_mode = kLoDefaultMode;
  h->lo_div = kLoDefaultDiv;
  if (const char *m = getenv("VMP_LAUNCH_ORDER")) {  // measurement: "<mode>" or "<mode>:<divisor>"
    if (m[0] >= '0' && m[0] <= '2') h->lo_mode = m[0] - '0';
    if (m[0] && m[1] == ':' && atoi(m + 2) >= 4) h->lo_div = atoi(m + 2);
  }
  EnvParams &p = h->prm;
  p.N = h->N;
  p.P = h->P;
  p.V = h->V;
  p.A = h->A;
  p.D = h->D;
  p.W32 = h->W32;
  p.reward = cfg->reward_function;
  p.cap_target_util = cfg->cap_target_util;
  int64_t M = cfg->training_steps > cfg->eval_steps ? cfg->training_steps : cfg->eval_steps;
  p.M2 = 2 * M;
  p.beta = cfg->beta;
  p.seq_lo = cfg->sequence == VMP_SEQ_HIGHUNIFORM ? 0.25 : 0.1;
  double hi = cfg->sequence == VMP_SEQ_LOWUNIFORM ? 0.65 : 1.0;
  p.seq_range = hi - p.seq_lo;  // Generator.uniform: low + (high-low)*u
  {
    PoisConst pc[2] = {h->arr, h->svc};
    HIP_TRY(dev_malloc(&h->pois_dev, sizeof(pc)));
    HIP_TRY(hipMemcpy(h->pois_dev, pc, sizeof(pc), hipMemcpyHostToDevice));
    p.pois = h->pois_dev;
    // PCG64 jump table for the lane-parallel draws (k_env prologue)
    uint64_t jt[kJumpWords];
    pcg_jump_table(jt);
    HIP_TRY(dev_malloc(&h->jump_dev, sizeof(jt)));
    HIP_TRY(hipMemcpy(h->jump_dev, jt, sizeof(jt), hipMemcpyHostToDevice));
    p.jump = h->jump_dev;
  }
  p.vmw = h->vmw;
  p.pm = h->pm;
  p.hdr = h->hdr;
  if (h->big) carve_big(h->P, h->V, p);
  else carve_wave(h->P, h->V, p);
  if (h->big) {
    HIP_TRY(dev_malloc(&h->bigscr, (size_t)n_env * 4 * (size_t)h->V));
    p.bigscr = h->bigscr;
  }
  // diagnostic per-env clocks: -DVMP_STAMPS builds, or VMP_STAMP_BUF=1 for the
  // workgroup timing build (-DVMP_WGTIME, tools/wgtime.py)
  bool want_stamps = getenv("VMP_STAMP_BUF") && getenv("VMP_STAMP_BUF")[0] == '1';
#ifdef VMP_STAMPS
  want_stamps = true;
#endif
  if (want_stamps) {
    HIP_TRY(dev_malloc(&h->stamps, sizeof(uint64_t) * kStamps * (size_t)n_env));
    HIP_TRY(hipMemset(h->stamps, 0, sizeof(uint64_t) * kStamps * (size_t)n_env));
    p.stamps = h->stamps;
  }
  if (pw_worst(h->V > h->P ? h->V : h->P).depth > 12)
    return fail(VMP_EINVAL, "config exceeds the pairwise-sum recursion depth of this build");
  if (!carve_fits(p, h->big))
    return fail(VMP_EINVAL, "config too large for the LDS carve of this build");
  refresh_params(h);
  int64_t *dseeds = nullptr;
  HIP_TRY(dev_malloc(&dseeds, sizeof(int64_t) * n_env));
  hipError_t e = hipMemcpy(dseeds, seeds, sizeof(int64_t) * n_env, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    dim3 grid((n_env + kWavesPerBlock - 1) / kWavesPerBlock), block(64 * kWavesPerBlock);
    hipLaunchKernelGGL(k_reset, grid, block, 0, h->stream, h->prm, dseeds, nullptr, nullptr);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  }
  dev_free(dseeds);
  if (e != hipSuccess) return fail(VMP_EDEVICE, std::string("vmp_create reset: ") + hipGetErrorString(e));
  return VMP_OK;
}

int vmp_destroy(vmp_handle *h) {
  if (!h) return VMP_OK;
  for (void *q : {(void *)h->vmw, (void *)h->pm, (void *)h->hdr, (void *)h->lg_arr, (void *)h->lg_svc,
                  (void *)h->scratch_bits, (void *)h->pois_dev, (void *)h->jump_dev, (void *)h->bigscr,
                  (void *)h->stamps, (void *)h->pois_env, (void *)h->lg_shared, (void *)h->tr_tab,
                  (void *)h->tr_data, (void *)h->br_stage, (void *)h->ob.mask})
    dev_free(q);
  std::free(h->wl);
  std::free(h->wl_rec);
  std::free(h->tr_host);
  std::free(h->tr_map);
  std::free(h->tr_info);
  vmp_series_enable(h, 0, 1, 0);
  vmp_reqlog_enable(h, 0);
  vmp_record_enable(h, 0);
  delete h;
  return VMP_OK;
}

// ---- per-env workload ----
// Env i's pair of records is what vmp_create computes for a config of its
// (arrival_rate, service_length), except that every PTRS record points into
// one loggam table (entry k = loggam(k) whatever the rate) sized for the
// largest tab_n in use; each record keeps its own tab_n, so an env takes the
// table / loggam_far branch exactly where a homogeneous handle of its rate does.
int vmp_set_workload(vmp_handle *h, const double *arrival_rate, const double *service_length) {
  if (!h) return fail(VMP_EINVAL, "null handle");
  if (h->tr_tab) return fail(VMP_ESTATE, "vmp_set_workload: the handle has a trace (vmp_clear_trace first)");
  if (!arrival_rate && !service_length) return VMP_OK;
  const size_t N = (size_t)h->N;
  for (size_t i = 0; i < N; i++) {
    const double a = arrival_rate ? arrival_rate[i] : 0.0, s = service_length ? service_length[i] : 0.0;
    if (!std::isfinite(a) || !std::isfinite(s) || a < 0 || s < 0)
      return fail(VMP_EINVAL, "arrival_rate and service_length must be finite and >= 0");
  }
  std::vector<double> wl(2 * N);
  std::vector<PoisConst> rec(2 * N);
  int32_t need_n = 0;
  for (size_t i = 0; i < N; i++) {
    wl[2 * i] = arrival_rate ? arrival_rate[i] : h->wl ? h->wl[2 * i] : h->cfg.arrival_rate;
    wl[2 * i + 1] = service_length ? service_length[i] : h->wl ? h->wl[2 * i + 1] : h->cfg.service_length;
    for (int j = 0; j < 2; j++) {
      pois_consts(wl[2 * i + j], rec[2 * i + j]);
      if (rec[2 * i + j].tab_n > need_n) need_n = rec[2 * i + j].tab_n;
    }
  }
  // host copies first: nothing below them can fail halfway
  const bool first = h->pois_env == nullptr;
  double *wl_new = h->wl;
  PoisConst *rec_new = h->wl_rec;
  if (first) {
    wl_new = (double *)std::malloc(sizeof(double) * 2 * N);
    rec_new = (PoisConst *)std::malloc(sizeof(PoisConst) * 2 * N);
    if (!wl_new || !rec_new) {
      std::free(wl_new);
      std::free(rec_new);
      return fail(VMP_EOOM, "vmp_set_workload: host allocation failed");
    }
  }
  double *tab = h->lg_shared, *tab_new = nullptr;
  PoisConst *dev_new = nullptr;
  int rc = VMP_OK;
  if (need_n > h->lg_shared_n) {
    rc = make_loggam_tab(need_n, &tab_new);
    tab = tab_new;
  }
  if (rc == VMP_OK && first) {
    const hipError_t e = dev_malloc(&dev_new, sizeof(PoisConst) * 2 * N);
    if (e != hipSuccess) rc = fail_hip("vmp_set_workload: ", e);
  }
  if (rc == VMP_OK) {
    for (PoisConst &c : rec)
      if (c.kind == 2) c.loggam_tab = tab;
    // stream-ordered behind the launches already queued, which read the old
    // values; the call returns once the new ones are in place
    PoisConst *dst = first ? dev_new : h->pois_env;
    hipError_t e = hipMemcpyAsync(dst, rec.data(), sizeof(PoisConst) * 2 * N, hipMemcpyHostToDevice,
                                  h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
      rc = fail(VMP_EDEVICE, std::string("vmp_set_workload copy: ") + hipGetErrorString(e));
      if (!first) {  // put the previous records back before the new table goes
        (void)hipMemcpyAsync(dst, h->wl_rec, sizeof(PoisConst) * 2 * N, hipMemcpyHostToDevice, h->stream);
        (void)hipStreamSynchronize(h->stream);
      }
    }
  }
  if (rc != VMP_OK)
    return fail_after(rc, [&] {
      dev_free(tab_new);
      dev_free(dev_new);
      if (first) {
        std::free(wl_new);
        std::free(rec_new);
      }
    });
  // commit. No queued launch reads the old table any more (synchronised above)
  if (tab_new) {
    dev_free(h->lg_shared);
    h->lg_shared = tab_new;
    h->lg_shared_n = need_n;
  }
  std::memcpy(wl_new, wl.data(), sizeof(double) * 2 * N);
  std::memcpy(rec_new, rec.data(), sizeof(PoisConst) * 2 * N);
  h->wl = wl_new;
  h->wl_rec = rec_new;
  if (first) {
    h->pois_env = dev_new;
    h->prm.pois = dev_new;  // launch_env picks the WL kernels from now on
  }
  return VMP_OK;
}

int vmp_get_workload(const vmp_handle *h, double *arrival_rate, double *service_length) {
  if (!h) return fail(VMP_EINVAL, "null handle");
  for (int32_t i = 0; i < h->N; i++) {
    if (arrival_rate) arrival_rate[i] = h->wl ? h->wl[2 * i] : h->cfg.arrival_rate;
    if (service_length) service_length[i] = h->wl ? h->wl[2 * i + 1] : h->cfg.service_length;
  }
  return VMP_OK;
}

// ---- trace-driven workload ----
// One device block holds every trace (offs, then packed requests: vmp_trace.h);
// the per-env descriptor table points into it. The first call allocates the
// table and moves prm.pois to it (launch_env then picks the trace kernels);
// later calls rewrite it in place behind the queued launches.
int vmp_set_trace(vmp_handle *h, int32_t n_traces, const vmp_trace *traces,
                  const int32_t *trace_of_env) {
  if (!h) return fail(VMP_EINVAL, "null handle");
  if (const char *why = trace_check(n_traces, traces, trace_of_env, h->N)) return fail(VMP_EINVAL, why);
  const size_t N = (size_t)h->N;
  std::vector<size_t> at((size_t)n_traces);
  size_t words = 0;
  for (int32_t i = 0; i < n_traces; i++) {
    at[(size_t)i] = words;
    words += trace_words(traces[i]);
  }
  std::vector<uint64_t> data(words);
  for (int32_t i = 0; i < n_traces; i++) trace_pack(traces[i], data.data() + at[(size_t)i]);
  // host copies first: nothing below them can fail halfway
  TraceDesc *host_new = (TraceDesc *)std::malloc(sizeof(TraceDesc) * N);
  int32_t *map_new = (int32_t *)std::malloc(sizeof(int32_t) * N);
  int64_t *info_new = (int64_t *)std::malloc(sizeof(int64_t) * 2 * (size_t)n_traces);
  uint64_t *data_new = nullptr;
  TraceDesc *tab_new = nullptr;
  const bool first = h->tr_tab == nullptr;
  int rc = VMP_OK;
  if (!host_new || !map_new || !info_new) rc = fail(VMP_EOOM, "vmp_set_trace: host allocation failed");
  if (rc == VMP_OK) {
    hipError_t e = dev_malloc(&data_new, sizeof(uint64_t) * words);
    if (e == hipSuccess && first) e = dev_malloc(&tab_new, sizeof(TraceDesc) * N);
    if (e != hipSuccess) rc = fail_hip("vmp_set_trace: ", e);
  }
  if (rc == VMP_OK) {
    for (size_t e = 0; e < N; e++) {
      const int32_t i = trace_of_env ? trace_of_env[e] : 0;
      const uint64_t *base = data_new + at[(size_t)i];
      map_new[e] = i;
      host_new[e] = TraceDesc{reinterpret_cast<const int64_t *>(base), base + traces[i].steps + 1,
                              traces[i].steps, 0};
    }
    for (int32_t i = 0; i < n_traces; i++) {
      info_new[2 * i] = traces[i].steps;
      info_new[2 * i + 1] = traces[i].offs[traces[i].steps];
    }
    // stream-ordered behind the launches already queued, which read the old
    // table and arrays; the call returns once the new ones are in place
    TraceDesc *dst = first ? tab_new : h->tr_tab;
    hipError_t e = hipMemcpyAsync(data_new, data.data(), sizeof(uint64_t) * words,
                                  hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(dst, host_new, sizeof(TraceDesc) * N, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
      rc = fail(VMP_EDEVICE, std::string("vmp_set_trace copy: ") + hipGetErrorString(e));
      if (!first) {  // put the previous table back before the new arrays go
        (void)hipMemcpyAsync(dst, h->tr_host, sizeof(TraceDesc) * N, hipMemcpyHostToDevice, h->stream);
        (void)hipStreamSynchronize(h->stream);
      }
    }
  }
  if (rc != VMP_OK)
    return fail_after(rc, [&] {
      dev_free(data_new);
      dev_free(tab_new);
      std::free(host_new);
      std::free(map_new);
      std::free(info_new);
    });
  // commit. No queued launch reads the old arrays any more (synchronised above)
  dev_free(h->tr_data);
  std::free(h->tr_host);
  std::free(h->tr_map);
  std::free(h->tr_info);
  h->tr_data = data_new;
  h->tr_host = host_new;
  h->tr_map = map_new;
  h->tr_info = info_new;
  h->tr_n = n_traces;
  h->tr_hash = trace_hash(n_traces, traces, trace_of_env, h->N);
  if (first) {
    h->tr_tab = tab_new;
    h->prm.pois = reinterpret_cast<const PoisConst *>(tab_new);  // launch_env: the trace kernels
  }
  return VMP_OK;
}

int vmp_clear_trace(vmp_handle *h) {
  if (!h) return fail(VMP_EINVAL, "null handle");
  if (!h->tr_tab) return VMP_OK;
  HIP_TRY(hipStreamSynchronize(h->stream));  // queued launches read the table
  h->prm.pois = h->pois_env ? h->pois_env : h->pois_dev;
  dev_free(h->tr_tab);
  dev_free(h->tr_data);
  std::free(h->tr_host);
  std::free(h->tr_map);
  std::free(h->tr_info);
  h->tr_tab = nullptr;
  h->tr_data = nullptr;
  h->tr_host = nullptr;
  h->tr_map = nullptr;
  h->tr_info = nullptr;
  h->tr_n = 0;
  h->tr_hash = 0;
  return VMP_OK;
}

int vmp_trace_info(const vmp_handle *h, int32_t *n_traces, int32_t *trace_of_env, int64_t *steps,
                   int64_t *requests) {
  if (!h) return fail(VMP_EINVAL, "null handle");
  if (n_traces) *n_traces = h->tr_n;
  if (!h->tr_tab) return VMP_OK;
  if (trace_of_env) std::memcpy(trace_of_env, h->tr_map, sizeof(int32_t) * (size_t)h->N);
  for (int32_t i = 0; i < h->tr_n; i++) {
    if (steps) steps[i] = h->tr_info[2 * i];
    if (requests) requests[i] = h->tr_info[2 * i + 1];
  }
  return VMP_OK;
}

int vmp_set_stream(vmp_handle *h, void *s) {
  if (!h) return fail(VMP_EINVAL, "null handle");
  h->stream = (hipStream_t)s;
  return VMP_OK;
}

int vmp_set_eval(vmp_handle *h, int32_t eval_mode) {
  if (!h) return fail(VMP_EINVAL, "null handle");
  h->eval_mode = eval_mode ? 1 : 0;
  refresh_params(h);
  return VMP_OK;
}

int vmp_dims(const vmp_handle *h, int32_t *n, int32_t *P, int32_t *V, int32_t *A, int32_t *D) {
  if (!h) return fail(VMP_EINVAL, "null handle");
  if (n) *n = h->N;
  if (P) *P = h->P;
  if (V) *V = h->V;
  if (A) *A = h->A;
  if (D) *D = h->D;
  return VMP_OK;
}

int vmp_reset(vmp_handle *h, const int64_t *seeds, const uint8_t *env_mask, float *obs) {
  if (!h) return fail(VMP_EINVAL, "null handle");
  dim3 grid((h->N + kWavesPerBlock - 1) / kWavesPerBlock), block(64 * kWavesPerBlock);
  hipLaunchKernelGGL(k_reset, grid, block, 0, h->stream, h->prm, seeds, env_mask, obs);
  if (const int rc = launched()) return rc;
  return h->ob.restart(h->prm, h->stream, env_mask);  // the observers of the envs just reset
}

int vmp_step(vmp_handle *h, const int32_t *actions, float *obs, double *reward, uint8_t *done,
             uint8_t *valid) {
  return vmp_step_mask(h, actions, obs, reward, done, valid, nullptr);
}

int vmp_step_mask(vmp_handle *h, const int32_t *actions, float *obs, double *reward, uint8_t *done,
                  uint8_t *valid, uint32_t *next_mask_bits) {
  if (!h || !actions) return fail(VMP_EINVAL, "null handle or actions");
  StepOut o = empty_out();
  o.actions = actions;
  o.obs = obs;
  o.reward = reward;
  o.done = done;
  o.valid = valid;
  o.mask_bits = next_mask_bits;  // written from the post-step state, as vmp_mask would
  o.k_steps = 1;
  return step_observed(h, o);
}

int vmp_heuristic_act(vmp_handle *h, int32_t policy, int32_t *actions) {
  if (!h || !actions) return fail(VMP_EINVAL, "null handle or actions");
  if (const int rc = check_policy(policy)) return rc;
  StepOut o = empty_out();
  o.policy = policy;
  o.act_out = actions;
  o.k_steps = 0;
  return launch_env(h, o);
}

int vmp_heuristic_act_obs(vmp_handle *h, int32_t policy, const float *obs, int32_t *actions) {
  if (!h || !obs || !actions) return fail(VMP_EINVAL, "null handle, obs or actions");
  if (const int rc = check_policy(policy)) return rc;
  // the whole PM view in one workgroup's LDS
  const size_t lds = act_obs_lds(h->P);
  if (lds > (size_t)kCuLdsBytes) return fail(VMP_EINVAL, "act from observation supports P <= 9045");
  hipLaunchKernelGGL(k_act_obs, dim3(h->N), dim3(64), lds, h->stream, h->P, h->V, policy, obs,
                     actions);
  return launched();
}

static int heuristic_step_impl(vmp_handle *h, int32_t policy, int32_t *actions_out, float *obs,
                               double *reward, uint8_t *done, uint8_t *valid,
                               int64_t *done_count) {
  if (!h) return fail(VMP_EINVAL, "null handle");
  if (const int rc = check_policy(policy)) return rc;
  StepOut o = empty_out();
  o.policy = policy;
  o.act_out = actions_out;
  o.obs = obs;
  o.reward = reward;
  o.done = done;
  o.done_count = done_count;
  o.valid = valid;
  o.k_steps = 1;
  return step_observed(h, o);
}

int vmp_heuristic_step(vmp_handle *h, int32_t policy, int32_t *actions_out, float *obs,
                       double *reward, uint8_t *done, uint8_t *valid) {
  return heuristic_step_impl(h, policy, actions_out, obs, reward, done, valid, nullptr);
}

int vmp_rollout_heuristic(vmp_handle *h, int32_t policy, int32_t k_steps, double *rewards,
                          int64_t *done_count) {
  if (!h || k_steps < 1) return fail(VMP_EINVAL, "null handle or k_steps < 1");
  if (const int rc = check_policy(policy)) return rc;
  if (h->ob.any()) {  // observed: one step per launch, the observers after each
    for (int32_t k = 0; k < k_steps; k++) {
      int rc = heuristic_step_impl(h, policy, nullptr, nullptr,
                                   rewards ? rewards + (int64_t)k * h->N : nullptr, nullptr,
                                   nullptr, done_count);
      if (rc) return rc;
    }
    return VMP_OK;
  }
  // launches of at most kMaxStepsPerLaunch steps (the per-launch draw region)
  for (int32_t k0 = 0; k0 < k_steps; k0 += kMaxStepsPerLaunch) {
    StepOut o = empty_out();
    o.policy = policy;
    o.reward = rewards ? rewards + (int64_t)k0 * h->N : nullptr;
    o.done_count = done_count;
    o.k_steps = k_steps - k0 < kMaxStepsPerLaunch ? k_steps - k0 : kMaxStepsPerLaunch;
    int rc = launch_env(h, o);
    if (rc) return rc;
  }
  return VMP_OK;
}

// ---- the observers: Record metrics, per-request outcome log, per-step time series ----
int vmp_record_enable(vmp_handle *h, int32_t on) {
  if (!h) return fail(VMP_EINVAL, "null handle");
  return h->ob.record_enable(h->prm, h->stream, on);
}

int vmp_record_read(vmp_handle *h, uint32_t *hist, double *sums) {
  if (!h || !hist || !sums) return fail(VMP_EINVAL, "null argument");
  return h->ob.record_read(h->prm, h->stream, hist, sums);
}

int vmp_reqlog_enable(vmp_handle *h, int64_t capacity) {
  if (!h) return fail(VMP_EINVAL, "null handle");
  return h->ob.reqlog_enable(h->prm, h->stream, capacity);
}

int vmp_reqlog_info(const vmp_handle *h, int64_t *capacity) {
  if (!h || !capacity) return fail(VMP_EINVAL, "null argument");
  return h->ob.reqlog_info(capacity);
}

int vmp_reqlog_read(vmp_handle *h, int32_t *rows, int64_t *meta) {
  if (!h) return fail(VMP_EINVAL, "null handle");
  return h->ob.reqlog_read(h->prm, h->stream, rows, meta);
}

int vmp_series_enable(vmp_handle *h, int64_t capacity, int32_t stride, int32_t pm_rows) {
  if (!h) return fail(VMP_EINVAL, "null handle");
  return h->ob.series_enable(h->prm, h->stream, capacity, stride, pm_rows);
}

int vmp_series_info(const vmp_handle *h, int64_t *capacity, int32_t *stride, int32_t *pm_rows) {
  if (!h) return fail(VMP_EINVAL, "null handle");
  return h->ob.series_info(capacity, stride, pm_rows);
}

int vmp_series_read(vmp_handle *h, double *rows, float *pm, int64_t *meta) {
  if (!h) return fail(VMP_EINVAL, "null handle");
  return h->ob.series_read(h->prm, h->stream, rows, pm, meta);
}

int vmp_mask(vmp_handle *h, uint32_t *bits) {
  if (!h || !bits) return fail(VMP_EINVAL, "null argument");
  StepOut o = empty_out();
  o.mask_bits = bits;
  return launch_env(h, o);
}

int vmp_mask_bool(vmp_handle *h, uint8_t *mask) {
  if (!h || !mask) return fail(VMP_EINVAL, "null argument");
  if (!h->scratch_bits)
    HIP_TRY(dev_malloc(&h->scratch_bits, sizeof(uint32_t) * (size_t)h->N * h->V * h->W32));
  int rc = vmp_mask(h, h->scratch_bits);
  if (rc) return rc;
  int64_t rows = (int64_t)h->N * h->V;
  int64_t n = rows * h->A;
  hipLaunchKernelGGL(k_mask_bool, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream,
                     rows, h->A, h->W32, h->scratch_bits, mask);
  return launched();
}

int vmp_get_obs(vmp_handle *h, float *obs) {
  if (!h || !obs) return fail(VMP_EINVAL, "null argument");
  StepOut o = empty_out();
  o.obs = obs;
  return launch_env(h, o);
}

int vmp_get_counters(vmp_handle *h, int64_t *counters) {
  if (!h || !counters) return fail(VMP_EINVAL, "null argument");
  hipLaunchKernelGGL(k_counters, dim3((h->N + 255) / 256), dim3(256), 0, h->stream, h->prm,
                     counters, nullptr);
  return launched();
}

int vmp_get_stats(vmp_handle *h, double *stats) {
  if (!h || !stats) return fail(VMP_EINVAL, "null argument");
  if (h->V > kMaxVPT * kWaveSize) {
    // beyond the static per-wave buffers: a private carve for this kernel alone
    EnvParams q = h->prm;
    const size_t lds = carve_target_means(q);
    hipLaunchKernelGGL(k_target_means_lds, dim3(h->N), dim3(64), lds, h->stream, q);
  } else
    hipLaunchKernelGGL(k_target_means, dim3((h->N + kWavesPerBlock - 1) / kWavesPerBlock),
                       dim3(64 * kWavesPerBlock), 0, h->stream, h->prm);
  hipLaunchKernelGGL(k_counters, dim3((h->N + 255) / 256), dim3(256), 0, h->stream, h->prm,
                     nullptr, stats);
  return launched();
}

int vmp_get_state(vmp_handle *h, int64_t *placement, double *vm_cpu, double *vm_mem,
                  double *cpu, double *mem, int64_t *remaining) {
  if (!h) return fail(VMP_EINVAL, "null handle");
  int64_t n = (int64_t)h->N * (h->V > h->P ? h->V : h->P);
  hipLaunchKernelGGL(k_export, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream,
                     h->prm, placement, vm_cpu, vm_mem, cpu, mem, remaining, nullptr);
  return launched();
}

int vmp_get_rank(vmp_handle *h, int64_t *rank) {
  if (!h || !rank) return fail(VMP_EINVAL, "null argument");
  hipLaunchKernelGGL(k_rank, dim3(h->N), dim3(64), sizeof(uint64_t) * ((h->P + 63) / 64),
                     h->stream, h->prm, rank);
  return launched();
}

// ---- checkpoint / resume of the batched env state ----
// Snapshot = a 256-B descriptor, then hdr[N] | pm[N][2P] | vmw[N][pitch] as the
// kernels keep them (PCG64 states, sequence bases, counters, step hints and
// finish keys included), so a restore is bit-exact by construction: the
// restored handle holds the very bytes every later kernel reads.
namespace {
constexpr uint64_t kSnapMagic = 0x31504e534d504d56ULL;  // "VMPMSNP1"
constexpr int64_t kSnapHead = 256;
struct SnapDesc {
  uint64_t magic;
  int32_t abi, hdr_bytes;
  int32_t N, P, V, A;
  vmp_config cfg;  // seed excluded from the compatibility check
  int32_t workload;  // 1: the handle had a per-env workload, f64 [N][2] follows the VM words
  int32_t traced;    // 1: the handle had a trace (vmp_set_trace) of content hash trace_hash
  uint64_t trace_hash;
};
static_assert(sizeof(SnapDesc) <= kSnapHead, "snapshot descriptor exceeds its header");
// byte offsets of the parts behind the descriptor, and their sizes
struct SnapLayout {
  size_t nh, np, nv, nw;  // hdr, pm, vmw, workload (0 without one)
  size_t hdr, pm, vmw, wl, end;
  explicit SnapLayout(const vmp_handle *h)
      : nh(sizeof(EnvHdr) * (size_t)h->N), np(16 * (size_t)h->N * h->P),
        nv(4 * (size_t)h->N * vm_pitch(h->V)), nw(h->wl ? 16 * (size_t)h->N : 0),
        hdr(kSnapHead), pm(hdr + nh), vmw(pm + np), wl(vmw + nv), end(wl + nw) {}
};
bool same_config(const vmp_config &a, const vmp_config &b) {
  vmp_config x = a, y = b;
  x.seed = y.seed = 0;
  return std::memcmp(&x, &y, sizeof(x)) == 0;
}
}  // namespace

int vmp_snapshot_bytes(const vmp_handle *h, int64_t *bytes) {
  if (!h || !bytes) return fail(VMP_EINVAL, "null argument");
  *bytes = (int64_t)SnapLayout(h).end;
  return VMP_OK;
}

int vmp_snapshot(vmp_handle *h, void *dst) {
  if (!h || !dst) return fail(VMP_EINVAL, "null argument");
  if (((uintptr_t)dst) & 15) return fail(VMP_EINVAL, "vmp_snapshot: dst must be 16-byte aligned");
  uint8_t head[kSnapHead];
  std::memset(head, 0, sizeof(head));
  SnapDesc d;
  std::memset(&d, 0, sizeof(d));
  d.magic = kSnapMagic;
  d.abi = VMP_ABI_VERSION;
  d.hdr_bytes = (int32_t)sizeof(EnvHdr);
  d.N = h->N, d.P = h->P, d.V = h->V, d.A = h->A;
  d.cfg = h->cfg;
  d.workload = h->wl ? 1 : 0;
  d.traced = h->tr_tab ? 1 : 0;
  d.trace_hash = h->tr_hash;
  std::memcpy(head, &d, sizeof(d));
  uint8_t *o = (uint8_t *)dst;
  const SnapLayout s(h);
  HIP_TRY(hipMemcpyAsync(o, head, kSnapHead, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(o + s.hdr, h->hdr, s.nh, hipMemcpyDeviceToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(o + s.pm, h->pm, s.np, hipMemcpyDeviceToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(o + s.vmw, h->vmw, s.nv, hipMemcpyDeviceToDevice, h->stream));
  if (h->wl) HIP_TRY(hipMemcpyAsync(o + s.wl, h->wl, s.nw, hipMemcpyHostToDevice, h->stream));
  // the descriptor's host copy is a stack buffer: the call returns after it is read
  HIP_TRY(hipStreamSynchronize(h->stream));
  return VMP_OK;
}

int vmp_restore(vmp_handle *h, const void *src) {
  if (!h || !src) return fail(VMP_EINVAL, "null argument");
  if (((uintptr_t)src) & 15) return fail(VMP_EINVAL, "vmp_restore: src must be 16-byte aligned");
  SnapDesc d;
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(&d, src, sizeof(d), hipMemcpyDeviceToHost));
  if (d.magic != kSnapMagic || d.abi != VMP_ABI_VERSION || d.hdr_bytes != (int32_t)sizeof(EnvHdr))
    return fail(VMP_EINVAL, "vmp_restore: not a snapshot of this library version");
  if (d.N != h->N || d.P != h->P || d.V != h->V || d.A != h->A || !same_config(d.cfg, h->cfg))
    return fail(VMP_EINVAL, "vmp_restore: snapshot of another env count or config");
  const uint8_t *s = (const uint8_t *)src;
  const SnapLayout l(h);
  // the env state continues bit-exactly only under the workload it ran with
  if ((d.workload != 0) != (h->wl != nullptr))
    return fail(VMP_EINVAL, "vmp_restore: snapshot and handle differ in having a per-env workload");
  // ... and a traced env only under the very requests it was replaying
  if ((d.traced != 0) != (h->tr_tab != nullptr))
    return fail(VMP_EINVAL, "vmp_restore: snapshot and handle differ in having a trace");
  if (h->tr_tab && d.trace_hash != h->tr_hash)
    return fail(VMP_EINVAL, "vmp_restore: snapshot of another trace");
  if (h->wl) {
    std::vector<double> w(2 * (size_t)h->N);
    HIP_TRY(hipMemcpy(w.data(), s + l.wl, l.nw, hipMemcpyDeviceToHost));
    if (std::memcmp(w.data(), h->wl, l.nw) != 0)
      return fail(VMP_EINVAL, "vmp_restore: snapshot of another per-env workload");
  }
  HIP_TRY(hipMemcpyAsync(h->hdr, s + l.hdr, l.nh, hipMemcpyDeviceToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(h->pm, s + l.pm, l.np, hipMemcpyDeviceToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(h->vmw, s + l.vmw, l.nv, hipMemcpyDeviceToDevice, h->stream));
  // no observer is part of a snapshot: all restart from the restored state
  return h->ob.restart(h->prm, h->stream, nullptr);
}

// ---- branch: env states between handles on the device ----
// One gather launch (vmp_branch.hip) on dst's stream. dst == src reads a staging
// copy of the three arrays made on the same stream just before, so any map is
// correct in place. The observers of the overwritten envs restart through the
// mask the kernel derives from the map.
namespace {
BranchSide branch_side(const vmp_handle *h) {
  BranchSide s;
  std::memset(&s, 0, sizeof(s));
  s.P = h->P, s.V = h->V, s.A = h->A;
  s.device = h->device;
  s.traced = h->tr_tab ? 1 : 0;
  s.cfg = h->cfg;
  return s;
}
}  // namespace

int vmp_branch(vmp_handle *dst, vmp_handle *src, const int32_t *src_of_dst, const int64_t *seeds) {
  if (!dst || !src || !src_of_dst) return fail(VMP_EINVAL, "vmp_branch: null handle or map");
  const BranchSide ds = branch_side(dst), ss = branch_side(src);
  const char *why = nullptr;
  if (const int rc = branch_check(&ds, &ss, src_of_dst, &why)) return fail(rc, why);
  const BranchGeom g = branch_geom(dst->P, vm_pitch(dst->V));
  if ((int64_t)dst->N * g.chunks > 0x7fffffffLL) return fail(VMP_EINVAL, "vmp_branch: too many envs for one launch");
  const SnapLayout l(src);  // sizes of src's three arrays
  if (dst == src && !dst->br_stage)
    if (const hipError_t e = dev_malloc(&dst->br_stage, l.nh + l.np + l.nv); e != hipSuccess)
      return fail_hip("vmp_branch staging: ", e);
  uint8_t *mask = nullptr;  // null with no observer on
  if (const int rc = dst->ob.restart_mask(dst->prm, "vmp_branch mask: ", &mask)) return rc;
  BranchArgs a;
  std::memset(&a, 0, sizeof(a));
  a.src_hdr = reinterpret_cast<const uint4 *>(src->hdr);
  a.src_pm = reinterpret_cast<const uint4 *>(src->pm);
  a.src_vmw = reinterpret_cast<const uint4 *>(src->vmw);
  if (dst == src) {
    uint8_t *st = dst->br_stage;
    HIP_TRY(hipMemcpyAsync(st, src->hdr, l.nh, hipMemcpyDeviceToDevice, dst->stream));
    HIP_TRY(hipMemcpyAsync(st + l.nh, src->pm, l.np, hipMemcpyDeviceToDevice, dst->stream));
    HIP_TRY(hipMemcpyAsync(st + l.nh + l.np, src->vmw, l.nv, hipMemcpyDeviceToDevice, dst->stream));
    a.src_hdr = reinterpret_cast<const uint4 *>(st);
    a.src_pm = reinterpret_cast<const uint4 *>(st + l.nh);
    a.src_vmw = reinterpret_cast<const uint4 *>(st + l.nh + l.np);
  }
  a.dst_hdr = reinterpret_cast<uint4 *>(dst->hdr);
  a.dst_pm = reinterpret_cast<uint4 *>(dst->pm);
  a.dst_vmw = reinterpret_cast<uint4 *>(dst->vmw);
  a.src_of_dst = src_of_dst;
  a.seeds = seeds;
  a.mask = mask;
  a.src_n = src->N;
  a.dst_n = dst->N;
  a.pm_units = (int32_t)g.pm_units;
  a.vm_units = (int32_t)g.vm_units;
  a.units = (int32_t)g.units;
  a.chunks = (int32_t)g.chunks;
  hipLaunchKernelGGL(k_branch, dim3((unsigned)((int64_t)dst->N * g.chunks)), dim3(kBranchThreads), 0,
                     dst->stream, a);
  if (const int rc = launched()) return rc;
  // the observers of the overwritten envs restart from the new state
  return dst->ob.restart(dst->prm, dst->stream, mask);
}

// ---- set state: env states from the caller's arrays ----
// One launch (vmp_state.hip), a workgroup per env: validation and stores happen
// on the device; the host only refuses calls that cannot be launched
// (vmp_state.h). The observers of the imported envs restart through the mask
// the kernel writes, which vmp_branch shares.
int vmp_set_state(vmp_handle *h, const uint8_t *env_mask, const int64_t *placement,
                  const double *vm_cpu, const double *vm_mem, const int64_t *remaining,
                  const double *cpu, const double *mem, const int64_t *counters,
                  const double *totals, const int64_t *seeds, uint8_t *status) {
  StateCall c;
  std::memset(&c, 0, sizeof(c));
  c.handle = h;
  c.placement = placement, c.vm_cpu = vm_cpu, c.vm_mem = vm_mem, c.remaining = remaining;
  c.cpu = cpu, c.mem = mem;
  c.P = h ? h->P : 1;
  const char *why = nullptr;
  if (const int rc = state_check(&c, &why)) return fail(rc, why);
  uint8_t *mask = nullptr;  // null with no observer on
  if (const int rc = h->ob.restart_mask(h->prm, "vmp_set_state mask: ", &mask)) return rc;
  StateArgs a;
  std::memset(&a, 0, sizeof(a));
  a.hdr = h->hdr, a.pm = h->pm, a.vmw = h->vmw;
  a.env_mask = env_mask;
  a.placement = placement, a.vm_cpu = vm_cpu, a.vm_mem = vm_mem, a.remaining = remaining;
  a.cpu = cpu, a.mem = mem;
  a.counters = counters, a.totals = totals, a.seeds = seeds;
  a.status = status;
  a.imported = mask;
  a.N = h->N, a.P = h->P, a.V = h->V;
  hipLaunchKernelGGL(k_set_state, dim3((unsigned)h->N), dim3(kStateThreads),
                     (size_t)state_lds_bytes(h->P), h->stream, a);
  if (const int rc = launched()) return rc;
  // the observers of the imported envs restart from the new state
  return h->ob.restart(h->prm, h->stream, mask);
}

int64_t vmp_debug_live_allocs(void) { return g_live.load(); }

int vmp_debug_launch_order(vmp_handle *h, int32_t mode) {
  if (!h) return fail(VMP_EINVAL, "null handle");
  if (mode < kLoIndex || mode > kLoIdleLast) return fail(VMP_EINVAL, "launch order mode must be 0, 1 or 2");
  h->lo_mode = mode;
  return VMP_OK;
}

int vmp_debug_launch_map(vmp_handle *h, int32_t *env_of_block, uint8_t *flags_read) {
  if (!h || !env_of_block || !flags_read) return fail(VMP_EINVAL, "null argument");
  if (h->big) return fail(VMP_EINVAL, "the block kernel (V > 1024) keeps index order");
  EnvParams p = h->prm;
  p.pad0 = (int32_t)launch_order_word(h);
  hipLaunchKernelGGL(k_launch_map, dim3(h->N), dim3(64), 0, h->stream, p, env_of_block);
  if (const int rc = launched()) return rc;
  const size_t nb = (size_t)lo_flag_bytes(h->N);
  const uint8_t *flags = reinterpret_cast<const uint8_t *>(h->hdr + h->N) + nb * (h->lo_count & 1u);
  HIP_TRY(hipMemcpyAsync(flags_read, flags, nb, hipMemcpyDeviceToDevice, h->stream));
  return VMP_OK;
}

int vmp_debug_quiet_violations(int64_t *count) {
  if (!count) return fail(VMP_EINVAL, "null argument");
  const int64_t v = quiet_violations_take();
  if (v == -1) return fail(VMP_EINVAL, "library built without -DVMP_CHECK_QUIET");
  if (v < 0) return fail(VMP_EDEVICE, "vmp_debug_quiet_violations: device read failed");
  *count = v;
  return VMP_OK;
}

int vmp_debug_fail_alloc(int32_t n) {
  if (n < 0) return fail(VMP_EINVAL, "n must be >= 0");
  g_fail_alloc.store(n);
  return VMP_OK;
}

int vmp_debug_occupancy(vmp_handle *h, int32_t *blocks_per_cu, int32_t *lds_bytes) {
  if (!h || !blocks_per_cu || !lds_bytes) return fail(VMP_EINVAL, "null argument");
  if (!h->big) return fail(VMP_EINVAL, "occupancy query covers the block kernel (V > 1024) only");
  const int spt = big_spt(h->V);
  const size_t lds1 = launch_lds(h->prm, 1, true, spt);  // the per-step launch
  int st = 0;
  *blocks_per_cu = big_occupancy(spt, lds1, &st);
  *lds_bytes = (int32_t)lds1 + st;
  return VMP_OK;
}

int vmp_debug_stamps(vmp_handle *h, uint64_t *out) {
  if (!h || !out) return fail(VMP_EINVAL, "null argument");
  if (!h->stamps) return fail(VMP_EINVAL, "library built without -DVMP_STAMPS");
  HIP_TRY(hipMemcpyAsync(out, h->stamps, sizeof(uint64_t) * kStamps * (size_t)h->N,
                         hipMemcpyDeviceToDevice, h->stream));
  HIP_TRY(hipMemsetAsync(h->stamps, 0, sizeof(uint64_t) * kStamps * (size_t)h->N, h->stream));
  return VMP_OK;
}

}  // extern "C"
