// vmp_observers.h — the host side of the three device observers a handle can run
// behind a step: the Record metrics (vmp_record.hip), the per-request outcome log
// (vmp_reqlog.hip) and the per-step time series (vmp_series.hip). Their state is one
// member of vmp_handle; every operation takes the handle's EnvParams (N, P, V and the
// env arrays) and its stream. Host only, included by vmp_capi.cpp alone.
#pragma once
#include <initializer_list>
#include <utility>

#include "vmp_carve.h"
#include "vmp_host.h"
#include "vmp_record.h"
#include "vmp_reqlog.h"
#include "vmp_series.h"

namespace vmp {

// All-or-nothing device allocation: add() allocates into *p and registers it, doing
// nothing once one has failed; done() keeps the set, or frees and nulls everything
// registered and fails with the first error behind the caller's prefix.
struct Staged {
  void **slot[9];
  int n = 0;
  hipError_t err = hipSuccess;
  template <class T>
  void add(T **p, size_t bytes) {
    if (err == hipSuccess && (err = dev_malloc(p, bytes)) == hipSuccess)
      slot[n++] = reinterpret_cast<void **>(p);
  }
  int done(const char *who) {
    if (err == hipSuccess) return VMP_OK;
    for (int i = 0; i < n; i++) dev_free(std::exchange(*slot[i], nullptr));
    return fail_hip(who, err);
  }
};

inline void dev_free_all(std::initializer_list<void *> bufs) {
  for (void *b : bufs) dev_free(b);
}

// Zero-initialised by vmp_create's memset: everything off, nothing allocated.
struct Observers {
  // eval-mode Record metrics (vmp_record.hip), allocated by vmp_record_enable
  bool rec_on;
  RecArgs rec;
  // per-request outcome log (vmp_reqlog.hip), allocated by vmp_reqlog_enable
  bool rq_on;
  ReqArgs rq;
  // per-step time series (vmp_series.hip), allocated by vmp_series_enable
  bool sr_on;
  SerArgs sr;
  // scratch action / validity where the caller passes none: the recorder and the
  // log share them, whichever is enabled first allocates, the last one off frees
  int32_t *act;
  uint8_t *valid;
  // scratch reward where the caller passes none: the recorder's, and the series',
  // which steps on the reward alone
  double *rec_reward, *sr_reward;
  // the envs a vmp_branch / vmp_set_state overwrote, whose observers restart;
  // allocated on first use (restart_mask)
  uint8_t *mask;

  bool any() const { return rec_on || rq_on || sr_on; }

  // ---- (re)start the observers of the envs flagged in env_mask (device, null = all) ----
  int record_init(const EnvParams &p, hipStream_t s, const uint8_t *env_mask) const {
    size_t n = (size_t)p.N * p.V;
    if ((size_t)p.N * 2 * VMP_REC_BINS > n) n = (size_t)p.N * 2 * VMP_REC_BINS;
    if ((size_t)p.N * VMP_NREC > n) n = (size_t)p.N * VMP_NREC;
    hipLaunchKernelGGL(k_record_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, rec, env_mask);
    return launched();
  }
  int reqlog_init(const EnvParams &p, hipStream_t s, const uint8_t *env_mask) const {
    const int64_t rows = rq.cap * VMP_RQ_NF;
    const int64_t n = (int64_t)p.N * (rows > p.V ? rows : p.V);
    const int64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_reqlog_init, dim3((unsigned)(blocks < (1 << 20) ? blocks : (1 << 20))), dim3(256),
                       0, s, p, rq, env_mask);
    return launched();
  }
  int series_init(const EnvParams &p, hipStream_t s, const uint8_t *env_mask) const {
    const int64_t per = sr.pm && 2 * (int64_t)p.P > VMP_SR_NF ? 2 * (int64_t)p.P : VMP_SR_NF;
    const int64_t n = (int64_t)p.N * sr.cap * per;
    const int64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_series_init, dim3((unsigned)(blocks < (1 << 20) ? blocks : (1 << 20))), dim3(256),
                       0, s, p, sr, env_mask);
    return launched();
  }
  // every writer of env state ends here: vmp_reset (the envs it resets), vmp_restore
  // (all: no observer is part of a snapshot), vmp_branch and vmp_set_state (mask)
  int restart(const EnvParams &p, hipStream_t s, const uint8_t *env_mask) const {
    if (rec_on)
      if (const int rc = record_init(p, s, env_mask)) return rc;
    if (rq_on)
      if (const int rc = reqlog_init(p, s, env_mask)) return rc;
    return sr_on ? series_init(p, s, env_mask) : VMP_OK;
  }
  // the N-byte mask a kernel that overwrites envs fills for restart(), null (and
  // VMP_OK) with no observer on; `who` prefixes the text of a failed allocation
  int restart_mask(const EnvParams &p, const char *who, uint8_t **out) {
    if (any() && !mask)
      if (const hipError_t e = dev_malloc(&mask, (size_t)p.N); e != hipSuccess) return fail_hip(who, e);
    *out = any() ? mask : nullptr;
    return VMP_OK;
  }

  // ---- the step ----
  // k_series where its static LDS holds the env, else k_series_lds on a private carve
  static bool series_wave(const EnvParams &p) { return p.V <= kMaxVPT * kWaveSize && p.P <= 1024; }
  // k_series_lds's dynamic LDS: carve_target_means' regions in q, then the used-PM bitmap
  static size_t series_lds(const EnvParams &p, EnvParams &q, int32_t *off_used) {
    q = p;
    *off_used = (int32_t)align16((int64_t)carve_target_means(q));
    return (size_t)*off_used + sizeof(uint64_t) * (size_t)((p.P + 63) / 64);
  }
  int launch_series(const EnvParams &p, hipStream_t s, const double *reward) const {
    SerArgs a = sr;
    a.reward = reward;
    if (series_wave(p)) {
      hipLaunchKernelGGL(k_series, dim3((p.N + 3) / 4), dim3(256), 0, s, p, a);
      return launched();
    }
    EnvParams q;
    const size_t lds = series_lds(p, q, &a.off_used);
    hipLaunchKernelGGL(k_series_lds, dim3(p.N), dim3(64), lds, s, q, a);
    return launched();
  }
  // One step, launch_env(o), and behind it the observers that are on: the recorder,
  // the request log, the time series. The recorder and the log need the step's actions
  // and validity flags, the recorder and the series its reward; each steps on the
  // handle's scratch where the caller passes no buffer. The series asks for no actions
  // or validity on its account, so a handle with nothing else on keeps the step
  // kernel's idle path. No allocation, copy or synchronisation here.
  template <class LaunchEnv>
  int step(const EnvParams &p, hipStream_t s, StepOut o, LaunchEnv launch_env) const {
    if (rec_on || rq_on) {
      if (!o.actions && !o.act_out) o.act_out = act;
      if (!o.valid) o.valid = valid;
    }
    if (!o.reward) o.reward = sr_on ? sr_reward : rec_on ? rec_reward : nullptr;
    if (const int rc = launch_env(o)) return rc;
    if (rec_on) {
      RecArgs r = rec;
      r.act = o.actions ? o.actions : o.act_out;
      r.valid = o.valid;
      r.reward = o.reward;
      const size_t lds = (size_t)4 * ((p.P + 63) / 64) * sizeof(unsigned long long);
      hipLaunchKernelGGL(k_record, dim3((p.N + 3) / 4), dim3(256), lds, s, p, r);
      if (const int rc = launched()) return rc;
    }
    if (rq_on) {
      ReqArgs q = rq;
      q.act = o.actions ? o.actions : o.act_out;
      q.valid = o.valid;
      hipLaunchKernelGGL(k_reqlog, dim3((p.N + 3) / 4), dim3(256), 0, s, p, q);
      if (const int rc = launched()) return rc;
    }
    return sr_on ? launch_series(p, s, o.reward) : VMP_OK;
  }

  // ---- enable / disable, info, read ----
  // Each enable stages a new set and commits it: on any failure the handle, and the
  // observer it had, stay as they were. Each buffer list stands once where it is
  // allocated and once where it is freed. Queued launches write an observer's buffers,
  // so the stream is synchronised before a live set is freed, and nowhere else.
  void scratch_add(const EnvParams &p, Staged &st) {
    const size_t nv = (size_t)p.N * p.V;
    if (!act) st.add(&act, sizeof(int32_t) * nv);
    if (!valid) st.add(&valid, nv);
  }
  void scratch_release() {  // once neither the recorder nor the log steps on it
    if (rec_on || rq_on) return;
    dev_free(std::exchange(act, nullptr));
    dev_free(std::exchange(valid, nullptr));
  }

  int record_enable(const EnvParams &p, hipStream_t s, int32_t on) {
    if (!on) {
      if (rec_on) (void)hipStreamSynchronize(s);
      dev_free_all({rec.prev, rec.life_n, rec.alloc, rec.waits, rec.hist, rec.sums});
      dev_free(std::exchange(rec_reward, nullptr));
      rec = RecArgs{};
      rec_on = false;
      scratch_release();
      return VMP_OK;
    }
    if (!rec.prev) {  // else the recorder it has restarts
      const size_t nv = (size_t)p.N * p.V;
      RecArgs r{};
      Staged st;
      st.add(&r.prev, sizeof(uint16_t) * nv);
      st.add(&r.life_n, sizeof(uint32_t) * nv);
      st.add(&r.alloc, sizeof(int32_t) * nv);
      st.add(&r.waits, sizeof(uint32_t) * nv);
      st.add(&r.hist, sizeof(uint32_t) * (size_t)p.N * 2 * VMP_REC_BINS);
      st.add(&r.sums, sizeof(double) * (size_t)p.N * VMP_NREC);
      scratch_add(p, st);
      st.add(&rec_reward, sizeof(double) * (size_t)p.N);
      if (const int rc = st.done("vmp_record_enable: ")) return rc;
      rec = r;
    }
    if (const int rc = record_init(p, s, nullptr)) return rc;
    rec_on = true;
    return VMP_OK;
  }
  int record_read(const EnvParams &p, hipStream_t s, uint32_t *hist, double *sums) const {
    if (!rec_on) return fail(VMP_ESTATE, "recording is not enabled (vmp_record_enable)");
    HIP_TRY(hipMemcpyAsync(hist, rec.hist, sizeof(uint32_t) * (size_t)p.N * 2 * VMP_REC_BINS,
                           hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(sums, rec.sums, sizeof(double) * (size_t)p.N * VMP_NREC,
                           hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_record_close, dim3((p.N + 3) / 4), dim3(256), 0, s, p, rec, hist, sums);
    return launched();
  }

  // capacity 0 is "off": the new set is the empty one
  int reqlog_enable(const EnvParams &p, hipStream_t s, int64_t capacity) {
    if (capacity < 0) return fail(VMP_EINVAL, "vmp_reqlog_enable: capacity must be >= 0");
    ReqArgs q{};
    if (capacity > 0) {
      ReqlogSizes sz;
      if (const char *why = reqlog_sizes(p.N, p.V, capacity, &sz)) return fail(VMP_EINVAL, why);
      q.cap = capacity;
      Staged st;
      st.add(&q.rows, sz.rows);
      st.add(&q.ids, sz.ids);
      st.add(&q.prev, sz.prev);
      st.add(&q.meta, sz.meta);
      scratch_add(p, st);
      if (const int rc = st.done("vmp_reqlog_enable: ")) return rc;
    }
    if (rq_on) (void)hipStreamSynchronize(s);  // the log that goes
    dev_free_all({rq.rows, rq.ids, rq.prev, rq.meta});
    rq = q;
    rq_on = capacity > 0;
    if (rq_on) return reqlog_init(p, s, nullptr);
    scratch_release();
    return VMP_OK;
  }
  int reqlog_info(int64_t *capacity) const {
    *capacity = rq_on ? rq.cap : 0;
    return VMP_OK;
  }
  int reqlog_read(const EnvParams &p, hipStream_t s, int32_t *rows, int64_t *meta) const {
    if (!rq_on) return fail(VMP_ESTATE, "the request log is not enabled (vmp_reqlog_enable)");
    ReqlogSizes sz;
    if (const char *why = reqlog_sizes(p.N, p.V, rq.cap, &sz)) return fail(VMP_EINVAL, why);
    if (rows) {
      HIP_TRY(hipMemcpyAsync(rows, rq.rows, sz.rows, hipMemcpyDeviceToDevice, s));
      // WAIT_STEPS of the VMs waiting now is kept open on the device: closed in the copy
      hipLaunchKernelGGL(k_reqlog_close, dim3((p.N + 3) / 4), dim3(256), 0, s, p, rq, rows);
      if (const int rc = launched()) return rc;
    }
    if (meta) HIP_TRY(hipMemcpyAsync(meta, rq.meta, sz.meta, hipMemcpyDeviceToDevice, s));
    return VMP_OK;
  }

  // capacity 0 is "off" likewise; the scratch reward lasts from the first enable until then
  int series_enable(const EnvParams &p, hipStream_t s, int64_t capacity, int32_t stride, int32_t pm_rows) {
    if (capacity < 0) return fail(VMP_EINVAL, "vmp_series_enable: capacity must be >= 0");
    SerArgs a{};
    if (capacity > 0) {
      SeriesSizes sz;
      if (const char *why = series_sizes(p.N, p.P, capacity, stride, pm_rows, &sz)) return fail(VMP_EINVAL, why);
      EnvParams q;
      int32_t off = 0;
      if (!series_wave(p) && series_lds(p, q, &off) > (size_t)64 * 1024)
        return fail(VMP_EINVAL, "vmp_series_enable: config too large for the series kernel's LDS");
      a.cap = capacity;
      a.stride = stride;
      Staged st;
      st.add(&a.rows, sz.rows);
      if (pm_rows) st.add(&a.pm, sz.pm);
      st.add(&a.meta, sz.meta);
      if (!sr_reward) st.add(&sr_reward, sz.reward);
      if (const int rc = st.done("vmp_series_enable: ")) return rc;
    }
    if (sr_on) (void)hipStreamSynchronize(s);  // the series that goes
    dev_free_all({sr.rows, sr.pm, sr.meta});
    sr = a;
    sr_on = capacity > 0;
    if (sr_on) return series_init(p, s, nullptr);
    dev_free(std::exchange(sr_reward, nullptr));
    return VMP_OK;
  }
  int series_info(int64_t *capacity, int32_t *stride, int32_t *pm_rows) const {
    if (capacity) *capacity = sr_on ? sr.cap : 0;
    if (stride) *stride = sr_on ? sr.stride : 0;
    if (pm_rows) *pm_rows = sr_on && sr.pm ? 1 : 0;
    return VMP_OK;
  }
  int series_read(const EnvParams &p, hipStream_t s, double *rows, float *pm, int64_t *meta) const {
    if (!sr_on) return fail(VMP_ESTATE, "the time series is not enabled (vmp_series_enable)");
    if (pm && !sr.pm) return fail(VMP_ESTATE, "the time series keeps no PM rows (pm_rows)");
    SeriesSizes sz;
    if (const char *why = series_sizes(p.N, p.P, sr.cap, sr.stride, sr.pm ? 1 : 0, &sz))
      return fail(VMP_EINVAL, why);
    if (rows) HIP_TRY(hipMemcpyAsync(rows, sr.rows, sz.rows, hipMemcpyDeviceToDevice, s));
    if (pm) HIP_TRY(hipMemcpyAsync(pm, sr.pm, sz.pm, hipMemcpyDeviceToDevice, s));
    if (meta) HIP_TRY(hipMemcpyAsync(meta, sr.meta, sz.meta, hipMemcpyDeviceToDevice, s));
    return VMP_OK;
  }
};

}  // namespace vmp
