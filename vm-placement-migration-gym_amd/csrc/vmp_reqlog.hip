// vmp_reqlog.hip — per-request outcome log on the device (include/vmp.h,
// vmp_reqlog_*): for every env one int32[VMP_RQ_NF] row per request offered
// since the env's last reset, updated after each logged step; no per-step host
// copies. A second observer beside the recorder (vmp_record.hip): it reads what
// k_record reads and touches no env state.
//
// A request's id is its ordinal among the requests offered to the env since
// its reset: the value of total_requests before the request is counted. On a
// traced env reset at step 0 that is the request's index in its trace, since
// a dropped request is consumed (vmp_set_trace). _accept_vm_requests
// (env.py:271-293) gives a step's first k requests to the k lowest NULL slots
// in ascending order, so the arrival in slot v is request
//   prev_total + (number of this step's arrival slots below v)
// and the step's other requests, prev_total + k .. total_requests - 1, were
// dropped. Arrivals are derived as k_record derives them: post-step placement
// WAIT, and neither a WAIT VM that stayed unplaced nor a running VM suspended
// this step. A VM that was running after the action phase and whose slot is
// NULL, or holds a new arrival, after the step finished in this step's
// _run_vms (env.py:244-268).
//
// Per slot the log keeps the id of the VM it holds (-1 = untracked: present
// before the log started, or an id at or above the capacity) and the previous
// post-step placement. A request row is written only by the lane that owns its
// slot (or, for a dropped id, by one lane of the tail loop): plain stores, no
// atomics, no LDS.
//
// WAIT_STEPS is kept open on the device. Counting every step that leaves a VM
// at WAIT would be one scattered read-modify-write per waiting VM and step
// (hundreds per env-step on a saturated workload, against a handful of
// arrivals, placements and finishes). Instead a stretch of waiting that begins
// in step s (the arrival, or a valid suspension) adds 1 - s to the field and
// the valid placement that ends it in step p adds p - 1: together p - s, the
// steps s .. p - 1 that left the VM at WAIT. Rows are then written at events
// only. While a VM waits, its true count is the stored value plus the t of the
// last step; vmp_reqlog_read adds that to its copy (k_reqlog_close), so a read
// always shows the counts as if they had been kept per step.
#include <hip/hip_runtime.h>

#include "../../include/vmp.h"
#include "vmp_layout.h"
#include "vmp_record.h"
#include "vmp_reqlog.h"

namespace vmp {

// One wave per env, after its step: the env's slots in rows of 64, every load
// coalesced and the five loads of a row issued together.
__global__ __launch_bounds__(256) void k_reqlog(EnvParams p, ReqArgs q) {
  const int lane = threadIdx.x & 63;
  const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= p.N) return;
  const int V = p.V, P = p.P, WAIT = p.P, NUL = p.P + 1;
  const int64_t cap = q.cap;
  int64_t *meta = q.meta + (int64_t)e * VMP_RQ_NMETA;
  // lane 0 reads the env's scalars (it alone rewrites them below)
  int64_t hv[3] = {0, 0, 0};
  if (lane == 0) {
    hv[0] = p.hdr[e].timestep;
    hv[1] = p.hdr[e].total_requests;
    hv[2] = meta[VMP_RQ_NEXT];
  }
  const int32_t t = (int32_t)(__shfl(hv[0], 0) - 1);  // the timestep the step started at
  const int64_t total = __shfl(hv[1], 0);
  const int64_t prev_total = __shfl(hv[2], 0);
  int32_t *rows = q.rows + (int64_t)e * cap * VMP_RQ_NF;
  const uint32_t *vmw = p.vmw + (int64_t)e * vm_pitch(V);
  const int64_t base = (int64_t)e * V;
  const unsigned long long below = (1ull << lane) - 1ull;
  int64_t next = prev_total;  // id of the next arrival slot (wave-uniform between rows)
  for (int v0 = 0; v0 < V; v0 += 64) {
    const int v = v0 + lane;
    const bool in = v < V;  // the last row may be partial
    uint32_t w = (uint32_t)NUL;
    int pv = NUL, a = -1, i = -1;
    bool ok = false;
    if (in) {
      w = vmw[vm_slot_idx(v)];
      pv = q.prev[base + v];
      i = q.ids[base + v];
      a = q.act[base + v];
      ok = q.valid[base + v] != 0;
    }
    const int st = (int)(w & 0xFFFFu);
    const bool placed = pv == WAIT && ok && a < P && a >= 0;
    const bool susp = pv < P && ok && a == WAIT;
    const bool arrival = in && st == WAIT && !(pv == WAIT && !placed) && !susp;
    if (i >= 0 && i < cap) {
      int32_t *r = rows + (int64_t)i * VMP_RQ_NF;
      if (placed) {  // the steps up to t - 1 left it at WAIT: close the stretch
        if (r[VMP_RQ_PLACED] == 0) r[VMP_RQ_PLACED] = t;
        r[VMP_RQ_WAIT_STEPS] += t - 1;
      }
      if (susp) {  // this step leaves it at WAIT: open a stretch
        r[VMP_RQ_SUSPENDS] += 1;
        r[VMP_RQ_WAIT_STEPS] += 1 - t;
      }
      const bool running = placed || (pv < P && !susp);  // after the action phase
      if (running && (st == NUL || arrival)) {
        r[VMP_RQ_FINISHED] = t;
        i = -1;
      }
    }
    const unsigned long long am = __ballot(arrival);
    if (arrival) {
      const int64_t id = next + __popcll(am & below);
      i = -1;  // an id the log cannot hold leaves the slot untracked
      if (id < cap) {
        i = (int32_t)id;
        int32_t *r = rows + id * VMP_RQ_NF;
        r[VMP_RQ_SLOT] = v;
        r[VMP_RQ_ARRIVED] = t;
        r[VMP_RQ_WAIT_STEPS] = 1 - t;  // an open stretch from this step on
      }
    }
    if (in) {
      q.ids[base + v] = i;
      q.prev[base + v] = (uint16_t)st;
    }
    next += __popcll(am);
  }
  // the step's other requests were dropped (and consumed)
  const int64_t end = total < cap ? total : cap;
  for (int64_t j = next + lane; j < end; j += 64) {
    rows[j * VMP_RQ_NF + VMP_RQ_SLOT] = -1;
    rows[j * VMP_RQ_NF + VMP_RQ_ARRIVED] = t;
  }
  if (lane == 0) {
    meta[VMP_RQ_NEXT] = total;
    meta[VMP_RQ_LOST] += reqlog_lost(prev_total, total, cap);
  }
}

// Read-out (after vmp_reqlog_read copied the rows into the caller's buffer):
// close the open waiting stretches in the copy; the log itself is untouched.
__global__ __launch_bounds__(256) void k_reqlog_close(EnvParams p, ReqArgs q, int32_t *rows) {
  const int lane = threadIdx.x & 63;
  const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= p.N) return;
  const int32_t last = (int32_t)(p.hdr[e].timestep - 1);  // t of the last step
  const int64_t base = (int64_t)e * p.V;
  int32_t *r = rows + (int64_t)e * q.cap * VMP_RQ_NF;
  for (int v = lane; v < p.V; v += 64) {
    const int i = q.ids[base + v];
    if (i >= 0 && i < q.cap && q.prev[base + v] == p.P) r[(int64_t)i * VMP_RQ_NF + VMP_RQ_WAIT_STEPS] += last;
  }
}

// Start the log of every env (of those flagged in env_mask) from the current
// state: no request observed, no slot tracked, previous placement = current,
// FIRST = NEXT = the env's total_requests.
__global__ void k_reqlog_init(EnvParams p, ReqArgs q, const uint8_t *env_mask) {
  const int64_t nrow = q.cap * VMP_RQ_NF;
  const int64_t span = nrow > p.V ? nrow : p.V;  // >= VMP_RQ_NMETA: cap >= 1
  const int64_t n = (int64_t)p.N * span;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
    const int64_t e = k / span, j = k - e * span;
    if (env_mask && !env_mask[e]) continue;
    if (j < nrow) q.rows[e * nrow + j] = j % VMP_RQ_NF == VMP_RQ_SLOT ? -2 : 0;
    if (j < p.V) {
      q.ids[e * p.V + j] = -1;
      q.prev[e * p.V + j] = (uint16_t)(p.vmw[e * vm_pitch(p.V) + vm_slot_idx((int)j)] & 0xFFFFu);
    }
    if (j < VMP_RQ_NMETA) q.meta[e * VMP_RQ_NMETA + j] = j == VMP_RQ_LOST ? 0 : p.hdr[e].total_requests;
  }
}

}  // namespace vmp
