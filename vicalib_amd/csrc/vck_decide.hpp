// vck_decide.hpp -- the step decision and the end of a pass: k_final, k_final_merged, k_wait_flag, k_signal_flag.
// k_final: fixed-order reduction of the step scalars + the accept/reject decision (device Ctrl).
// Kernel fragment: defines __global__ symbols, so it belongs to exactly ONE translation unit -- vc_kernels.hip, which includes the
// fragments in stage order.  Not one of the VC_HD arithmetic headers (vc_math.hpp, ..): host harnesses cannot include it.
#pragma once
#include <hip/hip_runtime.h>
#include "vc_math.hpp"
#include "vc_device.h"
#include "vc_kutil.hpp"
#include "vc_lm_rules.hpp"

namespace vc {

// ------------------------------------------------------------------------------------------ decision
// The Ceres trust-region bookkeeping (TrustRegionMinimizer + LevenbergMarquardtStrategy) and the
// reference's iteration callback (vicalibrator.h:690-721), run by one thread after every pass.
__device__ void trace_push(const DevView& v, Ctrl* c, const double* rec, bool writer = true) {
  if (writer && c->trace_len < c->trace_cap) {
    double* o = v.trace + (size_t)c->trace_len * kTraceCols;
    for (int i = 0; i < kTraceCols; ++i) o[i] = rec[i];
    if (v.host_progress && v.host_trace && c->trace_len < 64) {        // the host's copy (published by the progress word's store)
      double* ho = v.host_trace + (size_t)c->trace_len * kTraceCols;
      for (int i = 0; i < kTraceCols; ++i) ho[i] = rec[i];
    }
  }
  c->trace_len += 1;
  c->last_gnorm = rec[4];
}
// s: the frame-side step scalars of the judged pass, fail: a factorisation of that pass broke down, writer: this caller owns
// the global side effects (trace rows)
// t: the shared parameters' terms (k_reduced: scal[8..15]), R_cost: cost at the linearisation point (Sbuf's cost slot) -- nullptr / NaN-free
// defaults read them here; k_final's single-process path hands in what it requested at its entry
__device__ void lm_decide_local(const DevView& v, Ctrl* c, const double* s, bool fail, bool writer, const double* t_in = nullptr, const double* cost_in = nullptr) {
  const int D = v.D;
  const double* t = t_in ? t_in : v.scal + kNumScal;
  const double R_cost = cost_in ? *cost_in : v.Sbuf[(size_t)D * D + 3 * D];
  const double R_gd = s[kScGd] + t[kScGd], R_dld = s[kScDld] + t[kScDld];
  const double R_step2 = s[kScStep2] + t[kScStep2], R_x2 = s[kScX2] + t[kScX2];
  const double R_gnorm = sqrt(s[kScG2] + t[kScG2]), R_gmax = fmax(s[kScGmax], t[kScGmax]);
  const double R_new_cost = s[kScCost];
  c->passes += 1;
  c->likely_last = 0;
  c->res_sweeps += v.fused ? 0 : 1;
  c->jac_sweeps += (c->need_lin ? 1 : 0) + (v.fused ? 1 : 0);
  if (c->hold) { c->cost = R_cost; c->gmax = R_gmax; c->gnorm = R_gnorm; return; }
  if (c->pending) {            // the pass linearised at the newly accepted point
    c->cost = R_cost; c->gmax = R_gmax; c->gnorm = R_gnorm;
    c->pend[1] = R_cost; c->pend[3] = R_gmax; c->pend[4] = R_gnorm;
    trace_push(v, c, c->pend, writer);
    c->pending = 0;
    if (R_gmax <= c->gtol) { c->done = kDoneConvergence; return; }
  } else if (c->first) {
    c->cost = R_cost; c->gmax = R_gmax; c->gnorm = R_gnorm;
    const double rec[kTraceCols] = {0.0, R_cost, 0.0, R_gmax, R_gnorm, 0.0, 0.0, c->radius, 1.0, (double)c->stage};
    trace_push(v, c, rec, writer);
    c->first = 0; c->init_scale = 0;
    if (R_gmax <= c->gtol) { c->done = kDoneConvergence; return; }
  }
  c->init_scale = 0;
  // iteration callback (vicalibrator.h:690-721): ++num_iterations_, stop if 0 < |g| < LmRules::kCallbackGnorm
  c->num_callbacks += 1;
  if (c->last_gnorm > 0.0 && c->last_gnorm < LmRules::kCallbackGnorm) { c->done = kDoneUserSuccess; return; }
  if (c->iter >= c->max_iters) { c->done = kDoneNoConvergence; return; }
  c->iter += 1;
  double rec[kTraceCols] = {(double)c->iter, c->cost, 0.0, c->gmax, c->gnorm, 0.0, 0.0, c->radius, 0.0, (double)c->stage};
  const double model_change = -0.5 * R_gd + 0.5 * R_dld;
  if (fail || !(model_change > 0.0)) {
    c->invalid += 1;
    if (c->invalid >= LmRules::kMaxInvalid) { trace_push(v, c, rec, writer); c->done = kDoneFailure; return; }
    c->radius *= LmRules::kInvalidShrink; rec[7] = c->radius;
    trace_push(v, c, rec, writer);
    c->need_lin = 0; c->reuse_diag = 1;
    return;
  }
  c->invalid = 0;
  rec[5] = sqrt(R_step2);
  const double xnorm = sqrt(R_x2);
  if (rec[5] <= c->ptol * (xnorm + c->ptol)) { trace_push(v, c, rec, writer); c->done = kDoneConvergence; return; }
  rec[2] = c->cost - R_new_cost;
  if (fabs(rec[2]) < c->ftol * c->cost) { trace_push(v, c, rec, writer); c->done = kDoneConvergence; return; }
  rec[6] = rec[2] / model_change;
  if (rec[6] > LmRules::kMinRelativeDecrease) {
    {
      // convergence predictor for the feeding host (vc_solve.cpp: solve_once): quadratic-looking approach to the function tolerance
      const double rel = fabs(rec[2]) / c->cost;
      c->likely_last = (rel < 1e3 * c->ftol && rel < 0.1 * c->last_rel) ? 1 : 0;
      c->last_rel = rel;
    }
    c->cur = 1 - c->cur;
    const double q = 2.0 * rec[6] - 1.0;
    c->radius = fmin(LmRules::kMaxRadius, c->radius / fmax(1.0 / 3.0, 1.0 - q * q * q));
    c->decrease_factor = LmRules::kInitialDecrease;
    rec[7] = c->radius; rec[8] = 1.0;
    for (int i = 0; i < kTraceCols; ++i) c->pend[i] = rec[i];
    c->pending = 1; c->need_lin = v.fused ? 0 : 1; c->reuse_diag = 0;
  } else {
    c->radius = c->radius / c->decrease_factor; c->decrease_factor *= 2.0;
    rec[7] = c->radius;
    trace_push(v, c, rec, writer);
    if (c->radius < LmRules::kMinRadius) { c->done = kDoneConvergence; return; }
    c->need_lin = 0; c->reuse_diag = 1;
  }
}

// the host's view of the loop: one system-scope store per decision (vc_solve.cpp: solve_once feeds passes against it)
__device__ __forceinline__ void publish_progress(const DevView& v, const Ctrl& c) {
  if (v.host_progress) {
    // a finished solve: the record itself goes to the host's page-locked copy, then -- after a system-scope fence -- the progress word
    // says `done`; the host reads the result from there while the passes queued past the end drain (no copy, no synchronisation)
    // (the fence only then: it waits for the stores to host memory to be performed -- a round trip over the host link -- and the host
    //  reads the record and the trace rows only once it has seen `done`; the rows of earlier passes were completed by their kernels' ends)
    if (c.done && v.host_ctrl) { *v.host_ctrl = c; __threadfence_system(); }
    __hip_atomic_store(v.host_progress, ((unsigned long long)(unsigned)c.passes << 32) | (unsigned)c.done | (c.likely_last ? kProgressLikelyLast : 0u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
// void_pass: another rank of a sharded solve has marked this pass void (final_phase, mode 2) -- honoured whatever THIS rank's
// hand-over mode: a rank on events must withhold the decision the flag ranks withhold, or the ranks' states and collective
// schedules diverge
// Everything the deciding thread reads that this launch does not produce itself: the control record, the failure marks (set by the
// chain kernels of the main stream, long done), the shared parameters' terms and the linearisation cost (k_reduced).  One burst of loads.
struct DecideInputs { Ctrl c; double t[kNumScal]; double lin_cost; int f4, f5; };
__device__ __forceinline__ void load_decide_inputs(const DevView& v, DecideInputs* in) {
  in->c = *v.ctrl;
  in->f4 = v.flags[4 + 2 * v.par]; in->f5 = v.flags[5 + 2 * v.par];
#pragma unroll
  for (int k = 0; k < kNumScal; ++k) in->t[k] = v.scal[kNumScal + k];
  in->lin_cost = v.Sbuf[(size_t)v.D * v.D + 3 * v.D];
}
// s: the step scalars of the pass (v.scal, or registers of the launch that has just reduced them)
// marked: the sticky time-out word if the caller has read it already (behind its last wait), -1: read here
__device__ void lm_decide_with(const DevView& v, DecideInputs& in, bool void_pass, const double* s, long long marked = -1) {
  Ctrl& local = in.c;
  // device-flag hand-overs: a wait of this pass (or of one before it, noticed after that pass's decision) ran into its bound --
  // what this pass computed cannot be trusted.  No judgement: the record stays as the last valid decision left it, the solve ends
  // with kDoneSyncTimeout and the host resumes it with event hand-overs (vc_kutil.hpp: spin_until_flag)
  if (v.sync_seq > 0 && !void_pass) { const long long m = marked >= 0 ? marked : sync_marked(v); void_pass = m != 0 && m <= v.sync_seq; }
  if (void_pass) {
    local.done = kDoneSyncTimeout; local.abort_seq = (int)(v.pass_id & 0x7fffffff);      // (this pass is the first one without a decision; pass_id == sync_seq where flags are on)
    *v.ctrl = local;
    publish_progress(v, local);
    return;
  }
  const bool fail = (in.f4 != 0) || (in.f5 != 0);
  v.flags[4 + 2 * v.par] = 0; v.flags[5 + 2 * v.par] = 0;
  lm_decide_local(v, &local, s, fail, true, in.t, &in.lin_cost);
  *v.ctrl = local;
  publish_progress(v, local);
}
__device__ void lm_decide(const DevView& v, bool void_pass = false) {
  DecideInputs in;
  load_decide_inputs(v, &in);
  lm_decide_with(v, in, void_pass, v.scal);
}
// ---- merged decision --------------------------------------------------------------------------------------------
// The control record of the current pass from the previous pass's record: judge the pending trial point, or carry a finished
// state forward, or (first pass / after k_final_merged) take the record that is already in place.  All threads call it;
// `out` (LDS) holds the result after the trailing barrier; red: 8 x 4 doubles of LDS.  writer: this workgroup stores the
// record and the trace rows.
__device__ void merged_control(const DevView& v, Ctrl* out, double* red, bool writer) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const Ctrl* cp = v.ctrl_prev;
  // everything the decision may need is requested up front (the per-workgroup scalars, the previous record): one memory
  // latency instead of a chain of dependent ones
  const int nwg = (v.n_tiles + 3) / 4;
  double a[kNumScal];
#pragma unroll
  for (int k = 0; k < kNumScal; ++k) a[k] = 0.0;
  for (int i = tid; i < nwg; i += 256) {
#pragma unroll
    for (int k = 0; k < kNumScal; ++k) {
      const double x = v.wgpart[(size_t)i * kNumScal + k];
      a[k] = (k == kScGmax) ? fmax(a[k], x) : a[k] + x;
    }
  }
  Ctrl c;
  if (tid == 0) c = *cp;
  const int nd = cp->needs_decision, pdone = cp->done;       // wave-uniform
  if (nd) {
    // fixed-order sum of k_trial's per-workgroup scalars: every caller (each workgroup of k_frame_schur, k_final_merged)
    // gets bit-identical sums
#pragma unroll
    for (int k = 0; k < kNumScal; ++k) {
      double x = a[k];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) { const double y = __shfl_down(x, o, 64); x = (k == kScGmax) ? fmax(x, y) : x + y; }
      if (lane == 0) red[k * 4 + wave] = x;
    }
    __syncthreads();
    if (tid == 0) {
      double s[kNumScal];
#pragma unroll
      for (int k = 0; k < kNumScal; ++k)
        s[k] = (k == kScGmax) ? fmax(fmax(red[k * 4], red[k * 4 + 1]), fmax(red[k * 4 + 2], red[k * 4 + 3]))
                              : (red[k * 4] + red[k * 4 + 1]) + (red[k * 4 + 2] + red[k * 4 + 3]);
      bool fail;
      if (v.world > 1 || v.shard_src) {
        // sharded: the ranks' scalars (already halved costs, failure flags in slot kScSq) were gathered by the all-reduce
        for (int k = 0; k < kNumScal; ++k) {
          double a2 = 0.0;
          for (int r = 0; r < v.world; ++r) a2 = (k == kScGmax) ? fmax(a2, v.gath[r * kNumScal + k]) : a2 + v.gath[r * kNumScal + k];
          s[k] = a2;
        }
        fail = s[kScSq] > 0.0;
      } else {
        s[kScCost] *= 0.5;
        const int fp = 1 - v.par;                               // the judged pass ran with the other parity
        fail = (v.flags[4 + 2 * fp] != 0) || (v.flags[5 + 2 * fp] != 0);
      }
      lm_decide_local(v, &c, s, fail, writer);
      c.needs_decision = 0;
      *out = c;
      if (writer) { *v.ctrl = c; publish_progress(v, c); }
    }
  } else if (tid == 0) {
    if (pdone) { *out = c; if (writer) *v.ctrl = c; }
    else *out = *v.ctrl;
  }
  __syncthreads();
}
// batch end in merged mode: the last pass's trial point is judged here (the host reads the record this writes)
__global__ __launch_bounds__(256) void k_final_merged(DevView v) {
  __shared__ Ctrl c;
  __shared__ double red[kNumScal * 4];
  // here `ctrl` = record of the NEXT pass (to be written), `ctrl_prev` = record of the pass just run
  merged_control(v, &c, red, true);
  if (threadIdx.x == 0 && v.ctrl_prev->needs_decision) const_cast<Ctrl*>(v.ctrl_prev)->needs_decision = 0;
}
// mode 0: reduce + decide, 1: reduce only (an all-reduce follows), 2: decide only
__device__ void final_phase(const DevView& v, int mode, double* red) {
  const int tid = threadIdx.x;
  if (mode != 2) {
    double s[7] = {0, 0, 0, 0, 0, 0, 0};
    if (v.imu_on) {      // pre-reduced where they are produced (k_chain_back, k_reproj_jac / k_imu_jac in trial mode)
      // (unrolled: the loads of several rounds are in flight together -- one workgroup on the critical path, 49 rounds at 50 000 tiles)
#pragma unroll 4
      for (int g = tid; g < v.n_chain_groups; g += 256) {
        const double* p = v.grp_part + (size_t)g * kNumScal;
        s[0] += p[kScGd]; s[1] += p[kScDld]; s[2] += p[kScStep2]; s[3] += p[kScX2]; s[4] += p[kScG2];
        s[6] = fmax(s[6], p[kScGmax]);
      }
#pragma unroll 16
      for (int t = tid; t < (v.n_tiles + 3) / 4; t += 256) s[5] += v.wg_trial[t];
      if (v.final_wait > 0) {      // delivered by device-coherent stores while k_imu_jac still runs (see k_final)
#pragma unroll 4
        for (int t = tid; t < (v.n_frames - 1 + 7) / 8; t += 256) s[5] += __hip_atomic_load(v.wg_imu_trial + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
#pragma unroll 4
        for (int t = tid; t < (v.n_frames - 1 + 7) / 8; t += 256) s[5] += v.wg_imu_trial[t];
      }
    } else {
#pragma unroll 4
      for (int f = tid; f < v.n_frames; f += 256) {
        const double* p = v.fpart + (size_t)f * kNumScal;
        s[0] += p[kScGd]; s[1] += p[kScDld]; s[2] += p[kScStep2]; s[3] += p[kScX2]; s[4] += p[kScG2];
        s[6] = fmax(s[6], p[kScGmax]);
      }
#pragma unroll 16
      for (int t = tid; t < v.n_tiles; t += 256) s[5] += v.tile_trial[2 * t];
    }
    for (int k = 0; k < 7; ++k) red[k * 256 + tid] = s[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) {
        for (int k = 0; k < 6; ++k) red[k * 256 + tid] += red[k * 256 + tid + o];
        red[6 * 256 + tid] = fmax(red[6 * 256 + tid], red[6 * 256 + tid + o]);
      }
      __syncthreads();
    }
#ifdef VC_FINAL_STAMPS
    if (tid == 0) v.dbg[3] = (long long)__builtin_amdgcn_s_memrealtime();
#endif
    if (tid == 0) {
      double* o = v.scal;
      o[kScGd] = red[0]; o[kScDld] = red[256]; o[kScStep2] = red[512]; o[kScX2] = red[768]; o[kScG2] = red[1024];
      o[kScCost] = 0.5 * red[1280]; o[kScGmax] = red[1536]; o[kScSq] = 0.0;
      // sharded with flag hand-overs: a rank whose pass is marked void (vc_kutil.hpp) says so with kShardMark on top of its failure
      // count -- after the all-reduce every rank sees it and none of them judges the pass
      double mark = 0.0;
      if (mode == 1 && v.sync_seq > 0) { const long long m = sync_marked(v); if (m != 0 && m <= v.sync_seq) mark = kShardMark; }
      if (mode == 1) {       // sharded: publish this rank's terms (and its numeric-failure flags) in its slot of the gather table
        for (int r = 0; r < v.world; ++r)
          for (int k = 0; k < kNumScal; ++k) v.gath[r * kNumScal + k] = (r == v.rank) ? (k == kScSq ? (double)(v.flags[4 + 2 * v.par] + v.flags[5 + 2 * v.par]) + mark : o[k]) : 0.0;
      }
    }
  }
  bool void_pass = false;
  if (mode == 2 && tid == 0) {   // after the all-reduce: combine the ranks in fixed order, identically everywhere
    double* o = v.scal;
    for (int k = 0; k < kNumScal; ++k) {
      double a = 0.0;
      for (int r = 0; r < v.world; ++r) a = (k == kScGmax) ? fmax(a, v.gath[r * kNumScal + k]) : a + v.gath[r * kNumScal + k];
      o[k] = a;
    }
    // some rank's pass is void: this rank's is, too -- lm_decide below withholds the decision, on a rank that hands over through
    // events as well (ranks may disagree on the mode: a failed priority stream, a per-rank environment, a rank that fell back earlier)
    void_pass = o[kScSq] >= kShardMark;
    if (void_pass && v.sync_seq > 0) mark_sync_timeout(v, v.sync_seq);
    v.flags[4 + 2 * v.par] = (fmod(o[kScSq], kShardMark) > 0.0) ? 1 : 0; v.flags[5 + 2 * v.par] = 0;
  }
#ifdef VC_FINAL_STAMPS
  if (tid == 0) v.dbg[4] = (long long)__builtin_amdgcn_s_memrealtime();
#endif
  if (mode != 1 && tid == 0) lm_decide(v, void_pass);
}
// Single-process visual-inertial pass (k_final, mode 0): the same sums, arranged around the wait.  The main stream's terms -- the
// chain groups' step terms, the vision sweep's trial cost -- are reduced BEFORE the wait for the second stream's workgroup count
// (wave shuffles + one LDS exchange instead of an eight-level tree of barriers), the second stream's trial cost behind it, and the deciding
// thread takes the totals from registers.  Stamps (tools/final_stamps.py, round 4 form): 3.4 us reduction + 4.1 us decision behind the
// count, all of it on the critical path at the end of every pass.
__device__ void final_phase_vi(const DevView& v, double* red /* >= 40 */, bool counted, long long nwg_imu) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  // (the deciding thread's inputs: requested first, 2.4 us of round trips that used to follow the last barrier)
  DecideInputs din;
  if (tid == 0) load_decide_inputs(v, &din);
  double s[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll 4
  for (int g = tid; g < v.n_chain_groups; g += 256) {
    const double* p = v.grp_part + (size_t)g * kNumScal;
    s[0] += p[kScGd]; s[1] += p[kScDld]; s[2] += p[kScStep2]; s[3] += p[kScX2]; s[4] += p[kScG2];
    s[6] = fmax(s[6], p[kScGmax]);
  }
#pragma unroll 16
  for (int t = tid; t < (v.n_tiles + 3) / 4; t += 256) s[5] += v.wg_trial[t];
#pragma unroll
  for (int k = 0; k < 6; ++k) s[k] = wave_sum(s[k]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s[6] = fmax(s[6], __shfl_down(s[6], o, 64));
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 7; ++k) red[wave * 8 + k] = s[k];
  }
#ifdef VC_FINAL_STAMPS
  if (tid == 0) v.dbg[8] = (long long)__builtin_amdgcn_s_memrealtime();
#endif
  if (counted && tid == 0) {
    // the count is a running one (never reset inside a solve: a reset could race with workgroups still adding); this kernel keeps
    // the count at the end of the last judged pass in sync_flags[5]
    const long long base = __hip_atomic_load(v.sync_flags + 5, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    spin_until_flag(v, 4, base + nwg_imu);
    __hip_atomic_store(v.sync_flags + 5, base + nwg_imu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // the next pass counts on from here
  }
  __syncthreads();
  // (the sticky time-out word: behind this launch's last wait that could set it, requested together with the second stream's costs)
  const long long marked = (tid == 0 && v.sync_seq > 0) ? sync_marked(v) : 0;
  double b = 0.0;
  if (v.final_wait > 0) {      // delivered by device-coherent stores while k_imu_jac still runs (see k_final)
#pragma unroll 4
    for (int t = tid; t < (v.n_frames - 1 + 7) / 8; t += 256) b += __hip_atomic_load(v.wg_imu_trial + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
#pragma unroll 4
    for (int t = tid; t < (v.n_frames - 1 + 7) / 8; t += 256) b += v.wg_imu_trial[t];
  }
  b = wave_sum(b);
  if (lane == 0) red[32 + wave] = b;
#ifdef VC_FINAL_STAMPS
  if (tid == 0) { v.dbg[3] = (long long)__builtin_amdgcn_s_memrealtime(); }
#endif
  __syncthreads();
  if (tid == 0) {
#ifdef VC_FINAL_STAMPS
    v.dbg[4] = (long long)__builtin_amdgcn_s_memrealtime();
#endif
    double o[kNumScal];
    const int idx[6] = {kScGd, kScDld, kScStep2, kScX2, kScG2, kScCost};
#pragma unroll
    for (int k = 0; k < 6; ++k) o[idx[k]] = (red[k] + red[8 + k]) + (red[16 + k] + red[24 + k]);
    o[kScCost] = 0.5 * (o[kScCost] + ((red[32] + red[33]) + (red[34] + red[35])));
    o[kScGmax] = fmax(fmax(red[6], red[14]), fmax(red[22], red[30])); o[kScSq] = 0.0;
#pragma unroll
    for (int k = 0; k < kNumScal; ++k) v.scal[k] = o[k];      // (parity hooks read them)
#ifdef VC_FINAL_STAMPS
    v.dbg[9] = (long long)__builtin_amdgcn_s_memrealtime();
#endif
    lm_decide_with(v, din, false, o, marked);
#ifdef VC_FINAL_STAMPS
    v.dbg[10] = (long long)__builtin_amdgcn_s_memrealtime();
#endif
  }
}
// The waiting side as a kernel of its own: one wavefront on the second stream; the kernels behind it in that stream start when it
// returns (vc_kutil.hpp: spin_until_flag).
__global__ __launch_bounds__(64) void k_wait_flag(DevView v, int idx, long long seq) {
  if (threadIdx.x == 0) spin_until_flag(v, idx, seq);
}
// the producing side for kernels of many workgroups: a one-thread kernel behind them in their stream (the kernel boundary has
// written their results back; one fence per workgroup would cost more than this launch)
__global__ __launch_bounds__(64) void k_signal_flag(DevView v, int idx) {
  if (threadIdx.x == 0) signal_flag(v, idx);
}
#ifdef VC_FINAL_STAMPS
#define FSTAMP(i) do { if (threadIdx.x == 0 && !over_) v.dbg[i] = (long long)__builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define FSTAMP(i) do { } while (0)
#endif
__global__ __launch_bounds__(256) void k_final(DevView v, int mode) {
  __shared__ double red[256 * 7];
#ifdef VC_FINAL_STAMPS
  const long long fs0_ = (long long)__builtin_amdgcn_s_memrealtime();
#endif
  // the second stream's share of the trial cost (k_imu_jac's workgroup sums): wait for its flag here, inside the kernel, instead of
  // behind a cross-stream event (12 us between the second stream's last kernel and this one on the timeline); every wavefront
  // then drops what it may have cached of the other stream's results.  Also when the solve is over: the main stream must not
  // run ahead of the second one.
  //
  // Two waits: (1) for the count of k_imu_jac's workgroups that have delivered their share of the trial cost -- the decision is
  // taken while that kernel still writes its records; (2) at the very end, for the flag behind that kernel (k_signal_flag on the
  // second stream): this kernel must not end before the second stream's results are complete and written back -- the next pass's
  // k_chain_init reads them, and a solve that is over must leave nothing running.
  // Sharded (mode 1: reduce, all-reduce, mode 2: decide): the first wait belongs to the reducing launch, the second wait and the
  // flag to the deciding one.
  const bool over = v.ctrl->done != 0;
  [[maybe_unused]] const bool over_ = over;
#ifdef VC_FINAL_STAMPS
  if (threadIdx.x == 0 && !over) v.dbg[0] = fs0_;
#endif
  FSTAMP(1);
  __shared__ long long s_count_base;
  const long long nwg_imu = (long long)((v.n_frames - 1 + 7) / 8);
  const bool counted = v.final_wait > 0 && !over && v.n_frames > 1 && mode != 2;
  const bool vi_single = mode == 0 && v.imu_on && !over;      // the count is waited for inside final_phase_vi, behind the main stream's sums
  if (counted && !vi_single) {
    // the count is a running one (never reset inside a solve: a reset could race with workgroups still adding); this kernel keeps
    // the count at the end of the last judged pass in sync_flags[5]
    if (threadIdx.x == 0) {
      s_count_base = __hip_atomic_load(v.sync_flags + 5, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      spin_until_flag(v, 4, s_count_base + nwg_imu);
      __hip_atomic_store(v.sync_flags + 5, s_count_base + nwg_imu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // the next pass counts on from here
    }
    __syncthreads();
  }
  FSTAMP(2);
  if (vi_single) final_phase_vi(v, red, counted, nwg_imu);
  else if (!over) final_phase(v, mode, red);
  if (mode == 1) return;
  FSTAMP(5);
  __syncthreads();
  if (v.final_wait > 0 && v.n_frames > 1) {
    // the second stream's records are complete: every workgroup of k_imu_jac(trial) has counted itself a second time behind its
    // (device-coherent) stores -- a running count like the first, this kernel's book-keeping in sync_flags[12].  Also when the solve is
    // over (the workgroups count themselves at their exit): the main stream must not run ahead of the second one into the next solve.
    if (threadIdx.x == 0) {
      const long long base = __hip_atomic_load(v.sync_flags + 12, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      spin_until_flag(v, 11, base + nwg_imu);
      __hip_atomic_store(v.sync_flags + 12, base + nwg_imu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
  }
  FSTAMP(6);
  // (a pass that has been marked void still signals: the next pass's waiters return at once anyway, and the host takes over)
  if (threadIdx.x == 0) signal_flag(v, 0);
  FSTAMP(7);
}

}  // namespace vc
