// robustness.hip — the robustness sweep on gfx950: the audited closed loop under sensor noise and
// actuator disturbance, and the scan of the finished trajectories.
//
// k_robust_begin<Env> / k_robust_step<Env> have the shape of k_audit_begin / k_audit_step
// (certificate.hip): one env per lane, BLK lanes per block, no autoreset, a frozen env is never
// read or written again. They differ in what robustness.h adds: the applied action is the
// disturbed one, and the policy's next input obs_meas [E][D] is written beside the true
// observation. L noise levels x M paired trajectories are one batch of L * M envs: the
// disturbance is per env. k_robust_scan is one lane per env over coalesced time-major rows, like
// k_certificate_scan.
//
// No kernel has a spin wait, inter-block communication or an atomic; every loop is bounded by
// the compile-time D / A, by T or by n.
#include "robustness.h"
#include "rollout.h"

namespace mh {

template <class Env>
__global__ __launch_bounds__(BLK) void k_robust_begin(RobustArgs r) {
  constexpr int D = Env::D;
  const AuditArgs& a = r.a;
  const int64_t e = (int64_t)blockIdx.x * BLK + threadIdx.x;
  if (e >= a.E) return;
  float o[D], m[D];
  load_row<D>(a.obs + e * D, o);
  a.q_row[e] = audit_q<D>(o);
  if (a.traj_obs) store_row<D>(a.traj_obs + e * D, o);
  robust_measure<D>(r.d, e, 0, o, m);
  store_row<D>(r.obs_meas + e * D, m);
  a.len[e] = 0;
  a.status[e] = AUDIT_RUNNING;
  a.ret[e] = 0.0;
  a.cost[e] = 0.0;
}

template <class Env>
__global__ __launch_bounds__(BLK, 2) void k_robust_step(RobustArgs r) {
  constexpr int D = Env::D, A = Env::A, S = Env::S, XS = Env::XS;
  const AuditArgs& a = r.a;
  const int64_t E = a.E;
  const int64_t e = (int64_t)blockIdx.x * BLK + threadIdx.x;
  if (e >= E) return;
  if (a.status[e] != AUDIT_RUNNING) return;  // frozen: nothing of this env is read or written again
  const int k = a.steps[e];
  float s[S];
  double xs[XS > 0 ? XS : 1];
#pragma unroll
  for (int i = 0; i < S; ++i) s[i] = a.state[(int64_t)i * E + e];
#pragma unroll
  for (int i = 0; i < XS; ++i) xs[i] = a.xstate[(int64_t)i * E + e];
  float u[A];
  if (a.act_in) {  // the nominal action as given
    load_row<A>(a.act_in + e * A, u);
  } else {
    float lgt[2 * A];
    load_row<2 * A>(a.logits + e * 2 * A, lgt);
    audit_mode_action<Env>(lgt, u);
  }
  robust_actuate<Env>(r.d, e, (uint64_t)r.t, u);
  float obs2[D], q, rew;
  const int status = audit_env_step<Env>(s, xs, k, u, a.tab, obs2, &q, &rew);
  float m[D];
  robust_measure<D>(r.d, e, (uint64_t)r.t + 1, obs2, m);
#pragma unroll
  for (int i = 0; i < S; ++i) a.state[(int64_t)i * E + e] = s[i];
#pragma unroll
  for (int i = 0; i < XS; ++i) a.xstate[(int64_t)i * E + e] = xs[i];
  a.steps[e] = k + 1;
  store_row<D>(a.obs + e * D, obs2);
  store_row<D>(r.obs_meas + e * D, m);
  a.q_row[e] = q;
  if (a.traj_obs) store_row<D>(a.traj_obs + e * D, obs2);
  if (a.traj_act) store_row<A>(a.traj_act + e * A, u);
  a.len[e] = a.len[e] + 1;
  a.status[e] = status;
  a.ret[e] = a.ret[e] + (double)(rew * a.reward_scale);
  a.cost[e] = a.cost[e] + (double)(q * a.cost_scale);
}

__global__ __launch_bounds__(BLK) void k_robust_scan(RobustScanArgs a) {
  // the window's coefficients, staged once per block (every lane reads entry k at the same time)
  __shared__ float coef[CERT_MAX_N];
  if ((int)threadIdx.x < a.n) coef[threadIdx.x] = a.s[threadIdx.x];
  __syncthreads();
  const int64_t e = (int64_t)blockIdx.x * BLK + threadIdx.x;
  if (e >= a.E) return;
  RobustRow o;
  robust_scan_env(a.v, a.q, a.E, e, a.len[e], a.T, a.n, coef, a.W, a.settle_frac, a.ball_factor, &o);
  a.q_peak[e] = o.q_peak;
  a.t_peak[e] = o.t_peak;
  a.tail_max[e] = o.tail_max;
  a.tail_mean[e] = o.tail_mean;
  a.tail_count[e] = o.tail_count;
  a.settle[e] = o.settle;
  a.pairs_out[e] = o.pairs_out;
  a.viol_out[e] = o.viol_out;
  a.worst_out[e] = o.worst_out;
}

// --------------------------------------------------------------- launchers
template <class Env>
static hipError_t launch_robust_t(const RobustArgs& r, bool begin, hipStream_t st) {
  const AuditArgs& a = r.a;
  if (!robust_row_aligned(a.obs, Env::D) || !robust_row_aligned(r.obs_meas, Env::D) ||
      !robust_row_aligned(a.traj_obs, Env::D) || !robust_row_aligned(a.traj_act, Env::A) ||
      !robust_row_aligned(a.act_in, Env::A) || !robust_row_aligned(a.logits, 2 * Env::A))
    return hipErrorInvalidValue;
  if (a.E <= 0) return hipSuccess;
  const int grid = (int)((a.E + BLK - 1) / BLK);
  if (begin)
    k_robust_begin<Env><<<grid, BLK, 0, st>>>(r);
  else
    k_robust_step<Env><<<grid, BLK, 0, st>>>(r);
  return hipGetLastError();
}

static hipError_t launch_robust(int env_id, const RobustArgs& r, bool begin, hipStream_t st) {
  switch (env_id) {
    case ENV_VANDERPOL: return launch_robust_t<VanderPol>(r, begin, st);
    case ENV_PENDULUM: return launch_robust_t<Pendulum>(r, begin, st);
    case ENV_DUCTEDFAN: return launch_robust_t<DuctedFan>(r, begin, st);
    case ENV_TWOLINK: return launch_robust_t<TwoLink>(r, begin, st);
    case ENV_SINGLETRACKCAR: return launch_robust_t<SingleTrackCar>(r, begin, st);
    case ENV_QUADTRACKING: return launch_robust_t<QuadTracking>(r, begin, st);
  }
  return hipErrorInvalidValue;
}
hipError_t launch_robust_begin(int env_id, const RobustArgs& r, hipStream_t st) { return launch_robust(env_id, r, true, st); }
hipError_t launch_robust_step(int env_id, const RobustArgs& r, hipStream_t st) { return launch_robust(env_id, r, false, st); }

hipError_t launch_robust_scan(const RobustScanArgs& a, hipStream_t st) {
  if (a.E <= 0) return hipSuccess;
  k_robust_scan<<<(int)((a.E + BLK - 1) / BLK), BLK, 0, st>>>(a);
  return hipGetLastError();
}

}  // namespace mh
