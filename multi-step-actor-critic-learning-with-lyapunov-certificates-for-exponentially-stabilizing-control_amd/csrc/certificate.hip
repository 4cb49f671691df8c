// certificate.hip — closed-loop Lyapunov certificate audit on gfx950.
//
// k_audit_step<Env>: one lockstep of the deterministic closed loop, one env per lane, 256 envs per
// block like k_rollout, but WITHOUT autoreset: an env that terminates or truncates is frozen (its
// state, step counter, observation and accumulators are never written again), so a trajectory can
// be followed to its end and held. Trajectory columns are time-major ([T + 1][E]): each lockstep
// writes one coalesced row, and k_certificate_scan — one lane per env, one pass over t — reads
// coalesced rows. The per-env math is certificate.h, shared with the CPU build.
//
// Neither kernel has a spin wait, inter-block communication or an atomic; every loop is bounded by
// T or n.
#include "certificate.h"
#include "rollout.h"

namespace mh {

// mh_audit_begin after the reset: row 0 of the trajectory columns and the cleared accumulators
template <class Env>
__global__ __launch_bounds__(BLK) void k_audit_begin(AuditArgs a) {
  constexpr int D = Env::D;
  const int64_t e = (int64_t)blockIdx.x * BLK + threadIdx.x;
  if (e >= a.E) return;
  float o[D];
  load_row<D>(a.obs + e * D, o);
  a.q_row[e] = audit_q<D>(o);
  if (a.traj_obs) store_row<D>(a.traj_obs + e * D, o);
  a.len[e] = 0;
  a.status[e] = AUDIT_RUNNING;
  a.ret[e] = 0.0;
  a.cost[e] = 0.0;
}

template <class Env>
__global__ __launch_bounds__(BLK, 2) void k_audit_step(AuditArgs a) {
  constexpr int D = Env::D, A = Env::A, S = Env::S, XS = Env::XS;
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
  if (a.act_in) {  // parity mode: used as given
    load_row<A>(a.act_in + e * A, u);
  } else {
    float lgt[2 * A];
    load_row<2 * A>(a.logits + e * 2 * A, lgt);
    audit_mode_action<Env>(lgt, u);
  }
  float obs2[D], q, r;
  const int status = audit_env_step<Env>(s, xs, k, u, a.tab, obs2, &q, &r);
#pragma unroll
  for (int i = 0; i < S; ++i) a.state[(int64_t)i * E + e] = s[i];
#pragma unroll
  for (int i = 0; i < XS; ++i) a.xstate[(int64_t)i * E + e] = xs[i];
  a.steps[e] = k + 1;
  store_row<D>(a.obs + e * D, obs2);
  a.q_row[e] = q;
  if (a.traj_obs) store_row<D>(a.traj_obs + e * D, obs2);
  if (a.traj_act) store_row<A>(a.traj_act + e * A, u);
  a.len[e] = a.len[e] + 1;
  a.status[e] = status;
  a.ret[e] = a.ret[e] + (double)(r * a.reward_scale);
  a.cost[e] = a.cost[e] + (double)(q * a.cost_scale);
}

__global__ __launch_bounds__(BLK) void k_certificate_scan(ScanArgs a) {
  // the window's coefficients, staged once per block (every lane reads entry k at the same time)
  __shared__ float coef[3][CERT_MAX_N];
  if ((int)threadIdx.x < a.n) {
    coef[0][threadIdx.x] = a.c[threadIdx.x];
    coef[1][threadIdx.x] = a.w[threadIdx.x];
    coef[2][threadIdx.x] = a.s[threadIdx.x];
  }
  __syncthreads();
  const int64_t e = (int64_t)blockIdx.x * BLK + threadIdx.x;
  if (e >= a.E) return;
  // the window's last n values of V and q are re-read from the (L2-resident, coalesced) rows:
  // no runtime-indexed register array
  CertRow o;
  certificate_scan_env(a.v, a.q, a.E, e, a.len[e], a.T, a.n, coef[0], coef[1], coef[2], a.alpha1, a.alpha2, a.resid,
                       &o);
  a.lo_count[e] = o.lo_count;
  a.hi_count[e] = o.hi_count;
  a.pairs[e] = o.pairs;
  a.lya_viol[e] = o.lya_viol;
  a.esl_neg[e] = o.esl_neg;
  a.windows[e] = o.windows;
  a.lo_excess[e] = o.lo_excess;
  a.hi_excess[e] = o.hi_excess;
  a.lya_worst[e] = o.lya_worst;
  a.resid_sum[e] = o.resid_sum;
}

// --------------------------------------------------------------- launchers
static bool row_aligned(const void* p, int n) {
  const uintptr_t w = n % 4 == 0 ? 16 : (n % 2 == 0 ? 8 : 4);
  return p == nullptr || reinterpret_cast<uintptr_t>(p) % w == 0;
}

template <class Env>
static hipError_t launch_audit_t(const AuditArgs& a, bool begin, hipStream_t st) {
  if (!row_aligned(a.obs, Env::D) || !row_aligned(a.traj_obs, Env::D) || !row_aligned(a.traj_act, Env::A) ||
      !row_aligned(a.act_in, Env::A) || !row_aligned(a.logits, 2 * Env::A))
    return hipErrorInvalidValue;
  const int grid = (int)((a.E + BLK - 1) / BLK);
  if (begin)
    k_audit_begin<Env><<<grid, BLK, 0, st>>>(a);
  else
    k_audit_step<Env><<<grid, BLK, 0, st>>>(a);
  return hipGetLastError();
}

static hipError_t launch_audit(int env_id, const AuditArgs& a, bool begin, hipStream_t st) {
  switch (env_id) {
    case ENV_VANDERPOL: return launch_audit_t<VanderPol>(a, begin, st);
    case ENV_PENDULUM: return launch_audit_t<Pendulum>(a, begin, st);
    case ENV_DUCTEDFAN: return launch_audit_t<DuctedFan>(a, begin, st);
    case ENV_TWOLINK: return launch_audit_t<TwoLink>(a, begin, st);
    case ENV_SINGLETRACKCAR: return launch_audit_t<SingleTrackCar>(a, begin, st);
    case ENV_QUADTRACKING: return launch_audit_t<QuadTracking>(a, begin, st);
  }
  return hipErrorInvalidValue;
}
hipError_t launch_audit_begin(int env_id, const AuditArgs& a, hipStream_t st) { return launch_audit(env_id, a, true, st); }
hipError_t launch_audit_step(int env_id, const AuditArgs& a, hipStream_t st) { return launch_audit(env_id, a, false, st); }

hipError_t launch_certificate_scan(const ScanArgs& a, hipStream_t st) {
  if (a.E <= 0) return hipSuccess;
  k_certificate_scan<<<(int)((a.E + BLK - 1) / BLK), BLK, 0, st>>>(a);
  return hipGetLastError();
}

}  // namespace mh
