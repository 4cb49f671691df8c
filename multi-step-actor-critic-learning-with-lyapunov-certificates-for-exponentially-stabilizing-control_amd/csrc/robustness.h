// robustness.h — per-env expressions of the robustness sweep: the audited closed loop
// (certificate.h) under sensor noise and actuator disturbance, and the scan that turns the
// finished trajectories into robustness numbers. Shared by the gfx950 kernels (robustness.hip)
// and the engine's CPU build (host_engine.hip), as certificate.h is.
//
// Both disturbances act AROUND the unchanged Env::step:
//   sensor    the policy's input is obs_meas[i] = obs[i] + (obs_sigma[e] * obs_weight[i]) * xi_i;
//             the true observation is what is stepped, scored (q, cost, termination) and stored
//   actuator  u_i = clip(u_nom_i + half_i * (act_bias[e][i] + act_sigma[e] * zeta_i), lo_i, hi_i),
//             half_i = (hi_i - lo_i) / 2, u_nom the clipped mode of the logits (or act_in as given)
// All float32, the operations separate and in the order written. xi / zeta are standard normals of
// make_rng(seed, noise_id[e], tick).normal4f(stream, .): stream 16 + i / 4 for xi, 24 + i / 4 for
// zeta (ids no other draw of the engine uses); tick 0 in begin, t for step t's action, t + 1 for
// the observation step t produces. An env whose sigma is 0 skips the draw: its obs_meas row is
// the true row bit for bit.
#pragma once

#include "certificate.h"
#include "philox.h"

namespace mh {

constexpr uint32_t ROBUST_STREAM_OBS = 16;  // + i / 4, i < D <= 16: 16..19
constexpr uint32_t ROBUST_STREAM_ACT = 24;  // + i / 4, i < A <= 4: 24

// mh_disturbance_t (msacl_hip.h); every pointer nullable
struct Disturb {
  const float* obs_sigma;   // [E], null: 0
  const float* obs_weight;  // [D], null: 1
  const float* act_sigma;   // [E], null: 0
  const float* act_bias;    // [E][A], null: 0
  const int32_t* noise_id;  // [E], null: e
  uint64_t seed;
};

MH_HD uint64_t robust_noise_id(const Disturb& d, int64_t e) {
  return d.noise_id ? (uint64_t)(int64_t)d.noise_id[e] : (uint64_t)e;
}

// The policy's input for the true observation obs, drawn at `tick`
template <int D>
MH_HD void robust_measure(const Disturb& d, int64_t e, uint64_t tick, const float* obs, float* meas) {
  const float sg = d.obs_sigma ? d.obs_sigma[e] : 0.0f;
  if (sg == 0.0f) {
#pragma unroll
    for (int i = 0; i < D; ++i) meas[i] = obs[i];
    return;
  }
  const Rng rng = make_rng(d.seed, robust_noise_id(d, e), tick);
#pragma unroll
  for (int i0 = 0; i0 < D; i0 += 4) {
    float xi[4];
    rng.normal4f(ROBUST_STREAM_OBS + (uint32_t)(i0 / 4), xi);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = i0 + j;
      if (i < D) {
        const float w = d.obs_weight ? d.obs_weight[i] : 1.0f;
        const float amp = sg * w;
        meas[i] = obs[i] + amp * xi[j];
      }
    }
  }
}

// The applied action from the nominal one, in place, drawn at `tick`. Without act_sigma and
// act_bias the nominal action is left as it is (not even clipped: the audit's own step).
template <class Env>
MH_HD void robust_actuate(const Disturb& d, int64_t e, uint64_t tick, float* u) {
  constexpr int A = Env::A;
  const float sg = d.act_sigma ? d.act_sigma[e] : 0.0f;
  if (sg == 0.0f && !d.act_bias) return;
  float zeta[(A + 3) / 4 * 4];
  if (sg != 0.0f) {
    const Rng rng = make_rng(d.seed, robust_noise_id(d, e), tick);
#pragma unroll
    for (int i0 = 0; i0 < A; i0 += 4) rng.normal4f(ROBUST_STREAM_ACT + (uint32_t)(i0 / 4), zeta + i0);
  }
#pragma unroll
  for (int i = 0; i < A; ++i) {
    const float lo = Env::act_lo(i), hi = Env::act_hi(i);
    const float half = (hi - lo) / 2.0f;
    float b = d.act_bias ? d.act_bias[e * A + i] : 0.0f;
    if (sg != 0.0f) b = b + sg * zeta[i];
    const float v = u[i] + half * b;
    u[i] = fminf(fmaxf(v, lo), hi);
  }
}

// One env's row of mh_robust_out_t
struct RobustRow {
  float q_peak, tail_max, worst_out;
  double tail_mean;
  int32_t t_peak, tail_count, settle, pairs_out, viol_out;
};

// Robustness numbers of env e's trajectory: v / q are the audit's time-major [T + 1][E] columns,
// valid for t = 0..len (rows beyond len are never read); s is the algorithm's start_lya_coef [n].
//   q_peak / t_peak       max of q_t / its first argmax
//   tail_*                over rows max(0, len - W + 1)..len: max, float64 sum / count, count
//   settle                0 if no q_t > settle_frac * q_0, else 1 + the last such t
//                         (len + 1: not settled)
//   pairs_out / viol_out / worst_out
//                         the certificate scan's pairs (t, k), k = 1..n, t + k <= len, restricted
//                         to starts outside the residual ball, q_t > ball_factor * tail_max: their
//                         count, those with V_{t+k} > s_{k-1} V_t, and the largest difference
//                         (-inf without a pair)
// Two passes over t, each bounded by len <= T; the inner loop by n.
MH_HD void robust_scan_env(const float* v, const float* q, int64_t E, int64_t e, int len, int T, int n,
                           const float* s, int W, float settle_frac, float ball_factor, RobustRow* out) {
  RobustRow o;
  len = len < 0 ? 0 : (len > T ? T : len);
  const float q0 = q[e];
  const float thr = settle_frac * q0;
  const int tail0 = len - W + 1 > 0 ? len - W + 1 : 0;
  o.q_peak = q0;
  o.t_peak = 0;
  o.settle = 0;
  o.tail_max = -INFINITY;
  o.tail_count = 0;
  double tail_sum = 0.0;
  for (int t = 0; t <= len; ++t) {
    const float qt = q[(int64_t)t * E + e];
    if (qt > o.q_peak) {
      o.q_peak = qt;
      o.t_peak = t;
    }
    if (qt > thr) o.settle = t + 1;
    if (t >= tail0) {
      o.tail_max = fmaxf(o.tail_max, qt);
      tail_sum += (double)qt;
      o.tail_count += 1;
    }
  }
  o.tail_mean = tail_sum / (double)o.tail_count;  // count >= 1: row len is always in the tail
  const float r2 = ball_factor * o.tail_max;
  o.pairs_out = o.viol_out = 0;
  o.worst_out = -INFINITY;
  for (int t = 0; t <= len; ++t) {
    const float qt = q[(int64_t)t * E + e];
    if (!(qt > r2)) continue;
    const float Vt = v[(int64_t)t * E + e];
    const int kmax = len - t < n ? len - t : n;
    for (int k = 0; k < kmax; ++k) {
      const float V2 = v[(int64_t)(t + k + 1) * E + e];
      const float d = V2 - Vt * s[k];
      o.pairs_out += 1;
      o.viol_out += d > 0.0f ? 1 : 0;
      o.worst_out = fmaxf(o.worst_out, d);
    }
  }
  *out = o;
}

// Row alignment the vector row accesses need (robust begin / step): 16 B for rows of a multiple of
// 4 floats, 8 B for even rows; a null pointer passes
inline bool robust_row_aligned(const void* p, int n) {
  const uintptr_t w = n % 4 == 0 ? 16 : (n % 2 == 0 ? 8 : 4);
  return p == nullptr || reinterpret_cast<uintptr_t>(p) % w == 0;
}

}  // namespace mh
