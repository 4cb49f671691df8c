// certificate.h — per-env expressions of the closed-loop Lyapunov certificate audit, shared by the
// gfx950 kernels (certificate.hip) and the engine's CPU build (host_engine.hip), as env_math.h is.
//
// The audit follows the deterministic closed loop (TanhGaussDistribution.mode() actions) from a
// batch of initial states WITHOUT autoreset, then checks the certificate MSACL trains along every
// trajectory: the bounds alpha1 |x|^2 <= V(x) <= alpha2 |x|^2 (RL/algorithm/msacl.py:288-301) and
// the multi-step decay V(x_{t+k}) <= (1 - eta)^k V(x_t), k = 1..n (msacl.py:307-328).
#pragma once

#include "env_math.h"

namespace mh {

constexpr int CERT_MAX_N = 64;  // largest n-step window of the scan

enum AuditStatus : int { AUDIT_RUNNING = 0, AUDIT_TERMINATED = 1, AUDIT_TRUNCATED = 2 };

// tanh(z) = sign(z) (1 - t) / (1 + t), t = exp(-2|z|): the sampling branch's form (rollout.hip),
// on the device through the same hardware transcendentals (v_exp_f32 / v_rcp_f32, ~1 ulp)
MH_HD float mode_tanh(float z) {
#if defined(__HIP_DEVICE_COMPILE__)
  const float t = __builtin_amdgcn_exp2f(-2.88539008177792682f * fabsf(z));
  const float rt = __builtin_amdgcn_rcpf(1.0f + t);
#else
  const float t = exp2f(-2.88539008177792682f * fabsf(z));
  const float rt = 1.0f / (1.0f + t);
#endif
  return copysignf((1.0f - t) * rt, z);
}

// TanhGaussDistribution.mode() (act_distribution_cls.py:90-95) of the logits' mean half, then the
// sampler's clip to the action box (base.py:140-143)
template <class Env>
MH_HD void audit_mode_action(const float* mean, float* u) {
#pragma unroll
  for (int i = 0; i < Env::A; ++i) {
    const float lo = Env::act_lo(i), hi = Env::act_hi(i);
    const float half = (hi - lo) / 2.0f, mid = (hi + lo) / 2.0f;
    const float act = half * mode_tanh(mean[i]) + mid;
    u[i] = fminf(fmaxf(act, lo), hi);
  }
}

// |obs|^2 in the cost's summation order (rew_plus_cost.py:18-21 without the scale), so that
// q * cost_scale is the step's cost bit for bit
template <int D>
MH_HD float audit_q(const float* obs) {
  float sq[D];
#pragma unroll
  for (int i = 0; i < D; ++i) sq[i] = obs[i] * obs[i];
  return np_sum<D>(sq);
}

// One env.step of the audited closed loop: k = steps since reset before the step. Returns the
// env's status after it (the rollout kernel's termination / truncation test; terminated wins when
// both hold), the post-step observation, its q and the env's reward.
template <class Env>
MH_HD int audit_env_step(float* s, double* xs, int k, const float* u, const double* tab, float* obs2, float* q,
                         float* r) {
  if constexpr (Env::ROWN > 0) {
    double rowv[Env::ROWN];
    Env::load_row(tab, k, rowv);
    Env::step_row(s, xs, rowv, u, obs2, r);
  } else {
    Env::step(s, xs, k, u, tab, obs2, r);
  }
  bool term = false;
#pragma unroll
  for (int i = 0; i < Env::D; ++i) term = term || (obs2[i] < Env::obs_lo(i)) || (obs2[i] > Env::obs_hi(i));
  const bool trunc = k + 1 >= MAX_STEP;
  *q = audit_q<Env::D>(obs2);
  return term ? AUDIT_TERMINATED : (trunc ? AUDIT_TRUNCATED : AUDIT_RUNNING);
}

// One env's row of a row-major [E][N] float tensor as the widest aligned vector accesses (row
// offsets are multiples of N floats; the launchers check the base alignment). Device only: the
// audit's kernels (certificate.hip) and the robustness sweep's (robustness.hip) use them.
template <int N>
__device__ __forceinline__ void load_row(const float* p, float* out) {
  if constexpr (N % 4 == 0) {
#pragma unroll
    for (int i = 0; i < N; i += 4) {
      const float4 v = *reinterpret_cast<const float4*>(p + i);
      out[i] = v.x, out[i + 1] = v.y, out[i + 2] = v.z, out[i + 3] = v.w;
    }
  } else if constexpr (N % 2 == 0) {
#pragma unroll
    for (int i = 0; i < N; i += 2) {
      const float2 v = *reinterpret_cast<const float2*>(p + i);
      out[i] = v.x, out[i + 1] = v.y;
    }
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) out[i] = p[i];
  }
}
template <int N>
__device__ __forceinline__ void store_row(float* p, const float* v) {
  if constexpr (N % 4 == 0) {
#pragma unroll
    for (int i = 0; i < N; i += 4) *reinterpret_cast<float4*>(p + i) = make_float4(v[i], v[i + 1], v[i + 2], v[i + 3]);
  } else if constexpr (N % 2 == 0) {
#pragma unroll
    for (int i = 0; i < N; i += 2) *reinterpret_cast<float2*>(p + i) = make_float2(v[i], v[i + 1]);
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) p[i] = v[i];
  }
}

// One env's row of mh_certificate_out_t
struct CertRow {
  int32_t lo_count, hi_count, pairs, lya_viol, esl_neg, windows;
  float lo_excess, hi_excess, lya_worst;
  double resid_sum;
};

// The certificate along env e's trajectory: v / q are time-major [T + 1][E] columns of V(obs_t) and
// |obs_t|^2, valid for t = 0..len (rows beyond len are never read). c / w / s are the algorithm's
// start_obs_norm_coef / lya_diff_coef / start_lya_coef [n]. resid (nullable) is the dense
// [T][E] map of the training-consistent residual, 0 where start t has no full window.
// Element formulas and operation order are those of the Lyapunov loss (msacl_kernels.hip /
// mhh_msacl_lyapunov) with is_clip_ratio = 1: float32, the residual summed in k order.
MH_HD void certificate_scan_env(const float* v, const float* q, int64_t E, int64_t e, int len, int T, int n,
                                const float* c, const float* w, const float* s, float alpha1, float alpha2,
                                float* resid, CertRow* out) {
  CertRow o;
  o.lo_count = o.hi_count = o.pairs = o.lya_viol = o.esl_neg = o.windows = 0;
  o.lo_excess = o.hi_excess = 0.0f;
  o.lya_worst = -INFINITY;
  o.resid_sum = 0.0;
  len = len < 0 ? 0 : (len > T ? T : len);
  for (int t = 0; t <= len; ++t) {
    const float Vt = v[(int64_t)t * E + e], qt = q[(int64_t)t * E + e];
    const float l1 = alpha1 * qt - Vt, l2 = Vt - alpha2 * qt;
    o.lo_count += l1 > 0.0f ? 1 : 0;
    o.hi_count += l2 > 0.0f ? 1 : 0;
    o.lo_excess = fmaxf(o.lo_excess, l1);
    o.hi_excess = fmaxf(o.hi_excess, l2);
    const float start_norm = sqrtf(qt);
    const int kmax = len - t < n ? len - t : n;
    float r = 0.0f;
    for (int k = 0; k < kmax; ++k) {
      const float V2 = v[(int64_t)(t + k + 1) * E + e], q2 = q[(int64_t)(t + k + 1) * E + e];
      const float diff = start_norm * c[k] - sqrtf(q2);
      const float esl = diff >= 0.0f ? 1.0f : -1.0f;
      const float d = V2 - Vt * s[k];
      o.pairs += 1;
      o.lya_viol += d > 0.0f ? 1 : 0;
      o.lya_worst = fmaxf(o.lya_worst, d);
      o.esl_neg += esl < 0.0f ? 1 : 0;
      r = r + w[k] * fmaxf(esl * d, 0.0f);
    }
    const bool full = kmax == n;
    if (full) {
      o.windows += 1;
      o.resid_sum += (double)r;
    }
    if (resid && t < T) resid[(int64_t)t * E + e] = full ? r : 0.0f;
  }
  if (resid)
    for (int t = len + 1; t < T; ++t) resid[(int64_t)t * E + e] = 0.0f;
  *out = o;
}

}  // namespace mh
