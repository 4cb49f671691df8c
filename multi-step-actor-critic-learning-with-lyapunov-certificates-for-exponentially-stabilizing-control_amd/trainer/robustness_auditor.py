"""Robustness sweep: the closed-loop audit (certificate_auditor.py) under sensor and actuator noise
(new: the reference's README shows QuadrotorTracking "with noises" but ships no code for it).

L noise levels x M paired trajectories are ONE lockstep batch of L * M envs (env l * M + m is
level l, trajectory m): the disturbance of mh_robust_step is per env. Every level starts from the
same M initial states and, with common_noise, sees the same noise realisations scaled by its own
sigmas (common random numbers), so the level curves are paired. The loop is the auditor's with the
policy fed the MEASURED observation and V evaluated on the TRUE one:
    policy(obs_meas) -> mh_robust_step -> lyapunov(obs)
then mh_certificate_scan (the nominal certificate) and mh_robust_scan (peak, tail, settling time
and the decay outside the residual ball). Disturbance model, Philox ticks / streams and metric
definitions: csrc/robustness.h, include/msacl_hip.h. With an explicit device="cpu" the same loop
runs on the engine's CPU build.
"""
import ctypes
import math

import numpy as np
import torch

from .. import _native as N
from ..env.host_vector_env import make_vector_env
from .certificate_auditor import CertificateAuditor

_CERT_I32 = ("lo_count", "hi_count", "pairs", "lya_viol", "esl_neg", "windows")
_CERT_F32 = ("lo_excess", "hi_excess", "lya_worst")
_ROBUST_DTYPES = dict(q_peak=torch.float32, t_peak=torch.int32, tail_max=torch.float32, tail_mean=torch.float64,
                      tail_count=torch.int32, settle=torch.int32, pairs_out=torch.int32, viol_out=torch.int32,
                      worst_out=torch.float32)


def _level(lv, A):
    """One level's settings as (obs_sigma, act_sigma, act_bias [A]), validated."""
    unknown = set(lv) - {"obs_sigma", "act_sigma", "act_bias"}
    if unknown:
        raise ValueError(f"sweep level has unknown keys {sorted(unknown)}")
    so, sa = float(lv.get("obs_sigma", 0.0)), float(lv.get("act_sigma", 0.0))
    bias = np.asarray(lv.get("act_bias", 0.0), np.float32)
    if bias.ndim == 0:
        bias = np.full(A, bias, np.float32)
    if bias.shape != (A,):
        raise ValueError(f"act_bias must be a scalar or [{A}]")
    if not (math.isfinite(so) and math.isfinite(sa) and so >= 0 and sa >= 0 and np.isfinite(bias).all()):
        raise ValueError("sweep levels need finite obs_sigma >= 0, act_sigma >= 0 and act_bias")
    return so, sa, bias


class RobustnessAuditor(CertificateAuditor):
    def __init__(self, index=0, networks=None, **kwargs):
        super().__init__(index=index, networks=networks, **kwargs)
        self.noise_seed = int(kwargs.get("robust_noise_seed", self.seed + 15485863)) & ((1 << 64) - 1)
        w = kwargs.get("robust_obs_weight")
        self.obs_weight = None if w is None else torch.as_tensor(np.asarray(w, np.float32), device=self.device).contiguous()

    def _draw_initial_states(self, M):
        """M reset states drawn once from the env's reset distribution and read back (every env's
        state right after a reset is its reset state)."""
        envs = make_vector_env(self.env_id, M, seed=self.seed, device=self.device)
        try:
            if envs.state_dim != envs.reset_dim:
                raise RuntimeError(f"{self.env_id}: the reset state cannot be read back from the env state")
            envs.reset()
            return envs.get_state()[0].cpu().numpy().astype(np.float32)
        finally:
            envs.close()

    @torch.no_grad()
    def sweep(self, levels, initial_states=None, trajectories=None, horizon=None, tail_window=100, settle_frac=0.01,
              ball_factor=1.0, common_noise=True, keep_trajectory=False):
        """Follow the closed loop under every disturbance level of `levels` (dicts with obs_sigma,
        act_sigma, act_bias: a scalar or [A]; missing keys are 0) from the same M initial states
        (given [M][reset_dim], or `trajectories` of them drawn once; default num_audit_states)
        over at most `horizon` steps; tail_window is capped at horizon + 1 rows. Returns audit()'s
        per-env tensors [L * M] (level-major) without its `summary`, the robust scan's
        (mh_robust_out_t), `level` / `trajectory` (each env's indices),
        `initial_states` [M][reset_dim] and `levels`: one summary dict per level. common_noise
        gives trajectory m the same noise realisation at every level. keep_trajectory adds q, v,
        resid, obs (true), act (applied) as in audit()."""
        levels = list(levels)
        if not levels:
            raise ValueError("sweep needs at least one level")
        if initial_states is None:
            M = int(self.num_envs if trajectories is None else trajectories)
            if M <= 0:
                raise ValueError("trajectories must be positive")
            init = self._draw_initial_states(M)
        else:
            init = np.ascontiguousarray(np.asarray(initial_states, np.float32))
            M = int(init.shape[0])
            if trajectories is not None and int(trajectories) != M:
                raise ValueError("trajectories differs from the number of initial_states")
        L = len(levels)
        E = L * M
        T = int(self.horizon if horizon is None else horizon)
        envs = self._envs_for(E)
        if not 0 < T <= envs.info.max_step:
            raise ValueError(f"sweep horizon must be in [1, {envs.info.max_step}]")
        W = min(int(tail_window), T + 1)
        if W < 1:
            raise ValueError("tail_window must be positive")
        for name, val in (("settle_frac", settle_frac), ("ball_factor", ball_factor)):
            if not (math.isfinite(val) and val >= 0):
                raise ValueError(f"{name} must be finite and >= 0")
        dev, D, A = self.device, envs.obs_dim, envs.act_dim
        if init.ndim != 2 or init.shape[1] != envs.reset_dim:
            raise ValueError(f"initial_states must be [M][{envs.reset_dim}]")
        if self.obs_weight is not None and self.obs_weight.numel() != D:
            raise ValueError(f"robust_obs_weight must be [{D}]")
        sets = [_level(lv, A) for lv in levels]
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        to_dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev).contiguous()  # noqa: E731
        obs_sigma = to_dev(np.repeat(np.array([s[0] for s in sets], np.float32), M))
        act_sigma = to_dev(np.repeat(np.array([s[1] for s in sets], np.float32), M))
        act_bias = to_dev(np.repeat(np.stack([s[2] for s in sets]), M, axis=0))
        tr_idx = np.tile(np.arange(M, dtype=np.int32), L)
        noise_id = to_dev(tr_idx if common_noise else np.arange(E, dtype=np.int32))
        rs = to_dev(np.tile(init, (L, 1)))
        p = self._ptr
        dist = N.Disturbance(p(obs_sigma), p(self.obs_weight), p(act_sigma), p(act_bias), p(noise_id), self.noise_seed)

        q, v = torch.empty(T + 1, E, **f32), torch.empty(T + 1, E, **f32)
        t_obs = torch.empty(T + 1, E, D, **f32) if keep_trajectory else None
        t_act = torch.empty(T, E, A, **f32) if keep_trajectory else None
        ln, status = torch.empty(E, **i32), torch.empty(E, **i32)
        ret = torch.empty(E, dtype=torch.float64, device=dev)
        cost = torch.empty(E, dtype=torch.float64, device=dev)
        traj = N.AuditTraj(p(q), p(v), p(t_obs), p(t_act), p(ln), p(status), p(ret), p(cost), E, T,
                           self.reward_scale, self.cost_scale)
        h = envs.handle()
        obs, meas = torch.empty(E, D, **f32), torch.empty(E, D, **f32)
        nets = self.networks
        self._call("robust_begin", h, p(rs), p(obs), p(meas), ctypes.byref(traj), ctypes.byref(dist))
        v[0].copy_(nets.lyapunov(obs))
        for t in range(T):
            logits = nets.policy(meas).float().contiguous()
            self._call("robust_step", h, p(logits), None, p(obs), p(meas), ctypes.byref(traj), ctypes.byref(dist), t)
            v[t + 1].copy_(nets.lyapunov(obs))  # the TRUE observation; a frozen env's row is never read
            if t % 32 == 31 and bool((status != 0).all()):  # one host sync per 32 lockstep steps
                break
        out = {k: torch.empty(E, **i32) for k in _CERT_I32}
        out.update({k: torch.empty(E, **f32) for k in _CERT_F32})
        out["resid_sum"] = torch.empty(E, dtype=torch.float64, device=dev)
        co = N.CertificateOut(*(p(out[k]) for k, _ in N.CertificateOut._fields_))
        resid = torch.empty(T, E, **f32) if keep_trajectory else None
        c, w, s = self.coefs
        self._call("certificate_scan", ctypes.byref(traj), self.n_step, p(c), p(w), p(s), self.alpha1, self.alpha2,
                   ctypes.byref(co), p(resid))
        rob = {k: torch.empty(E, dtype=dt, device=dev) for k, dt in _ROBUST_DTYPES.items()}
        ro = N.RobustOut(*(p(rob[k]) for k, _ in N.RobustOut._fields_))
        self._call("robust_scan", ctypes.byref(traj), self.n_step, p(s), W, float(settle_frac), float(ball_factor),
                   ctypes.byref(ro))
        out.update(rob)
        out.update(len=ln, status=status, ret=ret, cost=cost, q0=q[0].clone(),
                   q_end=q.gather(0, ln.long().unsqueeze(0)).squeeze(0),
                   level=to_dev(np.repeat(np.arange(L, dtype=np.int32), M)), trajectory=to_dev(tr_idx))
        if keep_trajectory:
            out.update(q=q, v=v, resid=resid, obs=t_obs, act=t_act)
        out["initial_states"] = init
        out["levels"] = self._level_summaries(out, sets, L, M)
        return out

    @staticmethod
    def _level_summaries(o, sets, L, M):
        """One dict per level, reduced with torch over the [L][M] view of the per-env tensors."""
        view = lambda k: o[k].view(L, M)  # noqa: E731
        steps = view("len").double()
        frac = lambda mask: mask.double().mean(1)  # noqa: E731
        cols = dict(
            terminated=frac(view("status") == 1),
            cost_per_step=view("cost").sum(1) / steps.sum(1).clamp_min(1),
            tail_rms=view("tail_mean").mean(1).sqrt(),
            tail_max=view("tail_max").double().max(1).values,
            settled=frac(view("settle") <= view("len")),
            settle_mean=view("settle").double().mean(1),
            decay_ok=frac(view("lya_viol") == 0),
            decay_ok_outside=frac(view("viol_out") == 0),
        )
        cols = {k: t.cpu().tolist() for k, t in cols.items()}
        res = []
        for li, (so, sa, bias) in enumerate(sets):
            d = dict(level=li, obs_sigma=so, act_sigma=sa, act_bias=[float(b) for b in bias], trajectories=M)
            d.update({k: float(vals[li]) for k, vals in cols.items()})
            res.append(d)
        return res
