"""Closed-loop audit of the learned Lyapunov certificate (new: the reference only ever evaluates
the Lyapunov network inside the training loss, RL/algorithm/msacl.py:279-332).

From a batch of initial states the deterministic closed loop (the policy distribution's mode()
action) is followed in lockstep WITHOUT autoreset (mh_audit_step: an env that terminates or
truncates is frozen), V is evaluated on every observation, and one scan (mh_certificate_scan)
checks along every trajectory what MSACL trains:
  * the bounds alpha1 |x|^2 <= V(x) <= alpha2 |x|^2 (msacl.py:288-301);
  * the multi-step decay V(x_{t+k}) <= (1 - eta)^k V(x_t), k = 1..n, and the training-consistent
    residual (lya_diff of msacl.py:307-328 with is_clip_ratio = 1).
The policy and V run through the networks' own modules (their fused dispatch, any hidden size);
the host looks at the envs' status at most every 32 steps. With an explicit device="cpu" the same
loop runs on the engine's CPU build.
"""
import ctypes

import numpy as np
import torch

from .. import _native as N
from ..algorithm.msacl import certificate_coefs
from ..create_pkg.create_alg import create_approx_contrainer
from ..env.host_vector_env import make_vector_env

# envs whose reset state is the observation (state_grid)
_GRID_ENVS = ("VanderPol", "Pendulum", "DuctedFan", "TwoLink", "SingleTrackCar")


def state_grid(env_name, dims=(0, 1), points=33, span=None):
    """Phase-plane initial states [points * points][reset_dim]: a regular grid over state
    components dims = (i, j), every other component 0. span: half-width of the grid (a scalar or
    one per dim); default 0.9 of the observation box."""
    if env_name not in _GRID_ENVS:
        raise ValueError(f"state_grid: the reset state of {env_name} is not its observation")
    info = N.host_env_info(env_name)
    i, j = (int(d) for d in dims)
    if i == j or not (0 <= i < info.reset_dim and 0 <= j < info.reset_dim):
        raise ValueError(f"state_grid: dims {dims} outside the {info.reset_dim} state components")
    if span is None:
        span = (0.9 * info.obs_high[i], 0.9 * info.obs_high[j])
    si, sj = (float(span), float(span)) if np.isscalar(span) else (float(span[0]), float(span[1]))
    gi, gj = np.meshgrid(np.linspace(-si, si, int(points)), np.linspace(-sj, sj, int(points)), indexing="ij")
    out = np.zeros((gi.size, info.reset_dim), np.float32)
    out[:, i], out[:, j] = gi.ravel(), gj.ravel()
    return out


class CertificateAuditor:
    def __init__(self, index=0, networks=None, **kwargs):
        self.env_id = kwargs["env_name"]
        self.reward_scale = float(kwargs["reward_scale"])
        self.cost_scale = float(kwargs["cost_scale"])
        self.num_envs = int(kwargs.get("num_audit_states", 1024))
        self.horizon = int(kwargs.get("audit_horizon", 1000))
        dev = kwargs.get("device")
        self.device = torch.device(dev) if dev is not None else torch.device("cuda")
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.seed = int(kwargs.get("eval_env_seed", 2)) + 104729 * (index + 1)
        self.envs = None
        # a caller that owns networks (the trainer's hook) shares them; otherwise the auditor's own
        self.networks = networks if networks is not None else create_approx_contrainer(**kwargs)
        self.n_step = int(kwargs["n_step"])
        self.alpha1, self.alpha2 = float(kwargs.get("alpha1", 1.0)), float(kwargs.get("alpha2", 2.0))
        self.coefs = tuple(t.to(self.device).contiguous() for t in certificate_coefs(
            self.n_step, kwargs.get("lya_eta", 0.15), kwargs.get("retrace_lambda", 0.95), self.alpha1, self.alpha2))

    def close(self):
        """Release the audit envs' handle (idempotent)."""
        if self.envs is not None:
            self.envs.close()
            self.envs = None

    def load_state_dict(self, state_dict):
        self.networks.load_state_dict(state_dict)

    # ------------------------------------------------------------------ engine calls
    def _call(self, name, *args):
        if self.device.type == "cpu":
            N.host_check(getattr(N.host_lib(), "mhh_" + name)(*args), "mhh_" + name)
        else:
            N.check(getattr(N.lib(), "mh_" + name)(*args, N.stream_of(self.device)), "mh_" + name)

    def _ptr(self, t):
        return N.hptr(t) if self.device.type == "cpu" else N.ptr(t)

    def _envs_for(self, E):
        if self.envs is None or self.envs.num_envs != E:
            self.close()
            self.envs = make_vector_env(self.env_id, E, seed=self.seed, device=self.device)
        return self.envs

    @torch.no_grad()
    def audit(self, initial_states=None, horizon=None, keep_trajectory=False):
        """Audit the certificate from `initial_states` [E][reset_dim] (None: num_audit_states drawn
        from the env's reset distribution) over at most `horizon` steps. Returns a dict of
        per-env tensors — len, status (0 running, 1 terminated, 2 truncated), ret, cost (float64
        sums of the scaled reward / cost), q0, q_end, the scan's counts and excesses (see
        mh_certificate_out_t) — plus `summary` (floats). keep_trajectory adds the time-major
        columns q, v [T + 1][E], resid [T][E], obs [T + 1][E][D] and act [T][E][A]; of an env's
        column only rows t <= len (act, resid: t < len) are meaningful."""
        E = self.num_envs if initial_states is None else int(np.shape(initial_states)[0])
        T = int(self.horizon if horizon is None else horizon)
        envs = self._envs_for(E)
        if not 0 < T <= envs.info.max_step:
            raise ValueError(f"audit horizon must be in [1, {envs.info.max_step}]")
        dev, D, A = self.device, envs.obs_dim, envs.act_dim
        f32 = dict(dtype=torch.float32, device=dev)
        q, v = torch.empty(T + 1, E, **f32), torch.empty(T + 1, E, **f32)
        t_obs = torch.empty(T + 1, E, D, **f32) if keep_trajectory else None
        t_act = torch.empty(T, E, A, **f32) if keep_trajectory else None
        ln = torch.empty(E, dtype=torch.int32, device=dev)
        status = torch.empty(E, dtype=torch.int32, device=dev)
        ret = torch.empty(E, dtype=torch.float64, device=dev)
        cost = torch.empty(E, dtype=torch.float64, device=dev)
        p = self._ptr
        traj = N.AuditTraj(p(q), p(v), p(t_obs), p(t_act), p(ln), p(status), p(ret), p(cost), E, T,
                           self.reward_scale, self.cost_scale)
        h = envs.handle()
        obs = torch.empty(E, D, **f32)
        rs = None
        if initial_states is not None:
            rs = torch.as_tensor(np.asarray(initial_states, np.float32), device=dev).contiguous()
            if rs.numel() != E * envs.reset_dim:
                raise ValueError(f"initial_states must be [E][{envs.reset_dim}]")
        nets = self.networks
        self._call("audit_begin", h, p(rs), p(obs), ctypes.byref(traj))
        v[0].copy_(nets.lyapunov(obs))
        for t in range(T):
            logits = nets.policy(obs).float().contiguous()
            self._call("audit_step", h, p(logits), None, p(obs), ctypes.byref(traj), t)
            v[t + 1].copy_(nets.lyapunov(obs))  # a frozen env's row is never read (t + 1 > len)
            if t % 32 == 31 and bool((status != 0).all()):  # one host sync per 32 lockstep steps
                break
        i32 = dict(dtype=torch.int32, device=dev)
        out = {k: torch.empty(E, **i32) for k in ("lo_count", "hi_count", "pairs", "lya_viol", "esl_neg", "windows")}
        out.update({k: torch.empty(E, **f32) for k in ("lo_excess", "hi_excess", "lya_worst")})
        out["resid_sum"] = torch.empty(E, dtype=torch.float64, device=dev)
        co = N.CertificateOut(*(p(out[k]) for k, _ in N.CertificateOut._fields_))
        resid = torch.empty(T, E, **f32) if keep_trajectory else None
        c, w, s = self.coefs
        self._call("certificate_scan", ctypes.byref(traj), self.n_step, p(c), p(w), p(s), self.alpha1, self.alpha2,
                   ctypes.byref(co), p(resid))
        out.update(len=ln, status=status, ret=ret, cost=cost, q0=q[0].clone(),
                   q_end=q.gather(0, ln.long().unsqueeze(0)).squeeze(0))
        if keep_trajectory:
            out.update(q=q, v=v, resid=resid, obs=t_obs, act=t_act)
        out["summary"] = self._summary(out)
        return out

    @staticmethod
    def _summary(o):
        steps = o["len"].double()
        windows = float(o["windows"].sum())
        # |x_len|^2 = rate^len |x_0|^2: the per-step contraction of the squared norm actually seen
        ok = (o["len"] > 0) & (o["q0"] > 0) & (o["q_end"] > 0)
        rate = torch.exp((torch.log(o["q_end"][ok].double()) - torch.log(o["q0"][ok].double())) / steps[ok])
        return {
            "bounds_ok": float(((o["lo_count"] == 0) & (o["hi_count"] == 0)).double().mean()),
            "decay_ok": float((o["lya_viol"] == 0).double().mean()),
            "terminated": float((o["status"] == 1).double().mean()),
            "residual": float(o["resid_sum"].sum()) / windows if windows > 0 else 0.0,
            "cost_per_step": float(o["cost"].sum() / steps.sum().clamp_min(1)),
            "contraction_rate": float(rate.mean()) if rate.numel() else float("nan"),
        }
