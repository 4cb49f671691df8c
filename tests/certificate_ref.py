"""Shared by test_certificate_host.py and test_gpu_certificate.py: the certificate scan restated in
numpy, the scan / audit entry points behind one call for either library, and the test cases."""
import ctypes
import os

import numpy as np
import torch

import msacl_amd  # noqa: F401
import msacl_amd._native as N
from msacl_amd.algorithm.msacl import certificate_coefs
from oracle import envs as OE

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COUNTS = ("lo_count", "hi_count", "pairs", "lya_viol", "esl_neg", "windows")
FLOATS = ("lo_excess", "hi_excess", "lya_worst", "resid_sum")
f32 = np.float32


def coefs(n, eta=0.15, lam=0.95, alpha1=1.0, alpha2=2.0):
    return tuple(t.numpy().astype(f32) for t in certificate_coefs(n, eta, lam, alpha1, alpha2))


def scan_numpy(v, q, ln, n, c, w, s, alpha1, alpha2):
    """The scan in float32 numpy, vectorised over envs: same expressions, same order."""
    T, E = v.shape[0] - 1, v.shape[1]
    o = {k: np.zeros(E, np.int32) for k in COUNTS}
    o.update(lo_excess=np.zeros(E, f32), hi_excess=np.zeros(E, f32), lya_worst=np.full(E, -np.inf, f32),
             resid_sum=np.zeros(E, np.float64), resid=np.zeros((T, E), f32))
    a1, a2 = f32(alpha1), f32(alpha2)
    for t in range(T + 1):
        act = ln >= t
        Vt, qt = np.where(act, v[t], f32(0)), np.where(act, q[t], f32(0))
        l1, l2 = a1 * qt - Vt, Vt - a2 * qt
        o["lo_count"] += act & (l1 > 0)
        o["hi_count"] += act & (l2 > 0)
        o["lo_excess"] = np.where(act, np.maximum(o["lo_excess"], l1), o["lo_excess"])
        o["hi_excess"] = np.where(act, np.maximum(o["hi_excess"], l2), o["hi_excess"])
        sn = np.sqrt(qt)
        r = np.zeros(E, f32)
        for k in range(min(n, T - t)):
            ok = ln >= t + k + 1
            V2, q2 = np.where(ok, v[t + k + 1], f32(0)), np.where(ok, q[t + k + 1], f32(0))
            esl = np.where(sn * c[k] - np.sqrt(q2) >= 0, f32(1), f32(-1))
            d = V2 - Vt * s[k]
            o["pairs"] += ok
            o["lya_viol"] += ok & (d > 0)
            o["esl_neg"] += ok & (esl < 0)
            o["lya_worst"] = np.where(ok, np.maximum(o["lya_worst"], d), o["lya_worst"])
            r = np.where(ok, r + w[k] * np.maximum(esl * d, f32(0)), r)
        full = ln >= t + n
        o["windows"] += full
        o["resid_sum"] += np.where(full, r.astype(np.float64), 0.0)
        if t < T:
            o["resid"][t] = np.where(full, r, f32(0))
    return o


def _dev(device):
    return torch.device(device)


def _p(device, t):
    return N.hptr(t) if _dev(device).type == "cpu" else N.ptr(t)


def _call(device, name, *args):
    if _dev(device).type == "cpu":
        N.host_check(getattr(N.host_lib(), "mhh_" + name)(*args), "mhh_" + name)
    else:
        N.check(getattr(N.lib(), "mh_" + name)(*args, N.stream_of(_dev(device))), "mh_" + name)


def run_scan(device, v, q, ln, n, c, w, s, alpha1, alpha2):
    """mh(h)_certificate_scan on numpy inputs -> dict of numpy outputs (with the dense resid)."""
    T, E = v.shape[0] - 1, v.shape[1]
    to = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dt)).to(device)  # noqa: E731
    tv, tq, tl = to(v, f32), to(q, f32), to(ln, np.int32)
    tc, tw, ts = to(c, f32), to(w, f32), to(s, f32)
    out = {k: torch.full((E,), -7, dtype=torch.int32, device=device) for k in COUNTS}
    out.update({k: torch.full((E,), np.nan, dtype=torch.float32, device=device) for k in FLOATS[:3]})
    out["resid_sum"] = torch.full((E,), np.nan, dtype=torch.float64, device=device)
    resid = torch.full((max(T, 1), E), np.nan, dtype=torch.float32, device=device)
    p = lambda t: _p(device, t)  # noqa: E731
    traj = N.AuditTraj(p(tq), p(tv), None, None, p(tl), None, None, None, E, T, 1.0, 1.0)
    co = N.CertificateOut(*(p(out[k]) for k, _ in N.CertificateOut._fields_))
    _call(device, "certificate_scan", ctypes.byref(traj), n, p(tc), p(tw), p(ts), alpha1, alpha2, ctypes.byref(co),
          p(resid))
    res = {k: t.cpu().numpy() for k, t in out.items()}
    res["resid"] = resid.cpu().numpy()[:T]
    return res


def assert_scan_equal(got, want, tol=1e-5):
    for k in COUNTS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    for k in FLOATS + ("resid",):
        np.testing.assert_allclose(got[k], want[k], rtol=tol, atol=tol, err_msg=k)


# ------------------------------------------------------------------ scan cases
def golden_case():
    """tests/golden/msacl_update_bench.npz as 256 trajectories of T = 20 (its windows are
    contiguous): v / q [21][256], and the fixture's own arrays for the expectations."""
    g = np.load(os.path.join(G, "msacl_update_bench.npz"))
    V0, V2 = g["it0/lyapunov_update0/lya_obs"], g["it0/lyapunov_update0/lya_obs2"]
    v = np.concatenate([V0[:, :1], V2], axis=1).T.astype(f32)
    q0 = (g["in_obs"][:, 0] * g["in_obs"][:, 0]).sum(-1, dtype=f32)
    q2 = (g["in_obs2"] * g["in_obs2"]).sum(-1, dtype=f32)
    q = np.concatenate([q0[:, None], q2], axis=1).T.astype(f32)
    return g, np.ascontiguousarray(v), np.ascontiguousarray(q)


EDGE_CASES = [(E, n, T) for E in (1, 63, 64, 65, 257) for n in (1, 20, 64) for T in sorted({1, n - 1, n, n + 1})]


def edge_case(E, n, T, seed=0):
    """Random positive V / q with ragged len (0, 1 and T included) and NaN beyond len."""
    rng = np.random.default_rng(seed + 1000 * E + 10 * n + T)
    q = rng.uniform(0.05, 4.0, (T + 1, E)).astype(f32)
    v = (q * rng.uniform(0.6, 2.4, (T + 1, E))).astype(f32)  # both bounds violated somewhere
    ln = rng.integers(0, T + 1, E).astype(np.int32)
    ln[:3] = np.array([0, min(1, T), T], np.int32)[:min(3, E)]
    beyond = np.arange(T + 1)[:, None] > ln[None, :]
    v[beyond], q[beyond] = np.nan, np.nan
    return v, q, ln


# ------------------------------------------------------------------ audit trajectories
NAMES = list(OE.ENVS)


def audit_initial_states(name, E, seed=0):
    """E reset states from the oracle's reset distribution (QuadTracking: the reference's
    evaluation states, tiled); the first 8 start just inside a corner of the observation box with
    outward velocities, so they leave it within a step or two."""
    if name == "QuadTracking":
        init = np.load(os.path.join(G, "eval_QuadTracking.npz"))["init"].astype(f32)
        rs = np.ascontiguousarray(np.tile(init, ((E + len(init) - 1) // len(init), 1))[:E])
        rs[:8, 0] += f32(9.9)   # position error near the box (10), moving outward
        rs[:8, 3] = f32(9.0)
        return rs
    rng = np.random.default_rng(seed)
    rs = OE.ENVS[name].reset_draw(rng, E).astype(f32)
    hi = OE.ENVS[name].obs_high.astype(f32)
    sign = np.where(np.arange(8)[:, None] % 2 == 0, f32(1), f32(-1))
    rs[:8] = sign * f32(0.9995) * hi[None, :]
    return np.ascontiguousarray(rs)


class AuditRun:
    """One audit trajectory store on `device` around a vector env's handle."""

    def __init__(self, env, T, keep=True):
        self.env, self.T = env, T
        E, D, A, dev = env.num_envs, env.obs_dim, env.act_dim, env.device
        self.dev = dev
        z = lambda *s, dt=torch.float32: torch.full(s, -5, dtype=dt, device=dev)  # noqa: E731
        self.q, self.obs = z(T + 1, E), z(E, D)
        self.traj_obs = z(T + 1, E, D) if keep else None
        self.traj_act = z(T, E, A) if keep else None
        self.len, self.status = z(E, dt=torch.int32), z(E, dt=torch.int32)
        self.ret, self.cost = z(E, dt=torch.float64), z(E, dt=torch.float64)
        p = lambda t: _p(dev, t)  # noqa: E731
        self.traj = N.AuditTraj(p(self.q), None, p(self.traj_obs), p(self.traj_act), p(self.len), p(self.status),
                                p(self.ret), p(self.cost), E, T, 100.0, 100.0)

    def begin(self, reset_states):
        rs = None if reset_states is None else torch.as_tensor(reset_states, dtype=torch.float32).to(self.dev).contiguous()
        _call(self.dev, "audit_begin", self.env.handle(), _p(self.dev, rs), _p(self.dev, self.obs), ctypes.byref(self.traj))

    def step(self, t, logits=None, act=None):
        _call(self.dev, "audit_step", self.env.handle(), _p(self.dev, logits), _p(self.dev, act), _p(self.dev, self.obs),
              ctypes.byref(self.traj), t)


def check_injected_parity(device, name, E, T=8):
    """audit_step with injected actions against the vector env's own step (SyncVectorEnv contract),
    bit for bit while an env lives; after it terminates or truncates the audit holds everything of
    it unchanged and writes nothing for it."""
    from msacl_amd.env.host_vector_env import make_vector_env
    on = "cpu" if _dev(device).type == "cpu" else None  # None: the current HIP device
    A_env, B_env = (make_vector_env(name, E, seed=5, device=on) for _ in range(2))
    dev = A_env.device
    rs = audit_initial_states(name, E)
    run = AuditRun(A_env, T)
    run.begin(rs)
    obs_b, _ = B_env.reset(reset_states=rs)
    assert torch.equal(run.obs, obs_b) and torch.equal(run.traj_obs[0], obs_b)
    np.testing.assert_allclose(run.q[0].cpu().numpy(), (obs_b.cpu().numpy() ** 2).sum(-1), rtol=1e-6)
    assert not run.q[1:].any() and not run.len.any() and not run.status.any() and not run.ret.any()
    lo = torch.as_tensor(A_env.single_action_space.low, device=dev)
    hi = torch.as_tensor(A_env.single_action_space.high, device=dev)
    gen = torch.Generator().manual_seed(E)
    alive = torch.ones(E, dtype=torch.bool, device=dev)
    ret = torch.zeros(E, dtype=torch.float64, device=dev)
    cost = torch.zeros(E, dtype=torch.float64, device=dev)

    def snapshot():
        st, xs, sp = A_env.get_state()
        return [t.clone() for t in (run.obs, st, sp, run.len, run.status, run.ret, run.cost) + ((xs,) if xs is not None else ())]

    for t in range(T):
        act = (lo + (hi - lo) * torch.rand(E, A_env.act_dim, generator=gen).to(dev)).contiguous()
        before = snapshot()
        run.step(t, act=act)
        _, rew, term, trunc, info = B_env.step(act, reset_states=rs)
        real = info["final_observation"]
        after = snapshot()
        frozen = ~alive
        for a, b in zip(before, after):  # a frozen env: state, steps, observation, accumulators untouched
            assert torch.equal(a[frozen], b[frozen])
        assert not run.q[t + 1][frozen].any()                       # ... and nothing written for it
        assert (run.traj_obs[t + 1][frozen] == -5).all() and (run.traj_act[t][frozen] == -5).all()
        assert torch.equal(run.obs[alive], real[alive])
        assert torch.equal(run.traj_obs[t + 1][alive], real[alive])
        assert torch.equal(run.traj_act[t][alive], act[alive])
        np.testing.assert_allclose(run.q[t + 1][alive].cpu().numpy(), (real[alive].cpu().numpy() ** 2).sum(-1), rtol=1e-6)
        ret += torch.where(alive, (rew * 100.0).double(), 0.0)
        cost += torch.where(alive, (run.q[t + 1] * 100.0).double(), 0.0)
        assert torch.equal(run.ret, ret) and torch.equal(run.cost, cost)
        want = torch.where(term, 1, torch.where(trunc, 2, 0)).to(torch.int32)
        assert torch.equal(run.status[alive], want[alive])
        assert (run.len[alive] == t + 1).all()
        going = alive & ~(term | trunc)  # B autoresets the others: compare states only where both go on
        sa, sb = A_env.get_state(), B_env.get_state()
        for a, b in zip(sa, sb):
            if a is not None:
                assert torch.equal(a[going], b[going])
        alive = going
    ended = (~alive).cpu().numpy()
    assert ended[:8].any() and not ended.all(), "the case must hold early exits and survivors"
    assert (run.len[~alive] < T).any()
    A_env.close()
    B_env.close()
    return run
