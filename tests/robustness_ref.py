"""Shared by test_robustness_host.py and test_gpu_robustness.py: the sweep's noise (Philox4x32-10 +
float32 Box-Muller as csrc/philox.h writes it) and scan metrics restated in numpy, the robust entry
points behind one call for either library, and the test bodies both files run."""
import ctypes

import numpy as np
import pytest
import torch

import certificate_ref as R
import msacl_amd  # noqa: F401
import msacl_amd._native as N
from oracle import rng as ORNG

f32 = np.float32
TOL = 1e-5  # the project's parity tolerance (rtol = atol)
STREAM_OBS, STREAM_ACT = 16, 24
R_COUNTS = ("t_peak", "tail_count", "settle", "pairs_out", "viol_out")
R_FLOATS = ("q_peak", "tail_max", "tail_mean", "worst_out")
R_DTYPES = dict(q_peak=torch.float32, t_peak=torch.int32, tail_max=torch.float32, tail_mean=torch.float64,
                tail_count=torch.int32, settle=torch.int32, pairs_out=torch.int32, viol_out=torch.int32,
                worst_out=torch.float32)


# ------------------------------------------------------------------ noise
def normal4f(seed, ids, tick, stream):
    """Rng::normal4f(stream) of make_rng(seed, ids[e], tick) -> [n, 4] float32, every operation in
    float32 as philox.h writes it (numpy's float32 log / sin / cos stand for the C library's)."""
    w = ORNG.draw_words(seed, np.asarray(ids, np.int64).astype(np.uint64), np.full(len(ids), tick, np.uint64), stream)
    u = (w >> np.uint32(8)).astype(f32) * f32(5.9604644775390625e-08)
    u1, u2, u3, u4 = f32(1) - u[:, 0], u[:, 1], f32(1) - u[:, 2], u[:, 3]
    a, b = np.sqrt(f32(-2) * np.log(u1)), np.sqrt(f32(-2) * np.log(u3))
    tp = f32(6.28318530717958648)
    out = np.stack([a * np.cos(tp * u2), a * np.sin(tp * u2), b * np.cos(tp * u4), b * np.sin(tp * u4)], -1)
    assert out.dtype == f32
    return out


def normals(seed, ids, tick, base, n):
    """xi (base 16) or zeta (base 24) [len(ids), n]: component i from stream base + i // 4."""
    return np.concatenate([normal4f(seed, ids, tick, base + j) for j in range((n + 3) // 4)], 1)[:, :n]


def measure_numpy(obs, sigma, weight, seed, ids, tick):
    """obs + (sigma * w) * xi in float32; rows with sigma == 0 are the true rows."""
    D = obs.shape[1]
    w = np.ones(D, f32) if weight is None else weight.astype(f32)
    amp = sigma.astype(f32)[:, None] * w[None, :]
    return np.where(sigma[:, None] == 0, obs, obs + amp * normals(seed, ids, tick, STREAM_OBS, D))


def actuate_numpy(u_nom, lo, hi, bias, sigma, seed, ids, tick):
    """clip(u_nom + half * (bias + sigma * zeta), lo, hi) in float32 (zeta skipped where sigma == 0)."""
    A = u_nom.shape[1]
    half = (hi - lo) / f32(2)
    b = np.zeros_like(u_nom) if bias is None else bias.astype(f32)
    if sigma is not None:
        b = np.where(sigma[:, None] == 0, b, b + sigma.astype(f32)[:, None] * normals(seed, ids, tick, STREAM_ACT, A))
    return np.minimum(np.maximum(u_nom + half[None, :] * b, lo[None, :]), hi[None, :]).astype(f32)


# ------------------------------------------------------------------ scan
def scan_numpy(v, q, ln, n, s, W, settle_frac, ball_factor):
    """mh_robust_scan in float32 numpy, vectorised over envs: same expressions, same order."""
    T, E = q.shape[0] - 1, q.shape[1]
    ln = np.clip(ln, 0, T)
    o = dict(q_peak=q[0].copy(), t_peak=np.zeros(E, np.int32), settle=np.zeros(E, np.int32),
             tail_max=np.full(E, -np.inf, f32), tail_count=np.zeros(E, np.int32),
             pairs_out=np.zeros(E, np.int32), viol_out=np.zeros(E, np.int32), worst_out=np.full(E, -np.inf, f32))
    thr = f32(settle_frac) * q[0]
    tail0 = np.maximum(ln - W + 1, 0)
    tsum = np.zeros(E, np.float64)
    for t in range(T + 1):
        act = ln >= t
        qt = np.where(act, q[t], f32(0))
        up = act & (qt > o["q_peak"])
        o["q_peak"] = np.where(up, qt, o["q_peak"])
        o["t_peak"] = np.where(up, t, o["t_peak"]).astype(np.int32)
        o["settle"] = np.where(act & (qt > thr), t + 1, o["settle"]).astype(np.int32)
        tail = act & (t >= tail0)
        o["tail_max"] = np.where(tail, np.maximum(o["tail_max"], qt), o["tail_max"])
        tsum += np.where(tail, qt.astype(np.float64), 0.0)
        o["tail_count"] += tail
    o["tail_mean"] = tsum / o["tail_count"]
    r2 = f32(ball_factor) * o["tail_max"]
    for t in range(T + 1):
        act = ln >= t
        outside = act & (np.where(act, q[t], f32(0)) > r2)
        Vt = np.where(act, v[t], f32(0))
        for k in range(min(n, T - t)):
            ok = outside & (ln >= t + k + 1)
            d = np.where(ok, v[t + k + 1], f32(0)) - Vt * s[k]
            o["pairs_out"] += ok
            o["viol_out"] += ok & (d > 0)
            o["worst_out"] = np.where(ok, np.maximum(o["worst_out"], d), o["worst_out"])
    return o


def run_scan(device, v, q, ln, n, s, W, settle_frac=0.01, ball_factor=1.0):
    """mh(h)_robust_scan on numpy inputs -> dict of numpy outputs."""
    T, E = q.shape[0] - 1, q.shape[1]
    to = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dt)).to(device)  # noqa: E731
    tv, tq, tl, ts = to(v, f32), to(q, f32), to(ln, np.int32), to(s, f32)
    out = {k: torch.full((E,), -7, dtype=dt, device=device) for k, dt in R_DTYPES.items()}
    p = lambda t: R._p(device, t)  # noqa: E731
    traj = N.AuditTraj(p(tq), p(tv), None, None, p(tl), None, None, None, E, T, 1.0, 1.0)
    ro = N.RobustOut(*(p(out[k]) for k, _ in N.RobustOut._fields_))
    R._call(device, "robust_scan", ctypes.byref(traj), n, p(ts), W, settle_frac, ball_factor, ctypes.byref(ro))
    return {k: t.cpu().numpy() for k, t in out.items()}


def assert_scan_equal(got, want):
    for k in R_COUNTS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    for k in R_FLOATS:
        np.testing.assert_allclose(got[k], want[k], rtol=TOL, atol=TOL, err_msg=k)


# T = 1 with W = 5 is a window longer than the trajectory's T + 1 rows: that case must be rejected
SCAN_CASES = sorted({(E, n, T, W) for E in (1, 63, 64, 65, 257) for n in (1, 20) for W in (1, 5)
                     for T in (1, W - 1, W, W + 1)})


def check_scan_case(device, E, n, T, W, against=None):
    """One shape of SCAN_CASES against the numpy restatement (and the `against` library)."""
    v, q, ln = scan_case(E, n, T, W)
    s = R.coefs(n)[2]
    if W > T + 1:
        with pytest.raises(RuntimeError, match="tail_window outside"):
            run_scan(device, v, q, ln, n, s, W)
        return
    for frac, ball in ((0.01, 1.0), (0.5, 0.0), (0.0, 3.0)):
        got = run_scan(device, v, q, ln, n, s, W, frac, ball)
        assert_scan_equal(got, scan_numpy(v, q, ln, n, s, W, frac, ball))
        np.testing.assert_array_equal(got["tail_count"], np.minimum(ln + 1, W))
        assert np.isfinite(got["tail_mean"]).all() and np.isfinite(got["q_peak"]).all()
        if against is not None:
            assert_scan_equal(got, run_scan(against, v, q, ln, n, s, W, frac, ball))


def scan_case(E, n, T, W):
    """certificate_ref.edge_case (NaN beyond len) with len = 0 and len = T both present where E
    allows, and some q rows scaled down so that settle and the residual ball vary."""
    v, q, ln = R.edge_case(E, n, T, seed=7 + W)
    if E >= 3:
        assert (ln == 0).any() and (ln == T).any()
    rng = np.random.default_rng(E + 31 * T)
    q = (q * np.where(rng.random(q.shape) < 0.5, f32(1), f32(0.004))).astype(f32)
    return v, q, ln


# ------------------------------------------------------------------ runs
def make_env(device, name, E, seed=5):
    from msacl_amd.env.host_vector_env import make_vector_env
    return make_vector_env(name, E, seed=seed, device="cpu" if R._dev(device).type == "cpu" else None)


class RobustRun(R.AuditRun):
    """AuditRun through mh(h)_robust_begin / mh(h)_robust_step: the extra obs_meas row buffer and a
    disturbance of numpy arrays (None: the NULL default of that field; dist=False: a NULL struct)."""

    def __init__(self, env, T, keep=True, seed=1234, obs_sigma=None, obs_weight=None, act_sigma=None, act_bias=None,
                 noise_id=None, dist=True):
        super().__init__(env, T, keep)
        E, D = env.num_envs, env.obs_dim
        self.meas = torch.full((E, D), -5, dtype=torch.float32, device=self.dev)
        self.seed = seed
        to = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dt)).to(self.dev)  # noqa: E731
        self.arrays = [to(obs_sigma, f32), to(obs_weight, f32), to(act_sigma, f32), to(act_bias, f32),
                       to(noise_id, np.int32)]
        self.dist = N.Disturbance(*(R._p(self.dev, t) for t in self.arrays), seed) if dist else None

    def _d(self):
        return ctypes.byref(self.dist) if self.dist is not None else None

    def begin(self, reset_states):
        rs = None if reset_states is None else torch.as_tensor(reset_states, dtype=torch.float32).to(self.dev).contiguous()
        R._call(self.dev, "robust_begin", self.env.handle(), R._p(self.dev, rs), R._p(self.dev, self.obs),
                R._p(self.dev, self.meas), ctypes.byref(self.traj), self._d())

    def step(self, t, logits=None, act=None):
        R._call(self.dev, "robust_step", self.env.handle(), R._p(self.dev, logits), R._p(self.dev, act),
                R._p(self.dev, self.obs), R._p(self.dev, self.meas), ctypes.byref(self.traj), self._d(), t)

    def state(self):
        st, xs, sp = self.env.get_state()
        return [t.clone() for t in (st, sp) + ((xs,) if xs is not None else ())]


def injected_actions(env, E, T, seed):
    lo = torch.as_tensor(env.single_action_space.low)
    hi = torch.as_tensor(env.single_action_space.high)
    gen = torch.Generator().manual_seed(seed)
    return [(lo + (hi - lo) * torch.rand(E, env.act_dim, generator=gen)).contiguous() for _ in range(T)]


def rollout(device, name, E, T, robust=True, rs=None, acts=None, record=False, **dist):
    """Begin + T injected-action steps; returns the run (env closed) and, with record, the per-step
    copies of obs / meas (index 0: after begin)."""
    env = make_env(device, name, E)
    rs = R.audit_initial_states(name, E) if rs is None else rs
    acts = injected_actions(env, E, T, seed=E) if acts is None else acts
    run = RobustRun(env, T, **dist) if robust else R.AuditRun(env, T)
    run.begin(rs)
    hist = [(run.obs.cpu().clone(), run.meas.cpu().clone() if robust else None)]
    for t in range(T):
        run.step(t, act=acts[t].to(run.dev))
        if record:
            hist.append((run.obs.cpu().clone(), run.meas.cpu().clone() if robust else None))
    run.final_state = [t.cpu() for t in RobustRun.state(run)]
    run.hist = hist
    env.close()
    return run


TRUE_FIELDS = ("obs", "q", "traj_obs", "traj_act", "len", "status", "ret", "cost")


def assert_true_loop_equal(a, b, fields=TRUE_FIELDS):
    """Bit for bit: observation, q, trajectory columns, accumulators and the engine state."""
    for k in fields:
        assert torch.equal(getattr(a, k).cpu(), getattr(b, k).cpu()), k
    for x, y in zip(a.final_state, b.final_state):
        assert torch.equal(x, y)


# ------------------------------------------------------------------ test bodies (both libraries)
def check_zero_disturbance(device, name, E, T=8):
    """NULL disturbance and all-zero arrays: robust_step is audit_step bit for bit, obs_meas == obs."""
    A = N.host_env_info(name).act_dim
    ref = rollout(device, name, E, T, robust=False)
    ended = (ref.status != 0).cpu().numpy()
    assert ended.any() and not ended.all(), "the case must hold early exits and survivors"
    zeros = dict(obs_sigma=np.zeros(E, f32), act_sigma=np.zeros(E, f32), act_bias=np.zeros((E, A), f32),
                 noise_id=np.zeros(E, np.int32))
    for kw in (dict(dist=False), dict(), zeros):
        run = rollout(device, name, E, T, record=True, **kw)
        assert_true_loop_equal(run, ref)
        alive = torch.ones(E, dtype=torch.bool)
        for t, (o, m) in enumerate(run.hist):
            assert torch.equal(o, m)
            if t > 0:  # a live env's row is this step's true observation
                assert torch.equal(m[alive], run.traj_obs[t].cpu()[alive])
                alive = alive & (run.len.cpu() > t)


def check_frozen(device, name, E=65, T=8):
    """After an env ends, its obs_meas row, observation, accumulators and trajectory rows are
    never written again (sentinel -5 in the rows beyond its end), under a full disturbance."""
    rng = np.random.default_rng(3)
    A = N.host_env_info(name).act_dim
    env = make_env(device, name, E)
    acts = injected_actions(env, E, T, seed=E)
    run = RobustRun(env, T, obs_sigma=rng.uniform(0.01, 0.05, E), act_sigma=rng.uniform(0.05, 0.2, E),
                    act_bias=rng.uniform(-0.2, 0.2, (E, A)))
    run.begin(R.audit_initial_states(name, E))
    alive = torch.ones(E, dtype=torch.bool, device=run.dev)
    for t in range(T):
        before = [x.clone() for x in (run.obs, run.meas, run.len, run.status, run.ret, run.cost)] + run.state()
        run.step(t, act=acts[t].to(run.dev))
        after = [run.obs, run.meas, run.len, run.status, run.ret, run.cost] + run.state()
        frozen = ~alive
        for a, b in zip(before, after):
            assert torch.equal(a[frozen], b[frozen])
        assert not run.q[t + 1][frozen].any()
        assert (run.traj_obs[t + 1][frozen] == -5).all() and (run.traj_act[t][frozen] == -5).all()
        assert (run.len[alive] == t + 1).all()
        alive = alive & (run.status == 0)
    assert (~alive).any() and alive.any()
    env.close()


def sensor_case(name, E):
    rng = np.random.default_rng(11)
    D = N.host_env_info(name).obs_dim
    sigma = rng.uniform(0.01, 0.5, E).astype(f32)
    sigma[::3] = 0
    return dict(obs_sigma=sigma, obs_weight=rng.uniform(0.5, 2.0, D).astype(f32),
                noise_id=rng.integers(0, 1 << 20, E).astype(np.int32), seed=0x1234567887654321)


def check_sensor_noise(device, name, E=65, T=8):
    """Sensor noise enters only through obs_meas: the true loop is the undisturbed one bit for bit,
    obs_meas - obs is sigma * w_i * xi of the restatement, sigma == 0 rows are the true rows."""
    kw = sensor_case(name, E)
    ref = rollout(device, name, E, T, robust=False)
    run = rollout(device, name, E, T, record=True, **kw)
    assert_true_loop_equal(run, ref)
    zero = torch.as_tensor(kw["obs_sigma"] == 0)
    alive = np.ones(E, bool)
    ln = run.len.cpu().numpy()
    for t, (o, m) in enumerate(run.hist):
        assert torch.equal(o[zero], m[zero])
        want = measure_numpy(o.numpy(), kw["obs_sigma"], kw["obs_weight"], kw["seed"], kw["noise_id"], t)
        np.testing.assert_allclose(m.numpy()[alive], want[alive], rtol=TOL, atol=TOL)
        nz = alive & ~zero.numpy()
        assert (m.numpy()[nz] != o.numpy()[nz]).any()
        alive = alive & (ln > t)  # rows of an env that ended at step <= t keep their last draw
    return run


def actuator_case(name, E, with_sigma):
    rng = np.random.default_rng(13)
    A = N.host_env_info(name).act_dim
    bias = rng.uniform(-0.5, 0.5, (E, A)).astype(f32)
    bias[:6] = np.array([3.0, -3.0, 2.5, -2.5, 0.0, -0.0], f32)[:, None]  # saturate both ends
    kw = dict(act_bias=bias, seed=77)
    if with_sigma:
        sigma = rng.uniform(0.05, 1.0, E).astype(f32)
        sigma[1::4] = 0
        kw.update(act_sigma=sigma, noise_id=rng.integers(0, 1 << 20, E).astype(np.int32))
    return kw


def check_actuator(device, name, with_sigma, E=65, T=8):
    """traj_act is the applied action: exactly clip(u_nom + half * bias) with bias only; the
    restatement at 1e-5 and inside the action box with act_sigma."""
    kw = actuator_case(name, E, with_sigma)
    env = make_env(device, name, E)
    lo, hi = (np.asarray(x, f32) for x in (env.single_action_space.low, env.single_action_space.high))
    env.close()
    run = rollout(device, name, E, T, **kw)
    acts = injected_actions(make_env("cpu", name, E), E, T, seed=E)
    ln = run.len.cpu().numpy()
    ids = kw.get("noise_id", np.arange(E))
    sat_lo = sat_hi = changed = 0
    for t in range(T):
        live = ln > t
        got = run.traj_act[t].cpu().numpy()[live]
        want = actuate_numpy(acts[t].numpy(), lo, hi, kw["act_bias"], kw.get("act_sigma"), kw["seed"], ids, t)[live]
        if with_sigma:
            np.testing.assert_allclose(got, want, rtol=TOL, atol=TOL)
        else:
            np.testing.assert_array_equal(got, want)
        assert (got >= lo).all() and (got <= hi).all()
        sat_lo, sat_hi = sat_lo + (got == lo).sum(), sat_hi + (got == hi).sum()
        changed += (got != acts[t].numpy()[live]).sum()
    assert sat_lo > 0 and sat_hi > 0 and changed > 0
    return run


def check_noise_id(device, name="DuctedFan", T=8):
    """Equal noise_id, sigmas and initial state: bit-identical trajectories; different ids differ."""
    E = 6
    rs = np.ascontiguousarray(np.tile(R.audit_initial_states(name, 16)[12:13], (E, 1)))
    env = make_env(device, name, E)
    acts = [a[:1].repeat(E, 1).contiguous() for a in injected_actions(env, E, T, seed=1)]
    env.close()
    A = N.host_env_info(name).act_dim
    ids = np.array([5, 5, 9, 5, 9, 1 << 20], np.int32)
    run = rollout(device, name, E, T, rs=rs, acts=acts, record=True, obs_sigma=np.full(E, 0.1, f32),
                  act_sigma=np.full(E, 0.3, f32), act_bias=np.zeros((E, A), f32), noise_id=ids)
    assert (run.len == T).all()
    obs = run.traj_obs.cpu()
    meas = torch.stack([m for _, m in run.hist])
    for a, b in ((0, 1), (0, 3), (2, 4)):
        assert torch.equal(obs[:, a], obs[:, b]) and torch.equal(meas[:, a], meas[:, b])
        assert torch.equal(run.traj_act.cpu()[:, a], run.traj_act.cpu()[:, b])
    for a, b in ((0, 2), (0, 5), (2, 5)):
        assert not torch.equal(obs[1:, a], obs[1:, b]) and not torch.equal(meas[:, a], meas[:, b])
        assert not torch.equal(run.traj_act.cpu()[:, a], run.traj_act.cpu()[:, b])


def check_rejections(device):
    """Every MH_EINVAL case of the robust entry points."""
    name, E, T = "DuctedFan", 8, 4
    env = make_env(device, name, E)
    other = make_env(device, name, E + 1)
    run = RobustRun(env, T)
    rs = R.audit_initial_states(name, E)
    act = injected_actions(env, E, 1, seed=0)[0].to(run.dev)
    run.begin(rs)
    h, dev = env.handle(), run.dev
    p = lambda t: R._p(dev, t)  # noqa: E731
    tr = ctypes.byref(run.traj)

    def begin(**kw):
        a = dict(h=h, obs=p(run.obs), meas=p(run.meas), traj=tr)
        a.update(kw)
        R._call(dev, "robust_begin", a["h"], None, a["obs"], a["meas"], a["traj"], None)

    def step(**kw):
        a = dict(h=h, logits=None, act=p(act), obs=p(run.obs), meas=p(run.meas), traj=tr, t=0)
        a.update(kw)
        R._call(dev, "robust_step", a["h"], a["logits"], a["act"], a["obs"], a["meas"], a["traj"], None, a["t"])

    for call in (begin, step):
        for kw, msg in ((dict(h=None), "null handle"), (dict(traj=None), "null handle or trajectory"),
                        (dict(obs=None), "null obs"), (dict(meas=None), "null obs or obs_meas"),
                        (dict(h=other.handle()), "num_envs differs")):
            with pytest.raises(RuntimeError, match=msg):
                call(**kw)
    with pytest.raises(RuntimeError, match="need logits or act_in"):
        step(act=None)
    for t in (-1, T):
        with pytest.raises(RuntimeError, match=r"t outside \[0, T\)"):
            step(t=t)
    # misaligned rows: DuctedFan's obs rows (6 floats) and action rows (2 floats) need 8 bytes
    off = lambda t: ctypes.c_void_p(t.data_ptr() + 4)  # noqa: E731
    spare = torch.zeros(E * 6 + 2, dtype=torch.float32, device=dev)
    for kw in (dict(obs=off(spare)), dict(meas=off(spare)), dict(act=off(spare))):
        with pytest.raises(RuntimeError, match="misaligned rows"):
            step(**kw)
    with pytest.raises(RuntimeError, match="misaligned rows"):
        begin(meas=off(spare))
    misal = N.AuditTraj.from_buffer_copy(run.traj)
    misal.traj_obs = run.traj_obs.data_ptr() + 4
    with pytest.raises(RuntimeError, match="misaligned rows"):
        step(traj=ctypes.byref(misal))
    incomplete = N.AuditTraj.from_buffer_copy(run.traj)
    incomplete.len = None
    with pytest.raises(RuntimeError, match="incomplete trajectory"):
        step(traj=ctypes.byref(incomplete))
    step()  # and the accepted call still works
    assert (run.len == 1).all()
    env.close()
    other.close()
    # scan
    v, q, ln = R.edge_case(4, 2, 3)
    s = R.coefs(64)[2]
    for n in (0, 65):
        with pytest.raises(RuntimeError, match="n outside"):
            run_scan(device, v, q, ln, n, s, 1)
    for W in (0, 5, -1):
        with pytest.raises(RuntimeError, match=r"tail_window outside \[1, T \+ 1\]"):
            run_scan(device, v, q, ln, 2, s, W)
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="settle_frac"):
            run_scan(device, v, q, ln, 2, s, 1, settle_frac=bad)
        with pytest.raises(RuntimeError, match="ball_factor"):
            run_scan(device, v, q, ln, 2, s, 1, ball_factor=bad)
    big = np.zeros((1002, 1), f32)
    with pytest.raises(RuntimeError, match="T outside"):
        run_scan(device, big, big, np.zeros(1, np.int32), 2, s, 1)
    tq = torch.zeros(4, 4, device=dev)
    tl = torch.zeros(4, dtype=torch.int32, device=dev)
    out = {k: torch.zeros(4, dtype=dt, device=dev) for k, dt in R_DTYPES.items()}
    ro = N.RobustOut(*(p(out[k]) for k, _ in N.RobustOut._fields_))
    ts = torch.ones(2, device=dev)
    full = N.AuditTraj(p(tq), p(tq), None, None, p(tl), None, None, None, 4, 3, 1.0, 1.0)
    no_v = N.AuditTraj(p(tq), None, None, None, p(tl), None, None, None, 4, 3, 1.0, 1.0)
    no_out = N.RobustOut(*(p(out[k]) if k != "settle" else None for k, _ in N.RobustOut._fields_))
    for args, msg in (((None, 2, p(ts), 1, 0.01, 1.0, ctypes.byref(ro)), "null argument"),
                      ((ctypes.byref(full), 2, None, 1, 0.01, 1.0, ctypes.byref(ro)), "null argument"),
                      ((ctypes.byref(full), 2, p(ts), 1, 0.01, 1.0, None), "null argument"),
                      ((ctypes.byref(no_v), 2, p(ts), 1, 0.01, 1.0, ctypes.byref(ro)), "incomplete trajectory"),
                      ((ctypes.byref(full), 2, p(ts), 1, 0.01, 1.0, ctypes.byref(no_out)), "incomplete outputs")):
        with pytest.raises(RuntimeError, match=msg):
            R._call(dev, "robust_scan", *args)
    R._call(dev, "robust_scan", ctypes.byref(full), 2, p(ts), 1, 0.01, 1.0, ctypes.byref(ro))
