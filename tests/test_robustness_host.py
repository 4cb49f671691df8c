"""CPU: the robustness sweep on the engine's CPU build (mhh_robust_begin / mhh_robust_step /
mhh_robust_scan; csrc/robustness.h is the code the gfx950 kernels run). The disturbed step against
the audit step and a numpy restatement of the noise, the scan against a numpy restatement and
hand-built columns, RobustnessAuditor end to end. No GPU needed."""
import numpy as np
import pytest
import torch

import certificate_ref as R
import robustness_ref as RR

f32 = np.float32
DEV = "cpu"


@pytest.mark.parametrize("E", [65, 257])
@pytest.mark.parametrize("name", R.NAMES)
def test_zero_disturbance_is_the_audit_step(name, E):
    RR.check_zero_disturbance(DEV, name, E)


@pytest.mark.parametrize("name", ["VanderPol", "QuadTracking"])
def test_frozen_envs_are_never_written(name):
    RR.check_frozen(DEV, name)


@pytest.mark.parametrize("name", ["VanderPol", "DuctedFan", "QuadTracking"])  # D = 2, 6, 12
def test_sensor_noise_enters_only_through_obs_meas(name):
    RR.check_sensor_noise(DEV, name)


@pytest.mark.parametrize("with_sigma", [False, True])
@pytest.mark.parametrize("name", ["VanderPol", "DuctedFan", "QuadTracking"])  # A = 1, 2, 4
def test_actuator_disturbance(name, with_sigma):
    RR.check_actuator(DEV, name, with_sigma)


def test_noise_id_pairs_realisations():
    RR.check_noise_id(DEV)


@pytest.mark.parametrize("name", R.NAMES)
def test_noise_moments(name):
    """xi = (obs_meas - obs) / sigma over E = 257 envs and ticks 0..8 (the rows of live envs), all D
    components: N samples of a standard normal. The sample mean has standard error 1 / sqrt(N),
    the sample variance sqrt(2 / (N - 1)); both must lie within 5 of them. (The float32
    subtraction adds an error below 1e-5 of a unit, far under either bound.)"""
    E, T, sigma = 257, 8, 0.25
    run = RR.rollout(DEV, name, E, T, record=True, obs_sigma=np.full(E, sigma, f32), seed=99)
    ln = run.len.numpy()
    xi = np.concatenate([(m.numpy().astype(np.float64) - o.numpy().astype(np.float64))[ln >= t].ravel() / sigma
                         for t, (o, m) in enumerate(run.hist)])
    n = xi.size
    assert n >= E * run.obs.shape[1] * 2
    assert abs(xi.mean()) < 5.0 / np.sqrt(n)
    assert abs(xi.var(ddof=1) - 1.0) < 5.0 * np.sqrt(2.0 / (n - 1))
    # the actuator's stream: zeta = (u - u_nom) / (half * sigma) for nominal actions in the middle 40 %
    # of the box, which sigma = 0.05 cannot push to an edge (that would take |zeta| > 12). The float32
    # rounding of u adds at most ulp(u) / (half * sigma) < 1e-5 per sample.
    sg = 0.05
    run = RR.rollout(DEV, name, E, T, act_sigma=np.full(E, sg, f32), seed=99)
    env = RR.make_env(DEV, name, E)
    acts = RR.injected_actions(env, E, T, seed=E)
    lo, hi = (np.asarray(x, np.float64) for x in (env.single_action_space.low, env.single_action_space.high))
    zs = []
    for t in range(T):
        u, un = run.traj_act[t].numpy().astype(np.float64), acts[t].numpy().astype(np.float64)
        keep = (run.len.numpy() > t)[:, None] & (un > lo + 0.3 * (hi - lo)) & (un < hi - 0.3 * (hi - lo))
        zs.append(((u - un) / ((hi - lo) / 2 * sg))[keep])
    z = np.concatenate(zs)
    assert z.size >= 200
    assert abs(z.mean()) < 5.0 / np.sqrt(z.size)
    assert abs(z.var(ddof=1) - 1.0) < 5.0 * np.sqrt(2.0 / (z.size - 1))


@pytest.mark.parametrize("E,n,T,W", RR.SCAN_CASES)
def test_scan_matches_numpy(E, n, T, W):
    RR.check_scan_case(DEV, E, n, T, W)


def test_scan_hand_built_columns():
    """Known answers: monotone decay at exactly the certificate's rate (settles early, no violation
    outside the ball), the same with a late spike (not settled, peak at the spike), q = 0."""
    T, n, W = 40, 5, 4
    s = R.coefs(n)[2]
    rate = float(s[0])  # (1 - eta): V_{t+k} = s_{k-1} V_t up to rounding, made strict by 0.999
    t = np.arange(T + 1)
    q = np.stack([(f32(2.0) * (rate * 0.999) ** t).astype(f32)] * 3, 1)
    q[T - 1, 1] = f32(5.0)
    q[:, 2] = 0
    v = (f32(1.5) * q).astype(f32)
    ln = np.full(3, T, np.int32)
    got = RR.run_scan(DEV, v, q, ln, n, s, W, 0.01, 1.0)
    first_below = int(np.argmax(q[:, 0] <= f32(0.01) * q[0, 0]))
    np.testing.assert_array_equal(got["settle"], [first_below, T, 0])   # col 1: last q_t > thr is the spike at T - 1
    assert 0 < got["settle"][0] < T
    np.testing.assert_array_equal(got["t_peak"], [0, T - 1, 0])
    np.testing.assert_array_equal(got["q_peak"], [q[0, 0], f32(5.0), 0])
    np.testing.assert_array_equal(got["tail_count"], [W, W, W])
    np.testing.assert_array_equal(got["tail_max"], [q[T - W + 1, 0], f32(5.0), 0])
    np.testing.assert_allclose(got["tail_mean"], q[T - W + 1:].astype(np.float64).mean(0), rtol=1e-12)
    # col 0: starts outside the ball are t <= T - W (q_t > tail_max = q_{T-W+1}); all decay
    assert got["viol_out"][0] == 0 and got["worst_out"][0] < 0
    assert got["pairs_out"][0] == sum(min(n, T - t0) for t0 in range(T - W + 1))
    # col 1: the ball is the spike itself, nothing starts outside it; col 2: q = 0 is never outside
    np.testing.assert_array_equal(got["pairs_out"][1:], [0, 0])
    assert np.isneginf(got["worst_out"][1:]).all()
    # the spike as the LAST row with a later-ending tail that excludes it: not settled means len + 1
    q2 = q[:, :1].copy()
    q2[T, 0] = f32(1.0)
    got = RR.run_scan(DEV, (f32(1.5) * q2).astype(f32), q2, ln[:1], n, s, 1, 0.01, 0.0)
    assert got["settle"][0] == T + 1 and got["tail_max"][0] == f32(1.0) and got["t_peak"][0] == 0
    # ball_factor = 0: every start with q_t > 0 counts, so the pair that ends on the spike's V violates
    assert got["viol_out"][0] > 0 and got["worst_out"][0] > 0
    RR.assert_scan_equal(got, RR.scan_numpy((f32(1.5) * q2).astype(f32), q2, ln[:1], n, s, 1, 0.01, 0.0))


def test_rejections():
    RR.check_rejections(DEV)


def _auditor(tmp_path, name, auditor_name="robustness_auditor", **kw):
    from msacl_amd.create_pkg.create_auditor import create_auditor
    from msacl_amd.create_pkg.create_envs import create_envs
    from msacl_amd.utils.config import default_msacl_args
    from msacl_amd.utils.init_args import init_args
    args = default_msacl_args(env_name=name, env_num=1, save_folder=str(tmp_path), seed=0, device="cpu",
                              policy_hidden_sizes=[64, 64], value_hidden_sizes=[64, 64],
                              lyapunov_hidden_sizes=[64, 64], **kw)
    args = init_args(create_envs(**args), **args)
    args.pop("auditor_name", None)
    return create_auditor(auditor_name, **args)


def test_cpu_sweep_end_to_end(tmp_path):
    """RobustnessAuditor(device="cpu"), VanderPol, three levels (zero, sensor, actuator), M = 33,
    horizon 32: level 0 is CertificateAuditor.audit bit for bit, the summaries echo their
    settings, every level starts from the same states."""
    from msacl_amd.create_pkg import create_auditor
    from msacl_amd.trainer.robustness_auditor import RobustnessAuditor
    assert create_auditor.registry.get("robustness_auditor").entry_point is RobustnessAuditor
    au = _auditor(tmp_path, "VanderPol")
    assert isinstance(au, RobustnessAuditor)
    M, T = 33, 32
    init = R.audit_initial_states("VanderPol", M)
    levels = [dict(), dict(obs_sigma=0.05), dict(act_sigma=0.2, act_bias=0.1)]
    res = au.sweep(levels, initial_states=init, horizon=T, tail_window=8, keep_trajectory=True)
    ref = au.audit(initial_states=init, horizon=T, keep_trajectory=True)   # the inherited audit
    for k in R.COUNTS + R.FLOATS + ("len", "status", "ret", "cost", "q0", "q_end"):
        assert torch.equal(res[k][:M], ref[k]), k
    valid = torch.arange(T + 1)[:, None] <= ref["len"][None, :]
    for k in ("q", "v", "obs"):
        assert torch.equal(res[k][:, :M][valid], ref[k][valid]), k
    assert torch.equal(res["act"][:, :M][valid[1:]], ref["act"][valid[1:]])
    assert (ref["len"] < T).any() and (ref["len"] == T).any()
    obs0 = res["obs"][0].view(3, M, -1)
    assert torch.equal(obs0[0], obs0[1]) and torch.equal(obs0[0], obs0[2])
    np.testing.assert_array_equal(obs0[0].numpy(), init)
    assert not torch.equal(res["q"][:, M:2 * M], res["q"][:, :M])          # the noise does something
    assert not torch.equal(res["act"][:, 2 * M:], res["act"][:, :M])
    np.testing.assert_array_equal(res["level"].numpy(), np.repeat(np.arange(3), M))
    np.testing.assert_array_equal(res["trajectory"].numpy(), np.tile(np.arange(M), 3))
    # the robust scan's outputs are the restatement's
    s = au.coefs[2].numpy()
    want = RR.scan_numpy(res["v"].numpy(), res["q"].numpy(), res["len"].numpy(), au.n_step, s, 8, 0.01, 1.0)
    RR.assert_scan_equal({k: res[k].numpy() for k in RR.R_COUNTS + RR.R_FLOATS}, want)
    lv = res["levels"]
    assert len(lv) == 3
    keys = {"level", "obs_sigma", "act_sigma", "act_bias", "trajectories", "terminated", "cost_per_step", "tail_rms",
            "tail_max", "settled", "settle_mean", "decay_ok", "decay_ok_outside"}
    for i, d in enumerate(lv):
        assert set(d) == keys and d["level"] == i and d["trajectories"] == M
        assert np.isfinite([x for k, x in d.items() if k != "act_bias"]).all()
    assert [d["obs_sigma"] for d in lv] == [0.0, 0.05, 0.0] and [d["act_sigma"] for d in lv] == [0.0, 0.0, 0.2]
    assert [d["act_bias"] for d in lv] == [[0.0], [0.0], [pytest.approx(0.1)]]
    sl = slice(M, 2 * M)
    assert lv[1]["terminated"] == pytest.approx((res["status"][sl] == 1).double().mean().item())
    assert lv[1]["cost_per_step"] == pytest.approx(res["cost"][sl].sum().item() / res["len"][sl].sum().item())
    assert lv[1]["tail_rms"] == pytest.approx(res["tail_mean"][sl].mean().sqrt().item())
    assert lv[1]["tail_max"] == pytest.approx(res["tail_max"][sl].max().item())
    assert lv[1]["settled"] == pytest.approx((res["settle"][sl] <= res["len"][sl]).double().mean().item())
    assert lv[1]["decay_ok_outside"] == pytest.approx((res["viol_out"][sl] == 0).double().mean().item())
    assert lv[0]["decay_ok"] == pytest.approx(ref["summary"]["decay_ok"])
    assert lv[0]["terminated"] == pytest.approx(ref["summary"]["terminated"])
    assert lv[0]["cost_per_step"] == pytest.approx(ref["summary"]["cost_per_step"])
    # drawn initial states: drawn once, shared by every level; independent noise runs too
    res2 = au.sweep(levels[:2], trajectories=9, horizon=4, tail_window=100, common_noise=False, keep_trajectory=True)
    o2 = res2["obs"][0].view(2, 9, -1)
    assert torch.equal(o2[0], o2[1]) and res2["initial_states"].shape == (9, 2)
    assert len(torch.unique(o2[0], dim=0)) == 9
    for bad in ([], [dict(obs_sigma=-1.0)], [dict(act_sigma=float("nan"))], [dict(sigma=1.0)], [dict(act_bias=[0.0, 1.0])]):
        with pytest.raises(ValueError):
            au.sweep(bad, initial_states=init, horizon=4)
    au.close()
