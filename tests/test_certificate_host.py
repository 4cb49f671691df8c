"""CPU: the closed-loop certificate audit on the engine's CPU build (mhh_audit_begin /
mhh_audit_step / mhh_certificate_scan; csrc/certificate.h is the code the gfx950 kernels run).
The scan against the reference's Lyapunov-update fixture and against a numpy restatement on edge
shapes; the audit step against mhh_env_step. No GPU needed."""
import numpy as np
import pytest

import certificate_ref as R
import msacl_amd._native as N

f32 = np.float32


@pytest.fixture(scope="module")
def golden():
    return R.golden_case()


def test_scan_matches_the_reference_lyapunov_update(golden):
    """tests/golden/msacl_update_bench.npz: 256 contiguous windows, n = 20, fed as E = 256
    trajectories of T = 20 with len = 20, alpha1 = 1, alpha2 = 2, eta = 0.15, lambda = 0.95. The
    fixture's ESL row and lya_diff describe the pairs that start at t = 0; the scan counts every
    start, so the t = 0 share is the full scan minus the scan of the trajectories from t = 1 on."""
    g, v, q = golden
    E, n = 256, 20
    assert v.shape == (n + 1, E) and int(g["cfg_n"]) == n
    c, w, s = R.coefs(n)
    full_len = np.full(E, n, np.int32)
    full = R.run_scan("cpu", v, q, full_len, n, c, w, s, 1.0, 2.0)
    tail = R.run_scan("cpu", v[1:], q[1:], full_len - 1, n, c, w, s, 1.0, 2.0)
    V0 = g["it0/lyapunov_update0/lya_obs"][:, :1]
    V2, ESL = g["it0/lyapunov_update0/lya_obs2"], g["it0/lyapunov_update0/ESL"]
    # exponential-stability labels: zero mismatches (the fixture's smallest margin is 2.5e-5)
    np.testing.assert_array_equal(full["esl_neg"] - tail["esl_neg"], (ESL == -1).sum(1))
    # decay violations of the t = 0 pairs: exact (smallest |V2 - s V0| in the fixture: 0.12)
    np.testing.assert_array_equal(full["lya_viol"] - tail["lya_viol"], (V2 > s[None, :] * V0).sum(1))
    np.testing.assert_array_equal(full["pairs"] - tail["pairs"], np.full(E, n))
    np.testing.assert_array_equal(full["pairs"], np.full(E, n * (n + 1) // 2))
    # training-consistent residual of the one full window, t = 0
    want = (w[None, :] * np.maximum(ESL * (V2 - s[None, :] * V0), 0)).sum(1)
    np.testing.assert_allclose(full["resid"][0], want, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(full["resid_sum"], want, rtol=1e-5, atol=1e-5)
    assert not full["resid"][1:].any() and (full["windows"] == 1).all()
    # bounds, exact: t = 0..20 from the arrays fed, and the fixture's own V(obs) at t = 0..19
    np.testing.assert_array_equal(full["lo_count"], (v < f32(1) * q).sum(0))
    np.testing.assert_array_equal(full["hi_count"], (v > f32(2) * q).sum(0))
    head = R.run_scan("cpu", v, q, full_len - 1, n, c, w, s, 1.0, 2.0)
    pw = (g["in_obs"] * g["in_obs"]).sum(-1, dtype=f32)
    lya = g["it0/lyapunov_update0/lya_obs"]
    assert head["lo_count"].sum() == (lya < pw).sum() == 0
    assert abs(head["hi_count"].sum() / (E * n) - 0.993) < 5e-4
    assert abs((lya > f32(2) * pw).mean() - 0.993) < 5e-4
    R.assert_scan_equal(full, R.scan_numpy(v, q, full_len, n, c, w, s, 1.0, 2.0))


@pytest.mark.parametrize("E,n,T", R.EDGE_CASES)
def test_scan_edge_shapes(E, n, T):
    """Ragged len (0, 1 and T among them), NaN beyond len (never read), windows longer than,
    equal to and shorter than the trajectory, one lane to more than one block."""
    v, q, ln = R.edge_case(E, n, T)
    c, w, s = R.coefs(n)
    got = R.run_scan("cpu", v, q, ln, n, c, w, s, 1.0, 2.0)
    R.assert_scan_equal(got, R.scan_numpy(v, q, ln, n, c, w, s, 1.0, 2.0))
    assert all(np.isfinite(got[k]).all() for k in ("lo_excess", "hi_excess", "resid_sum", "resid"))
    np.testing.assert_array_equal(got["windows"], np.maximum(ln - n + 1, 0))


def test_scan_rejects_unsupported_shapes():
    v, q, ln = R.edge_case(4, 2, 3)
    c, w, s = R.coefs(65)
    for n in (0, 65):
        with pytest.raises(RuntimeError, match="n outside"):
            R.run_scan("cpu", v, q, ln, n, c, w, s, 1.0, 2.0)
    big = np.zeros((1002, 1), f32)
    with pytest.raises(RuntimeError, match="T outside"):
        R.run_scan("cpu", big, big, np.zeros(1, np.int32), 2, c, w, s, 1.0, 2.0)


@pytest.mark.parametrize("name", R.NAMES)
def test_audit_step_equals_env_step_until_frozen(name):
    R.check_injected_parity("cpu", name, 65, T=8)


def test_state_grid_and_registry():
    from msacl_amd.create_pkg import create_auditor
    from msacl_amd.trainer.certificate_auditor import CertificateAuditor, state_grid
    from msacl_amd.utils.config import default_msacl_args
    assert create_auditor.registry.get("certificate_auditor").entry_point is CertificateAuditor
    a = default_msacl_args()
    assert (a["auditor_name"], a["num_audit_states"], a["audit_horizon"]) == ("certificate_auditor", 1024, 1000)
    g = state_grid("DuctedFan", dims=(0, 3), points=5, span=(2.0, 1.0))
    assert g.shape == (25, 6) and g.dtype == np.float32
    assert not g[:, [1, 2, 4, 5]].any()
    np.testing.assert_allclose(np.unique(g[:, 0]), np.linspace(-2, 2, 5), rtol=1e-6)
    np.testing.assert_allclose(np.unique(g[:, 3]), np.linspace(-1, 1, 5), rtol=1e-6)
    info = N.host_env_info("VanderPol")
    assert np.abs(state_grid("VanderPol", points=3)).max() == pytest.approx(0.9 * info.obs_high[0])
    with pytest.raises(ValueError):
        state_grid("QuadTracking")
    with pytest.raises(ValueError):
        state_grid("VanderPol", dims=(0, 2))


def test_cpu_audit_end_to_end(tmp_path):
    """CertificateAuditor on device="cpu": the trajectories freeze where they end, and the summary
    and the kept trajectory agree with the per-env outputs."""
    import torch
    from msacl_amd.create_pkg.create_auditor import create_auditor
    from msacl_amd.create_pkg.create_envs import create_envs
    from msacl_amd.utils.config import default_msacl_args
    from msacl_amd.utils.init_args import init_args
    args = default_msacl_args(env_name="VanderPol", env_num=1, save_folder=str(tmp_path), seed=0, device="cpu",
                              policy_hidden_sizes=[32, 32], value_hidden_sizes=[32, 32],
                              lyapunov_hidden_sizes=[32, 32], lyapunov_output_dim=64)
    args = init_args(create_envs(**args), **args)
    au = create_auditor(**args)
    init = R.audit_initial_states("VanderPol", 33)
    T = 40
    res = au.audit(initial_states=init, horizon=T, keep_trajectory=True)
    ln, st = res["len"].numpy(), res["status"].numpy()
    assert ((st == 0) == (ln == T)).all() and (ln[st != 0] < T).all() and (st != 0).any() and (st == 0).any()
    obs, q, v = res["obs"], res["q"], res["v"]
    np.testing.assert_allclose(q[0].numpy(), (init ** 2).sum(-1), rtol=1e-6)
    for e in (0, 8, 32):
        L = int(ln[e])
        np.testing.assert_allclose(q[:L + 1, e].numpy(), (obs[:L + 1, e].numpy() ** 2).sum(-1), rtol=1e-6)
        np.testing.assert_allclose(v[:L + 1, e].numpy(), au.networks.lyapunov(obs[:L + 1, e]).detach().numpy(),
                                   rtol=1e-5, atol=1e-6)
        mode = au.networks.create_action_distributions(au.networks.policy(obs[:L, e])).mode().detach()
        np.testing.assert_allclose(res["act"][:L, e].numpy(), mode.numpy(), rtol=1e-5, atol=1e-5)
        assert float(res["q_end"][e]) == float(q[L, e])
    np.testing.assert_allclose(res["cost"].numpy(), [float(q[1:int(L) + 1, e].double().sum()) * 100.0
                                                      for e, L in enumerate(ln)], rtol=1e-6)
    c, w, s = (t.numpy() for t in au.coefs)
    vv, qq = v.numpy().copy(), q.numpy().copy()
    R.assert_scan_equal({k: res[k].numpy() for k in R.COUNTS + R.FLOATS + ("resid",)},
                        R.scan_numpy(vv, qq, ln, au.n_step, c, w, s, 1.0, 2.0))
    sm = res["summary"]
    assert set(sm) == {"bounds_ok", "decay_ok", "terminated", "residual", "cost_per_step", "contraction_rate"}
    assert sm["terminated"] == pytest.approx((st == 1).mean())
    assert sm["cost_per_step"] == pytest.approx(res["cost"].sum().item() / ln.sum())
    assert np.isfinite(list(sm.values())).all()
    assert torch.equal(au.audit(initial_states=init, horizon=T)["len"], res["len"])  # deterministic, re-runnable
    au.close()
