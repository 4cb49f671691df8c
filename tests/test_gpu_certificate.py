"""GPU: the closed-loop certificate audit on the device (csrc/certificate.hip: k_audit_step<Env>,
k_certificate_scan) against the engine's CPU build, the device vector env, the action
distribution's mode() and the reference evaluator's fixtures; CertificateAuditor end to end and
the trainer's certificate_interval hook."""
import os

import numpy as np
import pytest
import torch

import certificate_ref as R
import msacl_amd  # noqa: F401
from msacl_amd.utils.config import build_pipeline, default_msacl_args

pytestmark = pytest.mark.gpu
DEV = "cuda"
SMALL = dict(policy_hidden_sizes=[64, 64], value_hidden_sizes=[64, 64], lyapunov_hidden_sizes=[64, 64])


def _auditor(tmp_path, name, **kw):
    from msacl_amd.create_pkg.create_auditor import create_auditor
    from msacl_amd.create_pkg.create_envs import create_envs
    from msacl_amd.utils.init_args import init_args
    args = default_msacl_args(env_name=name, env_num=4, save_folder=str(tmp_path), seed=0, **SMALL, **kw)
    args = init_args(create_envs(**args), **args)
    return create_auditor(**args)


# ------------------------------------------------------------------ scan: device vs the host library
def test_scan_golden_equals_host_library():
    g, v, q = R.golden_case()
    n, E = 20, 256
    c, w, s = R.coefs(n)
    ln = np.full(E, n, np.int32)
    got = R.run_scan(DEV, v, q, ln, n, c, w, s, 1.0, 2.0)
    R.assert_scan_equal(got, R.run_scan("cpu", v, q, ln, n, c, w, s, 1.0, 2.0))
    V0 = g["it0/lyapunov_update0/lya_obs"][:, :1]
    V2, ESL = g["it0/lyapunov_update0/lya_obs2"], g["it0/lyapunov_update0/ESL"]
    tail = R.run_scan(DEV, v[1:], q[1:], ln - 1, n, c, w, s, 1.0, 2.0)
    np.testing.assert_array_equal(got["esl_neg"] - tail["esl_neg"], (ESL == -1).sum(1))
    np.testing.assert_array_equal(got["lya_viol"] - tail["lya_viol"], (V2 > s[None, :] * V0).sum(1))
    want = (w[None, :] * np.maximum(ESL * (V2 - s[None, :] * V0), 0)).sum(1)
    np.testing.assert_allclose(got["resid"][0], want, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("E,n,T", R.EDGE_CASES)
def test_scan_edge_shapes_equal_host_library(E, n, T):
    v, q, ln = R.edge_case(E, n, T)
    c, w, s = R.coefs(n)
    got = R.run_scan(DEV, v, q, ln, n, c, w, s, 1.0, 2.0)
    R.assert_scan_equal(got, R.run_scan("cpu", v, q, ln, n, c, w, s, 1.0, 2.0))
    assert all(np.isfinite(got[k]).all() for k in ("lo_excess", "hi_excess", "resid_sum", "resid"))


def test_scan_rejects_unsupported_shapes():
    v, q, ln = R.edge_case(4, 2, 3)
    c, w, s = R.coefs(65)
    for n in (0, 65):
        with pytest.raises(RuntimeError, match="n outside"):
            R.run_scan(DEV, v, q, ln, n, c, w, s, 1.0, 2.0)


# ------------------------------------------------------------------ step
@pytest.mark.parametrize("E", [65, 257])
@pytest.mark.parametrize("name", R.NAMES)
def test_audit_step_equals_vector_env_step_until_frozen(name, E):
    R.check_injected_parity(DEV, name, E, T=8)


@pytest.mark.parametrize("name", ["VanderPol", "DuctedFan", "QuadTracking"])  # A = 1, 2, 4
def test_mode_action_matches_the_distribution(name):
    """The kernel's action for random logits against TanhGaussDistribution.mode() in float64
    (means up to +-20: saturated tanh), rtol = atol = 1e-5."""
    from msacl_amd.env.hip_vector_env import HipVectorEnv
    from msacl_amd.utils.act_distribution_cls import TanhGaussDistribution
    E = 257
    env = HipVectorEnv(name, E, seed=1)
    A = env.act_dim
    gen = torch.Generator().manual_seed(A)
    mean = torch.randn(E, A, generator=gen) * 2.0
    mean[:64] = (torch.rand(64, A, generator=gen) * 2 - 1) * 20.0
    mean[64:72] = torch.tensor([0.0, -0.0, 1e-4, -1e-4, 20.0, -20.0, 9.0, -9.0])[:, None]
    logits = torch.cat([mean, torch.rand(E, A, generator=gen) + 0.1], dim=1).to(DEV).contiguous()
    run = R.AuditRun(env, 1)
    run.begin(None)
    run.step(0, logits=logits)
    assert (run.len == 1).all()
    dist = TanhGaussDistribution(logits.double().cpu())
    dist.act_high_lim = torch.as_tensor(env.single_action_space.high).double()
    dist.act_low_lim = torch.as_tensor(env.single_action_space.low).double()
    np.testing.assert_allclose(run.traj_act[0].cpu().numpy(), dist.mode().numpy(), rtol=1e-5, atol=1e-5)
    assert (run.traj_act[0].cpu() <= dist.act_high_lim).all() and (run.traj_act[0].cpu() >= dist.act_low_lim).all()
    env.close()


# ------------------------------------------------------------------ CertificateAuditor
@pytest.mark.parametrize("name", ["VanderPol", "DuctedFan", "QuadTracking"])
def test_audit_reproduces_the_reference_evaluation(tmp_path, name):
    """tests/golden/eval_*.npz (the reference Evaluator: same policy weights, same initial
    states): mean / std over envs of ret / len and cost / len, at the evaluator test's tolerance."""
    g = np.load(os.path.join(R.G, f"eval_{name}.npz"))
    au = _auditor(tmp_path, name)
    au.networks.policy.load_state_dict({k[7:]: torch.as_tensor(g[k]) for k in g.files if k.startswith("policy/")})
    au.networks.to(au.device)
    res = au.audit(initial_states=g["init"])
    ln = res["len"].double()
    ret, cost = (res["ret"] / ln).cpu().numpy(), (res["cost"] / ln).cpu().numpy()
    np.testing.assert_allclose([ret.mean(), ret.std(), cost.mean(), cost.std()], g["parallel"], rtol=1e-4, atol=1e-3)
    assert (res["status"] != 0).all() and np.isfinite(list(res["summary"].values())).all()
    au.close()


@pytest.mark.parametrize("name", ["VanderPol", "DuctedFan"])
def test_cpu_and_gpu_audits_agree(tmp_path, name):
    """The same audit (65 initial states with early exits, T = 32, the same networks) on the CPU
    build and on the device: len and status identical, q within 1e-5."""
    cpu = _auditor(tmp_path / "c", name, device="cpu")
    gpu = _auditor(tmp_path / "g", name)
    gpu.load_state_dict(cpu.networks.state_dict())
    gpu.networks.to(gpu.device)
    init = R.audit_initial_states(name, 65)
    a = cpu.audit(initial_states=init, horizon=32, keep_trajectory=True)
    b = gpu.audit(initial_states=init, horizon=32, keep_trajectory=True)
    assert torch.equal(a["len"], b["len"].cpu()) and torch.equal(a["status"], b["status"].cpu())
    assert (a["len"] < 32).any() and (a["len"] == 32).any()
    valid = torch.arange(33)[:, None] <= a["len"][None, :]
    qa, qb = a["q"][valid].numpy(), b["q"].cpu()[valid].numpy()
    np.testing.assert_allclose(qb, qa, rtol=1e-5, atol=1e-5)
    cpu.close()
    gpu.close()


# ------------------------------------------------------------------ trainer hook
def _train(tmp_path, sub, **kw):
    torch.manual_seed(0)
    args = default_msacl_args(env_name="DuctedFan", env_num=1024, buffer_warm_size=2000, buffer_max_size=60000,
                              max_iteration=6, eval_interval=10 ** 6, log_save_interval=10 ** 6,
                              apprfunc_save_interval=10 ** 6, save_folder=str(tmp_path / sub), seed=0, num_eval_episode=1,
                              num_audit_states=256, audit_horizon=64, **kw)
    args, alg, sampler, buffer, evaluator, trainer = build_pipeline(args)
    logged = {}
    add = trainer.writer.add_scalar

    def spy(tag, value, step):
        logged.setdefault(tag, []).append((int(step), float(value)))
        return add(tag, value, step)
    trainer.writer.add_scalar = spy
    trainer.train()
    torch.cuda.synchronize()
    sd = {k: v.detach().cpu().clone() for k, v in alg.networks.state_dict().items()}
    auditor = trainer.auditor
    trainer.close()
    return sd, logged, auditor


def test_trainer_certificate_interval(tmp_path):
    """certificate_interval = 3 logs the three Certificate/ tags at iterations 3 and 6; the default
    (key absent) and certificate_interval = 0 are the same code path: no auditor, bit-identical
    networks (deterministic GEMM mode, as the trainer's other bit-identity tests)."""
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        sd_a, log_a, au_a = _train(tmp_path, "a")
        sd_b, log_b, au_b = _train(tmp_path, "b", certificate_interval=0)
        _, log_c, au_c = _train(tmp_path, "c", certificate_interval=3)
    finally:
        torch.use_deterministic_algorithms(prev)
    tags = ["Certificate/bounds_ok", "Certificate/decay_ok", "Certificate/residual"]
    assert au_a is None and au_b is None and au_c is not None
    assert not any(t in log_a or t in log_b for t in tags)
    for k in sd_a:
        assert torch.equal(sd_a[k], sd_b[k]), k
    for t in tags:
        assert [s for s, _ in log_c[t]] == [3, 6], t
        assert np.isfinite([v for _, v in log_c[t]]).all(), t
    for t in tags[:2]:
        assert all(0.0 <= v <= 1.0 for _, v in log_c[t])
