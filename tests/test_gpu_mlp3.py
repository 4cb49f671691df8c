"""GPU: the fused 3-layer MLP forward (mh_mlp3_forward, csrc/mlp_fused.hip) against a float64
evaluation of each layer (RL/apprfunc/mlp.py:18-30: Linear -> act -> Linear -> act -> Linear -> act).

Each layer is checked on the kernel's own input to it (h1 and h2 as the kernel wrote them), so the
bound does not compound: |err| <= 2e-6 sqrt(K) sum_k |a_k w_k| + 1e-6 (tests/test_gpu_gemm.py's
f32-accumulation bound), plus tanhf's ulp where the activation is tanh. Shapes: the policy
(K1 = D, ReLU, N3 = 2A), the critics (K1 = D + A, N3 = 1), the Lyapunov network (tanh, N3 = 256),
ragged row counts and every supported K1; the grouped (twin-critic) launch; and the MLP module's
forward / backward through the fused launch against the per-layer launches. The split-f16 layers
(layer 2, a wide layer 3) are also held to the tighter bound their scheme implies
(tests/split_f16_ref.py) on rows of mixed magnitude within a tile and across the weight range."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import msacl_amd  # noqa: F401
import msacl_amd._native as N
import split_f16_ref as R
from msacl_amd.apprfunc import _fused as F

pytestmark = pytest.mark.gpu
ACT = {0: lambda v: v, 1: lambda v: np.maximum(v, 0.0), 2: np.tanh}


def _params(K1, N3, seed, H=256, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    f = lambda *s: (torch.rand(*s, generator=g) * 2 - 1)  # noqa: E731
    W1, b1 = f(H, K1) / K1 ** 0.5 * scale, f(H) * 0.1
    W2, b2 = f(H, H) / H ** 0.5 * scale, f(H) * 0.1
    W3, b3 = f(N3, H) / H ** 0.5 * scale, f(N3) * 0.1
    return [t.cuda().contiguous() for t in (W1, b1, W2, b2, W3, b3)]


def _check_layer(out, inp, W, b, act, what):
    a, w = inp.double().cpu().numpy(), W.double().cpu().numpy()
    lin = a @ w.T + b.double().cpu().numpy()
    mag = np.abs(a) @ np.abs(w).T + np.abs(b.double().cpu().numpy())
    ref = ACT[act](lin)
    tol = 2e-6 * (a.shape[1] ** 0.5) * mag + 1e-6 + (2e-7 * np.abs(ref) if act == 2 else 0.0)
    err = np.abs(out.double().cpu().numpy() - ref)
    assert np.all(err <= tol), f"{what}: max err {err.max():.3e}, worst ratio {(err / tol).max():.3f}"


def _run(x, ps, acts, keep=True, N3=None):
    W1, b1, W2, b2, W3, b3 = ps
    M, K1 = x.shape
    N3 = W3.shape[0]
    h1 = torch.full((M, 256), float("nan"), device="cuda") if keep else None
    h2 = torch.full((M, 256), float("nan"), device="cuda") if keep else None
    y = torch.full((M, N3), float("nan"), device="cuda")
    N.check(N.lib().mh_mlp3_forward(N.ptr(x), M, K1, K1, *[N.ptr(t) for t in ps], 256, N3, *acts, N.ptr(h1), N.ptr(h2),
                                    256, N.ptr(y), N3, 1, None, N.stream_of()), "mh_mlp3_forward")
    torch.cuda.synchronize()
    return y, h1, h2


CASES = [("policy", 5120, 12, 8, (1, 1, 0)), ("critic", 5120, 16, 1, (1, 1, 0)), ("lyapunov", 10240, 12, 256, (2, 2, 0)),
         ("ragged", 1000, 12, 8, (1, 1, 0)), ("tiny", 17, 6, 2, (1, 1, 0)), ("k1", 300, 1, 4, (1, 2, 0)),
         ("k20", 777, 20, 16, (2, 1, 0)), ("k32", 2048, 32, 64, (1, 1, 2)), ("n128", 512, 14, 128, (2, 2, 1))]


@pytest.mark.parametrize("name,M,K1,N3,acts", CASES, ids=[c[0] for c in CASES])
def test_mlp3_forward_matches_float64_layers(name, M, K1, N3, acts):
    ps = _params(K1, N3, seed=M + K1)
    x = (torch.rand(M, K1, generator=torch.Generator().manual_seed(1)) * 4 - 2).cuda()
    y, h1, h2 = _run(x, ps, acts)
    W1, b1, W2, b2, W3, b3 = ps
    _check_layer(h1, x, W1, b1, acts[0], "layer 1")
    _check_layer(h2, h1, W2, b2, acts[1], "layer 2")
    _check_layer(y, h2, W3, b3, acts[2], "layer 3")
    # without the kept activations: the same output, bit for bit
    y2, _, _ = _run(x, ps, acts, keep=False)
    assert torch.equal(y, y2)


def test_mlp3_forward_grouped_equals_ungrouped():
    """Two networks of one shape in one launch (the twin critics' joint buffers: W1 [2H][K],
    W2 [2][H][H], W3 [2][H], h [M][2H]); each group equals its ungrouped launch bit for bit."""
    M, K, H = 5120, 16, 256
    a, b = _params(K, 1, seed=3), _params(K, 1, seed=4)
    W1 = torch.cat([a[0], b[0]]).contiguous()
    b1 = torch.cat([a[1], b[1]]).contiguous()
    W2 = torch.stack([a[2], b[2]]).contiguous()
    b2 = torch.stack([a[3], b[3]]).contiguous()
    W3 = torch.cat([a[4], b[4]]).contiguous()
    b3 = torch.cat([a[5], b[5]]).contiguous()
    x = torch.randn(M, K, device="cuda")
    h1 = torch.empty(M, 2 * H, device="cuda")
    h2 = torch.empty(M, 2 * H, device="cuda")
    q = torch.empty(2, M, device="cuda")
    gs = (ctypes.c_int64 * 9)(0, H * K, H, H * H, H, H, 1, H, M)
    N.check(N.lib().mh_mlp3_forward(N.ptr(x), M, K, K, N.ptr(W1), N.ptr(b1), N.ptr(W2), N.ptr(b2), N.ptr(W3), N.ptr(b3),
                                    H, 1, 1, 1, 0, N.ptr(h1), N.ptr(h2), 2 * H, N.ptr(q), 1, 2, gs, N.stream_of()),
            "grouped")
    for g, ps in enumerate((a, b)):
        y, k1, k2 = _run(x, ps, (1, 1, 0))
        assert torch.equal(q[g], y[:, 0]), g
        assert torch.equal(h1[:, g * H:(g + 1) * H], k1), g
        assert torch.equal(h2[:, g * H:(g + 1) * H], k2), g


def test_mlp3_rejects_unsupported_shapes():
    ps = _params(12, 8, seed=0)
    x = torch.zeros(64, 40, device="cuda")
    y = torch.empty(64, 8, device="cuda")
    assert N.lib().mh_mlp3_forward(N.ptr(x), 64, 40, 40, *[N.ptr(t) for t in ps], 256, 8, 1, 1, 0, None, None, 256,
                                   N.ptr(y), 8, 1, None, N.stream_of()) == -1  # K1 > 32
    assert N.lib().mh_mlp3_forward(N.ptr(x), 64, 12, 40, *[N.ptr(t) for t in ps], 256, 20, 1, 1, 0, None, None, 256,
                                   N.ptr(y), 20, 1, None, N.stream_of()) == -1  # N3 = 20


def _kink_margin_rows(x, mods, margin=1e-5):
    """Rows whose ReLU pre-activations (float64) all keep `margin` x the layer's max |z| from 0.
    Two correct f32 evaluations of a layer (different summation orders, or the split-f16 layer
    against the f32 one) differ by ~1e-7 of its scale; a unit that close to the kink can take
    either side of it, and its mask then differs between the two paths, moving every gradient of
    its row by a whole term: a comparison of two paths' gradients is only meaningful where both
    agree on every mask."""
    D = lambda t: t.detach().double().cpu()  # noqa: E731
    a, keep = D(x), torch.ones(x.shape[0], dtype=torch.bool)
    for lin in (mods[0], mods[2]):
        z = a @ D(lin.weight).T + D(lin.bias)
        keep &= (z.abs() > margin * float(z.abs().max())).all(1)
        a = z.clamp_min(0.0)
    return keep.to(x.device), int((~keep).sum())


@pytest.mark.parametrize("acts", [(nn.ReLU, nn.ReLU, nn.Identity), (nn.Tanh, nn.Tanh, nn.Identity)])
def test_mlp_module_fused_forward_backward_matches_per_layer(acts):
    """The MLP module (apprfunc/_fused.py) through MLP3 vs through the per-layer LinearAct launches:
    outputs within the f32 summation-order bound, every gradient rtol 1e-4 / atol 1e-5 of its scale
    (ReLU: on rows clear of the kink, _kink_margin_rows; the rows dropped are counted and limited to
    4 %: 2 x 256 units each within 1e-5 of a Gaussian-ish pre-activation's scale exclude 2.2 - 2.8 %
    of randn rows, binomial spread 0.2 %)."""
    torch.manual_seed(0)
    mods = [nn.Linear(12, 256), acts[0](), nn.Linear(256, 256), acts[1](), nn.Linear(256, 8), acts[2]()]
    net = F.MLP(*mods).cuda()
    x = torch.randn(256 * 21, 12, device="cuda")
    if acts[0] is nn.ReLU:
        keep, dropped = _kink_margin_rows(x, mods)
        print(f"kink margin: {dropped} of {x.shape[0]} rows excluded ({100.0 * dropped / x.shape[0]:.2f} %)")
        assert dropped <= 0.04 * x.shape[0], dropped
        x = x[keep]
    x = x[:256 * 20].reshape(256, 20, 12).requires_grad_(True)
    g = torch.randn(256, 20, 8, device="cuda")
    outs = []
    for on in (True, False):
        F._MLP3["on"] = on
        try:
            net.zero_grad()
            xx = x.detach().clone().requires_grad_(True)
            y = net(xx)
            y.backward(g)
            outs.append((y.detach(), xx.grad.clone(), [p.grad.clone() for p in net.parameters()]))
        finally:
            F._MLP3["on"] = True
    (ya, gxa, gpa), (yb, gxb, gpb) = outs
    torch.testing.assert_close(ya, yb, rtol=1e-5, atol=1e-5 * float(yb.abs().max()))
    for u, v in [(gxa, gxb)] + list(zip(gpa, gpb)):
        torch.testing.assert_close(u, v, rtol=1e-4, atol=1e-5 * float(v.abs().max()))


@pytest.mark.parametrize("K1,N3,acts", [(12, 8, (1, 1)), (16, 1, (1, 1)), (12, 256, (2, 2)), (20, 16, (2, 1)),
                                        (5, 64, (1, 2))])
def test_mlp3_backward_chain_matches_float64(K1, N3, acts):
    """mh_mlp3_backward: g2 = (dy W3) act2'(h2), g1 = (g2 W2) act1'(h1), dx = g1 W1, each checked on
    the kernel's own previous gradient against float64 (the forward's bound)."""
    M = 3000
    ps = _params(K1, N3, seed=K1 * N3)
    W1, b1, W2, b2, W3, b3 = ps
    x = torch.randn(M, K1, device="cuda")
    y, h1, h2 = _run(x, ps, acts + (0,))
    dy = torch.randn(M, N3, device="cuda")
    g2 = torch.empty(M, 256, device="cuda")
    g1 = torch.empty(M, 256, device="cuda")
    dx = torch.empty(M, K1, device="cuda")
    N.check(N.lib().mh_mlp3_backward(N.ptr(dy), N3, N.ptr(h1), N.ptr(h2), 256, N.ptr(W1), N.ptr(W2), N.ptr(W3), M,
                                     K1, 256, N3, acts[0], acts[1], N.ptr(g2), N.ptr(g1), 256, N.ptr(dx), K1, 1, None,
                                     N.stream_of()), "mh_mlp3_backward")
    torch.cuda.synchronize()
    D = lambda t: t.double().cpu().numpy()  # noqa: E731
    dact = {1: lambda h: (h > 0).astype(np.float64), 2: lambda h: 1.0 - h * h}

    def check(out, g, W, h, act, what):
        lin = D(g) @ D(W)
        mag = np.abs(D(g)) @ np.abs(D(W))
        ref = lin * (dact[act](D(h)) if act else 1.0)
        tol = (2e-6 * (g.shape[1] ** 0.5) * mag + 1e-6) * (np.abs(dact[act](D(h))) if act else 1.0) + 1e-7
        err = np.abs(D(out) - ref)
        assert np.all(err <= tol), f"{what}: max err {err.max():.3e}, worst ratio {(err / tol).max():.3f}"

    check(g2, dy, W3, h2, acts[1], "g2")
    check(g1, g2, W2, h1, acts[0], "g1")
    check(dx, g1, W1, None, 0, "dx")


def test_twin_input_grad_chain_equals_per_layer():
    """TwinCritic.input_grad through mh_mlp3_backward (both critics, the input gradients summed in
    one launch) vs the per-layer launches: equal to the f32 summation-order bound."""
    from msacl_amd.apprfunc._twin import TwinCritic
    from msacl_amd.apprfunc.mlp import ActionValue
    torch.manual_seed(1)
    kw = dict(obs_dim=12, act_dim=4, hidden_sizes=[256, 256], hidden_activation="relu", output_activation="linear")
    q1, q2 = ActionValue(**kw).cuda(), ActionValue(**kw).cuda()
    tc = TwinCritic.build(q1, q2)
    M = 5120
    x = torch.randn(M, 16, device="cuda")
    q, h1, h2 = tc.forward(x)
    dq = torch.randn(2, M, device="cuda")
    outs = []
    for on in (True, False):
        F._MLP3["on"] = on
        try:
            outs.append(tc.input_grad(dq, h1, h2))
        finally:
            F._MLP3["on"] = True
    torch.testing.assert_close(outs[0], outs[1], rtol=1e-4, atol=1e-5 * float(outs[1].abs().max()))


@pytest.mark.parametrize("M", [5120, 3001])
def test_twin_forward_pair_equals_two_forwards(M):
    """TwinCritic.forward_pair (mh_mlp3_forward_pair: the critics and the target critics as the two
    network sets of one launch) equals the two separate forwards bit for bit."""
    from msacl_amd.apprfunc._twin import TwinCritic
    from msacl_amd.apprfunc.mlp import ActionValue
    torch.manual_seed(2)
    kw = dict(obs_dim=12, act_dim=4, hidden_sizes=[256, 256], hidden_activation="relu", output_activation="linear")
    nets = [ActionValue(**kw).cuda() for _ in range(4)]
    tc, tt = TwinCritic.build(nets[0], nets[1]), TwinCritic.build(nets[2], nets[3])
    x, xo = torch.randn(M, 16, device="cuda"), torch.randn(M, 16, device="cuda")
    q, h1, h2, qo = tc.forward_pair(x, tt, xo)
    q_ref, h1_ref, h2_ref = tc.forward(x)
    qo_ref, _, _ = tt.forward(xo, keep=False)
    for a, b in ((q, q_ref), (h1, h1_ref), (h2, h2_ref), (qo, qo_ref)):
        torch.testing.assert_close(a, b, rtol=0, atol=0)


@pytest.mark.parametrize("rows", [5120, 3001])
def test_weight_grads_multi_matches_float64(rows):
    """mh_weight_grads: the three layers' dW = g^T x and db = column sums of g of a policy-shaped MLP
    (a narrow output layer computed transposed, a 256 x 256 layer, a K1 = 12 input layer) in two
    launches, each element against float64 within 2e-6 sqrt(rows) sum|g x| + 1e-6."""
    from msacl_amd.apprfunc._fused import weight_grads
    torch.manual_seed(rows)
    dev = "cuda"
    g3, h2 = torch.randn(rows, 8, device=dev), torch.rand(rows, 256, device=dev)
    g2, h1 = torch.randn(rows, 256, device=dev), torch.rand(rows, 256, device=dev)
    g1, x = torch.randn(rows, 256, device=dev), torch.randn(rows, 12, device=dev)
    outs = [(torch.empty(8, 256, device=dev), torch.empty(8, device=dev)),
            (torch.empty(256, 256, device=dev), torch.empty(256, device=dev)),
            (torch.empty(256, 12, device=dev), None)]
    weight_grads([(g3, 8, h2, 256, 8, 256) + outs[0], (g2, 256, h1, 256, 256, 256) + outs[1],
                  (g1, 256, x, 12, 256, 12) + outs[2]], rows, torch.device(dev))
    torch.cuda.synchronize()
    D = lambda t: t.double().cpu().numpy()  # noqa: E731
    for (g, xin), (dw, db) in zip(((g3, h2), (g2, h1), (g1, x)), outs):
        ref = D(g).T @ D(xin)
        tol = 2e-6 * rows ** 0.5 * (np.abs(D(g)).T @ np.abs(D(xin))) + 1e-6
        assert np.all(np.abs(D(dw) - ref) <= tol), np.abs(D(dw) - ref).max()
        if db is not None:
            rb = D(g).sum(0)
            assert np.all(np.abs(D(db) - rb) <= 2e-6 * rows ** 0.5 * np.abs(D(g)).sum(0) + 1e-6)


def test_twin_weight_grads_fused_equals_per_layer():
    """TwinCritic.backward_weights through the chain + mh_weight_grads vs the per-layer launches:
    every gradient within rtol 1e-4 / atol 1e-5 of its scale. Both backward paths take the same
    kept activations (one forward): the forward's own paths are compared above, and the ReLU
    masks of two forwards can differ at units within rounding of the kink (_kink_margin_rows)."""
    from msacl_amd.apprfunc._twin import TwinCritic
    from msacl_amd.apprfunc.mlp import ActionValue
    torch.manual_seed(2)
    kw = dict(obs_dim=12, act_dim=4, hidden_sizes=[256, 256], hidden_activation="relu", output_activation="linear")
    q1, q2 = ActionValue(**kw).cuda(), ActionValue(**kw).cuda()
    tc = TwinCritic.build(q1, q2)
    M = 5120
    x = torch.randn(M, 16, device="cuda")
    dq = torch.randn(2, M, device="cuda")
    res = []
    q, h1, h2 = tc.forward(x)
    for on in (True, False):
        F._MLP3["on"] = on
        try:
            tc.backward_weights(x, dq, h1, h2)
            res.append([t.clone() for t in (tc.gW1, tc.gb1, tc.gW2, tc.gb2, tc.gW3, tc.gb3)])
        finally:
            F._MLP3["on"] = True
    for u, v in zip(*res):
        torch.testing.assert_close(u, v, rtol=1e-4, atol=1e-5 * float(v.abs().max()))


@pytest.mark.parametrize("mode", [-1, 1, 3, 4])
def test_forward_row_tile_modes_equal_default(mode):
    """mh_mlp3_set_row_tiles changes only the grid (rows per workgroup), never the bits: the twin
    critics' forward (2 x 5,120 rows and a ragged 1,037) under each mode equals the default."""
    from msacl_amd.apprfunc._twin import TwinCritic
    from msacl_amd.apprfunc.mlp import ActionValue
    N = F._native()
    torch.manual_seed(11)
    kw = dict(obs_dim=12, act_dim=4, hidden_sizes=[256, 256], hidden_activation="relu", output_activation="linear")
    tc = TwinCritic.build(ActionValue(**kw).cuda(), ActionValue(**kw).cuda())
    for M in (5120, 1037):
        x = torch.randn(M, 16, device="cuda")
        ref = [t.clone() for t in tc.forward(x)]
        N.check(N.lib().mh_mlp3_set_row_tiles(mode), "mh_mlp3_set_row_tiles")
        try:
            got = [t.clone() for t in tc.forward(x)]
        finally:
            N.lib().mh_mlp3_set_row_tiles(0)
        for a, b in zip(got, ref):
            torch.testing.assert_close(a, b, rtol=0, atol=0)
    assert N.lib().mh_mlp3_set_row_tiles(5) != 0


@pytest.mark.parametrize("M", [5120, 1037, 16400])
def test_twin_head_grads_folded_into_chain(M):
    """The q heads' dW3 / db3 formed inside the chain launch (mh_mlp3_backward_w3) equal the
    grouped head backward's bit for bit below 16,384 rows (same 16-row partials, same finish;
    1,037: a ragged last block), agree with float64 at any size, and leave g1 / g2 unchanged."""
    from msacl_amd.apprfunc import _twin as T
    from msacl_amd.apprfunc.mlp import ActionValue
    torch.manual_seed(M)
    kw = dict(obs_dim=12, act_dim=4, hidden_sizes=[256, 256], hidden_activation="relu", output_activation="linear")
    tc = T.TwinCritic.build(ActionValue(**kw).cuda(), ActionValue(**kw).cuda())
    x = torch.randn(M, 16, device="cuda")
    dq = torch.randn(2, M, device="cuda")
    q, h1, h2 = tc.forward(x)
    res = []
    saved = T._FOLD_W3
    for fold in (True, False):
        T._FOLD_W3 = fold
        try:
            tc.backward_weights(x, dq, h1, h2)
            torch.cuda.synchronize()
            res.append([t.clone() for t in (tc.gW1, tc.gb1, tc.gW2, tc.gb2, tc.gW3, tc.gb3)])
        finally:
            T._FOLD_W3 = saved
    exact = M < 16384
    for u, v in zip(*res):
        if exact:
            torch.testing.assert_close(u, v, rtol=0, atol=0)
        else:
            torch.testing.assert_close(u, v, rtol=1e-5, atol=1e-6 * float(v.abs().max()))
    D = lambda t: t.double().cpu().numpy()  # noqa: E731
    gW3, gb3 = res[0][4], res[0][5]
    for qn in range(2):
        hq = D(h2[:, qn * 256:(qn + 1) * 256])
        ref = D(dq[qn]) @ hq
        tol = 2e-6 * M ** 0.5 * (np.abs(D(dq[qn])) @ np.abs(hq)) + 1e-6
        assert np.all(np.abs(D(gW3[qn]).reshape(-1) - ref) <= tol)
        assert abs(float(gb3[qn]) - D(dq[qn]).sum()) <= 2e-6 * M ** 0.5 * np.abs(D(dq[qn])).sum() + 1e-6


@pytest.mark.parametrize("M", [10240, 5376, 999])
def test_lyapunov_square_sum_fused_equals_separate(M):
    """LyapunovValue through MLP3SquareSum (mh_mlp3_forward_sqsum / mh_mlp3_backward_sqsum: the
    square sums and dy = dV 2y inside the MLP's launches) vs the MLP's launches + SquareSum: V and
    every gradient bit for bit."""
    from msacl_amd.apprfunc.mlp import LyapunovValue
    torch.manual_seed(5)
    lya = LyapunovValue(input_dim=12, hidden_sizes=[256, 256], hidden_activation="tanh", output_dim=256,
                        output_activation="linear").cuda()
    x = torch.randn(M, 12, device="cuda")
    dv = torch.randn(M, device="cuda")
    outs = []
    for fused in (True, False):
        F._MLP3["sqsum"] = fused  # off: the same fused MLP launches, then SquareSum's two launches
        try:
            lya.zero_grad()
            v = lya(x)
            v.backward(dv)
            outs.append([v.detach().clone()] + [p.grad.detach().clone() for p in lya.parameters()])
        finally:
            F._MLP3["sqsum"] = True
    for a, b in zip(*outs):
        torch.testing.assert_close(a, b, rtol=0, atol=0)


def _layer64(inp, W, b, act):
    with np.errstate(invalid="ignore", over="ignore"):
        return ACT[act](inp.double().cpu().numpy() @ W.double().cpu().numpy().T + b.double().cpu().numpy())


def test_mlp3_forward_weights_past_the_split_range_and_nonfinite_rows():
    """The split-f16 hidden layers (csrc/mlp_fused.hip layer_cols_run_x3) scale weights by 2^10
    before the f16 split: a weight of 64 or more overflows its f16 hi. Such a row tile is recomputed
    by the f32 layer (x3_redo_nonfinite), so the results stay within the f32 bound. A non-finite
    input row (a NaN, +Inf, -Inf) or one that overflows the tile's scaled f16 range (3e38) gives, in
    each layer on the kernel's own input, a non-finite value wherever the float64 layer has one; the
    15 other rows of its tile stay within the f32 bound of float64, and the other row tiles keep
    their bits."""
    for K1, N3, acts in ((12, 256, (2, 2, 0)), (16, 1, (1, 1, 0))):
        ps = _params(K1, N3, seed=7)
        W1, b1, W2, b2, W3, b3 = ps
        W2[3, 5] = 100.0
        W2[200, 17] = -70.0
        if N3 > 16:
            W3[9, 250] = 65.0
        M = 1000
        x = (torch.rand(M, K1, generator=torch.Generator().manual_seed(3)) * 4 - 2).cuda()
        y, h1, h2 = _run(x, ps, acts)
        _check_layer(h2, h1, W2, b2, acts[1], "layer 2")
        _check_layer(y, h2, W3, b3, acts[2], "layer 3")
        rows = torch.arange(M, device="cuda")
        tile = rows // 16 == 40 // 16
        mates = tile & (rows != 40)
        for bad in (float("nan"), float("inf"), float("-inf"), 3e38):
            xb = x.clone()
            xb[40, 0] = bad
            yb, h1b, h2b = _run(xb, ps, acts)
            if bad != bad:
                assert torch.all(torch.isnan(yb[40]))
            for got, ref in ((yb, y), (h1b, h1), (h2b, h2)):
                assert torch.equal(got[~tile], ref[~tile]), bad
            for out, inp, W, b, act, what in ((h1b, xb, W1, b1, acts[0], "layer 1"), (h2b, h1b, W2, b2, acts[1], "layer 2"),
                                              (yb, h2b, W3, b3, acts[2], "layer 3")):
                ref_bad = _layer64(inp[40:41], W, b, act)[0]
                got_bad = out[40].double().cpu().numpy()
                loud = ~np.isfinite(ref_bad)
                assert not np.isfinite(got_bad[loud]).any(), (bad, what, int(np.isfinite(got_bad[loud]).sum()))
                assert torch.all(torch.isfinite(out[mates])), (bad, what)
                _check_layer(out[mates], inp[mates], W, b, act, f"{what}, tile mates of a {bad} row")


@pytest.mark.parametrize("name,M,K1,N3,acts", CASES[:3], ids=[c[0] for c in CASES[:3]])
def test_mlp3_hidden_layer_error_near_f32_rounding(name, M, K1, N3, acts):
    """The hidden layer's error against float64 on the kernel's own input, in units of the f32
    dot-product scale 2^-24 sqrt(K) sum_k |a_k w_k|: the split-f16 form drops the lo.lo products
    (<= 2^-22 of each product) and keeps weights to 22 bits."""
    ps = _params(K1, N3, seed=M + K1)
    x = (torch.rand(M, K1, generator=torch.Generator().manual_seed(1)) * 4 - 2).cuda()
    y, h1, h2 = _run(x, ps, acts)
    W2, b2 = ps[2], ps[3]
    a, w = h1.double().cpu().numpy(), W2.double().cpu().numpy()
    lin = a @ w.T + b2.double().cpu().numpy()
    mag = np.abs(a) @ np.abs(w).T + np.abs(b2.double().cpu().numpy())
    ref = ACT[acts[1]](lin)
    ratio = np.abs(h2.double().cpu().numpy() - ref) / (2.0 ** -24 * 16 * mag + 1e-30)
    print(f"{name}: layer-2 error / (2^-24 sqrt(K) mag): max {ratio.max():.3f} mean {ratio.mean():.4f}")
    assert ratio.max() < 4.0


# ---- the split-f16 layers against float64 with the bound of tests/split_f16_ref.py

def _pad_rows(ps, acts):
    """What the rows past M of a ragged tile hold (x = 0): h1 = act1(b1), h2 = act2(W2 h1 + b2)."""
    W1, b1, W2, b2, W3, b3 = [t.double().cpu().numpy() for t in ps]
    p1 = ACT[acts[0]](b1)
    p2 = ACT[acts[1]](W2 @ p1 + b2)
    return p1, p2


def _split_layer_ratios(out, inp, W, b, act, pad):
    """Per element, the split layer's |out - float64| over its tolerance on the kernel's own input:
    split_f16_bound per 16-row tile (tmax over the tile's rows and, in a ragged tile, the padded
    rows' input `pad`), plus what lies outside the product sum: one f32 rounding of (sum + bias),
    2^-24 (|z| + bound), and tanhf's 2e-7 |ref| where the activation is tanh (_check_layer's term).
    Also returns the bound itself (for the mask-flip count) and float64's pre-activation."""
    a, w, bb = inp.double().cpu().numpy(), W.double().cpu().numpy(), b.double().cpu().numpy()
    M = a.shape[0]
    z = a @ w.T + bb
    ref = ACT[act](z)
    bound = np.empty_like(z)
    for r0 in range(0, M, 16):
        t = a[r0:r0 + 16]
        tmax = float(np.abs(t).max())
        if t.shape[0] < 16:
            tmax = max(tmax, float(np.abs(pad).max()))
        bound[r0:r0 + 16] = R.split_f16_bound(t, w, tmax=tmax)
    tol = bound + 2.0 ** -24 * (np.abs(z) + bound) + (2e-7 * np.abs(ref) if act == 2 else 0.0)
    return np.abs(out.double().cpu().numpy() - ref) / tol, tol, z


def _check_split_layer(out, inp, W, b, act, pad, what):
    ratio, _, _ = _split_layer_ratios(out, inp, W, b, act, pad)
    i = np.unravel_index(np.argmax(ratio), ratio.shape)
    print(f"{what}: worst err / bound {ratio.max():.3f} at row {i[0]} col {i[1]}")
    assert ratio.max() <= 1.0, f"{what}: worst err / bound {ratio.max():.3f} at {i}"
    return float(ratio.max())


def _homogeneous_ratio(out, inp, W, b, act):
    """test_mlp3_hidden_layer_error_near_f32_rounding's figure: |err| / (2^-24 sqrt(256) mag)."""
    a, w, bb = inp.double().cpu().numpy(), W.double().cpu().numpy(), b.double().cpu().numpy()
    ref = ACT[act](a @ w.T + bb)
    mag = np.abs(a) @ np.abs(w).T + np.abs(bb)
    return float((np.abs(out.double().cpu().numpy() - ref) / (2.0 ** -24 * 16 * mag + 1e-30)).max())


def _check_all_layers(x, ps, acts, outs, what):
    """Layer 1 and a narrow layer 3 (f32 MFMA) to _check_layer's bound, the split layers (layer 2,
    layer 3 when N3 > 16) to the split bound; each on the kernel's own input."""
    W1, b1, W2, b2, W3, b3 = ps
    y, h1, h2 = outs
    p1, p2 = _pad_rows(ps, acts)
    _check_layer(h1, x, W1, b1, acts[0], f"{what} layer 1")
    worst = [_check_split_layer(h2, h1, W2, b2, acts[1], p1, f"{what} layer 2")]
    if W3.shape[0] > 16:
        worst.append(_check_split_layer(y, h2, W3, b3, acts[2], p2, f"{what} layer 3"))
    else:
        _check_layer(y, h2, W3, b3, acts[2], f"{what} layer 3")
    return worst


MIXED_NETS = [("lyapunov", 12, 256, (2, 2, 0)), ("policy", 12, 8, (1, 1, 0)), ("critic", 16, 1, (1, 1, 0))]


@pytest.mark.parametrize("M", [80, 70])
@pytest.mark.parametrize("name,K1,N3,acts", MIXED_NETS, ids=[c[0] for c in MIXED_NETS])
def test_mlp3_split_layers_rows_of_mixed_magnitude(name, K1, N3, acts, M):
    """One scale per 16-row tile: rows far below their tile's maximum keep their lo halves (and,
    from 2^-17 on, their hi halves) only as f16 subnormals. b1 = 0, so a row of h1 scales with its
    row of x: tile 1 row 0 x 2^-14, tile 2 row 7 x 2^-20, tile 3 row 15 x 2^-8 and row 3 x 2^-17,
    tile 4 (ragged at M = 70) every row x 2^-12, which is its own scale and must meet the
    homogeneous ratio < 4 bar. Every element of the split layers within the split bound; the f32
    layers within theirs; every row-tile mode the default's bits.
    Measured worst err / tolerance (MI355X): tanh 0.12 - 0.41; ReLU layer 2 0.84 - 0.95, at elements
    whose bias dominates the sum, where the f32 rounding of (sum + bias) is nearly the whole
    tolerance; tile 4 at 0.056 - 0.111 of the ratio bar."""
    ps = _params(K1, N3, seed=M + K1 + N3)
    ps[1].zero_()
    x = torch.rand(M, K1, generator=torch.Generator().manual_seed(2)) * 4 - 2
    x[16 + 0] *= 2.0 ** -14
    x[32 + 7] *= 2.0 ** -20
    x[48 + 15] *= 2.0 ** -8
    x[48 + 3] *= 2.0 ** -17
    x[64:] *= 2.0 ** -12
    x = x.cuda()
    outs = _run(x, ps, acts)
    y, h1, h2 = outs
    _check_all_layers(x, ps, acts, outs, name)
    r2 = _homogeneous_ratio(h2[64:], h1[64:], ps[2], ps[3], acts[1])
    print(f"{name} M={M}: tile 4 layer-2 error / (2^-24 sqrt(K) mag) {r2:.3f}")
    assert r2 < 4.0
    for mode in (-1, 1, 3, 4):
        N.check(N.lib().mh_mlp3_set_row_tiles(mode), "mh_mlp3_set_row_tiles")
        try:
            got = _run(x, ps, acts)
        finally:
            N.lib().mh_mlp3_set_row_tiles(0)
        for u, v in zip(got, outs):
            assert torch.equal(u, v), mode


@pytest.mark.parametrize("plant", ["in_range", "redo"])
@pytest.mark.parametrize("shift", [8, 13, 18])
def test_mlp3_split_layers_weight_range(shift, plant):
    """The fixed weight scale 2^10: W2 and W3 scaled by 2^-8, 2^-13, 2^-18 (lo halves, then hi
    halves, subnormal), with single entries planted at 63.96875 (the largest weight whose scaled
    hi is finite), 2^-24, 2^-30, 0.0 and -0.0; `redo`: also 63.99, whose hi rounds to Inf, so those
    columns come back through x3_redo_nonfinite. Every element within the split bound.
    Measured worst err / tolerance (MI355X): layer 2 0.21 - 0.33, layer 3 0.59 - 0.80 (bias-dominated
    elements); the redo columns 0.59 at 2^-8, where rerunning the f32 MFMA layer gave 1.28: the redo
    now sums exact products in double."""
    K1, N3, acts, M = 12, 256, (2, 2, 0), 40
    ps = _params(K1, N3, seed=shift)
    for W in (ps[2], ps[4]):
        W.mul_(2.0 ** -shift)
        W[3, 5] = 63.96875
        W[70, 130] = -63.96875
        W[140, 7] = 2.0 ** -24
        W[200, 255] = -2.0 ** -30
        W[250, 0] = 0.0
        W[255, 31] = -0.0
        if plant == "redo":
            W[100, 64] = 63.99
    x = (torch.rand(M, K1, generator=torch.Generator().manual_seed(4)) * 4 - 2).cuda()
    outs = _run(x, ps, acts)
    assert all(torch.isfinite(t).all() for t in outs)
    _check_all_layers(x, ps, acts, outs, f"W 2^-{shift} {plant}")


def test_mlp3_relu_masks_flip_only_inside_the_bound():
    """The ReLU critic at 5,120 rows: a hidden unit whose mask (h > 0) differs from the float64
    layer's (on the kernel's own input) must have |z64| within that element's bound (layer 1:
    _check_layer's, layer 2: the split bound): the kernel may take the other side of the kink
    only where rounding can put it there. The count is printed (MI355X: 0 of 1,310,720 units in
    layer 1, 1 in layer 2)."""
    M, K1, N3, acts = 5120, 16, 1, (1, 1, 0)
    ps = _params(K1, N3, seed=M + K1)
    W1, b1, W2, b2, W3, b3 = ps
    x = (torch.rand(M, K1, generator=torch.Generator().manual_seed(1)) * 4 - 2).cuda()
    y, h1, h2 = _run(x, ps, acts)
    D = lambda t: t.double().cpu().numpy()  # noqa: E731
    z1 = D(x) @ D(W1).T + D(b1)
    tol1 = 2e-6 * K1 ** 0.5 * (np.abs(D(x)) @ np.abs(D(W1)).T + np.abs(D(b1))) + 1e-6
    flip1 = (D(h1) > 0) != (z1 > 0)
    _, tol2, z2 = _split_layer_ratios(h2, h1, W2, b2, 1, _pad_rows(ps, acts)[0])
    flip2 = (D(h2) > 0) != (z2 > 0)
    print(f"mask flips of {M * 256} units: layer 1 {int(flip1.sum())}, layer 2 {int(flip2.sum())}")
    assert np.all(np.abs(z1[flip1]) <= tol1[flip1])
    assert np.all(np.abs(z2[flip2]) <= tol2[flip2])
