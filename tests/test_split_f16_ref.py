"""CPU: the numpy restatement of the split-f16 hidden layer (tests/split_f16_ref.py) against float64,
and the proof that its bound discriminates.

One row of a 16-row tile is scaled by 2^-{0, 8, 14, 17, 20, 24} at row 0, 7 or 15 (the tile's one
scale then leaves that row's lo halves f16 subnormals), and the weights by 2^-{0, 8, 13, 18} (the
fixed 2^10 then leaves their lo halves subnormal), for ReLU-like (half zeros, unbounded) and
tanh-like (dense, |a| < 1) inputs. Asserted: the emulation keeps every element within the bound; the
same emulation with f16 subnormals flushed to zero breaks it wherever a half is subnormal: in every
case with scaled weights, and in the scaled row (at one of its three positions at least) from 2^-14
on. A row at 2^-8 of its tile keeps normal halves, so there, as for the unscaled tile, flushing
must stay invisible. So a kernel held to this bound (tests/test_gpu_mlp3.py) cannot lose its
subnormal halves unnoticed.

Measured worst err / bound per case (this file, K = 256, N = 64): correct 0.03 - 0.13; flushing
3.4 - 143 where halves are subnormal and 0.03 - 0.21 where none is."""
import numpy as np
import pytest

import split_f16_ref as R

ROW_SHIFTS = (0, 8, 14, 17, 20, 24)
ROW_POS = (0, 7, 15)
W_SHIFTS = (0, 8, 13, 18)
K, NOUT = 256, 64


def _inputs(kind, seed):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((16, K))
    a = np.maximum(z, 0.0) if kind == "relu" else np.tanh(z)
    W = (rng.random((NOUT, K)) * 2 - 1) / K ** 0.5
    return a.astype(np.float32), W.astype(np.float32)


def _ratios(a, W):
    exact = a.astype(np.float64) @ W.astype(np.float64).T
    bound = R.split_f16_bound(a, W)
    ok = np.abs(R.split_f16_matmul(a, W) - exact) / bound
    fl = np.abs(R.split_f16_matmul(a, W, flush_subnormals=True) - exact) / bound
    return ok, fl


@pytest.mark.parametrize("wshift", W_SHIFTS)
@pytest.mark.parametrize("kind", ["relu", "tanh"])
def test_split_emulation_within_bound_and_flushing_outside(kind, wshift):
    worst_ok, flushed = 0.0, []
    for shift in ROW_SHIFTS:
        per_pos = []
        for pos in ROW_POS:
            a, W = _inputs(kind, seed=100 * shift + pos)
            a[pos] *= np.float32(2.0 ** -shift)
            W = W * np.float32(2.0 ** -wshift)
            ok, fl = _ratios(a, W)
            worst_ok = max(worst_ok, float(ok.max()))
            assert ok.max() <= 1.0, (kind, wshift, shift, pos, float(ok.max()))
            if wshift:
                # subnormal weight halves: every row of every tile is hit
                assert fl.max() > 1.0, (kind, wshift, shift, pos, float(fl.max()))
                flushed.append(float(fl.max()))
                continue
            # unscaled weights: only the scaled row can show it, its neighbours never do
            others = np.delete(fl, pos, axis=0)
            assert others.max() <= 1.0, (kind, shift, pos, float(others.max()))
            per_pos.append(float(fl[pos].max()))
        if wshift:
            continue
        if shift < 14:
            # a row at 2^-8 of its tile still has normal lo halves (scaled values >= 2^-3 keep
            # lo >= 2^-14): flushing is invisible, as it is for the homogeneous tile
            assert max(per_pos) <= 1.0, (kind, shift, per_pos)
        else:
            assert max(per_pos) > 1.0, (kind, shift, per_pos)
            flushed.append(max(per_pos))
    print(f"{kind} w 2^-{wshift}: correct worst err/bound {worst_ok:.3f}; "
          f"flushing {min(flushed):.2f} - {max(flushed):.1f}")


def test_tile_scale_matches_the_kernels_exponent_rule():
    """pm_scale_exp: 2^(14 - e) with tmax = m 2^e, m in [0.5, 1); +-40 clamp; 1 for 0 / non-finite."""
    assert R.tile_scale(1.0) == 2.0 ** 13          # 1 = 0.5 2^1
    assert R.tile_scale(0.99) == 2.0 ** 14
    assert R.tile_scale(3.0) == 2.0 ** 12
    assert R.tile_scale(2.0 ** -30) == 2.0 ** 40   # 14 + 29 clamped
    assert R.tile_scale(1e30) == 2.0 ** -40
    assert R.tile_scale(0.0) == 1.0 and R.tile_scale(float("nan")) == 1.0
    for t in (0.37, 1.0, 5.5, 1e-3, 123.0):
        assert 2.0 ** 13 <= t * R.tile_scale(t) <= 2.0 ** 14


def test_ragged_tile_scale_comes_from_tmax():
    """Rows the kernel sees but the caller does not pass (a ragged tile's padding) enter through tmax:
    the product and the bound both follow the larger scale."""
    a, W = _inputs("tanh", seed=5)
    a = a[:6] * np.float32(2.0 ** -10)
    exact = a.astype(np.float64) @ W.astype(np.float64).T
    got = R.split_f16_matmul(a, W, tmax=0.9)
    assert np.all(np.abs(got - exact) <= R.split_f16_bound(a, W, tmax=0.9))
    assert np.all(R.split_f16_bound(a, W, tmax=0.9) > R.split_f16_bound(a, W))
