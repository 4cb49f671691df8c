"""A numpy restatement of the split-f16 hidden layer (csrc/mlp_fused.hip layer_cols_run_x3) and the
error bound that follows from the scheme. Not a test module: tests/test_split_f16_ref.py checks it
on the CPU, tests/test_gpu_mlp3.py holds the kernel to the same bound.

The scheme, per 16-row tile `a` [rows][K] and weights `W` [N][K]:
  * a is scaled by 2^(14 - e), e the frexp exponent of the tile's max |a| (so every scaled value is
    <= 2^14), the exponent clamped to +-40 (pm_scale_exp); W by the fixed 2^10;
  * each scaled value v splits into hi = f16(v), lo = f16(v - hi) (v - hi is exact in f32);
  * out = sum_k (lo.hi + hi.lo + hi.hi) / (2^(14 - e) 2^10); the lo.lo product is dropped.

The bound. hi carries 11 bits and lo 11 more, so while lo is a normal f16 the split residual
v - hi - lo is <= 2^-22 |v|; once lo falls below 2^-14 (scaled units) it is a subnormal on the fixed
grid 2^-24 and the residual is at most half a step, 2^-25. Per product (a s_a)(w s_w):
  |a w - (kept terms)| <= |res_a| |w| + |a| |res_w| + |lo_a lo_w|
with |res_a| <= max(2^-22 |a|, 2^-25 / s_a), s_a >= 2^13 / tmax, so 2^-25 / s_a <= 2^-38 tmax, and
|res_w| <= max(2^-22 |w|, 2^-35), |lo_a lo_w| <= 2^-22 |a w|. Summed over k, with one more 2^-22 for
the f32 accumulation and a factor 2 on the subnormal terms:
  |err| <= 4 2^-22 sum_k |a_k w_k| + sum_k (2^-37 tmax |w_k| + 2^-34 |a_k|) + 1e-30.
An arithmetic that flushes f16 subnormals (in the split or in the matrix unit) loses every lo below
2^-14: a residual of up to 2^-14 / s_a ~ 2^-27 tmax per element, far outside the bound for a row
small against its tile, and invisible for a homogeneous tile."""
import numpy as np

WX = 1024.0          # the fixed weight scale 2^10
F16_MIN_NORMAL = 2.0 ** -14


def tile_scale(tmax):
    """2^k, k = 14 - frexp exponent of tmax, clamped to +-40 (0 -> 2^0): policy_x3.h pm_scale_exp."""
    if not (tmax > 0.0) or not np.isfinite(tmax):
        return 1.0
    k = 14 - int(np.frexp(np.float32(tmax))[1])
    return 2.0 ** max(-40, min(40, k))


def _split(v, flush_subnormals):
    """v (f32, already scaled) -> (hi, lo) as float64 arrays holding f16 values."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)
    hi, lo = hi.astype(np.float64), lo.astype(np.float64)
    if flush_subnormals:
        hi = np.where(np.abs(hi) < F16_MIN_NORMAL, 0.0, hi)
        lo = np.where(np.abs(lo) < F16_MIN_NORMAL, 0.0, lo)
    return hi, lo


def split_f16_matmul(a, W, flush_subnormals=False, tmax=None):
    """The split-f16 product of one row tile: a [rows <= 16][K] (f32 values), W [N][K] -> [rows][N]
    float64 (the three kept products summed exactly). tmax: the tile's max |a| where rows the
    kernel sees are not in `a` (the padded rows of a ragged tile)."""
    a = np.asarray(a, dtype=np.float32)
    W = np.asarray(W, dtype=np.float32)
    t = float(np.abs(a).max()) if tmax is None else float(tmax)
    sa = tile_scale(t)
    ah, al = _split(a * np.float32(sa), flush_subnormals)
    wh, wl = _split(W * np.float32(WX), flush_subnormals)
    with np.errstate(invalid="ignore"):
        acc = al @ wh.T + ah @ wl.T + ah @ wh.T
    return acc / (sa * WX)


def split_f16_bound(a, W, tmax=None):
    """The contract's bound on |split product - exact product|, per output element [rows][N]."""
    a = np.abs(np.asarray(a, dtype=np.float64))
    W = np.abs(np.asarray(W, dtype=np.float64))
    t = float(a.max()) if tmax is None else float(tmax)
    return (4.0 * 2.0 ** -22 * (a @ W.T) + 2.0 ** -37 * t * W.sum(1)[None, :] + 2.0 ** -34 * a.sum(1)[:, None]
            + 1e-30)
