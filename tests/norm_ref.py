"""InstanceNorm3d (+ residual) (+ ReLU / LeakyReLU), forward and backward, restated in float64 with plain tensor arithmetic, and the
per-element error bounds the kernels of csrc/instnorm.hip are held to (tests/norm_checks.py).  Nothing here is fitted to a kernel.

Every function takes (instances, S) tensors on any device; the 16 / 32-bit inputs convert to float64 exactly.

    mean, var (biased), rstd = (var + eps)^-1/2          per instance
    xh = (x - mean) rstd,  pre = xh + residual,  y = act(pre)
    g = dy act'(pre),  mg = mean(g),  mgx = mean(g xh),  dx = rstd (g - mg - xh mgx),  dresidual = g

The bounds.  u = 2^-24; p = 24 / 11 / 8 bits for fp32 / fp16 / bf16; ulp_T(a) = 2^(floor(log2 a) - p + 1), never below the spacing
of the type's subnormals; r = |mean| rstd.

Statistics: sum and sum of squares accumulated in fp32 in any order whose longest chain of additions is at most 256 (Higham:
(n - 1) u sum|x_i|), so
    |mean_k - mean| rstd <= eps_m = 2^-16 (1 + r)
    |rstd_k / rstd - 1|  <= eps_r = 2^-15 (1 + r^2)      (1 + r^2: the condition number of E[x^2] - mean^2)
Forward, no element left out (an activation of slope <= 1 is 1-Lipschitz: a flipped sign near zero costs at most d_y):
    d_y = eps_m + |xh| eps_r + 2^-22 (|x| rstd + |mean| rstd + |residual|)
    |y_k - y| <= d_y + ulp_T(|y| + d_y) / 2
Backward, given mean and rstd (the float64 values rounded to fp32), band = d_xh = 2^-22 (|x| rstd + |mean| rstd):
    e_mg  = 2^-16 mean|g| + F
    e_mgx = 2^-16 mean|g xh| + Fx + mean(|g| band)
    d_dx  = rstd (2^-22 (|g| + |mg| + |xh mgx|) + e_mg + |xh| e_mgx + band |mgx|) + 2^-23 |dx| + P
    |dx_k - dx| <= d_dx + ulp_T(|dx| + d_dx) / 2
An element is left out of the dx and dresidual comparisons iff there is an activation and |pre| <= band (its mask may flip); F and
Fx are what those flips can move the two means by: the sums over them of (1 - slope) |dy| / S and (1 - slope) |dy xh| / S.
P = rstd ulp_T(|g|) / 2 exactly when dresidual is wanted, the type has 16 bits and the activation is LeakyReLU: the backward
statistics pass parks g = dy act' in dresidual, rounded to the type, and the apply pass forms dx from that rounded value.
Backward through the kernel's own forward (its statistics, its mask): band = d_y, and eps_r |dx| is added to d_dx.
dresidual, outside the exclusions, equals (float(dy) * s) rounded to the type, s in {1, slope, 0}, bit for bit (-0 == 0)."""
import torch

P_BITS = {torch.float32: 24, torch.float16: 11, torch.bfloat16: 8}
MIN_EXP = {torch.float32: -149, torch.float16: -24, torch.bfloat16: -133}        # log2 of the subnormal spacing


def f32(v):
    """a Python number as the fp32 value a kernel argument of type float carries"""
    return float(torch.tensor(v, dtype=torch.float32))


def ulp(a, dtype):
    a = a.double()
    _, e = torch.frexp(a)                                  # a = m 2^e, m in [0.5, 1): floor(log2 a) = e - 1
    e = e.to(torch.int32) - P_BITS[dtype]
    e = torch.where(a > 0, e, torch.full_like(e, MIN_EXP[dtype])).clamp_(min=MIN_EXP[dtype])
    return torch.ldexp(torch.ones_like(a), e)


def restate(x, residual, dy, act, slope, eps):
    """-> dict of float64 tensors: mean, rstd (instances, 1); x, res, dy, xh, pre, y, g, mg, mgx, dx (dy = None: forward only)"""
    assert act in ("none", "relu", "leaky_relu") and x.dim() == 2
    slope = 0.0 if act == "relu" else f32(slope)
    x = x.double()
    S = x.shape[1]
    mean = x.sum(1, keepdim=True) / S
    xc = x - mean
    var = (xc * xc).sum(1, keepdim=True) / S
    rstd = (var + f32(eps)) ** -0.5
    xh = xc * rstd
    res = residual.double() if residual is not None else torch.zeros_like(x)
    pre = xh + res
    R = dict(S=S, slope=slope, act=act, x=x, res=res, mean=mean, rstd=rstd, xh=xh, pre=pre)
    R["y"] = pre if act == "none" else torch.where(pre > 0, pre, pre * slope)
    if dy is not None:
        dy = dy.double()
        g = dy if act == "none" else torch.where(pre > 0, dy, dy * slope)
        mg = g.sum(1, keepdim=True) / S
        mgx = (g * xh).sum(1, keepdim=True) / S
        R.update(dy=dy, g=g, mg=mg, mgx=mgx, dx=rstd * (g - mg - xh * mgx))
    return R


def stats_bounds(R):
    """-> (eps_m, eps_r), (instances, 1)"""
    r = R["mean"].abs() * R["rstd"]
    return 2.0 ** -16 * (1 + r), 2.0 ** -15 * (1 + r * r)


def stats_errors(R, mean_k, rstd_k):
    """-> (|mean_k - mean| rstd, |rstd_k / rstd - 1|), (instances, 1)"""
    return ((mean_k.double().reshape(-1, 1) - R["mean"]).abs() * R["rstd"],
            (rstd_k.double().reshape(-1, 1) / R["rstd"] - 1).abs())


def _d_xh(R):
    return 2.0 ** -22 * (R["x"].abs() + R["mean"].abs()) * R["rstd"]


def _d_y(R):
    eps_m, eps_r = stats_bounds(R)
    return eps_m + R["xh"].abs() * eps_r + _d_xh(R) + 2.0 ** -22 * R["res"].abs()


def forward_bound(R, dtype):
    d = _d_y(R)
    return d + 0.5 * ulp(R["y"].abs() + d, dtype)


def parks_g(dtype, act, want_dresidual):
    return bool(want_dresidual) and dtype in (torch.float16, torch.bfloat16) and act == "leaky_relu"


def backward_bound(R, dtype, want_dresidual, chained):
    """-> (bound on |dx_k - dx|, the mask of the elements left out).  chained: the kernel's own statistics and mask."""
    band = _d_y(R) if chained else _d_xh(R)
    S, g, xh, rstd, dx = R["S"], R["g"], R["xh"], R["rstd"], R["dx"]
    if R["act"] == "none":
        out = torch.zeros_like(g, dtype=torch.bool)
        F = Fx = 0.0
    else:
        out = R["pre"].abs() <= band
        flip = (1 - R["slope"]) * R["dy"].abs() * out
        F = flip.sum(1, keepdim=True) / S
        Fx = (flip * xh.abs()).sum(1, keepdim=True) / S
    e_mg = 2.0 ** -16 * g.abs().sum(1, keepdim=True) / S + F
    e_mgx = 2.0 ** -16 * (g * xh).abs().sum(1, keepdim=True) / S + Fx + (g.abs() * band).sum(1, keepdim=True) / S
    d = rstd * (2.0 ** -22 * (g.abs() + R["mg"].abs() + (xh * R["mgx"]).abs()) + e_mg + xh.abs() * e_mgx + band * R["mgx"].abs())
    d = d + 2.0 ** -23 * dx.abs()
    if parks_g(dtype, R["act"], want_dresidual):
        d = d + rstd * 0.5 * ulp(g.abs(), dtype)
    if chained:
        d = d + stats_bounds(R)[1] * dx.abs()
    return d + 0.5 * ulp(dx.abs() + d, dtype), out


def dresidual_expected(R, dy, dtype):
    """(float(dy) * s) rounded to the type, s = 1 / slope / 0 by the sign of the float64 pre-activation"""
    if R["act"] == "none":
        return dy.clone()
    s = torch.tensor(R["slope"], dtype=torch.float32, device=dy.device)
    return torch.where(R["pre"] > 0, dy.float(), dy.float() * s).to(dtype)
