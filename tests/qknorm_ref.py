"""fp64 restatement of the q/k RMSNorm + rope launches (csrc/qk_norm_rope.hip; transformers' Qwen3Attention.forward) and the
bound the kernels are held to.  TEST INFRASTRUCTURE.

    x      the model-dtype input [T, H + 2 Hkv, D] (for slabs: the fp32 sum s = 0..S-1, then the bias, rounded to the model dtype)
    rstd = (sum_d x^2 / D + eps)^-1/2,   y = x rstd w[d]      (w = q_w for q heads, k_w for k heads)
    o[:r] = y[:r] c - y[r:2r] s,   o[r:2r] = y[:r] s + y[r:2r] c,   o[rot:] = y[rot:]      (r = rot / 2; c, s the model-dtype tables)
    v heads: o = x, bit for bit.

Bound, derived from the kernel's arithmetic (u = 2^-24, the unit roundoff of fp32; u_out that of the output type):
  - the D-term sum of squares is 8 sequential fma per chunk and 4 butterfly levels: 12 roundings on a sum of positive terms,
    relative error <= 12 u; the division by D and the addition of eps add one each: 14 u on the mean, 7 u on its inverse
    square root, plus the 1 ulp (2 u) of the hardware rsqrt: rstd errs by <= 9 u relative;
  - y = (x rstd) w: two more roundings, 11 u relative;
  - the rotation: one rounding of y2 s (or y2 c) and one of the fma: 13 u on |y1 c| + |y2 s| (resp. |y1 s| + |y2 c|);
  - 13 u < 2^-20 = 16 u; then ONE rounding to the output type, u_out |ref|, and its smallest subnormal.
So |o - ref| <= u_out |ref| + 2^-20 (|y1 c| + |y2 s|) + tiny on the rotated dims, u_out |ref| + 2^-20 |y| + tiny behind them, and
0 on the v heads.  None of it is measured."""
import torch

U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
TINY = {torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -133}
F32 = 2.0 ** -20


def expect(x, q_w, k_w, eps, cos, sin, pos, H, Hkv, rot):
    """(ref, tol) in fp64, [T, H + 2 Hkv, D]; tol is 0 where the output must be a copy of x.  x, q_w, k_w, cos, sin: model-dtype
    tensors (cos / sin the [max_pos, rot / 2] tables of oracle.ops_ref.rope_tables), pos [T] integer positions."""
    dt = x.dtype
    T, heads, D = x.shape
    assert heads == H + 2 * Hkv and rot % 2 == 0 and 0 < rot <= D
    xd = x.double()
    ref, tol = xd.clone(), torch.zeros_like(xd)
    n = H + Hkv
    w = torch.cat([q_w.double().expand(H, D), k_w.double().expand(Hkv, D)])[None]  # [1, H + Hkv, D]
    xs = xd[:, :n]
    rstd = (xs.pow(2).sum(-1, keepdim=True) / D + eps).rsqrt()
    y = xs * rstd * w
    r = rot // 2
    c = cos.double()[pos.long()][:, None, :]
    s = sin.double()[pos.long()][:, None, :]
    y1, y2 = y[..., :r], y[..., r:rot]
    o1, o2 = y1 * c - y2 * s, y1 * s + y2 * c
    ref[:, :n, :r], ref[:, :n, r:rot], ref[:, :n, rot:] = o1, o2, y[..., rot:]
    tol[:, :n, :r] = U[dt] * o1.abs() + F32 * ((y1 * c).abs() + (y2 * s).abs()) + TINY[dt]
    tol[:, :n, r:rot] = U[dt] * o2.abs() + F32 * ((y1 * s).abs() + (y2 * c).abs()) + TINY[dt]
    tol[:, :n, rot:] = (U[dt] + F32) * y[..., rot:].abs() + TINY[dt]
    return ref, tol
