"""Restatement of the one-byte KV cache format (csrc/kv_layout.h) for the tests: OCP float8_e4m3fn codes of
sat(x / s), sat = clamp to +-448, round to nearest even.  torch's own cast is the rounding; the clamp comes first because
that cast turns values outside +-448 into NaN (0x7F / 0xFF), which the cache must never hold."""
import torch

E4M3_MAX = 448.0


def quantize(x: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """e4m3 codes (uint8) of x / scale: x is the model-dtype value the 16-bit pool would hold."""
    y = (x.float() / scale).clamp(-E4M3_MAX, E4M3_MAX)
    return y.to(torch.float8_e4m3fn).view(torch.uint8)


def dequantize(codes: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """float32 values of e4m3 codes (uint8) times the scale."""
    return codes.view(torch.float8_e4m3fn).float() * scale
