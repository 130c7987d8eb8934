"""Sliding-window attention restated in fp64 over unpacked K / V (TEST INFRASTRUCTURE; imports nothing of the code under test).

The semantics are those of transformers' MistralForCausalLM (config.sliding_window = W >= 1):
  * the q row at cache position p attends to the cache positions j with p - W < j <= p: W keys, its own among them;
  * q row i of a sequence of ctx cached tokens, the last q_len of them q rows, sits at p = ctx - q_len + i;
  * a window no row reaches (ctx <= W) is causal attention."""
import torch

PAGE = 32


def first_visible_key(ctx: int, q_len: int, i: int, window: int) -> int:
    """The first cache position q row i attends to."""
    assert window >= 1 and 1 <= q_len <= ctx and 0 <= i < q_len
    return max(0, ctx - q_len + i - window + 1)


def first_visible_page(ctx: int, q_len: int, window: int) -> int:
    """The first page any q row of the sequence attends to: every page below it lies wholly below the window."""
    return first_visible_key(ctx, q_len, 0, window) // PAGE


def visible(ctx: int, q_len: int, window: int) -> torch.Tensor:
    """bool [q_len, ctx]: whether q row i attends to cache position j."""
    p = torch.arange(ctx - q_len, ctx)[:, None]
    j = torch.arange(ctx)[None, :]
    return (j <= p) & (j > p - window)


def window_attention(q: torch.Tensor, K: torch.Tensor, V: torch.Tensor, window: int, scale: float) -> torch.Tensor:
    """softmax(q K^T scale + mask) V of one sequence: q [q_len, H, D], K / V [ctx, Hkv, D] -> fp64 [q_len, H, D]; q head h
    reads kv head h // (H / Hkv)."""
    q_len, H, _ = q.shape
    ctx, Hkv, _ = K.shape
    G = H // Hkv
    qd = q.double().transpose(0, 1)                                   # [H, q_len, D]
    kd = K.double().transpose(0, 1).repeat_interleave(G, dim=0)       # [H, ctx, D]
    vd = V.double().transpose(0, 1).repeat_interleave(G, dim=0)
    s = torch.matmul(qd, kd.transpose(1, 2)) * scale
    s = s.masked_fill(~visible(ctx, q_len, window)[None], float("-inf"))
    return torch.matmul(torch.softmax(s, dim=-1), vd).transpose(0, 1)
