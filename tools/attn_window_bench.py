"""Sliding-window decode attention next to the causal launch (tgis_attn_paged_window / tgis_attn_paged).  GPU box only.
    python tools/attn_window_bench.py [B H Hkv D W]        (default 32 32 8 128 4096: Mistral-7B's layer at batch 32)

Per ctx in 4096, 8192, 32768, one launch each, us of GPU time (tools/microbench.py timeit: 20 calls in one HIP graph over
rotating pools):
  windowed   the windowed launch at ctx, key splits from tgis_attn_num_splits(B, Hkv, H, 1, min(ctx, W + 31)) as the decode
             graph sizes them (ctx <= W: the library makes the causal launch)
  causal     the causal launch at the same ctx, its own split rule
  causal@W   the causal launch at ctx = W: the yardstick — the windowed launch reads the same number of pages plus one masked
             page per sequence
and the ratio windowed / causal@W."""
import sys

import torch

sys.path.insert(0, "tools")
sys.path.insert(0, "text-generation-inference_amd")
import microbench as mb  # noqa: E402
from microbench import dev, nat  # noqa: E402

B, H, Hkv, D, W = (int(v) for v in sys.argv[1:6]) if len(sys.argv) >= 6 else (32, 32, 8, 128, 4096)
CTXS = (4096, 8192, 32768)
SETS = 2


def launch_us(pools, bt, ctx, window):
    keys = ctx if window is None else min(ctx, window + 31)
    ns = nat.attn_num_splits(B, Hkv, H, 1, keys)
    q = torch.randn(B, H * D, device=dev).half()
    ctxl = torch.full((B,), ctx, dtype=torch.int32, device=dev)
    cu = torch.arange(B + 1, dtype=torch.int32, device=dev)
    out = torch.empty(B, H * D, device=dev, dtype=torch.float16)
    ws = nat.Workspace(nat.attn_workspace_bytes(B, H, Hkv, D, ns), dev)
    kw = {} if window is None else {"window": window}
    t = mb.timeit(lambda i: nat.attn_paged(q, H * D, pools[i][0], pools[i][1], bt, ctxl, cu, out, B, H, Hkv, D, 1, ctx,
                                           D ** -0.5, ns, ws, **kw), SETS)
    return t * 1e6, ns


def main():
    print(nat.version(), torch.cuda.get_device_name(0))
    print(f"B {B} H {H} Hkv {Hkv} D {D} W {W}, f16")
    pages_per = (max(CTXS) + 31) // 32
    total = B * pages_per
    pools = [(torch.randn(total, Hkv, 32 * D, device=dev).half(), torch.randn(total, Hkv, 32 * D, device=dev).half())
             for _ in range(SETS)]
    bt = torch.randperm(total, device=dev).int().view(B, pages_per).contiguous()
    base, base_ns = launch_us(pools, bt, W, None)
    print(f"causal@W ctx {W}: {base:8.1f} us ({base_ns} split(s))")
    for ctx in CTXS:
        win, win_ns = launch_us(pools, bt, ctx, W)
        cau, cau_ns = launch_us(pools, bt, ctx, None)
        print(f"ctx {ctx:6d}: windowed {win:8.1f} us ({win_ns} split(s))   causal {cau:8.1f} us ({cau_ns} split(s))   "
              f"causal@W {base:8.1f} us   windowed / causal@W = {win / base:.3f}")


if __name__ == "__main__":
    main()
