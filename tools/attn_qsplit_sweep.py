"""Key splits of tgis_attn_paged with a few q tokens per sequence (a verify step of speculative decoding, a short suffix
behind reused prefix pages) over long contexts: the sweep the rule tgis_attn_num_splits_q is fitted to.

Per (shape, B, q_len, ctx): the median us of the launch (HIP events around each call, `--iters` of them, rotating over
`--sets` pools so that no launch finds the previous one's pages in L2 / MALL) at 1, 2, 4, 8, 16 and 32 splits and at the
rule's own count; the rule's choice is printed next to the fastest measured count and marked where it is slower than that
by more than --spread (the box's block-to-block spread).  Shapes: Llama-2-7B (32 q heads on 32 kv
heads), GQA 8:1 (64 on 8), MQA 48:1 (q_len <= 4: beyond it the launch is the prefill form); D 128, f16.

--nw 8 forces the 8-wave blocks that one-token launches with few groups take (TGIS_ATTN_NW), for the A/B of
wide_decode_blocks at q_len > 1.

    python tools/attn_qsplit_sweep.py > profiles/attn_qsplit_sweep.log
    python tools/attn_qsplit_sweep.py --nw 8 --shapes 7b --bs 1 --qs 4"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "text-generation-inference_amd"))
import torch  # noqa: E402

from tgis_amd import native as nat  # noqa: E402

SHAPES = {"7b": (32, 32, (2, 4, 8)), "gqa8": (64, 8, (2, 4, 8)), "mqa48": (48, 1, (2, 4))}
SPLITS = (1, 2, 4, 8, 16, 32)
D = 128


def time_us(call, sets, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for i in range(3):
        call(i % sets)
    for i, (a, b) in enumerate(ev):
        a.record()
        call(i % sets)
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="7b,gqa8,mqa48")
    ap.add_argument("--bs", default="1,4,8")
    ap.add_argument("--qs", default="2,4,8")
    ap.add_argument("--ctxs", default="1024,2048,4096,8192,16384,32768")
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--spread", type=float, default=0.02)
    ap.add_argument("--nw", type=int, default=0, help="force this many waves per block (TGIS_ATTN_NW)")
    args = ap.parse_args()
    if args.nw:
        os.environ["TGIS_ATTN_NW"] = str(args.nw)
    dev = torch.device("cuda:0")
    nat.load_library()
    print(f"# {nat.version()} {torch.cuda.get_device_name(0)}  waves per block: {args.nw or 'the launcher`s'}  "
          f"median of {args.iters} launches, {args.sets} pool sets, us", flush=True)
    print("# shape B q_len ctx | " + " ".join(f"ns{n:<6d}" for n in SPLITS) + " | rule best | rule_us best_us", flush=True)
    worst = []
    for name in args.shapes.split(","):
        H, Hkv, qs = SHAPES[name]
        for B in (int(b) for b in args.bs.split(",")):
            for ctx in (int(c) for c in args.ctxs.split(",")):
                pages_per = (ctx + 31) // 32
                total = B * pages_per
                sets = max(1, min(args.sets, int(6e9 // (total * Hkv * 32 * D * 4))))
                pools = [(torch.randn(total, Hkv, 32 * D, device=dev, dtype=torch.float16),
                          torch.randn(total, Hkv, 32 * D, device=dev, dtype=torch.float16)) for _ in range(sets)]
                bt = torch.randperm(total, device=dev).int().view(B, pages_per).contiguous()
                ctxl = torch.full((B,), ctx, dtype=torch.int32, device=dev)
                for q in (int(x) for x in args.qs.split(",")):
                    if q not in qs:
                        continue
                    qa = torch.randn(B * q, H * D, device=dev, dtype=torch.float16)
                    cu = torch.arange(B + 1, dtype=torch.int32, device=dev) * q
                    out = torch.empty(B * q, H * D, device=dev, dtype=torch.float16)
                    rule = nat.attn_num_splits_q(B, Hkv, H, q, ctx)
                    t = {}
                    for ns in sorted(set(SPLITS) | {rule}):
                        ws = nat.Workspace(max(nat.attn_workspace_bytes(B * q, H, Hkv, D, ns), 256), dev)
                        t[ns] = time_us(lambda i: nat.attn_paged(qa, H * D, pools[i][0], pools[i][1], bt, ctxl, cu, out, B, H,
                                                                 Hkv, D, q, ctx, D ** -0.5, ns, ws if ns > 1 else None),
                                        sets, args.iters)
                    best = min(t, key=t.get)
                    off = t[rule] / t[best] - 1
                    mark = "" if off <= args.spread else f"  <-- rule {off * 100:.1f} % slower than {best} splits"
                    if mark:
                        worst.append((name, B, q, ctx, rule, best, t[rule], t[best]))
                    print(f"{name:6s} {B:2d} {q:2d} {ctx:6d} | " + " ".join(f"{t[n]:8.1f}" for n in SPLITS) +
                          f" | {rule:3d} {best:3d} | {t[rule]:8.1f} {t[best]:8.1f}{mark}", flush=True)
                del pools
                torch.cuda.empty_cache()
    print(f"# {len(worst)} points where the rule is more than {args.spread * 100:.0f} % off the fastest count", flush=True)


if __name__ == "__main__":
    main()
