#!/usr/bin/env python
"""Golden fixture of the GPTQ Mixtral flash path: transformers' MixtralForCausalLM, fp32 on the CPU, on the dequantised
weights of the seeded tiny GPTQ checkpoint of tests/mixtral_gptq_tiny.py (q/k/v/o and every expert's w1 / w3 / w2 at 4 bits,
group size 64; router, norms, embeddings and head in f16).  The pattern, the margins and the helpers are
make_mixtral_fixtures.py's; only outputs are written, the tests rebuild the checkpoint from the seed.

    python tests/golden/make_mixtral_gptq_fixtures.py [first seed] [output file]      (the committed file: seed 32, found from 0)

Writes tests/golden/mixtral_gptq_top2.npz: prompts of 5, 20 and 33 tokens, 5 greedy tokens each: ids, the logits each token
was chosen from, per prompt the router's top-2 expert indices of every layer and token of the last forward, and meta (seed,
prompts, margins).  The seed is the first at which every top-2 logit margin exceeds MARGIN = 0.7 = twice LOGIT_TOL and every
router's 2nd-to-3rd gap exceeds ROUTER_FACTOR times the largest router-logit deviation of a float16 CPU run of the same
weights: only then are exact ids and exact routing fair demands of a 16-bit run."""
import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import make_mixtral_fixtures as base  # noqa: E402
from mixtral_gptq_tiny import GS, dense_tensors, tiny_mixtral_gptq_tensors  # noqa: E402
from mixtral_tiny import TinyMixtralConfig, fused_names  # noqa: E402


def hf_model(cfg, seed):
    from transformers import MixtralConfig, MixtralForCausalLM

    model = MixtralForCausalLM(MixtralConfig(**cfg.to_dict(), attn_implementation="eager"))
    dense = dense_tensors(tiny_mixtral_gptq_tensors(cfg, seed))
    state = {k: v.float() for k, v in fused_names(dense, cfg).items()}
    missing, unexpected = model.load_state_dict(state, strict=False)
    assert not unexpected and all("rotary" in m or "inv_freq" in m for m in missing), (missing, unexpected)
    return model.float().eval()


def main():
    first = seed = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "mixtral_gptq_top2.npz")
    rng = np.random.default_rng(2027)
    prompts = [rng.integers(3, 256, size=n).tolist() for n in base.PROMPT_LENS]
    cfg = TinyMixtralConfig()
    while True:
        assert seed - first < base.MAX_TRIES, "no seed found: shorten the generation, do not lower ROUTER_FACTOR"
        model = hf_model(cfg, seed)
        runs = []
        for p in prompts:
            r = base.greedy(model, p)
            if r is None:
                break
            runs.append(r)
        if len(runs) < len(prompts):
            print(f"seed {seed}: a top-2 logit margin is below {base.MARGIN}", flush=True)
            seed += 1
            continue
        margin = min(r[2] for r in runs)
        half = copy.deepcopy(model).half()
        dev = max(float((base.forward(half, r[3])[1] - r[4]).abs().max()) for r in runs)
        router_margin = base.ROUTER_FACTOR * dev
        top3 = [torch.topk(r[4], 3, dim=-1).values for r in runs]
        gap = min(float((t[..., 1] - t[..., 2]).min()) for t in top3)
        events = sum(t.shape[0] * t.shape[1] for t in top3)
        print(f"seed {seed}: top-2 logit margin {margin:.3f}; f16 router deviation {dev:.5f} -> ROUTER_MARGIN "
              f"{router_margin:.5f}; smallest 2nd-3rd router gap {gap:.5f} over {events} events", flush=True)
        if gap > router_margin:
            break
        seed += 1
    restore = base.force_experts_0_1()
    try:
        moved = min(float((base.forward(model, r[3])[0][-1] - torch.from_numpy(r[1][-1])).abs().max()) for r in runs)
    finally:
        restore()
    assert moved > base.MARGIN / 2, moved

    import transformers

    meta = {"seed": seed, "config": cfg.to_dict(), "groupsize": GS, "bits": 4, "prompts": prompts,
            "max_new": base.NEW_TOKENS, "min_margin": margin, "margin_bound": base.MARGIN, "router_margin": router_margin,
            "router_factor": base.ROUTER_FACTOR, "f16_router_deviation": dev, "min_router_gap": gap,
            "router_events": events, "forced_experts_move": moved, "transformers": transformers.__version__,
            "torch": torch.__version__}
    arrays = {f"router_idx_{i}": torch.topk(r[4], 2, dim=-1).indices.numpy().astype(np.int32) for i, r in enumerate(runs)}
    np.savez_compressed(out_path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8),
                        ids=np.array([r[0] for r in runs], dtype=np.int64),
                        logits=np.stack([r[1] for r in runs]).astype(np.float32), **arrays)
    print("wrote", os.path.basename(out_path), json.dumps({k: meta[k] for k in ("seed", "min_margin", "router_margin",
                                                                                "min_router_gap")}))


if __name__ == "__main__":
    main()
