#!/usr/bin/env python
"""Golden fixture of the Mistral flash path: transformers' MistralForCausalLM, fp32 on the CPU, on the seeded tiny checkpoints
of tests/mistral_tiny.py (the reference project has no Mistral model; transformers' sliding-window semantics are the arbiter).
Only outputs are written; the tests rebuild the weights from the seed.

    python tests/golden/make_mistral_fixtures.py [first seed]      (the committed file: seed 1098, found from 0; minutes)

Writes tests/golden/mistral_window.npz:
  window   sliding_window 40, prompts of 7, 45 and 100 tokens (below the window, across it, beyond it), 50 greedy tokens each:
           ids [3, 50], logits [3, 50, vocab] (the logits each token was chosen from), the prompts, the smallest top-2 margin.
           Every step is a full forward over the sequence so far, so nothing depends on a cache implementation.  The seed is
           the first at which every top-2 margin exceeds MARGIN = 0.7 logits, twice the f16 logit bound of the GPU tests: exact
           ids are then a fair demand.
  headdim  head_dim 32 on hidden 256 / 4 heads (head size != hidden / heads), a prompt of 12 tokens: the prefill's logits
           [12, vocab].
The generator asserts that the window is applied: the windowed model's logits differ from its unwindowed twin's first at
position 40."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from mistral_tiny import TinyMistralConfig, tiny_mistral_tensors  # noqa: E402

MARGIN = 0.7
PROMPT_LENS = (7, 45, 100)
NEW_TOKENS = 50
HEADDIM_SEED = 5


def hf_model(cfg, seed):
    from transformers import MistralConfig, MistralForCausalLM

    kw = cfg.to_dict()
    model = MistralForCausalLM(MistralConfig(**kw, attn_implementation="eager"))
    missing, unexpected = model.load_state_dict({k: v.float() for k, v in tiny_mistral_tensors(cfg, seed).items()},
                                                strict=False)
    assert not unexpected and all("rotary" in m or "inv_freq" in m for m in missing), (missing, unexpected)
    return model.float().eval()


@torch.no_grad()
def logits_of(model, ids):
    return model(input_ids=torch.tensor([ids]), use_cache=False).logits[0].float()


def greedy(model, prompt):
    ids, out_ids, out_logits, margin = list(prompt), [], [], float("inf")
    for _ in range(NEW_TOKENS):
        row = logits_of(model, ids)[-1]
        top = torch.topk(row, 2).values
        margin = min(margin, float(top[0] - top[1]))
        out_ids.append(int(row.argmax()))
        out_logits.append(row.numpy())
        ids.append(out_ids[-1])
    return out_ids, np.stack(out_logits), margin


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    rng = np.random.default_rng(2026)
    prompts = [rng.integers(3, 256, size=n).tolist() for n in PROMPT_LENS]
    while True:
        cfg = TinyMistralConfig()
        model = hf_model(cfg, seed)
        runs = [greedy(model, p) for p in prompts]
        margin = min(r[2] for r in runs)
        print(f"seed {seed}: smallest top-2 margin {margin:.3f}", flush=True)
        if margin > MARGIN:
            break
        seed += 1
    assert margin > MARGIN
    # the window is applied: against the unwindowed twin the logits first differ at position W
    twin = hf_model(TinyMistralConfig(sliding_window=None), seed)
    full = prompts[2] + runs[2][0]
    diff = (logits_of(model, full) - logits_of(twin, full)).abs().amax(dim=1)
    first = int((diff > 1e-4).nonzero()[0])
    assert first == cfg.sliding_window, first

    hcfg = TinyMistralConfig(head_dim=32)
    hprompt = rng.integers(3, 256, size=12).tolist()
    hlogits = logits_of(hf_model(hcfg, HEADDIM_SEED), hprompt).numpy()

    import transformers

    meta = {"seed": seed, "config": cfg.to_dict(), "prompts": prompts, "max_new": NEW_TOKENS, "min_margin": margin,
            "margin_bound": MARGIN, "headdim_seed": HEADDIM_SEED, "headdim_config": hcfg.to_dict(),
            "headdim_prompt": hprompt, "transformers": transformers.__version__, "torch": torch.__version__}
    np.savez_compressed(os.path.join(HERE, "mistral_window.npz"),
                        meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8),
                        ids=np.array([r[0] for r in runs], dtype=np.int64),
                        logits=np.stack([r[1] for r in runs]).astype(np.float32),
                        headdim_logits=hlogits.astype(np.float32))
    print("wrote mistral_window.npz:", meta["seed"], meta["min_margin"])


if __name__ == "__main__":
    main()
