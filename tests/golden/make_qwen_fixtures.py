#!/usr/bin/env python
"""Golden fixtures of the Qwen3 and Qwen2 flash paths: transformers' Qwen3ForCausalLM / Qwen2ForCausalLM, fp32 on the CPU, on
the seeded tiny checkpoints of tests/qwen_tiny.py (the reference project has neither model; transformers is the arbiter).
Only outputs are written; the tests rebuild the weights from the seed.

    python tests/golden/make_qwen_fixtures.py qwen3 [first seed]      (the committed file: seed 255, found from 0)
    python tests/golden/make_qwen_fixtures.py qwen2 [first seed]      (the committed file: seed 163, found from 0)

A seed is given up at its first margin below the bound, so the search is minutes, most of them the accepted seed's 150 forwards.

Writes tests/golden/qwen3_tiny.npz / qwen2_tiny.npz: prompts of 7, 45 and 100 tokens, 50 greedy tokens each: ids [3, 50],
logits [3, 50, vocab] (the logits each token was chosen from), the prompts, the smallest top-2 margin.  Every step is a full
forward over the sequence so far (use_cache=False), so nothing depends on a cache implementation.  The seed is the first at
which every top-2 margin exceeds MARGIN = 0.7 logits, twice the f16 logit bound of the GPU tests: exact ids are then a fair
demand.
qwen3: the generator asserts that the q / k norm matters: a LlamaForCausalLM twin built from the same tensors without the norm
weights differs from the Qwen3 logits by more than 0.35 at the first generated token of every prompt.
qwen2: it asserts likewise that the q/k/v biases matter (a twin without them)."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from qwen_tiny import TinyQwenConfig, tiny_qwen_tensors  # noqa: E402

MARGIN = 0.7
TWIN_BAR = 0.35
PROMPT_LENS = (7, 45, 100)
NEW_TOKENS = 50


def _load(model, tensors):
    missing, unexpected = model.load_state_dict({k: v.float() for k, v in tensors.items()}, strict=False)
    assert not unexpected and all("rotary" in m or "inv_freq" in m or m == "lm_head.weight" for m in missing), \
        (missing, unexpected)
    return model.float().eval()


def hf_model(cfg, seed):
    import transformers

    name = {"qwen3": "Qwen3", "qwen2": "Qwen2"}[cfg.model_type]
    kw = cfg.to_dict()
    kw.pop("model_type")
    config = getattr(transformers, name + "Config")(**kw, attn_implementation="eager")
    return _load(getattr(transformers, name + "ForCausalLM")(config), tiny_qwen_tensors(cfg, seed))


def llama_twin(cfg, seed):
    """The same tensors as a Llama: no q_norm / k_norm, no q/k/v bias."""
    from transformers import LlamaConfig, LlamaForCausalLM

    kw = cfg.to_dict()
    for k in ("model_type", "sliding_window", "use_sliding_window", "max_window_layers"):
        kw.pop(k)
    kw.update(attention_bias=False, mlp_bias=False)
    tensors = {k: v for k, v in tiny_qwen_tensors(cfg, seed).items()
               if ".q_norm." not in k and ".k_norm." not in k and not k.endswith("_proj.bias")}
    return _load(LlamaForCausalLM(LlamaConfig(**kw, attn_implementation="eager")), tensors)


@torch.no_grad()
def logits_of(model, ids):
    return model(input_ids=torch.tensor([ids]), use_cache=False).logits[0].float()


def greedy(model, prompt, bound=None):
    """50 greedy tokens; with `bound`, gives up (None) at the first top-2 margin that does not exceed it."""
    ids, out_ids, out_logits, margin = list(prompt), [], [], float("inf")
    for _ in range(NEW_TOKENS):
        row = logits_of(model, ids)[-1]
        top = torch.topk(row, 2).values
        margin = min(margin, float(top[0] - top[1]))
        if bound is not None and margin <= bound:
            return None
        out_ids.append(int(row.argmax()))
        out_logits.append(row.numpy())
        ids.append(out_ids[-1])
    return out_ids, np.stack(out_logits), margin


def prompts_for():
    rng = np.random.default_rng(2026)
    return [rng.integers(3, 256, size=n).tolist() for n in PROMPT_LENS]


def try_seed(model_type, seed, prompts):
    model = hf_model(TinyQwenConfig(model_type), seed)
    runs = []
    for p in prompts:
        r = greedy(model, p, MARGIN)
        if r is None:
            return None, model
        runs.append(r)
    return runs, model


def main():
    model_type = sys.argv[1]
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    prompts = prompts_for()
    while True:
        runs, model = try_seed(model_type, seed, prompts)
        if runs is not None:
            break
        print(f"seed {seed}: a top-2 margin of at most {MARGIN}", flush=True)
        seed += 1
    cfg = TinyQwenConfig(model_type)
    margin = min(r[2] for r in runs)
    assert margin > MARGIN
    # the norm (qwen3) / the biases (qwen2) matter: the Llama twin is another model at the first generated token
    twin = llama_twin(cfg, seed)
    twin_diff = [float((logits_of(twin, p)[-1] - torch.from_numpy(r[1][0])).abs().max()) for p, r in zip(prompts, runs)]
    assert min(twin_diff) > TWIN_BAR, twin_diff

    import transformers

    meta = {"seed": seed, "config": cfg.to_dict(), "prompts": prompts, "max_new": NEW_TOKENS, "min_margin": margin,
            "margin_bound": MARGIN, "llama_twin_diff": twin_diff, "transformers": transformers.__version__,
            "torch": torch.__version__}
    out = os.path.join(HERE, f"{model_type}_tiny.npz")
    np.savez_compressed(out, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8),
                        ids=np.array([r[0] for r in runs], dtype=np.int64),
                        logits=np.stack([r[1] for r in runs]).astype(np.float32))
    print(f"wrote {out}: seed {seed}, smallest margin {margin:.3f}, twin differs by {min(twin_diff):.2f}")


if __name__ == "__main__":
    main()
