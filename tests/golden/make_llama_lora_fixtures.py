#!/usr/bin/env python
"""Golden fixture of per-request LoRA adapters on the Llama flash path: transformers' LlamaForCausalLM, fp32 on the CPU, on the
seeded tiny Llama and the three seeded adapters of tests/lora_tiny.py, each adapter MERGED into the weights (W + (alpha / r) B A:
peft is not needed).  Only outputs are written; the tests rebuild base and adapters from the seed.

    python tests/golden/make_llama_lora_fixtures.py [first seed]

Writes tests/golden/llama_lora.npz:
  prompts of 5, 20, 33 and 12 tokens, one each for no adapter, `qv`, `all` and `od`, 12 greedy tokens each:
    ids [4, 12], logits [4, 12, vocab] (the logits each token was chosen from) of request i under ITS model;
    base_ids [4, 12], base_logits [4, 12, vocab] of the same prompts under the base model (what a build that ignores the
    adapters gives);
  a prompt of 100 tokens under `all` (past the 64 rows of the kernel path), 4 greedy tokens: long_ids [4], long_logits [4, vocab].
Every step is a full forward over the sequence so far, so nothing depends on a cache implementation.  The seed is the first at
which every top-2 margin of all these runs exceeds MARGIN = 0.7 logits, twice the f16 logit bound of the GPU tests: exact ids are
then a fair demand.  The maker asserts that every adapter matters: its step-0 logits differ from the base model's by more than
MARGIN, and its ids leave the base model's within the run."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.lora_tiny import ADAPTER_NAMES, TinyLlamaConfig, merged_state_dict, tiny_llama_tensors  # noqa: E402

MARGIN = 0.7
PROMPT_LENS = (5, 20, 33, 12)
NEW_TOKENS = 12
LONG_LEN, LONG_TOKENS = 100, 4
VARIANTS = (None,) + ADAPTER_NAMES


def hf_model(cfg, sd):
    from transformers import LlamaConfig, LlamaForCausalLM

    hf_cfg = LlamaConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
                         num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                         num_key_value_heads=cfg.num_key_value_heads, rms_norm_eps=cfg.rms_norm_eps,
                         rope_theta=cfg.rope_theta, max_position_embeddings=cfg.max_position_embeddings,
                         pad_token_id=0, bos_token_id=1, eos_token_id=2, tie_word_embeddings=False,
                         attention_bias=False, attn_implementation="eager")
    model = LlamaForCausalLM(hf_cfg)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("rotary" in m or "inv_freq" in m for m in missing), (missing, unexpected)
    return model.float().eval()


@torch.no_grad()
def greedy(model, prompt, new_tokens):
    ids, out_ids, out_logits, margin = list(prompt), [], [], float("inf")
    for _ in range(new_tokens):
        row = model(input_ids=torch.tensor([ids]), use_cache=False).logits[0, -1].float()
        top = torch.topk(row, 2).values
        margin = min(margin, float(top[0] - top[1]))
        out_ids.append(int(row.argmax()))
        out_logits.append(row.numpy())
        ids.append(out_ids[-1])
    return out_ids, np.stack(out_logits), margin


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    rng = np.random.default_rng(2027)
    prompts = [rng.integers(3, 256, size=n).tolist() for n in PROMPT_LENS]
    long_prompt = rng.integers(3, 256, size=LONG_LEN).tolist()
    cfg = TinyLlamaConfig()
    while True:
        base = tiny_llama_tensors(cfg, seed)
        models = {v: hf_model(cfg, merged_state_dict(cfg, base, v, seed)) for v in VARIANTS}
        base_runs = [greedy(models[None], p, NEW_TOKENS) for p in prompts]
        margin = min(r[2] for r in base_runs)
        runs = None
        if margin > MARGIN:
            runs = [base_runs[0]] + [greedy(models[v], p, NEW_TOKENS) for v, p in zip(VARIANTS[1:], prompts[1:])]
            long_run = greedy(models["all"], long_prompt, LONG_TOKENS)
            margin = min([margin, long_run[2]] + [r[2] for r in runs])
        print(f"seed {seed}: smallest top-2 margin {margin:.3f}", flush=True)
        if margin > MARGIN:
            break
        seed += 1
    # every adapter matters
    moved = []
    for i in range(1, 4):
        diff = float(np.abs(runs[i][1][0] - base_runs[i][1][0]).max())
        moved.append(diff)
        assert diff > MARGIN, f"{VARIANTS[i]}: step-0 logits only {diff:.3f} from the base model's"
        assert runs[i][0] != base_runs[i][0], f"{VARIANTS[i]}: its ids never leave the base model's"
    long_base = greedy(models[None], long_prompt, 1)
    assert float(np.abs(long_run[1][0] - long_base[1][0]).max()) > MARGIN

    import transformers

    meta = {"seed": seed, "config": cfg.to_dict(), "prompts": prompts, "adapters": list(VARIANTS), "max_new": NEW_TOKENS,
            "long_prompt": long_prompt, "long_adapter": "all", "long_new": LONG_TOKENS, "min_margin": margin,
            "margin_bound": MARGIN, "step0_moved_by": moved, "transformers": transformers.__version__,
            "torch": torch.__version__}
    np.savez_compressed(os.path.join(HERE, "llama_lora.npz"),
                        meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8),
                        ids=np.array([r[0] for r in runs], dtype=np.int64),
                        logits=np.stack([r[1] for r in runs]).astype(np.float32),
                        base_ids=np.array([r[0] for r in base_runs], dtype=np.int64),
                        base_logits=np.stack([r[1] for r in base_runs]).astype(np.float32),
                        long_ids=np.array(long_run[0], dtype=np.int64), long_logits=long_run[1].astype(np.float32))
    print("wrote llama_lora.npz:", meta["seed"], meta["min_margin"], moved)


if __name__ == "__main__":
    main()
