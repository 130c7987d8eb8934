#!/usr/bin/env python
"""Golden fixture of the Mixtral flash path: transformers' MixtralForCausalLM, fp32 on the CPU, on the seeded tiny checkpoint
of tests/mixtral_tiny.py (the reference project has no Mixtral; transformers' routing semantics are the arbiter).  Only outputs
are written; the tests rebuild the weights from the seed.

    python tests/golden/make_mixtral_fixtures.py [first seed]      (the committed file: seed 1301, found from 0)

Writes tests/golden/mixtral_top2.npz: prompts of 5, 20 and 33 tokens, NEW_TOKENS = 5 greedy tokens each: ids [3, 5], logits
[3, 5, vocab] (the logits each token was chosen from), per prompt the router's top-2 expert indices of every layer and token
of the last forward (router_idx_0..2: [layers, tokens, 2]) and meta.  Every step is a full forward over the sequence so far
(use_cache=False, output_router_logits=True), so nothing depends on a cache implementation.

The seed is the first at which both hold:
  * every top-2 logit margin exceeds MARGIN = 0.7, twice the f16 logit bound of the GPU tests: exact ids are a fair demand;
  * at every layer and token the gap between the 2nd and the 3rd largest router logit exceeds ROUTER_MARGIN: a 16-bit run
    then routes every token as the fp32 run does.  ROUTER_MARGIN is measured, not chosen: the same weights run on the CPU in
    float16, the largest deviation of any router logit from the fp32 run is taken, and the bound is ROUTER_FACTOR = 8 times
    that (the kernels sum in another order than the CPU's half GEMM).
With 12 greedy tokens (182 routed events) no seed below MAX_TRIES = 2000 meets both: a float16 run moves router logits by
about 2.5e-3, so ROUTER_MARGIN is about 0.02, and the smallest of 182 gaps is typically 1e-3.  The generation was shortened,
not the factor: 5 tokens (140 events: the prompts' 58 tokens and 12 decoded ones that are fed back, two layers) is the longest generation for
which a seed below 2000 exists.
The generator asserts that routing matters: the same weights with every token sent to experts 0 and 1 (their router weights
renormalised) leave the fixture's logits by more than MARGIN / 2."""
import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from mixtral_tiny import TinyMixtralConfig, fused_names, tiny_mixtral_tensors  # noqa: E402

MARGIN = 0.7
ROUTER_FACTOR = 8.0
PROMPT_LENS = (5, 20, 33)
NEW_TOKENS = 5  # (12 at first: see the docstring)
MAX_TRIES = 2000


def hf_model(cfg, seed):
    from transformers import MixtralConfig, MixtralForCausalLM

    model = MixtralForCausalLM(MixtralConfig(**cfg.to_dict(), attn_implementation="eager"))
    state = {k: v.float() for k, v in fused_names(tiny_mixtral_tensors(cfg, seed), cfg).items()}
    missing, unexpected = model.load_state_dict(state, strict=False)
    assert not unexpected and all("rotary" in m or "inv_freq" in m for m in missing), (missing, unexpected)
    return model.float().eval()


@torch.no_grad()
def forward(model, ids):
    """(logits [tokens, vocab], router logits [layers, tokens, E]) of one full forward, as fp32."""
    out = model(input_ids=torch.tensor([ids]), use_cache=False, output_router_logits=True)
    return out.logits[0].float(), torch.stack([r.float().reshape(len(ids), -1) for r in out.router_logits])


def greedy(model, prompt):
    ids, out_ids, out_logits, margin = list(prompt), [], [], float("inf")
    for _ in range(NEW_TOKENS):
        logits, router = forward(model, ids)
        row = logits[-1]
        top = torch.topk(row, 2).values
        margin = min(margin, float(top[0] - top[1]))
        if margin <= MARGIN:
            return None
        out_ids.append(int(row.argmax()))
        out_logits.append(row.numpy())
        ids.append(out_ids[-1])
    return out_ids, np.stack(out_logits), margin, ids[:-1], router


def force_experts_0_1():
    """MixtralTopKRouter.forward with every token sent to experts 0 and 1, their softmax weights renormalised."""
    from transformers.models.mixtral import modeling_mixtral as mm

    def forced(self, hidden_states):
        hidden_states = hidden_states.reshape(-1, self.hidden_dim)
        router_logits = torch.nn.functional.linear(hidden_states, self.weight)
        probs = torch.softmax(router_logits.float(), dim=-1)[:, :2]
        idx = torch.tensor([0, 1]).expand(probs.shape[0], 2)
        return router_logits, probs / probs.sum(dim=-1, keepdim=True), idx

    original = mm.MixtralTopKRouter.forward
    mm.MixtralTopKRouter.forward = forced
    return lambda: setattr(mm.MixtralTopKRouter, "forward", original)


def main():
    first = seed = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    rng = np.random.default_rng(2027)
    prompts = [rng.integers(3, 256, size=n).tolist() for n in PROMPT_LENS]
    cfg = TinyMixtralConfig()
    while True:
        assert seed - first < MAX_TRIES, "no seed found: shorten the generation, do not lower ROUTER_FACTOR"
        model = hf_model(cfg, seed)
        runs = []
        for p in prompts:
            r = greedy(model, p)
            if r is None:
                break
            runs.append(r)
        if len(runs) < len(prompts):
            print(f"seed {seed}: a top-2 logit margin is below {MARGIN}", flush=True)
            seed += 1
            continue
        margin = min(r[2] for r in runs)
        # the float16 run of the same weights over the sequences of the last forwards: how far its router logits move
        half = copy.deepcopy(model).half()
        dev = max(float((forward(half, r[3])[1] - r[4]).abs().max()) for r in runs)
        router_margin = ROUTER_FACTOR * dev
        top3 = [torch.topk(r[4], 3, dim=-1).values for r in runs]
        gap = min(float((t[..., 1] - t[..., 2]).min()) for t in top3)
        events = sum(t.shape[0] * t.shape[1] for t in top3)
        print(f"seed {seed}: top-2 logit margin {margin:.3f}; f16 router deviation {dev:.5f} -> ROUTER_MARGIN "
              f"{router_margin:.5f}; smallest 2nd-3rd router gap {gap:.5f} over {events} events", flush=True)
        if gap > router_margin:
            break
        seed += 1
    # routing matters: everything through experts 0 and 1 is another model
    restore = force_experts_0_1()
    try:
        moved = min(float((forward(model, r[3])[0][-1] - torch.from_numpy(r[1][-1])).abs().max()) for r in runs)
    finally:
        restore()
    assert moved > MARGIN / 2, moved
    assert float((forward(model, runs[0][3])[0][-1] - torch.from_numpy(runs[0][1][-1])).abs().max()) < 1e-5

    import transformers

    meta = {"seed": seed, "config": cfg.to_dict(), "prompts": prompts, "max_new": NEW_TOKENS, "min_margin": margin,
            "margin_bound": MARGIN, "router_margin": router_margin, "router_factor": ROUTER_FACTOR,
            "f16_router_deviation": dev, "min_router_gap": gap, "router_events": events, "forced_experts_move": moved,
            "transformers": transformers.__version__, "torch": torch.__version__}
    arrays = {f"router_idx_{i}": torch.topk(r[4], 2, dim=-1).indices.numpy().astype(np.int32) for i, r in enumerate(runs)}
    np.savez_compressed(os.path.join(HERE, "mixtral_top2.npz"),
                        meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8),
                        ids=np.array([r[0] for r in runs], dtype=np.int64),
                        logits=np.stack([r[1] for r in runs]).astype(np.float32), **arrays)
    print("wrote mixtral_top2.npz:", json.dumps({k: meta[k] for k in ("seed", "min_margin", "router_margin", "min_router_gap")}))


if __name__ == "__main__":
    main()
