#!/usr/bin/env python
"""Golden fixtures for the GPT-NeoX flash path: the REFERENCE's CPU `causal_lm` (hf_transformers engine, fp32) on the
seeded tiny checkpoints of tests/neox_tiny.py.  Same shims, margin rule and file format as make_fixtures.py, which is
imported, not edited.  Needs the reference checkout; only the .npz outputs are committed.

    python tests/golden/make_neox_fixtures.py

Writes neox_equal.npz (variant A: head size 96, partial rotary 24, parallel residual), neox_ragged.npz (variant B: head
size 64, rotary 16, sequential residual) and neox_continuous.npz (variant A: prefill, decode, concatenate, prune)."""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_fixtures import decisive, install_shims, make_requests, run_reference, save, step  # noqa: E402
from neox_tiny import TinyNeoXConfig, tiny_neox_tensors  # noqa: E402

NEOX_MARGIN = 0.8
SEED = 11


def write_neox_dir(path, cfg, tensors):
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import GPTNeoXConfig, GPTNeoXForCausalLM, PreTrainedTokenizerFast

    vocab = {"<pad>": 0, "<s>": 1, "</s>": 2}
    for i in range(3, cfg.vocab_size):
        vocab[f"t{i}"] = i
    tk = Tokenizer(models.WordLevel(vocab, unk_token="<pad>"))
    tk.pre_tokenizer = pre_tokenizers.Whitespace()
    PreTrainedTokenizerFast(tokenizer_object=tk, eos_token="</s>", bos_token="<s>", unk_token="<pad>",
                            pad_token="<pad>").save_pretrained(path)
    model = GPTNeoXForCausalLM(GPTNeoXConfig(**cfg.hf_kwargs()))
    if hasattr(model, "lm_head"):  # transformers 5.x names the checkpoint's embed_out `lm_head`
        tensors = {("lm_head.weight" if k == "embed_out.weight" else k): v for k, v in tensors.items()}
    missing, unexpected = model.load_state_dict(tensors, strict=False)
    assert not unexpected and all("rotary" in m or "inv_freq" in m or "masked_bias" in m or ".attention.bias" in m
                                  for m in missing), (missing, unexpected)
    model.float().save_pretrained(path, safe_serialization=True)


def main():
    tmp = tempfile.mkdtemp(prefix="tgis_neox_fixture_")
    install_shims(tmp)
    from text_generation_server.models import get_model
    from text_generation_server.pb import generate_pb2 as pb2

    rng = np.random.default_rng(2025)
    models = {}
    for variant in ("A", "B"):
        cfg = TinyNeoXConfig(variant)
        mdir = os.path.join(tmp, f"neox_{variant}")
        os.makedirs(mdir)
        write_neox_dir(mdir, cfg, tiny_neox_tensors(cfg, seed=SEED))
        models[variant] = (cfg, get_model(mdir, None, "hf_transformers", "float32", None, 256))

    def meta(cfg):
        return {"variant": cfg.variant, "seed": SEED, "config": cfg.to_dict(),
                "transformers": __import__("transformers").__version__, "torch": torch.__version__}

    cfg, model = models["A"]

    def equal():
        prompts = [rng.integers(3, cfg.vocab_size, size=12).tolist() for _ in range(3)]
        batch = run_reference(model, make_requests(pb2, prompts, max_new=6))
        return {"prompts": prompts}, [step(model, batch, first=True)] + [step(model, batch) for _ in range(5)]

    extra, steps = decisive(equal, "neox_equal", NEOX_MARGIN)
    save("neox_equal", {**meta(cfg), **extra, "max_new": 6}, steps)

    def continuous():
        pa = [rng.integers(3, cfg.vocab_size, size=n).tolist() for n in (9, 14)]
        pb_ = [rng.integers(3, cfg.vocab_size, size=n).tolist() for n in (6,)]
        a = run_reference(model, make_requests(pb2, pa, max_new=10, first_id=0, batch_id=1))
        steps = [step(model, a, first=True), step(model, a)]
        b = run_reference(model, make_requests(pb2, pb_, max_new=10, first_id=2, batch_id=2))
        steps.append(step(model, b, first=True, for_concat=True))
        with model.context_manager():
            merged = model.batch_type.concatenate([a, b])
        steps += [step(model, merged)]
        with model.context_manager():
            merged = model.batch_type.prune(merged, [0])
        steps += [step(model, merged)]
        return {"prompts_a": pa, "prompts_b": pb_}, steps

    extra, steps = decisive(continuous, "neox_continuous", NEOX_MARGIN)
    save("neox_continuous", {**meta(cfg), **extra, "max_new": 10,
                             "script": ["prefill A(ids 0,1)", "decode A", "prefill B(id 2, for_concat)",
                                        "concatenate[A,B] + decode", "prune id 0 + decode"]}, steps)

    cfg, model = models["B"]

    def ragged():
        prompts = [rng.integers(3, cfg.vocab_size, size=n).tolist() for n in (5, 33, 17, 1)]
        batch = run_reference(model, make_requests(pb2, prompts, max_new=5))
        return {"prompts": prompts}, [step(model, batch, first=True)] + [step(model, batch) for _ in range(4)]

    extra, steps = decisive(ragged, "neox_ragged", NEOX_MARGIN)
    save("neox_ragged", {**meta(cfg), **extra, "max_new": 5}, steps)


if __name__ == "__main__":
    main()
