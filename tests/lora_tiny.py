"""The seeded tiny Llama of the LoRA tests and its three seeded adapters.  TEST INFRASTRUCTURE: needs no GPU.

The base is oracle/tiny_models.py's tiny Llama (hidden 256, 4 heads on 2 kv heads, 2 layers, I 512, vocab 256, weights rounded
to f16).  The adapters are a pure function of (config, seed) too, in peft's tensor names and rounded to f16, so the fixture
maker (tests/golden/make_llama_lora_fixtures.py: transformers' fp32 CPU LlamaForCausalLM on MERGED weights W + (alpha / r) B A)
and the tests rebuild identical weights; only outputs are committed.

  qv    r 8 on q_proj and v_proj
  all   r 16 on all seven modules
  od    r 4 on o_proj and down_proj only (a rank below the kernels' granule of 16)

B is scaled (`gain`) so that each adapter moves the logits well past the tests' tolerance; the maker asserts that it does."""
import json
import os
from typing import Dict, Optional

import torch

from oracle.tiny_models import TinyLlamaConfig, dense_state_dict, tiny_llama_tensors  # noqa: F401

ATTN = ("q_proj", "k_proj", "v_proj", "o_proj")
ALL_MODULES = ATTN + ("gate_proj", "up_proj", "down_proj")
ADAPTERS = {
    "qv": dict(r=8, alpha=16, modules=("q_proj", "v_proj"), gain=0.5),
    "all": dict(r=16, alpha=32, modules=ALL_MODULES, gain=0.3),
    "od": dict(r=4, alpha=8, modules=("o_proj", "down_proj"), gain=0.6),
}
ADAPTER_NAMES = ("qv", "all", "od")
GROUPSIZE = 64  # of the GPTQ variant of the base (the tiny GPTQ Llama of the existing fixtures)


def module_shapes(cfg):
    E, I = cfg.hidden_size, cfg.intermediate_size
    D = E // cfg.num_attention_heads
    kvw = cfg.num_key_value_heads * D
    return {"q_proj": (E, E), "k_proj": (kvw, E), "v_proj": (kvw, E), "o_proj": (E, E), "gate_proj": (I, E), "up_proj": (I, E),
            "down_proj": (E, I)}


def module_path(layer: int, module: str) -> str:
    return f"model.layers.{layer}.{'self_attn' if module in ATTN else 'mlp'}.{module}"


def adapter_tensors(cfg, name: str, seed: int) -> Dict[str, torch.Tensor]:
    """peft name -> f16 tensor: lora_A [r, in] of standard deviation in^-1/2, lora_B [out, r] of gain r^-1/2."""
    spec = ADAPTERS[name]
    g = torch.Generator().manual_seed(100003 * (ADAPTER_NAMES.index(name) + 1) + seed)
    shapes, r = module_shapes(cfg), spec["r"]
    t = {}
    for layer in range(cfg.num_hidden_layers):
        for module in spec["modules"]:
            out_f, in_f = shapes[module]
            base = f"base_model.model.{module_path(layer, module)}"
            t[f"{base}.lora_A.weight"] = (torch.randn(r, in_f, generator=g) * in_f ** -0.5).half()
            t[f"{base}.lora_B.weight"] = (torch.randn(out_f, r, generator=g) * spec["gain"] * r ** -0.5).half()
    return t


def adapter_config(name: str, **overrides) -> dict:
    spec = ADAPTERS[name]
    cfg = {"peft_type": "LORA", "task_type": "CAUSAL_LM", "r": spec["r"], "lora_alpha": spec["alpha"],
           "target_modules": list(spec["modules"]), "bias": "none", "fan_in_fan_out": False, "use_rslora": False,
           "use_dora": False, "modules_to_save": None, "rank_pattern": {}, "alpha_pattern": {}, "lora_dropout": 0.0}
    cfg.update(overrides)
    return cfg


def write_adapter(directory, name: str, cfg, seed: int, fmt: str = "safetensors", tensors: Optional[dict] = None,
                  **config_overrides) -> None:
    """A peft adapter directory: adapter_config.json + adapter_model.safetensors (or .bin)."""
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, "adapter_config.json"), "w") as fh:
        json.dump(adapter_config(name, **config_overrides), fh)
    tensors = adapter_tensors(cfg, name, seed) if tensors is None else tensors
    if fmt == "safetensors":
        from safetensors.torch import save_file

        save_file({k: v.contiguous() for k, v in tensors.items()}, os.path.join(directory, "adapter_model.safetensors"))
    else:
        torch.save(tensors, os.path.join(directory, "adapter_model.bin"))


def merged_state_dict(cfg, base: Dict[str, torch.Tensor], name: Optional[str], seed: int) -> Dict[str, torch.Tensor]:
    """fp32 dense state dict of the base (`base`: dense f16 or GPTQ tensors of tiny_llama_tensors) with adapter `name` merged
    in: W + (alpha / r) B A; name None: the base itself."""
    sd = dense_state_dict(cfg, base, GROUPSIZE)
    if name is None:
        return sd
    spec, t = ADAPTERS[name], adapter_tensors(cfg, name, seed)
    for layer in range(cfg.num_hidden_layers):
        for module in spec["modules"]:
            path = module_path(layer, module)
            A = t[f"base_model.model.{path}.lora_A.weight"].float()
            B = t[f"base_model.model.{path}.lora_B.weight"].float()
            sd[f"{path}.weight"] = sd[f"{path}.weight"] + (spec["alpha"] / spec["r"]) * (B @ A)
    return sd
