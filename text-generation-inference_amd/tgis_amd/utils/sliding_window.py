"""Sliding-window attention on the host side: reading `config.sliding_window` (Mistral) and refusing the options that do not
serve a window yet.  Pure functions, no GPU: tests/test_mistral_cpu.py calls them.

The kernels are native.attn_paged(window=...) (tgis_attn_paged_window); models/custom_modeling/flash_common.py `attend` passes
the window on, FlashCausalLM sets it on the KVArgs of the fresh prefill and of the decode graphs."""
from typing import Optional


USE_FLAG_TYPES = ("qwen2", "qwen3")


def use_sliding_window(config) -> bool:
    """Whether `config.sliding_window` is to be read at all.  Qwen2 / Qwen3 configs carry `sliding_window` next to
    `use_sliding_window: false`: for these two model types the window counts only when the flag is true, and then the model is
    refused, because it windows some layers and not others (`max_window_layers` / `layer_types`), which no launch here does
    (DESIGN.md section 8).  Every other model type: true."""
    if getattr(config, "model_type", None) not in USE_FLAG_TYPES:
        return True
    if not getattr(config, "use_sliding_window", False):
        return False
    raise NotImplementedError(
        f"{config.model_type} with use_sliding_window = true is not served: its `layer_types` / `max_window_layers` window "
        "some layers and not others, and per-layer windows are out of scope (DESIGN.md section 8); serve the checkpoint with "
        "use_sliding_window = false")


def parse_sliding_window(config) -> Optional[int]:
    """W keys per q row, or None: `sliding_window` absent, null or 0 is off, and so is one that `use_sliding_window` says is
    not in use."""
    if not use_sliding_window(config):
        return None
    w = getattr(config, "sliding_window", None)
    if w is None or w == 0:
        return None
    if not isinstance(w, int) or isinstance(w, bool) or w < 1:
        raise ValueError(f"sliding_window must be a positive integer or null, got {w!r}")
    return w


def window_in_reach(window: Optional[int], config) -> bool:
    """Whether a request within the model's position limit can ever reach the window."""
    limit = getattr(config, "max_position_embeddings", None)
    return window is not None and (limit is None or window < limit)


def check_window_options(window: Optional[int], config, spec_tokens: int = 0, kv_prefix_reuse: bool = False,
                         calibrate_kv_scales: bool = False):
    """A window below the model's position limit is not served together with speculative decoding (its verify steps are the
    causal or tree launches), KV prefix reuse (its suffix prefill is the causal launch with key splits) or
    calibrate_kv_scales (it scans positions the model no longer reads)."""
    if not window_in_reach(window, config):
        return
    for on, option in ((spec_tokens > 0, f"spec_tokens = {spec_tokens}"), (bool(kv_prefix_reuse), "kv_prefix_reuse"),
                       (calibrate_kv_scales, "calibrate_kv_scales")):
        if on:
            raise NotImplementedError(f"sliding_window = {window} and {option} are not served together: a checkpoint with a "
                                      f"sliding window below its position limit runs without {option.split(' ')[0]}")
