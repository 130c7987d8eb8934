"""Per-request LoRA adapters on the Llama flash path, the host side: the options, reading and checking a peft
adapter directory, the slot table (adapter id -> device slot, least recently used replacement, a pin count per slot for live
requests) and the wrapper that adds an adapter's delta behind whatever `Linear` it is given.  The kernels are tgis_lora_group
/ tgis_lora_shrink / tgis_lora_expand (csrc/lora.hip).  Everything up to `LoraLinear` needs no GPU.

A request names an adapter with its `prefix_id`: a directory under $PREFIX_STORE_PATH whose `adapter_config.json` says
`"peft_type": "LORA"` (prompt_cache.py).  Tensors are peft's:
`base_model.model.model.layers.{i}.{self_attn.{q,k,v,o}_proj | mlp.{gate,up,down}_proj}.lora_{A,B}.weight`, A [r, in] and
B [out, r]; the scale is lora_alpha / r."""
import json
import re
import threading
from collections import OrderedDict
from dataclasses import dataclass
from pathlib import Path
from typing import Callable, Dict, List, Optional, Tuple

import torch

from tgis_amd.utils.spec_decode import _parse_int

MAX_LORA_SLOTS = 32
MAX_LORA_RANK = 64
ATTN_MODULES = ("q_proj", "k_proj", "v_proj", "o_proj")
MLP_MODULES = ("gate_proj", "up_proj", "down_proj")
LORA_MODULES = ATTN_MODULES + MLP_MODULES
# (attention modules under self_attn, MLP modules under mlp: a misnamed tensor is refused, not mapped to its namesake)
_KEY = re.compile(r"base_model\.model\.model\.layers\.(\d+)\.(?:self_attn\.([qkvo]_proj)|mlp\.((?:gate|up|down)_proj))"
                  r"\.lora_([AB])\.weight")


# ---- options --------------------------------------------------------------------------------------------------------------
def parse_lora_slots(value=None) -> int:
    """S, the adapters resident on the device at once: the argument, else TGIS_LORA_SLOTS; 0 or unset = off, 1 .. 32."""
    return _parse_int(value, "TGIS_LORA_SLOTS", 0, 0, MAX_LORA_SLOTS, "lora_slots (TGIS_LORA_SLOTS)")


def parse_lora_max_rank(value=None) -> int:
    """R, the largest adapter rank a slot holds: the argument, else TGIS_LORA_MAX_RANK; default 64, a multiple of 16."""
    what = "lora_max_rank (TGIS_LORA_MAX_RANK)"
    n = _parse_int(value, "TGIS_LORA_MAX_RANK", MAX_LORA_RANK, 16, MAX_LORA_RANK, what)
    if n % 16:
        raise ValueError(f"{what} must be a multiple of 16, got {n}")
    return n


def check_lora_world(lora_slots: int, tp_world: int, spec_tokens: int) -> None:
    if lora_slots > 0 and tp_world > 1:
        raise NotImplementedError(
            f"lora_slots={lora_slots} with {tp_world} tensor-parallel ranks: adapters under tensor parallelism are out of "
            "scope (DESIGN.md §8); run on one rank or set lora_slots=0")
    if lora_slots > 0 and spec_tokens > 0:
        raise NotImplementedError(
            f"lora_slots={lora_slots} with spec_tokens={spec_tokens}: speculative decoding together with adapters is out of "
            "scope (DESIGN.md §8); set one of them to 0")


def check_lora_model(lora_slots: int, model) -> None:
    """Adapters are served by the Llama model class alone, for the model types llama and mistral: not for qwen2 / qwen3, which
    it serves too."""
    model_type = getattr(getattr(model, "config", None), "model_type", None)
    if lora_slots > 0 and model_type in ("qwen2", "qwen3"):
        raise NotImplementedError(
            f"lora_slots={lora_slots}: LoRA adapters are not served for model type {model_type}: the adapter forward "
            "(forward_lora) does not carry its q/k/v bias split and q / k norm (DESIGN.md §8); set lora_slots=0")
    if lora_slots > 0 and not hasattr(model, "enable_lora"):
        raise NotImplementedError(
            f"lora_slots={lora_slots}: {type(model).__name__} does not serve LoRA adapters, only the Llama class (llama, "
            "mistral) does (DESIGN.md §8); set lora_slots=0")


# ---- adapters -------------------------------------------------------------------------------------------------------------
class LoraError(ValueError):
    pass


class LoraSlotsBusy(LoraError):
    pass


def module_shapes(config) -> Dict[str, Tuple[int, int]]:
    """(out, in) of the seven base projections of a Llama config."""
    E, H = config.hidden_size, config.num_attention_heads
    Hkv = getattr(config, "num_key_value_heads", None) or H
    D = getattr(config, "head_dim", None) or E // H
    inter = config.intermediate_size
    return {"q_proj": (H * D, E), "k_proj": (Hkv * D, E), "v_proj": (Hkv * D, E), "o_proj": (E, H * D),
            "gate_proj": (inter, E), "up_proj": (inter, E), "down_proj": (E, inter)}


def read_adapter_config(directory: Path) -> Optional[dict]:
    """The directory's adapter_config.json if it names a LoRA adapter, else None (a prompt-tuning adapter, no config)."""
    path = Path(directory) / "adapter_config.json"
    if not path.is_file():
        return None
    with open(path) as fh:
        cfg = json.load(fh)
    if not isinstance(cfg, dict) or str(cfg.get("peft_type", "")).upper() != "LORA":
        return None
    return cfg


def check_adapter_config(prefix_id: str, cfg: dict, max_rank: int) -> Tuple[int, float]:
    """(r, alpha / r) of a config this engine serves; every variant it does not is refused by name."""
    def refuse(what):
        raise LoraError(f"LoRA adapter {prefix_id}: {what} is not supported")

    if cfg.get("use_rslora"):
        refuse("use_rslora")
    if cfg.get("use_dora"):
        refuse("use_dora")
    if cfg.get("bias", "none") not in ("none", None):
        refuse(f"bias={cfg['bias']!r}")
    for name in ("modules_to_save", "rank_pattern", "alpha_pattern"):
        if cfg.get(name):
            refuse(f"a non-empty {name}")
    if cfg.get("fan_in_fan_out"):
        refuse("fan_in_fan_out")
    targets = cfg.get("target_modules") or []
    if isinstance(targets, str):
        refuse(f"target_modules given as the pattern {targets!r}")
    outside = sorted(t for t in targets if t.split(".")[-1] not in LORA_MODULES)
    if outside:
        refuse(f"target modules {outside} (served: {', '.join(LORA_MODULES)})")
    r = cfg.get("r")
    if isinstance(r, bool) or not isinstance(r, int) or r < 1:
        raise LoraError(f"LoRA adapter {prefix_id}: r must be a positive integer, got {r!r}")
    if r > max_rank:
        raise LoraError(f"LoRA adapter {prefix_id}: r={r} is above lora_max_rank (TGIS_LORA_MAX_RANK) = {max_rank}")
    alpha = cfg.get("lora_alpha", r)
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not alpha == alpha or abs(alpha) == float("inf"):
        raise LoraError(f"LoRA adapter {prefix_id}: lora_alpha must be a finite number, got {alpha!r}")
    return r, float(alpha) / r


class LoraAdapter:
    """A checked adapter on the CPU in the model dtype: `tensors[(layer, module)] = (A [r, in], B [out, r])`.  The slot table
    drops the tensors once they are on the device."""

    def __init__(self, prefix_id: str, r: int, scale: float, tensors):
        self.prefix_id, self.r, self.scale, self.tensors = prefix_id, r, scale, tensors
        self.modules = sorted({m for _, m in tensors}, key=LORA_MODULES.index)

    def pair(self, layer: int, module: str):
        return self.tensors.get((layer, module), (None, None))


def build_adapter(prefix_id: str, cfg: dict, data: dict, shapes: Dict[str, Tuple[int, int]], num_layers: int, max_rank: int,
                  dtype: torch.dtype) -> LoraAdapter:
    """Checks config and tensors against the base model (`shapes`: module_shapes) before anything reaches the device."""
    r, scale = check_adapter_config(prefix_id, cfg, max_rank)
    halves: Dict[Tuple[int, str], dict] = {}
    for name, t in data.items():
        m = _KEY.fullmatch(name)
        if m is None:
            if ".lora_" in name:
                raise LoraError(f"LoRA adapter {prefix_id}: tensor {name} is outside the served target modules "
                                f"({', '.join(LORA_MODULES)} of model.layers)")
            raise LoraError(f"LoRA adapter {prefix_id}: unexpected tensor {name}")
        layer, module, half = int(m.group(1)), m.group(2) or m.group(3), m.group(4)
        if layer >= num_layers:
            raise LoraError(f"LoRA adapter {prefix_id}: tensor {name} names layer {layer}, the base model has {num_layers}")
        out_f, in_f = shapes[module]
        want = (r, in_f) if half == "A" else (out_f, r)
        if not torch.is_tensor(t) or tuple(t.shape) != want:
            got = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
            raise LoraError(f"LoRA adapter {prefix_id}: {name} has shape {got}, the base model needs {want}")
        cast = t.to(dtype)
        if not cast.isfinite().all():
            if not t.isfinite().all():
                raise LoraError(f"LoRA adapter {prefix_id}: {name} contains non-finite elements")
            raise LoraError(f"LoRA adapter {prefix_id}: {name} contains non-finite elements after conversion from {t.dtype} "
                            f"to {dtype}")
        halves.setdefault((layer, module), {})[half] = cast.contiguous()
    if not halves:
        raise LoraError(f"LoRA adapter {prefix_id}: no lora_A / lora_B tensors found")
    tensors = {}
    for (layer, module), h in halves.items():
        if len(h) != 2:
            raise LoraError(f"LoRA adapter {prefix_id}: layers.{layer}.{module} has lora_{'A' if 'A' in h else 'B'} without "
                            "its other half")
        tensors[(layer, module)] = (h["A"], h["B"])
    return LoraAdapter(prefix_id, r, scale, tensors)


# ---- slots ----------------------------------------------------------------------------------------------------------------
class LoraSlots:
    """Adapter ids -> the S device slots.  `acquire` pins a slot for a live request (loading the adapter into a free slot, or
    over the least recently used unpinned one, through `upload(slot, adapter)`); `release` unpins.  A pinned slot is never
    replaced: with every slot pinned `acquire` raises LoraSlotsBusy."""

    def __init__(self, S: int, max_rank: int, shapes: Dict[str, Tuple[int, int]], num_layers: int, dtype: torch.dtype,
                 upload: Optional[Callable[[int, LoraAdapter], None]] = None):
        self.S, self.max_rank, self.shapes, self.num_layers, self.dtype = S, max_rank, shapes, num_layers, dtype
        self.upload = upload
        self.pins = [0] * S
        self.ids: List[Optional[str]] = [None] * S
        self.adapters: List[Optional[LoraAdapter]] = [None] * S
        self._order: "OrderedDict[str, int]" = OrderedDict()  # id -> slot, least recently used first
        self._lock = threading.Lock()
        self.loads = 0

    def build(self, prefix_id: str, cfg: dict, data: dict) -> LoraAdapter:
        return build_adapter(prefix_id, cfg, data, self.shapes, self.num_layers, self.max_rank, self.dtype)

    def resident(self, prefix_id: str) -> Optional[LoraAdapter]:
        """The adapter's record if a slot holds it (its tensors are on the device, not here)."""
        with self._lock:
            s = self._order.get(prefix_id)
            return None if s is None else self.adapters[s]

    def slot_of(self, prefix_id: str) -> Optional[int]:
        return self._order.get(prefix_id)

    def acquire(self, adapter: LoraAdapter) -> int:
        with self._lock:
            s = self._order.get(adapter.prefix_id)
            if s is None:
                free = [i for i in range(self.S) if self.ids[i] is None]
                if free:
                    s = free[0]
                else:
                    s = next((i for i in self._order.values() if self.pins[i] == 0), None)
                    if s is None:
                        raise LoraSlotsBusy(
                            f"LoRA adapter {adapter.prefix_id}: all {self.S} adapter slots (lora_slots / TGIS_LORA_SLOTS) are "
                            "pinned by live requests")
                    del self._order[self.ids[s]]
                    self.ids[s] = self.adapters[s] = None
                if adapter.tensors is None:
                    raise LoraError(f"LoRA adapter {adapter.prefix_id}: its tensors were dropped, look it up again")
                if self.upload is not None:
                    self.upload(s, adapter)
                self.loads += 1
                self.ids[s] = adapter.prefix_id
                self.adapters[s] = LoraAdapter(adapter.prefix_id, adapter.r, adapter.scale, {})
                self.adapters[s].modules, self.adapters[s].tensors = adapter.modules, None
            self._order[adapter.prefix_id] = s
            self._order.move_to_end(adapter.prefix_id)
            self.pins[s] += 1
            return s

    def release(self, s: int) -> None:
        if s is None or s < 0:
            return
        with self._lock:
            assert self.pins[s] > 0, f"LoRA slot {s} is not pinned"
            self.pins[s] -= 1


def release_slots(table: Optional[LoraSlots], slots: Optional[List[int]]) -> None:
    if table is not None and slots:
        for s in slots:
            table.release(s)


# ---- the forward ----------------------------------------------------------------------------------------------------------
@dataclass
class LoraArgs:
    """What a forward that carries adapter rows hands the layers: `slots` int32 [T] on the device (-1: no adapter) and
    either `groups`, the device grouping of tgis_lora_group for every run of up to 64 rows as (row0, row1, LoraGroup) (the
    kernel path: prefills of up to 64 rows and every decode step), or, for longer prefills, the host's `ranges` (row0,
    row1, slot) of the requests that carry an adapter (their rows are contiguous)."""
    slots: torch.Tensor
    groups: Optional[List[Tuple[int, int, object]]] = None
    ranges: Optional[List[Tuple[int, int, int]]] = None

    @classmethod
    def grouped(cls, slots: torch.Tensor, S: int) -> "LoraArgs":
        """The kernel path over `slots`: one tgis_lora_group per 64 rows, nothing read on the host."""
        from tgis_amd import native

        T, step = slots.numel(), native.LORA_MAX_T
        return cls(slots, groups=[(r0, min(r0 + step, T), native.lora_group(slots[r0:min(r0 + step, T)], S))
                                  for r0 in range(0, T, step)])


class LoraLinear:
    """A projection in its tensor-parallel role (`layer`, a SuperLayer of utils/layers.py) plus the slot images of the
    adapters' deltas for it.  Everything the layer offers passes through; `forward_lora` is the plain GEMM followed by the
    delta, in place.  `modules`: the adapter modules fused into this linear, in column order, with `bounds` their P + 1
    column bounds."""

    def __init__(self, layer, layer_id: int, modules, bounds, K: int, S: int, max_rank: int, dtype, device):
        from tgis_amd import native

        self.layer, self.linear = layer, layer.linear
        self.layer_id, self.modules = layer_id, tuple(modules)
        self.images = native.LoraImages(K, bounds, S, max_rank, dtype, device)

    def __getattr__(self, name):  # (only what is not found on the wrapper itself)
        return getattr(self.layer, name)

    def forward(self, x, **kw):
        return self.layer.forward(x, **kw)

    __call__ = forward

    def load(self, s: int, adapter: LoraAdapter) -> None:
        pairs = [adapter.pair(self.layer_id, m) for m in self.modules]
        self.images.load(s, [a for a, _ in pairs], [b for _, b in pairs], adapter.scale)

    def forward_lora(self, x, lora: LoraArgs):
        y = self.layer.forward(x)
        return self.add_delta(x, y, lora)

    def add_delta(self, x, y, lora: LoraArgs):
        from tgis_amd import native

        w = self.images
        if lora.groups is not None:
            for row0, row1, g in lora.groups:
                native.lora_expand(native.lora_shrink(x[row0:row1], w, g), w, g, y[row0:row1])
            return y
        # long prefills: two library GEMMs per projection the adapter targets and row range, in fp32 as the kernels' contract
        # has it (v stays fp32, base + delta is rounded to the model dtype once)
        for row0, row1, s in lora.ranges:
            rank = w.host_ranks[s]
            if rank == 0:
                continue
            r16 = (rank + 15) // 16 * 16
            xs = x[row0:row1].float()
            b = w.B[s, :r16 // 16].permute(1, 0, 2).reshape(w.N, r16).float()
            for p in range(w.P):
                if not w.host_present[s][p]:
                    continue  # (the adapter leaves this projection out: its A and B are zero)
                v = torch.matmul(xs, w.A[s, p, :r16].float().t())
                n0, n1 = w.bounds[p], w.bounds[p + 1]
                ys = y[row0:row1, n0:n1]
                ys.copy_(torch.addmm(ys.float(), v, b[n0:n1].t(), alpha=w.host_scales[s]))
        return y
