"""The MLP speculator, the reference's drafter of speculative decoding (models/paged_causal_lm.py:481-562,
utils/paged.py:20-38,208 `SPECULATOR_NAME`): its checkpoint format, the options that turn it on, and the chain of launches
that drafts K tokens per request from the hidden state behind the request's latest token.

    x = h;  scale_input: x = x rsqrt(mean(x^2) + eps) / sqrt(2)
    head i = 0 .. K - 1:  s = proj_i x + alpha emb_i[t];  x = gelu_erf(rmsln_i(s));  t = argmax(head_i x);  draft[i] = t

Parsing a config, mapping the tensor names, resolving tied weights and every refusal need no GPU (`open_checkpoint`); only
`MLPSpeculator` puts weights on a device and launches kernels (csrc/spec_mlp.hip, the dense GEMM, the greedy argmax)."""
import json
import math
import os
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Tuple

import torch

from tgis_amd.utils.spec_decode import MAX_SPEC_TOKENS

EPS = 1e-6
MAX_INNER = 16384  # tgis_spec_mlp_state caches a row in registers

# The tensor names of the published format (ibm-fms/*-accelerator), one pattern per kind, {i} = the head; every name is
# accepted with each of PREFIXES in front.  Written from memory of that format: correct it HERE if a checkpoint differs.
TENSOR_NAMES = {
    "emb": "emb.{i}.weight",      # [V, I]
    "proj": "proj.{i}.weight",    # [I, E] for i = 0, [I, I] behind it
    "head": "head.{i}.weight",    # [V, I]
    "ln_weight": "ln.{i}.weight",  # [I]
    "ln_bias": "ln.{i}.bias",     # [I]
}
PREFIXES = ("", "speculator.")


@dataclass
class SpeculatorConfig:
    emb_dim: int
    inner_dim: int  # (0 in the file means emb_dim; resolved here)
    vocab_size: int
    n_predict: int
    tie_weights: bool = False
    scale_input: bool = False

    @classmethod
    def from_dict(cls, d: dict) -> "SpeculatorConfig":
        """`n_candidates` and `top_k_tokens_per_head` are read and ignored: one candidate, the top-1 chain, is drafted."""
        missing = [k for k in ("emb_dim", "vocab_size", "n_predict") if k not in d]
        if missing:
            raise ValueError(f"speculator config.json lacks {missing}")
        E, V, P = int(d["emb_dim"]), int(d["vocab_size"]), int(d["n_predict"])
        I = int(d.get("inner_dim", 0) or 0) or E
        if E <= 0 or I <= 0 or V <= 0 or P <= 0:
            raise ValueError(f"speculator config.json: emb_dim {E}, inner_dim {I}, vocab_size {V} and n_predict {P} must "
                             "be positive")
        return cls(E, I, V, P, bool(d.get("tie_weights", False)), bool(d.get("scale_input", False)))

    def shape_of(self, kind: str, i: int) -> Tuple[int, ...]:
        E, I, V = self.emb_dim, self.inner_dim, self.vocab_size
        return {"emb": (V, I), "head": (V, I), "proj": (I, E if i == 0 else I), "ln_weight": (I,), "ln_bias": (I,)}[kind]


def constants(n_predict: int, inner_dim: int) -> Tuple[float, float, float]:
    """(state_weight, emb_weight, alpha = emb_weight / state_weight) of a speculator with P heads of width I."""
    state_weight = 0.5 ** (0.5 / n_predict)
    emb_weight = math.sqrt((1.0 - state_weight ** 2) * inner_dim / 2.0)
    return state_weight, emb_weight, emb_weight / state_weight


def parse_speculator(value=None) -> Optional[str]:
    """The checkpoint directory of the MLP drafter: the argument, else TGIS_SPECULATOR; None / unset / empty = the lookup."""
    if value is None:
        value = os.getenv("TGIS_SPECULATOR")
    if value is None or str(value).strip() == "":
        return None
    if not isinstance(value, (str, os.PathLike)):
        raise ValueError(f"speculator (TGIS_SPECULATOR) must be a checkpoint directory, got {value!r}")
    return os.fspath(value).strip()


def check_spec_tokens(cfg: SpeculatorConfig, spec_tokens: int) -> None:
    hi = min(cfg.n_predict, MAX_SPEC_TOKENS)
    if spec_tokens < 1:
        raise ValueError(f"speculator is set but spec_tokens (TGIS_SPEC_TOKENS) is {spec_tokens}: an MLP drafter needs "
                         f"spec_tokens in 1 .. {hi}; unset speculator (TGIS_SPECULATOR) to run without speculation")
    if spec_tokens > hi:
        raise ValueError(f"spec_tokens (TGIS_SPEC_TOKENS) = {spec_tokens} but the speculator (TGIS_SPECULATOR) predicts "
                         f"n_predict = {cfg.n_predict} tokens: spec_tokens must be in 1 .. {hi}")


def check_shapes(cfg: SpeculatorConfig) -> None:
    """What the kernels cannot serve (they refuse it too, with a message of their own)."""
    if cfg.emb_dim % 8 or cfg.inner_dim % 8:
        raise ValueError(f"speculator: emb_dim {cfg.emb_dim} and inner_dim {cfg.inner_dim} must be multiples of 8")
    if cfg.inner_dim > MAX_INNER:
        raise ValueError(f"speculator: inner_dim {cfg.inner_dim} exceeds {MAX_INNER}")


def check_base(cfg: SpeculatorConfig, hidden_size: int, vocab_size: int) -> None:
    if cfg.emb_dim != hidden_size:
        raise ValueError(f"speculator emb_dim {cfg.emb_dim} != the base model's hidden size {hidden_size}")
    if cfg.vocab_size != vocab_size:
        raise ValueError(f"speculator vocab_size {cfg.vocab_size} != the base model's vocab_size {vocab_size}")


def _find(available, kind: str, i: int) -> Optional[str]:
    for prefix in PREFIXES:
        name = prefix + TENSOR_NAMES[kind].format(i=i)
        if name in available:
            return name
    return None


def resolve_names(available, cfg: SpeculatorConfig) -> List[Dict[str, str]]:
    """Per head, kind -> the checkpoint's tensor name.  With tie_weights index 0 of emb / head / ln serves every head and
    proj.1 every head i >= 1, whether the file stores the tied tensors once or repeats them: heads that share a tensor get
    the SAME name, so whoever loads by name aliases them."""
    available = set(available)
    heads, missing = [], []
    for i in range(cfg.n_predict):
        head = {}
        for kind in TENSOR_NAMES:
            j = i
            if cfg.tie_weights:
                j = min(i, 1) if kind == "proj" else 0
            name = _find(available, kind, j)
            if name is None:
                missing.append(TENSOR_NAMES[kind].format(i=j))
            head[kind] = name
        heads.append(head)
    if missing:
        raise ValueError(f"speculator checkpoint lacks {sorted(set(missing))} (each also looked for as 'speculator.<name>')")
    return heads


class SpeculatorCheckpoint:
    """A parsed and checked checkpoint: `cfg`, `names` (resolve_names) and `load(name)` -> the tensor on the CPU."""

    def __init__(self, cfg: SpeculatorConfig, shapes: Dict[str, Tuple[int, ...]], load: Callable[[str], torch.Tensor]):
        check_shapes(cfg)
        self.cfg, self.load = cfg, load
        self.names = resolve_names(shapes, cfg)
        for i, head in enumerate(self.names):
            for kind, name in head.items():
                if tuple(shapes[name]) != cfg.shape_of(kind, i):
                    raise ValueError(f"speculator tensor {name} has shape {tuple(shapes[name])}, head {i} needs "
                                     f"{cfg.shape_of(kind, i)}")


def open_checkpoint(path: str) -> SpeculatorCheckpoint:
    """Reads config.json and the safetensors headers of a checkpoint directory; no tensor is loaded yet."""
    from safetensors import safe_open

    cfg_path = os.path.join(path, "config.json")
    if not os.path.isfile(cfg_path):
        raise ValueError(f"speculator (TGIS_SPECULATOR): {cfg_path} not found")
    with open(cfg_path) as f:
        cfg = SpeculatorConfig.from_dict(json.load(f))
    files = sorted(os.path.join(path, n) for n in os.listdir(path) if n.endswith(".safetensors"))
    if not files:
        raise ValueError(f"speculator (TGIS_SPECULATOR): no .safetensors file in {path}")
    where, shapes = {}, {}
    for fn in files:
        with safe_open(fn, framework="pt") as f:
            for name in f.keys():
                where[name] = fn
                shapes[name] = tuple(f.get_slice(name).get_shape())

    def load(name: str) -> torch.Tensor:
        with safe_open(where[name], framework="pt") as f:
            return f.get_tensor(name)

    return SpeculatorCheckpoint(cfg, shapes, load)


def checked_checkpoint(speculator=None, spec_tokens: int = 0, base_config=None) -> Optional[SpeculatorCheckpoint]:
    """The model's `speculator` option as a checked checkpoint, or None for the lookup: a checkpoint directory, a
    SpeculatorCheckpoint made in memory (tools), or None, which reads TGIS_SPECULATOR.  Its config, tensor names and shapes,
    spec_tokens and, given the base model's config, that model's sizes are checked; no tensor is loaded."""
    ckpt = speculator if isinstance(speculator, SpeculatorCheckpoint) else None
    if ckpt is None:
        path = parse_speculator(speculator)
        if path is None:
            return None
        ckpt = open_checkpoint(path)
    check_spec_tokens(ckpt.cfg, spec_tokens)
    if base_config is not None:
        check_base(ckpt.cfg, base_config.hidden_size, base_config.vocab_size)
    return ckpt


@dataclass
class _Head:
    proj: object   # native.DenseWeight [I, E or I]
    emb: torch.Tensor
    ln_weight: torch.Tensor
    ln_bias: torch.Tensor
    head: object   # native.DenseWeight [V, I]


class DraftBuffers:
    """Everything one chain over `rows` requests writes, allocated once: a captured chain holds their pointers."""

    def __init__(self, cfg: SpeculatorConfig, K: int, rows: int, dtype, device):
        from tgis_amd import native

        self.rows = rows
        self.x_in = torch.zeros((rows, cfg.emb_dim), dtype=dtype, device=device) if cfg.scale_input else None
        self.proj_out = torch.zeros((rows, cfg.inner_dim), dtype=dtype, device=device)
        self.x = torch.zeros((rows, cfg.inner_dim), dtype=dtype, device=device)
        self.logits = torch.zeros((rows, cfg.vocab_size), dtype=torch.float32, device=device)
        self.toks = torch.zeros((K, rows), dtype=torch.int64, device=device)
        self.lps = torch.zeros(rows, dtype=torch.float32, device=device)
        self.argmax_scratch = native.argmax_scratch(rows, device)


class MLPSpeculator:
    """The speculator on the device.  Tied weights are loaded, cast and prepared once and shared by the heads."""

    def __init__(self, ckpt: SpeculatorCheckpoint, spec_tokens: int, dtype: torch.dtype, device):
        from tgis_amd import native

        cfg = self.cfg = ckpt.cfg
        check_spec_tokens(cfg, spec_tokens)
        self.K, self.dtype, self.device = spec_tokens, dtype, device
        self.alpha = constants(cfg.n_predict, cfg.inner_dim)[2]
        raw, images = {}, {}

        def tensor(name):  # weights are cast to the model dtype at load, as the reference does (torch_dtype=dtype)
            if name not in raw:
                raw[name] = ckpt.load(name).to(device=device, dtype=dtype).contiguous()
            return raw[name]

        def image(name):
            if name not in images:
                images[name] = native.DenseWeight(ckpt.load(name).to(device=device, dtype=dtype))
            return images[name]

        # only the K heads that draft are loaded
        self.heads = [_Head(image(h["proj"]), tensor(h["emb"]), tensor(h["ln_weight"]), tensor(h["ln_bias"]), image(h["head"]))
                      for h in ckpt.names[:spec_tokens]]
        self.nbytes = sum(t.numel() * t.element_size() for t in raw.values()) + sum(w.image.numel() for w in images.values())
        self._eager = {}  # rows -> DraftBuffers of the chains launched outside a captured graph

    def buffers(self, rows: int) -> DraftBuffers:
        return DraftBuffers(self.cfg, self.K, rows, self.dtype, self.device)

    def draft(self, hidden, latest_ids, drafts, hits, hits_copy=None, bufs: Optional[DraftBuffers] = None):
        """drafts [B, K] = the chain's top-1 tokens from hidden [B, E] (the states that predicted latest_ids [B]); hits (and
        hits_copy) = 1.  No allocation when `bufs` is given, no synchronisation either way."""
        from tgis_amd import native
        from tgis_amd.utils.layers import workspace

        B = hidden.shape[0]
        if bufs is None:
            bufs = self._eager.get(B)
            if bufs is None:
                bufs = self._eager[B] = self.buffers(B)
        assert bufs.rows == B and drafts.shape == (B, self.K)
        ws = workspace(hidden.device)
        x = hidden
        if self.cfg.scale_input:
            x = native.spec_mlp_input(hidden, None, 1, bufs.x_in, scale_input=True, eps=EPS)
        tok = latest_ids
        for i, h in enumerate(self.heads):
            native.dense_gemm(x, h.proj, ws, out=bufs.proj_out)
            x = native.spec_mlp_state(bufs.proj_out, tok, h.emb, h.ln_weight, h.ln_bias, self.alpha, bufs.x, eps=EPS)
            native.dense_gemm(x, h.head, ws, out_f32=True, out=bufs.logits)
            tok = bufs.toks[i]
            native.argmax_logprob(bufs.logits, ids_out=tok, logprob_out=bufs.lps, scratch=bufs.argmax_scratch)
        native.spec_mlp_drafts(bufs.toks, drafts, hits, hits_copy)
