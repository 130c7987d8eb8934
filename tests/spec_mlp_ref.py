"""The MLP speculator restated in fp64 (numpy), independent of tgis_amd/utils/mlp_speculator.py and of the kernels, plus
makers of tiny speculators and a writer of their checkpoint directories.

    state_weight = 0.5 ** (0.5 / P);  emb_weight = sqrt((1 - state_weight^2) I / 2);  alpha = emb_weight / state_weight
    x = h;  scale_input: x = x rsqrt(mean(x^2) + eps) / sqrt(2)
    head i:  s = proj_i x + alpha emb_i[t];  u = s rsqrt(mean(s^2) + eps) ln_i.weight + ln_i.bias;  x = gelu_erf(u)
             t = argmax(head_i x), lowest id on ties
"""
import json
import math
import os

import numpy as np

EPS = 1e-6
_erf = np.vectorize(math.erf, otypes=[np.float64])


def constants(P, I):
    state_weight = 0.5 ** (0.5 / P)
    emb_weight = math.sqrt((1.0 - state_weight * state_weight) * I / 2.0)
    return state_weight, emb_weight, emb_weight / state_weight


def gelu(u):
    u = np.asarray(u, dtype=np.float64)
    return 0.5 * u * (1.0 + _erf(u / math.sqrt(2.0)))


def scale_input(h):
    h = np.asarray(h, dtype=np.float64)
    return h / np.sqrt((h * h).mean(-1, keepdims=True) + EPS) / math.sqrt(2.0)


def state(proj_out, tok, emb, ln_weight, ln_bias, alpha):
    """(x, n w, u) of tgis_spec_mlp_state for rows proj_out [B, I]; token ids outside [0, V) are clamped."""
    emb = np.asarray(emb, dtype=np.float64)
    tok = np.clip(np.asarray(tok, dtype=np.int64), 0, emb.shape[0] - 1)
    s = np.asarray(proj_out, dtype=np.float64) + alpha * emb[tok]
    n = s / np.sqrt((s * s).mean(-1, keepdims=True) + EPS)
    nw = n * np.asarray(ln_weight, dtype=np.float64)
    u = nw + np.asarray(ln_bias, dtype=np.float64)
    return gelu(u), nw, u


class Speculator:
    """cfg: dict(emb_dim, inner_dim, vocab_size, n_predict, tie_weights, scale_input); tensors: name -> array, untied names
    ("emb.0.weight" ...) for every head — `write_checkpoint` stores tied ones once if asked to."""

    def __init__(self, cfg, tensors):
        self.cfg = dict(cfg)
        self.t = {k: np.asarray(v, dtype=np.float64) for k, v in tensors.items()}
        self.P = cfg["n_predict"]
        self.I = cfg.get("inner_dim") or cfg["emb_dim"]
        self.alpha = constants(self.P, self.I)[2]

    def draft(self, h, t, K):
        """(drafts [B, K] int64, margins [B, K]: top-1 minus top-2 logit of every head) from h [B, E] and ids t [B]."""
        x = np.asarray(h, dtype=np.float64)
        if self.cfg.get("scale_input"):
            x = scale_input(x)
        t = np.asarray(t, dtype=np.int64)
        drafts, margins = [], []
        for i in range(K):
            g = self.t
            x, _, _ = state(x @ g[f"proj.{i}.weight"].T, t, g[f"emb.{i}.weight"], g[f"ln.{i}.weight"], g[f"ln.{i}.bias"],
                            self.alpha)
            logits = x @ g[f"head.{i}.weight"].T
            t = logits.argmax(-1)  # numpy: the first (lowest) index on ties
            top2 = np.sort(logits, axis=-1)[:, -2:]
            drafts.append(t)
            margins.append(top2[:, 1] - top2[:, 0])
        return np.stack(drafts, 1), np.stack(margins, 1)


def _f16(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float32)


def make_random(E, I, V, P, seed, head_std=4.0, tie_weights=False, scale=False):
    """A seeded random speculator whose values are exact in f16.  Unit-normal embeddings, fan-in-scaled projections, norm
    weights around 1, heads drawn wide (head_std): the top-2 gaps of its logits are then several logits."""
    rng = np.random.default_rng(seed)
    t = {}
    for i in range(P):
        if tie_weights and i > 0:  # index 0 of emb / head / ln serves every head, proj.1 every head behind the first
            for kind in ("emb.{}.weight", "head.{}.weight", "ln.{}.weight", "ln.{}.bias"):
                t[kind.format(i)] = t[kind.format(0)]
        else:
            t[f"emb.{i}.weight"] = _f16(rng.standard_normal((V, I)))
            t[f"head.{i}.weight"] = _f16(rng.standard_normal((V, I)) * head_std)
            t[f"ln.{i}.weight"] = _f16(1.0 + 0.1 * rng.standard_normal(I))
            t[f"ln.{i}.bias"] = _f16(0.1 * rng.standard_normal(I))
        if tie_weights and i > 1:
            t[f"proj.{i}.weight"] = t["proj.1.weight"]
        else:
            k = E if i == 0 else I
            t[f"proj.{i}.weight"] = _f16(rng.standard_normal((I, k)) / math.sqrt(k))
    cfg = dict(emb_dim=E, inner_dim=I, vocab_size=V, n_predict=P, tie_weights=tie_weights, scale_input=scale,
               n_candidates=5, top_k_tokens_per_head=[4] * P)
    return Speculator(cfg, t)


def make_successor(E, V, P):
    """I = V, proj = 0, ln weight 1 and bias 0, head = identity, emb_i[t] = one-hot((t + i + 1) mod V): head i drafts its
    input token + i + 1, so the chain behind token t is t + 1, t + 3, t + 6 ... (mod V), whatever the hidden state.  The
    normed one-hot is sqrt(V) against zeros: that is each head's margin."""
    t = {}
    eye = np.eye(V, dtype=np.float32)
    for i in range(P):
        t[f"emb.{i}.weight"] = np.roll(eye, i + 1, axis=1)  # row t has its one at column (t + i + 1) mod V
        t[f"proj.{i}.weight"] = np.zeros((V, E if i == 0 else V), dtype=np.float32)
        t[f"head.{i}.weight"] = eye
        t[f"ln.{i}.weight"] = np.ones(V, dtype=np.float32)
        t[f"ln.{i}.bias"] = np.zeros(V, dtype=np.float32)
    return Speculator(dict(emb_dim=E, inner_dim=V, vocab_size=V, n_predict=P), t)


def successor_drafts(t, K, V):
    out, cur = [], int(t)
    for i in range(K):
        cur = (cur + i + 1) % V
        out.append(cur)
    return out


def write_checkpoint(path, spec, prefix="", store_tied_once=False, dtype="float16", inner_dim_zero=False):
    """config.json + model.safetensors in `path` (created); returns path.  prefix: "" or "speculator."."""
    import torch
    from safetensors.torch import save_file

    os.makedirs(path, exist_ok=True)
    cfg = dict(spec.cfg)
    if inner_dim_zero:
        assert cfg["inner_dim"] == cfg["emb_dim"]
        cfg["inner_dim"] = 0
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(cfg, f)
    tensors = {}
    for name, a in spec.t.items():
        i = int(name.split(".")[1])
        if store_tied_once and spec.cfg.get("tie_weights") and i > (1 if name.startswith("proj.") else 0):
            continue
        tensors[prefix + name] = torch.from_numpy(np.ascontiguousarray(a)).to(getattr(torch, dtype)).clone()
    save_file(tensors, os.path.join(path, "model.safetensors"))
    return path
