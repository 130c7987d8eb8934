"""Speculative verification of sampled and warped requests restated in numpy, on oracle/sampler_ref.py's `warp_row` and
`race_choice`: what tgis_warp_sample_verify and tgis_spec_accept_sampled (include/tgis_hip.h) and the chooser's
`choose_fused_verify` / `commit_verify` (utils/tokens.py) must compute.  Plain loops: this is the yardstick.

The law.  A request's plain run chooses token t from the logits behind its context with the parameters of the request, the
EOS rule t steps on and, if it samples, draw number offset + t of its Philox stream (seed, offset).  A verify step runs
that very choice behind its latest token and behind each of K drafts, row j assuming drafts[:j] were emitted; drafts are
accepted while the chosen token equals the draft.  So the step emits the plain stream, cut behind the first miss, and the
stream advances by the number emitted.  For a drafter that proposes one token with certainty this IS the rejection rule:
the draw picks the draft with probability p(draft), and on a miss the token drawn instead is distributed as p restricted
to the other tokens, renormalised."""
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from oracle import sampler_ref


def eos_rule(cur: int, min_new: int, lp: Optional[Tuple[int, float]]):
    """One step of the EOS rule for one request: ((mode, factor), counter afterwards).  mode 0: nothing."""
    if cur < min_new:
        return (1, 0.0), cur + 1
    if lp is not None:
        past = cur - lp[0]
        return ((2, pow(lp[1], past) - 1) if past > 0 else (0, 0.0)), cur + 1
    return (0, 0.0), cur


def choose(logits: np.ndarray, params: dict, context: Sequence[int], eos: Tuple[int, float], seed: int, offset: int):
    """One choice of the chooser: (id, warped scores, margin of the decision in warped-score units).
    params: temperature, top_k, top_p_cut, typical_p, rep_penalty, exclude_id, eos_id, sample."""
    warped = sampler_ref.warp_row(
        logits, temperature=params.get("temperature", 1.0), top_k=params.get("top_k", 0),
        top_p_cut=params.get("top_p_cut", 0.0), typical_p=params.get("typical_p", 1.0),
        rep_penalty=params.get("rep_penalty", 1.0), input_ids=list(context), exclude_id=params.get("exclude_id", -1),
        eos_id=params.get("eos_id", -1), eos_mode=eos[0], eos_factor=eos[1])
    if params.get("sample"):
        idx, margin = sampler_ref.race_choice(warped, seed & 0xFFFFFFFFFFFFFFFF, offset)
        return idx, warped, margin
    order = np.argsort(-warped, kind="stable")
    return int(order[0]), warped, float(warped[order[0]] - warped[order[1]])


class Request:
    """The state a request carries from step to step: context, EOS counter, stream offset."""

    def __init__(self, params: dict, context: Sequence[int], seed: int = 0, offset: int = 0, min_new: int = 0,
                 length_penalty: Optional[Tuple[int, float]] = None, generated: int = 0):
        self.params, self.context, self.seed, self.offset = params, list(context), seed, offset
        self.min_new, self.lp, self.cur = min_new, length_penalty, generated
        self.margins: List[float] = []
        self.drawn: List[bool] = []  # per plain step: the draw chose another token than the argmax would have

    def plain_step(self, model: Callable[[Sequence[int]], np.ndarray]) -> int:
        eos, self.cur = eos_rule(self.cur, self.min_new, self.lp)
        tok, warped, margin = choose(model(self.context), self.params, self.context, eos, self.seed, self.offset)
        self.drawn.append(tok != int(np.argmax(warped)))
        if self.params.get("sample"):
            self.offset += 1
        self.context.append(tok)
        self.margins.append(margin)
        return tok

    def verify_rows(self, model, drafts: Sequence[int]) -> List[int]:
        """The token chosen behind each of the K + 1 verify rows; no state moves."""
        cur, chosen = self.cur, []
        for j in range(len(drafts) + 1):
            ctx = self.context + list(drafts[:j])
            eos, cur = eos_rule(cur, self.min_new, self.lp)
            tok, _, _ = choose(model(ctx), self.params, ctx, eos, self.seed, self.offset + j)
            chosen.append(tok)
        return chosen

    def verify_step(self, model, drafts: Sequence[int]) -> List[int]:
        """Accept and commit: returns the tokens emitted."""
        chosen = self.verify_rows(model, drafts)
        n = 1
        while n <= len(drafts) and chosen[n - 1] == drafts[n - 1]:
            n += 1
        for _ in range(n):
            _, self.cur = eos_rule(self.cur, self.min_new, self.lp)
        if self.params.get("sample"):
            self.offset += n
        self.context.extend(chosen[:n])
        return chosen[:n]


def expand(B: int, K: int, L: int, input_ids: np.ndarray, drafts: np.ndarray, pad_id: int):
    """The host-expanded problem of a verify launch, for the plain chooser: one row per (b, j), whose context is
    input_ids[b, :L] followed by drafts[b, :j] and then `pad_id` (an id the chooser skips: out of range or excluded) up to
    the common width L + K.  Returns ids [B (K + 1), L + K]."""
    out = np.full((B * (K + 1), L + K), pad_id, dtype=np.int64)
    for b in range(B):
        for j in range(K + 1):
            out[b * (K + 1) + j, :L] = input_ids[b, :L]
            out[b * (K + 1) + j, L:L + j] = drafts[b, :j]
    return out


# ---- the prompts of tests/test_spec_sampled_model_gpu.py ------------------------------------------------------------------------
PROMPT_SEED = 2024


def drawn_prompt(length: int, draw: int) -> List[int]:
    """Prompt number `draw` of a given length (tests/golden/make_spec_sampled_prompts.py searches over `draw`)."""
    return np.random.default_rng([PROMPT_SEED, length, draw]).integers(3, 256, size=length).tolist()


def oracle_stream(llama, prompt: Sequence[int], n: int, params: dict, seed: int = 0, min_new: int = 0,
                  length_penalty: Optional[Tuple[int, float]] = None, bound: float = 0.0):
    """(ids, margins, drawn) of the first n tokens of ONE request on the fp32 CPU oracle (oracle/llama_ref.py LlamaRef),
    chosen by `choose`; stops early at the first token decided by less than `bound`.  drawn[t]: token t is not the argmax
    of its warped scores (the draw decided it)."""
    import torch

    state = llama.new_state(1)
    L = len(prompt)
    logits = llama.forward(torch.tensor(prompt, dtype=torch.int64), torch.arange(L), [0] * L, state, last_only=True)[0]
    req = Request(params, prompt, seed=seed, min_new=min_new, length_penalty=length_penalty)
    ids = []
    for t in range(n):
        tok = req.plain_step(lambda _ctx: logits.numpy())
        ids.append(tok)
        if req.margins[-1] < bound or t + 1 == n:
            break
        logits = llama.forward(torch.tensor([tok], dtype=torch.int64), torch.tensor([L + t]), [0], state)[0]
    return ids, req.margins, req.drawn
