"""Prompt-token details (`details.input_toks`) without the [T, V] logits, opt-in (FlashCausalLM fused_input_logprobs).

The path without the option sends all T prompt rows through lm_head and runs log_softmax, a gather and a rank compare over
the fp32 [T, V] result (utils/tokens.py get_input_tokens_info): three tensors of T V elements for the 2 T numbers wanted.
With the option the prefill keeps lm_head on the last rows, hands the final-normed hidden rows of all positions to one
native.head_logprobs call for the whole batch, and the same InputTokens messages are built from its results after one
device-to-host copy.  Per-position top-n tokens need the rows: a batch in which an input_toks request sets top_n_toks
keeps the path without the option.  Not under tensor parallelism, where the head is sharded over the vocabulary."""
import os
from typing import List, Union

import numpy as np
import torch

from tgis_amd import native
from tgis_amd.utils.token_types import InputTokens, TokenInfo


def parse_fused_input_logprobs(value: Union[None, bool, str] = None) -> bool:
    """Whether input_toks requests are scored by the fused head kernel: the argument, else TGIS_FUSED_INPUT_LOGPROBS
    (unset: false).  A bool, "true" or "false"; anything else raises."""
    if value is None:
        value = os.getenv("TGIS_FUSED_INPUT_LOGPROBS", "false")
    if isinstance(value, bool):
        return value
    name = str(value).strip().lower()
    if name not in ("true", "false"):
        raise ValueError(f"fused_input_logprobs (TGIS_FUSED_INPUT_LOGPROBS) {value!r} is not supported (true or false)")
    return name == "true"


def check_fused_input_world(fused: bool, tp_world: int) -> None:
    if fused and tp_world > 1:
        raise NotImplementedError(
            f"fused_input_logprobs with {tp_world} tensor-parallel ranks: the head is sharded over the vocabulary there, "
            "which is out of scope (DESIGN.md §8); run on one rank or set fused_input_logprobs=false")


def batch_takes_fused(requests) -> bool:
    """Whether a prefill of these requests scores its prompt tokens with the fused call: somebody asks for input_toks,
    and nobody who does also asks for top-n tokens per position."""
    asking = [r for r in requests if r.details.input_toks]
    return bool(asking) and not any(r.details.top_n_toks for r in asking)


def head_weight(model) -> torch.Tensor:
    """The head's checkpoint-layout [V, K] tensor (FastLinear.weight)."""
    linear = model.lm_head.linear
    if getattr(linear, "bias", None) is not None:
        raise NotImplementedError("fused_input_logprobs: a head with a bias is not served")
    return linear.weight


def fused_input_tokens(requests, input_lengths: List[int], all_input_ids: torch.Tensor, hidden: torch.Tensor,
                       weight: torch.Tensor) -> List[InputTokens]:
    """The InputTokens of every request that asks for them, in request order.  hidden [sum(input_lengths), K]: the rows of
    the prompts, concatenated; row j of a prompt predicts its token j + 1, its last row predicts no prompt token (target -1,
    like every row of a request that does not ask).  One launch sequence and one device-to-host copy for the batch."""
    starts = np.concatenate([[0], np.cumsum(input_lengths)])
    T = int(starts[-1])
    assert hidden.shape[0] == T, "the fused prompt scores need the hidden rows of every prompt position"
    ids = torch.zeros(T, dtype=torch.int64, device=hidden.device)
    targets = torch.full((T,), -1, dtype=torch.int64, device=hidden.device)
    for i, (r, n) in enumerate(zip(requests, input_lengths)):
        if r.details.input_toks:
            s = int(starts[i])
            ids[s:s + n] = all_input_ids[i, :n]
            targets[s:s + n - 1] = all_input_ids[i, 1:n]
    logprob, rank, _lse = native.head_logprobs(hidden, weight, targets)
    host = torch.stack([logprob.view(torch.int32), rank, ids.to(torch.int32)]).cpu().numpy()
    lps, ranks, tok = host[0].view(np.float32).tolist(), host[1].tolist(), host[2].tolist()
    out = []
    for i, (r, n) in enumerate(zip(requests, input_lengths)):
        if not r.details.input_toks:
            continue
        s = int(starts[i])
        want_lp, want_rank = r.details.logprobs, r.details.ranks
        # the first token has no score: NaN among logprobs, 0 among ranks; a detail that was not asked for stays 0
        out.append(InputTokens(request_id=r.id, tokens=[
            TokenInfo(token_id=tok[s + j],
                      logprob=(lps[s + j - 1] if j else float("nan")) if want_lp else 0.0,
                      rank=ranks[s + j - 1] if want_rank and j else 0)
            for j in range(n)]))
    return out
