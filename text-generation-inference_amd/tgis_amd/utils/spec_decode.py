"""Prompt-lookup speculative decoding, the host rules: the options, which decode steps verify drafts, and the
counters.  The kernels are tgis_spec_stage / tgis_spec_accept / tgis_spec_propose (csrc/spec_decode.hip); the captured
verify step is models/decode_graph.py's _VerifyGraph.  With spec_sampling, batches that sample or carry processors verify too:
tgis_warp_sample_verify chooses behind every row, tgis_spec_accept_sampled accepts and advances the streams (utils/tokens.py
choose_fused_verify / commit_verify).  Nothing here needs a GPU."""
import os
from typing import List, Optional

MAX_SPEC_TOKENS = 7   # K + 1 rows per request in a verify forward
MAX_SPEC_NGRAM = 4
MAX_VERIFY_ROWS = 64  # what the decode GEMMs serve: graph_bucket(B) * (K + 1) rows at the most

# why a decode step of a speculating model ran the plain step, one counter each (spec_stats()["fallback_" + cause])
FALLBACK_CAUSES = ("not_greedy", "details", "rows", "remaining", "no_match", "pages")
# verify_steps_sampled: those of `verify_steps` whose rows were chosen by the fused chooser (spec_sampling) and not the argmax
SPEC_STATS = ("decode_steps", "verify_steps", "verify_steps_sampled") + tuple("fallback_" + c for c in FALLBACK_CAUSES) + (
    "drafted", "accepted", "emitted")


def _parse_int(value, env: str, default: int, lo: int, hi: int, what: str) -> int:
    if value is None:
        value = os.getenv(env)
        if value is None or str(value).strip() == "":
            return default
    if isinstance(value, bool) or isinstance(value, float):
        raise ValueError(f"{what} must be an integer in {lo} .. {hi}, got {value!r}")
    try:
        n = int(str(value).strip())
    except ValueError:
        raise ValueError(f"{what} must be an integer in {lo} .. {hi}, got {value!r}") from None
    if not lo <= n <= hi:
        raise ValueError(f"{what} must be in {lo} .. {hi}, got {n}")
    return n


def parse_spec_tokens(value=None) -> int:
    """K, the drafts verified per request and step: the argument, else TGIS_SPEC_TOKENS; 0 or unset = off, 1 .. 7 = on."""
    return _parse_int(value, "TGIS_SPEC_TOKENS", 0, 0, MAX_SPEC_TOKENS, "spec_tokens (TGIS_SPEC_TOKENS)")


def parse_spec_ngram(value=None) -> int:
    """N, the longest suffix the lookup tries: the argument, else TGIS_SPEC_NGRAM; default 3, 1 .. 4."""
    return _parse_int(value, "TGIS_SPEC_NGRAM", 3, 1, MAX_SPEC_NGRAM, "spec_ngram (TGIS_SPEC_NGRAM)")


def parse_spec_sampling(value=None) -> bool:
    """Whether batches that are not plain greedy (sampling, warpers, penalties, an unmet min_new_tokens) verify drafts too:
    the argument, else TGIS_SPEC_SAMPLING (unset: false).  A bool, "true" or "false"; anything else raises.  It means
    something only with spec_tokens > 0."""
    if value is None:
        value = os.getenv("TGIS_SPEC_SAMPLING", "false")
    if isinstance(value, bool):
        return value
    name = str(value).strip().lower()
    if name not in ("true", "false"):
        raise ValueError(f"spec_sampling (TGIS_SPEC_SAMPLING) {value!r} is not supported (true or false)")
    return name == "true"


def check_spec_world(spec_tokens: int, tp_world: int) -> None:
    if spec_tokens > 0 and tp_world > 1:
        raise NotImplementedError(
            f"spec_tokens={spec_tokens} with {tp_world} tensor-parallel ranks: speculative decoding under tensor "
            "parallelism is out of scope (DESIGN.md §8); run it on one rank or set spec_tokens=0")


def fallback_cause(K: int, rows: int, plain_greedy: bool, details: bool, remaining: List[int],
                   hits: List[int]) -> Optional[str]:
    """Why a decode step must not verify drafts, or None if it may (the page look-ahead is tried after this).
    rows: graph_bucket(batch size); remaining: total_length - input_length per request; hits: the lookups' results, or a
    callable that fetches them — it is called only when nothing cheaper has decided the step.
    plain_greedy: with spec_sampling on, the caller passes "the fused chooser can choose for this batch on the device" in its
    place (always true for logits on the GPU), so that nothing answers `not_greedy`; details still keep the plain step."""
    if not plain_greedy:
        return "not_greedy"
    if details:  # top_n_toks / ranks are read from the warped scores of one row per request
        return "details"
    if rows * (K + 1) > MAX_VERIFY_ROWS:
        return "rows"
    if min(remaining) < K + 1:  # the block table, all_input_ids and the page budget end at total_length
        return "remaining"
    if not any(hits() if callable(hits) else hits):
        return "no_match"
    return None


def may_ever_verify(K: int, rows: int) -> bool:
    """Whether a batch of this bucket can verify at all: if not, nobody drafts for it."""
    return K > 0 and rows * (K + 1) <= MAX_VERIFY_ROWS


def new_stats() -> dict:
    return dict.fromkeys(SPEC_STATS, 0)
