"""Prompt-lookup speculative decoding, the host rules: the options, which decode steps verify drafts, and the
counters.  The kernels are tgis_spec_stage / tgis_spec_accept / tgis_spec_propose (csrc/spec_decode.hip); the captured
verify step is models/decode_graph.py's _VerifyGraph.  With spec_sampling, batches that sample or carry processors verify too:
tgis_warp_sample_verify chooses behind every row, tgis_spec_accept_sampled accepts and advances the streams (utils/tokens.py
choose_fused_verify / commit_verify).  With spec_candidates = C > 1 a greedy request brings up to C draft chains to a verify
step, verified in one forward as a token tree of 1 + C K rows per request (tgis_spec_tree_stage / tgis_attn_paged_tree /
tgis_spec_tree_accept / tgis_spec_tree_commit / tgis_spec_propose_multi; models/decode_graph.py's _TreeVerifyGraph).  Nothing
here needs a GPU."""
import os
from typing import List, Optional

MAX_SPEC_TOKENS = 7   # K + 1 rows per request in a verify forward
MAX_SPEC_NGRAM = 4
MAX_VERIFY_ROWS = 64  # what the decode GEMMs serve: graph_bucket(B) * (K + 1) rows at the most
MAX_SPEC_CANDIDATES = 4  # C draft chains per request; a verify forward then has 1 + C K rows per request

# why a decode step of a speculating model ran the plain step, one counter each (spec_stats()["fallback_" + cause])
FALLBACK_CAUSES = ("not_greedy", "details", "rows", "remaining", "no_match", "pages")
# verify_steps_sampled: those of `verify_steps` whose rows were chosen by the fused chooser (spec_sampling) and not the argmax
SPEC_STATS = ("decode_steps", "verify_steps", "verify_steps_sampled") + tuple("fallback_" + c for c in FALLBACK_CAUSES) + (
    "drafted", "accepted", "emitted", "won_by_later_candidate")


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


def parse_spec_candidates(value=None) -> int:
    """C, the draft chains a request brings to a verify step: the argument, else TGIS_SPEC_CANDIDATES; unset or 1 = one chain
    (the path without the option), 2 .. 4 = a token tree."""
    return _parse_int(value, "TGIS_SPEC_CANDIDATES", 1, 1, MAX_SPEC_CANDIDATES, "spec_candidates (TGIS_SPEC_CANDIDATES)")


def tree_rows(C: int, K: int) -> int:
    """Rows per request of a verify step: the latest token and C chains of K drafts."""
    return 1 + C * K


def check_spec_candidates(C: int, spec_tokens: int, mlp_drafter: bool, spec_sampling: bool) -> None:
    """What C > 1 needs of the other options, checked before anything is loaded."""
    if C <= 1:
        return
    if spec_tokens <= 0:
        raise ValueError(f"spec_candidates={C} needs spec_tokens > 0: there is nothing to verify without drafts")
    if mlp_drafter:
        raise NotImplementedError(
            f"spec_candidates={C} with an MLP speculator: the speculator drafts its top-1 chain, per-head top-k candidates "
            "are a drafter of their own (DESIGN.md §8); use the prompt lookup or spec_candidates=1")
    if spec_sampling:
        raise NotImplementedError(
            f"spec_candidates={C} with spec_sampling: the fused chooser's context behind a tree row is not built "
            "(DESIGN.md §8); sampled requests verify one chain")


def check_tree_rows(C: int, K: int, num_heads: int, num_kv_heads: int) -> None:
    """C > 1: the 1 + C K rows of a request must fit the attention's decode form for the model's head grouping (one mask
    word per row; rows * padded group size <= 64), or the verify step would be the prefill form, which takes no mask."""
    if C <= 1:
        return
    G = max(1, num_heads // max(1, num_kv_heads))
    Gp = 1 << (min(G, 16) - 1).bit_length()
    if tree_rows(C, K) * Gp > 64:
        raise ValueError(
            f"spec_candidates={C} with spec_tokens={K}: {tree_rows(C, K)} rows per request times the padded head group "
            f"({Gp}) exceed the 64 columns of the attention's decode form; use fewer candidates or drafts")


def tree_q_mask(C: int, K: int) -> List[int]:
    """The attention mask of one request's 1 + C K verify rows, one 64-bit word per row (tgis_attn_paged_tree): row 0 sees
    itself; row 1 + c K + j (draft j of candidate c) sees row 0 and its own candidate's rows up to and including itself."""
    words = [1]
    for c in range(C):
        first = 1 + c * K
        for j in range(K):
            words.append(1 | (((1 << (j + 1)) - 1) << first))
    return words


def check_spec_world(spec_tokens: int, tp_world: int) -> None:
    if spec_tokens > 0 and tp_world > 1:
        raise NotImplementedError(
            f"spec_tokens={spec_tokens} with {tp_world} tensor-parallel ranks: speculative decoding under tensor "
            "parallelism is out of scope (DESIGN.md §8); run it on one rank or set spec_tokens=0")


def fallback_cause(K: int, rows: int, plain_greedy: bool, details: bool, remaining: List[int],
                   hits: List[int], C: int = 1) -> Optional[str]:
    """Why a decode step must not verify drafts, or None if it may (the page look-ahead is tried after this).
    rows: graph_bucket(batch size); remaining: total_length - input_length per request; hits: the lookups' results, or a
    callable that fetches them — it is called only when nothing cheaper has decided the step.
    plain_greedy: with spec_sampling on, the caller passes "the fused chooser can choose for this batch on the device" in its
    place (always true for logits on the GPU), so that nothing answers `not_greedy`; details still keep the plain step.
    C: candidates per request; a verify step then has 1 + C K rows per request, which occupy cache positions up to C K behind
    the latest token.  A batch that cannot verify C candidates takes the plain step (never fewer candidates)."""
    if not plain_greedy:
        return "not_greedy"
    if details:  # top_n_toks / ranks are read from the warped scores of one row per request
        return "details"
    if rows * tree_rows(C, K) > MAX_VERIFY_ROWS:
        return "rows"
    if min(remaining) < C * K + 1:  # the block table, all_input_ids and the page budget end at total_length
        return "remaining"
    if not any(hits() if callable(hits) else hits):
        return "no_match"
    return None


def may_ever_verify(K: int, rows: int, C: int = 1) -> bool:
    """Whether a batch of this bucket can verify at all: if not, nobody drafts for it."""
    return K > 0 and rows * tree_rows(C, K) <= MAX_VERIFY_ROWS


def new_stats() -> dict:
    return dict.fromkeys(SPEC_STATS, 0)
