"""The search behind the prompts and seeds of tests/test_spec_sampled_model_gpu.py.

For every request of its scenarios: the first `draw` (tests/spec_sampled_ref.py `drawn_prompt`; a sampled request also
takes `draw` as its seed) at which the fp32 CPU oracle decides each of the request's first TOKENS tokens by at least
2 LOGIT_TOL / T in warped-score units, and (a sampled request) at least MIN_DRAWN of them by the draw and not the argmax — for a sampled request the race of `race_choice` (warped score plus the Gumbel term,
top-1 minus top-2), for a greedy one top-1 minus top-2 of the warped scores (times the repetition penalty where there is
one: it multiplies the error of a negative logit).  That is the condition the forced prompts of tests/test_spec_model_gpu.py
meet for the argmax: a whole fp16 step's logit error is bounded by LOGIT_TOL, so an id that differs from the plain run is
an error and not a near-tie.  Requests marked e4m3 must meet it, with the same ids, with the e4m3 round trip on the keys
and values of the oracle's cache too.

    python tests/golden/make_spec_sampled_prompts.py        prints SCENARIOS with the draws and the achieved margins
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "text-generation-inference_amd")]

from oracle import ops_ref  # noqa: E402
from oracle.llama_ref import LlamaRef  # noqa: E402
from oracle.tiny_models import TinyLlamaConfig, tiny_llama_tensors  # noqa: E402
from tests import spec_sampled_ref as ref  # noqa: E402
from tests.test_spec_sampled_model_gpu import LOGIT_TOL, SCENARIOS, TOKENS, oracle_request  # noqa: E402


# a sampled request's stream must depend on its draws: at least this many of its tokens are not the argmax of their warped
# scores.  (The tiny model is peaked: at temperature 0.8 the draw decides about one token in twenty-five, and rarely by the
# margin asked for; one such token per request is what a search of seconds finds.)
MIN_DRAWN = 1


def _with_e4m3_cache(fn):
    """Runs fn with the oracle's attention reading keys and values through an e4m3 round trip (scale 1)."""
    plain = ops_ref.attention_varlen

    def quantised(q, k, v, *a, **kw):
        rt = (lambda x: x.to(torch.float8_e4m3fn).to(torch.float32))
        return plain(q, rt(k), rt(v), *a, **kw)

    ops_ref.attention_varlen = quantised
    try:
        return fn()
    finally:
        ops_ref.attention_varlen = plain


def main():
    cfg = TinyLlamaConfig()
    llama = LlamaRef(cfg, tiny_llama_tensors(cfg, seed=7, quantize=None, groupsize=64))
    for name, requests in SCENARIOS.items():
        for i, r in enumerate(requests):
            bound = 2 * LOGIT_TOL / r.get("temperature", 1.0) * r.get("repetition_penalty", 1.0)
            n = r.get("tokens", TOKENS)
            for draw in range(100000):
                kw = oracle_request({**r, "draw": draw})
                ids, margins, drawn = ref.oracle_stream(llama, n=n, bound=bound, **kw)
                if len(ids) < n or min(margins) < bound or (kw["params"]["sample"] and sum(drawn) < MIN_DRAWN):
                    continue
                if r.get("e4m3"):
                    ids8, margins8, _ = _with_e4m3_cache(lambda: ref.oracle_stream(llama, n=n, bound=bound, **kw))
                    if ids8 != ids or min(margins8) < bound:
                        continue
                    margins = margins + margins8
                print(f"{name}[{i}]: draw={draw}  bound {bound:.3f}  achieved margin {min(margins):.3f}  "
                      f"tokens the draw decided {sum(drawn)}/{n}  ids {ids}", flush=True)
                break


if __name__ == "__main__":
    main()
