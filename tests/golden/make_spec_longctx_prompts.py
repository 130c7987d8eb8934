"""The search behind the prompts and seeds of tests/test_spec_longctx_model_gpu.py.

For every request of its scenarios: the first `draw` (`drawn_prompt` there; a sampled request also takes `draw` as its
seed) at which the fp32 CPU oracle decides each of the request's first TOKENS tokens by at least the scenario's bound — for
a greedy request top-1 minus top-2 of the logits, >= 0.9 (the rule of the forced prompts of tests/test_spec_model_gpu.py);
for a sampled one the race of `race_choice` in warped-score units, >= 2 LOGIT_TOL / T, with at least one token decided by
the draw and not the argmax (the rule of tests/test_spec_sampled_model_gpu.py).  Greedy requests must meet theirs, with the
same ids, with the e4m3 round trip on the keys and values of the oracle's cache too: the e4m3 test runs them as well.

    python tests/golden/make_spec_longctx_prompts.py        prints the draws and the achieved margins
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "text-generation-inference_amd")]

from oracle.llama_ref import LlamaRef  # noqa: E402
from oracle.tiny_models import tiny_llama_tensors  # noqa: E402
from tests import spec_sampled_ref as ref  # noqa: E402
from tests.golden.make_spec_sampled_prompts import MIN_DRAWN, _with_e4m3_cache  # noqa: E402
from tests.test_spec_longctx_model_gpu import SCENARIOS, TOKENS, bound_of, drawn_prompt, oracle_params, tiny_config  # noqa: E402


def main():
    cfg = tiny_config()
    llama = LlamaRef(cfg, tiny_llama_tensors(cfg, seed=7, quantize=None, groupsize=64))
    for name, requests in SCENARIOS.items():
        for i, r in enumerate(requests):
            bound, params = bound_of(r), oracle_params(r)
            for draw in range(100000):
                kw = dict(prompt=drawn_prompt(r["length"], draw), params=params, seed=draw)
                ids, margins, drawn = ref.oracle_stream(llama, n=TOKENS, bound=bound, **kw)
                if len(ids) < TOKENS or min(margins) < bound or (params["sample"] and sum(drawn) < MIN_DRAWN):
                    continue
                if not params["sample"]:
                    ids8, margins8, _ = _with_e4m3_cache(lambda: ref.oracle_stream(llama, n=TOKENS, bound=bound, **kw))
                    if ids8 != ids or min(margins8) < bound:
                        continue
                    margins = margins + margins8
                print(f"{name}[{i}]: length {r['length']} draw={draw}  bound {bound:.3f}  achieved margin "
                      f"{min(margins):.3f}  tokens the draw decided {sum(drawn)}/{TOKENS}  ids {ids}", flush=True)
                break


if __name__ == "__main__":
    main()
