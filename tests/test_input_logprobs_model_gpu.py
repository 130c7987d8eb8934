"""-m gpu: details.input_toks through FlashCausalLM with fused_input_logprobs off and on, on the tiny Llama checkpoint of
tests/test_model_gpu.py: same generated tokens, same prompt-token messages (ranks wherever the off path's own margin is
clear, logprobs within twice the fixture's logit tolerance: a logprob is a difference of two logits-sized quantities).
The prompts hold 31 rows in all: lm_head over all rows (off) and over the four last rows (on) then run the same GEMM plan,
whose rows do not depend on one another, so the generated tokens' logprobs are the same bits (across plans they agree as
the logprobs of any two batch sizes do)."""
import math

import pytest
import torch

from oracle.tiny_models import TinyLlamaConfig, tiny_llama_tensors
from tests.fixture_utils import FixtureTokenizer
from tests.test_model_gpu import LOGIT_TOL, _from_pb, _pb

pytestmark = pytest.mark.gpu

DTYPE = torch.float16
LENS = (7, 12, 9, 3)  # three prompts with input_toks, one without


@pytest.fixture(scope="module")
def models(gpu_device):
    from tgis_amd.inference_engine.synthetic import InferenceEngine
    from tgis_amd.models.custom_modeling.flash_llama_modeling import LlamaConfig
    from tgis_amd.models.flash_causal_lm import FlashCausalLM

    cfg = TinyLlamaConfig()
    tensors = tiny_llama_tensors(cfg, seed=11)
    tok = FixtureTokenizer(cfg.vocab_size)

    def build(fused):
        eng = InferenceEngine({k: v.clone() for k, v in tensors.items()}, LlamaConfig(**cfg.to_dict()), DTYPE, None,
                              tokenizer=tok)
        return FlashCausalLM("fixture", None, "synthetic", DTYPE, None, engine=eng, kv_cache_pages=32,
                             fused_input_logprobs=fused)

    return build(False), build(True), tok


def _batch_pb(top_n=0):
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(3, 256, (n,), generator=g).tolist() for n in LENS]
    pb = _pb(prompts, max_new=3, ranks=True)
    for r in pb.requests[:3]:
        r.details.input_toks = True
    pb.requests[1].details.top_n_toks = top_n
    return pb


def _run(lm, tok, pb, monkeypatch):
    """(generated TokenInfos, InputTokens, the prefill's logits, head_logprobs calls)."""
    from tgis_amd import native

    calls, rows = [], []
    orig, orig_new = native.head_logprobs, lm._process_new_tokens
    monkeypatch.setattr(native, "head_logprobs", lambda *a: calls.append(1) or orig(*a))
    monkeypatch.setattr(lm, "_process_new_tokens",
                        lambda batch, out, *a: rows.append(out.float().cpu()) or orig_new(batch, out, *a))
    batch = _from_pb(lm, tok, pb)
    with lm.context_manager():
        toks, inputs, errs, _ = lm.generate_token(batch, first=True)
        lm.generate_token(batch)
    batch.release()
    assert not errs
    return toks, inputs, rows[0], len(calls)


def test_fused_input_tokens_match_the_logits_path(models, monkeypatch):
    off, on, tok = models
    pb = _batch_pb()
    toks0, in0, logits, calls0 = _run(off, tok, pb, monkeypatch)
    toks1, in1, last_rows, calls1 = _run(on, tok, pb, monkeypatch)
    assert (calls0, calls1, logits.shape[0], last_rows.shape[0]) == (0, 1, sum(LENS), 4)  # lm_head on the last rows alone
    assert [(t.request_id, t.token_id, t.logprob, t.rank) for t in toks0] == \
        [(t.request_id, t.token_id, t.logprob, t.rank) for t in toks1]
    assert [m.request_id for m in in0] == [m.request_id for m in in1] == [0, 1, 2]
    start = 0
    for m0, m1, n in zip(in0, in1, LENS):
        assert [t.token_id for t in m0.tokens] == [t.token_id for t in m1.tokens] and len(m1.tokens) == n
        assert all(math.isnan(m.tokens[0].logprob) and m.tokens[0].rank == 0 for m in (m0, m1))
        for j in range(1, n):
            a, b = m0.tokens[j], m1.tokens[j]
            assert abs(a.logprob - b.logprob) <= 2 * LOGIT_TOL[DTYPE]
            row = logits[start + j - 1]
            near = int(((row - row[a.token_id]).abs() <= 2 * LOGIT_TOL[DTYPE]).sum()) - 1
            assert abs(a.rank - b.rank) <= near  # equal wherever no other logit lies within the tolerance of the token's
        start += n


def test_top_n_per_position_keeps_the_logits_path(models, monkeypatch):
    off, on, tok = models
    pb = _batch_pb(top_n=2)
    _t0, in0, _r0, calls0 = _run(off, tok, pb, monkeypatch)
    _t1, in1, _r1, calls1 = _run(on, tok, pb, monkeypatch)
    assert (calls0, calls1, len(in0)) == (0, 0, 3) and all(t.top_tokens for t in in0[1].tokens[1:])
    assert repr(in0) == repr(in1)  # (every field of every token; NaN prints as nan on both sides)
