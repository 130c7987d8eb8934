"""-m gpu: speculative decoding for sampled and warped requests on the product path
(FlashCausalLM(spec_tokens=3, spec_sampling=True)).

Speculation must change no token: the yardstick is the plain run (option off) of the same requests — a seeded request
emits the stream its plain run emits, whatever was drafted.  The drafts are forced (the Runner / forced-drafts pattern of
tests/test_spec_model_gpu.py): correct, wrong from a chosen index on, or garbage.

The prompts and seeds are drawn on the CPU (tests/golden/make_spec_sampled_prompts.py) so that the fp32 oracle decides every
compared token's race — warped score plus the Gumbel term of `race_choice`, top-1 minus top-2; the warped scores alone for a
greedy request — by at least 2 LOGIT_TOL / T (0.875 at T = 0.8, 0.7 for greedy, 0.84 under the repetition penalty 1.2, which
multiplies a negative logit's error): twice what a whole fp16 step may be off, so an id that differs is an error and not a
near-tie.  Every sampled request has at least one token that the draw decided against the argmax (the tiny model is peaked:
more of them, by this margin, are rare).  Achieved margins, the minimum over a request's TOKENS tokens, per request:
  sampled   1.337, 0.880, 2.317   (also with the e4m3 round trip on the oracle's keys and values, which gives the same ids)
  mixed     4.500 (greedy), 1.032
  penalty   1.194
  min_new   1.910
  joiner    0.877"""
import numpy as np
import pytest
import torch

from oracle.tiny_models import TinyLlamaConfig, tiny_llama_tensors
from tests import spec_sampled_ref as ref
from tests.fixture_utils import FixtureTokenizer, prompt_text
from tests.test_spec_model_gpu import LOGIT_TOL, Runner, _delta, _force

pytestmark = pytest.mark.gpu

K, TOKENS, STEPS, EOS = 3, 13, 3, 2
T = 0.8
# per request: prompt length, the draw the search settled on (prompt number and, for a sampled request, its seed), and its
# parameters.  `tokens`: fewer than TOKENS.  `e4m3`: searched with the quantised cache as well.
SCENARIOS = {
    "sampled": [dict(length=27, draw=14, temperature=T, e4m3=True), dict(length=5, draw=5, temperature=T, e4m3=True),
                dict(length=30, draw=59, temperature=T, e4m3=True)],
    "mixed": [dict(length=12, draw=0), dict(length=9, draw=2, temperature=T)],
    "penalty": [dict(length=20, draw=0, repetition_penalty=1.2)],
    "min_new": [dict(length=11, draw=7, temperature=T, min_new_tokens=3)],
    "joiner": [dict(length=7, draw=3, temperature=T)],
}


def oracle_request(r):
    """A scenario's request as tests/spec_sampled_ref.py `oracle_stream` takes it."""
    params = dict(temperature=r.get("temperature", 1.0), rep_penalty=r.get("repetition_penalty", 1.0), eos_id=EOS,
                  sample=int("temperature" in r))
    return dict(prompt=ref.drawn_prompt(r["length"], r["draw"]), params=params, seed=r["draw"],
                min_new=r.get("min_new_tokens", 0))


def _requests(name, first_id=0, tokens=None):
    from tgis_amd.pb import generate_pb2 as pb2

    out = []
    for i, r in enumerate(SCENARIOS[name]):
        prompt = ref.drawn_prompt(r["length"], r["draw"])
        n = (tokens or {}).get(i, r.get("tokens", TOKENS))
        q = pb2.Request(id=first_id + i, inputs=prompt_text(prompt), input_length=len(prompt), truncate=False,
                        max_output_length=n)
        q.details.logprobs = True
        if "temperature" in r:
            q.parameters.temperature, q.parameters.seed = r["temperature"], r["draw"]
        if "repetition_penalty" in r:
            q.parameters.repetition_penalty = r["repetition_penalty"]
        if "min_new_tokens" in r:
            q.parameters.min_new_tokens = r["min_new_tokens"]
        out.append(q)
    return out


_TENSORS = {}


def _model(spec, sampling=None, kv="auto"):
    from tgis_amd.inference_engine.synthetic import InferenceEngine
    from tgis_amd.models.custom_modeling.flash_llama_modeling import LlamaConfig
    from tgis_amd.models.flash_causal_lm import FlashCausalLM

    cfg = TinyLlamaConfig()
    if not _TENSORS:
        _TENSORS.update(tiny_llama_tensors(cfg, seed=7, quantize=None, groupsize=64))
    tok = FixtureTokenizer(cfg.vocab_size)
    eng = InferenceEngine({k: v.clone() for k, v in _TENSORS.items()}, LlamaConfig(**cfg.to_dict()), torch.float16, None,
                          tokenizer=tok, gptq_groupsize=64)
    lm = FlashCausalLM("fixture", None, "synthetic", torch.float16, None, engine=eng, kv_cache_pages=96, kv_cache_dtype=kv,
                       spec_tokens=spec, spec_sampling=sampling)
    return lm, tok


@pytest.fixture(scope="module")
def models(gpu_device):
    """(plain model: options off, speculating model: spec_tokens = 3 with spec_sampling)."""
    return _model(0), _model(K, True)


_PLAIN = {}


def _plain(models, name):
    """The plain run of a scenario, computed once and left unchanged."""
    if name not in _PLAIN:
        lm0, tok0 = models[0]
        run = Runner(lm0, tok0)
        run.run(run.batch(_requests(name)))
        assert lm0.spec_stats() == dict.fromkeys(lm0.spec_stats(), 0), "option off: nothing is counted"
        _PLAIN[name] = run
    return _PLAIN[name]


def _parting(run, plain, rid, scenario):
    """Where request rid left the plain run's stream, and by how much the fp32 oracle decided that token."""
    t = next((i for i, (a, b) in enumerate(zip(run.ids[rid], plain.ids[rid])) if a != b), None)
    if t is None:
        return "(streams of different length)"
    from oracle.llama_ref import LlamaRef

    cfg = TinyLlamaConfig()
    r = SCENARIOS[scenario][rid]
    ids, margins, _drawn = ref.oracle_stream(LlamaRef(cfg, _TENSORS), n=t + 1, **oracle_request(r))
    return (f"first at token {t}: {run.ids[rid][t]} vs the plain run's {plain.ids[rid][t]} (oracle: {ids[t]}, decided by "
            f"{margins[t]:.3f} in warped-score units)")


def _compare(run, plain, scenario, what, rids=None):
    for rid in (plain.ids if rids is None else rids):
        want = plain.ids[rid]
        assert run.ids[rid] == want, f"{what}: request {rid} {run.ids[rid]} != plain run {want} " \
                                     f"{_parting(run, plain, rid, scenario)}"
        np.testing.assert_allclose(run.lps[rid], plain.lps[rid], atol=LOGIT_TOL, err_msg=f"{what}: request {rid} logprobs")


def _wrong_at(mode, batch, rng):
    if mode == "correct":
        return lambda rid: K
    if mode == "garbage":
        return lambda rid: 0
    picks = {r.id: int(rng.integers(0, K + 1)) for r in batch.requests}  # another index per request and step, K among them
    return picks.__getitem__


def _garbage(batch, run, plain, rng):
    junk = rng.integers(3, 256, size=(len(batch), K))
    for i, r in enumerate(batch.requests):  # (a random id that happens to be the true one would be accepted)
        if int(junk[i, 0]) == plain.ids[r.id][len(run.ids[r.id])]:
            junk[i, 0] += 1
    batch.spec_drafts = torch.from_numpy(junk).to(batch.spec_hits.device)


def _forced_run(lm, tok, plain, scenario, mode, steps=STEPS):
    """`steps` verify steps with forced drafts, then the batch decodes on with its own lookups to the end."""
    run = Runner(lm, tok)
    batch, _ = run.step(run.batch(_requests(scenario)), first=True)
    before = lm.spec_stats()
    rng = np.random.default_rng(5)
    for s in range(steps):
        expect = _force(batch, run, plain, _wrong_at(mode, batch, rng), K)
        if mode == "garbage":
            _garbage(batch, run, plain, rng)
        batch, got = run.step(batch)
        assert got == expect, f"{scenario}/{mode} step {s}: tokens per request {got}, expected {expect}"
    d = _delta(lm, before)
    assert d["verify_steps"] == d["verify_steps_sampled"] == d["decode_steps"] == steps, d
    while batch is not None:
        batch, _ = run.step(batch)
    d = _delta(lm, before)
    assert d["fallback_not_greedy"] == 0, d
    _compare(run, plain, scenario, f"{scenario}/{mode}")
    assert d["emitted"] == sum(len(v) - 1 for v in plain.ids.values())
    assert lm.kv_cache.free_pages == lm.kv_cache.num_pages, "pages leaked"
    return run, d


@pytest.mark.parametrize("mode", ["correct", "mixed", "garbage"])
@pytest.mark.parametrize("scenario", ["sampled", "mixed", "penalty"])
def test_forced_drafts_emit_what_they_must_and_change_no_token(models, scenario, mode):
    """sampled: three requests at temperature 0.8, each its own seed (27, 5 and 30 prompt tokens: the first and the last
    cross a page boundary inside the verified rows).  mixed: a greedy and a sampled request together.  penalty: one greedy
    request with repetition penalty 1.2, whose verify rows must see the drafts in front of them as context."""
    (_lm0, _tok0), (lm, tok) = models
    plain = _plain(models, scenario)
    _run, d = _forced_run(lm, tok, plain, scenario, mode)
    print(f"\n[{scenario} {mode}] {d}")
    B = len(SCENARIOS[scenario])
    if mode == "correct":
        assert d["accepted"] >= STEPS * B * K and d["drafted"] >= STEPS * B * K
    if mode == "garbage":
        assert d["drafted"] >= STEPS * B * K and d["accepted"] <= d["drafted"] - STEPS * B * K


@pytest.mark.parametrize("eos_at", [0, 1, 2])
def test_min_new_tokens_is_met_inside_a_verify_step(models, eos_at):
    """A sampled request with min_new_tokens = 3: its prefill chose token 1, so of the first verify step's rows (tokens 2,
    3, 4, 5) the first two have EOS masked and the others do not.  EOS is forced as the draft at index eos_at (it is not
    the plain run's token there): the step must stop in front of it, with or without the mask on its row."""
    (_lm0, _tok0), (lm, tok) = models
    plain = _plain(models, "min_new")
    assert EOS not in plain.ids[0]
    run = Runner(lm, tok)
    batch, _ = run.step(run.batch(_requests("min_new")), first=True)
    assert batch.next_token_chooser.current_tokens == [1] and not batch.next_token_chooser.is_plain_greedy
    before = lm.spec_stats()
    _force(batch, run, plain, lambda rid: K, K)
    batch.spec_drafts[0, eos_at] = EOS
    batch, got = run.step(batch)
    assert got == {0: eos_at + 1}
    assert batch.next_token_chooser.current_tokens == [min(3, 2 + eos_at)], "the counter stops at min_new_tokens"
    assert batch.next_token_chooser.samplings[0].offset == 2 + eos_at, "one draw per emitted token"
    expect = _force(batch, run, plain, lambda rid: K, K)
    batch, got = run.step(batch)
    assert got == expect
    d = _delta(lm, before)
    assert d["verify_steps_sampled"] == 2 and d["fallback_not_greedy"] == 0, d
    while batch is not None:
        batch, _ = run.step(batch)
    _compare(run, plain, "min_new", f"min_new/eos_at={eos_at}")
    assert lm.kv_cache.free_pages == lm.kv_cache.num_pages


def test_forced_drafts_on_the_e4m3_cache_match_its_plain_run(gpu_device):
    pair = (_model(0, kv="fp8_e4m3"), _model(K, True, kv="fp8_e4m3"))
    assert pair[1][0].kv_cache.is_fp8
    run = Runner(*pair[0])
    run.run(run.batch(_requests("sampled")))
    _forced_run(*pair[1], run, "sampled", "mixed")


def test_streams_survive_a_prune_and_a_concatenate_between_verify_steps(models):
    """Request 1 of `sampled` asks for 5 tokens and is pruned after the first verify step; a fourth sampled request joins
    after the second.  Every stream still equals its plain run: the offset mirrors that prune and concatenate carry over
    were right."""
    (lm0, tok0), (lm, tok) = models
    short = {1: 5}
    plain = Runner(lm0, tok0)
    plain.run(plain.batch(_requests("sampled", tokens=short)))
    plain.run(plain.batch(_requests("joiner", first_id=3)))
    run = Runner(lm, tok)
    batch, _ = run.step(run.batch(_requests("sampled", tokens=short)), first=True)
    before = lm.spec_stats()
    rng = np.random.default_rng(9)
    expect = _force(batch, run, plain, lambda rid: K if rid == 1 else int(rng.integers(0, K + 1)), K)
    batch, got = run.step(batch)  # request 1 has its 5 tokens: the runner prunes it
    assert got == expect and [r.id for r in batch.requests] == [0, 2]
    assert [s.offset for s in batch.next_token_chooser.samplings] == [len(run.ids[0]), len(run.ids[2])]
    expect = _force(batch, run, plain, _wrong_at("mixed", batch, rng), K)
    batch, got = run.step(batch)
    assert got == expect
    joiner, _ = run.step(run.batch(_requests("joiner", first_id=3), batch_id=2), first=True)
    with lm.context_manager():
        batch = lm.batch_type.concatenate([batch, joiner])
    assert [s.offset for s in batch.next_token_chooser.samplings] == [len(run.ids[r.id]) for r in batch.requests]
    expect = _force(batch, run, plain, _wrong_at("mixed", batch, rng), K)
    batch, got = run.step(batch)
    assert got == expect
    d = _delta(lm, before)
    assert d["verify_steps_sampled"] == 3 and d["fallback_not_greedy"] == 0, d
    while batch is not None:
        batch, _ = run.step(batch)
    _compare(run, plain, "sampled", "prune + concatenate", rids=[0, 1, 2])
    assert run.ids[3] == plain.ids[3], f"the joiner: {run.ids[3]} != {plain.ids[3]}"
    assert lm.kv_cache.free_pages == lm.kv_cache.num_pages


def test_with_the_option_off_a_sampled_batch_stays_on_the_plain_step(models):
    """spec_tokens = 3 alone: every decode step of the same sampled batch reports fallback_not_greedy, and is the plain run."""
    lm, tok = _model(K)
    assert lm.spec_sampling is False
    plain = _plain(models, "sampled")
    run = Runner(lm, tok)
    run.run(run.batch(_requests("sampled")))
    st = lm.spec_stats()
    assert st["decode_steps"] == TOKENS - 1 == st["fallback_not_greedy"] and st["verify_steps"] == 0, st
    assert st["verify_steps_sampled"] == 0 and st["drafted"] == 0
    assert run.ids == plain.ids and run.lps == plain.lps, "the plain step of a speculating model is the plain step"

