"""CPU: verifying speculative drafts for sampled and warped requests, the host side.  The law in numpy
(tests/spec_sampled_ref.py: the emitted stream is the plain per-token stream cut behind the first miss, offsets advance by
what was emitted), the chooser's per-row EOS adjustments and its commit against stepping the per-step rule, the option
parser, and the step rule with the option on.  No kernel runs."""
import copy

import numpy as np
import pytest
import torch

from tests import spec_sampled_ref as ref
from tests.test_spec_decode_cpu import _after_prefill, _host_lm
from tests.fixture_utils import FixtureTokenizer, prompt_text
from tgis_amd.models.flash_causal_lm import FlashCausalLM, FlashCausalLMBatch
from tgis_amd.pb import generate_pb2 as pb2
from tgis_amd.utils import spec_decode as sd
from tgis_amd.utils.kv_cache import PagedKVCache
from tgis_amd.utils.tokens import HeterogeneousNextTokenChooser

CPU = torch.device("cpu")
V = 97


def _toy_model(seed):
    """Logits that depend on the whole context: a deterministic function, as a model's forward is."""
    def model(context):
        h = seed
        for t in context:
            h = (h * 1000003 + int(t) + 1) % (1 << 61)
        return (np.random.RandomState(h % (1 << 32)).randn(V) * 2.5).astype(np.float32)
    return model


PARAMS = {
    "sampled": dict(temperature=0.8, sample=1),
    "warped": dict(temperature=1.3, top_k=20, top_p_cut=float(np.float32(1) - np.float32(0.9)), typical_p=0.9, sample=1),
    "greedy-penalty": dict(rep_penalty=1.2),
    "sampled-penalty-eos": dict(temperature=0.7, rep_penalty=1.3, eos_id=5, sample=1),
}


@pytest.mark.parametrize("name", sorted(PARAMS))
@pytest.mark.parametrize("K", [1, 3, 7])
def test_the_emitted_stream_is_the_plain_stream_cut_behind_the_first_miss(name, K):
    params, model, N = PARAMS[name], _toy_model(len(name) + K), 24
    kw = dict(min_new=4, length_penalty=(6, 1.5)) if "eos" in name else {}
    plain = ref.Request(params, [3, 9, 4], seed=77, offset=5, **kw)
    want = [plain.plain_step(model) for _ in range(N + K + 1)]
    spec = ref.Request(params, [3, 9, 4], seed=77, offset=5, **kw)
    rs, got, counts = np.random.RandomState(K), [], []
    while len(got) < N:
        t = len(got)
        drafts = list(want[t:t + K])
        wrong = (K + len(counts)) % (K + 1)  # the first wrong draft; K: none (the first step), then 0, 1, ...
        if wrong < K:
            drafts[wrong] = (drafts[wrong] + 1 + int(rs.randint(0, V - 1))) % V
            if drafts[wrong] == want[t + wrong]:
                drafts[wrong] = (drafts[wrong] + 1) % V
        before = spec.offset
        emitted = spec.verify_step(model, drafts)
        assert len(emitted) == wrong + 1, "accepted up to the first miss, plus the model's own token behind it"
        assert emitted == want[t:t + len(emitted)]
        assert spec.offset - before == (len(emitted) if params.get("sample") else 0)
        got += emitted
        counts.append(len(emitted))
    assert got == want[:len(got)] and max(counts) == K + 1 and min(counts) == 1
    assert spec.context == plain.context[:len(spec.context)]
    if "eos" in name:
        assert 5 not in want[:4], "EOS is masked below min_new_tokens"


def test_k0_is_the_plain_step():
    model = _toy_model(3)
    a = ref.Request(PARAMS["warped"], [1, 2], seed=9)
    b = ref.Request(PARAMS["warped"], [1, 2], seed=9)
    for _ in range(6):
        assert b.verify_step(model, []) == [a.plain_step(model)]
    assert a.offset == b.offset == 6


# ---- the chooser: per-row EOS adjustments and the commit ----------------------------------------------------------------------
def _params(**kw):
    p = pb2.NextTokenChooserParameters()
    for k, v in kw.items():
        if k == "length_penalty":
            p.length_penalty.start_index, p.length_penalty.decay_factor = v
        else:
            setattr(p, k, v)
    return p


def _chooser(current=None):
    ps = [_params(min_new_tokens=3),                                  # met inside the verified rows
          _params(length_penalty=(2, 1.5)),                           # the penalty starts inside them
          _params(temperature=0.8, seed=5),                           # neither: its counter never moves
          _params(min_new_tokens=2, length_penalty=(4, 2.0), temperature=1.1, seed=6),
          _params(min_new_tokens=9)]                                  # not met by any row
    ch = HeterogeneousNextTokenChooser.from_pb(ps, 2, 0, [True] * len(ps), torch.float32, CPU)
    if current is not None:
        ch.current_tokens = list(current)
    return ch


@pytest.mark.parametrize("K", [0, 1, 3, 7])
@pytest.mark.parametrize("current", [[0, 0, 0, 0, 0], [1, 1, 1, 1, 1], [2, 4, 0, 3, 8]])
def test_per_row_eos_adjustments_are_the_per_step_rule_stepped(K, current):
    ch = _chooser(current)
    got = ch._eos_adjustments_verify(K)
    assert ch.current_tokens == list(current), "the verify form steps a copy"
    stepped = copy.deepcopy(ch)
    want = {}
    for j in range(K + 1):
        for idx, adj in stepped._eos_adjustments().items():
            want[idx, j] = adj
    assert got == want
    if K >= 3 and current == [1, 1, 1, 1, 1]:
        assert (0, 1) in got and (0, 2) not in got, "min_new_tokens = 3 is met behind row 1"
        assert (1, 1) not in got and got[1, 2][0] == 2.0, "the length penalty (start 2) begins at row 2"


@pytest.mark.parametrize("n_emit", [[1, 1, 1, 1, 1], [4, 1, 3, 2, 4], [2, 4, 4, 1, 3]])
def test_commit_is_n_emit_steps_of_the_rule_and_of_the_streams(n_emit):
    ch = _chooser([1, 1, 0, 1, 7])
    ch.commit_verify(n_emit)
    for idx, n in enumerate(n_emit):
        one = _chooser([1, 1, 0, 1, 7])
        for _ in range(n):  # request idx took part in n steps
            one._eos_adjustments()
        assert ch.current_tokens[idx] == one.current_tokens[idx]
    assert [s.offset if s else None for s in ch.samplings] == [None, None, n_emit[2], n_emit[3], None]
    assert ch.current_tokens[2] == 0, "a counter only advances below min_new_tokens or with a length penalty"
    # the streams survive filter (prune) and a rebuild from the carried samplings (concatenate)
    ch.filter([2, 3])
    assert [s.offset for s in ch.samplings] == [n_emit[2], n_emit[3]]
    carried = HeterogeneousNextTokenChooser.from_pb([_params(temperature=0.8, seed=5)] * 2, 2, 0, [True] * 2, torch.float32,
                                                    CPU, samplings=ch.samplings, current_tokens=ch.current_tokens)
    assert [s.state[1] for s in carried.samplings] == [n_emit[2], n_emit[3]]


# ---- the option -----------------------------------------------------------------------------------------------------------------
def test_option_from_argument_and_environment(monkeypatch):
    monkeypatch.delenv("TGIS_SPEC_SAMPLING", raising=False)
    assert sd.parse_spec_sampling() is False, "unset: off"
    assert [sd.parse_spec_sampling(v) for v in (True, False, "true", "FALSE", " True ")] == [True, False, True, False, True]
    monkeypatch.setenv("TGIS_SPEC_SAMPLING", "true")
    assert sd.parse_spec_sampling() is True and sd.parse_spec_sampling(False) is False, "the argument wins"
    monkeypatch.setenv("TGIS_SPEC_SAMPLING", "false")
    assert sd.parse_spec_sampling() is False


@pytest.mark.parametrize("bad", ["1", "yes", "", 1, 0.0, "on"])
def test_bad_option_raises(bad, monkeypatch):
    with pytest.raises(ValueError, match="TGIS_SPEC_SAMPLING"):
        sd.parse_spec_sampling(bad)
    monkeypatch.setenv("TGIS_SPEC_SAMPLING", str(bad))
    with pytest.raises(ValueError, match="TGIS_SPEC_SAMPLING"):
        sd.parse_spec_sampling()


class _Engine:
    world_size = 1


def test_the_constructor_checks_the_option_before_anything_else(monkeypatch):
    monkeypatch.delenv("TGIS_SPEC_SAMPLING", raising=False)
    with pytest.raises(ValueError, match="TGIS_SPEC_SAMPLING"):
        FlashCausalLM("x", None, "synthetic", torch.float16, None, engine=_Engine(), spec_tokens=3, spec_sampling="maybe")


def test_the_counter_exists():
    assert "verify_steps_sampled" in sd.SPEC_STATS and sd.new_stats()["verify_steps_sampled"] == 0


# ---- the step rule --------------------------------------------------------------------------------------------------------------
def _sampling_batch(cache, top_n=0):
    reqs = [pb2.Request(id=i, inputs=prompt_text([5, 6, 7]), input_length=3, max_output_length=20) for i in range(2)]
    reqs[1].parameters.temperature = 0.7
    reqs[0].parameters.repetition_penalty = 1.2
    reqs[1].details.top_n_toks = top_n
    s, errs = FlashCausalLMBatch.from_pb(pb2.Batch(id=1, requests=reqs), FixtureTokenizer(4096), torch.float16, CPU, None,
                                         None, True)
    assert not errs and not s.next_token_chooser.is_plain_greedy
    _after_prefill(s, cache)
    s.spec_tokens, s.spec_drafts, s.spec_hits = 3, torch.zeros((2, 3), dtype=torch.int64), torch.ones(2, dtype=torch.int32)
    return s


def test_with_the_option_on_nothing_reports_not_greedy_and_details_still_does():
    c = PagedKVCache(1, 1, 64, 8, torch.float16, CPU)
    off, on = _host_lm(3), _host_lm(3)
    on.spec_sampling = True
    assert off.spec_sampling is False
    s = _sampling_batch(c)
    assert off._grow_for_verify(s) is False and off.spec_stats()["fallback_not_greedy"] == 1
    assert on._grow_for_verify(s) is True
    st = on.spec_stats()
    assert st["fallback_not_greedy"] == 0 and st["verify_steps"] == st["verify_steps_sampled"] == 1
    s.release()
    d = _sampling_batch(c, top_n=2)
    assert on._grow_for_verify(d) is False
    st = on.spec_stats()
    assert st["fallback_details"] == 1 and st["fallback_not_greedy"] == 0 and st["verify_steps_sampled"] == 1
    d.release()
    # the other causes are untouched: no hits, no verify
    m = _sampling_batch(c)
    m.spec_hits = torch.zeros(2, dtype=torch.int32)
    assert on._grow_for_verify(m) is False and on.spec_stats()["fallback_no_match"] == 1
    m.release()
    assert c.free_pages == c.num_pages


# ---- the entry points check their arguments before touching the device ------------------------------------------------------
def test_argument_validation_needs_no_gpu():
    from tgis_amd import native

    lib = native.load_library()
    none6 = [None] * 6
    rc = lib.tgis_warp_sample_verify(None, 0, None, 0, 1, 3, 10, *none6, 0, 0, -1, None, None, -1, None, None, None, None, None,
                                     None)
    assert rc == -1 and b"tgis_warp_sample_verify" in lib.tgis_last_error()
    rc = lib.tgis_spec_accept_sampled(None, None, None, 0, None, None, None, None, None, None, 0, None, None, None, None, None, 1,
                                      None)
    assert rc == -1 and b"tgis_spec_accept_sampled" in lib.tgis_last_error()
    rc = lib.tgis_spec_accept(None, None, None, 0, None, None, None, None, None, None, 0, None, None, None, 1, None)
    assert rc == -1 and b"tgis_spec_accept:" in lib.tgis_last_error(), "the old entry keeps its own name in its message"
    lib.tgis_clear_error()
