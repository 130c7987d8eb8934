"""CPU: the MLP speculator drafter on the host (utils/mlp_speculator.py and what FlashCausalLM does with it): the options
and every refusal, the tensor-name table with and without the `speculator.` prefix, tied weights as aliases, the step rule
for hits that are all ones, the constants, and the fp64 restatement (tests/spec_mlp_ref.py) on a speculator whose answers
are known by construction.  No kernel runs."""
import math

import numpy as np
import pytest
import torch

from tests import spec_mlp_ref as ref
from tgis_amd.models.flash_causal_lm import FlashCausalLM
from tgis_amd.utils import mlp_speculator as ms
from tgis_amd.utils import spec_decode as sd


def _ckpt(tmp_path, spec=None, name="spec", **kw):
    spec = spec or ref.make_random(16, 24, 40, 3, seed=1)
    return ref.write_checkpoint(str(tmp_path / name), spec, **kw)


# ---- options ------------------------------------------------------------------------------------------------------------------
def test_the_speculator_option_from_argument_and_environment(monkeypatch, tmp_path):
    monkeypatch.delenv("TGIS_SPECULATOR", raising=False)
    assert ms.parse_speculator() is None and ms.parse_speculator("") is None, "unset: the lookup drafter"
    assert ms.parse_speculator("/a/b") == "/a/b" and ms.parse_speculator(tmp_path) == str(tmp_path)
    monkeypatch.setenv("TGIS_SPECULATOR", "/from/env")
    assert ms.parse_speculator() == "/from/env" and ms.parse_speculator("/arg") == "/arg", "the argument wins"
    monkeypatch.setenv("TGIS_SPECULATOR", " ")
    assert ms.parse_speculator() is None
    with pytest.raises(ValueError, match="TGIS_SPECULATOR"):
        ms.parse_speculator(3)


def test_spec_tokens_must_fit_the_speculator(tmp_path):
    cfg = ms.open_checkpoint(_ckpt(tmp_path)).cfg
    assert cfg.n_predict == 3
    for k in (1, 2, 3):
        ms.check_spec_tokens(cfg, k)
    with pytest.raises(ValueError, match=r"speculator.*spec_tokens|spec_tokens.*speculator"):
        ms.check_spec_tokens(cfg, 0)
    with pytest.raises(ValueError, match=r"spec_tokens.*speculator.*n_predict = 3"):
        ms.check_spec_tokens(cfg, 4)
    wide = ms.SpeculatorConfig(64, 64, 256, 9)
    ms.check_spec_tokens(wide, 7)
    with pytest.raises(ValueError, match=r"1 \.\. 7"):
        ms.check_spec_tokens(wide, 8)


def test_config_fields(tmp_path):
    cfg = ms.open_checkpoint(_ckpt(tmp_path, ref.make_random(16, 16, 40, 2, seed=1, scale=True), inner_dim_zero=True)).cfg
    assert (cfg.emb_dim, cfg.inner_dim, cfg.vocab_size, cfg.n_predict) == (16, 16, 40, 2), "inner_dim 0 means emb_dim"
    assert cfg.scale_input and not cfg.tie_weights
    plain = ms.SpeculatorConfig.from_dict(dict(emb_dim=8, vocab_size=5, n_predict=1))
    assert plain.inner_dim == 8 and not plain.scale_input and not plain.tie_weights, "the optional fields default to off"
    with pytest.raises(ValueError, match="n_predict"):
        ms.SpeculatorConfig.from_dict(dict(emb_dim=8, vocab_size=5))
    with pytest.raises(ValueError, match="positive"):
        ms.SpeculatorConfig.from_dict(dict(emb_dim=8, vocab_size=5, n_predict=0))


def test_base_model_mismatches_are_refused(tmp_path):
    cfg = ms.open_checkpoint(_ckpt(tmp_path)).cfg
    ms.check_base(cfg, 16, 40)
    with pytest.raises(ValueError, match="emb_dim 16 != the base model's hidden size 64"):
        ms.check_base(cfg, 64, 40)
    with pytest.raises(ValueError, match="vocab_size 40 != the base model's vocab_size 256"):
        ms.check_base(cfg, 16, 256)


@pytest.mark.parametrize("E,I", [(12, 24), (16, 20), (16, 16392)])
def test_sizes_the_kernels_cannot_serve_are_refused_by_the_loader(E, I):
    with pytest.raises(ValueError, match="multiples of 8|exceeds"):
        ms.check_shapes(ms.SpeculatorConfig(E, I, 40, 2))


def test_a_checkpoint_with_bad_sizes_is_refused_when_opened(tmp_path):
    with pytest.raises(ValueError, match="multiples of 8"):
        ms.open_checkpoint(_ckpt(tmp_path, ref.make_random(12, 24, 40, 2, seed=1)))


def test_missing_files_and_tensors_are_refused(tmp_path):
    with pytest.raises(ValueError, match="config.json not found"):
        ms.open_checkpoint(str(tmp_path / "nothing"))
    spec = ref.make_random(16, 24, 40, 3, seed=1)
    del spec.t["ln.2.bias"], spec.t["emb.1.weight"]
    with pytest.raises(ValueError, match=r"lacks \['emb.1.weight', 'ln.2.bias'\]"):
        ms.open_checkpoint(_ckpt(tmp_path, spec))
    spec = ref.make_random(16, 24, 40, 2, seed=1)
    spec.t["proj.1.weight"] = spec.t["proj.1.weight"][:, :16]
    with pytest.raises(ValueError, match=r"proj.1.weight has shape \(24, 16\), head 1 needs \(24, 24\)"):
        ms.open_checkpoint(_ckpt(tmp_path, spec, name="shape"))


class _Engine:
    def __init__(self, world_size, config=None):
        self.world_size = world_size
        if config is not None:
            self._config = config


class _Base:
    hidden_size, vocab_size = 64, 256


def test_the_constructor_refuses_before_anything_is_loaded(monkeypatch, tmp_path):
    """Every refusal comes before the GPU is looked at (on a machine without one a good set of options gets as far as
    NotImplementedError: FlashCausalLM is only available on GPU)."""
    monkeypatch.delenv("TGIS_SPEC_TOKENS", raising=False)
    monkeypatch.delenv("TGIS_SPECULATOR", raising=False)
    path = _ckpt(tmp_path)
    new = (lambda **kw: FlashCausalLM("x", None, "synthetic", torch.float16, None, **kw))
    with pytest.raises(ValueError, match=r"speculator.*spec_tokens"):
        new(engine=_Engine(1), speculator=path)  # spec_tokens unset = 0
    with pytest.raises(ValueError, match=r"speculator.*spec_tokens"):
        new(engine=_Engine(1), speculator=path, spec_tokens=0)
    with pytest.raises(ValueError, match=r"spec_tokens.*speculator"):
        new(engine=_Engine(1), speculator=path, spec_tokens=4)
    with pytest.raises(ValueError, match="emb_dim 16 != the base model's hidden size 64"):
        new(engine=_Engine(1, _Base), speculator=path, spec_tokens=3)
    with pytest.raises(NotImplementedError, match="tensor parallelism is out of scope"):
        new(engine=_Engine(2), speculator=path, spec_tokens=3)
    with pytest.raises(ValueError, match="config.json not found"):
        new(engine=_Engine(1), speculator=str(tmp_path / "nowhere"), spec_tokens=3)
    monkeypatch.setenv("TGIS_SPECULATOR", path)
    monkeypatch.setenv("TGIS_SPEC_TOKENS", "5")
    with pytest.raises(ValueError, match="n_predict = 3"):
        new(engine=_Engine(1))
    if not torch.cuda.is_available():
        monkeypatch.setenv("TGIS_SPEC_TOKENS", "3")
        with pytest.raises(NotImplementedError, match="only available on GPU"):
            new(engine=_Engine(1))


# ---- names and tying ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix", ["", "speculator."])
def test_names_map_with_and_without_the_prefix(tmp_path, prefix):
    ck = ms.open_checkpoint(_ckpt(tmp_path, prefix=prefix))
    assert len(ck.names) == 3
    for i, head in enumerate(ck.names):
        assert head == {"emb": f"{prefix}emb.{i}.weight", "proj": f"{prefix}proj.{i}.weight",
                        "head": f"{prefix}head.{i}.weight", "ln_weight": f"{prefix}ln.{i}.weight",
                        "ln_bias": f"{prefix}ln.{i}.bias"}
    spec = ref.make_random(16, 24, 40, 3, seed=1)
    got = ck.load(prefix + "proj.2.weight")
    assert got.dtype == torch.float16 and np.array_equal(got.float().numpy(), spec.t["proj.2.weight"].astype(np.float32))


def test_the_name_table_is_one_small_table():
    assert set(ms.TENSOR_NAMES) == {"emb", "proj", "head", "ln_weight", "ln_bias"} and ms.PREFIXES == ("", "speculator.")
    assert ms.resolve_names({"speculator.emb.0.weight", "proj.0.weight", "head.0.weight", "ln.0.weight", "ln.0.bias"},
                            ms.SpeculatorConfig(8, 8, 5, 1))[0]["emb"] == "speculator.emb.0.weight"


@pytest.mark.parametrize("once", [True, False], ids=["stored-once", "repeated"])
def test_tied_weights_resolve_to_aliases(tmp_path, once):
    spec = ref.make_random(16, 24, 40, 4, seed=2, tie_weights=True)
    ck = ms.open_checkpoint(_ckpt(tmp_path, spec, store_tied_once=once))
    assert ck.cfg.tie_weights
    for kind in ("emb", "head", "ln_weight", "ln_bias"):
        assert {h[kind] for h in ck.names} == {ms.TENSOR_NAMES[kind].format(i=0)}, "index 0 serves every head"
    assert [h["proj"] for h in ck.names] == ["proj.0.weight", "proj.1.weight", "proj.1.weight", "proj.1.weight"]
    # whoever loads by name loads each distinct tensor once: 4 + 2 of them, not 5 per head
    assert len({n for h in ck.names for n in h.values()}) == 6


# ---- the step rule ------------------------------------------------------------------------------------------------------------
def test_hits_that_are_all_ones_never_answer_no_match():
    for K in (1, 3, 7):
        ones = [1] * 4
        assert sd.fallback_cause(K, 4, True, False, [K + 1] * 4, ones) is None
        assert sd.fallback_cause(K, 4, True, False, [K + 1] * 4, lambda: ones) is None
        assert sd.fallback_cause(K, 4, False, False, [K + 1] * 4, ones) == "not_greedy"
        assert sd.fallback_cause(K, 4, True, True, [K + 1] * 4, ones) == "details"
        assert sd.fallback_cause(K, 64, True, False, [K + 1] * 4, ones) == "rows"
        assert sd.fallback_cause(K, 4, True, False, [K + 1, K, 9, 9], ones) == "remaining"
    assert sd.fallback_cause(3, 4, True, False, [9] * 4, [0] * 4) == "no_match", "(the lookup's answer, for contrast)"


# ---- constants and the restatement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,state_weight", [(3, 0.8908987181403393), (4, 0.9170040432046712), (5, 0.9330329915368074)])
def test_constants(P, state_weight):
    """state_weight = 2^(-1 / 2P): P heads of it halve the state's share of the variance."""
    for I in (64, 4096):
        sw, ew, alpha = ms.constants(P, I)
        assert sw == pytest.approx(state_weight, rel=1e-15) and sw ** (2 * P) == pytest.approx(0.5, rel=1e-14)
        assert ew == pytest.approx(math.sqrt((1 - state_weight ** 2) * I / 2), rel=1e-14)
        assert alpha == pytest.approx(ew / sw, rel=1e-15)
        assert (sw, ew, alpha) == pytest.approx(ref.constants(P, I), rel=1e-15)
    assert ms.EPS == ref.EPS == 1e-6


def test_the_restatement_on_the_successor_speculator():
    V, P = 40, 3
    spec = ref.make_successor(16, V, P)
    h = np.random.default_rng(0).standard_normal((5, 16))
    t = np.array([0, 1, 17, 38, 39])
    drafts, margins = spec.draft(h, t, P)
    assert drafts.tolist() == [ref.successor_drafts(x, P, V) for x in t] == [
        [1, 3, 6], [2, 4, 7], [18, 20, 23], [39, 1, 4], [0, 2, 5]]
    assert np.allclose(margins, math.sqrt(V), rtol=1e-4), "a normed one-hot against zeros"


def test_the_restatement_by_hand():
    """One head, I = 2, written out: s = proj h + alpha emb[t]; u = s / rms(s) * w + b; x = gelu(u); argmax(head x)."""
    spec = ref.Speculator(dict(emb_dim=2, inner_dim=2, vocab_size=2, n_predict=1), {
        "proj.0.weight": [[1.0, 0.0], [0.0, 2.0]], "emb.0.weight": [[0.0, 0.0], [1.0, -1.0]],
        "ln.0.weight": [1.0, 0.5], "ln.0.bias": [0.0, 0.25], "head.0.weight": [[1.0, 0.0], [0.0, 1.0]]})
    alpha = ref.constants(1, 2)[2]
    assert alpha == pytest.approx(1.0)  # P = 1, I = 2: state_weight^2 = 1/2, emb_weight^2 = I / 4 = 1/2
    s = np.array([3.0 + alpha, 2.0 * -1.0 - alpha])
    n = s / math.sqrt((s * s).mean() + 1e-6)
    u = n * [1.0, 0.5] + [0.0, 0.25]
    x = [0.5 * v * (1 + math.erf(v / math.sqrt(2))) for v in u]
    drafts, margins = spec.draft([[3.0, -1.0]], [1], 1)
    assert drafts.tolist() == [[0]] and margins[0, 0] == pytest.approx(x[0] - x[1], rel=1e-12)
    # scale_input: the state is normed (no parameters) and divided by sqrt(2) first
    got = ref.scale_input([[3.0, -4.0]])
    assert got == pytest.approx(np.array([[3.0, -4.0]]) / math.sqrt(12.5 + 1e-6) / math.sqrt(2))


def test_the_model_tests_speculator_decides_most_chains_clearly():
    """tests/test_spec_mlp_model_gpu.py compares drafts with the restatement wherever the restatement decides every head of
    a chain by >= 0.35 logits, and fails if more than a quarter of the chains fall under that margin.  Its seed is picked
    here, on the CPU: on unit-variance stand-in states the restatement alone stays within that share."""
    from tests.test_spec_mlp_model_gpu import LOGIT_TOL, UNDECIDED_SHARE, WIDE_HEAD_STD, WIDE_INNER, WIDE_SEED, E, V

    spec = ref.make_random(E, WIDE_INNER, V, 3, seed=WIDE_SEED, head_std=WIDE_HEAD_STD)
    rng = np.random.default_rng(0)
    h, t = rng.standard_normal((400, E)), rng.integers(0, V, 400)
    _, margins = spec.draft(h, t, 3)
    undecided = float((margins.min(1) < LOGIT_TOL).mean())
    print(f"\n[spec mlp] stand-in states: {undecided:.3f} of the chains have a head under {LOGIT_TOL} logits; "
          f"median margin {np.median(margins):.2f}")
    assert undecided <= UNDECIDED_SHARE
