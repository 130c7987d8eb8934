"""-m gpu: the fused sampler (`tgis_warp_sample`, `tgis_warp_sample_verify`, through the C ABI with both row strides) on the
inputs it gets in production and at its edges — tests/sampler_cases.py: tied f16 / bf16 logits, both zeros, rows of -inf,
every V at which a lane, the block or the kernel changes, context ids it must skip, contexts longer than the block —
against the group-wise fp64 reference of tests/sampler_sets_ref.py, which decides ties per group of equal values as the
header of csrc/sampler.hip says the kernel does.  tests/test_sampler_ties_cpu.py pins that reference to the existing
oracle and checks that no case is a photo finish, so every bar below is exact or this project's existing one:

  - the -inf pattern of the warped scores equals the reference's exactly; surviving scores rtol / atol 1e-6; lse and the
    chosen logprob 1e-5 max(1, |lse|); the greedy id is the lowest index of the maximum;
  - logits sit in a buffer 7 columns wider, scores go into a NaN-filled buffer with ld = V + 5 and 2 extra rows, the small
    outputs have 2 sentinel entries past row B: padding stays as it was, the logits are unchanged, a second call returns
    identical bits;
  - sampled rows: the drawn id equals oracle.sampler_ref.race_choice over the kernel's own warped scores whenever the race
    margin is above 1e-3 (V = 1025, 2049: elements beyond a thread's first are drawn; one stream crosses offset 2^32);
    4096 streams over a tied bf16 row follow the fp64 softmax of the surviving set (chi-square, 11 degrees of freedom);
  - the verify form against the same reference directly: row (b, j) is request b's plain step with the context extended by
    drafts[b][:j]; the streams are only read;
  - the global-row kernel (one fresh child process with TGIS_SAMPLER_GLOBAL_ROWS=1, all cases with V <= 32768) returns the
    register kernel's bits in every output of every case."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowwise_cases as rc  # noqa: E402
import sampler_cases as sc  # noqa: E402
import sampler_sets_ref as ssr  # noqa: E402
from oracle import sampler_ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -7
OUTPUTS = ("ids", "logprob", "lse", "scores", "rng")


@pytest.fixture(scope="module")
def lib(gpu_device):
    from tgis_amd import native

    return native.load_library()


def _p(t):
    return None if t is None else t.data_ptr()


def _launch(lib, d, rows, rng=None, verify=False):
    """One launch of a built case on fresh buffers.  `rows` are the per-request parameters ([B]); the plain form has one
    row per request, the verify form VERIFY_K + 1.  Returns the whole buffers, padding included."""
    from tgis_amd import native

    logits = d["logits"]
    R, V = logits.shape
    B = len(rows)

    def col(name, default, dtype):
        if all(name not in r for r in rows):
            return None
        return torch.tensor([r.get(name, default) for r in rows], dtype=dtype, device=DEV)

    eos = None
    if any("eos" in r for r in rows):
        per_row = [r.get("eos", (0.0, 0.0)) for r in rows for _ in range(R // B)]
        eos = torch.tensor(per_row, dtype=torch.float32, device=DEV)
    lbuf = torch.full((R, V + sc.LD_LOGITS_PAD), float("nan"), dtype=torch.float32, device=DEV)
    lbuf[:, :V] = torch.from_numpy(logits).to(DEV)
    before = lbuf.clone()
    sbuf = torch.full((R + sc.PAD_ROWS, V + sc.LD_SCORES_PAD), float("nan"), dtype=torch.float32, device=DEV)
    ids_out = torch.full((R + sc.PAD_ROWS,), SENTINEL, dtype=torch.int64, device=DEV)
    lp = torch.full((R + sc.PAD_ROWS,), float("nan"), dtype=torch.float32, device=DEV)
    lse = torch.full((R + sc.PAD_ROWS,), float("nan"), dtype=torch.float32, device=DEV)
    ctx = torch.from_numpy(d["ids"]).to(DEV) if d["use_ids"] else None
    pen = col("rep_penalty", 1.0, torch.float32) if d["use_ids"] else None
    head = (_p(lbuf), lbuf.stride(0), _p(sbuf), sbuf.stride(0), B)
    params = (col("temperature", 1.0, torch.float32), col("top_k", 0, torch.int32), col("top_p_cut", 0.0, torch.float32),
              col("typical_p", 1.0, torch.float32), pen)
    do_sample = col("sample", 0, torch.int32)
    ld_ids = ctx.stride(0) if ctx is not None else 0
    L = d["L"] if ctx is not None else 0
    tail = (_p(eos), d["eos_id"], _p(do_sample), _p(rng), _p(ids_out), _p(lp), _p(lse), native._stream())
    if verify:
        drafts = torch.from_numpy(d["drafts"]).to(DEV)
        r = lib.tgis_warp_sample_verify(*head, sc.VERIFY_K, V, *[_p(t) for t in params], _p(ctx), ld_ids, L, d["exclude_id"],
                                        _p(drafts), *tail)
    else:
        r = lib.tgis_warp_sample(*head, V, *[_p(t) for t in params], _p(ctx), ld_ids, L, d["exclude_id"], *tail)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # a GPU fault: nothing more may run on this device
        pytest.exit(f"tgis_warp_sample faulted: {e}", returncode=3)
    assert r == 0, lib.tgis_last_error().decode()
    assert torch.equal(lbuf.view(torch.int32), before.view(torch.int32)), "the logits buffer was written"
    return dict(ids=ids_out, logprob=lp, lse=lse, scores=sbuf, rng=rng)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _check_padding(out, R, V, what):
    assert torch.isnan(out["scores"][R:]).all() and torch.isnan(out["scores"][:, V:]).all(), f"{what}: scores padding written"
    assert (out["ids"][R:] == SENTINEL).all() and torch.isnan(out["logprob"][R:]).all() and torch.isnan(out["lse"][R:]).all(), \
        f"{what}: an output past the last row was written"


def _check_same(a, b, what):
    for name in OUTPUTS:
        if a[name] is not None:
            assert torch.equal(_bits(a[name]), _bits(b[name])), f"{what}: {name} differs"


def _check_row(got, want, what):
    """-inf pattern exact, survivors to 1e-6; returns the fp64 lse of the reference row."""
    assert not np.isnan(got).any(), f"{what}: NaN in the warped scores"
    gone_g, gone_w = np.isneginf(got), np.isneginf(want)
    if not np.array_equal(gone_g, gone_w):
        only_k, only_r = np.nonzero(~gone_g & gone_w)[0], np.nonzero(gone_g & ~gone_w)[0]
        raise AssertionError(
            f"{what}: kept {int((~gone_g).sum())} vs reference {int((~gone_w).sum())}; kept by the kernel only "
            f"{only_k[:4].tolist()} (values {np.unique(got[only_k])[:4].tolist()}), by the reference only {only_r[:4].tolist()} "
            f"(values {[repr(float(v)) for v in np.unique(want[only_r])[:4]]})")
    keep = ~gone_w
    np.testing.assert_allclose(got[keep], want[keep], rtol=1e-6, atol=1e-6, err_msg=what)
    return ssr.lse64(want)


def _check_greedy_case(out, refs, V, what):
    R = len(refs)
    _check_padding(out, R, V, what)
    scores = out["scores"][:R, :V].cpu().numpy()
    ids, lps, lses = out["ids"][:R].cpu().numpy(), out["logprob"][:R].cpu().numpy(), out["lse"][:R].cpu().numpy()
    for b, (want, _) in enumerate(refs):
        lse = _check_row(scores[b], want, f"{what} row {b}")
        assert ids[b] == int(np.argmax(want)), f"{what} row {b}: id {ids[b]}, the lowest index of the maximum is {np.argmax(want)}"
        assert abs(lses[b] - lse) < 1e-5 * max(1.0, abs(lse)), f"{what} row {b}: lse {lses[b]} vs {lse}"
        assert abs(lps[b] - (float(want[ids[b]]) - lse)) < 1e-5 * max(1.0, abs(lse)), f"{what} row {b}: logprob"


def _run_filter_case(lib, c):
    d, refs = sc.reference(c)
    out = _launch(lib, d, c["rows"])
    _check_greedy_case(out, refs, c["V"], c["id"])
    _check_same(out, _launch(lib, d, c["rows"]), c["id"] + ": second call")


@pytest.mark.parametrize("family,V", sc.GROUPS, ids=[f"{f}-V{V}" for f, V in sc.GROUPS])
def test_filtered_sets_and_values(lib, family, V):
    assert rc.query(lib, "sampler", V)[0] == int(V <= 32768)
    for c in sc.group(family, V):
        _run_filter_case(lib, c)


def test_wide_vocabulary_on_the_global_row_kernel(lib):
    assert rc.query(lib, "sampler", sc.V_GLOBAL)[0] == 0
    _run_filter_case(lib, sc.GLOBAL_CASE)


# ---- sampled rows ------------------------------------------------------------------------------------------------------------
def _draw_rng():
    return torch.tensor([[s, o] for s, o in zip(sc.DRAW_SEEDS, sc.DRAW_OFFSETS)], dtype=torch.int64, device=DEV)


def _draw_runs(lib, V):
    """Two consecutive draws of the draw case at V: [outputs of call 0, outputs of call 1] (rng cloned after each call)."""
    c = sc.draw_case(V)
    d = sc.build(c)
    rng = _draw_rng()
    outs = []
    for _ in range(2):
        out = _launch(lib, d, c["rows"], rng=rng)
        outs.append(dict(out, rng=rng.clone()))
    return c, outs


@pytest.mark.parametrize("V", sc.DRAW_V)
def test_draws_follow_the_philox_race(lib, V):
    c, outs = _draw_runs(lib, V)
    B = sc.DRAW_B
    exact = compared = 0
    for draw, out in enumerate(outs):
        _check_padding(out, B, V, f"{c['id']} draw {draw}")
        scores, ids = out["scores"][:B, :V].cpu().numpy(), out["ids"][:B].cpu().numpy()
        lps, lses = out["logprob"][:B].cpu().numpy(), out["lse"][:B].cpu().numpy()
        for b, r in enumerate(c["rows"]):
            lse = ssr.lse64(scores[b])
            assert abs(lses[b] - lse) < 1e-5 * max(1.0, abs(lse))
            assert abs(lps[b] - (float(scores[b][ids[b]]) - lse)) < 1e-5 * max(1.0, abs(lse))
            if not r.get("sample"):
                assert ids[b] == int(np.argmax(scores[b]))
                continue
            want, margin = sampler_ref.race_choice(scores[b], sc.DRAW_SEEDS[b] & 0xFFFFFFFFFFFFFFFF, sc.DRAW_OFFSETS[b] + draw)
            compared += 1
            if margin > 1e-3:
                assert ids[b] == want, f"{c['id']} row {b} draw {draw}: drew {ids[b]}, the race gives {want}"
                exact += 1
            assert not np.isneginf(scores[b][ids[b]])
    assert compared == 14 and exact >= 0.8 * compared
    first, second = outs[0]["rng"].cpu().tolist(), outs[1]["rng"].cpu().tolist()
    for b, r in enumerate(c["rows"]):
        step = 1 if r.get("sample") else 0
        seed = sc.DRAW_SEEDS[b]
        assert first[b] == [seed, sc.DRAW_OFFSETS[b] + step] and second[b] == [seed, sc.DRAW_OFFSETS[b] + 2 * step]
    assert first[2][1] == 2 ** 32  # the second draw of stream 2 ran with a non-zero high counter word


def test_draws_over_a_tied_row_are_distributed_as_softmax(lib):
    V, B = sc.CHI2_V, sc.CHI2_B
    row = sc.chi2_row()
    rows = [dict(top_k=sc.CHI2_K, sample=1)] * B
    d = dict(logits=np.tile(row, (B, 1)), use_ids=False, L=0, eos_id=-1, exclude_id=-1)
    rng = torch.tensor([[b * 7919 + 1, 0] for b in range(B)], dtype=torch.int64, device=DEV)
    out = _launch(lib, d, rows, rng=rng)
    _check_padding(out, B, V, "chi-square")
    want = ssr.top_k_filter(row, sc.CHI2_K)
    p = np.exp(want.astype(np.float64) - want.max())
    p /= p.sum()
    counts = np.bincount(out["ids"][:B].cpu().numpy(), minlength=V)
    assert counts[p == 0].sum() == 0, "a draw outside the surviving set"
    live = p > 0
    assert live.sum() == 12
    chi2 = (((counts - B * p) ** 2)[live] / (B * p[live])).sum()
    print(f"chi2 = {chi2:.2f}")
    assert chi2 < 33.0  # 11 degrees of freedom: P(chi2 > 33) < 6e-4


# ---- the verify form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,V", sc.VERIFY_CASES, ids=[f"{f}-V{V}" for f, V in sc.VERIFY_CASES])
def test_verify_rows_equal_the_plain_step_of_their_position(lib, family, V):
    c = sc.verify_case(family, V)
    d, refs = sc.verify_reference(c)
    K1, R = sc.VERIFY_K + 1, 2 * (sc.VERIFY_K + 1)
    seeds, offsets = [41, (1 << 40) + 5], [3, 2 ** 32 - 2]
    rng = torch.tensor([[s, o] for s, o in zip(seeds, offsets)], dtype=torch.int64, device=DEV)
    rng0 = rng.clone()
    out = _launch(lib, d, c["rows"], rng=rng, verify=True)
    assert torch.equal(rng, rng0), "the verify form wrote the streams"
    _check_padding(out, R, V, c["id"])
    scores = out["scores"][:R, :V].cpu().numpy()
    ids, lps, lses = out["ids"][:R].cpu().numpy(), out["logprob"][:R].cpu().numpy(), out["lse"][:R].cpu().numpy()
    for r, (want, _) in enumerate(refs):
        b, j = divmod(r, K1)
        what = f"{c['id']} request {b} row {j}"
        lse = _check_row(scores[r], want, what)
        assert abs(lses[r] - lse) < 1e-5 * max(1.0, abs(lse)), what
        assert abs(lps[r] - (float(want[ids[r]]) - lse)) < 1e-5 * max(1.0, abs(lse)), what
        if c["rows"][b].get("sample"):
            drawn, margin = sampler_ref.race_choice(scores[r], seeds[b], offsets[b] + j)
            assert not np.isneginf(want[ids[r]]), what
            if margin > 1e-3:
                assert ids[r] == drawn, f"{what}: drew {ids[r]}, the race at offset + {j} gives {drawn}"
        else:
            assert ids[r] == int(np.argmax(want)), what
    _check_same(out, _launch(lib, d, c["rows"], rng=rng, verify=True), c["id"] + ": second call")


# ---- the global-row kernel returns the register kernel's bits -----------------------------------------------------------------
def _digest(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def _all_runs(lib):
    """{run id: {output: digest of its bytes, padding included}} of every table case with V <= 32768 and of the draws."""
    runs = {}
    for c in sc.CASES:
        if c["V"] <= 32768:
            out = _launch(lib, sc.build(c), c["rows"])
            runs[c["id"]] = {k: _digest(out[k]) for k in OUTPUTS if out[k] is not None}
    for V in sc.DRAW_V:
        c, outs = _draw_runs(lib, V)
        for i, out in enumerate(outs):
            runs[f"{c['id']}-{i}"] = {k: _digest(out[k]) for k in OUTPUTS}
    return runs


def _child(path):
    from tgis_amd import native

    lib = native.load_library()
    for V in sc.VS:
        assert rc.query(lib, "sampler", V)[0] == 0, "TGIS_SAMPLER_GLOBAL_ROWS did not select the global-row kernel"
    with open(path, "w") as f:
        json.dump(_all_runs(lib), f)
    print("ok", flush=True)


def test_global_row_kernel_is_bit_identical_on_every_case(lib, tmp_path):
    assert all(rc.query(lib, "sampler", V)[0] == 1 for V in sc.VS if V <= 32768)
    mine = _all_runs(lib)
    path = str(tmp_path / "global_rows.json")
    env = dict(os.environ, TGIS_SAMPLER_GLOBAL_ROWS="1")
    here = os.path.dirname(os.path.abspath(__file__))
    paths = [here, os.path.dirname(here), os.path.join(os.path.dirname(here), "text-generation-inference_amd")]
    code = f"import sys; sys.path[:0] = {paths!r}; import test_sampler_edges_gpu as t; t._child({path!r})"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "ok" in r.stdout, f"child: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    with open(path) as f:
        theirs = json.load(f)
    assert set(theirs) == set(mine) and len(mine) > len(sc.CASES) // 2
    bad = [(cid, k) for cid in sorted(mine) for k in mine[cid] if mine[cid][k] != theirs[cid].get(k)]
    assert not bad, f"{len(bad)} outputs of the global-row kernel differ from the register kernel's; first: {bad[:6]}"
