"""-m gpu: tgis_warp_sample_verify and tgis_spec_accept_sampled through the C ABI.

The yardstick of the verify chooser is the existing tgis_warp_sample on the host-expanded problem: one row per (b, j) with
request b's parameters replicated, its context extended by drafts[b][:j] (tests/spec_sampled_ref.py `expand`) and the stream
state (seed, offset + j).  Equality is torch.equal on ids, logprobs, lse and warped scores: no tolerance, the order of
operations must be the same.  tgis_spec_accept_sampled is held to everything tests/test_spec_ops_gpu.py asks of
tgis_spec_accept, plus the offsets."""
import numpy as np
import pytest
import torch

from tests import spec_ref
from tests import spec_sampled_ref as ref
from tests.test_sampler_gpu import ROWSETS
from tests.test_spec_ops_gpu import BS, KS, _accept_case, _guarded, _tail_intact

pytestmark = pytest.mark.gpu

EOS_ID, EXCLUDE_ID, L, LD_EXTRA, OFFSET = 7, 3, 37, 5, 9


@pytest.fixture(scope="module")
def nat(gpu_device):
    from tgis_amd import native

    native.load_library()
    return native


def _col(rows, name, default, dtype, dev):
    if all(name not in r for r in rows):
        return None
    return torch.tensor([r.get(name, default) for r in rows], dtype=dtype, device=dev)


def _rep(t, K1):
    return None if t is None else t.repeat_interleave(K1, dim=0).contiguous()


def _problem(rows, V, K, seed):
    """Logits, contexts (in a tensor wider than L: ld_ids > L) and drafts with the special ids of the issue."""
    B, K1 = len(rows), K + 1
    rs = np.random.RandomState(seed)
    logits = (rs.randn(B * K1, V) * 3).astype(np.float32)
    wide = rs.randint(0, V, size=(B, L + LD_EXTRA)).astype(np.int64)
    wide[:, L - 5:L] = EXCLUDE_ID  # padding-like repeats of the excluded id
    wide[:, L:] = 11               # behind the context: never read (id 11 is in no context otherwise)
    wide[:, :L][wide[:, :L] == 11] = 12
    drafts = rs.randint(0, V, size=(B, K)).astype(np.int64)
    drafts[drafts == 11] = 12
    special = lambda b: [EOS_ID, int(wide[b, 0]), V + 3, -1]  # EOS, already in the context, out of range twice
    for b in range(B):
        if K == 1:
            drafts[b, 0] = special(b)[b % 4]
        for i, v in enumerate(special(b)[:K] if K > 1 else []):
            drafts[b, (b + i) % K] = v
    return logits, wide, drafts


def _eos_rows(rows, K1, dev):
    """[B, K + 1, 2]: the row set's (mode, factor) on even verify rows with a factor that grows, nothing on odd ones."""
    if all("eos" not in r for r in rows):
        return None
    out = np.zeros((len(rows), K1, 2), dtype=np.float32)
    for b, r in enumerate(rows):
        mode, factor = r.get("eos", (0.0, 0.0))
        for j in range(0, K1, 2):
            out[b, j] = (mode, factor * (1 + j))
    return torch.from_numpy(out).to(dev)


@pytest.mark.parametrize("K", [0, 1, 3, 7])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", [41, 32000, 50257])
def test_verify_chooser_equals_the_plain_chooser_on_the_expanded_problem(nat, gpu_device, V, B, K):
    """V = 41: a partial pass of the register form; 32000: the full register form; 50257: the global-row form."""
    dev, K1 = gpu_device, K + 1
    sampled_rows = 0
    for n, name in enumerate(sorted(ROWSETS)):
        rows = [ROWSETS[name][(b + K) % len(ROWSETS[name])] for b in range(B)]
        logits, wide, drafts = _problem(rows, V, K, 1000 * n + 10 * K + B + V)
        use_ids = any("rep_penalty" in r for r in rows)
        d_logits = torch.from_numpy(logits).to(dev)
        d_wide = torch.from_numpy(wide).to(dev)
        d_drafts = torch.from_numpy(drafts).to(dev) if K else None
        expanded = torch.from_numpy(ref.expand(B, K, L, wide, drafts, EXCLUDE_ID)).to(dev)
        par = {k: _col(rows, k, d, t, dev) for k, d, t in (
            ("temperature", 1.0, torch.float32), ("top_k", 0, torch.int32), ("top_p_cut", 0.0, torch.float32),
            ("typical_p", 1.0, torch.float32), ("rep_penalty", 1.0, torch.float32))}
        eos = _eos_rows(rows, K1, dev)
        for mixed in (False, True):
            do_sample = rng = rng_rows = None
            if mixed:  # B = 1: sampled; B = 3: sampled, greedy, sampled
                flags = [1 if B == 1 else int(b % 2 == 0) for b in range(B)]
                seeds = [(1 << 40) * (b + 1) + 17 if b != 2 else -3 for b in range(B)]  # -3: above 2^63 in two's complement
                do_sample = torch.tensor(flags, dtype=torch.int32, device=dev)
                rng = torch.tensor([[s, OFFSET] for s in seeds], dtype=torch.int64, device=dev)
                rng_rows = torch.tensor([[s, OFFSET + j] for s in seeds for j in range(K1)], dtype=torch.int64, device=dev)
                sampled_rows += sum(flags) * K1
            rng_before = None if rng is None else rng.clone()
            got = nat.warp_sample_verify(
                d_logits, d_drafts, K, input_ids=d_wide[:, :L] if use_ids else None, exclude_id=EXCLUDE_ID, eos_adjust=eos,
                eos_id=EOS_ID if eos is not None else -1, do_sample=do_sample, rng=rng, **par)
            want = nat.warp_sample(
                d_logits, input_ids=expanded if use_ids else None, exclude_id=EXCLUDE_ID,
                eos_adjust=None if eos is None else eos.view(-1, 2), eos_id=EOS_ID if eos is not None else -1,
                do_sample=_rep(do_sample, K1), rng=rng_rows, **{k: _rep(v, K1) for k, v in par.items()})
            torch.cuda.synchronize()
            what = f"{name} mixed={mixed}"
            assert got[0].shape == got[1].shape == got[2].shape == (B, K1) and got[3].shape == (B * K1, V)
            assert torch.equal(got[0].view(-1), want[0]), f"{what}: ids"
            assert torch.equal(got[1].view(-1), want[1]), f"{what}: logprobs"
            assert torch.equal(got[2].view(-1), want[2]), f"{what}: lse"
            assert torch.equal(got[3], want[3]), f"{what}: warped scores"
            assert torch.equal(d_logits.cpu(), torch.from_numpy(logits)), "the logits are read only"
            if mixed:
                assert torch.equal(rng, rng_before), "the verify form only reads the streams"
                # (the plain chooser advanced the copies it was given, for its sampled rows only)
                adv = rng_rows[:, 1].view(B, K1) - rng_before[:, 1:2] - torch.arange(K1, device=dev)
                assert adv.tolist() == [[f] * K1 for f in flags]
    assert sampled_rows > 0


def test_a_penalised_draft_changes_the_rows_behind_it_only(nat, gpu_device):
    """The context of row j ends with drafts[:j]: a draft's own row does not see it, the rows behind it do."""
    V, K = 32000, 3
    logits = torch.zeros((K + 1, V), dtype=torch.float32, device=gpu_device)
    logits[:, 100] = 2.0
    ids = torch.tensor([[5, 6]], dtype=torch.int64, device=gpu_device)
    drafts = torch.tensor([[9, 100, 9]], dtype=torch.int64, device=gpu_device)
    pen = torch.tensor([2.0], dtype=torch.float32, device=gpu_device)
    _ids, _lps, _lse, scores = nat.warp_sample_verify(logits, drafts, K, rep_penalty=pen, input_ids=ids)
    assert scores[:, 100].tolist() == [2.0, 2.0, 1.0, 1.0]


def test_verify_with_no_requests_returns_ok(nat, gpu_device):
    out = nat.warp_sample_verify(torch.zeros((0, 41), dtype=torch.float32, device=gpu_device), None, 0)
    assert out[0].shape == (0, 1) and out[3].shape == (0, 41)
    out = nat.warp_sample_verify(torch.zeros((0, 41), dtype=torch.float32, device=gpu_device),
                                 torch.zeros((0, 3), dtype=torch.int64, device=gpu_device), 3)
    assert out[0].shape == (0, 4)


# ---- accept -------------------------------------------------------------------------------------------------------------------
def _run_accept(nat, dev, B, K, call, am, lps, drafts, pos, all_ids, cu):
    """One accept launch into guarded buffers; returns every output on the host and checks what lies behind them."""
    K1 = K + 1
    up = (lambda a: torch.from_numpy(a).to(dev))
    n_emit, n_whole = _guarded(B, torch.int32, dev)
    out_ids, oi_whole = _guarded(B * K1, torch.int64, dev)
    out_lps, ol_whole = _guarded(B * K1, torch.float32, dev)
    st_ids, si_whole = _guarded(B, torch.int64, dev)
    st_pos, sp_whole = _guarded(B, torch.int32, dev)
    cu_view, cu_whole = _guarded(B + 1, torch.int32, dev)
    cu_view.copy_(up(cu))
    d_pos, d_all = up(pos), up(all_ids)
    latest = call(up(am).view(-1), up(lps).view(-1), up(drafts) if K else None, n_emit, d_pos, out_ids=out_ids,
                  out_logprobs=out_lps, all_input_ids=d_all[:B], cu_seqlens=cu_view, stage_ids=st_ids, stage_positions=st_pos)
    torch.cuda.synchronize()
    for whole, n in ((n_whole, B), (oi_whole, B * K1), (ol_whole, B * K1), (si_whole, B), (sp_whole, B), (cu_whole, B + 1)):
        assert _tail_intact(whole, n)
    return dict(n_emit=n_emit.cpu(), out_ids=out_ids.cpu().view(B, K1), out_lps=out_lps.cpu().view(B, K1), latest=latest.cpu(),
                stage_ids=st_ids.cpu(), positions=d_pos.cpu(), stage_pos=st_pos.cpu(), all_ids=d_all.cpu(),
                cu_seqlens=cu_view.cpu())


def _streams(B, dev):
    flags = [int(b % 3 != 1) for b in range(B)]  # sampled, greedy, sampled, ...
    rng = torch.tensor([[-(b + 1) if b % 2 else (b + 1) << 33, (1 << 32) - 2 + b] for b in range(B)], dtype=torch.int64)
    return torch.tensor(flags, dtype=torch.int32, device=dev), rng.to(dev), flags, rng


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("B", BS)
def test_accept_sampled_equals_the_restatement_and_advances_the_streams(nat, gpu_device, B, K):
    rs = np.random.default_rng(77 * B + K)
    case = _accept_case(B, K, rs)
    am, lps, drafts, pos, all_ids, cu = case
    want = spec_ref.accept(am, lps, drafts, pos, all_ids[:B], cu)
    assert sorted(set(want["n_emit"].tolist())) == sorted({b % (K + 1) + 1 for b in range(B)}), "0 .. K accepted all occur"
    do_sample, rng, flags, rng0 = _streams(B, gpu_device)
    call = (lambda *a, **kw: nat.spec_accept_sampled(*a, do_sample=do_sample, rng=rng, **kw))
    got = _run_accept(nat, gpu_device, B, K, call, *case)
    assert got["n_emit"].tolist() == want["n_emit"].tolist()
    assert got["out_ids"].tolist() == want["out_ids"].tolist()
    assert np.array_equal(got["out_lps"].numpy(), want["out_lps"]), "logprobs are copied, bit for bit"
    assert got["latest"].tolist() == want["latest"].tolist() == got["stage_ids"].tolist()
    assert got["positions"].tolist() == want["positions"].tolist() == got["stage_pos"].tolist()
    assert np.array_equal(got["all_ids"][:B].numpy(), want["all_ids"]), "the scatter writes the emitted ids and nothing else"
    assert np.array_equal(got["all_ids"][B:].numpy(), all_ids[B:]), "rows behind the batch"
    assert got["cu_seqlens"].tolist() == want["cu_seqlens"].tolist()
    after = rng.cpu()
    assert torch.equal(after[:, 0], rng0[:, 0]), "seeds are not touched"
    assert (after[:, 1] - rng0[:, 1]).tolist() == [int(n) * f for n, f in zip(want["n_emit"], flags)], \
        "one draw per emitted token, for sampled requests only (offsets cross 2^32 here)"


@pytest.mark.parametrize("K", [0] + KS)
@pytest.mark.parametrize("B", BS + [300])
def test_accept_sampled_without_streams_is_the_old_entry_bit_for_bit(nat, gpu_device, B, K):
    """do_sample NULL (with or without rng); 300 requests: more than the one workgroup has threads; K = 0 as well."""
    case = _accept_case(B, K, np.random.default_rng(5 * B + K))
    old = _run_accept(nat, gpu_device, B, K, nat.spec_accept, *case)
    _ds, rng, _flags, rng0 = _streams(B, gpu_device)
    for r in (None, rng):
        new = _run_accept(nat, gpu_device, B, K, (lambda *a, **kw: nat.spec_accept_sampled(*a, rng=r, **kw)), *case)
        for k in old:
            assert torch.equal(old[k], new[k]), k
    assert torch.equal(rng.cpu(), rng0)


def test_accept_sampled_without_drafts_advances_by_one(nat, gpu_device):
    """K = 0, the plain step of a sampled batch: tgis_decode_advance's outputs and one draw per sampled request."""
    B, Lw = 5, 50
    g = torch.Generator().manual_seed(B)
    ids = torch.randint(0, 32000, (B,), generator=g).to(gpu_device)
    pos = torch.randint(0, Lw - 1, (B,), generator=g).to(gpu_device)
    all_ids = torch.randint(0, 32000, (B, Lw), generator=g).to(gpu_device)
    want_all, want_pos = all_ids.clone(), pos.clone()
    want = nat.decode_advance(ids, want_pos, want_all)
    do_sample, rng, flags, rng0 = _streams(B, gpu_device)
    n_emit = torch.zeros(B, dtype=torch.int32, device=gpu_device)
    got = nat.spec_accept_sampled(ids, None, None, n_emit, pos, do_sample=do_sample, rng=rng, all_input_ids=all_ids)
    assert torch.equal(got, want) and torch.equal(pos, want_pos) and torch.equal(all_ids, want_all)
    assert (rng.cpu()[:, 1] - rng0[:, 1]).tolist() == flags and n_emit.tolist() == [1] * B


def test_accept_sampled_with_no_requests_returns_ok(nat, gpu_device):
    i64 = torch.full((4,), 5, dtype=torch.int64, device=gpu_device)
    i32 = torch.full((4,), 5, dtype=torch.int32, device=gpu_device)
    rng = torch.full((2, 2), 5, dtype=torch.int64, device=gpu_device)
    out = nat.spec_accept_sampled(i64[:0], None, None, i32[:0], i64[:0], do_sample=i32[:0], rng=rng[:0])
    torch.cuda.synchronize()
    assert out.numel() == 0 and (i64 == 5).all() and (i32 == 5).all() and (rng == 5).all()
