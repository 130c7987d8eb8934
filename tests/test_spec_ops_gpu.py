"""-m gpu: tgis_spec_propose, tgis_spec_accept and tgis_spec_stage against their numpy restatement (tests/spec_ref.py), bit
for bit.  Every output sits inside a larger buffer filled with a sentinel: what lies behind it must stay untouched."""
import numpy as np
import pytest
import torch

from tests import spec_ref

pytestmark = pytest.mark.gpu

SENT = -7777
BS, KS, NS = [1, 3, 16], [1, 3, 7], [1, 3]


@pytest.fixture(scope="module")
def nat(gpu_device):
    from tgis_amd import native

    native.load_library()
    return native


def _guarded(n, dtype, dev, shape=None):
    """(view of n elements, the whole buffer): n elements in front of 16 sentinels."""
    whole = torch.full((n + 16,), SENT, dtype=dtype, device=dev)
    view = whole[:n]
    return (view.view(shape) if shape else view), whole


def _tail_intact(whole, n):
    return bool((whole[n:] == SENT).all())


# ---- propose ------------------------------------------------------------------------------------------------------------------
def _contexts(B, K, N, rng):
    """B contexts that walk through the cases of the lookup, then random ones over a small vocabulary (many matches)."""
    rep = [11, 12, 13]
    cases = [
        [7] * min(N, 2) if N > 1 else [7],                      # shorter than N + 1 (N = 1: one token, no j at all)
        rep + [40, 41, 42, 43, 44, 45, 46] + rep,               # a match at index 0
        [21, 22, 30, 21, 22, 31, 50, 21, 22, 32, 60, 21, 22],   # several matches: the latest wins
        [1, 2, 3, 70, 71, 3, 72, 73, 9, 1, 2, 3],               # N = 3: n = 3 at j = 0 beats the later n = 1 match
        [5, 6, 7, 5, 6],                                        # the continuation runs into the context's end
        list(range(100, 120)),                                  # no match at all
    ]
    out = [cases[i % len(cases)] if i < len(cases) else rng.integers(0, 4, size=int(rng.integers(1, 90))).tolist()
           for i in range(B)]
    if B < len(cases):  # small batches: rotate through the cases by K and N so that every case runs somewhere
        out = [cases[(i + K + N) % len(cases)] for i in range(B)]
    return out


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("B", BS)
def test_propose_equals_the_restatement(nat, gpu_device, B, K, N):
    rng = np.random.default_rng(1000 * B + 10 * K + N)
    ctxs = _contexts(B, K, N, rng)
    L = 96
    all_ids = np.full((B + 2, L), 3, dtype=np.int64)  # rows behind the batch, columns behind every context
    for b, c in enumerate(ctxs):
        all_ids[b, :len(c)] = c
        all_ids[b, len(c):] = rng.integers(0, 4, size=L - len(c))  # what follows the context must not be looked at
    pos = np.array([len(c) - 1 for c in ctxs], dtype=np.int64)
    want_d, want_h = spec_ref.propose(all_ids[:B], pos, K, N)
    drafts, d_whole = _guarded(B * K, torch.int64, gpu_device, (B, K))
    hits, h_whole = _guarded(B, torch.int32, gpu_device)
    copy, c_whole = _guarded(B, torch.int32, gpu_device)
    dev_all = torch.from_numpy(all_ids).to(gpu_device)
    nat.spec_propose(dev_all[:B], torch.from_numpy(pos).to(gpu_device), N, drafts, hits, copy)
    torch.cuda.synchronize()
    assert drafts.cpu().numpy().tolist() == want_d.tolist(), (ctxs, want_h.tolist())
    assert hits.cpu().numpy().tolist() == want_h.tolist() and torch.equal(copy, hits)
    assert _tail_intact(d_whole, B * K) and _tail_intact(h_whole, B) and _tail_intact(c_whole, B)
    assert torch.equal(dev_all.cpu(), torch.from_numpy(all_ids)), "the contexts are read only"
    if B == 16:  # every case of the list ran, with the answers the list promises
        assert want_h[1] == min(N, 3) and want_h[5] == 0 and want_h[0] == (1 if N > 1 else 0)
        assert want_d[2, 0] == 32 and want_d[4].tolist()[:min(K, 3)] == [7, 5, 6][:min(K, 3)] and (K < 4 or want_d[4, 3] == 0)
        if N == 3:
            assert want_h[3] == 3 and want_d[3, 0] == 70


def test_propose_without_the_copy_and_at_the_row_end(nat, gpu_device):
    """hits_copy left out; a context that fills its whole row (len == ld) and one whose position lies behind the row."""
    all_ids = torch.tensor([[1, 2, 9, 1, 2], [4, 4, 4, 4, 4]], dtype=torch.int64)
    pos = torch.tensor([4, 11], dtype=torch.int64)  # the second is clamped to the row's 5 tokens
    want_d, want_h = spec_ref.propose(all_ids.numpy(), pos.numpy(), 3, 2)
    assert want_d.tolist() == [[9, 1, 2], [4, 0, 0]] and want_h.tolist() == [2, 2]
    drafts = torch.full((2, 3), SENT, dtype=torch.int64, device=gpu_device)
    hits = torch.full((2,), SENT, dtype=torch.int32, device=gpu_device)
    nat.spec_propose(all_ids.to(gpu_device), pos.to(gpu_device), 2, drafts, hits)
    assert drafts.cpu().tolist() == want_d.tolist() and hits.cpu().tolist() == want_h.tolist()


# ---- accept -------------------------------------------------------------------------------------------------------------------
def _accept_case(B, K, rng):
    K1 = K + 1
    L = 64
    am = rng.integers(3, 250, size=(B, K1)).astype(np.int64)
    lps = -rng.random((B, K1)).astype(np.float32)
    drafts = am[:, :K].copy()
    for b in range(B):  # 0 accepted, some, all K: the first wrong draft at index b % (K + 1) (== K: none is wrong)
        j = b % K1
        if j < K:
            drafts[b, j] += 1
            drafts[b, j + 1:] = rng.integers(3, 250, size=K - j - 1)
    pos = rng.integers(0, L - K1 - 1, size=B).astype(np.int64)
    all_ids = rng.integers(3, 250, size=(B + 2, L)).astype(np.int64)
    cu = (np.cumsum(rng.integers(1, 40, size=B + 1)) - 1).astype(np.int32)
    return am, lps, drafts, pos, all_ids, cu


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("B", BS)
def test_accept_equals_the_restatement(nat, gpu_device, B, K):
    rng = np.random.default_rng(77 * B + K)
    am, lps, drafts, pos, all_ids, cu = _accept_case(B, K, rng)
    K1 = K + 1
    want = spec_ref.accept(am, lps, drafts, pos, all_ids[:B], cu)
    assert sorted(set(want["n_emit"].tolist())) == sorted({b % K1 + 1 for b in range(B)}), "0 .. K accepted all occur"
    up = (lambda a: torch.from_numpy(a).to(gpu_device))
    n_emit, n_whole = _guarded(B, torch.int32, gpu_device)
    out_ids, oi_whole = _guarded(B * K1, torch.int64, gpu_device)
    out_lps, ol_whole = _guarded(B * K1, torch.float32, gpu_device)
    st_ids, si_whole = _guarded(B, torch.int64, gpu_device)
    st_pos, sp_whole = _guarded(B, torch.int32, gpu_device)
    cu_view, cu_whole = _guarded(B + 1, torch.int32, gpu_device)
    cu_view.copy_(up(cu))
    d_pos, d_all = up(pos), up(all_ids)
    latest = nat.spec_accept(up(am).view(-1), up(lps).view(-1), up(drafts), n_emit, d_pos, out_ids=out_ids,
                             out_logprobs=out_lps, all_input_ids=d_all[:B], cu_seqlens=cu_view, stage_ids=st_ids,
                             stage_positions=st_pos)
    torch.cuda.synchronize()
    assert n_emit.cpu().tolist() == want["n_emit"].tolist()
    assert out_ids.cpu().view(B, K1).tolist() == want["out_ids"].tolist()
    assert np.array_equal(out_lps.cpu().view(B, K1).numpy(), want["out_lps"]), "logprobs are copied, bit for bit"
    assert latest.cpu().tolist() == want["latest"].tolist() and st_ids.cpu().tolist() == want["latest"].tolist()
    assert d_pos.cpu().tolist() == want["positions"].tolist() and st_pos.cpu().tolist() == want["positions"].tolist()
    assert np.array_equal(d_all[:B].cpu().numpy(), want["all_ids"]), "the scatter writes the emitted ids and nothing else"
    assert np.array_equal(d_all[B:].cpu().numpy(), all_ids[B:]), "rows behind the batch"
    assert cu_view.cpu().tolist() == want["cu_seqlens"].tolist()
    for whole, n in ((n_whole, B), (oi_whole, B * K1), (ol_whole, B * K1), (si_whole, B), (sp_whole, B), (cu_whole, B + 1)):
        assert _tail_intact(whole, n)


@pytest.mark.parametrize("B", [1, 3, 16, 200, 300])
def test_accept_without_drafts_is_decode_advance(nat, gpu_device, B):
    """K = 0 against tgis_decode_advance on copies of the same inputs: every output bit-equal (300 rows: more than the
    one workgroup has threads)."""
    g = torch.Generator().manual_seed(B)
    L = 50
    ids = torch.randint(0, 32000, (B,), generator=g).to(gpu_device)
    lps = -torch.rand(B, generator=g).to(gpu_device)
    pos = torch.randint(0, L - 1, (B,), generator=g).to(gpu_device)
    pos[0] = L - 1  # a position whose successor lies behind the row: neither kernel writes there
    all_ids = torch.randint(0, 32000, (B + 3, L), generator=g).to(gpu_device)
    cu = (torch.cumsum(torch.randint(1, 40, (B + 1,), generator=g), 0).int() - 1).to(gpu_device)
    cu_q = torch.arange(B + 1, dtype=torch.int32, device=gpu_device)
    a = dict(pos=pos.clone(), all=all_ids.clone(), cu=cu.clone(), si=torch.zeros_like(ids), sp=torch.zeros_like(cu[:B]))
    s = {k: v.clone() for k, v in a.items()}
    want = nat.decode_advance(ids, a["pos"], a["all"][:B], a["cu"], cu_q, stage_ids=a["si"], stage_positions=a["sp"])
    n_emit, n_whole = _guarded(B, torch.int32, gpu_device)
    out_ids, oi_whole = _guarded(B, torch.int64, gpu_device)
    out_lps, ol_whole = _guarded(B, torch.float32, gpu_device)
    got = nat.spec_accept(ids, lps, None, n_emit, s["pos"], out_ids=out_ids, out_logprobs=out_lps, all_input_ids=s["all"][:B],
                          cu_seqlens=s["cu"], stage_ids=s["si"], stage_positions=s["sp"])
    torch.cuda.synchronize()
    assert torch.equal(got, want) and got.data_ptr() != ids.data_ptr()
    for k in a:
        assert torch.equal(a[k], s[k]), k
    assert (n_emit == 1).all() and torch.equal(out_ids, ids) and torch.equal(out_lps, lps)
    assert _tail_intact(n_whole, B) and _tail_intact(oi_whole, B) and _tail_intact(ol_whole, B)
    # optional outputs left out: only the positions and the counts move
    p2 = pos.clone()
    got2 = nat.spec_accept(ids, None, None, n_emit, p2)
    assert torch.equal(got2, ids) and torch.equal(p2, pos + 1)


# ---- stage --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("B", BS)
def test_stage_equals_the_restatement(nat, gpu_device, B, K):
    rng = np.random.default_rng(31 * B + K)
    K1, W, null = K + 1, 5, 4096
    pos = np.array([[0, 30, 31, 62, 63 + 32][b % 5] for b in range(B)], dtype=np.int32)  # pos % 32 in {0, 30, 31}
    if B == 1:
        pos[0] = [30, 31, 0][K % 3]
    bt = rng.permutation(200)[:B * W].reshape(B, W).astype(np.int32)
    latest = rng.integers(3, 250, size=B).astype(np.int64)
    drafts = rng.integers(3, 250, size=(B, K)).astype(np.int64)
    inactive = [b for b in range(B) if b % 4 == 3]  # rows a smaller batch leaves: position 0, null page, ids 0
    for b in inactive:
        pos[b], latest[b], drafts[b], bt[b] = 0, 0, 0, null
    want = spec_ref.stage(pos, latest, drafts, bt)
    up = (lambda a: torch.from_numpy(a).to(gpu_device))
    ids, i_whole = _guarded(B * K1, torch.int64, gpu_device)
    p_out, p_whole = _guarded(B * K1, torch.int32, gpu_device)
    slots, s_whole = _guarded(B * K1, torch.int32, gpu_device)
    ctx, c_whole = _guarded(B, torch.int32, gpu_device)
    nat.spec_stage(up(pos), up(latest), up(drafts), up(bt), ids, p_out, slots, ctx)
    torch.cuda.synchronize()
    for got, w in zip((ids, p_out, slots, ctx), want):
        assert got.cpu().tolist() == w.tolist()
    for whole, n in ((i_whole, B * K1), (p_whole, B * K1), (s_whole, B * K1), (c_whole, B)):
        assert _tail_intact(whole, n)
    s = slots.cpu().view(B, K1)
    for b in inactive:
        assert s[b].tolist() == [null * 32 + j for j in range(K1)], "inactive rows land on the null page"
    if B >= 3:  # position 31: the first draft starts the next page of the table
        assert s[2, 0] == bt[2, 0] * 32 + 31 and s[2, 1] == bt[2, 1] * 32
