"""-m gpu: tgis_rope_kv_write_prefill_at / _at_kv8, the page-wise cache writer that starts behind a reused prefix.

The reference is the EXISTING per-token writer tgis_rope_kv_write given the same tokens, rotary positions and explicit slots,
on a pool pre-filled with the same guard; the zeroed tail of a last partial page is restated by a second per-token launch
that writes zero-valued tokens (no rotary) to exactly those slots.  The two pools must then be equal BIT FOR BIT over every
page: written slots, zeroed tails, every page in front of past_lens[b] / 32 (they belong to other requests) and every page
nobody owns (still the guard).  Those last two are asserted on their own as well."""
import ctypes
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

PASTS = [0, 32, 64, 96, 32]       # {0, 32, 64, 96}
SUFFIXES = [1, 31, 32, 33, 70]    # {1, 31, 32, 33, 70}: one slot, a page short of one, a page, a page and one, 2 pages + 6
MAX_POS = 256
SHAPES = [(4, 4, 64, 64, True), (8, 1, 128, 128, True), (4, 2, 96, 24, True), (4, 2, 64, 64, False)]
SHAPE_IDS = ["mha-d64", "mqa-d128", "gqa-d96-rot24-general-path", "no-rotary"]
SCALES = (0.5, 4.0)               # non-unit powers of two


@pytest.fixture(scope="module")
def nat(gpu_device):
    from tgis_amd import native

    native.load_library()
    return native


def _bits(t):
    return t.view(torch.uint8) if t.element_size() == 1 else t.view(torch.int16)


def _guard_pool(pages, Hkv, D, dt, fp8, dev):
    if fp8:
        return torch.full((pages, Hkv, 32 * D), 0x7E, dtype=torch.uint8, device=dev)
    p = torch.full((pages, Hkv, 32 * D), 65504.0, dtype=torch.float32, device=dev)
    p.view(-1)[1::2] = -65504.0
    return p.to(dt)


def _setup(H, Hkv, D, rot, rope, dt, dev, pasts=PASTS, suffixes=SUFFIXES, seed=0):
    g = torch.Generator().manual_seed(1000 * D + 10 * H + seed)
    B, T, N = len(pasts), sum(suffixes), (H + 2 * Hkv) * D
    npg = [p // 32 + -(-s // 32) for p, s in zip(pasts, suffixes)]
    pages = sum(npg) + 3                                   # 3 pages no sequence owns
    max_pages = max(npg) + 1
    perm = torch.randperm(pages, generator=g).tolist()     # shuffled tables
    bt = torch.full((B, max_pages), perm[sum(npg)], dtype=torch.int32)  # entries past a sequence's pages: nobody's page
    k = 0
    for b, n in enumerate(npg):
        bt[b, :n] = torch.tensor(perm[k:k + n], dtype=torch.int32)
        k += n
    cu = torch.tensor([0] + list(itertools.accumulate(suffixes)), dtype=torch.int32)
    cache_pos = torch.cat([p + torch.arange(s) for p, s in zip(pasts, suffixes)])
    seq = torch.cat([torch.full((s,), b) for b, s in enumerate(suffixes)])
    slots = (bt[seq, cache_pos // 32] * 32 + cache_pos % 32).to(torch.int32)
    # the rotary position is whatever `positions` says, not the cache position: sequence 0's are shifted
    pos = (cache_pos + (seq == 0) * 17).to(torch.int32)
    # slots of each last partial page behind the sequence's end
    tail = []
    for b, (p, s) in enumerate(zip(pasts, suffixes)):
        end = p + s
        tail += [int(bt[b, end // 32]) * 32 + o for o in range(end % 32, 32)] if end % 32 else []
    x = (torch.randn((T, N), generator=g) * 1.5).to(dt)
    cos = sin = None
    if rope:
        ang = torch.arange(MAX_POS)[:, None] * (10000.0 ** (-torch.arange(rot // 2) / (rot // 2)))[None, :]
        cos, sin = ang.cos().to(dt).to(dev), ang.sin().to(dt).to(dev)
    before = sorted({int(bt[b, i]) for b, p in enumerate(pasts) for i in range(p // 32)})
    owned = sorted({int(bt[b, i]) for b, (p, s) in enumerate(zip(pasts, suffixes)) for i in range(p // 32, npg[b])})
    return dict(B=B, T=T, N=N, pages=pages, bt=bt.to(dev), cu=cu.to(dev), slots=slots.to(dev), pos=pos.to(dev),
                tail=torch.tensor(tail, dtype=torch.int32, device=dev), x=x.to(dev), cos=cos, sin=sin, before=before,
                owned=owned, pasts=list(pasts), max_len=max(suffixes))


def _activation(s, dt):
    """The qkv activation in a buffer with a padded row stride."""
    buf = torch.zeros((s["T"], s["N"] + 16), dtype=dt, device=s["x"].device)
    buf[:, :s["N"]] = s["x"]
    return buf[:, :s["N"]]


def _reference(nat, s, H, Hkv, D, rot, dt, fp8, kw):
    """(q, k pool, v pool) of the per-token writer, the zeroed tails restated by a launch of zero tokens."""
    dev = s["x"].device
    kp, vp = _guard_pool(s["pages"], Hkv, D, dt, fp8, dev), _guard_pool(s["pages"], Hkv, D, dt, fp8, dev)
    a = _activation(s, dt)
    nat.rope_kv_write(a, s["cos"], s["sin"], s["pos"] if s["cos"] is not None else None, s["slots"], kp, vp, H, Hkv, D, rot,
                      **kw)
    if s["tail"].numel():
        z = torch.zeros((s["tail"].numel(), s["N"]), dtype=dt, device=dev)
        nat.rope_kv_write(z, None, None, None, s["tail"], kp, vp, H, Hkv, D, rot, **kw)
    return a, kp, vp


@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "kv-e4m3"])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("H,Hkv,D,rot,rope", SHAPES, ids=SHAPE_IDS)
def test_prefill_at_equals_the_per_token_writer_and_leaves_every_other_page_alone(nat, gpu_device, H, Hkv, D, rot, rope, dt,
                                                                                    fp8):
    s = _setup(H, Hkv, D, rot, rope, dt, gpu_device)
    kw = {"kv_scales": SCALES} if fp8 else {}
    ref_q, ref_k, ref_v = _reference(nat, s, H, Hkv, D, rot, dt, fp8, kw)
    kp, vp = (_guard_pool(s["pages"], Hkv, D, dt, fp8, gpu_device) for _ in range(2))
    guard = _guard_pool(s["pages"], Hkv, D, dt, fp8, gpu_device)
    a = _activation(s, dt)
    out = nat.rope_kv_write_prefill_at(a, s["cos"], s["sin"], s["pos"] if rope else None, s["cu"], s["bt"], kp, vp,
                                       s["max_len"], H, Hkv, D, rot, s["pasts"], **kw)
    torch.cuda.synchronize()
    assert out is a
    assert torch.equal(_bits(a[:, :H * D]), _bits(ref_q[:, :H * D])), "q differs from the per-token writer's"
    assert torch.equal(_bits(a[:, H * D:]), _bits(s["x"][:, H * D:])), "k / v inside qkv were touched"
    for name, got, want in (("k", kp, ref_k), ("v", vp, ref_v)):
        gb, wb, ub = _bits(got), _bits(want), _bits(guard)
        assert torch.equal(gb[s["before"]], ub[s["before"]]), f"{name}: a page in front of past_lens / 32 was stored to"
        free = sorted(set(range(s["pages"])) - set(s["owned"]))
        assert torch.equal(gb[free], ub[free]), f"{name}: a page outside the written range was stored to"
        bad = (gb != wb).flatten(1).any(1).nonzero().flatten().tolist()
        assert not bad, f"{name}: pages {bad} differ from the per-token writer (+ zeroed tails)"
        assert not torch.equal(gb[s["owned"]], ub[s["owned"]]), f"{name}: nothing was written"
    if not fp8:
        # the zeroed tails once more in token order, through the oracle's unpacker
        from oracle import ops_ref

        kc, vc = kp.float().cpu(), vp.float().cpu()
        for slot in s["tail"].tolist():
            K, V = ops_ref.kv_page_unpack(kc, vc, slot // 32, Hkv, D)
            assert not K[slot % 32].any() and not V[slot % 32].any(), f"slot {slot} behind a sequence's end is not zero"


@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "kv-e4m3"])
@pytest.mark.parametrize("H,Hkv,D,rot,rope", [SHAPES[0], SHAPES[2], SHAPES[3]], ids=[SHAPE_IDS[0], SHAPE_IDS[2], SHAPE_IDS[3]])
def test_all_zero_past_lens_is_the_fresh_writer_bit_for_bit(nat, gpu_device, H, Hkv, D, rot, rope, fp8):
    dt = torch.float16
    s = _setup(H, Hkv, D, rot, rope, dt, gpu_device, pasts=[0] * 5, seed=1)
    kw = {"kv_scales": SCALES} if fp8 else {}
    pools = [_guard_pool(s["pages"], Hkv, D, dt, fp8, gpu_device) for _ in range(4)]
    a0, a1 = _activation(s, dt), _activation(s, dt)
    pos = s["pos"] if rope else None
    nat.rope_kv_write_prefill(a0, s["cos"], s["sin"], pos, s["cu"], s["bt"], pools[0], pools[1], s["max_len"], H, Hkv, D, rot,
                              **kw)
    nat.rope_kv_write_prefill_at(a1, s["cos"], s["sin"], pos, s["cu"], s["bt"], pools[2], pools[3], s["max_len"], H, Hkv, D,
                                 rot, torch.zeros(5, dtype=torch.int32, device=gpu_device), **kw)
    torch.cuda.synchronize()
    assert torch.equal(_bits(a0), _bits(a1))
    assert torch.equal(_bits(pools[0]), _bits(pools[2])) and torch.equal(_bits(pools[1]), _bits(pools[3]))


def test_argument_errors_return_einval_without_launching(nat, gpu_device):
    H, Hkv, D, dt = 4, 2, 64, torch.float16
    s = _setup(H, Hkv, D, D, True, dt, gpu_device)
    lib = nat.load_library()
    p = (lambda t: ctypes.c_void_p(t.data_ptr()))
    past = torch.tensor(s["pasts"], dtype=torch.int32, device=gpu_device)
    for fp8 in (False, True):
        kp, vp = (_guard_pool(s["pages"], Hkv, D, dt, fp8, gpu_device) for _ in range(2))
        guard = _guard_pool(s["pages"], Hkv, D, dt, fp8, gpu_device)
        a = _activation(s, dt)
        fn = lib.tgis_rope_kv_write_prefill_at_kv8 if fp8 else lib.tgis_rope_kv_write_prefill_at
        tail = (nat.KV_FP8_E4M3, 0.5, 4.0) if fp8 else ()

        def call(max_len, past_ptr):
            return fn(p(a), a.stride(0), p(s["cos"]), p(s["sin"]), p(s["pos"]), p(s["cu"]), p(s["bt"]), s["bt"].shape[1],
                      p(kp), p(vp), s["B"], s["T"], max_len, H, Hkv, D, D, nat.dtype_code(dt), None, *tail, past_ptr)

        lib.tgis_clear_error()
        assert call(s["max_len"], None) == -1 and b"past_lens" in lib.tgis_last_error()
        lib.tgis_clear_error()
        assert call(32 * s["bt"].shape[1] + 1, p(past)) == -1 and b"tgis_rope_kv_write_prefill" in lib.tgis_last_error()
        torch.cuda.synchronize()
        assert torch.equal(_bits(kp), _bits(guard)) and torch.equal(_bits(vp), _bits(guard))
        assert torch.equal(_bits(a), _bits(s["x"])), "a refused call rotated q"
    lib.tgis_clear_error()


def test_the_wrapper_refuses_a_past_that_is_not_whole_pages(nat, gpu_device):
    with pytest.raises(AssertionError, match="multiples of 32"):
        nat.past_lens_tensor([32, 40], gpu_device)
    assert nat.past_lens_tensor([0, 64], gpu_device).tolist() == [0, 64]
