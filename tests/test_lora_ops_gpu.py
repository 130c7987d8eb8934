"""-m gpu: tgis_lora_group / tgis_lora_shrink / tgis_lora_expand (csrc/lora.hip) against the fp64 restatement of their contract
(tests/lora_ref.py), element by element under the derived bound of tests/lora_cases.py.

Shapes: K 320 (the shrink's k-parts are uneven, three of its eight waves get no k64-step), N 80 / 528 / 512 as one, two and three
fused projections (q|k|v of 256 | 128 | 128 columns), ranks 1, 4, 16, 24 and 64 in S = 4 slots, T in {0, 1, 2, 31, 32, 33, 64}
(none, less than a slab, a slab, a slab and a row, two slabs), row patterns all -1 / one slot / every row another slot /
the last row alone in its slot / slots mixed with -1.  Every case runs on poisoned images: slots no row names are NaN
throughout, named slots are NaN past their rank rounded up to 16; rows at -1 must come back bit for bit."""
import pytest
import torch

from tests import lora_cases as lc
from tests import lora_ref
from tests.moe_bounds import A_OUT, B_ACC, U, close  # noqa: F401  (the bound of lora_cases.reference is built from these)

pytestmark = pytest.mark.gpu

DTYPES = (torch.float16, torch.bfloat16)
RANK_SETS = {"r1_4_16_24": (1, 4, 16, 24), "r64_24_4_16": (64, 24, 4, 16)}


def _apply(x, y, w, slot_dev):
    from tgis_amd import native

    g = native.lora_group(slot_dev, w.S)
    v = native.lora_shrink(x, w, g)
    native.lora_expand(v, w, g, y)
    return g, v


@pytest.mark.parametrize("name", lc.PATTERNS)
def test_group_lists(gpu_device, name):
    """counts, offsets and the rows, ascending inside a slot, for every T; values outside -1 .. S-1 name no slot."""
    from tgis_amd import native

    for T in lc.TS:
        slot = lc.pattern(name, T)
        g = native.lora_group(slot.to(gpu_device), lc.S)
        counts, offsets, rows = lora_ref.group(slot, lc.S)
        assert torch.equal(g.counts.cpu().long(), counts) and torch.equal(g.offsets.cpu().long(), offsets), (name, T)
        assert torch.equal(g.rows.cpu().long()[:int(offsets[-1])], rows), (name, T)
    wild = torch.tensor([0, 7, -3, 1, lc.S, -1], dtype=torch.int32)
    g = native.lora_group(wild.to(gpu_device), lc.S)
    assert g.counts.tolist() == [1, 1, 0, 0] and g.rows.tolist()[:2] == [0, 3]


@pytest.mark.parametrize("ranks", sorted(RANK_SETS))
@pytest.mark.parametrize("shape", sorted(lc.BOUNDS))
@pytest.mark.parametrize("dt", DTYPES, ids=("f16", "bf16"))
def test_linear_delta_in_bound(gpu_device, dt, shape, ranks):
    bounds, rk = lc.BOUNDS[shape], RANK_SETS[ranks]
    N = bounds[-1]
    adps = lc.adapters(rk, bounds, dt)
    for name in lc.PATTERNS:
        for T in lc.TS:
            slot = lc.pattern(name, T)
            w = lc.images(adps, bounds, dt, gpu_device, named=set(slot.tolist()) - {-1})
            x, y0 = lc.activations(T, lc.K, dt), lc.base_output(T, N, dt)
            y = y0.to(gpu_device)
            _g, v = _apply(x.to(gpu_device), y, w, slot.to(gpu_device))
            what = f"{shape} {ranks} {name} T {T}"
            assert y.shape == (T, N)
            ref, tol = lc.reference(y0, x, adps, slot, bounds, dt)
            close(y, ref, tol, what)
            none = slot < 0
            assert torch.equal(y.cpu()[none].view(torch.int16), y0[none].view(torch.int16)), f"{what}: a row at -1 was touched"
            # the shrink alone: fp32 v within its accumulation term of A_s x[t], up to the slot's rank rounded up to 16
            for t, vt in lora_ref.shrink(x, adps, slot).items():
                A = adps[int(slot[t])][0].double()
                vtol = B_ACC * lc.K * U[torch.float32] * torch.einsum("prk,k->pr", A.abs(), x[t].double().abs()) + 1e-30
                r = vt.shape[1]
                got = v[t, :, :(r + 15) // 16 * 16].double().cpu()
                assert ((got[:, :r] - vt).abs() <= vtol).all(), f"{what}: v row {t}"
                assert (got[:, r:] == 0).all(), f"{what}: v row {t} past the rank"


@pytest.mark.parametrize("dt", DTYPES, ids=("f16", "bf16"))
def test_strided_rows_and_same_bytes(gpu_device, dt):
    """x and y as views of wider matrices whose other columns are NaN; two runs give the same bytes."""
    bounds, rk = lc.BOUNDS["qkv_p3"], RANK_SETS["r64_24_4_16"]
    adps = lc.adapters(rk, bounds, dt)
    T, N = 33, bounds[-1]
    slot = lc.pattern("mixed", T)
    w = lc.images(adps, bounds, dt, gpu_device, named=set(slot.tolist()) - {-1})
    x, y0 = lc.activations(T, lc.K, dt), lc.base_output(T, N, dt)
    ref, tol = lc.reference(y0, x, adps, slot, bounds, dt)
    runs = []
    for _ in range(2):
        xw = torch.full((T, lc.K + 24), float("nan"), dtype=dt, device=gpu_device)
        yw = torch.full((T, N + 40), float("nan"), dtype=dt, device=gpu_device)
        xw[:, :lc.K] = x.to(gpu_device)
        yw[:, :N] = y0.to(gpu_device)
        _apply(xw[:, :lc.K], yw[:, :N], w, slot.to(gpu_device))
        close(yw[:, :N], ref, tol, "strided")
        assert torch.isnan(yw[:, N:]).all() and torch.isnan(xw[:, lc.K:]).all()
        runs.append(yw[:, :N].contiguous().cpu().view(torch.int16))
    assert torch.equal(runs[0], runs[1]), "two runs differ"


def test_one_capture_follows_the_slots(gpu_device):
    """group + shrink + expand captured once over a static slot buffer: replays follow three different slot vectors."""
    dt = torch.float16
    bounds, rk = lc.BOUNDS["n528_p2"], RANK_SETS["r1_4_16_24"]
    adps = lc.adapters(rk, bounds, dt)
    T, N = 32, bounds[-1]
    w = lc.images(adps, bounds, dt, gpu_device)
    x, y0 = lc.activations(T, lc.K, dt), lc.base_output(T, N, dt)
    xd, y0d = x.to(gpu_device), y0.to(gpu_device)
    slot_buf = torch.full((T,), -1, dtype=torch.int32, device=gpu_device)
    y = torch.empty_like(y0d)

    def step():
        y.copy_(y0d)
        _apply(xd, y, w, slot_buf)

    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for name in ("round_robin", "mixed", "all_none", "last_alone"):
        slot = lc.pattern(name, T)
        slot_buf.copy_(slot.to(gpu_device))
        graph.replay()
        torch.cuda.synchronize()
        ref, tol = lc.reference(y0, x, adps, slot, bounds, dt)
        close(y, ref, tol, f"replay {name}")
        eager = y0d.clone()
        _apply(xd, eager, w, slot_buf)
        assert torch.equal(eager.view(torch.int16), y.view(torch.int16)), f"replay {name}: graph and eager differ"
