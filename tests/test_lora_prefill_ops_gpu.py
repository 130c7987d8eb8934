"""-m gpu: tgis_lora_shrink_tiles + tgis_lora_expand_tiles (csrc/lora_prefill.hip) against the fp64 restatement of the LoRA
contract (tests/lora_ref.py), element by element under the derived bound of tests/lora_cases.py, which assumes fp32 sums of
both products: a v rounded on the way would miss it.

A prefill is a list of (slot, rows) segments, one per request; the tile table is the host's (utils.lora.lora_tile_table).
S = 4 slots of ranks 64, 1, 40 and 24 (read as 64, 16, 48 and 32), K 320 (five k64-steps over the shrink's eight waves) and
every column layout of lora_cases.BOUNDS.  Images are poisoned as in tests/test_lora_ops_gpu.py: NaN in slots no row names
and past a named slot's rank rounded up to 16.  y is a view of a wider NaN matrix, 16-byte aligned rows (pad 40) and not
(pad 44)."""
import pytest
import torch

from tests import lora_cases as lc
from tests.moe_bounds import close
from tgis_amd.utils.lora import lora_tile_table

pytestmark = pytest.mark.gpu

DTYPES = (torch.float16, torch.bfloat16)
RANKS = (64, 1, 40, 24)
SEGMENTS = {
    "one_65": [(2, 65)],                                        # tiles of 64 + 1
    "edges": [(0, 1), (1, 64), (-1, 5), (3, 63), (2, 2)],       # one row, a full tile, a gap at -1, one row short, two rows
    "r64_by_r1": [(0, 130), (1, 3)],                            # three tiles of the widest slot beside the narrowest
    "slot_twice": [(2, 40), (-1, 3), (3, 70), (2, 66)],         # slot 2 in two separate segments
    "none": [(-1, 70)],                                         # n_tiles == 0: nothing is launched
}


def _run(dt, bounds, segs, ranks, K, dev, pads):
    from tgis_amd import native

    slots, rows = [s for s, _ in segs], [n for _, n in segs]
    slot = torch.tensor(slots, dtype=torch.int32).repeat_interleave(torch.tensor(rows))
    T, N = int(slot.numel()), bounds[-1]
    adps = lc.adapters(ranks, bounds, dt, K)
    w = lc.images(adps, bounds, dt, dev, named=set(slots) - {-1}, Kx=K)
    x, y0 = lc.activations(T, K, dt), lc.base_output(T, N, dt)
    ref, tol = lc.reference(y0, x, adps, slot, bounds, dt)
    tiles = native.LoraTiles(lora_tile_table(slots, rows), T, dev)
    assert tiles.n == sum((n + 63) // 64 for s, n in segs if s >= 0)
    xd, outs = x.to(dev), []
    for pad in pads:
        yw = torch.full((T, N + pad), float("nan"), dtype=dt, device=dev)
        yw[:, :N] = y0.to(dev)
        native.lora_expand_tiles(native.lora_shrink_tiles(xd, w, tiles), w, tiles, yw[:, :N])
        close(yw[:, :N], ref, tol, f"pad {pad}")
        assert torch.isnan(yw[:, N:]).all(), f"pad {pad}: columns past N were written"
        y = yw[:, :N].cpu()
        assert torch.equal(y[slot < 0].view(torch.int16), y0[slot < 0].view(torch.int16)), f"pad {pad}: a row at -1 was touched"
        outs.append(y.contiguous().view(torch.int16))
    assert torch.equal(outs[0], outs[1]), "two runs differ"


@pytest.mark.parametrize("segs", sorted(SEGMENTS))
@pytest.mark.parametrize("shape", sorted(lc.BOUNDS))
@pytest.mark.parametrize("dt", DTYPES, ids=("f16", "bf16"))
def test_tiles_delta_in_bound(gpu_device, dt, shape, segs):
    _run(dt, lc.BOUNDS[shape], SEGMENTS[segs], RANKS, lc.K, gpu_device, pads=(40, 40, 44))


@pytest.mark.parametrize("K", (4096, 72), ids=("k4096", "k72_tail"))
@pytest.mark.parametrize("dt", DTYPES, ids=("f16", "bf16"))
def test_deep_k_widest_accumulators(gpu_device, dt, K):
    """q|k|v at rank 64: 2 x 6 accumulators per wave in the shrink.  K 4096: eight k64-steps per wave; K 72: one wave gets a
    k64-step that is only 8 columns wide, the rest of it is zeroed."""
    _run(dt, lc.BOUNDS["qkv_p3"], [(1, 70), (-1, 2), (3, 33)], (64, 64, 64, 64), K, gpu_device, pads=(40, 40))
