"""-m gpu: tgis_kv_absmax (csrc/kv_stats.hip) against a host restatement, BIT-IDENTICAL (a max is exact in any order).

The pools are built on the host with ops_ref.kv_page_pack on top of +-65504 in every slot (the stale tail of a reused page,
as in tests/test_attention_edges_gpu.py): a slot past a sequence's last token, a table entry past its last page (all of them
name a spare page of 65504) or the pool's last page (the null page of a padded decode graph) that reaches the result shows
as 65504.  The last valid token of every sequence holds that sequence's largest |k| and |v|, so a token too few shows too.
Every sequence is also measured alone: in a batch the longest sequence could hide another one's mistake."""
import pytest
import torch

from oracle import ops_ref

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
POISON = 65504.0  # bf16 holds it as 65536
GUARD = 256
# every side of the 16-token tile of the K block and of the 32-token page; 95 = three pages, the last one short by one
CTX = [1, 15, 16, 17, 31, 32, 33, 95]


def _nat():
    from tgis_amd import native

    native.load_library()
    return native


class _Case:
    def __init__(self, dev, dtype, Hkv, D, ctxs, seed, pad=2):
        g = torch.Generator().manual_seed(seed)
        self.dev, self.dtype, self.Hkv, self.D, self.ctxs = dev, dtype, Hkv, D, ctxs
        npages = [(c + 31) // 32 for c in ctxs]
        total = sum(npages) + 2  # + a spare page that the table padding names, + the null page (the pool's last)
        perm = torch.randperm(total - 1, generator=g)
        spare = int(perm[-1])
        bt = torch.full((len(ctxs), max(npages + [1]) + pad), spare, dtype=torch.int32)
        if len(ctxs) > 1:
            bt[-1, -1] = total - 1  # one padding entry names the null page instead

        def poisoned():
            sign = torch.randint(0, 2, (total, Hkv, 32 * D), generator=g, dtype=torch.int8) * 2 - 1
            return (sign.to(torch.float32) * POISON).to(dtype)

        kpool, vpool = poisoned(), poisoned()
        self.K, self.V = [], []
        o = 0
        for b, ctx in enumerate(ctxs):
            # heads of different magnitude, k and v of different magnitude: a swapped row or head shows
            head = (1.0 + torch.arange(Hkv, dtype=torch.float32))[None, :, None]
            K = (torch.randn(ctx, Hkv, D, generator=g) * head).to(dtype)
            V = (torch.randn(ctx, Hkv, D, generator=g) * head * 0.125 + 0.25).to(dtype)
            if ctx:  # the sequence's largest values sit in its last token, 65504 in the slot right after it
                d = int(torch.randint(0, D, (1,), generator=g))
                K[ctx - 1, :, d] = -(8.0 + b) * head[0, :, 0]
                V[ctx - 1, :, D - 1 - d] = (3.0 + b) * head[0, :, 0]
            self.K.append(K)
            self.V.append(V)
            pages = perm[o:o + npages[b]]
            o += npages[b]
            bt[b, :npages[b]] = pages.int()
            for j, pg in enumerate(pages.tolist()):
                ops_ref.kv_page_pack(kpool, vpool, pg, K[32 * j:32 * j + 32], V[32 * j:32 * j + 32])
        self.kpool, self.vpool, self.bt = kpool.to(dev), vpool.to(dev), bt.to(dev)
        self.ctx = torch.tensor(ctxs, dtype=torch.int32, device=dev)

    def want(self, rows=None):
        """[2, Hkv] fp32 on the host: max |x| over the tokens of the given sequences, 0 where there are none."""
        out = torch.zeros(2, self.Hkv, dtype=torch.float32)
        for b in (range(len(self.ctxs)) if rows is None else rows):
            if self.ctxs[b]:
                out[0] = torch.maximum(out[0], self.K[b].float().abs().amax(dim=(0, 2)))
                out[1] = torch.maximum(out[1], self.V[b].float().abs().amax(dim=(0, 2)))
        return out

    def new_out(self):
        """A zeroed [2, Hkv] inside a NaN-filled region."""
        region = torch.full((2 * GUARD + 2 * self.Hkv,), float("nan"), dtype=torch.float32, device=self.dev)
        out = region[GUARD:GUARD + 2 * self.Hkv].view(2, self.Hkv)
        out.zero_()
        return region, out

    def run(self, out, rows=None):
        bt, ctx = (self.bt, self.ctx) if rows is None else (self.bt[rows].contiguous(), self.ctx[rows].contiguous())
        _nat().kv_absmax(self.kpool, self.vpool, bt, ctx, self.Hkv, self.D, out)

    def check(self, region, out, want, what):
        torch.cuda.synchronize()
        got = out.cpu()
        assert torch.equal(got, want), f"{what}: kernel {got.tolist()} != host {want.tolist()}"
        r = region.cpu()
        assert bool(r[:GUARD].isnan().all()) and bool(r[GUARD + 2 * self.Hkv:].isnan().all()), f"{what}: wrote past out"


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("Hkv", [1, 2, 8])
@pytest.mark.parametrize("D", [64, 96, 128])
def test_absmax_is_bit_identical_to_the_host(gpu_device, dtype, Hkv, D):
    c = _Case(gpu_device, dtype, Hkv, D, CTX, seed=1000 + D + Hkv)
    region, out = c.new_out()
    c.run(out)
    c.check(region, out, c.want(), f"batch D={D} Hkv={Hkv}")
    assert float(out.max()) < 1000.0  # far from the 65504 of every slot that does not count
    for b, ctx in enumerate(CTX):
        region, out = c.new_out()
        c.run(out, [b])
        c.check(region, out, c.want([b]), f"ctx={ctx} alone D={D} Hkv={Hkv}")


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_empty_sequences_contribute_nothing(gpu_device, dtype):
    c = _Case(gpu_device, dtype, 2, 128, [0, 40, 0, 7], seed=5)
    assert c.bt[0].eq(c.bt[0, 0]).all()  # an empty sequence's whole table row names the spare page of 65504
    region, out = c.new_out()
    c.run(out)
    c.check(region, out, c.want(), "batch with empty sequences")
    region, out = c.new_out()
    c.run(out, [0, 2])
    c.check(region, out, torch.zeros(2, 2), "only empty sequences")


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("ctx", [1, 16, 17, 33, 63])
def test_last_valid_token_holds_the_maximum(gpu_device, dtype, ctx):
    """One sequence whose largest |k| and |v| sit in the last valid token of a partly filled page: the kernel must reach
    that token and stop before the 65504 right behind it."""
    c = _Case(gpu_device, dtype, 2, 96, [ctx], seed=70 + ctx, pad=1)
    want = c.want()
    assert torch.equal(want[0], c.K[0][ctx - 1].float().abs().amax(dim=1))
    assert torch.equal(want[1], c.V[0][ctx - 1].float().abs().amax(dim=1))
    if ctx > 1:
        assert (c.K[0][:ctx - 1].float().abs().amax(dim=(0, 2)) < want[0]).all()
    region, out = c.new_out()
    c.run(out)
    c.check(region, out, want, f"ctx={ctx}")


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_calls_accumulate(gpu_device, dtype):
    c = _Case(gpu_device, dtype, 8, 64, [33, 5, 64, 20], seed=9)
    region, out = c.new_out()
    c.run(out, [0, 1])
    c.check(region, out, c.want([0, 1]), "first call")
    c.run(out, [2, 3])
    c.check(region, out, c.want(), "second call on the same buffer")
    # what the buffer already holds stays if it is larger
    out[1, 3] = 1.0e6
    want = c.want()
    want[1, 3] = 1.0e6
    c.run(out)
    c.check(region, out, want, "a larger earlier maximum")


def test_no_sequences_is_ok(gpu_device):
    c = _Case(gpu_device, F16, 2, 64, [3], seed=1)
    region, out = c.new_out()
    out.fill_(0.5)
    c.run(out, [])
    c.check(region, out, torch.full((2, 2), 0.5), "B == 0")


def test_bad_arguments_are_refused(gpu_device):
    nat = _nat()
    lib = nat.load_library()
    c = _Case(gpu_device, F16, 2, 64, [3], seed=1)
    region, out = c.new_out()
    good = dict(k=c.kpool.data_ptr(), v=c.vpool.data_ptr(), bt=c.bt.data_ptr(), w=c.bt.shape[1], ctx=c.ctx.data_ptr(), B=1,
                Hkv=2, D=64, dtype=nat.F16, out=out.data_ptr())

    def call(**kw):
        a = {**good, **kw}
        lib.tgis_clear_error()
        rc = lib.tgis_kv_absmax(a["k"], a["v"], a["bt"], a["w"], a["ctx"], a["B"], a["Hkv"], a["D"], a["dtype"], a["out"],
                                None)
        return rc, lib.tgis_last_error()

    for kw in (dict(k=None), dict(v=None), dict(bt=None), dict(ctx=None), dict(out=None),  # null pointers
               dict(D=80), dict(D=0),                                                        # no such head_dim
               dict(dtype=2), dict(dtype=-1),                                                # not a 16-bit element code
               dict(B=-1), dict(w=0), dict(Hkv=0)):
        rc, msg = call(**kw)
        assert rc == -1 and b"tgis_kv_absmax" in msg, (kw, rc, msg)
    # one-byte pools never reach the entry point
    with pytest.raises(nat.TgisHipError):
        nat.kv_absmax(c.kpool.view(torch.uint8), c.vpool.view(torch.uint8), c.bt, c.ctx, 2, 64, out)
    rc, _ = call()
    assert rc == 0
    c.check(region, out, c.want(), "after the refused calls")
