#!/usr/bin/env python
"""The 8-bit GPTQ pack pin: the REFERENCE's own packer (QuantLinear.new(8, ...).pack, run unmodified on CPU) on integers
that cover the extremes — codes 0 and 255, zero points 1 and 256.  Needs /root/reference; the output
(tests/golden/gptq8_pack_reference.npz) is committed, this script is how it was made.  Same recipe as the 4-bit pin of
make_fixtures.py, same harness-side shims, no edits to reference files.

    python tests/golden/make_gptq8_fixture.py"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_fixtures  # noqa: E402  (sets sys.path for the repo; install_shims gives access to the reference)


def main():
    with tempfile.TemporaryDirectory() as tmp:
        make_fixtures.install_shims(tmp)
        from text_generation_server.utils.gptq.quant_linear import QuantLinear

        rng = np.random.default_rng(8)
        K, N, G = 128, 64, 2
        intw = rng.integers(0, 256, size=(K, N)).astype(np.uint8)
        intw[0, :], intw[1, :], intw[K - 1, ::2] = 0, 255, 255
        zeros = rng.integers(1, 257, size=(G, N)).astype(np.int32)  # true zero points; stored as zero - 1
        zeros[0, :4], zeros[1, :4], zeros[0, 4:8], zeros[1, 4:8] = 1, 256, 256, 1
        # powers of two: weights exactly on the grid in fp32, so that pack()'s round() recovers intw
        scales = (2.0 ** -rng.integers(7, 11, size=(G, N))).astype(np.float16)
        ql = QuantLinear.new(8, K // G, K, N, bias=False)
        # QuantLinear.__init__ derives infeatures as rows * 32 // 4 whatever the width (quant_linear.py:267), which is 2 K
        # at 8 bits; pack() loops over it.  Set on the instance here, the reference file is not edited.
        ql.infeatures = K
        g_idx = torch.tensor([i // (K // G) for i in range(K)], dtype=torch.int32)
        w = (torch.from_numpy(intw.astype(np.float32)) - torch.from_numpy(zeros.astype(np.float32))[g_idx.long()]) \
            * torch.from_numpy(scales.astype(np.float32))[g_idx.long()]
        lin = torch.nn.Linear(K, N, bias=False)
        lin.weight.data = w.t().contiguous()
        ql.pack(lin, torch.from_numpy(scales.astype(np.float32)).t().contiguous(),
                torch.from_numpy(zeros.astype(np.float32)).t().contiguous(), g_idx)
        np.savez_compressed(os.path.join(HERE, "gptq8_pack_reference.npz"), intw=intw, zeros=zeros, scales=scales,
                            qweight=ql.qweight.numpy(), qzeros=ql.qzeros.numpy(), ref_scales=ql.scales.numpy(),
                            dequant=w.numpy())
        print("wrote gptq8_pack_reference")


if __name__ == "__main__":
    main()
