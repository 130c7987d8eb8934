"""RankGroup: what the ranks of a tensor-parallel group agree on outside the layers' own collectives (utils/layers.py).

Built once per model from the engine (`world_size`, `rank`, `process_group`; a missing attribute means 1, 0, None) and the model
device.  It is REAL only when there are several ranks and the group is a torch.distributed.ProcessGroup; on one rank, and on
utils/dist.py's FakeGroup standing in for a rank of several (the single-GPU TP emulation in tools/), every method is the
identity on the caller's value and issues nothing.  Small host values are staged on the model device under `nccl` (RCCL
reduces device memory) and on the CPU under any other backend (gloo: TGIS_DIST_BACKEND, the CPU tests).

The invariant every caller holds, and that a change here or in a caller must keep: ON EVERY PATH, ERROR PATHS INCLUDED, EVERY
RANK ISSUES THE SAME SEQUENCE OF COLLECTIVES.  A rank that skips or adds one leaves its peers waiting until the collective
timeout — a hang, not a wrong number.  So a rank that fails does not raise where it fails: it carries its exception to the next
`fail_together`, which every rank calls, and all of them raise there.
"""
from typing import List, Optional, Tuple

import torch
import torch.distributed as dist


class RankGroup:
    def __init__(self, engine, device: torch.device):
        self.world = getattr(engine, "world_size", 1)
        self.rank = getattr(engine, "rank", 0)
        self.process_group = getattr(engine, "process_group", None)
        self.real = self.world > 1 and isinstance(self.process_group, dist.ProcessGroup)
        self.nccl = self.real and dist.get_backend(self.process_group) == "nccl"
        self.device = torch.device(device) if self.nccl else torch.device("cpu")

    def _reduce_int(self, v: int, op) -> int:
        if not self.real:
            return int(v)
        t = torch.tensor([int(v)], dtype=torch.int64, device=self.device)
        dist.all_reduce(t, op=op, group=self.process_group)
        return int(t.item())

    def min_int(self, v: int) -> int:
        return self._reduce_int(v, dist.ReduceOp.MIN)

    def max_int(self, v: int) -> int:
        return self._reduce_int(v, dist.ReduceOp.MAX)

    def all_true(self, ok: bool) -> bool:
        """True iff `ok` holds on every rank."""
        return bool(self.min_int(1 if ok else 0))

    def broadcast_from_rank0(self, values: Optional[List[float]], n: int) -> Optional[List[float]]:
        """Rank 0's `values` (n floats, as float64) on every rank, None where rank 0 had None; what other ranks pass is
        ignored."""
        if not self.real:
            return values
        t = torch.zeros(1 + n, dtype=torch.float64, device=self.device)  # [found, values]
        if self.rank == 0 and values is not None:
            t[0] = 1.0
            t[1:] = torch.tensor(values, dtype=torch.float64)
        dist.broadcast(t, src=0, group=self.process_group)
        vals = t.tolist()
        return vals[1:] if vals[0] == 1.0 else None

    def broadcast_int64_pair(self, a: int, b: int) -> Tuple[int, int]:
        """Rank 0's (a, b) on every rank."""
        if not self.real:
            return a, b
        t = torch.tensor([a, b], dtype=torch.int64, device=self.device)
        dist.broadcast(t, src=0, group=self.process_group)
        a, b = t.tolist()
        return a, b

    def max_reduce(self, tensor: torch.Tensor) -> torch.Tensor:
        """Elementwise max over the ranks; reduced in place under nccl, on a CPU copy otherwise."""
        if not self.real:
            return tensor
        tensor = tensor.to(self.device)
        dist.all_reduce(tensor, op=dist.ReduceOp.MAX, group=self.process_group)
        return tensor

    def fail_together(self, error: Optional[Exception], peer_message: str) -> None:
        """Every rank calls this with its own exception or None (one MIN all-reduce).  A rank holding an error raises it, a
        rank whose peer held one raises ValueError(peer_message); returns only if no rank failed."""
        all_ok = self.all_true(error is None)
        if error is not None:
            raise error
        if not all_ok:
            raise ValueError(peer_message)
