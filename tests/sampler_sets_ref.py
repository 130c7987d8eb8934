"""Group-wise fp64 reference of the next-token chooser's filters for one row: the checker of `tgis_warp_sample` on rows
whose elements are tied (what f16 / bf16 logits are: a bf16 row of 32000 holds a few hundred distinct values).

TEST INFRASTRUCTURE ONLY.  oracle/sampler_ref.warp_row restates the reference with a stable sort and an fp32 cumulative sum,
so it splits a group of equal values by index wherever a top-p boundary falls inside it; no kernel can be held to that
split.  `warp_row_sets` follows warp_row's order (EOS adjustment, repetition penalty, temperature, top-k, top-p, typical-p)
and decides every filter per group of equal values, which is the rule csrc/sampler.hip states for itself: ties with the
k-th value are kept, ties at a top-p / typical-p boundary are kept or removed together.

  pre-warp   fp32, operation by operation as warp_row does it (each a single correctly rounded operation); context ids
             outside [0, V) are skipped, as the kernel skips them (warp_row would index with them);
  top-k      keep s >= kth under float comparison: -0.0 == +0.0;
  top-p      fp64 probabilities, elements grouped by float value (-0.0 and +0.0 are one group), A_g the cumulative group
             mass in ascending value order; every group with A_g <= cut goes, the top group never does;
  typical-p  fp64 log-probabilities and entropy H, groups sorted by |(-logp) - H|; everything up to and including the
             first group whose cumulative mass reaches `mass` stays.

tests/test_sampler_ties_cpu.py pins it to warp_row (and through it to the reference's golden vectors) on tie-free rows.

Margins.  A kernel that sums in fp32 cannot be held to a boundary the fp64 masses miss by less than its own rounding, so
the reference reports how close every decision was (`Margins`), and tests/test_sampler_ties_cpu.py requires of every case
of tests/sampler_cases.py

  mass margin  min over all group boundaries of |A_g - cut| / cut (top-p) or |C_g - mass| / mass (typical-p) > 4 gamma(V),
  dist gap     min over the other groups of the distance in |(-logp) - H| to the boundary group
               > 2^-18 (|log_z| + max|x| + H).

Where gamma comes from.  gamma(V) = (2 (ceil(V / 1024) + 21) + 6) 2^-24 bounds the relative error of one masked probability
sum of the kernel.  The kernel's summation order is fixed: a thread adds at most ceil(V / 1024) terms in sequence, a wave
butterfly adds 6 levels, thread after thread adds the 16 wave partials (15 adds); with recursive summation of positive terms
each add contributes at most one rounding of 2^-24 relative, so one block sum is off by at most (ceil(V / 1024) + 6 + 15)
2^-24 = (ceil(V / 1024) + 21) 2^-24.  A masked sum depends on two of them — the normaliser z and the masked sum itself —
hence the factor 2; the 6 remaining roundings are those of a term: expf (assumed within 2 ulp, which counts as 4 roundings
of half an ulp), the reciprocal of z and the product with it.  That is 6.7e-6 at V = 32768.  The bound is derived, not
measured, and it holds only as far as expf is within 2 ulp."""
import math
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np


def gamma(V: int) -> float:
    return (2 * (-(-V // 1024) + 21) + 6) * 2.0 ** -24


class Margins(NamedTuple):
    top_p_mass: Optional[float]      # min |A_g - cut| / cut, None where top-p did not run
    top_p_boundary: Optional[float]  # value of the lowest group that stays (None: top-p did not run)
    typical_mass: Optional[float]    # min |C_g - mass| / mass
    typical_gap: Optional[float]     # min distance in dist from the boundary group to any other group (inf: no other)
    typical_gap_bar: Optional[float]  # 2^-18 (|log_z| + max|x| + H) of that row


def _groups(s: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(ascending distinct values, group index of every element); -0.0 and +0.0 fall into one group."""
    vals, inv = np.unique(s + np.float32(0.0), return_inverse=True)  # -0.0 + 0.0 is +0.0
    return vals, inv.reshape(-1)


def pre_warp(logits: np.ndarray, *, temperature: float = 1.0, rep_penalty: float = 1.0,
             input_ids: Optional[Sequence[int]] = None, exclude_id: int = -1, eos_id: int = -1, eos_mode: int = 0,
             eos_factor: float = 0.0) -> np.ndarray:
    """EOS adjustment, repetition penalty, temperature: fp32, in warp_row's order and operations."""
    f32 = np.float32
    s = logits.astype(np.float32).copy()
    V = s.shape[0]
    if eos_mode == 1:
        s[eos_id] = -np.inf
    elif eos_mode == 2:
        s[eos_id] = s[eos_id] + np.abs(s[eos_id]) * f32(eos_factor)
    if rep_penalty != 1.0 and input_ids is not None:
        ids = np.unique(np.asarray(input_ids, dtype=np.int64))
        ids = ids[(ids >= 0) & (ids < V) & (ids != exclude_id)]
        seen = s[ids]
        s[ids] = np.where(seen < 0, seen * f32(rep_penalty), seen / f32(rep_penalty))
    return s / f32(temperature)


def top_k_filter(s: np.ndarray, top_k: int) -> np.ndarray:
    s = s.copy()
    if top_k:
        kth = np.sort(s)[::-1][min(top_k, s.shape[0]) - 1]
        s[s < kth] = -np.inf  # float comparison: the two zeros are equal
    return s


def top_p_filter(s: np.ndarray, cut: float) -> Tuple[np.ndarray, float, float]:
    """(filtered row, mass margin, value of the lowest group that stays)."""
    vals, inv = _groups(s)
    x = s.astype(np.float64)
    e = np.exp(x - x.max())
    p = e / e.sum()
    A = np.cumsum(np.bincount(inv, weights=p, minlength=vals.shape[0]))
    remove = A <= float(cut)
    remove[-1] = False
    out = s.copy()
    out[remove[inv]] = -np.inf
    margin = float(np.min(np.abs(A - float(cut)) / float(cut)))
    return out, margin, float(vals[~remove][0])


def typical_filter(s: np.ndarray, mass: float) -> Tuple[np.ndarray, float, float, float]:
    """(filtered row, mass margin, dist gap of the boundary group, the bar that gap is held to)."""
    vals, inv = _groups(s)
    x = s.astype(np.float64)
    m = x.max()
    log_z = m + math.log(np.exp(x - m).sum())
    gv = vals.astype(np.float64)
    glogp = gv - log_z
    gp = np.bincount(inv, weights=np.exp(x - log_z), minlength=vals.shape[0])  # group masses
    finite = ~np.isneginf(gv)
    H = float(-(gp[finite] * glogp[finite]).sum())
    dist = np.abs(-glogp - H)  # inf for the -inf group
    order = np.argsort(dist, kind="stable")
    C = np.cumsum(gp[order])
    reached = np.nonzero(C >= float(mass))[0]
    last = int(reached[0]) if reached.size else int(finite.sum()) - 1
    keep = np.zeros(vals.shape[0], dtype=bool)
    keep[order[:last + 1]] = True
    out = s.copy()
    out[~keep[inv]] = -np.inf
    margin = float(np.min(np.abs(C - float(mass)) / float(mass)))
    others = np.delete(dist, order[last])
    gap = float(np.min(np.abs(others - dist[order[last]]))) if others.size else math.inf
    bar = 2.0 ** -18 * (abs(log_z) + float(np.abs(gv[finite]).max()) + H)
    return out, margin, gap, bar


def warp_row_sets(logits: np.ndarray, *, temperature: float = 1.0, top_k: int = 0, top_p_cut: float = 0.0,
                  typical_p: float = 1.0, rep_penalty: float = 1.0, input_ids: Optional[Sequence[int]] = None,
                  exclude_id: int = -1, eos_id: int = -1, eos_mode: int = 0, eos_factor: float = 0.0
                  ) -> Tuple[np.ndarray, Margins]:
    """Warped scores of one row (float32, -inf where filtered) and how close every decision was."""
    s = pre_warp(logits, temperature=temperature, rep_penalty=rep_penalty, input_ids=input_ids, exclude_id=exclude_id,
                 eos_id=eos_id, eos_mode=eos_mode, eos_factor=eos_factor)
    V = s.shape[0]
    if top_k and top_k < V:
        s = top_k_filter(s, top_k)
    pm = pb = tm = tg = tb = None
    if np.float32(top_p_cut) > 0.0:
        s, pm, pb = top_p_filter(s, float(np.float32(top_p_cut)))
    if np.float32(typical_p) < 1.0:
        s, tm, tg, tb = typical_filter(s, float(np.float32(typical_p)))
    return s, Margins(pm, pb, tm, tg, tb)


def lse64(s: np.ndarray) -> float:
    x = s.astype(np.float64)
    m = x.max()
    return float(m + math.log(np.exp(x - m).sum()))
