"""CPU restatements of native.rope_kv_write / rope_kv_write_prefill / rope_kv_write_prefill_at with the `qk_norm` keyword, for
tests that replace those functions on the module (tests/test_qwen_dispatch_cpu.py).  TEST INFRASTRUCTURE; tests/cpu_backend.py
stays as it is.

Each function computes what the launch computes (tests/qknorm_ref.py in fp64, rounded once to the model dtype; without qk_norm
the plain rotation), rotates q (and, per token, k) in place, scatters k and v into 16-bit pools in the page layout of
csrc/kv_layout.h, and notes its name and keywords in CALLS."""
import torch

import qknorm_ref

CALLS = []


def k_index(tok, d, D):
    return (((tok >> 4) * (D >> 3) + (d >> 3)) * 16 + (tok & 15)) * 8 + (d & 7)


def v_index(tok, d, D):
    i = tok & 15
    col = (i >> 2) * 8 + (tok >> 4) * 4 + (i & 3)
    return ((col >> 3) * D + d) * 8 + (col & 7)


def _rotated(qkv, cos, sin, positions, H, Hkv, D, rot_dim, qk_norm):
    T = qkv.shape[0]
    x = qkv.view(T, H + 2 * Hkv, D)
    if qk_norm is not None:
        q_w, k_w, eps = qk_norm
        ref, _tol = qknorm_ref.expect(x, q_w, k_w, eps, cos, sin, positions, H, Hkv, rot_dim)
        return ref.to(qkv.dtype)
    out = x.double().clone()
    r = rot_dim // 2
    c, s = cos.double()[positions.long()][:, None], sin.double()[positions.long()][:, None]
    x1, x2 = out[:, :H + Hkv, :r].clone(), out[:, :H + Hkv, r:rot_dim].clone()
    out[:, :H + Hkv, :r], out[:, :H + Hkv, r:rot_dim] = x1 * c - x2 * s, x1 * s + x2 * c
    return out.to(qkv.dtype)


def _scatter(out, slots, k_pool, v_pool, H, Hkv, D):
    slots = slots.long()
    page, tok = slots >> 5, slots & 31
    d = torch.arange(D)
    for h in range(Hkv):
        k_pool[page[:, None], h, k_index(tok[:, None], d[None], D)] = out[:, H + h]
        v_pool[page[:, None], h, v_index(tok[:, None], d[None], D)] = out[:, H + Hkv + h]


def rope_kv_write(qkv, cos, sin, positions, slots, k_pool, v_pool, H, Hkv, D, rot_dim, kv_scales=(1.0, 1.0), qk_norm=None):
    CALLS.append(("rope_kv_write", dict(qk_norm=qk_norm)))
    out = _rotated(qkv, cos, sin, positions, H, Hkv, D, rot_dim, qk_norm)
    _scatter(out, slots, k_pool, v_pool, H, Hkv, D)
    qkv.copy_(out.view(qkv.shape))
    return qkv


def _page_wise(name, qkv, cos, sin, positions, cu_seqlens, block_tables, k_pool, v_pool, H, Hkv, D, rot_dim, past_lens, qk_norm):
    CALLS.append((name, dict(qk_norm=qk_norm)))
    out = _rotated(qkv, cos, sin, positions, H, Hkv, D, rot_dim, qk_norm)
    cu = cu_seqlens.tolist()
    slots = []
    for b in range(len(cu) - 1):
        w = torch.arange(cu[b + 1] - cu[b]) + (0 if past_lens is None else int(past_lens[b]))
        slots.append(block_tables[b, w // 32].long() * 32 + w % 32)
    _scatter(out, torch.cat(slots), k_pool, v_pool, H, Hkv, D)
    qkv.view(qkv.shape[0], -1, D)[:, :H] = out[:, :H]  # (k / v inside qkv are left as they came)
    return qkv


def rope_kv_write_prefill(qkv, cos, sin, positions, cu_seqlens, block_tables, k_pool, v_pool, max_len, H, Hkv, D, rot_dim,
                          kv_scales=(1.0, 1.0), qk_norm=None):
    return _page_wise("rope_kv_write_prefill", qkv, cos, sin, positions, cu_seqlens, block_tables, k_pool, v_pool, H, Hkv, D,
                      rot_dim, None, qk_norm)


def rope_kv_write_prefill_at(qkv, cos, sin, positions, cu_seqlens, block_tables, k_pool, v_pool, max_len, H, Hkv, D, rot_dim,
                             past_lens, kv_scales=(1.0, 1.0), qk_norm=None):
    return _page_wise("rope_kv_write_prefill_at", qkv, cos, sin, positions, cu_seqlens, block_tables, k_pool, v_pool, H, Hkv, D,
                      rot_dim, past_lens, qk_norm)


def install(monkeypatch, native):
    """Replaces the three writers on the `native` module and empties CALLS."""
    CALLS.clear()
    for fn in (rope_kv_write, rope_kv_write_prefill, rope_kv_write_prefill_at):
        monkeypatch.setattr(native, fn.__name__, fn)
