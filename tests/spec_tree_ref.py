"""Speculative decoding over several candidates per request, restated in numpy / fp32 torch: the row layout of a tree verify
step, its attention mask, what tgis_spec_tree_stage, tgis_spec_tree_accept and tgis_spec_propose_multi (include/tgis_hip.h) must
compute integer for integer, which cache positions tgis_spec_tree_commit moves, and an fp32 masked-attention oracle for
tgis_attn_paged_tree.  Plain loops, no cleverness: this is the yardstick."""
import numpy as np
import torch

PAGE = 32


# ---- layout ---------------------------------------------------------------------------------------------------------
def rows(C, K):
    return 1 + C * K


def parents(C, K):
    """parent[r] of every row of one request; row 0 has none (-1).  Row 1 + c K + j is draft j of candidate c: its parent is
    row 0 (j = 0) or the candidate's draft j - 1."""
    par = [-1]
    for c in range(C):
        for j in range(K):
            par.append(0 if j == 0 else 1 + c * K + j - 1)
    return par


def depths(C, K):
    """Rotary offset of every row behind the latest token's position: 0 for row 0, 1 + j for draft j of any candidate."""
    return [0] + [1 + j for _ in range(C) for j in range(K)]


def mask_from_parents(par):
    """Brute force: row r sees row r and every ancestor of it, found by walking up.  One python int (64 bits) per row."""
    words = []
    for r in range(len(par)):
        w, x = 0, r
        while x >= 0:
            w |= 1 << x
            x = par[x]
        words.append(w)
    return words


def q_mask(C, K):
    """The mask of the (C, K) layout in closed form: row 0 sees itself; draft j of candidate c sees row 0 and the
    candidate's drafts 0 .. j."""
    words = [1]
    for c in range(C):
        for j in range(K):
            w = 1
            for i in range(j + 1):
                w |= 1 << (1 + c * K + i)
            words.append(w)
    return words


def as_int64(words):
    """64-bit mask words as the int64 tensor the binding takes (bit 63 becomes the sign)."""
    return torch.from_numpy(np.array([w & (2 ** 64 - 1) for w in words], dtype=np.uint64).view(np.int64).copy())


def commit_moves(pos, C, K, best, n_emit):
    """[(source position, destination position)] of tgis_spec_tree_commit for one request."""
    if best == 0 or n_emit <= 1:
        return []
    return [(pos + 1 + best * K + j, pos + 1 + j) for j in range(n_emit - 1)]


# ---- stage / accept / propose ------------------------------------------------------------------------------------------
def stage(positions, latest, drafts, block_tables):
    """input_ids, positions (by depth), slots (by row) of the B R rows and ctx_lens [B]; drafts [B, C, K]."""
    drafts = np.asarray(drafts)
    B, C, K = drafts.shape
    R = rows(C, K)
    dep = depths(C, K)
    block_tables = np.asarray(block_tables)
    ids = np.zeros(B * R, dtype=np.int64)
    pos = np.zeros(B * R, dtype=np.int32)
    slots = np.zeros(B * R, dtype=np.int32)
    ctx = np.zeros(B, dtype=np.int32)
    flat = drafts.reshape(B, C * K)
    for b in range(B):
        for r in range(R):
            p = int(positions[b]) + r
            page = block_tables[b, min(p // PAGE, block_tables.shape[1] - 1)]
            ids[b * R + r] = latest[b] if r == 0 else flat[b, r - 1]
            pos[b * R + r] = int(positions[b]) + dep[r]
            slots[b * R + r] = int(page) * PAGE + p % PAGE
        ctx[b] = int(positions[b]) + R
    return ids, pos, slots, ctx


def n_correct(argmax_row, drafts_b):
    """a_c per candidate for one request: argmax_row [R], drafts_b [C, K]."""
    C, K = drafts_b.shape
    out = []
    for c in range(C):
        a = 0
        while a < K and argmax_row[0 if a == 0 else 1 + c * K + a - 1] == drafts_b[c, a]:
            a += 1
        out.append(a)
    return out


def accept(argmax_ids, argmax_lps, drafts, positions, all_ids, cu_seqlens):
    """argmax_ids / argmax_lps [B, R], drafts [B, C, K].  Returns NEW arrays: n_emit, best [B] int32, out_ids / out_lps
    [B, K + 1] (-1 / 0 behind the emitted), latest [B], positions [B], all_ids, cu_seqlens [B + 1]."""
    drafts = np.asarray(drafts, dtype=np.int64)
    B, C, K = drafts.shape
    R, K1 = rows(C, K), K + 1
    argmax_ids = np.asarray(argmax_ids, dtype=np.int64).reshape(B, R)
    argmax_lps = np.asarray(argmax_lps, dtype=np.float32).reshape(B, R)
    n_emit = np.zeros(B, dtype=np.int32)
    best = np.zeros(B, dtype=np.int32)
    out_ids = np.full((B, K1), -1, dtype=np.int64)
    out_lps = np.zeros((B, K1), dtype=np.float32)
    latest = np.zeros(B, dtype=np.int64)
    positions = np.array(positions, dtype=np.int64)
    all_ids = np.array(all_ids, dtype=np.int64)
    cu = np.array(cu_seqlens, dtype=np.int32)
    for b in range(B):
        a = n_correct(argmax_ids[b], drafts[b])
        bc = a.index(max(a))  # the lowest c with the largest a_c
        n = a[bc] + 1
        n_emit[b], best[b] = n, bc
        for j in range(n):
            row = 0 if j == 0 else 1 + bc * K + j - 1
            out_ids[b, j] = argmax_ids[b, row]
            out_lps[b, j] = argmax_lps[b, row]
            p = positions[b] + 1 + j
            if 0 <= p < all_ids.shape[1]:
                all_ids[b, p] = argmax_ids[b, row]
        latest[b] = out_ids[b, n - 1]
        positions[b] += n
    for b in range(B + 1):
        cu[b] += int(n_emit[:b].sum())
    return dict(n_emit=n_emit, best=best, out_ids=out_ids, out_lps=out_lps, latest=latest, positions=positions,
                all_ids=all_ids, cu_seqlens=cu)


def reference_best(argmax_ids, drafts):
    """The rule of the reference's process_outputs_with_speculation on its own layout: every candidate is the sequence
    [latest, draft 0 .. K - 1] with the model's choice behind each of its K + 1 tokens; test = inputs.roll(-1).eq(choices)
    .cumprod(); n_correct = test.sum().clamp(0, K); best = argmax (first maximum).  argmax_ids [R] and drafts [C, K] are one
    request's; returns (best, n_correct[best])."""
    C, K = drafts.shape
    n_adds = K + 1
    inputs = np.zeros((C, n_adds), dtype=np.int64)
    choices = np.zeros((C, n_adds), dtype=np.int64)
    for c in range(C):
        inputs[c, 0] = -7  # the latest token: its value only matters through the roll's wrap-around, which the clamp undoes
        inputs[c, 1:] = drafts[c]
        choices[c, 0] = argmax_ids[0]
        for j in range(K):
            choices[c, 1 + j] = argmax_ids[1 + c * K + j]
    test = np.cumprod((np.roll(inputs, -1, axis=1) == choices).astype(np.int64), axis=1)
    nc = np.clip(test.sum(1), 0, n_adds - 1)
    bc = int(np.argmax(nc))
    return bc, int(nc[bc])


def propose_multi(all_ids, positions, C, K, N):
    """drafts [B, C, K] int64, hits [B] int32: sites with n from N down to 1 and within one n from the latest to the
    earliest; a site is taken if its continuation's first token differs from every taken candidate's."""
    all_ids = np.asarray(all_ids)
    B = len(positions)
    drafts = np.zeros((B, C, K), dtype=np.int64)
    hits = np.zeros(B, dtype=np.int32)
    for b in range(B):
        length = min(max(int(positions[b]) + 1, 0), all_ids.shape[1])
        tok = all_ids[b, :length]
        firsts = []
        for n in range(N, 0, -1):
            for j in range(length - n - 1, -1, -1):  # j + n < len, latest first
                if len(firsts) == C:
                    break
                if np.array_equal(tok[j:j + n], tok[length - n:length]) and int(tok[j + n]) not in firsts:
                    cont = tok[j + n:j + n + K]
                    drafts[b, len(firsts), :len(cont)] = cont
                    if not firsts:
                        hits[b] = n
                    firsts.append(int(tok[j + n]))
    return drafts, hits


# ---- attention --------------------------------------------------------------------------------------------------------
def attention_masked(q, k, v, words, scale):
    """One sequence in fp32: q [ql, H, D] are the last ql of the ctx positions of k / v [ctx, Hkv, D].  q row i sees every key
    below ctx - ql, and the key of q row j when bit j of words[i] is set and j <= i.  A row that sees nothing gives zeros."""
    ql, H, D = q.shape
    ctx, Hkv = k.shape[0], k.shape[1]
    G = H // Hkv
    base = ctx - ql
    vis = torch.zeros((ql, ctx), dtype=torch.bool)
    vis[:, :base] = True
    for i in range(ql):
        for j in range(i + 1):
            if (int(words[i]) >> j) & 1:
                vis[i, base + j] = True
    qb = q.float().transpose(0, 1)
    kb = k.float().transpose(0, 1).repeat_interleave(G, dim=0)
    vb = v.float().transpose(0, 1).repeat_interleave(G, dim=0)
    s = torch.matmul(qb, kb.transpose(1, 2)) * scale
    s = s.masked_fill(~vis[None], float("-inf"))
    p = torch.softmax(s, dim=-1)
    p = torch.where(vis.any(1)[None, :, None], p, torch.zeros_like(p))
    return torch.matmul(p, vb).transpose(0, 1)
