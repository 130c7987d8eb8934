"""Prompt-lookup speculative decoding restated in numpy: what tgis_spec_propose, tgis_spec_accept and tgis_spec_stage
(include/tgis_hip.h) must compute, integer for integer.  Plain loops, no cleverness: this is the yardstick."""
import numpy as np

PAGE = 32


def propose(all_ids, positions, K, N):
    """drafts [B, K] int64, hits [B] int32.  The context of request b is all_ids[b, :positions[b] + 1]; for n = N .. 1 the
    largest j with j + n < len and tokens[j:j + n] == tokens[len - n:len]; the first n that has one wins."""
    all_ids = np.asarray(all_ids)
    B = len(positions)
    drafts = np.zeros((B, K), dtype=np.int64)
    hits = np.zeros(B, dtype=np.int32)
    for b in range(B):
        length = min(max(int(positions[b]) + 1, 0), all_ids.shape[1])
        tok = all_ids[b, :length]
        for n in range(N, 0, -1):
            found = -1
            for j in range(0, length - n):  # j + n < len
                if n <= length and np.array_equal(tok[j:j + n], tok[length - n:length]):
                    found = j
            if found >= 0:
                cont = tok[found + n:found + n + K]
                drafts[b, :len(cont)] = cont
                hits[b] = n
                break
    return drafts, hits


def accept(argmax_ids, argmax_lps, drafts, positions, all_ids, cu_seqlens):
    """argmax_ids / argmax_lps [B, K + 1], drafts [B, K] (K may be 0).  Returns a dict of NEW arrays: n_emit [B] int32,
    out_ids [B, K + 1] (-1 behind the emitted), out_lps [B, K + 1] (0 behind them), latest [B], positions [B], all_ids,
    cu_seqlens [B + 1]."""
    argmax_ids = np.asarray(argmax_ids, dtype=np.int64)
    B, K1 = argmax_ids.shape
    K = K1 - 1
    argmax_lps = np.asarray(argmax_lps, dtype=np.float32).reshape(B, K1)
    n_emit = np.zeros(B, dtype=np.int32)
    out_ids = np.full((B, K1), -1, dtype=np.int64)
    out_lps = np.zeros((B, K1), dtype=np.float32)
    latest = np.zeros(B, dtype=np.int64)
    positions = np.array(positions, dtype=np.int64)
    all_ids = np.array(all_ids, dtype=np.int64)
    cu = np.array(cu_seqlens, dtype=np.int32)
    for b in range(B):
        a = 0
        while a < K and argmax_ids[b, a] == drafts[b][a]:
            a += 1
        n = a + 1
        n_emit[b] = n
        out_ids[b, :n] = argmax_ids[b, :n]
        out_lps[b, :n] = argmax_lps[b, :n]
        for j in range(n):
            p = positions[b] + 1 + j
            if 0 <= p < all_ids.shape[1]:
                all_ids[b, p] = argmax_ids[b, j]
        latest[b] = argmax_ids[b, n - 1]
        positions[b] += n
    for b in range(B + 1):
        cu[b] += int(n_emit[:b].sum())
    return dict(n_emit=n_emit, out_ids=out_ids, out_lps=out_lps, latest=latest, positions=positions, all_ids=all_ids,
                cu_seqlens=cu)


def stage(positions, latest, drafts, block_tables):
    """input_ids, positions, slots of the B (K + 1) verify rows and ctx_lens [B]."""
    B = len(positions)
    K = np.asarray(drafts).shape[1] if drafts is not None else 0
    K1 = K + 1
    block_tables = np.asarray(block_tables)
    ids = np.zeros(B * K1, dtype=np.int64)
    pos = np.zeros(B * K1, dtype=np.int32)
    slots = np.zeros(B * K1, dtype=np.int32)
    ctx = np.zeros(B, dtype=np.int32)
    for b in range(B):
        for j in range(K1):
            p = int(positions[b]) + j
            page = block_tables[b, min(p // PAGE, block_tables.shape[1] - 1)]
            ids[b * K1 + j] = latest[b] if j == 0 else drafts[b][j - 1]
            pos[b * K1 + j] = p
            slots[b * K1 + j] = int(page) * PAGE + p % PAGE
        ctx[b] = int(positions[b]) + K1
    return ids, pos, slots, ctx
