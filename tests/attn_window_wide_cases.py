"""The case grid of tests/test_attn_window_wide_gpu.py (windows wider than four pages), kept free of torch so that
tests/test_attn_window_wide_cpu.py asserts without a GPU, from tests/attn_window_walk.py, that these cases reach the loops they
are there for.  TEST INFRASTRUCTURE.  dtype is "f16" / "bf16" here."""

WINDOWS = (129, 300, 1000, 1024, 4096)
GEOMS = ((4, 4), (8, 2), (8, 1), (20, 1))  # tests/test_attn_window_gpu.py's: MHA, GQA 4 and 8, a padded group of two chunks


def aligned_ctx(W):
    """A ctx whose window starts on a page edge while the sequence ends inside a page: (ctx - W) % 32 == 0, ctx % 32 != 0.
    None where W is a multiple of 32 (1024, 4096): there ctx - W and ctx leave the same remainder."""
    return W + 64 if W % 32 else None


def window_ctxs(W):
    cs = {1, W - 1, W, W + 1, W + 31, W + 32, W + 33, 2 * W + 5}
    if aligned_ctx(W):
        cs.add(aligned_ctx(W))
    return sorted(cs)


def decode_batches(W):
    """As tests/test_attn_window_gpu.py decode_batches: ragged batches of 3, each with the longest ctx in it."""
    ctxs = window_ctxs(W)
    top, rest = ctxs[-1], ctxs[:-1]
    assert top > W
    if len(rest) % 2:
        rest.append(rest[0])
    return [[rest[i], top, rest[i + 1]] for i in range(0, len(rest), 2)]


# (H, Hkv, dtype) per window: every geometry in both types up to W 1024, two at W 4096 (pools of a few tens of MB)
def decode_geoms(W):
    if W <= 1024:
        return [(H, Hkv, dt) for H, Hkv in GEOMS for dt in ("f16", "bf16")]
    return [(8, 2, "f16"), (4, 4, "bf16")]


OTHER_HEAD_SIZES = [(64, "f16", 8, 2), (96, "bf16", 4, 4)]  # (D, dtype, H, Hkv) at W 300 and 1000
OTHER_HEAD_SIZE_WINDOWS = (300, 1000)
FRAGMENT_ORDER_WINDOW = 1000
FP8_WINDOWS = (300, 1000)

# ---- key splits -----------------------------------------------------------------------------------------------------------------
# (name, dtype, H, Hkv, D); ctx 1, 31 and 33 beside the long ones: every split of theirs but the first is unreached
SPLIT_GEOMS = [
    ("g4-d128-f16", "f16", 8, 2, 128),
    ("mha-d64-bf16", "bf16", 4, 4, 64),
    ("g20pad-d128-bf16", "bf16", 20, 1, 128),
    ("g8-d96-f16", "f16", 8, 1, 96),
]
SPLIT_WINDOWS = (1000, 1024, 4096)
EXPLICIT_SPLITS = (2, 5, 9, 13, 40)  # at W 1000: 9 and 13 cross the 8-record merge batch, 40 leave splits without a page
BY_RULE = "rule"                     # the count attn_num_splits gives for min(max_ctx, W + 31)


def split_ctxs(W):
    return [1, 2 * W + 5, 31, W + 33, 33]


def split_cases():
    """(W, name, dtype, H, Hkv, D, ctxs, split counts): every geometry at W 1000, two of them at W 1024 and 4096."""
    out = []
    for W in SPLIT_WINDOWS:
        for g in SPLIT_GEOMS if W == 1000 else SPLIT_GEOMS[:2]:
            out.append((W,) + g + (split_ctxs(W), (BY_RULE,) + (EXPLICIT_SPLITS if W == 1000 else ())))
    return out


# ---- prefill form ---------------------------------------------------------------------------------------------------------------
PREFILL_WINDOWS = (129, 300)
PREFILL = [
    ("mha-d128-f16", "f16", 4, 4, 128),
    ("g4-d128-bf16", "bf16", 8, 2, 128),
    ("g8-d64-f16", "f16", 8, 1, 64),
    ("g20pad-d96-bf16", "bf16", 20, 1, 96),
]
# q_len = ctx in {1, 127, 128, 129, 333, 700} as two ragged batches of 3, and suffixes of 5 and 40 rows over cached tokens.
# (40, 440) starts half-way through a page: its GQA blocks straddle a page edge, which no q_len = ctx block of theirs does, so
# their first waves skip the block's last page by the upper bound.
PREFILL_BATCHES = (
    [(127, 127), (700, 700), (1, 1)],
    [(128, 128), (333, 333), (129, 129)],
    [(5, 700), (40, 440), (40, 450)],
)
