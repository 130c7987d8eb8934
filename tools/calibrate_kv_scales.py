#!/usr/bin/env python3
"""Calibrate the per-layer scales of the one-byte KV cache (kv_cache_dtype="fp8_e4m3") and write kv_cache_scales.json.

    python tools/calibrate_kv_scales.py MODEL_PATH PROMPTS.txt [--dtype float16] [--quantize gptq] [--decode-steps 16]
                                        [--headroom 2.0] [--batch-size 8] [--out MODEL_PATH/kv_cache_scales.json]

PROMPTS.txt holds one prompt per line.  The model runs them on its ordinary 16-bit cache
(FlashCausalLM.calibrate_kv_scales); a model served from MODEL_PATH with the one-byte cache then finds the
file next to its weights.  Tensor parallel: start one process per rank as for serving; rank 0 writes the file."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "text-generation-inference_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("model_path")
    ap.add_argument("prompts", help="text file, one prompt per line")
    ap.add_argument("--dtype", default="float16", choices=["float16", "bfloat16"])
    ap.add_argument("--quantize", default=None, choices=["gptq"])
    ap.add_argument("--decode-steps", type=int, default=16)
    ap.add_argument("--headroom", type=float, default=2.0)
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--max-sequence-length", type=int, default=2048)
    ap.add_argument("--out", default=None, help="default: kv_cache_scales.json in the model directory")
    args = ap.parse_args()

    os.environ["TGIS_KV_CACHE_DTYPE"] = "auto"  # the statistic is taken from the 16-bit cache
    from tgis_amd.models import get_model
    from tgis_amd.pb import generate_pb2
    from tgis_amd.utils.kv_cache import KV_SCALES_FILE, save_kv_scales

    with open(args.prompts) as f:
        prompts = [line.rstrip("\n") for line in f if line.strip()]
    if not prompts:
        sys.exit(f"{args.prompts} holds no prompt")
    lm = get_model(args.model_path, None, "tgis_native", args.dtype, args.quantize, args.max_sequence_length)
    if not hasattr(lm, "calibrate_kv_scales"):
        sys.exit("this model is not served by the flash path: it has no paged KV cache to calibrate")
    limit = args.max_sequence_length - args.decode_steps - 1
    lengths = [min(len(ids), limit) for ids in lm.tokenizer(prompts, return_token_type_ids=False)["input_ids"]]
    batches = []
    for start in range(0, len(prompts), args.batch_size):
        reqs = [generate_pb2.Request(id=i, inputs=prompts[i], input_length=lengths[i], truncate=True,
                                     max_output_length=args.decode_steps + 1)
                for i in range(start, min(start + args.batch_size, len(prompts)))]
        batches.append(generate_pb2.Batch(id=len(batches), requests=reqs))
    stats = lm.calibrate_kv_scales(batches, decode_steps=args.decode_steps, headroom=args.headroom)
    out = args.out or os.path.join(lm.engine.model_path, KV_SCALES_FILE)
    if int(os.getenv("RANK", "0")) == 0:
        save_kv_scales(stats, out)
        print(f"{out}: {stats['tokens']} cached tokens over {stats['num_layers']} layers; k_scale {stats['k_scale']}, "
              f"v_scale {stats['v_scale']}")


if __name__ == "__main__":
    main()
