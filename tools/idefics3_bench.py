#!/usr/bin/env python3
"""Training-step benchmark of the Idefics3 path (a tool, not bench.py): ms per iteration of a synthetic step at the 8B geometry, and the
achieved GB/s of the pixel-shuffle kernel.

    python tools/idefics3_bench.py [--layers 32] [--tower-layers 27] [--steps 10] [--warmup 3] [--out profiles/idefics3_step.json]

Batch: 2 samples x (4 tiles of 364 x 364 px + 512 text tokens); a tile is 26 x 26 patches -> 169 <image> tokens at scale 2, so a row
holds 512 + 676 = 1188 tokens.  Random weights, `MantisHipTrainer.training_step` (forward + backward into the gradient arena; no
optimizer), timed with HIP events around each step, median.  The shuffle kernel is timed alone on the step's own shape (8 tiles:
[5408, 1152] -> [1352, 4608]) in batches of launches between one event pair, over operand copies that rotate through more than the
last-level cache; bytes = read once + written once."""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
COLD_BYTES = 1 << 30      # a timed kernel's operands rotate over copies totalling at least this much: well past the 256 MiB last-level cache


def _clock():
    """the shader clock the box reports while the benchmark runs (read only), or 'unavailable'"""
    import re
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        lines = [re.sub(r"\s+", " ", l).strip() for l in out.splitlines() if "sclk" in l.lower()]
        return lines[0] if lines else "unavailable"
    except Exception:
        return "unavailable"


def synthetic_batch(cfg, B=2, tiles=4, text_tokens=512, seed=0):
    import torch
    g = torch.Generator().manual_seed(seed)
    S = cfg.vision_config.image_size
    n_tok = (S // cfg.vision_config.patch_size // cfg.scale_factor) ** 2
    T = text_tokens + tiles * n_tok
    ids = torch.randint(1, 128000, (B, T), generator=g)
    gap = text_tokens // (tiles + 1)
    for j in range(tiles):
        s = gap * (j + 1) + j * n_tok
        ids[:, s: s + n_tok] = cfg.image_token_id
    lab = ids.clone()
    lab[:, :8] = -100
    lab[ids == cfg.image_token_id] = -100             # what a collator that wants <image> positions ignored writes on this path
    return dict(input_ids=ids, attention_mask=torch.ones_like(ids), labels=lab, pixel_values=torch.randn(B, tiles, 3, S, S, generator=g))


def step_ms(layers, tower_layers, steps, warmup):
    import torch
    from mantis_amd.configuration_idefics3 import idefics3_8b_llama3
    from mantis_amd.modeling_idefics3 import Idefics3ForConditionalGeneration
    from mantis_amd.trainer import MantisHipTrainer
    cfg = idefics3_8b_llama3()
    cfg.text_config.num_hidden_layers = layers
    cfg.vision_config.num_hidden_layers = tower_layers
    model = Idefics3ForConditionalGeneration(cfg, device="cuda", seed=0)
    tr = MantisHipTrainer(model, gradient_accumulation_steps=1)
    batch = synthetic_batch(cfg)
    ts, loss = [], None
    for i in range(warmup + steps):
        for p in model.parameters():
            p.grad = None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = tr.training_step(model, batch)
        e1.record()
        e1.synchronize()
        if i >= warmup:
            ts.append(e0.elapsed_time(e1))
    B, T = batch["input_ids"].shape
    return dict(ms_per_iter=statistics.median(ts), ms_min=min(ts), ms_max=max(ts), samples_per_s=B / statistics.median(ts) * 1e3,
                loss=float(loss), batch=dict(B=B, T=T, tiles=int(batch["pixel_values"].shape[1])), layers=layers, tower_layers=tower_layers,
                steps=steps, warmup=warmup)


def shuffle_gbs(I=8, H=26, C=1152, s=2, batches=9, warm=1):
    """us per launch from BATCHES of launches between one event pair: a single launch of this kernel (~10 us) between two events would
    time launch and event latency, not the kernel.  One batch = one pass over all operand copies (>= 1 GiB in total: no launch finds its
    operand in the last-level cache); median over the batches."""
    import torch
    import mantis_amd._lib as _lib
    from mantis_amd import hip_ops as K
    nbytes = I * H * H * C * 2
    copies = max(2, -(-COLD_BYTES // (2 * nbytes)))
    xs = [torch.randn(I * H * H, C, device="cuda").to(torch.bfloat16) for _ in range(copies)]
    outs = [torch.empty(I * (H // s) ** 2, s * s * C, dtype=torch.bfloat16, device="cuda") for _ in range(copies)]

    def batch():
        st = K._stream()
        for i in range(copies):
            _lib.check(K._L.mantis_pixel_shuffle(xs[i].data_ptr(), C, outs[i].data_ptr(), s * s * C, I, H, C, s, st), "pixel_shuffle")
    for _ in range(warm):
        batch()
    ts = []
    for _ in range(batches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        batch()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / copies)
    us = statistics.median(ts)
    return dict(shape=[I, H, C, s], us=us, us_min=min(ts), gb_per_s=2 * nbytes / us * 1e-3, bytes=2 * nbytes, launches_per_batch=copies,
                batches=batches)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--tower-layers", type=int, default=27)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = dict(tool="idefics3_bench", clock=_clock(), pixel_shuffle=shuffle_gbs(), step=step_ms(a.layers, a.tower_layers, a.steps, a.warmup))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
