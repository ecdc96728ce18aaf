#!/usr/bin/env python3
"""Headline benchmark: train samples/s of the Mantis-8B-SigLIP-Llama-3 step on N MI355X (BASELINE.json configs[1]/[2]).

    python bench.py --gpus 1 --steps 5 --warmup 2
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port 29500 \
        bench.py --gpus 8 --steps 5 --warmup 2

One step = one `MantisHipTrainer.training_step` (ViT forward, projector, packing, 32-layer Llama-3 forward + backward,
gradient all-reduce over RCCL when N > 1) followed by the fused clip + AdamW update (`--no-optimizer` times the bare
training_step boundary of the reference, transformers/trainer.py:1892-1963).  Defaults of round 4 (each with a switch): the frozen
vision tower of the NEXT batch is queued at the start of the step on a lowest-priority stream (`--vision-prefetch early`; every
timed step still computes exactly one tower forward), and on a single rank the gradient norm rides in the weight-gradient GEMMs'
epilogues instead of a separate pass (`--no-norm-fold`).  Weak scaling: 2 samples per GPU
(4 images 336x336 + 512 text tokens each -> merged length 2812), random-init weights, and a FRESH synthetic batch every step
(the loss stays at ~ln V = 11.76, it cannot be memorised away, so the timed backward sees random-init operands).

A plain run sets up, warms up, times the K steps (and writes their outputs with `--dump-outputs DIR`) and prints the line; `roofline`
and `cpu_baseline` take runs of their own and are measured only with `--full` (null on a plain line).

Prints ONE JSON line (rank 0) with the driver's fields plus
  ms_per_step_median / p10 / p90   per-step HIP-event durations over the K timed steps
  roofline      (--full) dominant kernel (the bf16 MFMA GEMM family on the compute stream): algorithmic FLOPs / HIP-event time per launch,
                live in the timed steps (`--gemm-table PATH` writes the per-shape table behind it); `traffic` and `mfma_busy_pct` need
                PMC passes this run does not make and are null -- what the builder's own rocprofv3 passes of this command measured
                (profiles/r05_pmc_step.json, tools/pmc_step_report.py) is carried under `pmc_static`
  cpu_baseline  (--full) the oracle's CPU restatement of the same training_step ("port"), timed on this host's cores on a bounded
                sample (1 sample, 1 ViT + {1,2} LLM layers + lm_head) and extrapolated linearly in depth; fp32 is `value`,
                the bf16 leg is reported beside it
  dp            (N > 1) buckets / bytes per step and the time the compute stream waited for RCCL (exposed communication)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FLOP_PER_SAMPLE = 1.351e14      # SURVEY.md section 8d (ViT fwd x1, projector + LLM fwd+bwd x3, causal attention at 1/2)
PEAK_BF16_TFLOPS = 2500.0       # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
PEAK_FP8_TFLOPS = 5000.0        # MI355X dense fp8 MFMA (MX-scaled K = 64 / 128 forms; MI355X_MICROARCH.md)
PMC_JSON = os.path.join(ROOT, "profiles", "r06_pmc_step.json")   # tools/pmc_step_report.py output (offline PMC passes, tracked)
PMC_JSON_QWEN_FP8 = os.path.join(ROOT, "profiles", "r06_pmc_qwen2vl_fp8.json")   # same, for `--config qwen2_vl_7b --precision fp8`


def synthetic_batch(cfg, B, T, n_img, img_hw, rank, step=0):
    import torch
    g = torch.Generator().manual_seed(1234 + rank + 1000 * step)
    ids = torch.randint(0, 128000 if cfg.vocab_size > 128000 else cfg.vocab_size - 2, (B, T), generator=g)
    for b in range(B):
        pos = torch.randperm(T - 1, generator=g)[:n_img].sort().values
        ids[b, pos] = cfg.image_token_index
    labels = ids.clone()
    labels[:, : T // 2] = -100
    labels[ids == cfg.image_token_index] = -100
    pix = [torch.randn(n_img, 3, img_hw, img_hw, generator=g) for _ in range(B)]
    return dict(input_ids=ids, attention_mask=torch.ones_like(ids), labels=labels, pixel_values=pix)


def synthetic_batch_idefics2(cfg, B, T, n_img, img_hw, rank, step=0):
    """BASELINE.json configs[3]: n_img interleaved images of img_hw^2 pixels per sample, each standing for resampler_n_latents <image>
    tokens inside a T-token sequence; labels ignore (= image_token_id, train_idefics2.py:164) the first half and the image tokens."""
    import torch
    g = torch.Generator().manual_seed(4321 + rank + 1000 * step)
    nl, IMG = cfg.perceiver_config.resampler_n_latents, cfg.image_token_id
    ids = torch.randint(3, 32000 if cfg.vocab_size > 32000 else cfg.vocab_size - 3, (B, T), generator=g)
    gap = (T - n_img * nl) // (n_img + 1)
    for b in range(B):
        for j in range(n_img):
            s = gap + j * (nl + gap)
            ids[b, s: s + nl] = IMG
    labels = ids.clone()
    labels[:, : T // 2] = IMG
    pix = torch.randn(B, n_img, 3, img_hw, img_hw, generator=g)
    return dict(input_ids=ids, attention_mask=torch.ones_like(ids), labels=labels, pixel_values=pix, pixel_attention_mask=None)


def idefics2_flop_per_sample(cfg, T, n_img, img_hw):
    """Algorithmic FLOPs of one sample (matmul = 2mnk, causal attention at half, frozen ViT forward only, connector + LLM x3)."""
    vc, pc, tc = cfg.vision_config, cfg.perceiver_config, cfg.text_config
    N = (img_hw // vc.patch_size) ** 2
    dv, iv = vc.hidden_size, vc.intermediate_size
    vit = n_img * vc.num_hidden_layers * N * (2 * (4 * dv * dv + 2 * dv * iv) + 4 * N * dv)
    d, it, nl = tc.hidden_size, tc.intermediate_size, pc.resampler_n_latents
    pq, pkv = pc.resampler_n_heads * pc.resampler_head_dim, pc.num_key_value_heads * pc.resampler_head_dim
    conn = n_img * (N * 2 * (2 * dv * it + it * d)
                    + pc.resampler_depth * ((N + nl) * 2 * 2 * pkv * d + nl * 2 * (2 * pq * d) + 4 * nl * (N + nl) * pq + nl * 2 * 12 * d * d))
    hd = tc.head_dim
    per_tok = 2 * ((tc.num_attention_heads + 2 * tc.num_key_value_heads) * hd * d + tc.num_attention_heads * hd * d + 3 * d * it)
    llm = tc.num_hidden_layers * (T * per_tok + 4 * T * T * tc.num_attention_heads * hd / 2) + T * 2 * d * tc.vocab_size
    return vit + 3 * (conn + llm)


def synthetic_batch_qwen2vl(cfg, B, T, grids, rank, step=0):
    """BASELINE.json configs[4]: per sample the images of `grids` [(t, h, w) in patches] as the Qwen2-VL processor delivers them
    (flattened fp32 patches + image_grid_thw), each standing for t*h*w/4 <|image_pad|> tokens between <|vision_start|> / <|vision_end|>
    inside a T-token sequence; labels ignore (-100) the first half and the image tokens."""
    import torch
    g = torch.Generator().manual_seed(9876 + rank + 1000 * step)
    vc = cfg.vision_config
    mg2 = vc.spatial_merge_size ** 2
    IMG, VS, VE = cfg.image_token_id, cfg.vision_start_token_id, cfg.vision_end_token_id
    ids = torch.randint(3, min(cfg.vocab_size, 151000), (B, T), generator=g)
    ntok = [t * h * w // mg2 for t, h, w in grids]
    gap = (T - sum(n + 2 for n in ntok)) // (len(grids) + 1)
    assert gap >= 1, "sequence too short for the images"
    for b in range(B):
        s = gap
        for n in ntok:
            ids[b, s] = VS
            ids[b, s + 1: s + 1 + n] = IMG
            ids[b, s + 1 + n] = VE
            s += n + 2 + gap
    labels = ids.clone()
    labels[:, : T // 2] = -100
    labels[ids == IMG] = -100
    npatch = sum(t * h * w for t, h, w in grids)
    pix = torch.randn(B * npatch, vc.in_channels * vc.temporal_patch_size * vc.patch_size ** 2, generator=g)
    return dict(input_ids=ids, attention_mask=torch.ones_like(ids), labels=labels, pixel_values=pix,
                image_grid_thw=torch.tensor(list(grids) * B, dtype=torch.int64))


def qwen2vl_flop_per_sample(cfg, T, grids):
    """Algorithmic FLOPs of one sample (matmul = 2mnk, causal attention at half, frozen tower + merger forward only, LLM x3)."""
    vc, tc = cfg.vision_config, cfg.text_config
    dv, iv = vc.embed_dim, int(vc.embed_dim * vc.mlp_ratio)
    dm = dv * vc.spatial_merge_size ** 2
    vit = 0
    for t, h, w in grids:
        N = t * h * w
        vit += N * 2 * vc.in_channels * vc.temporal_patch_size * vc.patch_size ** 2 * dv
        vit += vc.depth * N * (2 * (4 * dv * dv + 2 * dv * iv) + 4 * N * dv)
        vit += (N // vc.spatial_merge_size ** 2) * 2 * (dm * dm + dm * tc.hidden_size)
    d, it, hd = tc.hidden_size, tc.intermediate_size, tc.head_dim
    per_tok = 2 * ((tc.num_attention_heads + 2 * tc.num_key_value_heads) * hd * d + tc.num_attention_heads * hd * d + 3 * d * it)
    llm = tc.num_hidden_layers * (T * per_tok + 4 * T * T * tc.num_attention_heads * hd / 2) + T * 2 * d * tc.vocab_size
    return vit + 3 * llm


class _HostEvent:
    """Stand-in for torch.cuda.Event on the host-only plumbing run (MANTIS_BENCH_DEVICE=cpu, tests/test_bench_launch.py)."""
    def __init__(self, enable_timing=True):
        self.t = None

    def record(self):
        self.t = time.perf_counter()

    def elapsed_time(self, other):
        return 1e3 * (other.t - self.t)


def _self_launch(n):
    """`python bench.py --gpus N` without a launcher around it (the driver's plain command form): re-exec this very command line under
    torch.distributed.run, one rank per GPU, rendezvous on 127.0.0.1; rank 0 of the child job prints the JSON line."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    # torch.distributed.run exports OMP_NUM_THREADS=1 when it is unset, which slows every host-side torch op of the step (index
    # bookkeeping of the packing plan, the CPU baseline): give each rank its share of the cores instead
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or n) // n)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(sys.argv[0]), *sys.argv[1:]]
    raise SystemExit(subprocess.call(cmd, env=env))


def _pct(xs, q):
    xs = sorted(xs)
    if not xs:
        return None
    i = q * (len(xs) - 1)
    lo, hi = int(i), min(int(i) + 1, len(xs) - 1)
    return xs[lo] + (xs[hi] - xs[lo]) * (i - lo)


def write_gemm_table(path, entries, steps, config, step_ms):
    """The in-step bf16 GEMM table: one row per (M, N, K, layout, epilogue) over the launches of the timed steps, from the HIP events
    recorded around every launch on the launch stream (launch.LaunchContext.timer).  Layout: NT = x . W^T (forward), NN = dY . W (dX),
    TN = dY^T . X (dW).  Written as markdown; the last row is the family (= roofline.achieved)."""
    groups = {}
    for x in entries:
        key = x[5] if len(x) > 5 else ("?",)
        groups.setdefault(key, []).append((x[3].elapsed_time(x[4]) * 1e3, x[1]))       # (us, flops)
    fam_us = sum(u for v in groups.values() for u, _ in v)
    fam_fl = sum(f for v in groups.values() for _, f in v)
    rows = []
    for key, v in groups.items():
        us = [u for u, _ in v]
        tot_us, fl = sum(us), sum(f for _, f in v)
        rows.append((tot_us, key, len(v) / steps, tot_us / len(v), min(us), max(us), fl / tot_us / 1e6))
    rows.sort(key=lambda r: -r[0])
    by_lay = {}
    for tot_us, key, *_ in rows:
        lay = key[3] if len(key) > 3 else "?"
        fl = sum(f for _, f in groups[key])
        a = by_lay.setdefault(lay, [0.0, 0.0])
        a[0] += tot_us
        a[1] += fl
    with open(path, "w") as fh:
        fh.write(f"# in-step bf16 GEMM table -- `bench.py --config {config}`, {steps} timed steps, step {step_ms:.1f} ms\n\n"
                 "HIP events around every launch of the timed steps (the numbers `roofline.achieved` is built from).  "
                 "NT = forward, NN = dX, TN = dW.\n\n"
                 "| M x N x K | layout | epilogue | launches/step | mean us | min us | max us | TFLOP/s | frac of 2.5 PF | ms/step | % of family |\n"
                 "|---|---|---|---|---|---|---|---|---|---|---|\n")
        for tot_us, key, n, mean, lo, hi, tf in rows:
            shape = " x ".join(str(k) for k in key[:3]) if len(key) > 3 else "?"
            fh.write(f"| {shape} | {key[3] if len(key) > 3 else '?'} | {key[4] if len(key) > 4 else '?'} | {n:g} | {mean:.1f} | {lo:.1f} | {hi:.1f} | "
                     f"{tf:.0f} | {tf / PEAK_BF16_TFLOPS:.3f} | {tot_us / steps / 1e3:.2f} | {100 * tot_us / fam_us:.1f} |\n")
        fh.write("\n| layout | ms/step | TFLOP/s | frac of 2.5 PF |\n|---|---|---|---|\n")
        for lay, (u, fl) in sorted(by_lay.items()):
            fh.write(f"| {lay} | {u / steps / 1e3:.2f} | {fl / u / 1e6:.0f} | {fl / u / 1e6 / PEAK_BF16_TFLOPS:.3f} |\n")
        fh.write(f"| family | {fam_us / steps / 1e3:.2f} | {fam_fl / fam_us / 1e6:.0f} | {fam_fl / fam_us / 1e6 / PEAK_BF16_TFLOPS:.3f} |\n")


DUMP_SAMPLE = 1 << 21           # elements of params.npy / grads.npy: 2 x 8 MB


def dump_outputs(path, model, loss):
    """`--dump-outputs`: what the last timed step handed its caller -- the loss, the trainable parameters after the optimizer update and
    the gradients its backward left in the gradient arena (`.grad` views are dropped by zero_grad, the arena keeps them) -- as float32
    .npy files.  Parameters and gradients are sampled at the same DUMP_SAMPLE flat positions over the trainable parameters in
    named_parameters() order, drawn from a fixed seed, so two builds of the project compare element for element."""
    import numpy as np
    import torch
    os.makedirs(path, exist_ok=True)
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    sizes = np.array([p.numel() for _, p in named], dtype=np.int64)
    total = int(sizes.sum())
    idx = np.arange(total) if total <= DUMP_SAMPLE else np.unique(np.random.default_rng(0).integers(0, total, DUMP_SAMPLE))
    seg = np.searchsorted(np.cumsum(sizes), idx, side="right")
    starts = np.cumsum(sizes) - sizes
    grads = getattr(model, "_grad_views", None) or {}
    ps, gs = [], []
    with torch.no_grad():
        for s in np.unique(seg):
            n, p = named[s]
            local = torch.from_numpy(idx[seg == s] - starts[s]).to(p.device)
            ps.append(p.detach().reshape(-1)[local].float())
            g = grads.get(n, p.grad)
            gs.append(g.reshape(-1)[local].float() if g is not None else torch.full_like(ps[-1], float("nan")))
    np.save(os.path.join(path, "loss.npy"), np.array([float(loss)], dtype=np.float32))
    np.save(os.path.join(path, "params.npy"), torch.cat(ps).cpu().numpy())
    np.save(os.path.join(path, "grads.npy"), torch.cat(gs).cpu().numpy())


def cpu_baseline(cfg_name):
    """Oracle ("port") timing on the host cores; bounded sample, depth extrapolated.  Returns the cpu_baseline object."""
    import torch
    from oracle.llava_ref import LlavaRef, random_weights
    from mantis_amd import configuration_llava as C
    cfg = getattr(C, cfg_name)()
    full_v, full_l = cfg.vision_config.num_hidden_layers + cfg.vision_feature_layer + 1, cfg.text_config.num_hidden_layers
    meta = dict(vision=cfg.vision_config.to_dict(), text=cfg.text_config.to_dict(), image_token_index=cfg.image_token_index,
                pad_token_id=cfg.pad_token_id, vision_feature_select_strategy=cfg.vision_feature_select_strategy,
                vision_feature_layer=cfg.vision_feature_layer, projector_hidden_act=cfg.projector_hidden_act)
    meta["vision"]["num_hidden_layers"] = 2
    meta["text"]["num_hidden_layers"] = 2
    tiny = cfg_name == "mantis_tiny"
    batch = synthetic_batch(cfg, 1, 128 if tiny else 512, 1 if tiny else 4, cfg.vision_config.image_size, 0)

    def leg(dtype):
        w = random_weights(meta, seed=0, dtype=dtype)
        model = LlavaRef(w, meta, dtype=dtype)
        del w

        with torch.no_grad():
            pv = torch.cat(batch["pixel_values"], 0).to(dtype)
            t0 = time.perf_counter(); model.vision_tower(pv, 1); tv1 = time.perf_counter() - t0
            t0 = time.perf_counter(); model.vision_tower(pv, 2); tv2 = time.perf_counter() - t0
        # the whole step at depth 1 (tower layer, projector, merge, ONE decoder layer, lm_head + loss, backward) ...
        rec = {}
        model.zero_grad()
        t0 = time.perf_counter()
        model.training_step(batch, n_vit_layers=1, n_llm_layers=1, record=rec)
        t11 = time.perf_counter() - t0
        # ... and one more decoder layer on its own (forward + backward on the merged sequence length): ~30 s of host work for both
        # precisions together instead of ~80 s for timing the step again at depth 2
        L, d = rec["llm_final_norm"].shape[1], rec["llm_final_norm"].shape[2]
        del rec
        model.zero_grad()
        g = torch.Generator().manual_seed(1)
        x = torch.randn(1, L, d, generator=g).to(dtype).requires_grad_(True)
        t0 = time.perf_counter()
        y = model.decoder(x, torch.ones(1, L, dtype=torch.int64), torch.arange(L)[None], n_layers=1)
        y.float().sum().backward()
        per_llm = max(time.perf_counter() - t0, 1e-9)
        model.zero_grad()
        per_vit = max(tv2 - tv1, 1e-9)
        total = t11 + (full_l - 1) * per_llm + (full_v - 1) * per_vit
        return total, t11, per_llm, per_vit
    total, t11, per_llm, per_vit = leg(torch.float32)
    out = dict(value=1.0 / total, unit="samples/s", cores=torch.get_num_threads(), kind="port",
               sample=f"oracle/llava_ref.py training_step, fp32, 1 sample ({'1 img 224^2 + 128' if tiny else '4 img 336^2 + 512'} "
                      f"tok), measured: the step with 1 ViT + 1 LLM layer + lm_head {t11:.1f}s, one more LLM layer fwd+bwd {per_llm:.1f}s, "
                      f"one more ViT layer {per_vit:.2f}s; extrapolated linearly to {full_v} ViT / {full_l} LLM layers = {total:.0f}s per sample")
    try:
        tb, b11, bl, _ = leg(torch.bfloat16)
        out["value_bf16"] = 1.0 / tb
        out["sample_bf16"] = f"same sample and extrapolation with bf16 weights/activations on the CPU ({b11:.1f}s, +{bl:.1f}s per LLM layer) = {tb:.0f}s per sample"
    except Exception as e:  # a CPU without usable bf16 kernels must not take the bench line down
        out["value_bf16"] = None
        out["sample_bf16"] = f"bf16 leg failed: {type(e).__name__}: {e}"
    return out


def cpu_baseline_qwen2vl(cfg, T, grids):
    """Qwen2-VL configuration: the oracle (oracle/qwen2vl_ref.py, "port") on the host cores, fp32, one sample, depth extrapolated."""
    import torch
    from oracle.qwen2vl_ref import Qwen2VLRef
    from mantis_amd.modeling_qwen2_vl import _param_specs
    full_v, full_l = cfg.vision_config.depth, cfg.text_config.num_hidden_layers
    meta = dict(vision=cfg.vision_config.to_dict(), text=cfg.text_config.to_dict(), image_token_id=cfg.image_token_id)
    g = torch.Generator().manual_seed(0)
    w = {}
    for name, shape in _param_specs(cfg):
        if ".blocks." in name and int(name.split(".blocks.")[1].split(".")[0]) >= 2:
            continue
        if ".layers." in name and int(name.split(".layers.")[1].split(".")[0]) >= 2:
            continue
        if len(shape) == 1:
            w[name] = torch.ones(shape) if (("norm" in name or "ln_q" in name) and name.endswith("weight")) else torch.zeros(shape)
        else:
            w[name] = torch.randn(shape, generator=g).mul_(0.02)
    model = Qwen2VLRef(w, meta)
    del w
    batch = synthetic_batch_qwen2vl(cfg, 1, T, grids, 0)

    # the whole step at depth 1 (patch embedding, ONE tower block, merger, rope index, ONE decoder layer, lm_head + loss, backward) ...
    model.zero_grad()
    t0 = time.perf_counter()
    loss, _ = model.forward(batch["input_ids"], batch["pixel_values"], batch["image_grid_thw"], batch["attention_mask"], batch["labels"],
                            n_vit_layers=1, n_llm_layers=1)
    loss.backward()
    t11 = time.perf_counter() - t0
    del loss
    model.zero_grad()
    # ... one more tower block (frozen: forward only) as the difference of two tower forwards, and one more decoder layer (forward +
    # backward) on its own
    with torch.no_grad():
        t0 = time.perf_counter(); model.vision(batch["pixel_values"].float(), batch["image_grid_thw"], n_layers=1); tv1 = time.perf_counter() - t0
        t0 = time.perf_counter(); model.vision(batch["pixel_values"].float(), batch["image_grid_thw"], n_layers=2); tv2 = time.perf_counter() - t0
    x = torch.randn(1, T, cfg.text_config.hidden_size, generator=g).requires_grad_(True)
    pos3 = torch.arange(T)[None, None].expand(3, 1, T)
    t0 = time.perf_counter()
    model.text(x, torch.ones(1, T, dtype=torch.int64), pos3, n_layers=1).sum().backward()
    per_llm = max(time.perf_counter() - t0, 1e-9)
    model.zero_grad()
    per_vit = max(tv2 - tv1, 1e-9)
    total = t11 + (full_v - 1) * per_vit + (full_l - 1) * per_llm
    return dict(value=1.0 / total, unit="samples/s", cores=torch.get_num_threads(), kind="port",
                sample=f"oracle/qwen2vl_ref.py forward + backward, fp32, 1 sample ({len(grids)} images of {grids[0][1]}x{grids[0][2]} patches + "
                       f"{T} tokens), measured: the step with 1 tower block + 1 decoder layer + merger + lm_head {t11:.1f}s, one more tower block "
                       f"(frozen, forward) {per_vit:.1f}s, one more decoder layer fwd+bwd {per_llm:.1f}s; extrapolated linearly to {full_v} blocks / {full_l} layers = {total:.0f}s per sample")


def cpu_baseline_idefics2(cfg, T, n_img, img_hw):
    """Idefics2 configuration: the oracle (oracle/idefics2_ref.py, "port") on the host cores, fp32, one sample, depth extrapolated
    (connector / resampler at full depth: it is 3 blocks)."""
    import torch
    from oracle.idefics2_ref import Idefics2Ref
    from mantis_amd.modeling_idefics2 import _param_specs
    full_v, full_l = cfg.vision_config.num_hidden_layers, cfg.text_config.num_hidden_layers
    meta = dict(vision=cfg.vision_config.to_dict(), perceiver=cfg.perceiver_config.to_dict(), text=cfg.text_config.to_dict(),
                image_token_id=cfg.image_token_id)
    g = torch.Generator().manual_seed(0)
    w = {}
    for name, shape in _param_specs(cfg):
        if ".layers." in name and "perceiver_resampler" not in name and int(name.split(".layers.")[1].split(".")[0]) >= 2:
            continue
        if len(shape) == 1:
            w[name] = torch.ones(shape) if ("norm" in name and name.endswith("weight")) else torch.zeros(shape)
        else:
            w[name] = torch.randn(shape, generator=g).mul_(0.02)
    model = Idefics2Ref(w, meta)
    del w
    batch = synthetic_batch_idefics2(cfg, 1, T, n_img, img_hw, 0)
    # the whole step at depth 1 (NaViT embeddings, ONE tower layer, connector, merge, ONE decoder layer, lm_head + loss, backward) ...
    model.vc["num_hidden_layers"] = model.tc["num_hidden_layers"] = 1
    model.zero_grad()
    t0 = time.perf_counter()
    loss, _ = model.forward(batch["input_ids"], batch["pixel_values"], None, batch["attention_mask"], batch["labels"])
    loss.backward()
    t11 = time.perf_counter() - t0
    del loss
    model.zero_grad()
    # ... one more tower layer (frozen: forward only) as the difference of two tower forwards, one more decoder layer (fwd + bwd) alone
    pv = batch["pixel_values"].reshape(-1, *batch["pixel_values"].shape[2:]).float()
    pm = torch.ones(pv.shape[0], img_hw // cfg.vision_config.patch_size, img_hw // cfg.vision_config.patch_size, dtype=torch.bool)
    with torch.no_grad():
        t0 = time.perf_counter(); model.vision(pv, pm); tv1 = time.perf_counter() - t0
        model.vc["num_hidden_layers"] = 2
        t0 = time.perf_counter(); model.vision(pv, pm); tv2 = time.perf_counter() - t0
    x = torch.randn(1, T, cfg.text_config.hidden_size, generator=g).requires_grad_(True)
    t0 = time.perf_counter()
    model.text(x, torch.ones(1, T, dtype=torch.int64)).sum().backward()
    per_llm = max(time.perf_counter() - t0, 1e-9)
    model.zero_grad()
    per_vit = max(tv2 - tv1, 1e-9)
    total = t11 + (full_v - 1) * per_vit + (full_l - 1) * per_llm
    return dict(value=1.0 / total, unit="samples/s", cores=torch.get_num_threads(), kind="port",
                sample=f"oracle/idefics2_ref.py forward + backward, fp32, 1 sample ({n_img} images of {img_hw}^2 px + {T} tokens), measured: the "
                       f"step with 1 tower layer + connector + 1 decoder layer + lm_head {t11:.1f}s, one more tower layer (frozen, forward) "
                       f"{per_vit:.1f}s, one more decoder layer fwd+bwd {per_llm:.1f}s; extrapolated linearly to {full_v} tower / {full_l} "
                       f"decoder layers = {total:.0f}s per sample")


def run_hf_loop(args, model, batches, B, Event, sync, vmode):
    """The timed workload through `transformers.Trainer.train()` (the loop the reference drives, train_mllava.py:312-329) with
    `as_hf_trainer()`'s training_step: one Dataset item = one pre-built pinned batch of B samples, served in order by HF's own DataLoader;
    optimizer, LR scheduler, clip_grad_norm_ call and zero_grad are the loop's.  Returns what the native loop's bookkeeping produces:
    (elapsed seconds over the timed steps, per-step event triples, losses, GEMM timer entries, the batches of the timed steps)."""
    import tempfile
    import torch
    import transformers
    from torch.utils.data import Dataset, SequentialSampler
    from mantis_amd.trainer import as_hf_trainer
    W, Kt = args.warmup, args.steps
    total = W + Kt

    class Batches(Dataset):
        def __len__(self):
            return total + 1                     # + 1: the last timed step, too, has a successor to prefetch (as in the native loop)

        def __getitem__(self, i):
            return i
    state = dict(t0=None, t1=None, split=[], losses=[], timer=[], fed=[], cur=None)

    class Timed(as_hf_trainer()):
        mantis_prefetch = "early" if vmode == "early" else None

        def _get_train_sampler(self, *a, **k):
            return SequentialSampler(self.train_dataset)

        def training_step(self, model_, inputs, num_items_in_batch=None):
            timed = self.state.global_step >= W
            impl = getattr(self, "_mantis_impl", None)
            if impl is not None:
                impl.launch.timer = None          # bare, like the native loop's timed region: `roofline` comes from the native loop's instrumented steps
            loss = super().training_step(model_, inputs, num_items_in_batch)
            if timed and state["cur"] is not None:
                state["cur"][1].record()
                state["losses"].append(loss)
                state["fed"].append(inputs)
            return loss

    class Clock(transformers.TrainerCallback):
        def on_step_begin(self, a, st, control, **kw):
            if st.global_step == W:
                sync()
                state["t0"] = time.perf_counter()
            if st.global_step >= W:
                state["cur"] = [Event(enable_timing=True) for _ in range(3)]
                state["cur"][0].record()

        def on_step_end(self, a, st, control, **kw):
            if state["cur"] is not None:
                state["cur"][2].record()
                state["split"].append(state["cur"])
                state["cur"] = None
            if st.global_step == total:
                sync()
                state["t1"] = time.perf_counter()
    targs = transformers.TrainingArguments(
        output_dir=tempfile.mkdtemp(), report_to=[], remove_unused_columns=False, per_device_train_batch_size=1,
        gradient_accumulation_steps=1, max_steps=total, learning_rate=1e-5, weight_decay=0.0, max_grad_norm=1.0, lr_scheduler_type="cosine",
        warmup_steps=1, save_strategy="no", logging_strategy="no", logging_nan_inf_filter=False, disable_tqdm=True,
        dataloader_pin_memory=False, dataloader_num_workers=0, seed=0)
    tr = Timed(model=model, args=targs, train_dataset=Batches(), data_collator=lambda idx: batches[idx[0] % len(batches)], callbacks=[Clock()])
    for cb in (transformers.PrinterCallback, transformers.ProgressCallback):      # stdout carries exactly one JSON line
        tr.remove_callback(cb)
    tr.train()
    if state["t1"] is None:
        sync()
        state["t1"] = time.perf_counter()
    impl = getattr(tr, "_mantis_impl", None)
    if impl is not None:
        impl.launch.timer = None
    return state["t1"] - state["t0"], state["split"], state["losses"], state["timer"], state["fed"], tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", default="mantis_8b_siglip_llama3",
                    choices=["mantis_8b_siglip_llama3", "mantis_8b_clip_llama3", "mantis_tiny", "mantis_8b_idefics2", "qwen2_vl_7b"],
                    help="mantis_8b_siglip_llama3 = the headline (BASELINE.json configs[1]/[2]); mantis_8b_idefics2 = configs[3] "
                         "(8 interleaved images x 448^2 and 2048 tokens per sample, 2 samples per GPU packed into one row); "
                         "qwen2_vl_7b = configs[4] (two 1280x960 dynamic-resolution images = 2 x 6256 patches -> 2 x 1564 tokens "
                         "inside a 4096-token sample)")
    ap.add_argument("--precision", default=None, choices=["bf16", "fp8", "fp8_rowwise"],
                    help="decoder linears: bf16 MFMA or fp8 (e4m3 / e5m2) MFMA with per-tensor scaling (fp8_rowwise: the opt-in finer "
                         "recipe, one scale per token / feature).  Default: fp8 for qwen2_vl_7b (BASELINE configs[4] names fp8 MFMA), "
                         "bf16 otherwise")
    ap.add_argument("--batch-per-gpu", type=int, default=None, help="samples per GPU and step (default 2 on every configuration)")
    ap.add_argument("--stage", default="finetune", choices=["finetune", "pretrain"],
                    help="finetune: projector + LLM trainable (the headline metric); pretrain: only multi_modal_projector "
                         "(the reference's stage 1, train_mllava.py:177-181)")
    ap.add_argument("--no-pack", action="store_true", help="Idefics2 config: feed the samples as a batch instead of one packed row")
    ap.add_argument("--vision-prefetch", default="early", choices=["early", "optimizer", "off"],
                    help="what training_step does with the NEXT batch (what a DataLoader with prefetch_factor already holds).  early (default): "
                         "its frozen vision tower is queued at the START of the step on a stream of the lowest hardware-queue priority and "
                         "fills the compute units the step's own kernels leave idle in incomplete tile rounds (measured -4 ... -5 ms per "
                         "step, profiles/r04_experiments.md 3; every timed step still computes exactly one tower forward: the next "
                         "batch's instead of its own).  optimizer: queued behind the backward, beside clip + AdamW on CU-masked streams "
                         "(--adam-cus; measured slower, profiles/r02_experiments.md).  off: every step computes its own tower in line")
    ap.add_argument("--prefetch", action="store_true", help="alias of --vision-prefetch optimizer (round-2 flag)")
    ap.add_argument("--prefetch-early", action="store_true", help="alias of --vision-prefetch early")
    ap.add_argument("--adam-cus", type=int, default=192, help="with --prefetch: compute units given to the optimizer pass")
    ap.add_argument("--no-optimizer", action="store_true")
    ap.add_argument("--gradient-checkpointing", action="store_true",
                    help="activation checkpointing per decoder layer (the reference launches with --gradient_checkpointing True, "
                         "train_mllava.sh:168): one kept tensor per layer, the layer forward runs again in the backward -- same results, "
                         "less memory, more time; NOT the default line (288 GB hold the activations of every configuration)")
    ap.add_argument("--no-norm-fold", action="store_true",
                    help="keep clip_grad_norm_'s separate pass over the gradients also on a single rank (default there: the sum of squares rides "
                         "in the weight-gradient GEMMs' epilogues)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-kernel-timer", action="store_true")
    ap.add_argument("--gemm-table", default=None, metavar="PATH",
                    help="write the in-step bf16 GEMM table (per shape x layout x epilogue: launches per step, mean / min / max us from the "
                         "HIP events around every launch of the timed steps, TFLOP/s, fraction of the bf16 MFMA peak, share of the family) "
                         "as markdown to PATH")
    ap.add_argument("--gemm-series", default=None, metavar="PATH",
                    help="write the (shape, layout, epilogue, us) of every bf16 GEMM launch of the LAST timed step, in launch order, as JSON")
    ap.add_argument("--recycle-batches", type=int, default=0, help="0 = a fresh synthetic batch every step (default); n > 0 = cycle n batches")
    ap.add_argument("--loop", default="native", choices=["native", "hf"],
                    help="native (default, the driver's line): the transformers-free MantisHipTrainer loop.  hf: the SAME workload through the "
                         "reference's own loop -- `as_hf_trainer()` + `transformers.Trainer.train()` on a synthetic Dataset (train_mllava.py:312-329: "
                         "HF's dataloader, get_batch_samples, the fused optimizer from create_optimizer, HF's scheduler / clip call / zero_grad), "
                         "after the native loop has been timed in the same process; the JSON line then describes the HF loop and carries the "
                         "native numbers and the difference under `native_loop` (N = 1 only)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what takes runs of its own: the instrumented steps behind `roofline` (--no-kernel-timer drops them) and "
                         "the CPU baseline (--no-cpu-baseline drops it).  Without it both are null on the line")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step computed as float32 .npy files to DIR: loss.npy, and a fixed "
                         "seeded sample of the trainable parameters after the update (params.npy) and of the gradients of its backward "
                         "(grads.npy), the same elements in both")
    args = ap.parse_args()
    if (args.gemm_table or args.gemm_series) and not args.full:
        ap.error("--gemm-table / --gemm-series come from the instrumented steps: add --full")

    if args.gpus > 1 and "RANK" not in os.environ:
        _self_launch(args.gpus)
    import mantis_amd  # noqa: F401  (sets GPU_MAX_HW_QUEUES before the HIP runtime initialises: the RCCL stream needs its own hardware queue)
    import torch
    import torch.distributed as dist
    import __graft_entry__
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
    # MANTIS_BENCH_DEVICE=cpu: host-only plumbing run of this script (launcher, rank wiring, gloo reduction, JSON contract) for
    # tests/test_bench_launch.py, whose harness installs a CPU operator backend first; without such a harness the product operators
    # refuse host tensors.  Never a measurement.
    host_only = os.environ.get("MANTIS_BENCH_DEVICE") == "cpu"
    on_gpu = not host_only
    if local_rank == 0 and on_gpu:
        __graft_entry__.build()
    if on_gpu:
        torch.cuda.set_device(local_rank)
    device = f"cuda:{local_rank}" if on_gpu else "cpu"
    Event = torch.cuda.Event if on_gpu else _HostEvent
    sync = torch.cuda.synchronize if on_gpu else (lambda: None)
    force_dp = os.environ.get("MANTIS_DP_FORCE") == "1" and "RANK" in os.environ
    if world > 1 or force_dp:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if on_gpu:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group("gloo")
        dist.barrier()
        # the line that is printed must describe the job that ran: the communicator itself has to report N ranks (not only the launcher's
        # environment), or no line is printed at all
        if dist.get_world_size() != max(1, args.gpus) and not force_dp:
            raise SystemExit(f"--gpus {args.gpus} but the process group has {dist.get_world_size()} ranks: refusing to print a bench line")
    from mantis_amd import configuration_llava as C
    from mantis_amd import hip_ops as K
    from mantis_amd.modeling_llava import LlavaForConditionalGeneration
    from mantis_amd.trainer import MantisHipTrainer
    from mantis_amd.dp import GradReducer
    from mantis_amd.optim import FusedAdamW

    idefics = args.config == "mantis_8b_idefics2"
    qwen = args.config == "qwen2_vl_7b"
    tiny = args.config == "mantis_tiny"
    grids = None
    if qwen:
        from mantis_amd import configuration_qwen2_vl as C3
        from mantis_amd.modeling_qwen2_vl import Qwen2VLForConditionalGeneration
        cfg = C3.qwen2_vl_7b()
        B = args.batch_per_gpu or 2          # 2 samples per GPU like the headline configuration (measured: 1 -> 4.39, 2 -> 5.10 samples/s)
        # 1280 x 960 px -> smart_resize to multiples of 28: 1288 x 952 -> 92 x 68 patches of 14 px (max_pixels raised to hold it,
        # train_qwen2_vl.py:126-128's default budget would shrink it)
        T, grids = 4096, [(1, 68, 92), (1, 68, 92)]
        n_img, img_hw = len(grids), None
        model = Qwen2VLForConditionalGeneration(cfg, device=device, seed=0)
        flop_per_sample = qwen2vl_flop_per_sample(cfg, T, grids)
    elif idefics:
        from mantis_amd import configuration_idefics2 as C2
        from mantis_amd.modeling_idefics2 import Idefics2ForConditionalGeneration
        cfg = C2.mantis_8b_idefics2()
        B = args.batch_per_gpu or 2
        T, n_img, img_hw = 2048, 8, 448
        model = Idefics2ForConditionalGeneration(cfg, device=device, seed=0)
        flop_per_sample = idefics2_flop_per_sample(cfg, T, n_img, img_hw)
    else:
        cfg = getattr(C, args.config)()
        B = args.batch_per_gpu or 2
        T, n_img = (128, 1) if tiny else (512, 4)
        img_hw = cfg.vision_config.image_size
        model = LlavaForConditionalGeneration(cfg, device=device, seed=0)      # same seed -> identical replicas
        flop_per_sample = FLOP_PER_SAMPLE
    precision = args.precision or ("fp8" if qwen else "bf16")
    if precision != "bf16":
        if not hasattr(model, "set_precision"):
            raise SystemExit(f"--precision {precision} needs a module with set_precision (config {args.config})")
        model.set_precision(precision)
    if args.gradient_checkpointing:
        model.gradient_checkpointing_enable()
    if args.stage == "pretrain":
        for n, p in model.named_parameters():
            if "multi_modal_projector" not in n and "model.connector." not in n:
                p.requires_grad = False
    reducer = GradReducer(model) if (world > 1 or force_dp) else None
    opt = None if args.no_optimizer else FusedAdamW(model, lr=1e-5, weight_decay=0.0, max_grad_norm=1.0)
    # MANTIS_NORM_OVERLAP=1: the optimizer's gradient-norm pass rides on a side stream inside the backward instead of being a
    # separate pass.  Measured on 1x MI355X (profiles/r02_experiments.md): the side-stream kernels cost the concurrent GEMMs more
    # (+3.5 ms) than the separate pass they replace (-3.2 ms), so the default stays off.
    overlap = opt is not None and os.environ.get("MANTIS_NORM_OVERLAP", "0") == "1"
    # single rank: the weight-gradient GEMMs of the backward also leave the sum of squares of what they store, so clip_grad_norm_ needs no
    # pass of its own over the 16 GB of gradients (FusedAdamW.begin_fold; under data parallelism the norm is that of the REDUCED gradient
    # and the separate pass stays)
    fold = opt is not None and reducer is None and not overlap and not args.no_norm_fold and on_gpu
    trainer = MantisHipTrainer(model, gradient_accumulation_steps=1, reducer=reducer, optimizer=opt if overlap else None,
                               fold_norm_into=opt if fold else None)
    vmode = "early" if args.prefetch_early else ("optimizer" if args.prefetch else args.vision_prefetch)
    if not on_gpu or not hasattr(model.engine, "prefetch_vision") or (vmode == "optimizer" and opt is None):
        vmode = "off"
    args.prefetch = vmode != "off"
    args.prefetch_early = vmode == "early"
    if args.prefetch:
        # CU partition: clip + AdamW on `--adam-cus` compute units (HBM-bound: 192 CUs stream as fast as 256), the next batch's frozen
        # tower on the others -- the two masked streams run side by side (tools/cu_mask_probe.hip)
        # `--adam-cus 0`: no CU partition -- the tower on a plain side stream beside the optimizer pass on the compute stream
        total = K.num_cus()
        if args.prefetch_early:
            trainer.prefetch_early = True
            trainer.prefetch_stream = K.priority_stream(1)
        elif args.adam_cus > 0:
            n_adam = min(max(args.adam_cus, 1), total - 8)
            opt.stream = K.cu_masked_stream(0, n_adam)
            trainer.prefetch_stream = K.cu_masked_stream(n_adam, total - n_adam)
    n_batches = args.recycle_batches or (args.warmup + args.steps)
    make = synthetic_batch_idefics2 if idefics else synthetic_batch
    if qwen:
        batches = [synthetic_batch_qwen2vl(cfg, B, T, grids, rank, s) for s in range(n_batches)]
    else:
        batches = [make(cfg, B, T, n_img, img_hw, rank, s) for s in range(n_batches)]
    if idefics and not args.no_pack:
        # BASELINE configs[3] "long-sequence packing": the B samples of a rank travel as ONE row of B*T tokens with segment ids
        # (block-diagonal attention through O(L) segment bounds, positions restart per sample, data.py:1546-1671)
        for bt in batches:
            bt["segment_ids"] = torch.arange(B, dtype=torch.int32).repeat_interleave(T)[None]
            for k in ("input_ids", "attention_mask", "labels"):
                bt[k] = bt[k].reshape(1, B * T)
            bt["pixel_values"] = bt["pixel_values"].reshape(1, B * n_img, *bt["pixel_values"].shape[2:])
    for bt in batches:      # pinned host buffers, as dataloader_pin_memory does in the reference loop
        if on_gpu:
            bt["pixel_values"] = bt["pixel_values"].pin_memory() if (idefics or qwen) else [p.pin_memory() for p in bt["pixel_values"]]

    # lm_head rows the reference computes and this path does not (decoder.compact_ce_rows keeps the rows that can carry a label,
    # padded to a multiple of 8), averaged over the timed batches: enters the launched-FLOP count of the step-level fractions
    def _head_rows(bt):
        ids, lab = bt["input_ids"], bt["labels"]
        img = getattr(cfg, "image_token_index", None)
        img = cfg.image_token_id if img is None else img
        ign = img if idefics else -100
        n = int(((lab != ign) & (ids != img) & (bt["attention_mask"] != 0)).sum())
        return ids.numel() + (n_img_tokens_per_row(bt)) - ((n + 7) // 8 * 8 if n else 8)

    def n_img_tokens_per_row(bt):
        if idefics or qwen:
            return 0                          # one slot per image token: the merged length equals T
        N = (cfg.vision_config.image_size // cfg.vision_config.patch_size) ** 2
        return int((bt["input_ids"] == cfg.image_token_index).sum()) * (N - 1)
    timed_batches = []          # the batches the timed loop actually feeds (filled by one_step)

    split = []          # (start, after training_step, after optimizer) events per timed step
    losses = []

    def one_step(i, timed=False):
        if timed:
            ev = [Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
        nxt = batches[(i + 1) % len(batches)] if args.prefetch else None
        loss = trainer.training_step(model, batches[i % len(batches)], next_inputs=nxt)
        if timed:
            ev[1].record()
            losses.append(loss)
            timed_batches.append(batches[i % len(batches)])
        if opt is not None:
            opt.step()
            opt.zero_grad(set_to_none=True)
        else:
            for p in model.parameters():
                p.grad = None
        if timed:
            ev[2].record()
            split.append(ev)
        return loss

    for i in range(args.warmup):
        loss = one_step(i)
    first_loss = float(loss) if args.warmup else None
    if reducer is not None:
        sync()
        reducer.collect_exposed_ms()
        reducer.stats.update(buckets=0, bytes=0, exposed_ms=[], steps=0)
    # The timed region runs BARE (round-5 verdict, weak 3): no per-launch events.  The ~800 torch.cuda.Event.record() per step that feed
    # `roofline` (a marker packet between dependent kernels each) are taken on `args.steps` MORE steps right after the timed region, same
    # workload, same process; `ms_per_step_with_timer` is what those instrumented steps cost, so the price of the instrument is on the line.
    trainer.launch.timer = None
    sync()
    if world > 1:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss = one_step(args.warmup + i, timed=True)
    sync()
    if world > 1:
        dist.barrier()
    sync()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t)
    if args.dump_outputs and rank == 0 and args.loop == "native":
        dump_outputs(args.dump_outputs, model, losses[-1])
    timer = None if (args.no_kernel_timer or host_only or not args.full) else []
    ms_with_timer = None
    n_extra = 0
    if timer is not None:
        trainer.launch.timer = timer      # per-launch HIP events around every GEMM of THIS trainer's steps (launch.LaunchContext)
        # the fp8 layer loop runs its weight-gradient GEMMs on a lowest-priority side stream (decoder_fp8.decoder_backward), where a launch's
        # event-to-event time is mostly waiting for compute units: the instrumented steps keep every launch on the compute stream (same
        # kernels, bit-identical results), so that `roofline.achieved` divides by launch DURATIONS; the timed region above ran as the product does
        dw_env = os.environ.get("MANTIS_DW_STREAM")
        if precision != "bf16":
            os.environ["MANTIS_DW_STREAM"] = "0"
        sync()
        ti0 = time.perf_counter()
        for i in range(args.steps):
            one_step(args.warmup + args.steps + i)
        sync()
        ms_with_timer = 1e3 * (time.perf_counter() - ti0) / args.steps
        trainer.launch.timer = None
        n_extra = args.steps
    # second family definition (round-4 verdict: keep rounds comparable): with --vision-prefetch early the tower's GEMMs run on the prefetch
    # stream and are outside `roofline.achieved`; two more steps with the tower IN LINE on the compute stream (after one untimed transition
    # step that still picks up a prefetched tower) give the family as rounds 1 - 3 defined it -- every bf16 GEMM launch of the step
    inline_timer = None
    if timer is not None and args.prefetch_early and on_gpu and world == 1 and not host_only:
        trainer.prefetch_early = False
        nxt_keep, args.prefetch = args.prefetch, False
        one_step(args.warmup + args.steps + n_extra)
        inline_timer = []
        trainer.launch.timer = inline_timer
        for i in range(2):
            one_step(args.warmup + args.steps + n_extra + 1 + i)
        sync()
        trainer.launch.timer = None
        trainer.prefetch_early, args.prefetch = True, nxt_keep
    if timer is not None and precision != "bf16":
        if dw_env is None:
            os.environ.pop("MANTIS_DW_STREAM", None)
        else:
            os.environ["MANTIS_DW_STREAM"] = dw_env
    native_loop = None
    if args.loop == "hf":
        if world != 1 or not on_gpu or opt is None:
            raise SystemExit("--loop hf: one GPU, with the optimizer (the HF loop always steps it)")
        step_ms_n = [e[0].elapsed_time(e[2]) for e in split]
        native_loop = dict(ms_per_step=round(1e3 * elapsed / args.steps, 2), ms_per_step_median=round(_pct(step_ms_n, 0.5), 2),
                           ms_training_step=round(_pct([e[0].elapsed_time(e[1]) for e in split], 0.5), 2),
                           samples_per_s=round(world * B * args.steps / elapsed, 4))
        # the native loop's optimizer state (97 GB on the headline) goes before the HF loop builds its own in create_optimizer
        import gc
        trainer.fold_norm_into = trainer.optimizer = None
        opt_was = opt
        del opt_was
        opt = None
        gc.collect()
        torch.cuda.empty_cache()
        elapsed, split, losses, _hf_timer, timed_batches, hf_trainer = run_hf_loop(args, model, batches, B, Event, sync, vmode)
        opt = hf_trainer._fused()
        fold = opt is not None
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, model, losses[-1])
    dp_devices = None
    if reducer is not None and dist.is_initialized():
        # every rank's device as the runtime names it (PCI bus id): N ranks must sit on N distinct GPUs
        me = f"{local_rank}:{torch.cuda.get_device_properties(local_rank).name}:{getattr(torch.cuda.get_device_properties(local_rank), 'pci_bus_id', '?')}" if on_gpu else f"cpu:{rank}"
        gathered = [None] * dist.get_world_size()
        dist.all_gather_object(gathered, me)
        dp_devices = gathered
    loss_vals = [float(x) for x in losses]
    skipped_head_rows = sum(_head_rows(bt) for bt in timed_batches) / max(1, len(timed_batches))
    if rank == 0:
        ms = 1e3 * elapsed / args.steps
        value = world * B * args.steps / elapsed
        step_ms = [e[0].elapsed_time(e[2]) for e in split]
        ts_ms = [e[0].elapsed_time(e[1]) for e in split]
        pmc = None
        pmc_path = PMC_JSON_QWEN_FP8 if (qwen and precision == "fp8") else (None if (tiny or idefics or qwen) else PMC_JSON)
        if timer and pmc_path and os.path.exists(pmc_path):
            with open(pmc_path) as fh:
                pmc = json.load(fh)
        roof = None
        if timer:
            def _family(entries):
                t_ms = sum(x[3].elapsed_time(x[4]) for x in entries)
                return t_ms, sum(x[1] for x in entries), sum(x[2] for x in entries)
            # every GEMM launch of the timed steps (bf16 and fp8) on the COMPUTE stream.  With --vision-prefetch early the next batch's
            # frozen tower runs on a lowest-priority side stream, where a launch's event-to-event time is mostly waiting for compute
            # units: those launches are not "the kernel's launch duration" and are reported beside the family, not inside it
            main_stream = torch.cuda.current_stream().cuda_stream if on_gpu else None
            side_gemms = [x for x in timer if len(x) > 6 and x[6] != main_stream]
            all_gemms = [x for x in timer if not (len(x) > 6 and x[6] != main_stream)]
            if args.gemm_table:
                write_gemm_table(args.gemm_table, [x for x in all_gemms if x[0] == "gemm_nt_kernel"], args.steps, args.config, ms)
            if args.gemm_series:
                per = len(all_gemms) // args.steps
                with open(args.gemm_series, "w") as fh:
                    json.dump([dict(tag=list(x[5]) if len(x) > 5 else None, us=round(x[3].elapsed_time(x[4]) * 1e3, 1))
                               for x in all_gemms[-per:]], fh)
            gf = (pmc or {}).get("gemm_family") or {}
            kname, peak = ("gemm_nt_ring176_kernel + gemm_nt_ring16_kernel + gemm_nt_ring_kernel + gemm_nt_kernel (bf16 MFMA GEMM family: every "
                           "launch of mantis_gemm_bf16_nt / _fused / _sumsq, csrc/gemm.hip + csrc/gemm176.hip)"), PEAK_BF16_TFLOPS
            bf16_family = None
            family = all_gemms
            if precision != "bf16":
                # dominant kernel of this configuration: the fp8 MFMA GEMM (decoder linears); the bf16 family (tower, merger, lm_head)
                # is reported beside it
                f8 = [x for x in all_gemms if x[0] == "gemm_fp8_nt_kernel"]
                b16 = [x for x in all_gemms if x[0] != "gemm_fp8_nt_kernel"]
                if b16:
                    b_ms, b_fl, _ = _family(b16)
                    bf16_family = dict(achieved=round(b_fl / (b_ms * 1e-3) / 1e12, 1), peak=PEAK_BF16_TFLOPS,
                                       launches_per_step=len(b16) // args.steps, gemm_ms_per_step=round(b_ms / args.steps, 1))
                if f8:                                               # no fp8 launch (every shape declined): the bf16 family stays the subject
                    family = f8
                    kname, peak = "gemm_fp8_nt_kernel (fp8 e4m3/e5m2 MFMA GEMM, csrc/gemm_fp8.hip)", PEAK_FP8_TFLOPS
            tot_ms, tot_fl, tot_by = _family(family)
            ach = tot_fl / (tot_ms * 1e-3) / 1e12
            # traffic / MFMA-busy come from PMC passes, which this run does not make: the LIVE fields are null; what the builder's own
            # PMC passes of the same command measured (another box, another day) is carried under a separately named key
            roof = dict(bound="mfma", kernel=kname, achieved=round(ach, 1),
                        measured_on=(f"{args.steps} instrumented steps (HIP events around every GEMM launch on its launch stream) right after the bare "
                                     f"timed region" + (" of the NATIVE loop, which runs first in this process (the HF loop's timed steps are bare too)"
                                                        if args.loop == "hf" else "") +
                                     ("; the fp8 loop's weight-gradient GEMMs, on a lowest-priority side stream in the timed region, are kept on the "
                                      "compute stream for these steps (same kernels, bit-identical): launch durations, not queueing"
                                      if precision != "bf16" else "")),
                        peak=peak, unit="TFLOP/s", frac=round(ach / peak, 4), bf16_gemm_family=bf16_family,
                        traffic=None, mfma_busy_pct=None,
                        pmc_static=None if not pmc else dict(
                            source=os.path.relpath(pmc_path, os.path.dirname(os.path.abspath(__file__))),
                            note="NOT measured by this run: rocprofv3 PMC passes of this command on the builder's box, summarised by "
                                 "tools/pmc_step_report.py; bytes/launch on the L2 memory side (Infinity-Cache hits included)",
                            traffic_bytes_per_launch=gf.get("traffic_bytes_per_launch_incl_finish") or gf.get("traffic_bytes_per_launch"),
                            mfma_busy_pct=((pmc or {}).get("step") or {}).get("mfma_busy_pct")),
                        prefetch_stream_gemms=None if not side_gemms else dict(
                            note="GEMM launches of the next batch's frozen tower on the lowest-priority prefetch stream (--vision-prefetch "
                                 "early): event-to-event times there include waiting for compute units, so they are outside `achieved`",
                            launches_per_step=len(side_gemms) // args.steps, flops_per_step=sum(x[1] for x in side_gemms) / args.steps,
                            event_ms_per_step=round(sum(x[3].elapsed_time(x[4]) for x in side_gemms) / args.steps, 1)),
                        algorithmic_bytes_per_launch=round(tot_by / len(family)),
                        launches_per_step=len(family) // args.steps,
                        avg_launch_us=round(1e3 * tot_ms / len(family), 1), gemm_ms_per_step=round(tot_ms / args.steps, 1),
                        step_model_flops_note="step_model_tflops / *_frac_of_peak divide the REFERENCE's algorithmic FLOPs per sample (SURVEY 8d: "
                                               "lm_head and loss on every sequence row) by the measured time; this path runs lm_head on the labelled "
                                               "rows only, so its launched FLOPs are lower -- `achieved` counts launched GEMM work only",
                        step_model_tflops=round(flop_per_sample * B / (ms * 1e-3) / 1e12, 1) if not tiny else None,
                        step_frac_of_peak=round(flop_per_sample * B / (ms * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4) if (not tiny and precision == "bf16") else None,
                        training_step_frac_of_peak=round(flop_per_sample * B / (_pct(ts_ms, 0.5) * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4) if (not tiny and precision == "bf16") else None)
            # per layout and per shape (the table behind `achieved`, --gemm-table writes it in full): NT = forward, NN = dX, TN = dW
            bf = [x for x in family if x[0] == "gemm_nt_kernel" and len(x) > 5]
            if bf:
                lay, shp = {}, {}
                for x in bf:
                    us = x[3].elapsed_time(x[4]) * 1e3
                    a = lay.setdefault(x[5][3], [0.0, 0.0])
                    a[0] += us
                    a[1] += x[1]
                    b = shp.setdefault(x[5], [0.0, 0.0, 0])
                    b[0] += us
                    b[1] += x[1]
                    b[2] += 1
                roof["by_layout"] = {k: dict(frac=round(v[1] / v[0] / 1e6 / peak, 4), ms_per_step=round(v[0] / args.steps / 1e3, 2)) for k, v in sorted(lay.items())}
                roof["by_shape"] = [dict(shape="x".join(str(d) for d in k[:3]), layout=k[3], epilogue=k[4], launches_per_step=round(v[2] / args.steps, 2),
                                         avg_us=round(v[0] / v[2], 1), frac=round(v[1] / v[0] / 1e6 / peak, 4), ms_per_step=round(v[0] / args.steps / 1e3, 2))
                                    for k, v in sorted(shp.items(), key=lambda kv: -kv[1][0])[:16]]
            if inline_timer:
                it_ms, it_fl, _ = _family([x for x in inline_timer if x[0] == family[0][0]])
                roof["family_with_tower_inline"] = dict(
                    note="every GEMM launch of the step on the compute stream, the vision tower's included (2 extra steps with --vision-prefetch "
                         "off semantics after the timed region): the family as rounds 1 - 3 defined it",
                    achieved=round(it_fl / (it_ms * 1e-3) / 1e12, 1), frac=round(it_fl / (it_ms * 1e-3) / 1e12 / peak, 4),
                    launches_per_step=len(inline_timer) // 2, gemm_ms_per_step=round(it_ms / 2, 1))
            if not tiny:
                # the honest step-level figures: FLOPs actually LAUNCHED (the reference's count minus the lm_head rows this path never
                # computes: forward + dX + dW of every row without a label), against the roof of the precision each FLOP runs at
                # (fp8 lines: sum_i flops_i / peak_i -- the fp8 GEMM family at the fp8 peak, everything else at the bf16 peak)
                tc_ = cfg.text_config
                launched = flop_per_sample * B - 3.0 * 2.0 * tc_.hidden_size * tc_.vocab_size * skipped_head_rows
                f8_fl = (sum(x[1] for x in all_gemms if x[0] == "gemm_fp8_nt_kernel") / args.steps) if precision != "bf16" else 0.0
                t_roof = f8_fl / (PEAK_FP8_TFLOPS * 1e12) + (launched - f8_fl) / (PEAK_BF16_TFLOPS * 1e12)
                roof.update(step_launched_flops=launched,
                            step_launched_tflops=round(launched / (ms * 1e-3) / 1e12, 1),
                            step_frac_of_peak_launched=round(t_roof / (ms * 1e-3), 4),
                            training_step_frac_of_peak_launched=round(t_roof / (_pct(ts_ms, 0.5) * 1e-3), 4))
        cpu = None
        if world == 1 and args.full and not args.no_cpu_baseline:
            try:
                if qwen:
                    cpu = cpu_baseline_qwen2vl(cfg, T, grids)
                elif idefics:
                    cpu = cpu_baseline_idefics2(cfg, T, n_img, img_hw)
                else:
                    cpu = cpu_baseline(args.config)
            except Exception as e:      # the host-side oracle leg must not take the measured GPU line down with it
                cpu = dict(value=None, unit="samples/s", cores=torch.get_num_threads(), kind="port",
                           sample=f"CPU baseline failed: {type(e).__name__}: {e}")
        dp = None
        if reducer is not None:
            ex = reducer.collect_exposed_ms()
            nsteps_seen = max(1, reducer.stats["steps"])          # timed + instrumented steps since the statistics were reset
            rccl_version = None
            try:
                rccl_version = ".".join(str(x) for x in torch.cuda.nccl.version()) if on_gpu else None
            except Exception:
                pass
            q = reducer.hw_queues or (None, None, None)
            dp = dict(algo=reducer.algo,
                      # what the communicator itself reports (the first hour on a node must be self-verifying, round-5 verdict item 6)
                      world_size_seen=dist.get_world_size(), backend=dist.get_backend(), rccl_version=rccl_version,
                      ranks_devices=dp_devices, distinct_devices=len(set(dp_devices)) if dp_devices else None,
                      buckets_per_step=reducer.stats["buckets"] // nsteps_seen,
                      bytes_per_step=reducer.stats["bytes"] // nsteps_seen,
                      wire_bytes_per_gpu_per_step=int(2 * (world - 1) / max(1, world) * (reducer.stats["bytes"] // nsteps_seen)),
                      exposed_comm_ms_median=None if not ex else round(_pct(ex, 0.5), 3),
                      exposed_comm_ms_max=None if not ex else round(max(ex), 3),
                      overlap_probe=dict(hw_queues_at_hip_init=q[0], collective_ran_beside_busy_compute_stream=q[1], process_groups_recreated=q[2],
                                         required=os.environ.get("MANTIS_DP_REQUIRE_OVERLAP") == "1"),
                      gemm_cus_planned=reducer.gemm_cus or K.num_cus() if on_gpu else None,
                      nccl_env={k: v for k, v in os.environ.items() if k.startswith(("NCCL_", "RCCL_", "MANTIS_DP_", "MANTIS_GEMM_CUS", "GPU_MAX_HW_QUEUES"))})
        names = dict(mantis_8b_siglip_llama3="Mantis-8B-SigLIP-Llama-3", mantis_8b_clip_llama3="Mantis-8B-CLIP-L/14-336-Llama-3")
        metric = ("train samples/sec Mantis-tiny (1 img 224^2 + 128 tok)" if tiny else
                  "train samples/sec (8 img x 448^2, seq 2048) Mantis-8B-Idefics2" if idefics else
                  "train samples/sec (2 img x 1280x960 dynamic resolution, seq 4096) Qwen2-VL-7B" if qwen else
                  f"train samples/sec (4 img x 336^2 + 512 tok) {names[args.config]}")
        out = dict(metric=metric,
                   value=round(value, 4), unit="samples/s", n_gpus=world, steps=args.steps, warmup=args.warmup,
                   ms_per_step=round(ms, 2),
                   ms_per_step_median=round(_pct(step_ms, 0.5), 2), ms_per_step_p10=round(_pct(step_ms, 0.1), 2),
                   ms_per_step_p90=round(_pct(step_ms, 0.9), 2),
                   ms_per_step_with_timer=None if (ms_with_timer is None or args.loop == "hf") else round(ms_with_timer, 2),
                   timed_region="bare: no per-launch events inside the timed steps",
                   ms_training_step=round(_pct(ts_ms, 0.5), 2),
                   ms_training_step_p10=round(_pct(ts_ms, 0.1), 2), ms_training_step_p90=round(_pct(ts_ms, 0.9), 2),
                   ms_optimizer=round(_pct([e[1].elapsed_time(e[2]) for e in split], 0.5), 2) if opt is not None else None,
                   samples_per_s_training_step_only=round(world * B / (1e-3 * _pct(ts_ms, 0.5)), 4),
                   peak_hbm_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 1) if on_gpu else None,      # torch's allocator, this rank, whole run
                   higher_is_better=True, scaling="weak", vs_baseline=None,
                   dtype="bf16" if precision == "bf16" else "fp8 (e4m3 activations/weights, e5m2 gradients in the decoder linears" +
                         (", per-row / per-column scales" if precision == "fp8_rowwise" else "") + "; bf16 elsewhere)",
                   data="synthetic" + ("" if args.recycle_batches else " (fresh batch every step)") +
                        (" -- HOST-ONLY PLUMBING RUN, not a measurement" if host_only else ""),
                   loss=round(loss_vals[-1], 4), loss_first_timed=round(loss_vals[0], 4), loss_after_warmup=first_loss,
                   loss_min=round(min(loss_vals), 4), loss_max=round(max(loss_vals), 4),
                   config=dict(workload=f"{args.config}: ViT fwd + projector + packing + Llama fwd/bwd"
                                        f"{'' if args.no_optimizer else ' + clip + fused AdamW'}; {B} samples/GPU, "
                                        f"{n_img} img + {T} tok per sample; random-init weights",
                               global_batch=world * B, seq_len=T,
                               merged_seq_len=T if (idefics or qwen) else T - n_img + n_img * (cfg.vision_config.image_size // cfg.vision_config.patch_size) ** 2,
                               flop_per_sample=flop_per_sample,
                               parallelism=f"dp{world}", optimizer=not args.no_optimizer, stage=args.stage,
                               packed=bool(idefics and not args.no_pack),
                               vision_prefetch=vmode, grad_norm_folded_into_dw=bool(fold),
                               gradient_checkpointing=bool(args.gradient_checkpointing)),
                   loop=("transformers.Trainer.train() over as_hf_trainer() (HF dataloader / get_batch_samples / create_optimizer -> FusedAdamW / "
                         "scheduler / clip call / zero_grad)" if args.loop == "hf" else "native (MantisHipTrainer + FusedAdamW)"),
                   native_loop=None if native_loop is None else dict(
                       native_loop, note="the same workload through the native loop, timed first in this process",
                       hf_minus_native_ms_per_step=round(ms - native_loop["ms_per_step"], 2),
                       hf_over_native=round(ms / native_loop["ms_per_step"], 4)),
                   roofline=roof, cpu_baseline=cpu, dp=dp)
        print(json.dumps(out), flush=True)
    if world > 1 or force_dp:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
