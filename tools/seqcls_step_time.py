#!/usr/bin/env python3
"""Full-size Mantis-8B-Idefics2 training step, classification head (regression, num_labels = 5) beside the generation head, on the same
batch (bench.py's Idefics2 geometry: 2 samples x (8 images 448^2 + 2048 tokens)) in one process, alternating, timed with a host clock
around a device synchronise.  No optimizer pass: the two steps differ only in the head.   Usage: python tools/seqcls_step_time.py [reps]
Prints one JSON line (profiles/seqcls_head.md)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import bench
    from mantis_amd import configuration_idefics2 as C
    from mantis_amd.modeling_idefics2 import Idefics2ForConditionalGeneration, Idefics2ForSequenceClassification
    from mantis_amd.trainer import MantisHipTrainer
    assert torch.cuda.is_available(), "needs the GPU: a step time is not measured on the host"
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    B, T, n_img, hw = 2, 2048, 8, 448
    gen = Idefics2ForConditionalGeneration(C.mantis_8b_idefics2(), device="cuda", seed=0)
    cfg = C.mantis_8b_idefics2(num_labels=5, problem_type="regression", pad_token_id=0)
    cls = Idefics2ForSequenceClassification(cfg, device="cuda", seed=0)
    batch = bench.synthetic_batch_idefics2(cfg, B, T, n_img, hw, 0)
    cbatch = dict(batch, labels=torch.rand(B, 5) * 4 + 1)
    runs = {"generation": (gen, MantisHipTrainer(gen, 1), batch), "classification": (cls, MantisHipTrainer(cls, 1), cbatch)}
    times = {k: [] for k in runs}
    for it in range(3 + reps):
        for name, (model, tr, b) in runs.items():
            for p in model.parameters():
                p.grad = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = tr.training_step(model, b)
            torch.cuda.synchronize()
            if it >= 3:
                times[name].append((time.perf_counter() - t0) * 1e3)
            assert torch.isfinite(loss)
    out = dict(device=torch.cuda.get_device_name(0), B=B, T=T, images=n_img, image_px=hw, reps=reps)
    try:
        out["clock_mhz"] = torch.cuda.clock_rate()
    except Exception as e:           # not every build exposes it
        out["clock_mhz"] = None
    for name, ts in times.items():
        ts = sorted(ts)
        out[name + "_ms_median"] = round(ts[len(ts) // 2], 2)
        out[name + "_ms_min_max"] = [round(ts[0], 2), round(ts[-1], 2)]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
