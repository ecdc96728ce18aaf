#!/usr/bin/env python3
"""Golden fixtures for the sequence-classification / regression head of the Idefics2 path, recorded by RUNNING the reference fork's
Idefics2ForSequenceClassification (/root/reference/mantis/models/idefics2/modeling_idefics2.py:2017-2222) in the build container.

Backbone weights are those of tests/golden/weights_idefics2.npz (the generation model of make_golden_idefics2.py, `model.*` copied
into the classification model and checked); only `score.weight` / `score.bias` are stored here.  Vision tower frozen.  B = 2 with
images in both rows.  Cases: regression C = 5, regression C = 1, single-label C = 5, multi-label C = 5 on one full row + one
right-padded row, and regression C = 5 with a LEFT-padded row (the pooling rule looks at input_ids: a row that starts with the pad id
pools position T - 1).  Recorded per case: inputs, labels, pooled positions, pooled logits, loss and every trainable gradient (rounded to
14 mantissa bits; pixels stored as fp16, exactly).
Runs only here; tests read the .npz files.   Usage: python tests/golden/make_golden_idefics2_seqcls.py
"""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_idefics2 as G      # noqa: E402

T = 28


def round_mantissa(a, bits=14):
    """fp32 rounded to `bits` mantissa bits (relative error <= 2^-15 per element): keeps each fixture under the 1 MiB file limit."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    drop = 23 - bits
    return (((u + np.uint32(1 << (drop - 1))) >> np.uint32(drop)) << np.uint32(drop)).view(np.float32)


def build_cls(gen, num_labels, problem_type, seed):
    sys.path.insert(0, G.REF)
    from mantis.models.idefics2.modeling_idefics2 import Idefics2ForSequenceClassification
    from transformers import Idefics2Config

    class Oracle(Idefics2ForSequenceClassification):
        def tie_weights(self, *a, **k):
            return None

    m = G.meta()
    cfg = Idefics2Config(vision_config=m["vision"], perceiver_config=m["perceiver"], text_config=m["text"], image_token_id=G.IMG,
                         tie_word_embeddings=False, num_labels=num_labels, problem_type=problem_type, pad_token_id=G.PAD)
    cfg._attn_implementation = "eager"
    torch.manual_seed(seed)
    model = Oracle(cfg)
    model.model.load_state_dict(gen.model.state_dict(), strict=True)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        model.score.weight.copy_(0.2 * torch.randn(model.score.weight.shape, generator=g))
        model.score.bias.copy_(0.1 * torch.randn(model.score.bias.shape, generator=g))
    for p in model.model.vision_model.parameters():
        p.requires_grad_(False)
    model.train()
    return model


def main():
    gen = G.build(31)
    ref = np.load(os.path.join(HERE, "weights_idefics2.npz"))
    for k, v in gen.state_dict().items():
        assert np.array_equal(v.detach().numpy(), ref[k]), k
    rng = np.random.default_rng(515)
    NL, IMG, PAD = G.NL, G.IMG, G.PAD

    def text(img_starts, n_pad=0, left=False):
        ids = rng.integers(1, 290, size=T, dtype=np.int64)
        mask = np.ones(T, np.int64)
        if n_pad and left:
            ids[:n_pad] = PAD
            mask[:n_pad] = 0
        elif n_pad:
            ids[T - n_pad:] = PAD
            mask[T - n_pad:] = 0
        for s in img_starts:
            ids[s: s + NL] = IMG
        return ids, mask

    pv = np.zeros((2, 2, 3, 56, 56), np.float32)
    pv[0] = rng.standard_normal((2, 3, 56, 56)).astype(np.float32)
    pv[1, 0] = rng.standard_normal((3, 56, 56)).astype(np.float32)
    pv = pv.astype(np.float16).astype(np.float32)      # stored as fp16, exactly
    a = text([1, 16])
    b = text([6], n_pad=5)
    c = text([9], n_pad=4, left=True)
    right = (np.stack([a[0], b[0]]), np.stack([a[1], b[1]]))
    left = (np.stack([a[0], c[0]]), np.stack([a[1], c[1]]))
    cases = [("idefics2_seqcls_regression_c5", 5, "regression", right, rng.uniform(1, 5, (2, 5)).astype(np.float32)),
             ("idefics2_seqcls_regression_c1", 1, "regression", right, rng.uniform(1, 5, (2, 1)).astype(np.float32)),
             ("idefics2_seqcls_single_label_c5", 5, "single_label_classification", right, np.array([3, 0], np.int64)),
             ("idefics2_seqcls_multi_label_c5", 5, "multi_label_classification", right,
              (rng.uniform(0, 1, (2, 5)) > 0.5).astype(np.float32)),
             ("idefics2_seqcls_regression_c5_leftpad", 5, "regression", left, rng.uniform(1, 5, (2, 5)).astype(np.float32))]
    for i, (name, C, problem, (ids, mask), labels) in enumerate(cases):
        model = build_cls(gen, C, problem, 100 + i)
        for k, v in gen.model.state_dict().items():
            assert torch.equal(v, model.model.state_dict()[k]), k
        model.zero_grad(set_to_none=True)
        res = model(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask), labels=torch.from_numpy(labels),
                    pixel_values=torch.from_numpy(pv), use_cache=False)
        res.loss.backward()
        pos = (torch.eq(torch.from_numpy(ids), PAD).int().argmax(-1) - 1) % T
        out = dict(input_ids=ids, attention_mask=mask, labels=labels, pixel_values=pv.astype(np.float16), num_labels=np.array(C),
                   problem_type=np.array(problem), pad_token_id=np.array(PAD), pooled_positions=pos.numpy(),
                   logits=res.logits.detach().numpy(), loss=res.loss.detach().numpy())
        out["weight.score.weight"] = model.score.weight.detach().numpy()
        out["weight.score.bias"] = model.score.bias.detach().numpy()
        for n, p in model.named_parameters():
            if p.grad is not None:
                out["grad." + n] = round_mantissa(p.grad.detach().numpy())
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        print(f"{name}: loss={float(res.loss):.6f} pooled at {pos.tolist()} logits{tuple(res.logits.shape)} "
              f"grads={sum(1 for k in out if k.startswith('grad.'))} {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
