#!/usr/bin/env python3
"""Golden fixture for Mistral's sliding-window attention on the Idefics2 path, recorded by RUNNING the reference fork
/root/reference/mantis/models/idefics2/modeling_idefics2.py (Idefics2ForConditionalGeneration) over the HF Mistral text model, whose
mask is HF:models/mistral/modeling_mistral.py create_sliding_window_causal_mask (masking_utils: kv_idx > q_idx - sliding_window).

The weights are those of tests/golden/weights_idefics2.npz (same seed and parameter order as make_golden_idefics2.py; checked below);
only the text config's sliding_window differs: W = 24 over rows of T = 100 tokens.  The batch: B = 2, right padding, sample 0 with its
two images before the window's edge of most queries, sample 1 with one image and padded by more than W (its last queries see only
padding).  Recorded: inputs, loss and the gradient of every trainable parameter (rounded to 14 mantissa bits); and `loss_nowindow`, the loss of the same batch with
sliding_window=None, which proves the fixture is sensitive to the window.   Usage: python tests/golden/make_golden_idefics2_window.py
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

W, T = 24, 100


def round_mantissa(a, bits=14):
    """fp32 rounded to `bits` mantissa bits (relative error <= 2^-15): keeps the compressed fixture under the 1 MiB file limit."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    drop = 23 - bits
    return (((u + np.uint32(1 << (drop - 1))) >> np.uint32(drop)) << np.uint32(drop)).view(np.float32)


def build(window):
    meta = G.meta()
    meta["text"]["sliding_window"] = window
    orig = G.meta
    G.meta = lambda: meta
    try:
        return G.build(31)
    finally:
        G.meta = orig


def main():
    model = build(W)
    ref = np.load(os.path.join(HERE, "weights_idefics2.npz"))
    for k, v in model.state_dict().items():
        assert np.array_equal(v.detach().numpy(), ref[k]), k          # same weights as the window-less fixtures
    rng = np.random.default_rng(2024)
    NL, IMG, PAD = G.NL, G.IMG, G.PAD

    def text(img_starts, n_pad=0):
        ids = rng.integers(1, 290, size=T, dtype=np.int64)
        for s in img_starts:
            ids[s: s + NL] = IMG
        mask = np.ones(T, np.int64)
        if n_pad:
            ids[T - n_pad:] = PAD
            mask[T - n_pad:] = 0
        lab = ids.copy()
        lab[:5] = IMG
        lab[mask == 0] = IMG
        return ids, mask, lab

    a = text([3, 11])
    b = text([7], n_pad=40)
    ids, mask, lab = np.stack([a[0], b[0]]), np.stack([a[1], b[1]]), np.stack([a[2], b[2]])
    pv = np.zeros((2, 2, 3, 56, 56), np.float32)
    pv[0] = rng.standard_normal((2, 3, 56, 56)).astype(np.float32)
    pv[1, 0] = rng.standard_normal((3, 56, 56)).astype(np.float32)
    pv = pv.astype(np.float16).astype(np.float32)      # stored as fp16, exactly

    def run(m):
        m.zero_grad(set_to_none=True)
        res = m(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask), labels=torch.from_numpy(lab),
                pixel_values=torch.from_numpy(pv), use_cache=False)
        res.loss.backward()
        return res.loss

    loss = run(model)
    out = dict(input_ids=ids, attention_mask=mask, labels=lab, pixel_values=pv.astype(np.float16), sliding_window=np.array(W),
               loss=loss.detach().numpy())
    for n, p in model.named_parameters():
        if p.grad is not None:
            out["grad." + n] = round_mantissa(p.grad.detach().numpy())
    out["loss_nowindow"] = run(build(None)).detach().numpy()
    name = "idefics2_window_b2_rightpad"
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print(f"{name}: loss={float(out['loss']):.6f} (no window: {float(out['loss_nowindow']):.6f}) "
          f"grads={sum(1 for k in out if k.startswith('grad.'))}")


if __name__ == "__main__":
    main()
