#!/usr/bin/env python3
"""Golden fixtures of greedy generation on the Idefics3 path, recorded by RUNNING the reference class (see make_golden_idefics3.py for
where it lives and the shims it needs: this script runs only where the reference is installed; the suite reads nothing but the
``generation/idefics3_generate_*.npz`` files it writes).  The model is the seeded tiny model of make_golden_idefics3.py (``build(37)``:
its weights are tests/golden/idefics3/weights.npz), ``model.eval()``.

WHICH OF THE TWO PRODUCED THE FIXTURE: under the installed transformers the reference class has no ``generate``, so the fixture records
what greedy ``generate`` computes BY DEFINITION: a loop over the reference's own ``forward`` on the growing ``input_ids`` /
``attention_mask`` (one column of ones appended per step), with ``position_ids = attention_mask.cumsum(-1) - 1`` (masked positions at 1)
passed explicitly, as its ``prepare_inputs_for_generation`` (modeling_idefics3.py:1243-1249) does, ``argmax`` of the last row, no cache.

Per case, the fields of the LLaVA fixtures (make_golden_generation.py) plus ``pixel_attention_mask``: the inputs, ``tokens [B, n]``
(free-running, no EOS), the fp32 last-row logits of every step ``logits [n, B, V]``, the same loop with the model in bf16 fed the fp32
tokens (``logits_bf16``), ``delta = max |logits_bf16 - logits|``, the fp32 top-2 ``margins [n, B]``, ``eos_token_id`` (-1: none) and
``sequences``: what HF's greedy search returns.  ``pixel_values`` is [B, images, 3, H, W] as the collator pads it: an unused image slot is
all zeros (the model drops it) and fully masked.

Token equality is a fair demand only where the argmax survives the arithmetic's error: the prompt seeds are SEARCHED until every step of
every row has fp32 top-2 margin > 2 x eps, eps = 1.5 x delta, and no generated token is the image placeholder or the pad id; asserted
here and again by tests/test_generation_idefics3.py on the committed files.

Usage:  python tests/golden/make_golden_idefics3_generation.py
"""
import copy
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_idefics3 as MG      # noqa: E402

N_STEPS = 12
MAX_SEEDS = 4000
FACTOR = 1.5
N_TOK = 4          # <image> tokens per 56 x 56 image at scale_factor 2


def _prompt(rng, T, img_starts, n_left_pad):
    ids = rng.integers(1, 290, size=T, dtype=np.int64)
    for s in img_starts:
        ids[s: s + N_TOK] = MG.IMG
    mask = np.ones(T, dtype=np.int64)
    if n_left_pad:
        ids[:n_left_pad] = MG.PAD
        mask[:n_left_pad] = 0
    return ids, mask


def positions(mask):
    pos = mask.long().cumsum(-1) - 1
    return pos.masked_fill(mask == 0, 1)


@torch.no_grad()
def _loop(model, ids, mask, pixels, pixel_mask, n, forced=None, floor=None):
    """greedy search by definition; forced [B, n]: feed these tokens instead of the argmax.  Returns tokens [B, n], logits [n, B, V] (fp32),
    margins [n, B], or None as soon as a margin falls under `floor` or a generated token is the image placeholder / pad id."""
    ids, mask = torch.from_numpy(ids), torch.from_numpy(mask)
    pv = None if pixels is None else torch.from_numpy(pixels).to(next(model.parameters()).dtype)
    pm = None if pixel_mask is None else torch.from_numpy(pixel_mask)
    toks, logits, margins = [], [], []
    for i in range(n):
        out = model(input_ids=ids, attention_mask=mask, position_ids=positions(mask), pixel_values=pv, pixel_attention_mask=pm,
                    use_cache=False)
        last = out.logits[:, -1, :].float()
        top = last.topk(2, dim=-1).values
        margin = top[:, 0] - top[:, 1]
        nxt = last.argmax(-1) if forced is None else torch.from_numpy(forced[:, i])
        if forced is None and (bool((margin < floor).any()) or bool(((nxt == MG.IMG) | (nxt == MG.PAD)).any())):
            return None
        toks.append(nxt), logits.append(last), margins.append(margin)
        ids = torch.cat([ids, nxt[:, None]], 1)
        mask = torch.cat([mask, torch.ones_like(mask[:, :1])], 1)
    return torch.stack(toks, 1).numpy(), torch.stack(logits, 0).numpy(), torch.stack(margins, 0).numpy()


def _sequences(ids, tokens, eos):
    """HF greedy search's return value for the free-running `tokens` under `eos` (None: run to the length limit)."""
    B, n = tokens.shape
    unfinished = np.ones(B, bool)
    cols = []
    for i in range(n):
        t = np.where(unfinished, tokens[:, i], MG.PAD)
        cols.append(t)
        if eos is not None:
            unfinished &= t != eos
            if not unfinished.any():
                break
    return np.concatenate([ids, np.stack(cols, 1)], 1)


def _pixels(rng, counts):
    """[B, max images, 3, 56, 56] fp16-exact pixels and the bool pixel mask; an unused slot is all zeros and fully masked"""
    M = max(counts)
    if M == 0:
        return None, None
    pv = np.zeros((len(counts), M, 3, 56, 56), np.float32)
    pm = np.zeros((len(counts), M, 56, 56), bool)
    for b, c in enumerate(counts):
        pv[b, :c] = rng.standard_normal((c, 3, 56, 56)).astype(np.float16).astype(np.float32)
        pm[b, :c] = True
    return pv, pm


def main():
    model = MG.build(37)
    model.eval()
    model16 = copy.deepcopy(model).to(torch.bfloat16).eval()
    cases = {      # name: (rows of (T, starts of the <image> runs, left pads), with eos)
        "b1_img2": ([(24, [3, 13], 0)], False),
        "b1_text_only": ([(16, [], 0)], False),
        "b2_leftpad": ([(24, [2, 12], 0), (24, [10], 5)], False),
        "b2_text_leftpad": ([(16, [], 0), (16, [], 6)], False),
        "b2_eos": ([(22, [1, 11], 0), (22, [9], 4)], True),
    }
    for ci, (name, (rows, with_eos)) in enumerate(cases.items()):
        n = N_STEPS
        t0 = time.time()
        floor = 0.0
        found = None
        for seed in range(MAX_SEEDS):
            rng = np.random.default_rng(300000 * (ci + 1) + seed)
            pr = [_prompt(rng, T, pos, lp) for T, pos, lp in rows]
            ids, mask = np.stack([p[0] for p in pr]), np.stack([p[1] for p in pr])
            pixels, pixel_mask = _pixels(rng, [len(pos) for _, pos, _ in rows])
            r = _loop(model, ids, mask, pixels, pixel_mask, n, floor=floor)
            if r is None:
                continue
            tokens, logits, margins = r
            _, logits16, _ = _loop(model16, ids, mask, pixels, pixel_mask, n, forced=tokens)
            delta = float(np.abs(logits16 - logits).max())
            floor = max(floor, 2 * FACTOR * delta * 0.5)      # later seeds: give up early under half of a typical bound
            if margins.min() <= 2 * FACTOR * delta:
                continue
            eos = None
            if with_eos:
                # a token BOTH rows emit, first at different steps, neither in the first two steps nor in the last two: the rows stop
                # at different steps, both before step n (the LLaVA script's rule, plus the demand that the other row emits it too)
                first = lambda b, t: int(np.argmax(tokens[b] == t))
                cand = [(max(first(0, t), first(1, t)), int(t)) for t in np.intersect1d(tokens[0], tokens[1])
                        if first(0, t) != first(1, t) and min(first(0, t), first(1, t)) >= 2 and max(first(0, t), first(1, t)) <= n - 3]
                if cand:
                    eos = min(cand)[1]
                if eos is None:
                    continue
            found = (seed, ids, mask, pixels, pixel_mask, tokens, logits, logits16, delta, margins, eos)
            break
        assert found is not None, f"{name}: no prompt seed in {MAX_SEEDS} keeps every margin above 2 x eps"
        seed, ids, mask, pixels, pixel_mask, tokens, logits, logits16, delta, margins, eos = found
        assert margins.min() > 2 * FACTOR * delta
        seq = _sequences(ids, tokens, eos)
        if with_eos:
            assert seq.shape[1] < ids.shape[1] + n, "both rows must stop before the length limit"
        out = dict(input_ids=ids, attention_mask=mask, tokens=tokens, logits=logits, logits_bf16=logits16, delta=np.float64(delta),
                   margins=margins, eos_token_id=np.int64(-1 if eos is None else eos), pad_token_id=np.int64(MG.PAD),
                   sequences=seq, prompt_seed=np.int64(seed), n_steps=np.int64(n))
        if pixels is not None:
            out["pixel_values"] = pixels
            out["pixel_attention_mask"] = pixel_mask
            out["pixel_counts"] = np.array([len(pos) for _, pos, _ in rows], dtype=np.int64)
        os.makedirs(os.path.join(HERE, "generation"), exist_ok=True)
        path = os.path.join(HERE, "generation", f"idefics3_generate_{name}.npz")
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) < (1 << 20), (name, os.path.getsize(path))
        print(f"{name}: seed {seed} n {n} delta {delta:.4f} min margin {margins.min():.4f} (bound {2 * FACTOR * delta:.4f}) eos {eos} "
              f"sequences {seq.shape} {os.path.getsize(path)} B [{time.time() - t0:.0f} s]", flush=True)


if __name__ == "__main__":
    main()
