#!/usr/bin/env python3
"""Golden fixtures of greedy generation on the LLaVA path, recorded by RUNNING the reference class (see make_golden.py for where it
lives and the rules: this script runs only where the reference is installed; the suite reads nothing but the ``generation/llava_generate_*.npz``
files it writes -- a directory of their own, because tests/test_oracle_vs_golden.py takes every ``*.npz`` directly under tests/golden/ for
a training-step fixture).  The model is the seeded tiny SigLIP model of make_golden.py (its weights are tests/golden/weights_siglip.npz),
``model.eval()``.

WHICH OF THE TWO PRODUCED THE FIXTURE: on the installed transformers (5.x) the reference class has no ``generate`` (it no longer
inherits GenerationMixin and its ``prepare_inputs_for_generation`` speaks the 4.x cache API), so the fixture records what greedy
``generate`` computes BY DEFINITION: a loop over the reference's own ``forward`` on the growing ``input_ids`` / ``attention_mask``
(one column of ones appended per step, as HF's ``_update_model_kwargs_for_generation`` does), ``argmax`` of the last row, no cache.

Per case: the inputs, ``tokens [B, n]`` (free-running, no EOS), the fp32 last-row logits of every step ``logits [n, B, V]``, the same loop
with the model in bf16 fed the fp32 tokens (``logits_bf16``), ``delta = max |logits_bf16 - logits|``, the fp32 top-2 ``margins [n, B]``,
``eos_token_id`` (-1: none) and ``sequences``: what HF's greedy search returns (prompt + new tokens, a finished row filled with
``pad_token_id``, stopping once every row has emitted the EOS).

Token equality is a fair demand only where the argmax survives the arithmetic's error: with eps = 1.5 x delta (the project's envelope
factor, tests/helpers.py ENVELOPE_FACTOR), logits within eps of the fp32 record keep the argmax wherever the fp32 top-2 margin exceeds
2 x eps.  The prompt seeds are therefore SEARCHED until every step of every row has margin > 2 x eps (and no generated token is the
image placeholder or the pad id); the script asserts it and tests/test_generation.py asserts it again on the committed files.

Usage:  python tests/golden/make_golden_generation.py
"""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG      # noqa: E402

N_STEPS = 12
MAX_SEEDS = 4000
FACTOR = 1.5


def _prompt(rng, T, img_positions, n_left_pad):
    ids = rng.integers(0, MG.IMG - 1, size=T, dtype=np.int64)
    for p in img_positions:
        ids[p] = MG.IMG
    mask = np.ones(T, dtype=np.int64)
    if n_left_pad:
        ids[:n_left_pad] = MG.PAD
        mask[:n_left_pad] = 0
    return ids, mask


@torch.no_grad()
def _loop(model, ids, mask, pixels, n, forced=None, floor=None):
    """greedy search by definition; forced [B, n]: feed these tokens instead of the argmax.  Returns tokens [B, n], logits [n, B, V] (fp32),
    margins [n, B], or None as soon as a margin falls under `floor` or a generated token is the image placeholder / pad id."""
    ids, mask = torch.from_numpy(ids), torch.from_numpy(mask)
    pv = None if pixels is None else [torch.from_numpy(p).to(next(model.parameters()).dtype) for p in pixels]
    toks, logits, margins = [], [], []
    for i in range(n):
        out = model(input_ids=ids, pixel_values=pv, attention_mask=mask)
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


def main():
    model, cfg = MG.build("siglip", 11)
    model.eval()
    import copy
    model16 = copy.deepcopy(model).to(torch.bfloat16).eval()
    cases = {      # name: (rows of (T, image positions, left pads), with eos)
        "b1_img2": ([(20, [3, 9], 0)], False),
        "b1_img4_first": ([(20, [0, 5, 9, 14], 0)], False),
        "b1_text_only": ([(16, [], 0)], False),
        "b2_leftpad": ([(20, [2, 8], 0), (20, [7, 12], 5)], False),
        "b2_eos": ([(18, [1, 10], 0), (18, [6, 11], 4)], True),
    }
    for ci, (name, (rows, with_eos)) in enumerate(cases.items()):
        n = N_STEPS
        t0 = time.time()
        floor = 0.0
        found = None
        for seed in range(MAX_SEEDS):
            rng = np.random.default_rng(100000 * (ci + 1) + seed)
            pr = [_prompt(rng, T, pos, lp) for T, pos, lp in rows]
            ids, mask = np.stack([p[0] for p in pr]), np.stack([p[1] for p in pr])
            pixels = [rng.standard_normal((len(pos), 3, 56, 56)).astype(np.float32) for _, pos, _ in rows]
            if not any(len(pos) for _, pos, _ in rows):
                pixels = None
            r = _loop(model, ids, mask, pixels, n, floor=floor)
            if r is None:
                continue
            tokens, logits, margins = r
            _, logits16, _ = _loop(model16, ids, mask, pixels, n, forced=tokens)
            delta = float(np.abs(logits16 - logits).max())
            floor = max(floor, 2 * FACTOR * delta * 0.5)      # later seeds: give up early under half of a typical bound
            if margins.min() > 2 * FACTOR * delta:
                found = (seed, ids, mask, pixels, tokens, logits, logits16, delta, margins)
                break
        assert found is not None, f"{name}: no prompt seed in {MAX_SEEDS} keeps every margin above 2 x eps"
        seed, ids, mask, pixels, tokens, logits, logits16, delta, margins = found
        assert margins.min() > 2 * FACTOR * delta
        eos = None
        if with_eos:
            # a token one row emits mid-way (steps 3 .. n - 4) that the other row has not emitted by then: the rows stop at different steps
            for s in range(3, n - 3):
                for b in range(tokens.shape[0]):
                    tok = int(tokens[b, s])
                    other = 1 - b
                    if tok not in tokens[b, :s] and tok not in tokens[other, : s + 1]:
                        eos = tok
                        break
                if eos is not None:
                    break
            assert eos is not None
        out = dict(input_ids=ids, attention_mask=mask, tokens=tokens, logits=logits, logits_bf16=logits16, delta=np.float64(delta),
                   margins=margins, eos_token_id=np.int64(-1 if eos is None else eos), pad_token_id=np.int64(MG.PAD),
                   sequences=_sequences(ids, tokens, eos), prompt_seed=np.int64(seed), n_steps=np.int64(n))
        if pixels is not None:
            out["pixel_values"] = np.concatenate(pixels, 0)
            out["pixel_counts"] = np.array([p.shape[0] for p in pixels], dtype=np.int64)
        os.makedirs(os.path.join(HERE, "generation"), exist_ok=True)
        np.savez_compressed(os.path.join(HERE, "generation", f"llava_generate_{name}.npz"), **out)
        print(f"{name}: seed {seed} n {n} delta {delta:.4f} min margin {margins.min():.4f} (bound {2 * FACTOR * delta:.4f}) eos {eos} "
              f"sequences {out['sequences'].shape} [{time.time() - t0:.0f} s]", flush=True)


if __name__ == "__main__":
    main()
