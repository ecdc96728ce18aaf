"""Test infrastructure of Idefics3 generation: a torch-CPU restatement of `hip_ops.greedy_select` (row by row, straight from the
specification in include/mantis_hip.h), the CPU backend for `mantis_amd.modeling_idefics2.K` (tests/generation_ref.backend() + the
Idefics3 pixel shuffle + that restatement), and the helpers both test files share for the fixtures
tests/golden/generation/idefics3_generate_*.npz (recorded by tests/golden/make_golden_idefics3_generation.py)."""
import os

import numpy as np
import torch

from tests import generation_ref as GR
from tests import helpers as Hh
from tests import idefics3_ref as R

CASES = ["b1_img2", "b1_text_only", "b2_leftpad", "b2_text_leftpad", "b2_eos"]


def greedy_select(logits, V, eos_ids, pad_id, unfinished, finish_step, out, step, next_tokens):
    eos = [] if eos_ids is None else [int(e) for e in eos_ids.tolist()]
    for b in range(logits.shape[0]):
        t = int(logits[b, :V].float().argmax())           # torch: the first maximal index
        if eos and int(unfinished[b]) == 0:
            t = int(pad_id)
        out[b, step] = t
        next_tokens[b] = t
        if eos and int(unfinished[b]) != 0 and t in eos:
            unfinished[b] = 0
            finish_step[b] = step
    return next_tokens


def backend(fp32_tables=False, with_select=True):
    ns = GR.backend(fp32_tables=fp32_tables)
    ns.pixel_shuffle = R.pixel_shuffle
    if with_select:
        ns.greedy_select = greedy_select
    return ns


def load(case):
    return np.load(os.path.join(Hh.G, "generation", f"idefics3_generate_{case}.npz"))


def inputs(z):
    """-> (keyword arguments of generate, eos or None, pad)"""
    eos = int(z["eos_token_id"])
    kw = dict(input_ids=torch.from_numpy(z["input_ids"]), attention_mask=torch.from_numpy(z["attention_mask"]),
              pixel_values=torch.from_numpy(z["pixel_values"]) if "pixel_values" in z.files else None,
              pixel_attention_mask=torch.from_numpy(z["pixel_attention_mask"]) if "pixel_attention_mask" in z.files else None,
              max_new_tokens=int(z["n_steps"]))
    return kw, (None if eos < 0 else eos), int(z["pad_token_id"])


def positions(mask):
    """the reference's generation positions (idefics3 modeling_idefics3.py:1243-1249)"""
    pos = mask.long().cumsum(-1) - 1
    return pos.masked_fill(mask == 0, 1)


@torch.no_grad()
def teacher_forced_logits(model, kw, tokens):
    """the product's prefill / decode_step fed `tokens` [B, n] -> fp32 logits [n, B, V] of every step"""
    from mantis_amd import generation as Gn
    V = model.config.text_config.vocab_size
    n = tokens.shape[1]
    cache, logits = Gn.prefill(model, kw["input_ids"], kw["attention_mask"], kw["pixel_values"], n,
                               pixel_attention_mask=kw["pixel_attention_mask"])
    out = [logits[:, :V].float().cpu()]
    for i in range(n - 1):
        out.append(Gn.decode_step(model, cache, tokens[:, i].to(model.device))[:, :V].float().cpu())
    return torch.stack(out)


@torch.no_grad()
def cache_free_logits(model, kw, ids, am):
    """the engine's cache-free evaluation step on the grown sequence at the generation positions -> fp32 last-row logits [B, V]"""
    V = model.config.text_config.vocab_size
    out = model.engine.step(ids, am, None, kw["pixel_values"], kw["pixel_attention_mask"], position_ids=positions(am), need_logits=True,
                            compute_grads=False)
    return out["logits"][:, -1, :V].float()
