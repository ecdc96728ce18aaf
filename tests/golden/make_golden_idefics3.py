#!/usr/bin/env python3
"""Golden fixtures for the Idefics3 path by RUNNING the reference fork's `Idefics3ForConditionalGeneration`
(mantis/models/idefics3/modeling_idefics3.py, forward :1076-1211 over Idefics3Model.forward :899-1017) in the build container, and the
reference's own bf16-vs-fp32 deviation on the same cases.  Nothing of the reference is restated here: it is imported and run.

Written to tests/golden/idefics3/ (a directory of its own: tests/test_oracle_vs_golden.py globs tests/golden/*.npz):
  weights.npz          the seeded tiny model's state_dict (values exactly representable in bf16) + the config as json
  <case>.npz           inputs, the vision tower's last_hidden_state, the connector output, merged embeddings, every text layer's output,
                       fp32 logits, loss, the gradient of every trainable parameter (the tower is frozen, train_idefics3.py:141-143;
                       mantissas rounded to 14 bits), and `loss_ignoring_image_labels`: the loss recomputed from the recorded logits with
                       labels == image_token_id ignored as well -- the reference's loss (:1186-1198, CrossEntropyLoss() with its default
                       ignore index -100) COUNTS them, and the two numbers must differ wherever the batch holds images
  bf16_envelope.json   {case: {tensor: [cosine, rel-L2]}} of the reference's bf16 gradients against its fp32 gradients
                       ("reference_bf16:<case>"), and -- with the argument `full_width` -- the pinned restatement (tests/idefics3_ref.py) in
                       bf16 against fp32 at the geometry of the GPU check `idefics3_full_width_vs_oracle` ("oracle_bf16:idefics3_full_width")

Shims needed under the installed transformers: the `tie_weights` override, `use_cache=False`, and `_attn_implementation = "eager"` on
the config and on both of its sub-configs.    Usage: python tests/golden/make_golden_idefics3.py [cases] [full_width]
"""
import copy
import json
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "idefics3")
REF = os.environ.get("MANTIS_REFERENCE", "/root/reference")
V, IMG, PAD = 300, 298, 0
PROJ = "model.connector.modality_projection.proj.weight"


def meta(scale_factor=2):
    return dict(
        vision=dict(hidden_size=64, intermediate_size=112, num_hidden_layers=3, num_attention_heads=4, image_size=56, patch_size=14,
                    num_channels=3, hidden_act="gelu_pytorch_tanh", layer_norm_eps=1e-6),
        text=dict(model_type="llama", hidden_size=64, intermediate_size=176, num_hidden_layers=2, num_attention_heads=4,
                  num_key_value_heads=2, vocab_size=V, rope_theta=10000.0, rms_norm_eps=1e-5, max_position_embeddings=512,
                  hidden_act="silu", pad_token_id=PAD, tie_word_embeddings=False),
        image_token_id=IMG, scale_factor=scale_factor, vocab_size=V, pad_token_id=PAD)


def round_mantissa(a, bits=14):
    """fp32 rounded to `bits` mantissa bits (relative error <= 2^-15): keeps every compressed fixture under the 1 MiB file limit."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    drop = 23 - bits
    return (((u + np.uint32(1 << (drop - 1))) >> np.uint32(drop)) << np.uint32(drop)).view(np.float32)


def build(seed, scale_factor=2):
    import transformers.utils.hub as hub
    for n in ("is_remote_url", "download_url"):
        if not hasattr(hub, n):
            setattr(hub, n, lambda *a, **k: False)
    sys.path.insert(0, REF)
    from mantis.models.idefics3.configuration_idefics3 import Idefics3Config
    from mantis.models.idefics3.modeling_idefics3 import Idefics3ForConditionalGeneration

    class Oracle(Idefics3ForConditionalGeneration):
        def tie_weights(self, *a, **k):
            return None

    m = meta(scale_factor)
    cfg = Idefics3Config(vision_config=dict(m["vision"]), text_config=dict(m["text"]), image_token_id=IMG, scale_factor=scale_factor,
                         tie_word_embeddings=False, pad_token_id=PAD, use_cache=False)
    for c in (cfg, cfg.vision_config, cfg.text_config):
        c._attn_implementation = "eager"
    torch.manual_seed(seed)
    model = Oracle(cfg)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.dim() == 1:
                if "norm" in n and n.endswith("weight"):
                    p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
                else:
                    p.copy_(0.05 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(p + 0.05 * torch.randn(p.shape, generator=g))
            p.copy_(p.to(torch.bfloat16).float())          # bf16-exact values: the product's arena holds these very weights
    for n, p in model.named_parameters():
        if "vision_model" in n:
            p.requires_grad_(False)
    model.train()
    return model


def forward(model, z, dtype=torch.float32):
    model.zero_grad(set_to_none=True)
    pv = z.get("pixel_values")
    pm = z.get("pixel_attention_mask")
    res = model(input_ids=torch.from_numpy(z["input_ids"]), attention_mask=torch.from_numpy(z["attention_mask"]),
                labels=torch.from_numpy(z["labels"]), pixel_values=None if pv is None else torch.from_numpy(pv).to(dtype),
                pixel_attention_mask=None if pm is None else torch.from_numpy(pm), use_cache=False)
    res.loss.backward()
    return res


def run_case(model, name, ids, mask, labels, pixels, pixel_mask, extra=None):
    out = dict(input_ids=ids, attention_mask=mask, labels=labels)
    acts, hooks = {}, []
    mm = model.model
    if pixels is not None:
        out["pixel_values"] = pixels
        if pixel_mask is not None:
            out["pixel_attention_mask"] = pixel_mask
        hooks.append(mm.vision_model.register_forward_hook(lambda m, a, o: acts.__setitem__("vision_last_hidden_state", o.last_hidden_state.detach())))
        hooks.append(mm.connector.register_forward_hook(lambda m, a, o: acts.__setitem__("connector_out", o.detach())))
        orig = mm.inputs_merger

        def merger(*a, **k):
            r = orig(*a, **k)
            acts["merged_embeds"] = r.detach().clone()
            return r
        mm.inputs_merger = merger
    for i, layer in enumerate(mm.text_model.layers):
        hooks.append(layer.register_forward_hook(lambda m, a, o, i=i: acts.__setitem__(f"llm_layer{i}_out", (o[0] if isinstance(o, tuple) else o).detach())))
    res = forward(model, out)
    for h in hooks:
        h.remove()
    if pixels is not None:
        del mm.inputs_merger
    out["loss"] = res.loss.detach().numpy()
    out["logits"] = res.logits.detach().numpy()
    keep = torch.from_numpy(mask)[:, 1:] != 0
    tgt = torch.from_numpy(labels)[:, 1:][keep]
    alt = F.cross_entropy(res.logits.detach()[:, :-1][keep], torch.where(tgt == IMG, torch.full_like(tgt, -100), tgt))
    out["loss_ignoring_image_labels"] = alt.numpy()
    n_img_lab = int(((tgt == IMG)).sum())
    assert (n_img_lab > 0) == (pixels is not None)
    if n_img_lab:
        assert abs(float(alt) - float(res.loss)) > 1e-3 * float(res.loss), "the fixture cannot tell the two loss rules apart"
    for k, v in acts.items():
        out[k] = v.numpy()
    for n, p in model.named_parameters():
        if p.grad is not None:
            out["grad." + n] = round_mantissa(p.grad.detach().numpy())
    out.update(extra or {})
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20), (name, os.path.getsize(path))
    print(f"{name}: loss={float(res.loss):.6f} (image labels ignored: {float(alt):.6f}; {n_img_lab} such targets, "
          f"{int((tgt == -100).sum())} at -100) logits{tuple(res.logits.shape)} grads={sum(1 for k in out if k.startswith('grad.'))} "
          f"{os.path.getsize(path)} B", flush=True)
    return out


def cos_rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    na, nb = np.linalg.norm(a), np.linalg.norm(b)
    if na == 0 or nb == 0:
        return (1.0 if na == nb else 0.0), (0.0 if na == nb else 1.0)
    return float(a @ b / (na * nb)), float(np.linalg.norm(a - b) / nb)


def merge_envelope(results):
    path = os.path.join(OUT, "bf16_envelope.json")
    cur = {}
    if os.path.exists(path):
        with open(path) as f:
            cur = json.load(f)
    cur.update(results)
    cur["__doc__"] = ("per case and trainable tensor: [cosine, rel-L2] of the reference's bf16 gradient against its fp32 gradient on the same "
                      "bf16-exact weights; written by tests/golden/make_golden_idefics3.py (see its docstring)")
    with open(path, "w") as f:
        json.dump(cur, f, indent=0, sort_keys=True)
        f.write("\n")


def envelope(model, name, z):
    """The reference class with the module in bf16 (weights + activations, as the training script runs it) against its fp32 run."""
    m16 = copy.deepcopy(model).to(torch.bfloat16)
    grads, losses = {}, {}
    for tag, m, dt in (("fp32", model, torch.float32), ("bf16", m16, torch.bfloat16)):
        r = forward(m, z, dt)
        losses[tag] = float(r.loss)
        grads[tag] = {n: p.grad.detach().float().numpy().copy() for n, p in m.named_parameters() if p.grad is not None}
    rep = {n: list(cos_rel(grads["bf16"][n], grads["fp32"][n])) for n in grads["fp32"]}
    rep["__loss__"] = [losses["bf16"], losses["fp32"]]
    wn = max((n for n in rep if not n.startswith("__")), key=lambda n: rep[n][1])
    print(f"   envelope {name}: loss bf16 {losses['bf16']:.5f} fp32 {losses['fp32']:.5f}; worst rel-L2 {rep[wn][1]:.4f} ({wn})", flush=True)
    return {"reference_bf16:" + name: rep}


def cases():
    os.makedirs(OUT, exist_ok=True)
    model = build(37)
    sd = {k: v.detach().numpy() for k, v in model.state_dict().items()}
    path = os.path.join(OUT, "weights.npz")
    np.savez_compressed(path, __config__=np.array(json.dumps(meta())), **sd)
    assert os.path.getsize(path) < (1 << 20), os.path.getsize(path)
    print(f"weights.npz: {len(sd)} tensors, {os.path.getsize(path)} B")
    rng = np.random.default_rng(83)
    env = {}

    def text(T, img_starts, n_pad=0, n_tok=4):
        """labels as the training collator leaves them for this class: the prompt head and the padding at -100; <image> positions keep
        their own id, which the reference's loss counts"""
        ids = rng.integers(1, 290, size=T, dtype=np.int64)
        for s in img_starts:
            ids[s: s + n_tok] = IMG
        mask = np.ones(T, np.int64)
        if n_pad:
            ids[T - n_pad:] = PAD
            mask[T - n_pad:] = 0
        lab = ids.copy()
        lab[:5] = -100
        lab[mask == 0] = -100
        return ids, mask, lab

    def px(n, side=56):
        return rng.standard_normal((n, 3, side, side)).astype(np.float16).astype(np.float32)      # fp16-exact pixels

    def record(mdl, name, *a, **k):
        z = run_case(mdl, name, *a, **k)
        env.update(envelope(mdl, name, z))

    # B=1, two full-resolution images (4 <image> tokens each at scale 2)
    i, m, l = text(26, [3, 14])
    record(model, "b1_img2", i[None], m[None], l[None], px(2)[None], None)
    # B=1, a pixel_attention_mask that masks part of image 0 (42 x 28 px attended inside the 56 x 56 canvas); the connector ignores it
    pm = np.ones((1, 2, 56, 56), bool)
    pm[0, 0] = False
    pm[0, 0, :42, :28] = True
    pv = px(2)[None]
    pv[0, 0][:, ~pm[0, 0]] = 0.0
    i, m, l = text(26, [2, 12])
    record(model, "b1_navit", i[None], m[None], l[None], pv, pm)
    # B=2: sample 0 has two images, sample 1 one image (+ an all-zero padding image) and right-padded text
    pv = np.zeros((2, 2, 3, 56, 56), np.float32)
    pv[0] = px(2)
    pv[1, 0] = px(1)[0]
    pm = np.ones((2, 2, 56, 56), bool)
    pm[1, 0] = False
    pm[1, 0, :28, :56] = True
    pv[1, 0][:, ~pm[1, 0]] = 0.0
    a = text(28, [1, 16])
    b = text(28, [6], n_pad=4)
    record(model, "b2_padimg_rightpad", np.stack([a[0], b[0]]), np.stack([a[1], b[1]]), np.stack([a[2], b[2]]), pv, pm)
    # text only
    i, m, l = text(20, [], n_pad=3)
    record(model, "b1_text_only", i[None], m[None], l[None], None, None)
    # the pin for the loss rule: -100 AND image_token_id labels at attended positions, some <image> positions at -100, some counted
    i, m, l = text(26, [6, 15])
    l[6:8] = -100
    l[15] = -100
    assert (l == -100).any() and (l[m != 0] == IMG).sum() == 5
    record(model, "b1_label_quirk", i[None], m[None], l[None], px(2)[None], None)
    # 112 x 112 images, scale_factor 4: 8 x 8 patches -> 4 <image> tokens; the connector weight is [64, 16 * 64], everything else is the
    # model above
    m4 = build(37, scale_factor=4)
    with torch.no_grad():
        own = dict(model.named_parameters())
        for n, p in m4.named_parameters():
            if n != PROJ:
                p.copy_(own[n])
    i, m, l = text(26, [4, 13])
    record(m4, "b1_scale4", i[None], m[None], l[None], px(2, 112)[None], None,
           extra={"scale_factor": np.array(4), "weight." + PROJ: dict(m4.named_parameters())[PROJ].detach().numpy()})
    merge_envelope(env)


def full_width():
    """bf16 vs fp32 of the restatement (pinned to the reference class by tests/test_idefics3.py) at 8B widths, tower depth 2, decoder
    depth 2: the reference's own arithmetic deviation at the geometry the tiny cases cannot show."""
    import time
    sys.path.insert(0, ROOT)
    from mantis_amd.configuration_idefics3 import idefics3_8b_llama3
    from mantis_amd.modeling_idefics3 import Idefics3ForConditionalGeneration
    from tests.idefics3_ref import Idefics3Ref, full_width_batch
    cfg = idefics3_8b_llama3()
    cfg.vision_config.num_hidden_layers = 2
    cfg.text_config.num_hidden_layers = 2
    model = Idefics3ForConditionalGeneration(cfg, device="cpu", seed=0)
    m = cfg.to_oracle_meta()
    w = {n: p.detach().float().clone() for n, p in model.named_parameters()}
    train = {n for n, p in model.named_parameters() if p.requires_grad}
    del model
    b = full_width_batch(cfg)
    out = {}
    for tag, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        t0 = time.time()
        o = Idefics3Ref(w, m, dtype=dt)
        loss, _ = o.forward(b["input_ids"].numpy(), b["pixel_values"].numpy(), None, b["attention_mask"].numpy(), b["labels"].numpy())
        loss.backward()
        out[tag] = ({n: t.grad.detach().float().numpy().copy() for n, t in o.w.items() if t.grad is not None}, float(loss))
        print(f"    {tag}: loss {float(loss):.5f} in {time.time() - t0:.0f} s", flush=True)
        del o
    g32, g16 = out["fp32"][0], out["bf16"][0]
    rep = {n: list(cos_rel(g16[n], g32[n])) for n in g32 if n in g16 and n in train}
    rep["__loss__"] = [out["bf16"][1], out["fp32"][1]]
    merge_envelope({"oracle_bf16:idefics3_full_width": rep})
    wn = max((n for n in rep if not n.startswith("__")), key=lambda n: rep[n][1])
    print(f"full_width: {len(rep) - 1} tensors, worst rel-L2 {rep[wn][1]:.4f} / cos {rep[wn][0]:.5f} ({wn})", flush=True)


if __name__ == "__main__":
    torch.manual_seed(0)
    for what in (sys.argv[1:] or ["cases", "full_width"]):
        {"cases": cases, "full_width": full_width}[what]()
