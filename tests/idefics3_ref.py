"""Test infrastructure: fp32 torch-CPU restatement of the Idefics3 training step of the Mantis fork
(mantis/models/idefics3/modeling_idefics3.py: Idefics3Model.forward :899-1017, Idefics3ForConditionalGeneration.forward :1076-1211),
built on the Idefics2 oracle -- the NaViT SigLIP tower and the Llama / Mistral block are the same code there -- and on the oracle's
operator restatement (oracle/ops_ref.py) for the backend that drives the product's host logic on the CPU.

What is Idefics3's own:
  connector   pixel shuffle (:651-660, a row permutation) + ONE bias-free linear (Idefics3SimpleMLP :387-395); ignores the patch mask
  loss        shifted cross-entropy over attention_mask[:, 1:] != 0 with torch's DEFAULT ignore index -100 (:1186-1198): a label equal to
              image_token_id is a counted target, unlike on the Idefics2 path

PARITY PIN: tests/golden/make_golden_idefics3.py runs the reference class and records inputs, weights, activations, loss and gradients
under tests/golden/idefics3/; tests/test_idefics3.py checks this restatement against them."""
import json
import os
import types

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ops_ref
from oracle.idefics2_ref import Idefics2Ref, patch_mask_from_pixel_mask

G3 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "idefics3")
CASES = ["b1_img2", "b1_navit", "b2_padimg_rightpad", "b1_text_only", "b1_scale4", "b1_label_quirk"]
PROJ = "model.connector.modality_projection.proj.weight"


def pixel_shuffle_closed_form(x, s):
    """out[i, hq*(W/s) + wq, (hr*s + wr)*C + c] = x[i, (hq*s + hr)*W + wq*s + wr, c] with W = H = sqrt(N); x [I, N, C]"""
    I, N, C = x.shape
    H = int(round(N ** 0.5))
    assert H * H == N and H % s == 0, (N, s)
    Wq = H // s
    out = torch.empty((I, Wq * Wq, s * s * C), dtype=x.dtype)
    for hq in range(Wq):
        for wq in range(Wq):
            for hr in range(s):
                for wr in range(s):
                    j = hr * s + wr
                    out[:, hq * Wq + wq, j * C: (j + 1) * C] = x[:, (hq * s + hr) * H + wq * s + wr]
    return out


def pixel_shuffle_ref(x, s):
    """The same permutation as one reshape / permute (what the restatement and the CPU backend run): [I, N, C] -> [I, N/s^2, s*s*C]"""
    I, N, C = x.shape
    H = int(round(N ** 0.5))
    assert H * H == N and H % s == 0, (N, s)
    Wq = H // s
    return x.reshape(I, Wq, s, Wq, s, C).permute(0, 1, 3, 2, 4, 5).reshape(I, Wq * Wq, s * s * C)


def pixel_shuffle(x, I, H, s):
    """Backend operator with the signature of mantis_amd.hip_ops.pixel_shuffle: x [I*H*H, C] -> [I*(H/s)^2, s*s*C]"""
    if x.shape[1] % 8 or H % s:
        raise RuntimeError("pixel_shuffle failed: unsupported shape/alignment (rc=-2)")
    return pixel_shuffle_ref(x.reshape(I, H * H, -1), s).reshape(I * (H // s) ** 2, -1).contiguous()


def backend():
    """The oracle's operator restatement + pixel_shuffle, as one backend object for `mantis_amd.modeling_idefics2.K`."""
    ns = types.SimpleNamespace(**{k: getattr(ops_ref, k) for k in dir(ops_ref) if not k.startswith("__")})
    ns.pixel_shuffle = pixel_shuffle
    return ns


class Idefics3Ref(Idefics2Ref):
    """cfg = dict(vision=..., text=..., image_token_id=..., scale_factor=...); weights under the reference's state_dict names."""

    def __init__(self, weights, cfg, dtype=torch.float32):
        self.cfg = cfg
        self.vc, self.tc = cfg["vision"], cfg["text"]
        self.w = {}
        for k, v in weights.items():
            t = torch.as_tensor(np.asarray(v) if not isinstance(v, torch.Tensor) else v).to(dtype).clone()
            t.requires_grad_(not k.startswith("model.vision_model."))           # the tower is frozen (train_idefics3.py:141-143)
            self.w[k] = t

    @classmethod
    def from_golden(cls, case=None, bf16_weights=False, **kw):
        """The recorded weights (+ the case's own connector weight and scale factor where it carries them: b1_scale4)."""
        meta, sd = golden_cfg_and_weights(case)
        if bf16_weights:
            sd = {k: torch.from_numpy(v).to(torch.bfloat16).float() for k, v in sd.items()}
        return cls(sd, meta, **kw)

    def connector(self, feats, patch_key_mask=None, record=None):
        return F.linear(pixel_shuffle_ref(feats, self.cfg["scale_factor"]), self.w[PROJ])

    def forward(self, input_ids, pixel_values, pixel_attention_mask, attention_mask, labels, record=None, ignore_image_labels=False):
        """Same signature as Idefics2Ref.forward.  ignore_image_labels: the loss with labels == image_token_id dropped as well -- NOT
        what the reference computes (the fixtures record it as `loss_ignoring_image_labels` to prove they can tell the two apart)."""
        cfg, w = self.cfg, self.w
        ids = torch.as_tensor(input_ids)
        am = torch.as_tensor(attention_mask)
        emb = F.embedding(ids, w["model.text_model.embed_tokens.weight"])
        if pixel_values is not None:
            pv = torch.as_tensor(pixel_values).float()
            B, M = pv.shape[:2]
            pv = pv.reshape(B * M, *pv.shape[2:])
            real = (pv == 0.0).sum(dim=(-1, -2, -3)) != pv[0].numel()                       # :953-956
            pv = pv[real]
            if pixel_attention_mask is None:
                pm = torch.ones(pv.shape[0], pv.shape[2], pv.shape[3], dtype=torch.bool)
            else:
                pm = torch.as_tensor(pixel_attention_mask).bool().reshape(B * M, *pixel_attention_mask.shape[2:])[real]
            patch_mask = patch_mask_from_pixel_mask(pm, self.vc["patch_size"])              # :972-975
            feats = self.vision(pv.to(w["lm_head.weight"].dtype), patch_mask)
            if record is not None:
                record["vision_last_hidden_state"] = feats
            img = self.connector(feats)
            if record is not None:
                record["connector_out"] = img
            sel = ids == cfg["image_token_id"]
            rows = img.reshape(-1, img.shape[-1])
            if int(sel.sum()) != rows.shape[0]:
                raise ValueError(f"{int(sel.sum())} <image> tokens for {rows.shape[0]} image hidden states")
            bi, ti = torch.nonzero(sel, as_tuple=True)
            emb = emb.index_put((bi, ti), rows)                                             # :880-885
            if record is not None:
                record["merged_embeds"] = emb
        h = self.text(emb, am, record)
        logits = F.linear(h, w["lm_head.weight"]).float()
        loss = None
        if labels is not None:
            lab = torch.as_tensor(labels)
            keep = am[..., 1:] != 0
            tgt = lab[..., 1:][keep]
            if ignore_image_labels:
                tgt = torch.where(tgt == cfg["image_token_id"], torch.full_like(tgt, -100), tgt)
            loss = F.cross_entropy(logits[..., :-1, :][keep], tgt)                          # :1186-1198: CrossEntropyLoss(), ignore -100
        return loss, logits


# ----------------------------------------------------------------------------------------------------------- fixtures and builders
def load_case(name):
    return np.load(os.path.join(G3, name + ".npz"))


def golden_cfg_and_weights(case=None):
    z = np.load(os.path.join(G3, "weights.npz"))
    meta = json.loads(str(z["__config__"]))
    sd = {k: z[k] for k in z.files if k != "__config__"}
    if case is not None:
        c = load_case(case)
        if "scale_factor" in c.files:
            meta["scale_factor"] = int(c["scale_factor"])
        for k in c.files:
            if k.startswith("weight."):
                sd[k[7:]] = c[k]
    return meta, sd


def build_product(device, case=None):
    from mantis_amd.configuration_idefics3 import Idefics3Config
    from mantis_amd.modeling_idefics3 import Idefics3ForConditionalGeneration
    meta, sd = golden_cfg_and_weights(case)
    model = Idefics3ForConditionalGeneration(Idefics3Config.from_oracle_meta(meta), device=device, init=None)
    model.load_reference_state_dict(sd)
    return model


def batch(z):
    b = dict(input_ids=torch.from_numpy(z["input_ids"]), attention_mask=torch.from_numpy(z["attention_mask"]),
             labels=torch.from_numpy(z["labels"]))
    b["pixel_values"] = torch.from_numpy(z["pixel_values"]) if "pixel_values" in z.files else None
    b["pixel_attention_mask"] = torch.from_numpy(z["pixel_attention_mask"]) if "pixel_attention_mask" in z.files else None
    return b


def full_width_batch(cfg, seed=0):
    """The batch of the GPU check `idefics3_full_width_vs_oracle`: B = 2, three and two 364 x 364 tiles, T = 1024, every <image> run
    whole (169 tokens per tile); the prompt head and the <image> positions of sample 1 at -100, those of sample 0 counted."""
    g = torch.Generator().manual_seed(seed)
    n_tok = (cfg.vision_config.image_size // cfg.vision_config.patch_size // cfg.scale_factor) ** 2
    B, T, counts = 2, 1024, (3, 2)
    V_ = cfg.text_config.vocab_size
    ids = torch.randint(1, 120000, (B, T), generator=g)
    ids[ids == cfg.image_token_id] = 7
    for b, c in enumerate(counts):
        for j in range(c):
            s = 8 + j * (n_tok + 24)
            ids[b, s: s + n_tok] = cfg.image_token_id
    assert V_ > 120000
    am = torch.ones(B, T, dtype=torch.int64)
    am[1, T - 37:] = 0
    lab = ids.clone()
    lab[:, :6] = -100
    lab[am == 0] = -100
    lab[1][ids[1] == cfg.image_token_id] = -100
    S = cfg.vision_config.image_size
    pv = torch.zeros(B, max(counts), 3, S, S)
    for b, c in enumerate(counts):
        pv[b, :c] = torch.randn(c, 3, S, S, generator=g).to(torch.bfloat16).float()
    return dict(input_ids=ids, attention_mask=am, labels=lab, pixel_values=pv, pixel_attention_mask=None)


def bf16_envelope(case):
    """{tensor: (cosine, rel-L2)} of the reference's bf16 run against its fp32 run for `case` (a key of tests/golden/idefics3/bf16_envelope.json)"""
    with open(os.path.join(G3, "bf16_envelope.json")) as f:
        env = json.load(f)
    return {k: (float(v[0]), float(v[1])) for k, v in env[case].items() if not k.startswith("__")}
