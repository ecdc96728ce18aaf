"""Drop-in module for the reference's `LlavaForConditionalGeneration`
(/root/reference/mantis/models/mllava/modeling_llava.py:251-262 constructor, :364-549 forward): same forward keyword
arguments, same output fields, same parameter names (state_dict-compatible with the reference / HF checkpoints), but

  * every parameter is a VIEW into one flat bf16 arena in HBM (and every gradient a view into one flat gradient arena):
    q|k|v and gate|up are stored adjacently so the fused projections are zero-copy views, data-parallel buckets are
    contiguous slices, and the optimizer is a single launch over the arena;
  * forward+backward run through `LlavaEngine` (hand-written gfx950 kernels via the C-ABI), not autograd.

`forward(..., labels=...)` in training mode with grad enabled runs the fused forward+backward and returns a loss whose
`.backward()` (called by a stock `transformers.Trainer`) publishes the already-computed gradients scaled by the incoming
gradient; `MantisHipTrainer.training_step` (trainer.py) skips even that and accumulates straight into `.grad`.
"""
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
from torch import nn

from . import backbone as BB
from .arena import ArenaModule, numel as _numel
from .configuration_llava import LlavaConfig
from . import engine as _engine


@dataclass
class LlavaCausalLMOutputWithPast(BB.ModelOutput):
    """modeling_llava.py:63-103"""
    loss: Optional[torch.Tensor] = None
    logits: Optional[torch.Tensor] = None
    past_key_values: Optional[Tuple] = None
    hidden_states: Optional[Tuple] = None
    attentions: Optional[Tuple] = None
    image_hidden_states: Optional[Tuple] = None

    def keys(self):
        return [k for k in ("loss", "logits", "past_key_values", "hidden_states", "attentions", "image_hidden_states")
                if getattr(self, k) is not None]


def _param_specs(cfg: LlavaConfig):
    """(name, shape) in ARENA ORDER: [vision tower | projector | embed | layer 0..n-1 | final norm | lm_head]."""
    vc, tc = cfg.vision_config, cfg.text_config
    dv, P, C = vc.hidden_size, vc.patch_size, vc.num_channels
    is_clip = vc.model_type == "clip_vision_model"
    npos = (vc.image_size // P) ** 2 + (1 if is_clip else 0)
    s = []
    vtp = "vision_tower."
    if is_clip:
        s.append((vtp + "embeddings.class_embedding", (dv,)))
    s.append((vtp + "embeddings.patch_embedding.weight", (dv, C, P, P)))
    if not is_clip:
        s.append((vtp + "embeddings.patch_embedding.bias", (dv,)))
    s.append((vtp + "embeddings.position_embedding.weight", (npos, dv)))
    if is_clip:
        s += [(vtp + "pre_layrnorm.weight", (dv,)), (vtp + "pre_layrnorm.bias", (dv,))]
    for i in range(vc.num_hidden_layers):
        s += BB.vit_layer_specs(f"{vtp}encoder.layers.{i}.", vc)
    s += [(vtp + "post_layernorm.weight", (dv,)), (vtp + "post_layernorm.bias", (dv,))]
    d, V = tc.hidden_size, tc.vocab_size
    s += [("multi_modal_projector.linear_1.weight", (d, dv)), ("multi_modal_projector.linear_1.bias", (d,)),
          ("multi_modal_projector.linear_2.weight", (d, d)), ("multi_modal_projector.linear_2.bias", (d,))]
    s.append(("language_model.model.embed_tokens.weight", (V, d)))
    for i in range(tc.num_hidden_layers):
        s += BB.decoder_layer_specs(f"language_model.model.layers.{i}.", tc)
    s += [("language_model.model.norm.weight", (d,)), ("language_model.lm_head.weight", (V, d))]
    return s


class LlavaForConditionalGeneration(ArenaModule):
    config_class = LlavaConfig
    supports_gradient_checkpointing = True       # per decoder layer (decoder.decoder_forward(checkpoint=True)); the frozen tower saves nothing anyway
    frozen_prefixes = ("vision_tower.",)      # train_mllava.py:240-242

    def __init__(self, config: LlavaConfig, device=None, dtype=torch.bfloat16, init="normal", seed=0):
        super().__init__()
        self.config = config
        self.vocab_size = config.vocab_size
        self.pad_token_id = config.pad_token_id if config.pad_token_id is not None else -1
        self._init_arena(_param_specs(config), device, dtype)
        self._trainable_start = self._offs["multi_modal_projector.linear_1.weight"]
        self.engine = _engine.LlavaEngine(self)
        self._build_views()
        if init == "normal":
            self.reset_parameters(seed)
        self.train()

    def _build_views(self):
        vc, tc = self.config.vision_config, self.config.text_config
        g = lambda n: self._param(n).data
        is_clip = vc.model_type == "clip_vision_model"
        vtp = "vision_tower."
        kp, patch_w_padded = BB.patch_w_padded(self, vtp + "embeddings.patch_embedding.weight", vc)
        self.vt = dict(patch_kp=kp, patch_w_padded=patch_w_padded,
                       patch_b=None if is_clip else g(vtp + "embeddings.patch_embedding.bias"),
                       pos=g(vtp + "embeddings.position_embedding.weight"),
                       cls=g(vtp + "embeddings.class_embedding") if is_clip else None,
                       pre_ln=(g(vtp + "pre_layrnorm.weight"), g(vtp + "pre_layrnorm.bias")) if is_clip else None,
                       layers=[BB.vit_layer_views(self, f"{vtp}encoder.layers.{i}.", vc) for i in range(vc.num_hidden_layers)])
        self.proj = dict(w1=g("multi_modal_projector.linear_1.weight"), b1=g("multi_modal_projector.linear_1.bias"),
                         w2=g("multi_modal_projector.linear_2.weight"), b2=g("multi_modal_projector.linear_2.bias"))
        ll = [BB.decoder_layer_views(f"language_model.model.layers.{i}.", tc, g, self._flat) for i in range(tc.num_hidden_layers)]
        self.lm = dict(embed=g("language_model.model.embed_tokens.weight"), layers=ll,
                       norm=g("language_model.model.norm.weight"), head=g("language_model.lm_head.weight"))

    def _init_value(self, name, p):
        """modeling_llava.py:150-170 / HF _init_weights; CLIP's 1-D class embedding is drawn like a matrix"""
        return None if "class_embedding" in name else super()._init_value(name, p)

    # ------------------------------------------------------------------ reference-compatible accessors
    def get_input_embeddings(self):
        return self.language_model.model.embed_tokens

    def get_output_embeddings(self):
        return self.language_model.lm_head

    def load_reference_state_dict(self, sd, strict=True):
        """Accepts the reference's state_dict names (HF-5 flat `vision_tower.*` or 4.x `vision_tower.vision_model.*`);
        pooling-head tensors of SigLIP (dead on this path) are ignored."""
        return self.copy_state_dict(sd, rename=lambda k: k.replace("vision_tower.vision_model.", "vision_tower."),
                                    ignorable=lambda k: ".head." in k or k.endswith("position_ids"), strict=strict)

    def _build_grad_views(self):
        tc = self.config.text_config
        gv = self._grad_views.get
        self.grads = dict(head=gv("language_model.lm_head.weight"), norm=gv("language_model.model.norm.weight"),
                          embed=gv("language_model.model.embed_tokens.weight"),
                          w1=gv("multi_modal_projector.linear_1.weight"), b1=gv("multi_modal_projector.linear_1.bias"),
                          w2=gv("multi_modal_projector.linear_2.weight"), b2=gv("multi_modal_projector.linear_2.bias"))
        self.grads_layers = [BB.decoder_layer_views(f"language_model.model.layers.{i}.", tc, gv, self._gflat)
                             for i in range(tc.num_hidden_layers)]

    def grad_buckets(self):
        """Contiguous slices of the gradient arena in the order backward completes them (for the DP reducer): 'head' (final norm +
        lm_head); the three sub-buckets of every decoder layer n-1 .. 0 (backbone.decoder_buckets); 'front' (projector + embedding)."""
        self._ensure_grad_arena()
        span = self._bucket_span
        out = {"head": span(lambda n: n.startswith("language_model.model.norm") or n.startswith("language_model.lm_head")),
               **BB.decoder_buckets(span, "language_model.model.layers.", self.config.text_config.num_hidden_layers),
               "front": span(lambda n: n.startswith("multi_modal_projector.") or n.startswith("language_model.model.embed_tokens"))}
        return {k: v for k, v in out.items() if v is not None}

    # ------------------------------------------------------------------ generation (greedy, KV cache: mantis_amd/generation.py)
    def generate(self, input_ids=None, pixel_values=None, attention_mask=None, max_new_tokens=None, max_length=None, eos_token_id=None,
                 pad_token_id=None, do_sample=False, num_beams=1, streamer=None, **rest):
        """Greedy search exactly as HF's `generate` returns it for the reference class (what `chat_mllava` / `chat_mllava_stream` call,
        /root/reference/mantis/models/mllava/utils.py:33-42,77-88): LongTensor [B, T + n] = the prompt followed by the new tokens, a
        finished row filled with pad_token_id, stopping when every row has emitted an EOS (int or list) or at the length limit.
        pixel_values: a tensor or the reference's list of per-sample tensors (None: text only).  B > 1 needs left padding.  Any other
        generation argument raises NotImplementedError naming it.  Works in train() and eval() mode; touches no gradient buffer."""
        from . import generation as _generation
        _generation._refuse_unsupported(rest)          # generation.generate's own keywords beyond this signature are not public here
        return _generation.generate(self, input_ids, pixel_values=pixel_values, attention_mask=attention_mask,
                                    max_new_tokens=max_new_tokens, max_length=max_length, eos_token_id=eos_token_id,
                                    pad_token_id=pad_token_id, streamer=streamer, do_sample=do_sample, num_beams=num_beams, **rest)

    # ------------------------------------------------------------------ forward (contract 2 of SURVEY.md section 8b)
    def forward(self, input_ids=None, pixel_values=None, attention_mask=None, position_ids=None, past_key_values=None,
                inputs_embeds=None, vision_feature_layer=None, vision_feature_select_strategy=None, labels=None,
                use_cache=None, output_attentions=None, output_hidden_states=None, return_dict=None, return_logits=None,
                _record=None, segment_ids=None):
        if inputs_embeds is not None or past_key_values is not None or use_cache:
            raise NotImplementedError("forward() takes no inputs_embeds / past_key_values / use_cache (training and evaluation forward "
                                      "only); for greedy decoding with a KV cache call generate()")
        if output_attentions or output_hidden_states:
            raise NotImplementedError("output_attentions / output_hidden_states are not produced by the fused kernels")
        if vision_feature_layer is not None and vision_feature_layer != self.config.vision_feature_layer:
            raise NotImplementedError("per-call vision_feature_layer override")
        if vision_feature_select_strategy is not None and vision_feature_select_strategy != self.config.vision_feature_select_strategy:
            if vision_feature_select_strategy not in ("default", "full"):
                raise ValueError(f"Unexpected select feature strategy: {vision_feature_select_strategy}")
            raise NotImplementedError("per-call vision_feature_select_strategy override")
        if attention_mask is not None and attention_mask.dim() == 4:
            # the reference's packed batch (mantis/train/data.py:1609-1671): block-diagonal 4-D mask + restarting position ids
            from .data import segments_from_packed
            segment_ids, attention_mask = segments_from_packed(dict(attention_mask=attention_mask, position_ids=position_ids,
                                                                    segment_ids=segment_ids))
        # this class hands the logits out as the head wrote them (no `.float()`, unlike the Idefics2 / Qwen2-VL classes)
        return self._forward_step(input_ids, attention_mask, labels, (pixel_values,), LlavaCausalLMOutputWithPast, return_dict, return_logits,
                                  float_logits=False, record=_record, segment_ids=segment_ids)
