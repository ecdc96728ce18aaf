"""Drop-in module for the reference fork's `Idefics3ForConditionalGeneration` (mantis/models/idefics3/modeling_idefics3.py:1024-1211 over
Idefics3Model :816-1017; what mantis/train/train_idefics3.py instantiates): same forward keyword arguments, same output fields, same
parameter names (state_dict-compatible), on the flat-arena layout of `ArenaModule` and the hand-written gfx950 kernels.

Idefics3 is a new composition of what the other paths already run: the NaViT SigLIP tower of the Idefics2 path (frozen,
train_idefics3.py:141-143), the one-slot-per-<image>-token merger of the Idefics2 path, and the Llama-3 decoder, head and loss kernels of
the LLaVA path.  Its own part is the connector (:642-665): a pixel shuffle -- a pure row permutation, `hip_ops.pixel_shuffle` -- followed
by ONE bias-free linear.  The tower being frozen, the connector's backward is only dW = dY^T . shuffled rows (kept by the forward): no
inverse shuffle exists or is needed.

THE LOSS RULE (:1186-1198): shifted cross-entropy over the positions with attention_mask[:, 1:] != 0 through `CrossEntropyLoss()` with
torch's default ignore index -100.  Unlike on the Idefics2 path, a label equal to `image_token_id` is therefore a COUNTED target (class
`image_token_id` of the vocabulary), also where it sits on an <image> token: the training script's `set_ignore_index(image_token_id)`
(train_idefics3.py:161) steers the collator, it does not reach this loss.  Reproduced here as it is; a collator that wants such positions
ignored must write -100.

GENERATION: `generate` is greedy search with a KV cache (generation.py), as mantis/mllm_tools/idefics3_eval.py:64 calls the reference
class; the prefill is this engine's evaluation forward at the reference's generation positions (`attention_mask.cumsum(-1) - 1`), the
decode steps are the LLaVA path's Llama-3 decode kernels.  `forward` itself keeps refusing the cache arguments.

Out of scope: sampling / beam search, the image processor and its tile splitting, LoRA / QLoRA, and the fp8 decoder variant
(`set_precision("fp8")` refuses by name)."""
import torch

from . import backbone as BB
from . import modeling_idefics2 as I2       # the engine's operators are I2.K: tests monkeypatch that one name
from .configuration_idefics3 import Idefics3Config
from .modeling_idefics2 import Idefics2CausalLMOutputWithPast, Idefics2Engine, Idefics2ForConditionalGeneration

PROJ = "model.connector.modality_projection.proj.weight"


class Idefics3CausalLMOutputWithPast(Idefics2CausalLMOutputWithPast):
    """modeling_idefics3.py:92-126: the same fields as the Idefics2 output"""


class Idefics3ForConditionalGeneration(Idefics2ForConditionalGeneration):
    """`model(**batch).loss.backward()` (arena.FusedStep), `MantisHipTrainer` / `as_hf_trainer()`, `grad_buckets()`,
    `gradient_checkpointing_enable()`, `FusedAdamW` and the low-priority tower prefetch work as on the Idefics2 path: the forward
    contract, the refusals (KV cache arguments of `forward`, inputs_embeds, image_hidden_states, output_attentions / output_hidden_states, explicit
    position_ids -> NotImplementedError) and the gradient buckets ('front' = connector projection + token embedding) are inherited."""
    config_class = Idefics3Config
    output_class = Idefics3CausalLMOutputWithPast

    def _param_specs(self, config):
        """(name, shape) in ARENA ORDER: [vision tower | connector projection | embed | text layer 0..n-1 | final norm | lm_head]"""
        dv, d, s = config.vision_config.hidden_size, config.text_config.hidden_size, config.scale_factor
        return I2._vision_specs(config.vision_config) + [(PROJ, (d, dv * s * s))] + I2._text_specs(config, self.head_kind)

    def _make_engine(self):
        return Idefics3Engine(self)

    def _build_connector_views(self, g):
        self.conn = dict(proj=g(PROJ))

    def _build_connector_grad_views(self, gv):
        self.grads_conn = dict(proj=gv(PROJ))

    def generate(self, input_ids=None, pixel_values=None, pixel_attention_mask=None, attention_mask=None, max_new_tokens=None,
                 max_length=None, eos_token_id=None, pad_token_id=None, do_sample=False, num_beams=1, streamer=None, **rest):
        """Greedy search exactly as HF's `generate` returns it for the reference class (mantis/mllm_tools/idefics3_eval.py:64:
        `model.generate(**inputs, max_new_tokens=512, num_beams=1)` with the processor's input_ids, attention_mask, pixel_values
        [B, images, 3, H, W] and pixel_attention_mask): LongTensor [B, T + n] = the prompt followed by the new tokens, a finished row
        filled with pad_token_id, stopping when every row has emitted an EOS (int or list) or at the length limit.  B > 1 needs left
        padding; a padded text-only batch is fine (positions come from the mask).  Any other generation argument raises
        NotImplementedError naming it.  Works in train() and eval() mode; touches no gradient buffer."""
        from . import generation as _generation
        _generation._refuse_unsupported(rest)          # generation.generate's own keywords beyond this signature are not public here
        return _generation.generate(self, input_ids, pixel_values=pixel_values, pixel_attention_mask=pixel_attention_mask,
                                    attention_mask=attention_mask, max_new_tokens=max_new_tokens, max_length=max_length,
                                    eos_token_id=eos_token_id, pad_token_id=pad_token_id, streamer=streamer, do_sample=do_sample,
                                    num_beams=num_beams, **rest)

    def set_precision(self, precision):
        if precision != "bf16":
            raise NotImplementedError(f"set_precision({precision!r}): the fp8 decoder variant is not wired up on the Idefics3 path yet; "
                                      "it runs the bf16 kernels")
        return super().set_precision(precision)


class Idefics3Engine(Idefics2Engine):
    """Host side of the Idefics3 step.  Image preparation, the tower (`vision_forward`, `prefetch_vision`), the merger plan, the decoder,
    the head and the gradient plumbing are the Idefics2 engine's; the connector and the choice of cross-entropy rows are Idefics3's."""

    def __init__(self, model):
        super().__init__(model)
        self.ignore_index = -100            # CrossEntropyLoss() default (:1197), NOT image_token_id

    def step(self, input_ids, attention_mask, labels, pixel_values, pixel_attention_mask=None, segment_ids=None, **kw):
        """Packed rows are refused: the reference has no sample packing for this family, and `select_ce_rows` below builds the
        cross-entropy lists from attention_mask and labels alone -- it would drop what `pack_segments` writes into them so that
        nothing is predicted across a sample boundary."""
        if segment_ids is not None:
            raise NotImplementedError("packed rows (segment_ids / a 4-D block-diagonal attention_mask) are not implemented on the Idefics3 "
                                      "path: one sample per row")
        return super().step(input_ids, attention_mask, labels, pixel_values, pixel_attention_mask, **kw)

    def vision_forward(self, pix, pos_ids, kmask):
        """The reference takes height = width = int(seq ** 0.5) in the pixel shuffle (:652-655) and would mis-shape a non-square
        patch grid silently: refuse it before the tower runs.  The check lives HERE, not in the step, on purpose: this is the one
        function both routes to the tower pass through -- the step itself and `prefetch_vision`, which runs a future batch's tower
        on another stream -- and the only place where the padded pixel shape is still known (downstream only N is)."""
        P, s = self.cfg.vision_config.patch_size, self.cfg.scale_factor
        Hh, Ww = pix.shape[2], pix.shape[3]
        if Hh != Ww:
            raise ValueError(f"pixel_values padded to {Hh} x {Ww}: the Idefics3 pixel shuffle needs a square patch grid")
        if (Hh // P) % s:
            raise ValueError(f"{Hh // P} patches per side are not divisible by scale_factor = {s}")
        return super().vision_forward(pix, pos_ids, kmask)

    def connector_forward(self, feats, I, N, km_all, record=None):
        """feats [I*N, d_v] -> image hidden states [I*N/s^2, d]: pixel shuffle + one linear.  The patch mask is not used (:662-665)."""
        K = I2.K
        H = int(round(N ** 0.5))
        if H * H != N:
            raise ValueError(f"{N} patches per image do not form a square grid")
        shuffled = K.pixel_shuffle(feats, I, H, self.cfg.scale_factor)
        return K.gemm_nt(shuffled, self.m.conn["proj"]), dict(shuffled=shuffled)

    def connector_backward(self, dimg, c, acc):
        g = self.m.grads_conn["proj"]
        if g is not None:
            I2.K.linear_dw(dimg, c["shuffled"], g, acc)          # the tower below is frozen: nothing flows further back

    def select_ce_rows(self, plan, ids_cpu, am_cpu, labels, dev):
        """The loss rule of :1186-1198 as compact cross-entropy lists: token t >= 1 of sample b is a target iff attention_mask[b, t] != 0
        and labels[b, t] != -100 -- <image> tokens and labels equal to image_token_id included (the merger plan's own lists leave
        every <image> token out, which is the Idefics2 rule) -- predicted from merged row b*T + t - 1 (one slot per token: L = T).
        Taken on the host copy of the batch, padded to a multiple of 8 rows with (row -1, target -100) entries.  A counted label
        outside [0, vocab_size) raises IndexError, as torch's CrossEntropyLoss does."""
        if labels is None:
            return
        lab = BB.to_host(labels)
        V = self.cfg.text_config.vocab_size
        valid = (am_cpu != 0) & (lab != -100)
        valid[:, 0] = False
        bad = valid & ((lab < 0) | (lab >= V))
        if bool(bad.any()):
            raise IndexError(f"{int(bad.sum())} label(s) are outside [0, vocab_size = {V}) "
                             f"(torch.nn.CrossEntropyLoss: 'Target out of bounds')")
        sel = torch.nonzero(valid.reshape(-1)).reshape(-1)
        n = int(sel.numel())
        pad = 8 if n == 0 else (-n) % 8
        row = torch.cat([(sel - 1).to(torch.int32), torch.full((pad,), -1, dtype=torch.int32)])
        tgt = torch.cat([lab.reshape(-1)[sel].to(torch.int32), torch.full((pad,), -100, dtype=torch.int32)])
        plan.ce_row, plan.ce_tgt = row.to(dev, non_blocking=True).contiguous(), tgt.to(dev, non_blocking=True).contiguous()
