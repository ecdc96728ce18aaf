"""Greedy generation with a KV cache: the host side of `LlavaForConditionalGeneration.generate` and
`Idefics3ForConditionalGeneration.generate`.  Family-agnostic: the operator backend (`engine.K`), the family's prefill inputs
(`engine.prefill_inputs`) and whether its prefill positions follow the attention mask come from the model's engine.

Reference control flow being reproduced: HF GenerationMixin's greedy search driving
/root/reference/mantis/models/mllava/modeling_llava.py:478-508 (the cached branch of forward: one new token, `position_ids =
attention_mask.sum(1) - 1`) and :551-602 (prepare_inputs_for_generation), as `chat_mllava` / `chat_mllava_stream`
(/root/reference/mantis/models/mllava/utils.py:10-97) call it; on the Idefics3 path mantis/mllm_tools/idefics3_eval.py:64 over the
reference's prepare_inputs_for_generation (idefics3 modeling_idefics3.py:1243-1249: position_ids = attention_mask.cumsum(-1) - 1).

  prefill      = the engine's evaluation forward (tower, projector, pack plan, decoder without gradients) that also hands every layer's
                 rotated K and its V to the cache, then final norm + lm_head on the LAST LIVE ROW of each sample only.
  decode_step  = embedding row -> decoder.decoder_decode (weight-streaming linears, cache append with RoPE, split-key decode attention)
                 -> final norm, lm_head, argmax.  One new token per sample.

Cache slot s of a sample holds position s of the MERGED prefill sequence (image rows and padding slots included, masked by `kmask`), the
new tokens follow at slots L, L + 1, ...; a token's RoPE position is the number of live keys before it.  Everything the step loop touches is
preallocated in KVCache.  The token of a step is chosen, written and tested against the EOS list by ONE kernel (`K.greedy_select`) that keeps
finished-ness on the device; the loop reads it back every `EOS_CHECK_EVERY` steps when an EOS is set and never otherwise (see `generate`)."""
import torch

from . import decoder as D

# With an EOS set the loop reads the per-row finish steps back every this many steps (and at the end).  1 = after every token.  Larger
# values were not measured on an MI355X yet (tools/decode_bench.py --family idefics3 prints the table; profiles/generation_decode.md),
# so the default stays at the behaviour the loop had before.
EOS_CHECK_EVERY = 1


class KVCache:
    """Per-layer K / V preallocated for the merged prompt + max_new_tokens, the key mask and the per-sample counters (plain tensors)."""

    def __init__(self, K, tc, B, L, max_new_tokens, device):
        self.B, self.L, self.S_max = B, L, L + max_new_tokens
        H, Hkv, hd = tc.num_attention_heads, tc.num_key_value_heads, tc.head_dim
        self.layers = [K.kv_cache_alloc(B, Hkv, self.S_max, hd, device) for _ in range(tc.num_hidden_layers)]
        self.kmask = torch.zeros((B, self.S_max), dtype=torch.int32, device=device)       # 1 = live key
        self.n_keys = torch.zeros((B,), dtype=torch.int32, device=device)                  # cache slots in use (the same for every sample)
        self.slot = torch.zeros((B,), dtype=torch.int32, device=device)                    # where the next token goes
        self.position = torch.zeros((B,), dtype=torch.int64, device=device)                # its RoPE position = live keys so far
        self.prefill_slot = torch.arange(L, dtype=torch.int32, device=device).repeat(B)
        self.ws = K.attn_decode_workspace(B, H, Hkv, hd, self.S_max, device)
        self.steps = 0

    def advance(self):
        """after a decode step: the token just written is a live key; the next one goes one slot further"""
        self.n_keys += 1
        self.slot += 1
        self.position += 1
        self.steps += 1


def _last_live_rows(plan, B, L):
    """row index (into [B*L]) of the last live position of every sample of the merged sequence"""
    am = plan.attention_mask != 0
    idx = torch.arange(L, device=am.device)[None].expand(B, L)
    last = torch.where(am, idx, torch.full_like(idx, -1)).max(dim=1).values
    return (last + torch.arange(B, device=am.device) * L).to(torch.int32)


def prefill(model, input_ids, attention_mask, pixel_values, max_new_tokens, pixel_attention_mask=None):
    """-> (cache, bf16 logits [B, pad8(V)] of the last live row of every sample)"""
    K = model.engine.K
    tc = model.config.text_config
    H, Hkv, hd = tc.num_attention_heads, tc.num_key_value_heads, tc.head_dim
    B = input_ids.shape[0]
    box = {}

    def sink(i, qkv):
        cache = box.get("cache")
        if cache is None:          # the merged length is known once the first layer reports
            L = qkv.shape[0] // B
            cache = box["cache"] = KVCache(K, tc, B, L, max_new_tokens, qkv.device)
        K.kv_cache_write(qkv, cache.layers[i][0], cache.layers[i][1], cache.prefill_slot, None, None, cache.L, H, Hkv, hd)

    out = model.engine.step(input_ids, attention_mask, None, pixel_values, compute_grads=False, kv_sink=sink,
                            **model.engine.prefill_inputs(attention_mask, pixel_attention_mask))
    cache, plan, L = box["cache"], out["plan"], out["L"]
    cache.kmask[:, :L] = (plan.attention_mask != 0).to(torch.int32)
    cache.kmask[:, L:] = 1
    n_live = (plan.attention_mask != 0).sum(1)
    cache.position.copy_(n_live)
    cache.n_keys.fill_(L + 1)          # a decode step attends the prefill slots and the token it has just appended
    cache.slot.fill_(L)
    x = K.gather_rows(out["hidden"], _last_live_rows(plan, B, L))
    return cache, D.head_rows(K, model.lm, tc, x)


def decode_step(model, cache, tokens):
    """tokens int64 [B] (the tokens chosen by the previous step) -> bf16 logits [B, pad8(V)] of the next position; appends to the cache"""
    K = model.engine.K
    tc = model.config.text_config
    if cache.steps >= cache.S_max - cache.L:
        raise RuntimeError("KV cache is full: it was allocated for max_new_tokens decode steps")
    x = K.gather_rows(model.lm["embed"], tokens.to(torch.int32))
    x = D.decoder_decode(K, model.lm, tc, x, cache.layers, cache.slot, cache.position, cache.kmask, cache.n_keys, ws=cache.ws)
    cache.advance()
    return D.head_rows(K, model.lm, tc, x)


_UNSUPPORTED_DEFAULTS = dict(do_sample=False, num_beams=1, num_beam_groups=1, num_return_sequences=1, temperature=None, top_k=None,
                             top_p=None, repetition_penalty=None, no_repeat_ngram_size=None, length_penalty=None, penalty_alpha=None,
                             logits_processor=None, stopping_criteria=None, prefix_allowed_tokens_fn=None, assistant_model=None,
                             output_scores=None, output_logits=None, output_attentions=None, output_hidden_states=None,
                             return_dict_in_generate=None, min_new_tokens=None, min_length=None, bad_words_ids=None,
                             past_key_values=None, inputs_embeds=None, generation_config=None)
_NEUTRAL = {"temperature": (None, 1.0), "top_k": (None, 0, 50), "top_p": (None, 1.0), "repetition_penalty": (None, 1.0),
            "no_repeat_ngram_size": (None, 0), "length_penalty": (None, 1.0), "min_new_tokens": (None, 0), "min_length": (None, 0),
            "output_scores": (None, False), "output_logits": (None, False), "output_attentions": (None, False),
            "output_hidden_states": (None, False), "return_dict_in_generate": (None, False), "penalty_alpha": (None, 0.0)}


def _refuse_unsupported(kwargs):
    for k, v in kwargs.items():
        if k == "use_cache":                         # the cache is how this path works; True / False / None give the same tokens
            continue
        if k not in _UNSUPPORTED_DEFAULTS:
            raise NotImplementedError(f"generate(): argument `{k}` is not supported (greedy decoding with a KV cache only)")
        ok = _NEUTRAL.get(k, (_UNSUPPORTED_DEFAULTS[k],))
        if not any(v is o or (o is not None and v is not None and not isinstance(v, (list, tuple, dict)) and v == o) for o in ok):
            raise NotImplementedError(f"generate(): `{k}={v!r}` is not supported (greedy decoding with a KV cache only)")


def _eos_list(eos_token_id):
    if eos_token_id is None:
        return []
    if isinstance(eos_token_id, torch.Tensor):
        eos_token_id = eos_token_id.reshape(-1).tolist()
    if isinstance(eos_token_id, (list, tuple)):
        return [int(e) for e in eos_token_id]
    return [int(eos_token_id)]


def select_composition(K, logits, V, eos_ids, pad_id, unfinished, finish_step, out, step, next_tokens):
    """One step of greedy search's token choice and bookkeeping as a composition of small operators: THE DEFINITION `K.greedy_select` is
    tested against, and what the loop runs on a backend without that operator.  Same arguments and effects as hip_ops.greedy_select."""
    nxt = K.argmax_rows(logits, V)
    if eos_ids is not None and eos_ids.numel():
        live = unfinished != 0
        nxt = torch.where(live, nxt, torch.full_like(nxt, int(pad_id)))
        hit = live & torch.isin(nxt, eos_ids)
        finish_step.copy_(torch.where(hit, torch.full_like(finish_step, step), finish_step))
        unfinished.copy_((live & ~hit).to(unfinished.dtype))
    out[:, step] = nxt
    next_tokens.copy_(nxt)
    return next_tokens


@torch.no_grad()
def generate(model, input_ids, pixel_values=None, attention_mask=None, max_new_tokens=None, max_length=None, eos_token_id=None,
             pad_token_id=None, streamer=None, pixel_attention_mask=None, eos_check_every=None, **rest):
    """HF greedy search (GenerationMixin._sample with do_sample=False) on the KV-cache decode path -> LongTensor [B, T + n].
    Finished-ness lives on the device (int32 `unfinished`, `finish_step` [B], updated by the select kernel).  With an EOS set the host reads
    `finish_step` back every `eos_check_every` steps (default EOS_CHECK_EVERY; 1 with a streamer, whose stream must end where HF's does) and
    at the length limit; once every row is found finished the result is cut to max(finish_step) + 1 new tokens, so the returned tensor is
    HF's whatever the interval, and at most eos_check_every - 1 decode steps run after the last row finished.  Without an EOS nothing is
    read back before the end."""
    _refuse_unsupported(rest)
    cfg = model.config
    eng = model.engine
    if eng.w8 is not None:
        raise NotImplementedError("generate() runs the bf16 decoder; call set_precision('bf16') first")
    if input_ids is None or input_ids.dim() != 2:
        raise ValueError("generate() needs input_ids [B, T]")
    B, T = input_ids.shape
    if attention_mask is None:
        attention_mask = torch.ones_like(input_ids)
    am_cpu = attention_mask.detach().to("cpu")
    if B > 1 and bool((am_cpu[:, -1] == 0).any()):
        raise ValueError("generate() with B > 1 needs LEFT padding: a right-padded batch of unequal lengths continues from padding "
                         "(HF's result for it is not meaningful); pad on the left (tokenizer.padding_side = 'left')")
    if bool((am_cpu[:, -1] == 0).any()):
        raise ValueError("generate(): the last position of the prompt is masked out")
    if not eng.prefill_positions_follow_mask and pixel_values is None and B > 1 and bool((am_cpu == 0).any()):
        raise NotImplementedError("generate(): a padded TEXT-ONLY batch is not supported (without pixel_values the prefill's position ids "
                                  "ignore the padding, as the reference's forward does); pass the prompts one by one")
    if max_new_tokens is None:
        if max_length is None:
            max_length = getattr(cfg, "max_length", None) or 20          # HF GenerationConfig's default
        max_new_tokens = int(max_length) - T                               # (HF: a given max_new_tokens takes precedence over max_length)
    if max_new_tokens < 1:
        raise ValueError(f"generate(): nothing to generate (prompt length {T}, max_new_tokens {max_new_tokens})")
    eos = _eos_list(eos_token_id)
    if pad_token_id is None:
        pad_token_id = cfg.pad_token_id if cfg.pad_token_id is not None else (eos[0] if eos else None)
    if eos and pad_token_id is None:
        raise ValueError("generate(): an eos_token_id needs a pad_token_id to fill finished rows with")
    every = EOS_CHECK_EVERY if eos_check_every is None else int(eos_check_every)
    if every < 1:
        raise ValueError(f"generate(): eos_check_every = {every} (the read-back interval in steps, >= 1)")
    if streamer is not None:
        every = 1
    K = eng.K
    dev = model.device
    V = cfg.text_config.vocab_size
    select = getattr(K, "greedy_select", None)
    if select is None:
        select = lambda *a: select_composition(K, *a)
    if streamer is not None:
        streamer.put(input_ids.cpu())                                      # HF: the prompt first
    cache, logits = prefill(model, input_ids, attention_mask, pixel_values, max_new_tokens, pixel_attention_mask=pixel_attention_mask)
    eos_dev = torch.tensor(eos, dtype=torch.int64, device=dev) if eos else None
    unfinished = torch.ones((B,), dtype=torch.int32, device=dev)
    finish_step = torch.full((B,), -1, dtype=torch.int32, device=dev)
    nxt = torch.zeros((B,), dtype=torch.int64, device=dev)
    out = torch.full((B, max_new_tokens), -1 if pad_token_id is None else int(pad_token_id), dtype=torch.int64, device=dev)
    n = 0
    for step in range(max_new_tokens):
        select(logits, V, eos_dev, pad_token_id, unfinished, finish_step, out, step, nxt)
        n = step + 1
        if streamer is not None:
            streamer.put(nxt.cpu())
        if eos and (n % every == 0 or n == max_new_tokens):
            done = finish_step.cpu()                                       # the one host read-back, every `every` steps
            if bool((done >= 0).all()):
                n = int(done.max()) + 1
                break
        if n < max_new_tokens:
            logits = decode_step(model, cache, nxt)
    if streamer is not None:
        streamer.end()
    return torch.cat([input_ids.to(dev), out[:, :n]], dim=1)
