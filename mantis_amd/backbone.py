"""Host-side descriptions shared by the model classes (modeling_llava.py, modeling_idefics2.py / modeling_idefics3.py, modeling_qwen2_vl.py)
and their engines: the (name, shape) specs, arena views and gradient buckets of a decoder layer; the specs, views and encoder block loop
of the SigLIP / CLIP tower; the output base class; the prefetch slots of `prefetch_vision`.  Nothing here is on the launch path except
`vit_encoder`, which -- like decoder.py -- takes the operator backend `K` from its caller: this module binds no backend of its own (the
host-logic tests replace `engine.K` / `modeling_idefics2.K` / `modeling_qwen2_vl.K`, and that must reach every launch).  Pure Python:
importable without the HIP library."""
import dataclasses

import torch


# ---------------------------------------------------------------------- decoder layer (Llama-3 / Mistral / Qwen2)
def decoder_layer_specs(prefix, tc, qkv_bias=False):
    """(name, shape) of one text layer in arena order.  Order inside a layer = REVERSE of backward completion, so that the three DP
    sub-buckets of a layer are contiguous slices: [norms | q k v (| q k v biases: Qwen2) | o] (done last), [gate up], [down] (done
    first) -- see decoder_buckets()."""
    d, it = tc.hidden_size, tc.intermediate_size
    H, Hkv, hd = tc.num_attention_heads, tc.num_key_value_heads, tc.head_dim
    p = prefix
    s = [(p + "input_layernorm.weight", (d,)), (p + "post_attention_layernorm.weight", (d,)),
         (p + "self_attn.q_proj.weight", (H * hd, d)), (p + "self_attn.k_proj.weight", (Hkv * hd, d)),
         (p + "self_attn.v_proj.weight", (Hkv * hd, d))]
    if qkv_bias:
        s += [(p + "self_attn.q_proj.bias", (H * hd,)), (p + "self_attn.k_proj.bias", (Hkv * hd,)), (p + "self_attn.v_proj.bias", (Hkv * hd,))]
    return s + [(p + "self_attn.o_proj.weight", (d, H * hd)),
                (p + "mlp.gate_proj.weight", (it, d)), (p + "mlp.up_proj.weight", (it, d)), (p + "mlp.down_proj.weight", (d, it))]


def decoder_layer_views(prefix, tc, get, flat, qkv_bias=False):
    """dict(qkv, o, gu, down, ln1, ln2[, qkv_b]) of one text layer, as decoder.py reads it: q|k|v and gate|up as zero-copy views over the
    adjacent parameters.  (get, flat) = (parameter data, ArenaModule._flat) for the parameters, (gradient view or None,
    ArenaModule._gflat) for the gradients -- there a frozen tensor or fused group is None."""
    d, it = tc.hidden_size, tc.intermediate_size
    nqkv = (tc.num_attention_heads + 2 * tc.num_key_value_heads) * tc.head_dim
    p = prefix
    v = dict(qkv=flat(p + "self_attn.q_proj.weight", p + "self_attn.v_proj.weight", nqkv, d), o=get(p + "self_attn.o_proj.weight"),
             gu=flat(p + "mlp.gate_proj.weight", p + "mlp.up_proj.weight", 2 * it, d), down=get(p + "mlp.down_proj.weight"),
             ln1=get(p + "input_layernorm.weight"), ln2=get(p + "post_attention_layernorm.weight"))
    if qkv_bias:
        b = flat(p + "self_attn.q_proj.bias", p + "self_attn.v_proj.bias", 1, nqkv)
        v["qkv_b"] = None if b is None else b.view(-1)
    return v


def decoder_buckets(span, layer_prefix, n_layers):
    """The per-layer entries of `grad_buckets()`: three sub-buckets per decoder layer, fired (n-1 .. 0) as their last dW lands --
    ('layer', i, 'down') after dW(down_proj), ('layer', i, 'gu') after dW(gate|up), ('layer', i, 'attn') = norms + q|k|v|o at the end of
    the layer -- so the first byte of a layer moves after its first GEMM, not after its last.  span = ArenaModule._bucket_span."""
    out = {}
    for i in range(n_layers):
        p = f"{layer_prefix}{i}."
        out[("layer", i, "down")] = span(lambda n: n == p + "mlp.down_proj.weight")
        out[("layer", i, "gu")] = span(lambda n: n in (p + "mlp.gate_proj.weight", p + "mlp.up_proj.weight"))
        out[("layer", i, "attn")] = span(lambda n: n.startswith(p) and ".mlp." not in n)
    return out


# ---------------------------------------------------------------------- SigLIP / CLIP tower (frozen, forward only)
def vit_layer_specs(prefix, vc):
    """(name, shape) of one encoder layer of the SigLIP / CLIP tower in arena order"""
    dv, iv = vc.hidden_size, vc.intermediate_size
    p = prefix
    return [(p + "self_attn.q_proj.weight", (dv, dv)), (p + "self_attn.k_proj.weight", (dv, dv)), (p + "self_attn.v_proj.weight", (dv, dv)),
            (p + "self_attn.q_proj.bias", (dv,)), (p + "self_attn.k_proj.bias", (dv,)), (p + "self_attn.v_proj.bias", (dv,)),
            (p + "self_attn.out_proj.weight", (dv, dv)), (p + "self_attn.out_proj.bias", (dv,)),
            (p + "layer_norm1.weight", (dv,)), (p + "layer_norm1.bias", (dv,)), (p + "layer_norm2.weight", (dv,)), (p + "layer_norm2.bias", (dv,)),
            (p + "mlp.fc1.weight", (iv, dv)), (p + "mlp.fc1.bias", (iv,)), (p + "mlp.fc2.weight", (dv, iv)), (p + "mlp.fc2.bias", (dv,))]


def vit_layer_views(module, prefix, vc):
    """The views of one encoder layer as vit_encoder reads them (q|k|v weights and biases fused); module = the ArenaModule"""
    dv = vc.hidden_size
    p = prefix
    g = lambda n: module._param(n).data
    return dict(qkv_w=module._flat(p + "self_attn.q_proj.weight", p + "self_attn.v_proj.weight", 3 * dv, dv),
                qkv_b=module._flat(p + "self_attn.q_proj.bias", p + "self_attn.v_proj.bias", 1, 3 * dv).view(-1),
                out_w=g(p + "self_attn.out_proj.weight"), out_b=g(p + "self_attn.out_proj.bias"),
                ln1_w=g(p + "layer_norm1.weight"), ln1_b=g(p + "layer_norm1.bias"), ln2_w=g(p + "layer_norm2.weight"), ln2_b=g(p + "layer_norm2.bias"),
                fc1_w=g(p + "mlp.fc1.weight"), fc1_b=g(p + "mlp.fc1.bias"), fc2_w=g(p + "mlp.fc2.weight"), fc2_b=g(p + "mlp.fc2.bias"))


def patch_w_padded(module, name, vc):
    """-> (kp, closure): the patch-embedding weight `name` as the [d_v, kp] GEMM operand of the im2col rows, kp = C*P*P rounded up to 8
    elements (16-byte rows); the closure returns the parameter itself where no padding is needed, else a zero-padded copy made per call."""
    dv = vc.hidden_size
    kraw = vc.num_channels * vc.patch_size * vc.patch_size
    kp = (kraw + 7) // 8 * 8

    def padded():
        w = module._param(name).data.view(dv, kraw)
        if kp == kraw:
            return w
        out = torch.zeros((dv, kp), dtype=w.dtype, device=w.device)
        out[:, :kraw] = w
        return out
    return kp, padded


def vit_encoder(K, layers, x, I, n_tokens, vc, kmask):
    """The pre-LN encoder blocks `layers` (vit_layer_views) over x [I * n_tokens, d_v]: LayerNorm, q|k|v, attention (kmask: int32 [I,
    n_tokens] key mask or None), out-proj + residual, LayerNorm, fc1 + activation, fc2 + residual -- seven launches per block."""
    eps = vc.layer_norm_eps
    nh = vc.num_attention_heads
    hd = vc.hidden_size // nh
    for lw in layers:
        y = K.layernorm_fwd(x, lw["ln1_w"], lw["ln1_b"], eps)
        qkv = K.gemm_nt(y, lw["qkv_w"], bias=lw["qkv_b"])
        o, _ = K.attn_fwd(qkv, I, n_tokens, nh, nh, hd, kmask, hd ** -0.5, False, want_lse=False)
        x = K.gemm_nt(o, lw["out_w"], bias=lw["out_b"], residual=x)
        y = K.layernorm_fwd(x, lw["ln2_w"], lw["ln2_b"], eps)
        hmid = K.gemm_nt(y, lw["fc1_w"], bias=lw["fc1_b"], act=vc.hidden_act)
        x = K.gemm_nt(hmid, lw["fc2_w"], bias=lw["fc2_b"], residual=x)
    return x


# ---------------------------------------------------------------------- model outputs and engine bookkeeping
class ModelOutput:
    """Base of the output dataclasses: out["loss"] reads a field, out[i] indexes the fields that are not None, in order (what HF's
    ModelOutput does for the reference's classes)."""

    def __getitem__(self, k):
        if isinstance(k, str):
            return getattr(self, k)
        return tuple(v for v in (getattr(self, f.name) for f in dataclasses.fields(self)) if v is not None)[k]


def to_host(t):
    """The host copy of a batch tensor that the engines take their host-side decisions on (t itself if it already lives there)"""
    return t.detach().to("cpu") if t.device.type != "cpu" else t


class PrefetchSlots(dict):
    """What `prefetch_vision` computed ahead, id(pixel_values object) -> (that object, *results).  A step takes the entry of the SAME
    pixel_values object; at most two batches are in flight (with the trainer's early prefetch the tower of batch i+1 is enqueued before
    step i has picked up its own), so older entries are dropped: a prefetched batch that never arrives must not pile up."""

    def put(self, pixel_values, *results):
        self[id(pixel_values)] = (pixel_values, *results)
        while len(self) > 2:
            self.pop(next(iter(self)))

    def take(self, pixel_values):
        """Remove and return the entry of this very object, or None"""
        pre = self.pop(id(pixel_values), None)
        return pre if pre is not None and pre[0] is pixel_values else None
