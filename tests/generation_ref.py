"""Test infrastructure: fp32 torch-CPU restatements of the four decode operators of mantis_amd/hip_ops.py (linear_skinny / linear_decode,
kv_cache_write, attn_decode, argmax_rows) on top of the oracle's operator restatement (oracle/ops_ref.py), with the same signatures, so
that
  * tests/test_generation_gpu.py can compare each gfx950 kernel with its restatement on identical inputs, and
  * tests/test_generation.py (CPU) can drive the product's host logic (mantis_amd/generation.py, decoder.layer_decode) with `backend()`
    in place of the HIP operators.
`fp32_model` re-homes a product model's arena in fp32 so the CPU run can be held to fp32 accuracy against the reference's fp32 record."""
import types

import torch

from oracle import ops_ref


def linear_skinny(x, w, bias=None, residual=None, n_valid=None, ldc=None, out=None):
    assert 1 <= x.shape[0] <= 16
    return ops_ref.gemm_nt(x, w, bias=bias, residual=residual, n_valid=n_valid, ldc=ldc, out=out)


def linear_decode(x, w, bias=None, residual=None, n_valid=None, ldc=None):
    return ops_ref.gemm_nt(x, w, bias=bias, residual=residual, n_valid=n_valid, ldc=ldc)


def kv_cache_alloc(B, Hkv, S_max, hd, device, dtype=torch.bfloat16):
    return torch.zeros((B, Hkv, S_max, hd), dtype=dtype, device=device), torch.zeros((B, Hkv, S_max, hd), dtype=dtype, device=device)


def kv_cache_write(qkv, k_cache, v_cache, slot, cos, sin, rows_per_sample, H, Hkv, hd):
    B, _, S_max, _ = k_cache.shape
    R = qkv.shape[0]
    k = qkv[:, H * hd: (H + Hkv) * hd].clone()
    if cos is not None:
        qk = qkv[:, : (H + Hkv) * hd].clone()
        ops_ref.rope_apply_(qk, cos, sin, H + Hkv, hd)
        qkv[:, : H * hd] = qk[:, : H * hd]            # q in place; the buffer's k columns stay unrotated
        k = qk[:, H * hd:]
    v = qkv[:, (H + Hkv) * hd: (H + 2 * Hkv) * hd]
    for r in range(R):
        s = int(slot[r])
        if 0 <= s < S_max:
            b = r // rows_per_sample
            k_cache[b, :, s] = k[r].reshape(Hkv, hd).to(k_cache.dtype)
            v_cache[b, :, s] = v[r].reshape(Hkv, hd).to(v_cache.dtype)


def attn_decode_splits(B, Hkv, S_max):
    return 1, (S_max + 63) // 64 * 64


def attn_decode_workspace(B, H, Hkv, hd, S_max, device):
    return None


def attn_decode(q, k_cache, v_cache, kmask, n_keys, H, Hkv, hd, scale, ws=None):
    B, _, S_max, _ = k_cache.shape
    G = H // Hkv
    qh = q[:, : H * hd].float().reshape(B, Hkv, G, hd)
    s = torch.einsum("bkgd,bksd->bkgs", qh, k_cache.float()) * scale
    live = torch.arange(S_max)[None, :] < n_keys.long()[:, None]
    if kmask is not None:
        live = live & (kmask != 0)
    s = s.masked_fill(~live[:, None, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1).nan_to_num(0.0)          # a row without a live key: zeros
    o = torch.einsum("bkgs,bksd->bkgd", p, v_cache.float())
    return o.reshape(B, H * hd).to(q.dtype)


def argmax_rows(logits, V):
    return logits[:, :V].float().argmax(dim=-1)         # torch: the first maximal index


def backend(fp32_tables=False):
    """The oracle's operator restatement + the decode operators, as one backend object for `mantis_amd.engine.K`.
    fp32_tables: RoPE tables in fp32 (a run held to fp32 accuracy; the product's tables are bf16 like the reference's bf16 graph)."""
    ns = types.SimpleNamespace(**{k: getattr(ops_ref, k) for k in dir(ops_ref) if not k.startswith("__")})
    for f in (linear_skinny, linear_decode, kv_cache_write, attn_decode_splits, attn_decode_workspace, attn_decode, argmax_rows):
        setattr(ns, f.__name__, f)
    ns.kv_cache_alloc = kv_cache_alloc
    if fp32_tables:
        def rope_table(position_ids, inv_freq):
            f = position_ids.reshape(-1, 1).float() * inv_freq.float()[None]
            return f.cos(), f.sin()
        ns.rope_table = rope_table

        def im2col(pixels, patch, kp):
            cols = torch.nn.functional.unfold(pixels.float(), kernel_size=patch, stride=patch)       # [I, C*P*P, N]
            out = torch.zeros((pixels.shape[0] * cols.shape[2], kp), dtype=torch.float32)
            out[:, : cols.shape[1]] = cols.transpose(1, 2).reshape(-1, cols.shape[1])
            return out
        ns.im2col = im2col
        ns.kv_cache_alloc = lambda B, Hkv, S_max, hd, device: kv_cache_alloc(B, Hkv, S_max, hd, device, dtype=torch.float32)
    return ns


def fp32_model(model, state_dict):
    """Re-home a (CPU) product model's parameter arena in fp32 and load `state_dict` unrounded: the host logic under test is unchanged,
    the arithmetic of the oracle backend then follows the storage dtype."""
    arena = torch.zeros(model.arena.numel(), dtype=torch.float32)
    model.arena = arena
    for name, shape in model._specs:
        n = 1
        for s in shape:
            n *= s
        model._param(name).data = arena[model._offs[name]: model._offs[name] + n].view(shape)
    model._build_views()
    model.load_reference_state_dict(state_dict)
    return model


@torch.no_grad()
def teacher_forced_logits(model, input_ids, attention_mask, pixel_values, tokens):
    """Drive the product's prefill / decode_step with the given tokens [B, n] (instead of its own argmax) -> fp32 logits [n, B, V] of every
    step, the way a test obtains per-step logits without a hook inside `generate`."""
    from mantis_amd import generation as Gn
    V = model.config.text_config.vocab_size
    n = tokens.shape[1]
    cache, logits = Gn.prefill(model, input_ids, attention_mask, pixel_values, n)
    out = [logits[:, :V].float().cpu()]
    for i in range(n - 1):
        out.append(Gn.decode_step(model, cache, tokens[:, i].to(model.device))[:, :V].float().cpu())
    return torch.stack(out)
