"""GPU: the decode kernels of csrc/decode.hip against fp32 torch on the same bf16-rounded inputs (SURVEY 8c's bars: cosine >= 0.999,
rel-L2 <= 2e-2, plus bitwise repeatability), and `LlavaForConditionalGeneration.generate` against the reference's record
(tests/golden/generation/llava_generate_*.npz: teacher-forced logits within eps = 1.5 x the reference's own bf16 deviation, free-running tokens
exactly) and against the product's own cache-free forward at full width."""
import glob
import os

import numpy as np
import pytest
import torch

from tests import generation_ref as GR
from tests import helpers as Hh

pytestmark = pytest.mark.gpu
DEV = "cuda"
COS, REL = 0.999, 2e-2
FIXTURES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(Hh.G, "generation", "llava_generate_*.npz")))


def _k():
    from mantis_amd import hip_ops
    return hip_ops


def _rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(DEV)


def _bars(got, ref, what):
    a, b = got.float().reshape(-1).double(), ref.float().reshape(-1).double()
    cos = float(a @ b / (a.norm() * b.norm() + 1e-30))
    rel = float((a - b).norm() / (b.norm() + 1e-30))
    print(f"{what}: cosine {cos:.6f} rel-L2 {rel:.5f}")
    assert cos >= COS and rel <= REL, (what, cos, rel)


# ------------------------------------------------------------------------------------------------------------------ skinny linear
SHAPES_8B = [(6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336), (128258, 4096)]
SHAPES_TINY = [(128, 64), (64, 64), (352, 64), (64, 176), (300, 64)]


@pytest.mark.parametrize("N,Kd", SHAPES_8B + SHAPES_TINY)
def test_linear_skinny(N, Kd):
    K = _k()
    Np = K.pad8(N)
    w = _rnd(Np, Kd, seed=N + Kd, scale=0.05)
    bias = _rnd(Np, seed=1, scale=0.5)
    wf = w[:N].float()
    for M in (1, 2, 3, 8, 16):
        x = _rnd(M, Kd, seed=M)
        res = _rnd(M, Np, seed=M + 100)
        ref = x.float() @ wf.t()
        y = K.linear_skinny(x, w, n_valid=N, ldc=Np)
        _bars(y[:, :N], ref, f"skinny {M}x{N}x{Kd}")
        assert torch.equal(y[:, :N], K.linear_skinny(x, w, n_valid=N, ldc=Np)[:, :N]), "not bitwise repeatable"
        yb = K.linear_skinny(x, w, bias=bias, residual=res, n_valid=N, ldc=Np)
        refb = (ref + bias[:N].float()).to(torch.bfloat16).float() + res[:, :N].float()
        _bars(yb[:, :N], refb, f"skinny+bias+res {M}x{N}x{Kd}")
        assert torch.equal(yb[:, :N], K.linear_skinny(x, w, bias=bias, residual=res, n_valid=N, ldc=Np)[:, :N])
        g = K.gemm_nt(x, w, bias=bias, residual=res, n_valid=N, ldc=Np)
        _bars(yb[:, :N], g[:, :N], f"skinny vs gemm_nt {M}x{N}x{Kd}")
    with pytest.raises(Exception):
        K.linear_skinny(_rnd(17, Kd), w)


# ------------------------------------------------------------------------------------------------------------------ cache write
@pytest.mark.parametrize("hd,H,Hkv", [(16, 4, 2), (64, 7, 1), (128, 32, 8)])
def test_kv_cache_write_copy_and_rotate(hd, H, Hkv):
    K = _k()
    B, L, S_max = 2, 37, 50
    qkv = _rnd(B * L, (H + 2 * Hkv) * hd, seed=hd)
    kc, vc = K.kv_cache_alloc(B, Hkv, S_max, hd, DEV)
    slot = torch.arange(L, dtype=torch.int32, device=DEV).repeat(B)
    keep = qkv.clone()
    K.kv_cache_write(qkv, kc, vc, slot, None, None, L, H, Hkv, hd)
    assert torch.equal(qkv, keep)
    kk = keep[:, H * hd: (H + Hkv) * hd].reshape(B, L, Hkv, hd).permute(0, 2, 1, 3)
    vv = keep[:, (H + Hkv) * hd:].reshape(B, L, Hkv, hd).permute(0, 2, 1, 3)
    assert torch.equal(kc[:, :, :L], kk) and torch.equal(vc[:, :, :L], vv), "copy is not exact"
    assert not kc[:, :, L:].any() and not vc[:, :, L:].any()
    # one decode row per sample: rotate q in place and k on the way == rope_apply's bits
    row = _rnd(B, (H + 2 * Hkv) * hd, seed=hd + 1)
    pos = torch.tensor([L, L - 5], dtype=torch.int64, device=DEV)
    from mantis_amd import decoder as D
    cos, sin = K.rope_table(pos, D.inv_freq(hd, 500000.0).to(DEV))
    want = K.rope_apply_(row.clone(), cos, sin, H + Hkv, hd)
    got = row.clone()
    slot1 = torch.tensor([L, L + 3], dtype=torch.int32, device=DEV)
    K.kv_cache_write(got, kc, vc, slot1, cos, sin, 1, H, Hkv, hd)
    assert torch.equal(got[:, : H * hd], want[:, : H * hd]), "q rotation differs from rope_apply"
    assert torch.equal(got[:, H * hd:], row[:, H * hd:]), "k / v columns of the buffer must stay as they were"
    for b, s in ((0, L), (1, L + 3)):
        assert torch.equal(kc[b, :, s].reshape(-1), want[b, H * hd: (H + Hkv) * hd]), "k rotation differs from rope_apply"
        assert torch.equal(vc[b, :, s].reshape(-1), row[b, (H + Hkv) * hd:])
    # a slot outside the cache is skipped, not written
    before = kc.clone()
    K.kv_cache_write(row.clone(), kc, vc, torch.tensor([-1, S_max], dtype=torch.int32, device=DEV), cos, sin, 1, H, Hkv, hd)
    assert torch.equal(kc, before)


# ------------------------------------------------------------------------------------------------------------------ decode attention
def _attn_ref(q, kc, vc, kmask, n_keys, H, Hkv, hd, scale):
    B, _, S_max, _ = kc.shape
    G = H // Hkv
    s = torch.einsum("bkgd,bksd->bkgs", q.float().reshape(B, Hkv, G, hd), kc.float()) * scale
    live = torch.arange(S_max, device=q.device)[None] < n_keys.long()[:, None]
    if kmask is not None:
        live = live & (kmask != 0)
    p = torch.softmax(s.masked_fill(~live[:, None, None], float("-inf")), dim=-1).nan_to_num(0.0)
    return torch.einsum("bkgs,bksd->bkgd", p, vc.float()).reshape(B, H * hd)


@pytest.mark.parametrize("B", [1, 2, 8])
@pytest.mark.parametrize("G", [1, 4, 7])
@pytest.mark.parametrize("hd", [16, 64, 128])
def test_attn_decode(hd, G, B):
    K = _k()
    Hkv, S_max = 2, 8192
    H = G * Hkv
    scale = hd ** -0.5
    kc, vc = _rnd(B, Hkv, S_max, hd, seed=hd + G), _rnd(B, Hkv, S_max, hd, seed=hd + G + 1)
    q = _rnd(B, H * hd, seed=B)
    splits, chunk = K.attn_decode_splits(B, Hkv, S_max)
    assert (splits, chunk) == K.attn_decode_splits(B, Hkv, S_max) and splits * chunk >= S_max
    counts = [1, 63, 64, 65, 4096, 8192]
    for i in range(1, splits):
        counts += [i * chunk - 1, i * chunk, i * chunk + 1]
    counts = [c for c in counts if 1 <= c <= S_max]
    counts += [counts[-1]] * ((-len(counts)) % B)
    g = torch.Generator().manual_seed(7)
    kmask = (torch.rand(B, S_max, generator=g) > 0.3).to(torch.int32).to(DEV)
    ws = K.attn_decode_workspace(B, H, Hkv, hd, S_max, DEV)
    worst = (1.0, 0.0)
    for i in range(0, len(counts), B):
        n_keys = torch.tensor(counts[i: i + B], dtype=torch.int32, device=DEV)
        for km in (None, kmask):
            o = K.attn_decode(q, kc, vc, km, n_keys, H, Hkv, hd, scale, ws=ws)
            ref = _attn_ref(q, kc, vc, km, n_keys, H, Hkv, hd, scale)
            a, b = o.float().reshape(-1).double(), ref.reshape(-1).double()
            if float(b.norm()) == 0.0:                      # every key of every row masked out
                assert not o.any()
                continue
            cos, rel = float(a @ b / (a.norm() * b.norm())), float((a - b).norm() / b.norm())
            worst = (min(worst[0], cos), max(worst[1], rel))
            assert cos >= COS and rel <= REL, (hd, G, B, counts[i: i + B], km is not None, cos, rel)
            assert torch.equal(o, K.attn_decode(q, kc, vc, km, n_keys, H, Hkv, hd, scale, ws=ws)), "not bitwise repeatable"
    print(f"attn_decode hd {hd} G {G} B {B} splits {splits}: worst cosine {worst[0]:.6f} rel-L2 {worst[1]:.5f} over {len(counts)} key counts")
    # one fully masked row: zeros, not NaN; the other rows unaffected
    km = kmask.clone()
    km[0] = 0
    n_keys = torch.full((B,), 4096, dtype=torch.int32, device=DEV)
    o = K.attn_decode(q, kc, vc, km, n_keys, H, Hkv, hd, scale, ws=ws)
    assert not o[0].any() and bool(torch.isfinite(o.float()).all())
    if B > 1:
        _bars(o[1:], _attn_ref(q, kc, vc, km, n_keys, H, Hkv, hd, scale)[1:], "rows beside a fully masked row")
    # the composition the parent commit offers: mantis_attn_fwd_cross with one query row per sample, on the same data
    Lk = 4096
    krow = kc[:, :, :Lk].permute(0, 2, 1, 3).reshape(B * Lk, Hkv * hd).contiguous()
    vrow = vc[:, :, :Lk].permute(0, 2, 1, 3).reshape(B * Lk, Hkv * hd).contiguous()
    kml = kmask[:, :Lk].contiguous()
    oc, _ = K.attn_fwd_cross(q, krow, vrow, B, 1, Lk, H, Hkv, hd, kml, scale)
    _bars(K.attn_decode(q, kc, vc, kmask, n_keys, H, Hkv, hd, scale, ws=ws), oc, f"attn_decode vs attn_fwd_cross hd {hd} G {G} B {B}")


def test_attn_decode_refuses_unsupported_geometry():
    K = _k()
    kc, vc = K.kv_cache_alloc(1, 1, 64, 80, DEV)
    with pytest.raises(Exception):
        K.attn_decode(_rnd(1, 80), kc, vc, None, torch.ones(1, dtype=torch.int32, device=DEV), 1, 1, 80, 1.0)


# ------------------------------------------------------------------------------------------------------------------ argmax
def test_argmax_rows_ties_and_full_vocab():
    K = _k()
    V = 128258
    x = _rnd(4, K.pad8(V), seed=3)
    x[:, V:] = 100.0                                         # pad columns beyond V must not be looked at
    assert torch.equal(K.argmax_rows(x, V), x[:, :V].float().argmax(-1))
    x[0, :V] = 1.0                                           # all equal: index 0
    x[1, 5] = x[1, 77777] = x[1, V - 1] = 50.0               # ties: the lowest index
    x[2, V - 1] = 60.0
    got = K.argmax_rows(x, V)
    assert got.dtype == torch.int64 and got.tolist()[:3] == [0, 5, V - 1]
    assert torch.equal(got, K.argmax_rows(x, V))
    t = _rnd(3, 304, seed=4)
    assert torch.equal(K.argmax_rows(t, 300), t[:, :300].float().argmax(-1))


# ------------------------------------------------------------------------------------------------------------------ model level
def _inputs(z):
    pv = Hh.pixels_list(z)
    eos = int(z["eos_token_id"])
    return (torch.from_numpy(z["input_ids"]), pv, torch.from_numpy(z["attention_mask"]), None if eos < 0 else eos, int(z["pad_token_id"]),
            int(z["n_steps"]))


@pytest.mark.parametrize("case", FIXTURES)
def test_generate_matches_reference_record(case):
    assert len(FIXTURES) == 5
    z = Hh.load_case("generation/" + case)
    model, _, _ = Hh.build_product_model("siglip", DEV)
    ids, pv, am, eos, pad, n = _inputs(z)
    eps = Hh.ENVELOPE_FACTOR * float(z["delta"])
    lg = GR.teacher_forced_logits(model, ids, am, pv, torch.from_numpy(z["tokens"]))
    err = np.abs(lg.numpy() - z["logits"])
    print(f"{case}: teacher-forced max |logit error| per step {err.max(axis=(1, 2)).round(4).tolist()} (eps {eps:.4f})")
    assert err.max() <= eps, (case, float(err.max()), eps)
    out = model.generate(ids, pixel_values=pv, attention_mask=am, max_new_tokens=n, eos_token_id=eos, pad_token_id=pad)
    assert out.dtype == torch.int64 and np.array_equal(out.cpu().numpy(), z["sequences"]), case
    model.train()
    again = model.generate(ids, pixel_values=pv, attention_mask=am, max_new_tokens=n, eos_token_id=eos, pad_token_id=pad)
    assert torch.equal(out, again), "two runs differ"


def test_generate_inside_training_loop_leaves_the_step_untouched():
    from mantis_amd.trainer import MantisHipTrainer
    z = Hh.load_case("siglip_training_step_ga1")
    g = Hh.load_case("generation/llava_generate_b2_leftpad")
    batch = dict(input_ids=torch.from_numpy(z["mb0.input_ids"]), attention_mask=torch.from_numpy(z["mb0.attention_mask"]),
                 labels=torch.from_numpy(z["mb0.labels"]), pixel_values=Hh.pixels_list(z, "mb0."))
    res = []
    for with_generate in (False, True):
        model, _, _ = Hh.build_product_model("siglip", DEV)
        tr = MantisHipTrainer(model, gradient_accumulation_steps=1)
        tr.training_step(model, batch)
        for p in model.parameters():
            p.grad = None
        if with_generate:
            ids, pv, am, _, _, n = _inputs(g)
            model.generate(ids, pixel_values=pv, attention_mask=am, max_new_tokens=n)
            assert model.training
        loss = tr.training_step(model, batch)
        res.append((loss.clone(), model.grad_arena.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_cached_decode_matches_cache_free_forward_at_full_width():
    """8B geometry, 2 decoder layers, the tower at 1 layer, B = 2 left-padded, 2 images + 256 tokens, 32 new tokens.  The tokens come from
    the product's own cache-free evaluation forward (argmax of the last row, the sequence grown by one each step) and are FED to the
    cached path; every step's cached-decode logits against that step's cache-free logits -- two paths through different kernels."""
    from mantis_amd import configuration_llava as C
    from mantis_amd import generation as Gn
    from mantis_amd.modeling_llava import LlavaForConditionalGeneration
    cfg = C.mantis_8b_siglip_llama3()
    cfg.vision_config.num_hidden_layers = 1
    cfg.text_config.num_hidden_layers = 2
    model = LlavaForConditionalGeneration(cfg, device=DEV, seed=0)
    model.eval()
    V, T, n_new = cfg.text_config.vocab_size, 258, 32
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, 128000, (2, T), generator=g)
    am = torch.ones_like(ids)
    ids[0, 3] = ids[0, 40] = ids[1, 20] = ids[1, 100] = cfg.image_token_index
    ids[1, :9] = cfg.pad_token_id
    am[1, :9] = 0
    pix = [torch.randn(2, 3, 336, 336, generator=g), torch.randn(2, 3, 336, 336, generator=g)]
    with torch.no_grad():
        cache, logits = Gn.prefill(model, ids, am, pix, n_new)
        cur_ids, cur_am = ids, am
        for step in range(n_new):
            ref = model(input_ids=cur_ids, pixel_values=pix, attention_mask=cur_am, return_logits=True).logits[:, -1, :V].float()
            _bars(logits[:, :V], ref, f"full-width step {step}")
            nxt = ref[:, :128000].argmax(-1)
            cur_ids = torch.cat([cur_ids, nxt.cpu()[:, None]], 1)
            cur_am = torch.cat([cur_am, torch.ones_like(cur_am[:, :1])], 1)
            if step + 1 < n_new:
                logits = Gn.decode_step(model, cache, nxt)
