"""-m gpu: the sequence-classification / regression head on the gfx950 kernels (csrc/seqcls.hip) and through the Idefics2 model.

Kernel level: mantis_seqcls_pool_index exact; mantis_seqcls_head_fwd / _bwd against the fp32 restatement (tests/seqcls_ref.py) on the
device with the same bf16-rounded inputs.  Model level: the reference's fixtures through engine.step_from_batch; the full-width,
reduced-depth step against the restatement in fp32 on the device; activation checkpointing, gradient accumulation, trainer + fused
optimizer, evaluation forward.  Bars: SURVEY 8c's (cosine >= 0.999, rel-L2 <= 2e-2; loss rtol 5e-3; logits max-abs <= 3e-2 * rms)."""
import numpy as np
import pytest
import torch

from tests import helpers as Hh
from tests import seqcls_ref as S
from tests import test_seqcls as TS

DEV = "cuda"
BF = torch.bfloat16
pytestmark = pytest.mark.gpu
PROBLEMS = S.PROBLEM_TYPES


def K():
    import mantis_amd.hip_ops as k
    return k


def test_pool_index_kernel_is_exact():
    k = K()
    ids = torch.tensor(list(TS.POOL_ROWS.values()), dtype=torch.int64)
    assert k.seqcls_pool_index(ids.to(DEV), 0).cpu().tolist() == S.pool_positions(ids, 0).tolist()
    assert k.seqcls_pool_index(ids.to(DEV), None).cpu().tolist() == [5] * 6
    g = torch.Generator().manual_seed(3)
    for T in (1, 63, 64, 65, 2048, 5000):                                   # around the wave stride, and long rows
        big = torch.randint(1, 50, (6, T), generator=g)                   # row 2: no pad id at all
        big[0, 0] = 0                                                      # starts with the pad id (left padding)
        big[1, T - 1] = 0                                                  # only the last token
        big[3, T // 3:] = 0                                                # right padding
        big[4, T // 2] = 0                                                 # a single pad id mid-row
        big[5, :] = 0                                                      # all pad
        got = k.seqcls_pool_index(big.to(DEV), 0).cpu().tolist()
        assert got == S.pool_positions(big, 0).tolist(), T


def make_labels(problem, B, C, g):
    if problem == "single_label_classification":
        return torch.randint(0, C, (B,), generator=g)
    if problem == "multi_label_classification":
        return (torch.rand(B, C, generator=g) > 0.5).float()
    return torch.rand(B, C, generator=g) * 4 + 1


ROW_BAR = 2 * 2.0 ** -8


def rows_close(got, want, what):
    """rel-L2 of every ROW of a bf16 gradient against the fp32 restatement: a wrong pooled row of dx or class row of dW must not hide in
    the whole-tensor norm.  The kernels (csrc/seqcls.hip) keep everything in fp32 and round each output element to bf16 once, at most
    2^-8 of the element and so of the row; a second 2^-8 covers the fp32 arithmetic (the cancelling g - xhat . mean(g . xhat) of dx, sums
    over B and C in another order) and the last-place differences of the logits upstream.  A zero row of the restatement must be zero."""
    got, want = got.double().cpu().reshape(want.shape[0], -1), want.double().cpu().reshape(want.shape[0], -1)
    num, den = (got - want).norm(dim=1), want.norm(dim=1)
    zero = den < 1e-12
    assert not bool((zero & (got.norm(dim=1) >= 1e-6)).any()), what
    err = torch.where(zero, torch.zeros_like(num), num / den.clamp_min(1e-300))
    assert float(err.max()) <= ROW_BAR, f"{what}: worst row rel-L2 {float(err.max()):.3e} > {ROW_BAR:.3e} at row {int(err.argmax())}"
    return float(err.max())


def logits_close(logits, nf, W, bias, what):
    """every logit (fp32) of every sample against the fp64 product of the kernel's OWN normalised row: d fp32 additions in any order cost
    at most d . 2^-24 . (sum |nf| |W| + |b|), doubled for the second-order terms (tests/local_error.py gemm_bound's `acc`)"""
    nf64, W64, b64 = nf.double().cpu(), W.double().cpu(), bias.double().cpu()
    ref = nf64 @ W64.t() + b64
    bound = 2.0 * nf.shape[1] * 2.0 ** -24 * (nf64.abs() @ W64.abs().t() + b64.abs())
    ratio = (logits.double().cpu() - ref).abs() / bound.clamp_min(1e-300)
    assert float(ratio.max()) <= 1.0, f"{what}: logit {divmod(int(ratio.argmax()), ratio.shape[1])} (sample, class) is {float(ratio.max()):.3g} x its bound"
    return float(ratio.max())


def nf_close(nf, x_rows, nw, eps, what):
    """the normalised row bf16(bf16(x . rstd) . w) per element against the same chain from an fp64 rstd: the kernel's fp32 rstd may turn a
    tie of the first rounding (1 ulp, up to 2^-7 of the value), which the second rounding can carry to 3 ulps of a result in a finer
    binade; nothing else differs"""
    from tests import local_error as LE
    x64 = x_rows.double().cpu()
    rstd = torch.rsqrt(x64.pow(2).mean(-1, keepdim=True) + eps)
    y = (x64 * rstd).float().to(BF).double() * nw.double().cpu()
    ulp = LE.ulp_distance_bf16(nf.cpu(), y)
    assert int(ulp.max()) <= 3, f"{what}: nf element {divmod(int(ulp.argmax()), ulp.shape[1])} (sample, column) is {int(ulp.max())} ulps off"
    return int(ulp.max())


def close(got, want, what):
    got, want = got.float().cpu().numpy(), want.float().cpu().numpy()
    if np.linalg.norm(want) < 1e-12:
        assert np.linalg.norm(got) < 1e-6, what
        return
    c, r = Hh.cosine(got, want), Hh.rel_l2(got, want)
    assert c >= 0.999 and r <= 2e-2, (what, c, r)


@pytest.mark.parametrize("d", [64, 4096])
@pytest.mark.parametrize("C", [1, 5, 128])
@pytest.mark.parametrize("B", [1, 2, 8])
def test_head_kernels_match_restatement(d, C, B):
    k = K()
    T, eps = 37, 1e-5
    g = torch.Generator().manual_seed(1000 * d + 10 * C + B)
    x = (torch.randn(B * T, d, generator=g) * 1.5).to(BF).to(DEV)
    nw = (1 + 0.1 * torch.randn(d, generator=g)).to(BF).to(DEV)
    W = (torch.randn(C, d, generator=g) * d ** -0.5).to(BF).to(DEV)
    bias = (0.1 * torch.randn(C, generator=g)).to(BF).to(DEV)
    pool = torch.randint(0, T, (B,), generator=g).to(torch.int32).to(DEV)
    for problem in PROBLEMS:
        lab = make_labels(problem, B, C, g).to(DEV)
        lab_k = lab.to(torch.int32) if problem == "single_label_classification" else lab.contiguous()
        ref = S.head_reference(x, pool, nw, W, bias, lab, problem, B, T, eps)
        runs = []
        for rep in range(2):
            r = k.seqcls_head_fwd(x, pool, nw, W, bias, lab_k, problem, B, T, eps, grad_scale=1.0, loss_scale=1.0)
            gW, gb, gn = torch.zeros_like(W), torch.zeros_like(bias), torch.zeros_like(nw)
            dx_rows = k.seqcls_head_bwd(r["dlogits"], r["nf"], x, r["rows"], r["rstd"], nw, W, gW, gb, gn, False)
            dx = k.scatter_rows(dx_rows, r["rows"], B * T)
            torch.cuda.synchronize()
            runs.append((r["loss"].clone(), r["logits"].clone(), gW, gb, gn, dx))
        for a, b_ in zip(runs[0], runs[1]):
            assert torch.equal(a, b_), f"{problem}: two runs differ"
        loss, logits, gW, gb, gn, dx = runs[0]
        what = f"d{d} C{C} B{B} {problem}"
        assert int(r["status"][0]) == 0 and r["rows"].cpu().tolist() == [b * T + int(pool[b]) for b in range(B)]
        rms = float(ref["logits"].pow(2).mean().sqrt())
        assert float((logits - ref["logits"]).abs().max()) <= 3e-2 * rms, what
        assert abs(float(loss) - float(ref["loss"])) <= 5e-3 * abs(float(ref["loss"])) + 1e-12, (what, float(loss), float(ref["loss"]))
        close(gW, ref["dW"], what + " dW")
        close(gb, ref["db"], what + " db")
        close(gn, ref["dnorm"], what + " dnorm")
        close(dx, ref["dx"], what + " dx")
        # localised: the normalised row per element, every logit per sample, dW per class row, dx per pooled row
        rows = r["rows"].long()
        nf_close(r["nf"], x[rows], nw, eps, what + " nf")
        logits_close(logits, r["nf"], W, bias, what + " logits")
        rows_close(gW, ref["dW"], what + " dW row")
        rows_close(dx[rows], ref["dx"][rows], what + " dx row")
        off = torch.ones(B * T, dtype=torch.bool, device=DEV)
        off[r["rows"].long()] = False
        assert not dx[off].any(), what + ": dx must be exactly zero off the pooled rows"
        # accumulate: a second backward on top of the first doubles the weight gradients; grad_scale / loss_scale scale linearly
        r2 = k.seqcls_head_fwd(x, pool, nw, W, bias, lab_k, problem, B, T, eps, grad_scale=0.5, loss_scale=0.5)
        aW, ab, an = gW.clone(), gb.clone(), gn.clone()
        k.seqcls_head_bwd(r2["dlogits"], r2["nf"], x, r2["rows"], r2["rstd"], nw, W, aW, ab, an, True)
        torch.cuda.synchronize()
        assert abs(float(r2["loss"]) - 0.5 * float(ref["loss"])) <= 5e-3 * abs(0.5 * float(ref["loss"])) + 1e-12
        close(aW, 1.5 * ref["dW"], what + " dW accumulate")
        # accumulate reads the bf16 gW (2^-8 of dW), adds the halved run in fp32 and rounds (2^-8 of 1.5 dW): 2.5 / 1.5 . 2^-8 of the sum
        rows_close(aW, 1.5 * ref["dW"], what + " dW row accumulate")
        close(ab, 1.5 * ref["db"], what + " db accumulate")
        close(an, 1.5 * ref["dnorm"], what + " dnorm accumulate")


def test_unsupported_shapes_and_bad_class_labels():
    k = K()
    B, T = 2, 4
    pool = torch.zeros(B, dtype=torch.int32, device=DEV)

    def args(d, C):
        return (torch.zeros(B * T, d, dtype=BF, device=DEV), pool, torch.ones(d, dtype=BF, device=DEV),
                torch.zeros(C, d, dtype=BF, device=DEV), torch.zeros(C, dtype=BF, device=DEV))
    with pytest.raises(ValueError):
        k.seqcls_head_fwd(*args(64, 129), None, None, B, T, 1e-5)
    with pytest.raises(ValueError):
        k.seqcls_head_fwd(*args(8200, 5), None, None, B, T, 1e-5)
    r = k.seqcls_head_fwd(*args(64, 5), torch.tensor([1, 7], dtype=torch.int32, device=DEV), "single_label_classification", B, T, 1e-5)
    assert int(r["status"][0]) == 1 and not r["dlogits"][1].any()


# ----------------------------------------------------------------------------------------------------------------- model level
@pytest.mark.parametrize("case", TS.CASES)
def test_fixture_step_matches_restatement_and_reference(case):
    z, model = TS.build_product(case, DEV)
    _, ref = TS.build_ref(case, bf16=True)
    assert model._ensure_grad_arena()
    out = model.engine.step_from_batch(TS.batch_of(z), compute_grads=True, overwrite_grads=True)
    torch.cuda.synchronize()
    assert np.array_equal(out["pooled_positions"].cpu().numpy(), z["pooled_positions"])
    TS.check_step(model, ref, z, out)
    for name, p in model.named_parameters():          # and against the reference's own recorded fp32 gradients
        if p.requires_grad and np.linalg.norm(z["grad." + name]) > 1e-12:
            assert Hh.cosine(p.grad.float().cpu().numpy(), z["grad." + name]) >= 0.99, name
        elif not p.requires_grad:
            assert p.grad is None, name


def full_width_model(problem="regression", C=5):
    from mantis_amd import configuration_idefics2 as Cf
    from mantis_amd.modeling_idefics2 import Idefics2ForSequenceClassification
    cfg = Cf.mantis_8b_idefics2(num_labels=C, problem_type=problem, pad_token_id=0)
    cfg.vision_config.num_hidden_layers = 1
    cfg.text_config.num_hidden_layers = 2
    cfg.perceiver_config.resampler_depth = 1
    return cfg, Idefics2ForSequenceClassification(cfg, device=DEV, seed=0)


def full_width_batch(cfg, B=2, T=2048, pad=300, seed=0):
    import bench
    b = bench.synthetic_batch_idefics2(cfg, B, T, 2, 448, 0)
    b["input_ids"][B - 1, T - pad:] = 0                                   # the last row is right-padded (pad id 0 occurs nowhere else)
    b["attention_mask"][B - 1, T - pad:] = 0
    g = torch.Generator().manual_seed(seed)
    b["labels"] = torch.rand(B, cfg.num_labels, generator=g) * 4 + 1
    return b


def test_full_width_step_vs_restatement():
    """mantis_8b_idefics2(num_labels=5, regression), tower 1 / perceiver 1 / text 2 layers, B = 2, T = 2048, one row right-padded, against the
    restatement in fp32 on the device: the bars of the generation class's full-width check (check_idefics2_full_width_vs_oracle: loss rtol
    5e-3, logits rel-L2 < 3e-2, every gradient at 0.999 / 2e-2 or the bf16 envelope helper's bar, unchanged)."""
    cfg, model = full_width_model()
    batch = full_width_batch(cfg)
    assert model._ensure_grad_arena()
    out = model.engine.step_from_batch(batch, compute_grads=True, overwrite_grads=True)
    torch.cuda.synchronize()
    loss = float(out["loss"].float().cpu().reshape(-1)[0])
    assert out["pooled_positions"].cpu().tolist() == [2047, 2048 - 300 - 1]
    meta = dict(vision=cfg.vision_config.to_dict(), perceiver=cfg.perceiver_config.to_dict(), text=cfg.text_config.to_dict(),
                image_token_id=cfg.image_token_id)
    with torch.device(DEV):
        ref = S.Idefics2SeqClsRef({n: p.detach().float() for n, p in model.named_parameters()}, meta, 5, "regression", 0)
        oloss, opooled, _ = ref.forward(batch["input_ids"].to(DEV), batch["pixel_values"].to(DEV), None, batch["attention_mask"].to(DEV),
                                        batch["labels"].to(DEV))
        oloss.backward()
    torch.cuda.synchronize()
    assert abs(loss - float(oloss)) <= 5e-3 * abs(float(oloss)), (loss, float(oloss))
    # logits as Hh.check_idefics2_step_against_oracle compares them at this geometry: rel-L2 < 3e-2
    r = Hh.rel_l2(out["logits"].float().cpu().numpy(), opooled.detach().cpu().numpy())
    print(f"full width: loss {loss:.5f} / {float(oloss):.5f}, pooled logits rel-L2 {r:.4f}", flush=True)
    assert r < 3e-2, r
    env = Hh.bf16_envelope("oracle_bf16:idefics2_full_width")
    n = 0
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        og = ref.w[name].grad.float().cpu().numpy()
        g = p.grad.float().cpu().numpy()
        if np.linalg.norm(og) < 1e-12:
            assert np.linalg.norm(g) < 1e-6, name
            continue
        c, r = Hh.cosine(g, og), Hh.rel_l2(g, og)
        cbar, rbar = Hh.envelope_bars(env, name)
        assert c >= cbar and r <= rbar, (name, c, r, cbar, rbar)
        n += 1
    assert n >= 20


def test_checkpointing_is_bitwise():
    from mantis_amd.trainer import MantisHipTrainer
    cfg, model = full_width_model()
    batch = full_width_batch(cfg, T=1024, pad=100)
    tr = MantisHipTrainer(model, gradient_accumulation_steps=1)
    res = []
    for on in (False, True):
        (model.gradient_checkpointing_enable if on else model.gradient_checkpointing_disable)()
        for p in model.parameters():
            p.grad = None
        loss = tr.training_step(model, batch)
        torch.cuda.synchronize()
        res.append((loss.clone(), model.grad_arena.clone()))
    model.gradient_checkpointing_disable()
    assert res[0][0].dim() == 0 and not res[0][0].requires_grad and torch.isfinite(res[0][0])
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), "activation checkpointing changed the step"


def test_accumulation_of_two_single_sample_steps_matches_restatement():
    """Gradient accumulation 2 x (B = 1) with loss / 2 on the regression fixture's two rows against the restatement's gradients
    accumulated the same way (fp32, same bf16-rounded weights): SURVEY 8c's bars."""
    from mantis_amd.trainer import MantisHipTrainer
    case = "idefics2_seqcls_regression_c5"
    z, model = TS.build_product(case, DEV)
    _, ref = TS.build_ref(case, bf16=True)
    batch = TS.batch_of(z)
    halves = [{k: (v[i: i + 1] if torch.is_tensor(v) else v) for k, v in batch.items()} for i in range(2)]
    tr = MantisHipTrainer(model, gradient_accumulation_steps=2)
    losses = [tr.training_step(model, h) for h in halves]
    torch.cuda.synchronize()
    ref.zero_grad()
    total = 0.0
    for h in halves:
        ol, _, _ = ref.forward(h["input_ids"], h["pixel_values"], None, h["attention_mask"], h["labels"])
        (ol / 2).backward()
        total += float(ol.detach()) / 2
    assert all(l.dim() == 0 and not l.requires_grad for l in losses)
    assert abs(float(losses[0] + losses[1]) - total) <= 5e-3 * abs(total), (losses, total)
    for name, p in model.named_parameters():
        if p.requires_grad:
            want = ref.w[name].grad.numpy()
            got = p.grad.float().cpu().numpy()
            if np.linalg.norm(want) > 1e-12:
                c, r = Hh.cosine(got, want), Hh.rel_l2(got, want)
                assert c >= Hh.GRAD_COS and r <= Hh.GRAD_REL, (name, c, r)


def test_trainer_optimizer_and_eval_forward():
    from mantis_amd.optim import FusedAdamW
    from mantis_amd.trainer import MantisHipTrainer
    z, model = TS.build_product("idefics2_seqcls_regression_c5", DEV)
    batch = TS.batch_of(z)
    tr = MantisHipTrainer(model, gradient_accumulation_steps=1)
    opt = FusedAdamW(model, lr=2e-3, weight_decay=0.0)
    w0, b0 = model.score.weight.detach().clone(), model.score.bias.detach().clone()
    losses = []
    for _ in range(4):
        for p in model.parameters():
            p.grad = None
        loss = tr.training_step(model, batch)
        assert loss.dim() == 0 and not loss.requires_grad
        losses.append(float(loss))
        if len(losses) <= 3:
            opt.clip_grad_norm(1.0)
            opt.step()
    assert not torch.equal(w0, model.score.weight.detach()) and not torch.equal(b0, model.score.bias.detach())
    assert losses[3] < losses[0], losses
    # evaluation forward: the same pooled logits as the training step, bit for bit; gradients untouched
    for p in model.parameters():
        p.grad = None
    assert model._ensure_grad_arena()
    out = model.engine.step_from_batch(batch, compute_grads=True, overwrite_grads=True)
    g = model.grad_arena.clone()
    model.eval()
    with torch.no_grad():
        ev = model(**batch)
    torch.cuda.synchronize()
    assert torch.equal(ev.logits, out["logits"]) and torch.equal(ev.loss.reshape(-1), out["loss"].reshape(-1))
    assert torch.equal(model.grad_arena, g)
    model.train()
