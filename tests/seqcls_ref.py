"""Test-side fp32 restatement of the sequence-classification / regression head (test infrastructure, never imported by the product):

  * `pool_positions`: the pooled position rule of the reference's Idefics2ForSequenceClassification (modeling_idefics2.py:2174-2187);
  * `head_loss`: MSE / cross-entropy / BCE-with-logits on the pooled logits, mean reduction (:2187-2211);
  * `Idefics2SeqClsRef`: oracle.idefics2_ref.Idefics2Ref (tower, connector, merger, text model -- pinned to the reference by
    tests/test_idefics2_oracle.py) with the score head in place of lm_head + cross-entropy;
  * `head_reference`: the head alone in fp32 autograd, for the kernel-level checks;
  * `SeqclsOps`: oracle.ops_ref plus torch restatements of the three seqcls operators, so the product's host logic can run on the CPU.

tests/test_seqcls.py checks the restatement against fixtures recorded from the reference class (tests/golden/make_golden_idefics2_seqcls.py)."""
import torch
import torch.nn.functional as F

from oracle import ops_ref
from oracle.idefics2_ref import Idefics2Ref, patch_mask_from_pixel_mask

PROBLEM_TYPES = ("regression", "single_label_classification", "multi_label_classification")


def pool_positions(input_ids, pad_token_id):
    ids = torch.as_tensor(input_ids)
    B, T = ids.shape
    if pad_token_id is None:
        if B != 1:
            raise ValueError("Cannot handle batch sizes > 1 if no padding token is defined.")
        return torch.full((B,), T - 1, dtype=torch.int64)
    return (torch.eq(ids, pad_token_id).int().argmax(-1) - 1) % T


def head_loss(pooled, labels, problem_type, num_labels):
    """pooled fp32 [B, C] -> mean loss, as modeling_idefics2.py:2200-2211"""
    if problem_type == "regression":
        return F.mse_loss(pooled.squeeze(), labels.squeeze()) if num_labels == 1 else F.mse_loss(pooled, labels)
    if problem_type == "single_label_classification":
        return F.cross_entropy(pooled.view(-1, num_labels), labels.view(-1).long())
    if problem_type == "multi_label_classification":
        return F.binary_cross_entropy_with_logits(pooled, labels)
    raise ValueError(problem_type)


class Idefics2SeqClsRef(Idefics2Ref):
    """weights: the reference class's state_dict (model.* + score.weight + score.bias)."""

    def __init__(self, weights, cfg, num_labels, problem_type, pad_token_id, **kw):
        super().__init__(weights, cfg, **kw)
        self.num_labels, self.problem_type, self.pad_token_id = num_labels, problem_type, pad_token_id

    def hidden(self, input_ids, pixel_values, pixel_attention_mask, attention_mask, record=None):
        """Idefics2Ref.forward up to the final norm (that method reads lm_head, which this class does not have)."""
        cfg, w = self.cfg, self.w
        ids = torch.as_tensor(input_ids)
        am = torch.as_tensor(attention_mask)
        emb = F.embedding(ids, w["model.text_model.embed_tokens.weight"])
        if pixel_values is not None:
            pv = torch.as_tensor(pixel_values).float()
            B, M = pv.shape[:2]
            pv = pv.reshape(B * M, *pv.shape[2:])
            real = (pv == 0.0).sum(dim=(-1, -2, -3)) != pv[0].numel()
            pv = pv[real]
            if pixel_attention_mask is None:
                pm = torch.ones(pv.shape[0], pv.shape[2], pv.shape[3], dtype=torch.bool, device=pv.device)
            else:
                pm = torch.as_tensor(pixel_attention_mask).bool().reshape(B * M, *pixel_attention_mask.shape[2:])[real]
            patch_mask = patch_mask_from_pixel_mask(pm, self.vc["patch_size"])
            feats = self.vision(pv.to(w["score.weight"].dtype), patch_mask)
            img = self.connector(feats, patch_mask.reshape(patch_mask.shape[0], -1), record)
            sel = ids == cfg["image_token_id"]
            rows = img.reshape(-1, img.shape[-1])
            bi, ti = torch.nonzero(sel, as_tuple=True)
            emb = emb.index_put((bi, ti), rows)
        return self.text(emb, am, record)

    def forward(self, input_ids, pixel_values, pixel_attention_mask, attention_mask, labels, record=None):
        """-> (loss or None, pooled logits fp32 [B, C], pooled positions int64 [B])"""
        h = self.hidden(input_ids, pixel_values, pixel_attention_mask, attention_mask, record)
        pos = pool_positions(torch.as_tensor(input_ids).cpu(), self.pad_token_id).to(h.device)
        rows = h[torch.arange(h.shape[0], device=h.device), pos]                 # score on the pooled rows = score everywhere, then index
        pooled = F.linear(rows, self.w["score.weight"], self.w["score.bias"]).float()
        loss = None
        if labels is not None:
            loss = head_loss(pooled, torch.as_tensor(labels).to(h.device), self.problem_type, self.num_labels)
        return loss, pooled, pos


def head_reference(x, pool, norm_w, score_w, score_b, labels, problem_type, B, T, eps):
    """The head alone in fp32 autograd on given (bf16-valued) inputs: x [B*T, d] pre-norm.  -> dict(loss, logits, dW, db, dnorm, dx);
    the normalised row is rounded to bf16 where the bf16 module rounds it (after x * rstd and after * weight), straight-through."""
    xf = x.detach().float().clone().requires_grad_(True)
    nw = norm_w.detach().float().clone().requires_grad_(True)
    W = score_w.detach().float().clone().requires_grad_(True)
    b = score_b.detach().float().clone().requires_grad_(True)
    rows = xf.view(B, T, -1)[torch.arange(B, device=x.device), pool.long()]
    y = rows * torch.rsqrt(rows.pow(2).mean(-1, keepdim=True) + eps)
    y = y + (y.to(torch.bfloat16).float() - y).detach()
    nf = y * nw
    nf = nf + (nf.to(torch.bfloat16).float() - nf).detach()
    logits = F.linear(nf, W, b)
    loss = head_loss(logits, labels, problem_type, W.shape[0])
    loss.backward()
    return dict(loss=loss.detach(), logits=logits.detach(), dW=W.grad, db=b.grad, dnorm=nw.grad, dx=xf.grad)


class _SeqclsOps:
    """oracle.ops_ref + the classification-head operators in torch (fp32 math on the tensors' own dtype, like ops_ref)."""

    def __getattr__(self, name):
        return getattr(ops_ref, name)

    @staticmethod
    def seqcls_pool_index(input_ids, pad_token_id):
        B, T = input_ids.shape
        if pad_token_id is None:
            return torch.full((B,), T - 1, dtype=torch.int32)
        return ((torch.eq(input_ids, pad_token_id).int().argmax(-1) - 1) % T).to(torch.int32)

    @staticmethod
    def seqcls_head_fwd(x, pool, norm_w, score_w, score_b, labels, problem_type, B, T, eps, grad_scale=1.0, loss_scale=1.0, write_grad=True):
        rows = (torch.arange(B) * T + pool.long()).to(torch.int32)
        xr = x.float()[rows.long()]
        rstd = torch.rsqrt(xr.pow(2).mean(-1) + eps)
        nf = ((xr * rstd[:, None]).to(x.dtype).float() * norm_w.float()).to(x.dtype)
        logits = F.linear(nf.float(), score_w.float(), score_b.float())
        loss = dlogits = status = None
        if labels is not None:
            z = logits.detach().clone().requires_grad_(True)
            with torch.enable_grad():
                raw = head_loss(z, labels.long() if problem_type == "single_label_classification" else labels, problem_type, score_w.shape[0])
                raw.backward()
            loss = (raw.detach() * loss_scale).reshape(1)
            dlogits = z.grad * grad_scale if write_grad else None
            status = torch.zeros(1, dtype=torch.int32)
        return dict(logits=logits, loss=loss, status=status, dlogits=dlogits, nf=nf, rstd=rstd, rows=rows)

    @staticmethod
    def seqcls_head_bwd(dlogits, nf, x, rows, rstd, norm_w, score_w, grad_score_w, grad_score_b, grad_norm_w, accumulate):
        def put(g, v):
            if g is not None:
                g.copy_(((g.float() + v) if accumulate else v).to(g.dtype))
        put(grad_score_w, dlogits.t() @ nf.float())
        put(grad_score_b, dlogits.sum(0))
        dnf = dlogits @ score_w.float()
        xhat = x.float()[rows.long()] * rstd[:, None]
        g = dnf * norm_w.float()
        put(grad_norm_w, (dnf * xhat).sum(0))
        return (rstd[:, None] * (g - xhat * (g * xhat).mean(-1, keepdim=True))).to(x.dtype)


SeqclsOps = _SeqclsOps()
