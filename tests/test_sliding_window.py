"""CPU: Mistral's sliding-window attention on the Idefics2 path -- the C-ABI entries, the config defaults, the host rule that engages the
window, and the semantics `q - W < k <= q` pinned to the reference through the oracle and tests/golden/idefics2_window_b2_rightpad.npz
(recorded by tests/golden/make_golden_idefics2_window.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(__file__), "golden")
FIXTURE = os.path.join(G, "idefics2_window_b2_rightpad.npz")


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def windowed_attention(window):
    """oracle.llava_ref.attention with the sliding window of HF masking_utils (kv_idx > q_idx - sliding_window) on causal calls."""
    from oracle.llava_ref import attention

    def attn(q, k, v, scale, causal, key_mask=None):
        if not causal:
            return attention(q, k, v, scale, causal, key_mask=key_mask)
        B, H, L, hd = q.shape
        rep = H // k.shape[1]
        if rep > 1:
            k = k.repeat_interleave(rep, dim=1)
            v = v.repeat_interleave(rep, dim=1)
        s = torch.matmul(q, k.transpose(-1, -2)) * scale
        qi, ki = torch.arange(L)[:, None], torch.arange(k.shape[2])[None, :]
        s = s.masked_fill(~((ki <= qi) & (ki > qi - window)), torch.finfo(s.dtype).min)
        if key_mask is not None:
            s = s.masked_fill(key_mask[:, None, None, :] == 0, torch.finfo(s.dtype).min)
        p = torch.softmax(s, dim=-1, dtype=torch.float32).to(q.dtype)
        return torch.matmul(p, v).transpose(1, 2).contiguous()
    return attn


def test_window_entries_are_exported():
    import __graft_entry__
    __graft_entry__.build()
    from mantis_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("mantis_attn_fwd_window", "mantis_attn_bwd_window"):
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n


def test_config_window_defaults():
    from mantis_amd.configuration_idefics2 import Idefics2Config, mantis_8b_idefics2
    assert Idefics2Config().text_config.sliding_window == 4096                      # mistral: HF MistralConfig's default
    assert Idefics2Config(text_config=dict(model_type="mistral")).sliding_window == 4096
    assert Idefics2Config(text_config=dict(model_type="llama")).text_config.sliding_window is None
    assert Idefics2Config(text_config=dict(model_type="mistral", sliding_window=None)).text_config.sliding_window is None
    assert Idefics2Config(text_config=dict(model_type="mistral", sliding_window=24)).text_config.sliding_window == 24
    cfg = mantis_8b_idefics2()
    assert cfg.text_config.sliding_window == 4096 and cfg.sliding_window == 4096
    # the window-less goldens state sliding_window=None: they keep full causal attention
    from tests import helpers
    meta, _ = helpers.golden_cfg_and_weights("idefics2")
    assert Idefics2Config.from_oracle_meta(meta).text_config.sliding_window is None


def test_window_engages_only_past_its_length():
    from mantis_amd.configuration_idefics2 import Idefics2Config, mantis_8b_idefics2
    from mantis_amd import decoder as D
    tc = mantis_8b_idefics2().text_config
    assert D.attn_window(tc, 4096) is None            # bench.py's packed Idefics2 row (2 x 2048): the plain causal kernels
    assert D.attn_window(tc, 4097) == 4096
    assert D.attn_window(tc, 8192) == 4096
    assert D.attn_window(Idefics2Config(text_config=dict(model_type="llama")).text_config, 8192) is None
    # Qwen2 configs carry a sliding_window that use_sliding_window=False switches off
    from mantis_amd.configuration_llava import SubConfig
    assert D.attn_window(SubConfig(sliding_window=4096, use_sliding_window=False), 8192) is None
    assert D._window_kw(tc, 100) == {} and D._window_kw(tc, 5000) == dict(window=4096)
    from mantis_amd import hip_ops
    assert not hip_ops.window_engaged(None, 10) and not hip_ops.window_engaged(10, 10) and hip_ops.window_engaged(9, 10)


def test_decoder_passes_the_window_to_attention(monkeypatch):
    """layer_forward -- the forward of a decoder layer, which the backward also runs again under activation checkpointing -- hands the
    window to the attention forward exactly when the row is longer than it.  (The backward's attn_bwd call, the checkpointed re-run and
    their bits are exercised on the GPU: tests/test_sliding_window_gpu.py.)"""
    from mantis_amd import decoder as D
    from mantis_amd.configuration_llava import SubConfig
    seen = []

    class FakeK:
        def __getattr__(self, name):
            def f(*a, **k):
                if name in ("attn_fwd", "attn_bwd"):
                    seen.append((name, k.get("window")))
                raise StopIteration
            return f
    tc = SubConfig(num_attention_heads=2, num_key_value_heads=1, head_dim=4, rms_norm_eps=1e-5, sliding_window=8)
    for L, want in ((8, None), (9, 8)):
        seen.clear()
        K = FakeK()
        K.rmsnorm_fwd = lambda x, w, eps: (x, None)
        K.linear_qkv_rope = lambda *a: None
        with pytest.raises(StopIteration):
            D.layer_forward(K, {"ln1": None, "qkv": None}, tc, None, 1, L, None, None, None, None, 1.0)
        assert seen == [("attn_fwd", want)]


def test_oracle_with_window_reproduces_reference_fixture(monkeypatch):
    """The oracle's attention restated with the window reproduces the reference's loss and every gradient on the windowed fixture (so
    `q - W < k <= q` on top of the key mask is what Idefics2's Mistral computes), and the window-less oracle does not."""
    import oracle.idefics2_ref as O
    from oracle.idefics2_ref import Idefics2Ref
    z = np.load(FIXTURE)
    W = int(z["sliding_window"])
    assert z["input_ids"].shape[1] > 3 * W
    assert (z["attention_mask"] == 0).sum(axis=1).max() > W          # a row padded by more than the window
    gap = abs(float(z["loss"]) - float(z["loss_nowindow"]))
    assert gap > 100 * 1e-6 * abs(float(z["loss"]))                   # the fixture is sensitive to the window

    def run():
        m = Idefics2Ref.from_npz(os.path.join(G, "weights_idefics2.npz"))
        loss, _ = m.forward(z["input_ids"], z["pixel_values"].astype(np.float32), None, z["attention_mask"], z["labels"])
        loss.backward()
        return m, loss
    m0, loss0 = run()
    assert abs(float(loss0) - float(z["loss_nowindow"])) <= 1e-5 * abs(float(z["loss"]))
    monkeypatch.setattr(O, "attention", windowed_attention(W))
    m, loss = run()
    assert abs(float(loss) - float(z["loss"])) <= 1e-6 * abs(float(z["loss"])) + 1e-6, (float(loss), float(z["loss"]))
    n = 0
    for k in z.files:
        if k.startswith("grad."):
            g = m.w[k[5:]].grad
            assert g is not None, k
            assert rel_l2(g.numpy(), z[k]) < 2e-4 or np.abs(z[k]).max() < 1e-7, (k, rel_l2(g.numpy(), z[k]))
            n += 1
    assert n >= 21
