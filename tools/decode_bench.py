#!/usr/bin/env python3
"""Decode-step benchmark of the generation path (a tool, not bench.py): ms per token and achieved bytes / s at the full 8B geometry.

    python tools/decode_bench.py --all [--layers 32] [--new-tokens 128] [--out profiles/generation_decode.json]
    python tools/decode_bench.py --kernels                 # per-kernel A/B on every step shape
    python tools/decode_bench.py --batch 8 --path new      # one end-to-end measurement (what --all runs in child processes)
    python tools/decode_bench.py --family idefics3 --batch 1   # Idefics3 generate(): ms / token without an EOS and with a never-firing EOS
                                                               # read back every k = 1, 4, 8, 16 steps, three repeats each (+ --markdown)

Prompt = the headline sample (4 x 336^2 images + 512 tokens), B in {1, 8}, 128 new tokens.  The comparator is what the library offered
before the decode kernels: the same step composed from the existing entries (`gemm_nt` at M = B, `rope_apply_`, `attn_fwd_cross` with one query row
per sample over a row-major cache), measured by this tool in the same run.  `--all` starts one fresh child process per measurement, each under
its own time limit, and stops at the first one that fails.  Bytes moved per token = decoder + lm_head weights once + the live K / V of every layer."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_PEAK_TBS = 8.0        # MI355X HBM3E, specification
HBM_ACHIEVABLE_TBS = 6.3  # what a plain streaming read reaches on this chip
COLD_BYTES = 1 << 30      # a timed kernel's operands rotate over copies totalling at least this much: well past the 256 MiB last-level cache


def _clock():
    """the shader clock the box reports while the benchmark runs (read only), or 'unavailable'"""
    import re
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        lines = [re.sub(r"\s+", " ", l).strip() for l in out.splitlines() if "sclk" in l.lower()]
        return lines[0] if lines else "unavailable"
    except Exception:
        return "unavailable"


def _model(layers):
    import torch
    from mantis_amd import configuration_llava as C
    from mantis_amd.modeling_llava import LlavaForConditionalGeneration
    cfg = C.mantis_8b_siglip_llama3()
    cfg.text_config.num_hidden_layers = layers
    model = LlavaForConditionalGeneration(cfg, device="cuda", seed=0)
    model.eval()
    return model, cfg


def _prompt(cfg, B, T=516, n_img=4):
    import torch
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 128000, (B, T), generator=g)
    for j in range(n_img):
        ids[:, 1 + j * 100] = cfg.image_token_index
    pix = [torch.randn(n_img, 3, 336, 336, generator=g) for _ in range(B)]
    return ids, torch.ones_like(ids), pix


def _timeit(fn, copies, n=20, warm=3):
    """median us of fn(i) over n timed calls; i walks `copies` operand sets (COLD_BYTES in total), so no call finds its streamed operand in
    the last-level cache -- as in a decode step, where 15 GB pass between two uses of a weight"""
    import torch
    for i in range(warm):
        fn(i % copies)
    ts = []
    for i in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn((warm + i) % copies)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts)


def kernels():
    """per kernel, per step shape: the new entry vs the existing one, us (median of 20) and achieved TB/s of the new one"""
    import torch
    from mantis_amd import hip_ops as K
    rows = []
    for N, Kd in ((6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336), (128258, 4096)):
        nc = max(2, -(-COLD_BYTES // (2 * K.pad8(N) * Kd)))
        ws = [(torch.randn(K.pad8(N), Kd, device="cuda") * 0.02).to(torch.bfloat16) for _ in range(nc)]
        for M in (1, 8, 16):
            x = torch.randn(M, Kd, device="cuda").to(torch.bfloat16)
            t_new = _timeit(lambda i: K.linear_skinny(x, ws[i], n_valid=N, ldc=K.pad8(N)), nc)
            t_old = _timeit(lambda i: K.gemm_nt(x, ws[i], n_valid=N, ldc=K.pad8(N)), nc)
            rows.append(dict(kernel="linear", shape=f"{M} x {N} x {Kd}", new_us=round(t_new, 1), old_us=round(t_old, 1),
                             new_tbs=round(2.0 * N * Kd / t_new / 1e6, 2), old_tbs=round(2.0 * N * Kd / t_old / 1e6, 2),
                             dispatch="skinny" if K.decode_uses_skinny(M, N) else "gemm_nt", copies=nc))
        del ws
    H, Hkv, hd, S = 32, 8, 128, 3556
    for B in (1, 8):
        nc = max(2, -(-COLD_BYTES // (4 * B * Hkv * S * hd)))
        kcs = [torch.randn(B, Hkv, S, hd, device="cuda").to(torch.bfloat16) for _ in range(nc)]
        vcs = [torch.randn(B, Hkv, S, hd, device="cuda").to(torch.bfloat16) for _ in range(nc)]
        q = torch.randn(B, H * hd, device="cuda").to(torch.bfloat16)
        nk = torch.full((B,), S, dtype=torch.int32, device="cuda")
        km = torch.ones(B, S, dtype=torch.int32, device="cuda")
        ws = K.attn_decode_workspace(B, H, Hkv, hd, S, "cuda")
        krs = [k.permute(0, 2, 1, 3).reshape(B * S, Hkv * hd).contiguous() for k in kcs]
        vrs = [v.permute(0, 2, 1, 3).reshape(B * S, Hkv * hd).contiguous() for v in vcs]
        t_new = _timeit(lambda i: K.attn_decode(q, kcs[i], vcs[i], km, nk, H, Hkv, hd, hd ** -0.5, ws=ws), nc)
        t_old = _timeit(lambda i: K.attn_fwd_cross(q, krs[i], vrs[i], B, 1, S, H, Hkv, hd, km, hd ** -0.5), nc)
        rows.append(dict(kernel="attention", shape=f"B {B}, {S} keys, 32/8 heads, hd 128 (splits {K.attn_decode_splits(B, Hkv, S)[0]})",
                         new_us=round(t_new, 1), old_us=round(t_old, 1), new_tbs=round(4.0 * B * Hkv * S * hd / t_new / 1e6, 2),
                         old_tbs=round(4.0 * B * Hkv * S * hd / t_old / 1e6, 2), dispatch="attn_decode", copies=nc))
        del kcs, vcs, krs, vrs
    lg = torch.randn(8, K.pad8(128258), device="cuda").to(torch.bfloat16)
    t_new = _timeit(lambda i: K.argmax_rows(lg, 128258), 1)
    t_old = _timeit(lambda i: lg[:, :128258].float().argmax(-1), 1)
    rows.append(dict(kernel="argmax", shape="8 x 128258 (torch .float().argmax as the comparator)", new_us=round(t_new, 1), old_us=round(t_old, 1),
                     new_tbs=round(16.0 * 128258 / t_new / 1e6, 3), dispatch="argmax_rows", copies=1))
    rows.append(dict(kernel="clock", shape=_clock()))
    return rows


def _composed_step(K, D, model, tc, st, tokens):
    """the decode step from the entries that existed before csrc/decode.hip (gemm_nt at M = B, attn_fwd_cross with Lq = 1)"""
    import torch
    H, Hkv, hd = tc.num_attention_heads, tc.num_key_value_heads, tc.head_dim
    B, S = st["B"], st["S"]
    x = K.gather_rows(model.lm["embed"], tokens.to(torch.int32))
    cos, sin = K.rope_table(st["position"], st["inv_freq"])
    for i, lw in enumerate(model.lm["layers"]):
        n1, _ = K.rmsnorm_fwd(x, lw["ln1"], tc.rms_norm_eps, want_rstd=False)
        qkv = K.rope_apply_(K.gemm_nt(n1, lw["qkv"]), cos, sin, H + Hkv, hd)
        kr, vr = st["rows"][i]
        kr.view(B, S, Hkv * hd)[st["ar"], st["slot"]] = qkv[:, H * hd: (H + Hkv) * hd]
        vr.view(B, S, Hkv * hd)[st["ar"], st["slot"]] = qkv[:, (H + Hkv) * hd:]
        o, _ = K.attn_fwd_cross(qkv, kr, vr, B, 1, S, H, Hkv, hd, st["kmask"], hd ** -0.5)
        x_mid = K.gemm_nt(o, lw["o"], residual=x)
        n2, _ = K.rmsnorm_fwd(x_mid, lw["ln2"], tc.rms_norm_eps, want_rstd=False)
        x = K.gemm_nt(K.swiglu_fwd(K.gemm_nt(n2, lw["gu"])), lw["down"], residual=x_mid)
    nf, _ = K.rmsnorm_fwd(x, model.lm["norm"], tc.rms_norm_eps, want_rstd=False)
    lg = K.gemm_nt(nf, model.lm["head"], ldc=K.pad8(tc.vocab_size))
    st["kmask"][st["ar"], st["slot"]] = 1
    st["slot"] += 1
    st["position"] += 1
    return lg[:, : tc.vocab_size].float().argmax(-1)


def end_to_end(B, path, layers, n_new):
    import torch
    from mantis_amd import decoder as D
    from mantis_amd import generation as G
    from mantis_amd import hip_ops as K
    if path == "skinny":                 # every linear of the step on the weight-streaming kernel, whatever the dispatch table says
        K.SKINNY_MAX_N = 1 << 30
    model, cfg = _model(layers)
    tc = cfg.text_config
    ids, am, pix = _prompt(cfg, B)
    with torch.no_grad():
        t0 = time.perf_counter()
        cache, logits = G.prefill(model, ids, am, pix, n_new)
        torch.cuda.synchronize()
        prefill_ms = (time.perf_counter() - t0) * 1e3
        nxt = K.argmax_rows(logits, tc.vocab_size)
        L, S = cache.L, cache.S_max
        if path == "composed":
            H, Hkv, hd = tc.num_attention_heads, tc.num_key_value_heads, tc.head_dim
            st = dict(B=B, S=S, rows=[(k.permute(0, 2, 1, 3).reshape(B * S, Hkv * hd).contiguous(),
                                       v.permute(0, 2, 1, 3).reshape(B * S, Hkv * hd).contiguous()) for k, v in cache.layers],
                      kmask=cache.kmask.clone(), slot=cache.slot.long().clone(), position=cache.position.clone(),
                      ar=torch.arange(B, device="cuda"), inv_freq=D.inv_freq(tc.head_dim, tc.rope_theta).cuda())
            st["kmask"][:, L:] = 0
            cache.layers = None
            step = lambda t: _composed_step(K, D, model, tc, st, t)
        else:
            step = lambda t: K.argmax_rows(G.decode_step(model, cache, t), tc.vocab_size)
        for _ in range(3):                       # warm-up steps (they are tokens too: the cache keeps growing)
            nxt = step(nxt)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_new - 4):
            nxt = step(nxt)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / (n_new - 4)
        ms_rb = None
        if path != "composed":           # what reading finished-ness back every step costs: the same step + one [B] bool reduction to the host
            cache2, logits = G.prefill(model, ids, am, pix, 40)
            nxt = K.argmax_rows(logits, tc.vocab_size)
            step2 = lambda t: K.argmax_rows(G.decode_step(model, cache2, t), tc.vocab_size)
            res = {}
            for rb in (False, True):
                for _ in range(3):
                    nxt = step2(nxt)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(16):
                    nxt = step2(nxt)
                    if rb and not bool((nxt >= 0).any()):
                        break
                torch.cuda.synchronize()
                res[rb] = (time.perf_counter() - t0) * 1e3 / 16
            ms_rb = round(res[True] - res[False], 3)
    d, I, V = tc.hidden_size, tc.intermediate_size, tc.vocab_size
    wbytes = 2.0 * (layers * ((tc.num_attention_heads + 2 * tc.num_key_value_heads) * tc.head_dim * d + d * d + 3 * I * d) + V * d)
    cbytes = 2.0 * 2 * layers * B * tc.num_key_value_heads * tc.head_dim * (L + n_new / 2)
    return dict(batch=B, path=path, layers=layers, merged_prompt=L, new_tokens=n_new, prefill_ms=round(prefill_ms, 1), ms_per_token=round(ms, 3),
                weight_gb=round(wbytes / 1e9, 2), cache_gb=round(cbytes / 1e9, 3), tbs=round((wbytes + cbytes) / ms / 1e9, 2),
                frac_of_hbm_peak=round((wbytes + cbytes) / ms / 1e9 / HBM_PEAK_TBS, 3),
                frac_of_achievable=round((wbytes + cbytes) / ms / 1e9 / HBM_ACHIEVABLE_TBS, 3), readback_ms_per_token=ms_rb, clock=_clock())


def idefics3_generate(B, layers, n_new, repeats=3, intervals=(1, 4, 8, 16)):
    """`Idefics3ForConditionalGeneration`'s generation loop end to end at the 8B Llama-3 geometry: a prompt of 4 images' worth of <image>
    tokens + 512 text tokens, n_new new tokens.  ms / token = (end of generate - end of prefill) / (n_new - 1), `repeats` times for: no EOS
    (the loop never reads back), then an EOS that never fires read back every k steps.  The rule for generation.EOS_CHECK_EVERY: the
    smallest k whose median lies within the no-EOS loop's own max - min spread of the no-EOS median."""
    import torch
    from mantis_amd import generation as G
    from mantis_amd.configuration_idefics3 import idefics3_8b_llama3
    from mantis_amd.modeling_idefics3 import Idefics3ForConditionalGeneration
    cfg = idefics3_8b_llama3()
    cfg.text_config.num_hidden_layers = layers
    model = Idefics3ForConditionalGeneration(cfg, device="cuda", seed=0)
    model.eval()
    vc = cfg.vision_config
    n_tok = (vc.image_size // vc.patch_size // cfg.scale_factor) ** 2
    n_img, n_text = 4, 512
    g = torch.Generator().manual_seed(1)
    T = n_img * n_tok + n_text
    ids = torch.randint(1, 120000, (B, T), generator=g)
    for j in range(n_img):
        s = 8 + j * (n_tok + 24)
        ids[:, s: s + n_tok] = cfg.image_token_id
    am = torch.ones_like(ids)
    pix = torch.randn(B, n_img, 3, vc.image_size, vc.image_size, generator=g)
    eos = cfg.text_config.vocab_size - 1
    marks = []
    real_prefill = G.prefill

    def timed_prefill(*a, **k):
        r = real_prefill(*a, **k)
        torch.cuda.synchronize()
        marks.append(time.perf_counter())
        return r
    G.prefill = timed_prefill

    def run(**kw):
        t0 = time.perf_counter()
        out = G.generate(model, ids, pixel_values=pix, attention_mask=am, max_new_tokens=n_new, **kw)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if out.shape[1] != T + n_new or bool((out[:, T:] == eos).any()):
            raise SystemExit(f"the EOS {eos} fired: this run does not measure a never-firing EOS")
        return (t1 - marks[-1]) * 1e3 / (n_new - 1), (marks[-1] - t0) * 1e3
    run()                                                                  # warm-up: allocator, first-step checks
    rows = []
    for name, kw in [("no EOS", {})] + [(f"k = {k}", dict(eos_token_id=eos, pad_token_id=cfg.pad_token_id, eos_check_every=k)) for k in intervals]:
        r = [run(**kw) for _ in range(repeats)]
        ms = [x[0] for x in r]
        rows.append(dict(loop=name, ms_per_token=[round(x, 4) for x in ms], median=round(statistics.median(ms), 4),
                         spread=round(max(ms) - min(ms), 4), prefill_ms=round(statistics.median(x[1] for x in r), 1)))
    base = rows[0]
    pick = next((int(r["loop"][4:]) for r in rows[1:] if r["median"] - base["median"] <= base["spread"]), None)
    tc = cfg.text_config
    d, I, V = tc.hidden_size, tc.intermediate_size, tc.vocab_size
    wbytes = 2.0 * (layers * ((tc.num_attention_heads + 2 * tc.num_key_value_heads) * tc.head_dim * d + d * d + 3 * I * d) + V * d)
    cbytes = 2.0 * 2 * layers * B * tc.num_key_value_heads * tc.head_dim * (T + n_new / 2)
    return dict(family="idefics3", batch=B, layers=layers, prompt=T, new_tokens=n_new, rows=rows, smallest_k_within_spread=pick,
                tbs_no_eos=round((wbytes + cbytes) / base["median"] / 1e9, 2), default_in_tree=G.EOS_CHECK_EVERY, clock=_clock())


def _markdown(res):
    out = [f"B = {res['batch']}, {res['layers']} layers, prompt {res['prompt']} tokens, {res['new_tokens']} new tokens; clock: {res['clock']}", "",
           "| loop | ms / token (three repeats) | median | max - min | median - no-EOS median |", "|---|---|---|---|---|"]
    base = res["rows"][0]["median"]
    for r in res["rows"]:
        out.append(f"| {r['loop']} | {', '.join(f'{x:.3f}' for x in r['ms_per_token'])} | {r['median']:.3f} | {r['spread']:.3f} | "
                   f"{r['median'] - base:+.3f} |")
    out += ["", f"no-EOS loop: {res['tbs_no_eos']} TB/s of weights + live cache per token; prefill {res['rows'][0]['prefill_ms']} ms; "
                f"smallest k within the no-EOS spread: {res['smallest_k_within_spread']}"]
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", choices=("llava", "idefics3"), default="llava")
    ap.add_argument("--markdown", action="store_true", help="--family idefics3: print the table as markdown after the JSON line")
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--path", choices=("new", "skinny", "composed"), default="new")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--limit", type=int, default=240, help="seconds per child process of --all")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.all:
        res = []
        jobs = [["--kernels"]] + [["--batch", str(B), "--path", p] for B in (1, 8) for p in ("new", "skinny", "composed")]
        for j in jobs:
            cmd = [sys.executable, os.path.abspath(__file__), *j, "--layers", str(a.layers), "--new-tokens", str(a.new_tokens)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
            if r.returncode != 0:
                print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
                raise SystemExit(f"{' '.join(j)} failed with status {r.returncode}: nothing more is started")
            line = [l for l in r.stdout.splitlines() if l.startswith("{") or l.startswith("[")][-1]
            res.append(json.loads(line))
            print(line, flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        return
    if a.family == "idefics3":
        res = idefics3_generate(a.batch, a.layers, a.new_tokens)
        print(json.dumps(res), flush=True)
        if a.markdown:
            print(_markdown(res), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        return
    print(json.dumps(kernels() if a.kernels else end_to_end(a.batch, a.path, a.layers, a.new_tokens)), flush=True)


if __name__ == "__main__":
    main()
