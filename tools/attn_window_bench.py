#!/usr/bin/env python3
"""Sliding-window attention micro-benchmark at Mistral's shape (L = 8192, 32/8 heads x 128, B = 1 and 2): HIP-event time of the forward
and of the whole backward for three variants, alternated round by round in one process --
  causal   full causal attention (mantis_attn_fwd / _bwd);
  window   W = 4096 through the window kernels (mantis_attn_fwd_window / _bwd_window: the band, bounds computed in the kernels);
  bounds   W = 4096 written as kstart[q] = q - W + 1 / qend[k] = k + W arrays on the plain causal kernels (the cheap alternative);
plus each variant's visible score pairs (W = L/2: 0.75 of causal).   `python tools/attn_window_bench.py [iters] [rounds] [--out FILE]`"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from mantis_amd import hip_ops as K  # noqa: E402


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if out_path in args:
        args.remove(out_path)
    it = int(args[0]) if args else 10
    rounds = int(args[1]) if len(args) > 1 else 3
    L, H, Hkv, hd, W = 8192, 32, 8, 128, 4096
    scale = hd ** -0.5
    rows = []
    for B in (1, 2):
        g = torch.Generator(device="cuda").manual_seed(B)
        qkv = torch.randn(B * L, (H + 2 * Hkv) * hd, generator=g, device="cuda").to(torch.bfloat16)
        do = torch.randn(B * L, H * hd, generator=g, device="cuda").to(torch.bfloat16)
        pos = torch.arange(L, device="cuda", dtype=torch.int32)
        kstart = (pos - W + 1).clamp(min=0)[None].expand(B, L).contiguous()
        qend = (pos + W).clamp(max=L)[None].expand(B, L).contiguous()
        variants = {
            "causal": (dict(), dict()),
            "window": (dict(window=W), dict(window=W)),
            "bounds": (dict(kstart=kstart), dict(kstart=kstart, qend=qend)),
        }
        band = int(torch.clamp(pos + 1, max=W).sum())
        pairs = {"causal": L * (L + 1) // 2, "window": band, "bounds": band}
        state = {}
        for name, (fk, bk) in variants.items():
            o, lse = K.attn_fwd(qkv, B, L, H, Hkv, hd, None, scale, True, **fk)
            K.attn_bwd(qkv, o, do, lse, B, L, H, Hkv, hd, None, scale, True, **bk)
            state[name] = (o, lse)
        torch.cuda.synchronize()
        wo, bo = state["window"][0].float(), state["bounds"][0].float()
        diff = float((wo - bo).norm() / bo.norm())

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(it):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / it * 1e3
        times = {n: ([], []) for n in variants}
        for _ in range(rounds):
            for name, (fk, bk) in variants.items():
                o, lse = state[name]
                times[name][0].append(timed(lambda: K.attn_fwd(qkv, B, L, H, Hkv, hd, None, scale, True, **fk)))
                times[name][1].append(timed(lambda: K.attn_bwd(qkv, o, do, lse, B, L, H, Hkv, hd, None, scale, True, **bk)))
        base_f, base_b = min(times["causal"][0]), min(times["causal"][1])
        for name in variants:
            tf, tb = min(times[name][0]), min(times[name][1])
            rows.append(dict(B=B, L=L, H=H, Hkv=Hkv, hd=hd, W=None if name == "causal" else W, variant=name, fwd_us=round(tf, 1),
                             bwd_us=round(tb, 1), fwd_vs_causal=round(tf / base_f, 3), bwd_vs_causal=round(tb / base_b, 3),
                             visible_pairs_vs_causal=round(pairs[name] / pairs["causal"], 4),
                             fwd_us_rounds=[round(t, 1) for t in times[name][0]], bwd_us_rounds=[round(t, 1) for t in times[name][1]]))
            print(f"B={B} {name:7s} fwd {tf:8.1f} us ({tf / base_f:5.3f}x causal)  bwd {tb:8.1f} us ({tb / base_b:5.3f}x causal)  "
                  f"visible pairs {pairs[name] / pairs['causal']:.4f} of causal", flush=True)
        print(f"B={B} window vs bounds forward output rel-L2 {diff:.2e}", flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), iters=it, rounds=rounds, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
