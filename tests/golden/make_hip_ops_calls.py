"""Records tests/golden/hip_ops_calls.json: the words the GEMM-family wrappers of mantis_amd/hip_ops.py hand to libmantis_hip.so -- every entry
that takes a flag word or leaves a timer record, under the neutral LaunchContext and under LaunchContext(gemm_cus=240, shared_gpu=True).  No GPU:
for the duration of `record()` the library handle `hip_ops._L` is an object that logs (entry, every int / float / None argument, "<ptr>" for the
rest) and returns 0 (or the codes a case queues: -2 = the library declines), and `_p`, `_stream`, `_chk2d`, `_gemm_workspace` are trivial
stand-ins, so the wrappers run unchanged on CPU tensors; the five names are restored on return.  The sum-of-squares collector is a stand-in
whose take / give_back land in the same log, which pins their order around a declined launch.
`python tests/golden/make_hip_ops_calls.py` rewrites the fixture: do that only on a commit whose flag words are known good (the first recording
came from the wrappers as they stood before the flag bits had names in Python; tests/test_cabi_exports.py holds the wrappers to it)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIXTURE = os.path.join(ROOT, "tests", "golden", "hip_ops_calls.json")
PATCHED = ("_L", "_p", "_stream", "_chk2d", "_gemm_workspace")


class Library:
    """Stands for the ctypes handle: any entry can be called; `declines` queues return codes per entry (default 0)."""

    def __init__(self):
        self.log, self.declines = [], {}

    def __getattr__(self, entry):
        def call(*args):
            self.log.append([entry] + [a if a is None or isinstance(a, (int, float)) else "<ptr>" for a in args])
            queued = self.declines.get(entry)
            return queued.pop(0) if queued else 0
        return call


class Collector:
    """Stands for optim.FusedAdamW.begin_fold(): hands out a slot per take (None from the `refuse_from`-th take on)."""

    def __init__(self, log, refuse_from=None):
        self.log, self.refuse_from, self.takes = log, refuse_from, 0

    def take(self, grad, tiles):
        self.takes += 1
        ok = self.refuse_from is None or self.takes < self.refuse_from
        self.log.append(["take", list(grad.shape), tiles, ok])
        return "<slot>" if ok else None

    def give_back(self, grad, tiles):
        self.log.append(["give_back", list(grad.shape), tiles])


def _cases(k, torch):
    """(name, callable(lib, ctx_kwargs)) in a fixed order; every callable runs under its own LaunchContext."""
    bf = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32)
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    a, b, bias, res = bf(300, 72), bf(200, 72), bf(200), bf(300, 208)
    at, bt = bf(72, 300), bf(72, 200)
    cases = []

    def case(name, fn, declines=None, collector=None):
        cases.append((name, fn, declines or {}, collector))

    case("gemm_nt", lambda: k.gemm_nt(a, b))
    case("gemm_nt bias", lambda: k.gemm_nt(a, b, bias=bias))
    for act in ("gelu", "gelu_pytorch_tanh", "quick_gelu"):
        case(f"gemm_nt bias {act}", lambda act=act: k.gemm_nt(a, b, bias=bias, act=act))
    case("gemm_nt residual", lambda: k.gemm_nt(a, b, residual=res))
    case("gemm_nt bias gelu residual", lambda: k.gemm_nt(a, b, bias=bias, act="gelu", residual=res))
    case("gemm_nt accumulate", lambda: k.gemm_nt(a, b, out=bf(300, 200), accumulate=True))
    case("gemm_nt a_kmajor", lambda: k.gemm_nt(at, b, a_kmajor=True))
    case("gemm_nt b_kmajor", lambda: k.gemm_nt(a, bt, b_kmajor=True))
    case("gemm_nt both kmajor accumulate", lambda: k.gemm_nt(at, bt, out=bf(300, 200), accumulate=True, a_kmajor=True, b_kmajor=True))
    case("gemm_nt variant 14", lambda: k.gemm_nt(a, b, variant=14))
    case("gemm_nt cus 97", lambda: k.gemm_nt(a, b, cus=97))
    case("gemm_nt cus 0", lambda: k.gemm_nt(a, b, cus=0))
    case("gemm_nt sk_inkernel", lambda: k.gemm_nt(a, b, variant=13, sk_inkernel=True))
    case("gemm_nt n_valid ldc", lambda: k.gemm_nt(a, b, n_valid=193, ldc=200))
    case("gemm_nt k", lambda: k.gemm_nt(a, b, k=64))

    x, w_gu = bf(333, 64), bf(256, 64)
    case("linear_gu_swiglu fused", lambda: k.linear_gu_swiglu(x, w_gu))
    case("linear_gu_swiglu declined", lambda: k.linear_gu_swiglu(x, w_gu), {"mantis_gemm_bf16_nt_fused": [-2]})
    case("linear_gu_swiglu variant|64", lambda: k.linear_gu_swiglu(x, w_gu, variant=14 | 64))
    case("linear_gu_swiglu N%256", lambda: k.linear_gu_swiglu(x, bf(384, 64)))
    w_qkv, qb, cos, sin = bf(512, 64), bf(512), bf(333, 64), bf(333, 64)
    case("linear_qkv_rope fused", lambda: k.linear_qkv_rope(x, w_qkv, qb, cos, sin, 3, 128))
    case("linear_qkv_rope fused no bias", lambda: k.linear_qkv_rope(x, w_qkv, None, cos, sin, 3, 128))
    case("linear_qkv_rope declined", lambda: k.linear_qkv_rope(x, w_qkv, qb, cos, sin, 3, 128), {"mantis_gemm_bf16_nt_fused": [-2]})
    case("linear_qkv_rope variant|64", lambda: k.linear_qkv_rope(x, w_qkv, qb, cos, sin, 3, 128, variant=15 | 64))
    case("linear_qkv_rope hd 64", lambda: k.linear_qkv_rope(x, w_qkv, qb, bf(333, 32), bf(333, 32), 6, 64))

    w_down, gu = bf(64, 176), bf(333, 352)
    case("linear_dx_swiglu", lambda: k.linear_dx_swiglu(x, w_down, gu))
    case("linear_dx_swiglu variant sk_inkernel", lambda: k.linear_dx_swiglu(x, w_down, gu, variant=14, sk_inkernel=True))

    dy, xa = bf(512, 264)[:, :260], bf(512, 256)
    for acc in (False, True):
        case(f"linear_dw acc={acc}", lambda acc=acc: k.linear_dw(dy, xa, bf(256, 256), acc))
        case(f"linear_dw collector acc={acc}", lambda acc=acc: k.linear_dw(dy, xa, bf(256, 256), acc), collector=0)
    case("linear_dw collector declined", lambda: k.linear_dw(dy, xa, bf(256, 256), True), {"mantis_gemm_bf16_nt_sumsq": [-2]}, collector=0)
    case("linear_dw collector refuses", lambda: k.linear_dw(dy, xa, bf(256, 256), False), collector=1)
    case("linear_dw collector ragged", lambda: k.linear_dw(bf(512, 300), bf(512, 520), bf(300, 520), False), collector=0)

    dy2, x2 = bf(512, 520), bf(512, 768)
    pair = lambda acc=False: k.linear_dw_pair(dy, xa, bf(256, 256), dy2, x2, bf(515, 768), acc)
    case("linear_dw_pair", pair)
    case("linear_dw_pair acc", lambda: pair(True))
    case("linear_dw_pair collector", pair, collector=0)
    case("linear_dw_pair collector acc", lambda: pair(True), collector=0)
    case("linear_dw_pair declined", pair, {"mantis_gemm_bf16_tn_pair": [-2]})
    case("linear_dw_pair collector declined", pair, {"mantis_gemm_bf16_tn_pair": [-2]}, collector=0)
    case("linear_dw_pair collector declined twice", pair, {"mantis_gemm_bf16_tn_pair": [-2], "mantis_gemm_bf16_nt_sumsq": [-2, 0]}, collector=0)
    case("linear_dw_pair collector refuses the second", pair, collector=2)
    case("linear_dw_pair collector refuses the first", pair, collector=1)
    case("linear_dw_pair shape mismatch", lambda: k.linear_dw_pair(dy, xa, bf(256, 256), bf(512, 520), bf(512, 200), bf(515, 200), False))
    case("linear_dw_pair shape mismatch collector", lambda: k.linear_dw_pair(dy, xa, bf(256, 256), bf(512, 520), bf(512, 200), bf(515, 200), True),
         collector=0)

    a8, b8, one = u8(300, 256), u8(112, 256), f32(1)
    case("gemm_fp8_nt", lambda: k.gemm_fp8_nt(a8, one, b8, one))
    case("gemm_fp8_nt e5m2 bias residual accumulate variant", lambda: k.gemm_fp8_nt(a8, one, b8, one, fmt_a=k.FP8_E5M2, bias=bf(112), residual=bf(300, 120),
                                                                                  out=bf(300, 112), accumulate=True, variant=2, k=240))
    case("gemm_fp8_nt rowwise", lambda: k.gemm_fp8_nt(a8, f32(300), b8, f32(112), rowwise=True))
    case("gemm_fp8_nt rowwise bias", lambda: k.gemm_fp8_nt(a8, f32(300), b8, f32(112), bias=bf(112), rowwise=True))
    case("gemm_fp8_dx_swiglu", lambda: k.gemm_fp8_dx_swiglu(a8, one, b8, one, bf(300, 224)))

    xs, ws = bf(3, 72), bf(200, 72)
    case("linear_skinny", lambda: k.linear_skinny(xs, ws))
    case("linear_skinny bias residual n_valid ldc", lambda: k.linear_skinny(xs, ws, bias=bf(200), residual=bf(3, 208), n_valid=193, ldc=200))
    case("linear_decode 16 rows", lambda: k.linear_decode(bf(16, 72), ws, bias=bf(200)))
    case("linear_decode 17 rows", lambda: k.linear_decode(bf(17, 72), ws, bias=bf(200)))
    wide = bf(16384, 8)
    case("linear_decode 16383 weight rows", lambda: k.linear_decode(xs[:, :8], wide, residual=bf(3, 16384), n_valid=16383, ldc=16384))
    case("linear_decode 16384 weight rows", lambda: k.linear_decode(xs[:, :8], wide, residual=bf(3, 16384)))
    return cases


def record(k):
    """Run every case under both contexts against the stand-ins; `k` is the imported mantis_amd.hip_ops."""
    import torch
    assert k.FUSE_FWD_EPILOGUES, "recorded with the fused forward epilogues on (MANTIS_NO_FUSE unset)"
    saved = {n: getattr(k, n) for n in PATCHED}
    lib = Library()
    k._L = lib
    k._p = lambda t: None if t is None else "<ptr>"
    k._stream = lambda: "<stream>"
    k._chk2d = lambda t, name: None
    k._gemm_workspace = lambda: ("<ws>", 1 << 20)
    out = {}
    try:
        for ctx_name, kw in (("neutral", {}), ("cus240_shared", dict(gemm_cus=240, shared_gpu=True))):
            rows = out[ctx_name] = []
            for name, fn, declines, refuse_from in _cases(k, torch):
                lib.log, lib.declines = [], {e: list(v) for e, v in declines.items()}
                col = None if refuse_from is None else Collector(lib.log, refuse_from or None)
                with k.launch_context(k.LaunchContext(dw_sumsq=col, **kw)):
                    fn()
                assert not any(lib.declines.values()), f"{name}: a queued return code was not consumed"
                rows.append({"case": name, "calls": lib.log})
    finally:
        for n, v in saved.items():
            setattr(k, n, v)
    return json.loads(json.dumps(out))


def write(table, path):
    """One line per call, so that a changed word shows as a one-line diff."""
    with open(path, "w") as f:
        f.write("{\n")
        for i, (ctx, rows) in enumerate(table.items()):
            f.write(f"{json.dumps(ctx)}: [\n")
            f.write(",\n".join(' {"case": %s, "calls": [\n  %s]}' % (json.dumps(r["case"]), ",\n  ".join(json.dumps(c) for c in r["calls"])) for r in rows))
            f.write("\n]" + (",\n" if i + 1 < len(table) else "\n"))
        f.write("}\n")
    with open(path) as f:
        assert json.load(f) == table


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from mantis_amd import hip_ops
    write(record(hip_ops), sys.argv[1] if len(sys.argv) > 1 else FIXTURE)
