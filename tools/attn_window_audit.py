#!/usr/bin/env python3
"""Build audit of the sliding-window attention kernels (no GPU needed):
  1. every attention kernel that exists in the base revision's attn.hip / attn_fwd64.hip compiles to the SAME instructions from this tree
     (device code of both sources compiled with the build's flags, disassembled per kernel symbol, addresses stripped);
  2. every *_win_kernel: registers, scratch and spills from -Rpass-analysis=kernel-resource-usage -- no scratch, no VGPR spill.
`python tools/attn_window_audit.py [BASE_REV] [--sources gemm,gemm176]`  (default HEAD~1; give the revision before the window kernels).
With --sources the same comparison runs over other translation units -- a refactor that must not move an instruction -- and step 2 becomes:
every kernel's register, AGPR, scratch and spill figures equal the base revision's."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mantis_amd.build import EXTRA_FLAGS, FLAGS, _hipcc  # noqa: E402

LLVM = "/opt/rocm/llvm/bin"
SOURCES = ("attn", "attn_fwd64")


def compile_device(csrc, name, out_dir):
    co = os.path.join(out_dir, name + ".co")
    r = subprocess.run([_hipcc(), *FLAGS, *EXTRA_FLAGS.get(name, []), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(csrc, name + ".hip"), "-o", co], capture_output=True, text=True, check=True)
    elf = os.path.join(out_dir, name + ".elf")
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + co,
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + elf], check=True)
    return elf, r.stderr


def kernels(elf):
    out = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", elf], capture_output=True,
                         text=True, check=True).stdout
    cur, res = None, {}
    for line in out.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", line)
        if m:
            cur = m.group(1)
            res[cur] = []
        elif cur and line.strip():
            ins = re.sub(r"//.*", "", line).strip()
            # s_getpc_b64 + s_add_u32 <literal>: the distance from here to a function or table elsewhere in the code object -- an address, which
            # moves with the order the kernels are emitted in, not an instruction
            if res[cur] and res[cur][-1].startswith("s_getpc_b64") and ins.startswith("s_add_u32"):
                ins = re.sub(r"0x[0-9a-f]+$", "<pc-relative>", ins)
            res[cur].append(ins)
    return {k: hashlib.sha1("\n".join(v).encode()).hexdigest() for k, v in res.items()}


def resources(log):
    res, cur = {}, None
    for line in log.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            res[cur] = {}
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur:
            res[cur][m.group(1).strip()] = int(m.group(2))
    return res


def main():
    args = sys.argv[1:]
    sources = SOURCES
    if "--sources" in args:
        i = args.index("--sources")
        sources = tuple(args[i + 1].split(","))
        del args[i:i + 2]
    base = args[0] if args else "HEAD~1"
    tmp = tempfile.mkdtemp()
    base_dir = os.path.join(tmp, "base")
    os.makedirs(base_dir)
    arch = subprocess.run(["git", "-C", ROOT, "archive", base, "mantis_amd/csrc", "include"], capture_output=True, check=True).stdout
    subprocess.run(["tar", "-x", "-C", base_dir], input=arch, check=True)
    ok = True
    for name in sources:
        b_elf, b_log = compile_device(os.path.join(base_dir, "mantis_amd", "csrc"), name, base_dir)
        n_elf, log = compile_device(os.path.join(ROOT, "mantis_amd", "csrc"), name, tmp)
        b, n = kernels(b_elf), kernels(n_elf)
        same = [k for k in b if n.get(k) == b[k]]
        diff = [k for k in b if k not in same]
        print(f"{name}.hip: {len(b)} kernels of {base}: {len(same)} identical, {len(diff)} differ or missing; {len(set(n) - set(b))} new")
        for k in diff:
            print(f"  DIFFERS: {k}")
        ok &= not diff
        if sources != SOURCES:
            b_res, n_res = resources(b_log), resources(log)
            moved = [k for k in b_res if n_res.get(k) != b_res[k]]
            print(f"  resource usage (VGPRs, AGPRs, scratch, spills, occupancy, LDS): {len(b_res) - len(moved)} kernels unchanged, {len(moved)} changed")
            for k in moved:
                print(f"  CHANGED: {k}: {b_res[k]} -> {n_res.get(k)}")
            ok &= not moved
            continue
        for k, r in sorted(resources(log).items()):
            if "win_kernel" not in k:
                continue
            bad = r.get("ScratchSize") != 0 or r.get("VGPRs Spill") != 0
            ok &= not bad
            print(f"  {'BAD ' if bad else ''}{k}: VGPRs {r.get('VGPRs')} AGPRs {r.get('AGPRs')} scratch {r.get('ScratchSize')} B "
                  f"VGPR spill {r.get('VGPRs Spill')} SGPR spill {r.get('SGPRs Spill')} occupancy {r.get('Occupancy')}")
    print("OK" if ok else "FAILED")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
