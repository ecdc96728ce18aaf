"""Records tests/golden/gemm_plan.json: every decision of the bf16 GEMM planner (mantis_amd/csrc/gemm_plan.h) as tools/gemm_plan_dump.cpp prints
it -- the full sweep with the default environment, the reduced sweep once per value of each MANTIS_GEMM_* switch (a process each: the switches
are read once).  Host compiler only, no GPU.  `python tests/golden/make_gemm_plan.py` rewrites the fixture: do that only on a commit whose
decisions are known good (profiles/gemm_plan_refactor.md: the first recording came from the planner as it stood inside gemm.hip)."""
import json
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIXTURE = os.path.join(ROOT, "tests", "golden", "gemm_plan.json")
ENV = [("MANTIS_GEMM_CUS", "97"), ("MANTIS_GEMM_CUS", "200"), ("MANTIS_GEMM_SPLIT_MAX", "2"), ("MANTIS_GEMM_SPLIT_MAX", "4"),
       ("MANTIS_GEMM_SK_BALANCED", "0"), ("MANTIS_GEMM_SK_FINISH", "0"), ("MANTIS_GEMM_176", "0"), ("MANTIS_GEMM_176", "2"),
       ("MANTIS_GEMM_RING", "12"), ("MANTIS_GEMM_RING", "13"), ("MANTIS_GEMM_RING", "14"), ("MANTIS_GEMM_PAIR", "0"), ("MANTIS_GEMM_PAIR", "2")]


def compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    raise RuntimeError("no C++ compiler found (CXX, c++, g++, clang++): the planner's dump program cannot be built")


def build(out_dir, extra=()):
    exe = os.path.join(out_dir, "gemm_plan_dump")
    subprocess.run([compiler(), "-std=c++17", "-O1", *extra, os.path.join(ROOT, "tools", "gemm_plan_dump.cpp"), "-o", exe], check=True)
    return exe


def run_text(exe, reduced=False, env=None):
    base = {k: v for k, v in os.environ.items() if not k.startswith("MANTIS_GEMM_")}
    return subprocess.run([exe] + (["reduced"] if reduced else []), env={**base, **(env or {})}, capture_output=True, text=True, check=True).stdout


def run(exe, reduced=False, env=None):
    return json.loads(run_text(exe, reduced, env))


def row(table, M, N, K, budget):
    """One recorded row as a dict (see tools/gemm_plan_dump.cpp for the fields)."""
    if budget in table["budgets"] and f"{M},{N}" in table["rows"] and str(K) in table["rows"][f"{M},{N}"]:
        text = table["rows"][f"{M},{N}"][str(K)][table["budgets"].index(budget)]
    else:
        text = table["more"][f"{M},{N},{K},{budget}"]
    f = text.split()
    names = ("pick", "S", "full", "rem", "units", "tails", "nwg")
    return {**{n: int(v) for n, v in zip(names, f)}, "digest": f[7], "needs_ws": f[8] == "1", "grid12": int(f[9]), "grid14": int(f[10]), "entries": f[11]}


def write(exe, path):
    """The fixture is the dump's own text (one line per (M, N)), the default run and one reduced run per switch value."""
    with open(path, "w") as f:
        f.write('{"default": ' + run_text(exe).strip() + ',\n"env": {\n')
        f.write(",\n".join(json.dumps(f"{k}={v}") + ": " + run_text(exe, True, {k: v}).strip() for k, v in ENV))
        f.write("\n}}\n")
    with open(path) as f:
        json.load(f)


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        write(build(d), sys.argv[1] if len(sys.argv) > 1 else FIXTURE)
