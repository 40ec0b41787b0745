"""Build libnrms_hip.so in-tree for gfx950 (hipcc cross-compiles without a GPU).

    python -m newsrecommendationsystem_amd.build [--force]

The .so lands next to this file so it travels to the GPU box with the repo
snapshot (it is git-ignored, not gpurun-ignored).
"""
import argparse
import concurrent.futures as cf
import os
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
INCLUDE = os.path.join(ROOT, "include")
OBJ = os.path.join(PKG, "_build")
LIB = os.path.join(PKG, "libnrms_hip.so")
SOURCES = ["gather.hip", "gemm_f32.hip", "proj_x6.hip", "attention.hip", "news_fused.hip", "user_fused.hip", "score.hip", "eval.hip", "topk.hip", "views.hip", "train.hip", "fedavg.hip", "fit.hip","embed_sort.hip", "tsv_io.hip", "capi.hip"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"
FLAGS = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-I", INCLUDE, "-I", CSRC,
         "-Wall", "-Wno-unused-function"]
# Per-file machine-scheduler strategy (measured in A/B runs on one box, bench
# workload): the x6 projection GEMM is 2 % faster under max-ILP. The news
# kernel ran 2.5 % faster under the iterative ILP scheduler until round 3;
# since the token-compaction rewrite that scheduler spills ~45 registers
# (scratch reloads inside the B epilogue) where the default spills 7 outside
# the hot phases, so the news kernel took the default; after the round-4
# pipeline changes max-ILP is 0.9 % faster end to end (news_fused -3.7 us,
# 44 B of scratch per lane against 8; profiles/r4r2_news_sched_ab.txt).
# Round 6 re-check (profiles/r6/r7k_sched_strategy_ab.txt, r7l_user_maxilp_ab.txt,
# same box x3 each): news_fused under the default scheduler and proj_x6 under
# max-ILP within noise; the UserEncoder under max-ILP user_fused -0.7..-1.4 %
# but the graph-replayed step +0.25 % / -0.2 % -- not taken.
FILE_FLAGS = {
    "gemm_f32.hip": ["-mllvm", "-amdgpu-sched-strategy=max-ilp"],
    "news_fused.hip": ["-mllvm", "-amdgpu-sched-strategy=max-ilp"],
}


def _newer(src_paths, dst):
    if not os.path.exists(dst):
        return True
    t = os.path.getmtime(dst)
    return any(os.path.getmtime(p) > t for p in src_paths)


def _deps():
    # every header of csrc/ (a source whose header changed must recompile: a
    # stale object compiled against an older struct layout links silently)
    hdrs = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".h")))
    return hdrs + [os.path.join(INCLUDE, "nrms_hip.h"), os.path.abspath(__file__)]   # flag changes rebuild too


def build(force=False, verbose=True):
    os.makedirs(OBJ, exist_ok=True)
    jobs = []
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(OBJ, s.replace(".hip", ".o"))
        if force or _newer([src] + _deps(), obj):
            jobs.append((src, obj))

    def compile_one(job):
        src, obj = job
        cmd = [HIPCC] + FLAGS + FILE_FLAGS.get(os.path.basename(src), []) + ["-c", src, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for {src}:\n{r.stdout}\n{r.stderr}")
        return src, r.stderr

    with cf.ThreadPoolExecutor(max_workers=min(8, max(1, len(jobs)))) as ex:
        for src, err in ex.map(compile_one, jobs):
            if verbose:
                print(f"[nrms build] compiled {os.path.basename(src)}")
                if err.strip():
                    print(err)
    objs = [os.path.join(OBJ, s.replace(".hip", ".o")) for s in SOURCES]
    if force or jobs or _newer(objs, LIB):
        tmp = LIB + ".tmp"
        cmd = [HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", tmp] + objs
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")
        os.replace(tmp, LIB)
        if verbose:
            print(f"[nrms build] linked {LIB}")
    return LIB


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--force", action="store_true")
    a = ap.parse_args()
    build(force=a.force)
    sys.exit(0)
