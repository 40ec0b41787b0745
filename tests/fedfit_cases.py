"""Splits, a CPU scorer and the child-process launcher shared by
tests/test_fedfit_cpu.py, tests/test_gpu_fedfit.py and their worker
(tests/fedfit_worker.py)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import torch

from newsrecommendationsystem_amd import data as Dt
from tests import fit_cases as FC

F = FC.F
ROOT = FC.ROOT
WORKER = os.path.join(ROOT, "tests", "fedfit_worker.py")
S, N_USERS, N_NEWS, V, N_CLICKED = 40, 11, 60, 500, 50


def make_split(directory, seed=5):
    """directory/train: 40 samples of 11 users U0..U10 (sample k is user
    U{k % 11}, so every user has several samples), 1 + K = 3, V = 500;
    directory/val: a raw split of 30 impressions of 9 users over the same
    vocabulary."""
    tr = os.path.join(str(directory), "train")
    Dt.synthetic_train_split(tr, seed=seed, n_samples=S, n_news=N_NEWS, V=V, K=2)
    path = os.path.join(tr, "behaviors_parsed.tsv")
    lines = open(path).read().splitlines()
    out = [lines[0]]
    for k, ln in enumerate(lines[1:]):
        out.append(f"U{k % N_USERS}\t" + ln.split("\t", 1)[1])
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")
    Dt.synthetic_split(os.path.join(str(directory), "val"), seed=seed + 1, n_news=N_NEWS, n_users=9,
                       n_impressions=30, V=V)
    return str(directory)


def train_set(directory, device="cpu"):
    tr = os.path.join(str(directory), "train")
    corpus = Dt.read_news_parsed(os.path.join(tr, "news_parsed.tsv"))
    return F.TrainSet(os.path.join(tr, "behaviors_parsed.tsv"), corpus, device=device)


def config(dropout=0.0, hip=False, **fields):
    """The reference's layout (300-d, 15 heads, 200-d query) over V = 500."""
    from newsrecommendationsystem_amd import NRMSConfig
    return type("FedCfg", (NRMSConfig,), dict(num_words=V, dropout_probability=dropout, hip_train=hip, **fields))


def model(cfg, seed=0, device="cpu"):
    from newsrecommendationsystem_amd import NRMS
    torch.manual_seed(seed)
    return NRMS(cfg).to(device)


def flat_params(m):
    return torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu().numpy()


@torch.no_grad()
def cpu_score_plan(m, plan):
    """evaluate.score_plan restated on the CPU (ATen encoders in eval mode,
    the oracle's per-impression metrics): (scores, metrics [n_imp, 4] fp64)."""
    from newsrecommendationsystem_amd import train as TR
    from oracle import metrics as M
    titles = torch.from_numpy(np.concatenate([plan.corpus.titles, np.zeros((1, plan.corpus.titles.shape[1]), np.int64)]))
    news = TR.news_encode_autograd(m.news_encoder, titles, training=False)
    news[-1] = 0                                                    # PADDED_NEWS: the zero vector
    users = TR.user_encode_autograd(m.user_encoder, news[torch.from_numpy(plan.hist_rows.astype(np.int64))])
    cand = torch.from_numpy(plan.cand.astype(np.int64))
    scores = (news[cand] * users[torch.from_numpy(plan.pair_user.astype(np.int64))]).sum(-1)
    s, off = scores.double().numpy(), plan.offsets
    rows = [M.single_impression(np.asarray(plan.labels[off[i]:off[i + 1]]), s[off[i]:off[i + 1]])
            for i in range(plan.n_impressions)]
    return scores, torch.tensor(np.array(rows, dtype=np.float64).reshape(-1, 4))


CPU_THREADS = 2


class cpu_threads:
    """The CPU workers' thread count in this process for a while: ATen's
    reductions are then split as theirs are, and results compare bitwise."""

    def __enter__(self):
        self.prev = torch.get_num_threads()
        torch.set_num_threads(CPU_THREADS)

    def __exit__(self, *exc):
        torch.set_num_threads(self.prev)
        return False


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def run_workers(out, job, world=2, backend="gloo", device="cpu", timeout=240):
    """One child process per rank running tests/fedfit_worker.py on `job` (a
    dict, written to out/job.json); returns each rank's result dict. Every
    child has a time limit and is killed when another fails."""
    with open(os.path.join(str(out), "job.json"), "w") as f:
        json.dump(job, f)
    port = free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        if device == "cpu":       # no GPU; a few threads per rank (cpu_threads() gives a hand loop the same)
            env.update(HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", OMP_NUM_THREADS=str(CPU_THREADS),
                       MKL_NUM_THREADS=str(CPU_THREADS))
        procs.append(subprocess.Popen([sys.executable, "-u", WORKER, str(out), backend, device], env=env, cwd=ROOT,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = []
    try:
        for p in procs:
            o, _ = p.communicate(timeout=timeout)
            logs.append(o)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, o in zip(procs, logs):
        assert p.returncode == 0, o[-3000:]
    return [json.load(open(os.path.join(str(out), f"rank{r}.json"))) for r in range(world)]
