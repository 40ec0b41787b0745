"""The command line of the training path, `python -m
newsrecommendationsystem_amd.train` (train.py hands over to _main, whose
docstring lists the modes). Nothing here is imported by the library."""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch
import torch.distributed as dist

from .config import NRMSConfig
from .data import read_news_parsed, synthetic_split, synthetic_train_split
from .distributed import init_from_env
from .fit import ImpressionSet, TrainSet, fit
from .nrms import NRMS
from .quality import resample_vs_static
from .train import FedAvg, make_optimizer, synthetic_train_batches, train_step


def _max_token_id(path):
    t = read_news_parsed(path).titles
    return int(t.max()) if t.size else 0


def _fit_main(a):
    """The DIR form of the command line: src/train.py's train() on DIR/train
    (behaviors_parsed.tsv, news_parsed.tsv, optionally
    pretrained_word_embedding.npy) validated on DIR/val (behaviors.tsv,
    news_parsed.tsv); one JSON line."""
    rank, world, _, dev, group = _fed_setup(a)
    tr, va = os.path.join(a.dir, "train"), os.path.join(a.dir, "val")
    corpus = read_news_parsed(os.path.join(tr, "news_parsed.tsv"))
    try:                                       # src/train.py:76-80
        emb = torch.from_numpy(np.load(os.path.join(tr, "pretrained_word_embedding.npy"))).float()
        V = emb.shape[0]
    except FileNotFoundError:
        emb = None
        V = int(corpus.titles.max()) + 1 if corpus.titles.size else 1
        if os.path.exists(os.path.join(va, "news_parsed.tsv")):
            V = max(V, _max_token_id(os.path.join(va, "news_parsed.tsv")) + 1)
    has_val = os.path.exists(os.path.join(va, "behaviors.tsv"))

    class Cfg(NRMSConfig):
        num_words = V
        hip_train = not a.aten
        num_epochs = a.epochs if a.epochs is not None else NRMSConfig.num_epochs
        num_batches_validate = (a.validate_every if a.validate_every is not None
                                else NRMSConfig.num_batches_validate)
    if a.negatives == "resample":              # raw behaviors.tsv, negatives drawn per (seed, epoch) on the device
        k = Cfg.negative_sampling_ratio if a.k is None else a.k
        ts = ImpressionSet(os.path.join(tr, "behaviors.tsv"), corpus, k=k, num_clicked=Cfg.num_clicked_news_a_user,
                           device="cpu" if a.export_epoch is not None else dev)
        if a.export_epoch is not None:
            ts.export_epoch(a.export_epoch[1], a.seed, int(a.export_epoch[0]))
            print(json.dumps({"mode": "export", "epoch": int(a.export_epoch[0]), "path": a.export_epoch[1],
                              "samples": len(ts), "n_dropped": ts.n_dropped, "k": k}))
            return
        if rank == 0:
            print(f"Load training dataset with size {len(ts)} ({ts.n_dropped} positives dropped: their impression "
                  f"has fewer than {k} negatives).", flush=True)
    else:
        if a.export_epoch is not None or a.k is not None:
            raise SystemExit("--export-epoch and --k go with --negatives resample")
        ts = TrainSet(os.path.join(tr, "behaviors_parsed.tsv"), corpus,
                      num_clicked=Cfg.num_clicked_news_a_user, device=dev)
        if rank == 0:
            print(f"Load training dataset with size {len(ts)}.", flush=True)
    torch.manual_seed(a.seed)
    model = NRMS(Cfg, emb).to(dev)
    fed = FedAvg(model, a.every, group=group) if group is not None else None
    try:
        r = fit(model, ts, va if has_val else None, checkpoint_dir=a.checkpoint_dir, seed=a.seed,
                steps=a.max_steps, batch_size=a.batch, fed=fed)
    finally:
        if fed is not None:
            fed.dist.destroy_process_group()
    if rank != 0:
        return
    out = {"mode": "fit (HIP kernels)" if dev.type == "cuda" and not a.aten else "fit (ATen autograd)",
           "steps": r.steps, "step": r.step, "start_step": r.start_step, "batch": a.batch,
           "steps_per_s": r.steps_per_s if r.steps else None, "last_auc": r.last_auc, "best_auc": r.best_auc,
           "early_stopped": r.early_stopped, "checkpoint": r.checkpoint,
           "final_loss": float(r.losses[-1]) if r.steps else None}
    if a.negatives == "resample":
        out.update({"negatives": "resample", "k": ts.K, "samples": len(ts), "n_dropped": ts.n_dropped})
    if fed is not None:
        out.update({"world": world, "fedavg_every": fed.every, "syncs": r.syncs, "shard_sizes": r.shard_sizes,
                    "fedavg_native": fed.native, "dist_backend": a.dist_backend})
    print(json.dumps(out), flush=True)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _nccl_short_of_gpus(a):
    """The message when nccl (RCCL), which needs a GPU per rank, sees fewer
    than --gpus; else None. gloo may share one GPU or use the CPU."""
    if a.dist_backend == "nccl" and torch.cuda.device_count() < a.gpus:
        return (f"train: --gpus {a.gpus} with the nccl backend needs {a.gpus} GPUs, "
                f"{torch.cuda.device_count()} visible")


def _launch_ranks(a):
    """DIR --gpus N (N > 1) started without a launcher: run
    torch.distributed.run with N ranks of this command line as a CHILD process
    (started before this process touches a GPU; the program of this process is
    never replaced) and return its exit code. The ranks' output goes straight
    to ours."""
    short = _nccl_short_of_gpus(a)
    if short:
        print(short, file=sys.stderr)
        return 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr", "127.0.0.1", f"--master-port={_free_port()}",
           "-m", "newsrecommendationsystem_amd.train", *sys.argv[1:]]
    return subprocess.run(cmd).returncode


def _fed_setup(a):
    """(rank, world, local rank, device, process group or None) of the DIR
    form. --gpus N is the world size: without it one process and no group;
    with it this process is one client (a group even at N = 1, so one GPU
    exercises the federated route). Fatal: a launcher whose WORLD_SIZE is not
    N, or nccl with fewer GPUs than ranks."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank, local = int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    gpu = torch.cuda.is_available()
    if a.gpus is None:
        dev = torch.device("cuda", 0) if gpu else torch.device("cpu")
        if gpu:
            torch.cuda.set_device(dev)
        return 0, 1, 0, dev, None
    if world != a.gpus:
        raise SystemExit(f"train: WORLD_SIZE={world} but --gpus={a.gpus}: the launcher's process count and "
                         f"--gpus must agree")
    short = _nccl_short_of_gpus(a)
    if short:
        raise SystemExit(short)
    dev = torch.device("cuda", local % torch.cuda.device_count()) if gpu else torch.device("cpu")
    if gpu:
        torch.cuda.set_device(dev)
    if not dist.is_initialized():
        if "MASTER_ADDR" not in os.environ:                # --gpus 1 run plainly: a group of one
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
        kw = {"device_id": dev} if a.dist_backend == "nccl" else {}
        dist.init_process_group(a.dist_backend, rank=rank, world_size=world, **kw)
    return rank, world, local, dev, dist.group.WORLD


def _alternate(legs, pairs):
    """Run the legs [(name, () -> steps/s)] in turn, `pairs` rounds: (name ->
    its rates in run order, name -> their median)."""
    rate = {name: [] for name, _ in legs}
    for _ in range(pairs):
        for name, fn in legs:
            rate[name].append(fn())
    return rate, {k: statistics.median(v) for k, v in rate.items()}


def _leg_lines(rate, med):
    """The table of _alternate's result: one line per leg."""
    return ["steps/s per round (in run order):"] + [
        f"  {name:22s} median {med[name]:7.1f}  range {min(v):7.1f} .. {max(v):7.1f}  "
        f"[{', '.join(f'{x:.1f}' for x in v)}]" for name, v in rate.items()]


def _profile_path(name, override):
    out = override or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", name)
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    return out


def _print_and_write(text, name, override):
    print(text, end="")
    with open(_profile_path(name, override), "w") as f:
        f.write(text)


def _fit_bench(a, out_name, setup):
    """What --bench and --bench-resample share: one model on GPU 0, the legs
    of setup(dev, Cfg, model, fit_leg) -> (head, [(name, n -> steps/s of n
    steps)], medians -> closing lines) warmed up untimed, then alternated;
    the table printed and written. fit_leg(train_set, **kw): the leg that
    runs fit on it, logging to nowhere."""
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, steps, pairs = a.batch, a.steps, max(5, a.pairs)

    class Cfg(NRMSConfig):
        num_batches_show_loss = 100
    torch.manual_seed(0)
    model = NRMS(Cfg, torch.randn(Cfg.num_words, 300)).to(dev)

    def fit_leg(train_set, **kw):
        return lambda n: fit(model, train_set, steps=n, batch_size=B, log=lambda *_: None, **kw).steps_per_s

    head, legs, closing = setup(dev, Cfg, model, fit_leg)
    for _, leg in legs:
        leg(a.warmup + 20)
    rate, med = _alternate([(name, lambda leg=leg: leg(steps)) for name, leg in legs], pairs)
    lines = [f"{head}, 1+K = 3, N = 50, B = {B}, V = {Cfg.num_words}, dropout {Cfg.dropout_probability}, "
             f"validation off; {pairs} alternated rounds of {steps} steps per leg, one process, "
             f"{torch.cuda.get_device_name(dev)}"] + _leg_lines(rate, med) + closing(med)
    _print_and_write("\n".join(lines) + "\n", out_name, a.bench_out)


def _bench_main(a):
    """--bench: the fit loop's device route against its host_batches route and
    the synthetic train_step loop, alternated on one model in one process, on a
    generated split (20,000 samples, 1 + K = 3, 50 clicked, V = 70,976, dropout
    0.2, no validation). Prints the table and writes it to
    profiles/fit_bench.txt."""
    S, n_news = 20000, 20000

    def setup(dev, Cfg, model, fit_leg):
        with tempfile.TemporaryDirectory() as d:
            corpus = synthetic_train_split(d, seed=0, n_samples=S, n_news=n_news, V=Cfg.num_words, K=2)
            ts = TrainSet(os.path.join(d, "behaviors_parsed.tsv"), corpus, device=dev)
        syn = synthetic_train_batches(100, a.steps, a.batch, Cfg.num_words, device=dev)
        opt = make_optimizer(model)

        def leg_synthetic(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for cand, clk in syn[:n]:
                train_step(model, opt, cand, clk)
            torch.cuda.synchronize()
            return n / (time.perf_counter() - t0)

        def closing(med):
            return [f"fit device / synthetic train_step (medians): "
                    f"{med['fit device'] / med['synthetic train_step']:.4f}",
                    f"fit device / fit host_batches (medians):     "
                    f"{med['fit device'] / med['fit host_batches']:.4f}"]
        return (f"fit bench: S = {S}",
                [("fit device", fit_leg(ts)), ("fit host_batches", fit_leg(ts, host_batches=True)),
                 ("synthetic train_step", leg_synthetic)], closing)
    _fit_bench(a, "fit_bench.txt", setup)


def _bench_resample_main(a):
    """--bench-resample: fit on an ImpressionSet (negatives drawn in the gather
    launch) against fit on the TrainSet of its exported epoch 0 (the static
    route), alternated on one model in one process, on a generated raw split
    (about 20,000 samples, 1 + K = 3, 50 clicked, V = 70,976, dropout 0.2, no
    validation). Prints the table and writes it to
    profiles/fit_resample_bench.txt."""
    def setup(dev, Cfg, model, fit_leg):
        with tempfile.TemporaryDirectory() as d:
            synthetic_split(d, seed=0, n_news=20000, n_users=2000, n_impressions=4800, V=Cfg.num_words)
            corpus = read_news_parsed(os.path.join(d, "news_parsed.tsv"))
            iset = ImpressionSet(os.path.join(d, "behaviors.tsv"), corpus, k=2, device=dev)
            iset.export_epoch(os.path.join(d, "behaviors_parsed.tsv"), 0, 0)
            ts = TrainSet(os.path.join(d, "behaviors_parsed.tsv"), corpus, device=dev)
        assert len(ts) == len(iset)
        ts_bytes = sum(t.numel() * t.element_size() for t in (ts.titles, ts.rows))

        def closing(med):
            return [f"fit ImpressionSet / fit TrainSet (medians): "
                    f"{med['fit ImpressionSet'] / med['fit TrainSet (static)']:.4f}",
                    f"device bytes: TrainSet {ts_bytes} (titles {ts.titles.numel() * 8}, rows "
                    f"{ts.rows.numel() * 4}); ImpressionSet {iset.device_bytes} (titles {iset.titles.numel() * 8}, "
                    f"the rest {iset.device_bytes - iset.titles.numel() * 8})"]
        return (f"fit resample bench: S = {len(iset)} samples of {iset.imp_hist.shape[0]} impressions "
                f"({iset.neg_rows.shape[0]} negatives, {iset.hist_rows.shape[0]} distinct histories, "
                f"{iset.n_dropped} positives dropped)",
                [("fit TrainSet (static)", fit_leg(ts)), ("fit ImpressionSet", fit_leg(iset))], closing)
    _fit_bench(a, "fit_resample_bench.txt", setup)


def _quality_resample_main(a):
    """--quality-resample: quality.resample_vs_static, one run, written to
    profiles/resample_quality.txt."""
    text = resample_vs_static(epochs=a.epochs if a.epochs is not None else 6, B=a.batch, seed=a.seed)
    _print_and_write(text, "resample_quality.txt", a.bench_out)


def _synthetic_main(a):
    """No DIR: a.steps timed train_step calls on synthetic batches, under
    torch.distributed.run with FedAvg across the ranks every a.every steps
    (config 5 shape); rank 0 prints one JSON line with steps/s, the time spent
    in the syncs and the final loss."""
    rank, world, local, distributed = init_from_env()
    dev = torch.device("cuda", local) if torch.cuda.is_available() else torch.device("cpu")
    if dev.type == "cuda":
        torch.cuda.set_device(dev)
    torch.manual_seed(0)                        # identical initial weights on every rank

    class Cfg(NRMSConfig):
        hip_train = not a.aten
    model = NRMS(Cfg, torch.randn(NRMSConfig.num_words, 300)).to(dev)
    opt = (torch.optim.Adam(model.parameters(), lr=Cfg.learning_rate) if a.aten
           else make_optimizer(model))
    fed = FedAvg(model, a.every) if distributed else None
    batches = synthetic_train_batches(100 + rank, a.steps + a.warmup, a.batch, NRMSConfig.num_words,
                                      device=dev)
    for cand, clk in batches[:a.warmup]:
        train_step(model, opt, cand, clk)
    batches = batches[a.warmup:]
    wait = torch.cuda.synchronize if dev.type == "cuda" else (lambda: None)
    sync_t = 0.0
    wait()
    t0 = time.perf_counter()
    loss = None
    for cand, clk in batches:
        loss = train_step(model, opt, cand, clk)
        if fed is not None:
            wait()
            ts = time.perf_counter()
            if fed.step():
                wait()
            sync_t += time.perf_counter() - ts
    wait()
    dt = time.perf_counter() - t0
    if rank == 0:
        print(json.dumps({"mode": ("train (HIP kernels)" if dev.type == "cuda" and not a.aten
                                   else "train (ATen autograd)") + " + FedAvg", "world": world, "steps": a.steps,
                          "batch_per_rank": a.batch, "fedavg_every": a.every,
                          "steps_per_s": a.steps / dt, "samples_per_s": world * a.batch * a.steps / dt,
                          "fedavg_sync_s_total": sync_t, "final_loss": float(loss),
                          "param_bytes": int(sum(p.numel() for p in model.parameters()) * 4)}))


def _parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir", nargs="?", default=None, help="MIND directory (train/ and val/): fit on it")
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--every", type=int, default=5, help="FedAvg: average the models every E steps")
    ap.add_argument("--gpus", type=int, default=None,
                    help="DIR: federated fit over N ranks (started here as a torch.distributed.run child "
                         "unless a launcher already runs this process)")
    ap.add_argument("--dist-backend", choices=("nccl", "gloo"), default=None,
                    help="DIR --gpus: process-group backend (default: nccl on a GPU, gloo on the CPU)")
    ap.add_argument("--aten", action="store_true", help="ATen autograd + torch Adam instead of HIP")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--checkpoint-dir", default="checkpoint/NRMS")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--epochs", type=int, default=None)
    ap.add_argument("--max-steps", type=int, default=None)
    ap.add_argument("--validate-every", type=int, default=None,
                    help="DIR: validate (and checkpoint on improvement) every n steps (default: the config's 1000)")
    ap.add_argument("--bench", action="store_true", help="fit loop: device route vs host_batches vs synthetic")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--bench-out", default=None)
    ap.add_argument("--negatives", choices=("file", "resample"), default="file",
                    help="file: behaviors_parsed.tsv's negatives; resample: behaviors.tsv, new negatives per epoch")
    ap.add_argument("--k", type=int, default=None, help="negatives per positive with --negatives resample")
    ap.add_argument("--export-epoch", nargs=2, metavar=("E", "PATH"), default=None,
                    help="with --negatives resample: write epoch E's samples as a behaviors_parsed.tsv and exit")
    ap.add_argument("--bench-resample", action="store_true", help="fit loop: ImpressionSet vs exported TrainSet")
    ap.add_argument("--quality-resample", action="store_true",
                    help="planted teacher: validation AUC per epoch, static vs resampled negatives")
    return ap


def _main(argv=None):
    """python -m newsrecommendationsystem_amd.train [--steps 20] [--batch 128] [--every 5]
    Under torch.distributed.run: FedAvg across ranks (config 5 shape); prints
    one JSON line on rank 0 with steps/s, sync time and the final loss (_synthetic_main).

    python -m newsrecommendationsystem_amd.train DIR [--checkpoint-dir checkpoint/NRMS] [--seed 0]
        [--epochs N] [--batch B] [--max-steps n] [--negatives file|resample] [--k K] [--export-epoch E PATH]
        [--validate-every n] [--gpus N [--every E] [--dist-backend nccl|gloo]]
    trains on a MIND directory (fit.py; _fit_main). --negatives file (default): DIR/train/
    behaviors_parsed.tsv with the negatives it lists; resample: DIR/train/behaviors.tsv, K new negatives per
    positive and epoch (fit.ImpressionSet); --export-epoch E PATH writes epoch E's draw (for --seed) as a
    behaviors_parsed.tsv and exits. --bench: _bench_main; --bench-resample: _bench_resample_main;
    --quality-resample: _quality_resample_main. --gpus N: a federated fit (fit(fed=FedAvg)) over N ranks,
    each a client on the samples of the users it owns, models averaged every E steps; under
    torch.distributed.run this process is one client, run plainly it starts the N ranks as a child process
    and waits (_launch_ranks). Rank 0 prints the JSON line (with world, fedavg_every, syncs, shard_sizes)
    and writes ckpt-{t}.pth; rank r its optimizer state to ckpt-{t}.rank{r}.pth."""
    ap = _parser()
    a = ap.parse_args(argv)
    if a.bench or a.bench_resample:
        a.steps = 300 if a.steps is None else a.steps
        a.batch = 64 if a.batch is None else a.batch
        return _bench_main(a) if a.bench else _bench_resample_main(a)
    if a.quality_resample:
        a.batch = 64 if a.batch is None else a.batch
        return _quality_resample_main(a)
    a.batch = 128 if a.batch is None else a.batch
    if a.dir is None:
        a.steps = 20 if a.steps is None else a.steps
        return _synthetic_main(a)
    if a.gpus is not None:
        if a.gpus < 1:
            ap.error("--gpus must be at least 1")
        if a.dist_backend is None:
            a.dist_backend = "nccl" if torch.cuda.is_available() else "gloo"
        if "WORLD_SIZE" not in os.environ and a.gpus > 1:
            sys.exit(_launch_ranks(a))                  # no launcher around us: start one
    return _fit_main(a)
