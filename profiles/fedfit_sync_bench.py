"""The federated fit's exchange and loop on one GPU (a world-size-1 RCCL
group, as profiles/fedavg_sync_bench.py sets one up: the RCCL call path runs,
no link traffic).

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 \
        --master-port 29556 profiles/fedfit_sync_bench.py [sync] [loop] [--out profiles/fedfit_sync_bench.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python profiles/fedfit_sync_bench.py kernels

sync     train.FedAvg.sync at the model's real size (21,955,400 parameters)
         with native=False (one copy_ per parameter each way, div_) against
         native=True (nrms_params_pack, nrms_params_unpack_div): alternated
         pairs in one process after warm-up, each sync timed with HIP events;
         median and range per leg, and in how many pairs the native route won.
loop     fit steps/s on the --bench split (20,000 samples, B = 64) with fed at
         world 1, every 1 and 5, against the plain fit, alternated.
kernels  nothing but the two kernels, a few times each, for a kernel trace of
         its own (no process group, no timing here): 175.6 MB moved per launch.
"""
import argparse
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # HBM3E spec peak, as bench.py's PEAK_HBM_GBS


def _event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _line(name, v):
    return (f"  {name:28s} median {statistics.median(v):8.4f}  range {min(v):8.4f} .. {max(v):8.4f}  "
            f"[{', '.join(f'{x:.3f}' for x in v)}]")


def sync_leg(dev, pairs, inner):
    import bench
    from newsrecommendationsystem_amd.train import FedAvg
    model = bench.build_model(dev)
    legs = {"native=False (torch)": FedAvg(model, 1, native=False), "native=True (HIP)": FedAvg(model, 1, native=True)}
    before = [p.detach().clone() for p in model.parameters()]
    for fa in legs.values():                                          # warm-up, untimed
        for _ in range(5):
            fa.sync()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(pairs):
        for k, fa in legs.items():
            ms[k].append(_event_ms(lambda: [fa.sync() for _ in range(inner)]) / inner)
    same = all(torch.equal(p, b) for p, b in zip(model.parameters(), before))
    a, b = ms["native=False (torch)"], ms["native=True (HIP)"]
    won = sum(y < x for x, y in zip(a, b))
    n = next(iter(legs.values())).flat.numel()
    lines = [f"FedAvg.sync, {n} parameters ({4 * n / 1e6:.1f} MB), world 1 on "
             f"{torch.distributed.get_backend()}, {torch.cuda.get_device_name(dev)}; {pairs} alternated pairs, "
             f"each the mean of {inner} consecutive syncs between two HIP events; ms per sync:",
             _line("native=False (torch)", a), _line("native=True (HIP)", b),
             f"  native faster in {won} of {pairs} pairs; median ratio native / torch "
             f"{statistics.median(b) / statistics.median(a):.4f}",
             f"  parameters bitwise unchanged by every sync (world 1): {same}"]
    return lines


def loop_leg(dev, pairs, steps, B):
    from newsrecommendationsystem_amd.config import NRMSConfig
    from newsrecommendationsystem_amd.data import synthetic_train_split
    from newsrecommendationsystem_amd.fit import TrainSet, fit
    from newsrecommendationsystem_amd.nrms import NRMS
    from newsrecommendationsystem_amd.train import FedAvg

    class Cfg(NRMSConfig):
        num_batches_show_loss = 100
    torch.manual_seed(0)
    model = NRMS(Cfg, torch.randn(Cfg.num_words, 300)).to(dev)
    with tempfile.TemporaryDirectory() as d:
        corpus = synthetic_train_split(d, seed=0, n_samples=20000, n_news=20000, V=Cfg.num_words, K=2)
        ts = TrainSet(os.path.join(d, "behaviors_parsed.tsv"), corpus, device=dev)
    quiet = lambda *_: None  # noqa: E731
    feds = {1: FedAvg(model, 1), 5: FedAvg(model, 5)}
    legs = [("plain fit", lambda: fit(model, ts, steps=steps, batch_size=B, log=quiet))]
    for e, fa in feds.items():
        legs.append((f"fed, world 1, every {e}", lambda fa=fa: fit(model, ts, steps=steps, batch_size=B, log=quiet, fed=fa)))
    for _, fn in legs:                                                # warm-up, untimed
        fn()
    rate = {name: [] for name, _ in legs}
    syncs = {}
    for _ in range(pairs):
        for name, fn in legs:
            r = fn()
            rate[name].append(r.steps_per_s)
            syncs[name] = r.syncs
    lines = [f"fit loop, S = 20000, 1+K = 3, N = 50, B = {B}, V = {Cfg.num_words}, dropout {Cfg.dropout_probability}, "
             f"validation off; {pairs} alternated rounds of {steps} steps per leg; FedAvg native = "
             f"{feds[1].native}; steps/s:"]
    lines += [_line(f"{name} ({syncs[name]} syncs)", v) for name, v in rate.items()]
    base = statistics.median(rate["plain fit"])
    lines += [f"  {name} / plain fit (medians): {statistics.median(v) / base:.4f}" for name, v in rate.items()
              if name != "plain fit"]
    return lines


def kernels_leg(dev, reps):
    import bench
    from newsrecommendationsystem_amd.train import FedAvg

    import torch.distributed as dist
    with tempfile.TemporaryDirectory() as d:        # a gloo group of one: FedAvg asks it for its size only
        dist.init_process_group("gloo", init_method=f"file://{d}/store", rank=0, world_size=1)
        try:
            fa = FedAvg(bench.build_model(dev), 1, native=True)
            for _ in range(reps):
                fa._pack()
                fa._unpack(2)               # the dividing kernel (divisor 1 is the plain copy)
                fa._unpack(1)
            torch.cuda.synchronize()
        finally:
            dist.destroy_process_group()
    n = fa.flat.numel()
    print(f"ran nrms_params_pack, unpack_div(2), unpack_div(1) x {reps}: {8 * n / 1e6:.1f} MB moved per launch; at the "
          f"{HBM_PEAK_GBS / 1e3:.1f} TB/s spec peak that is {8 * n / HBM_PEAK_GBS / 1e3:.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("legs", nargs="*", default=["sync", "loop"])
    ap.add_argument("--pairs", type=int, default=24)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--loop-pairs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    local = int(os.environ.get("LOCAL_RANK", 0))
    dev = torch.device("cuda", local % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    if a.legs == ["kernels"]:
        return kernels_leg(dev, a.reps)
    import torch.distributed as dist
    dist.init_process_group("nccl", device_id=dev)
    lines = []
    try:
        if "sync" in a.legs:
            lines += sync_leg(dev, max(20, a.pairs), a.inner) + [""]
        if "loop" in a.legs:
            lines += loop_leg(dev, a.loop_pairs, a.steps, a.batch) + [""]
    finally:
        dist.destroy_process_group()
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
