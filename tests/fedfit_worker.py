"""One rank of the federated-fit tests (tests/test_fedfit_cpu.py on gloo and
the CPU, tests/test_gpu_fedfit.py with every rank on cuda:0): started as a
plain child process per rank by tests/fedfit_cases.run_workers.

    python tests/fedfit_worker.py OUT_DIR gloo|nccl cpu|cuda:0

OUT_DIR/job.json: {"split": DIR, "hip": bool, "dropout": p, "runs": {name:
{"B", "every", "validate_every", "seed", "val": bool, "ckdir": name or null,
"first_sync": bool, "calls": [{"steps": n, "delete_own_rank_file": bool}]}}}.
Every call of a run builds a new model (seeded differently on every rank: the
start broadcast must make them one) and a FedAvg over the default group, runs
fit(fed=...) and saves OUT_DIR/{run}.call{k}.rank{r}.npz (params, moments,
losses); OUT_DIR/rank{r}.json gets the rest."""
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from newsrecommendationsystem_amd import checkpoint as CK  # noqa: E402
from newsrecommendationsystem_amd import evaluate as EV  # noqa: E402
from newsrecommendationsystem_amd import train as TR  # noqa: E402
from tests import fedfit_cases as C  # noqa: E402

F = C.F


def moments(opt):
    st = opt.state_dict()["state"]
    if not st:
        return np.zeros(0, np.float32), np.zeros(0, np.float32)
    return (torch.cat([st[i]["exp_avg"].reshape(-1) for i in sorted(st)]).cpu().numpy(),
            torch.cat([st[i]["exp_avg_sq"].reshape(-1) for i in sorted(st)]).cpu().numpy())


def main():
    out, backend, device = sys.argv[1], sys.argv[2], sys.argv[3]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    job = json.load(open(os.path.join(out, "job.json")))
    dev = torch.device(device)
    if dev.type == "cuda":
        torch.cuda.set_device(dev)
    else:
        EV.score_plan = C.cpu_score_plan            # the HIP scorer needs a GPU
    kw = {"device_id": dev} if backend == "nccl" else {}
    dist.init_process_group(backend, rank=rank, world_size=world, **kw)
    res = {}
    try:
        ts = C.train_set(job["split"], device=dev)
        val = os.path.join(job["split"], "val")
        for name, run in job["runs"].items():
            cfg = C.config(job["dropout"], job["hip"], num_batches_validate=run["validate_every"],
                           num_batches_show_loss=0)
            ck = os.path.join(out, run["ckdir"]) if run.get("ckdir") else None
            rr = res[name] = []
            for k, call in enumerate(run["calls"]):
                m = C.model(cfg, seed=10 * k + rank, device=dev)
                fed = TR.FedAvg(m, run["every"], native=job.get("native"))
                snaps = []
                if run.get("first_sync"):
                    real = fed.sync

                    def sync(real=real, m=m, snaps=snaps):
                        if not snaps:
                            snaps.append(C.flat_params(m))
                            real()
                            snaps.append(C.flat_params(m))
                        else:
                            real()
                    fed.sync = sync
                if call.get("delete_own_rank_file") and rank > 0:
                    os.remove(CK.rank_path(CK.latest_checkpoint(ck), rank))
                lines = []
                r = F.fit(m, ts, val if run["val"] else None, checkpoint_dir=ck, seed=run["seed"],
                          steps=call["steps"], batch_size=run["B"], log=lines.append, fed=fed)
                m1, m2 = moments(r.optimizer)
                arrays = dict(params=C.flat_params(m), exp_avg=m1, exp_avg_sq=m2, losses=r.losses.numpy())
                if snaps:
                    arrays.update(pre_sync=snaps[0], post_sync=snaps[1])
                np.savez(os.path.join(out, f"{name}.call{k}.rank{rank}.npz"), **arrays)
                dist.barrier()                      # every rank's checkpoint files are written
                rec = {"start_step": r.start_step, "step": r.step, "steps": r.steps, "syncs": r.syncs,
                       "aucs": r.aucs, "shard_sizes": r.shard_sizes, "lines": lines, "native": fed.native,
                       "optimizer": type(r.optimizer).__name__, "checkpoint": r.checkpoint,
                       "files": sorted(os.listdir(ck)) if ck else None}
                if run["val"] and call.get("unsharded_auc"):
                    m.eval()
                    rec["unsharded_auc"] = float(F._DirValidator(val, cfg.num_clicked_news_a_user)(m))
                rr.append(rec)
                dist.barrier()                      # the listing above before the next call writes
        with open(os.path.join(out, f"rank{rank}.json"), "w") as f:
            json.dump(res, f)
        dist.barrier()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
