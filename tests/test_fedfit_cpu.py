"""The federated fit (fit.fit(fed=train.FedAvg)) on the CPU over gloo: the
sync schedule, the per-client shards and step count, a federation of one
against the plain fit, and two ranks (child processes, tests/fedfit_worker.py)
against a hand loop of train.train_step with numpy fp32 averaging, sharded
validation, per-rank checkpoint files and resume. Dropout 0, a generated split
of 40 samples of 11 users with V = 500."""
import copy
import os
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist

from newsrecommendationsystem_amd import checkpoint as CK
from newsrecommendationsystem_amd import train as TR
from newsrecommendationsystem_amd.distributed import user_rank
from tests import fedfit_cases as C
from tests import fit_cases as FC

F = C.F
quiet = lambda *_: None  # noqa: E731


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    return C.make_split(tmp_path_factory.mktemp("fedsplit"))


@pytest.fixture(scope="module")
def group1(tmp_path_factory):
    """A gloo process group of this process alone."""
    assert not dist.is_initialized()
    store = tmp_path_factory.mktemp("store") / "s"
    dist.init_process_group("gloo", init_method=f"file://{store}", rank=0, world_size=1)
    yield dist.group.WORLD
    dist.destroy_process_group()


def test_sync_schedule():
    def due(every, validate_every, last):
        return [t for t in range(1, last + 1) if F.sync_due(t, every, validate_every, last)]
    assert due(2, 0, 6) == [2, 4, 6]
    assert due(4, 3, 6) == [3, 4, 6]                 # a validation step that is no multiple of `every`
    assert due(5, 0, 7) == [5, 7]                    # the last step always
    assert due(0, 0, 3) == [3]                       # never on its own: only at the end
    assert due(3, 4, 8) == [3, 4, 6, 8]
    assert due(1, 1000, 3) == [1, 2, 3]
    # a function of t alone: the resumed half of a run syncs where the whole run does
    assert [t for t in due(3, 4, 8) if t > 4] == [t for t in range(5, 9) if F.sync_due(t, 3, 4, 8)]


def test_rank_files_do_not_count_as_checkpoints(tmp_path):
    for name in ("ckpt-4.pth", "ckpt-4.rank1.pth", "ckpt-12.rank1.pth", "ckpt-12.rank10.pth"):
        (tmp_path / name).write_bytes(b"")
    assert CK.latest_checkpoint(str(tmp_path)) == str(tmp_path / "ckpt-4.pth")
    assert CK.rank_path(str(tmp_path / "ckpt-4.pth"), 1) == str(tmp_path / "ckpt-4.rank1.pth")


class _Client:
    """What fit() reads of a FedAvg before its first collective: enough to
    reach the argument checks as rank `rank` of `world`."""

    def __init__(self, rank, world):
        self.world, self.group, self.every = world, None, 1
        self.dist = types.SimpleNamespace(get_rank=lambda group=None: rank)


def test_shards_steps_and_argument_errors(split, tmp_path):
    ts = C.train_set(split)
    assert len(ts) == C.S and len(ts.users) == C.S and ts.users[12] == "U1"
    for world in (2, 3):
        shards = [F.client_shard(ts, r, world) for r in range(world)]
        assert all(s.dtype == np.int64 and np.all(np.diff(s) > 0) for s in shards)
        allidx = np.concatenate(shards)
        assert np.array_equal(np.sort(allidx), np.arange(C.S))              # disjoint and complete
        owner = {}
        for r, s in enumerate(shards):
            for k in s:
                assert owner.setdefault(ts.users[k], r) == r                # a user sits on one rank
                assert user_rank(ts.users[k], world) == r
        assert F.shard_sizes(ts, world) == [len(s) for s in shards] and min(map(len, shards)) > 0
    assert np.array_equal(F.client_shard(ts, 0, 1), np.arange(C.S)) and F.shard_sizes(ts, 1) == [C.S]
    assert F.federated_total_steps(3, 40, 2, 4) == 15 and F.federated_total_steps(3, 41, 3, 4) == 9
    assert F.federated_total_steps(2, 40, 1, 16) == 2 * 40 // 16              # world 1: the plain fit's count
    assert F.client_seed(7, 0) == 7 and F.client_seed(7, 1) == F.mix64(F.mix64(7) + 1) & (2 ** 62 - 1)
    assert len({F.client_seed(7, r) for r in range(8)}) == 8
    m = C.model(C.config())
    # 11 users over 3 ranks: rank 2 owns U2, U5, U8 = 4 + 4 + 3 samples < 12, the others 15 and 14
    assert F.shard_sizes(ts, 3)[2] < 12 <= min(F.shard_sizes(ts, 3)[:2])
    for rank in (0, 2):
        with pytest.raises(ValueError, match="rank 2"):
            F.fit(m, ts, steps=1, batch_size=12, log=quiet, fed=_Client(rank, 3))
    # no `user` column: fine for the plain fit, an error for a federated one
    src = os.path.join(split, "train", "behaviors_parsed.tsv")
    bare = tmp_path / "behaviors_parsed.tsv"
    with open(src) as f, open(bare, "w") as g:
        for ln in f:
            g.write(ln.split("\t", 1)[1])
    from newsrecommendationsystem_amd import data as Dt
    nouser = F.TrainSet(str(bare), Dt.read_news_parsed(os.path.join(split, "train", "news_parsed.tsv")))
    assert nouser.users is None and np.array_equal(nouser.rows_host, ts.rows_host)
    assert F.fit(copy.deepcopy(m), nouser, steps=1, batch_size=4, log=quiet).steps == 1
    with pytest.raises(ValueError, match="user"):
        F.fit(m, nouser, steps=1, batch_size=4, log=quiet, fed=_Client(0, 2))


def test_world1_federated_fit_is_the_plain_fit(split, group1, tmp_path):
    ts = C.train_set(split)
    cfg = C.config(num_batches_validate=2, num_batches_show_loss=3)
    base = C.model(cfg, seed=4)
    aucs = [0.51, 0.52, 0.50]
    ma, mb = copy.deepcopy(base), copy.deepcopy(base)
    la, lb = [], []
    ra = F.fit(ma, ts, checkpoint_dir=str(tmp_path / "a"), seed=3, steps=5, batch_size=8,
               validate=FC.scripted(aucs), log=la.append)
    fed = TR.FedAvg(mb, every=2, group=group1)
    assert fed.native is False                                             # the torch route on the CPU
    rb = F.fit(mb, ts, checkpoint_dir=str(tmp_path / "b"), seed=3, steps=5, batch_size=8,
               validate=FC.scripted(aucs), log=lb.append, fed=fed)
    assert torch.equal(ra.losses, rb.losses) and ra.aucs == rb.aucs and la == lb
    FC.assert_same_training_state(ma, ra.optimizer, mb, rb.optimizer)
    assert ra.syncs == 0 and ra.shard_sizes is None
    assert rb.syncs == 3 and rb.shard_sizes == [C.S]                        # t = 2, 4 and the last, 5
    assert sorted(os.listdir(tmp_path / "a")) == sorted(os.listdir(tmp_path / "b")) == ["ckpt-2.pth", "ckpt-4.pth"]
    # default step count of the federation of one: the plain fit's
    mc = copy.deepcopy(base)
    rc = F.fit(mc, ts, seed=3, batch_size=16, log=quiet, fed=TR.FedAvg(mc, every=0, group=group1))
    assert rc.steps == cfg.num_epochs * C.S // 16 and rc.syncs == 1
    with pytest.raises(ValueError):
        TR.FedAvg(base, every=1, group=group1, native=True)                 # the kernels need a GPU


def test_impression_set_shards_by_its_impressions_users(split, group1):
    """An ImpressionSet takes each sample's user from its impression, its
    shards are by that user, and a federation of one on it is the plain fit."""
    from newsrecommendationsystem_amd import data as Dt
    val = os.path.join(split, "val")
    corpus = Dt.read_news_parsed(os.path.join(val, "news_parsed.tsv"))
    iset = F.ImpressionSet(os.path.join(val, "behaviors.tsv"), corpus, k=1)
    imps = Dt.read_behaviors(os.path.join(val, "behaviors.tsv"))
    assert iset.users == [imps[i].user for i in iset.pos_imp_host.tolist()] and len(iset.users) == len(iset) > 8
    shards = [F.client_shard(iset, r, 2) for r in range(2)]
    assert np.array_equal(np.sort(np.concatenate(shards)), np.arange(len(iset)))
    assert all(user_rank(iset.users[k], 2) == r for r, s in enumerate(shards) for k in s)
    cfg = C.config(num_batches_show_loss=0)
    base = C.model(cfg, seed=8)
    ma, mb = copy.deepcopy(base), copy.deepcopy(base)
    ra = F.fit(ma, iset, seed=2, steps=3, batch_size=4, log=quiet)
    rb = F.fit(mb, iset, seed=2, steps=3, batch_size=4, log=quiet, fed=TR.FedAvg(mb, every=2, group=group1))
    assert torch.equal(ra.losses, rb.losses) and rb.syncs == 2
    FC.assert_same_training_state(ma, ra.optimizer, mb, rb.optimizer)


def test_cli_starts_its_ranks_as_a_child(split, tmp_path):
    """`train DIR --gpus 2` without a launcher around it, on the CPU over
    gloo: one JSON line, rank 0's, with the federation's fields; a launcher
    whose process count is not --gpus is fatal."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", OMP_NUM_THREADS=str(C.CPU_THREADS))
    cmd = [sys.executable, "-m", "newsrecommendationsystem_amd.train", split, "--gpus", "2", "--every", "2",
           "--max-steps", "3", "--batch", "4", "--aten", "--checkpoint-dir", str(tmp_path / "ck")]
    p = subprocess.run(cmd, cwd=C.ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-3000:]
    out = json.loads(lines[0])
    assert (out["world"], out["fedavg_every"], out["syncs"], out["steps"]) == (2, 2, 2, 3)          # t = 2, 3
    assert out["shard_sizes"] == F.shard_sizes(C.train_set(split), 2) and out["dist_backend"] == "gloo"
    assert out["fedavg_native"] is False and np.isfinite(out["final_loss"])
    p = subprocess.run(cmd, cwd=C.ROOT, env=dict(env, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0"),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "must agree" in p.stderr


RUNS = {
    "six": dict(B=4, every=4, validate_every=3, seed=3, val=True, ckdir=None, first_sync=True,
                calls=[dict(steps=6, unsharded_auc=True)]),
    "halves": dict(B=4, every=3, validate_every=4, seed=1, val=True, ckdir="ck_halves",
                   calls=[dict(steps=4), dict(steps=4)]),
    "whole": dict(B=4, every=3, validate_every=4, seed=1, val=True, ckdir="ck_whole", calls=[dict(steps=8)]),
    "lost": dict(B=4, every=3, validate_every=4, seed=1, val=True, ckdir="ck_lost",
                 calls=[dict(steps=4), dict(steps=2, delete_own_rank_file=True)]),
}


@pytest.fixture(scope="module")
def two_ranks(split, tmp_path_factory):
    out = tmp_path_factory.mktemp("fed2")
    res = C.run_workers(out, dict(split=split, hip=False, dropout=0.0, runs=RUNS), world=2)
    return out, res


def _load(out, run, call, rank):
    with np.load(os.path.join(str(out), f"{run}.call{call}.rank{rank}.npz")) as z:
        return {k: z[k] for k in z.files}


def test_two_ranks_equal_the_hand_loop(split, two_ranks):
    out, res = two_ranks
    got = [_load(out, "six", 0, r) for r in range(2)]
    assert np.array_equal(got[0]["params"], got[1]["params"])
    assert not np.array_equal(got[0]["pre_sync"], got[1]["pre_sync"])        # the clients trained apart
    assert not np.array_equal(got[0]["losses"], got[1]["losses"])
    for g in got:
        assert np.array_equal(g["post_sync"], (got[0]["pre_sync"] + got[1]["pre_sync"]) / np.float32(2))
    rec = [res[r]["six"][0] for r in range(2)]
    assert all(x["syncs"] == 3 and x["steps"] == 6 and x["native"] is False for x in rec)      # t = 3, 4, 6
    assert rec[0]["shard_sizes"] == rec[1]["shard_sizes"] and sum(rec[0]["shard_sizes"]) == C.S
    assert rec[0]["lines"] and not rec[1]["lines"]                            # rank 0 speaks
    # the same two clients, one after the other in this process
    ts = C.train_set(split)
    cfg = C.config(num_batches_validate=3, num_batches_show_loss=0)
    run = RUNS["six"]
    clients = [copy.deepcopy(C.model(cfg, seed=0)) for _ in range(2)]          # rank 0's model, broadcast
    opts = [TR.make_optimizer(m) for m in clients]
    shards = [torch.from_numpy(F.client_shard(ts, r, 2)) for r in range(2)]
    seeds = [F.client_seed(run["seed"], r) for r in range(2)]
    losses = [[], []]
    with C.cpu_threads():
        for t in range(1, 7):
            for r, (m, opt) in enumerate(zip(clients, opts)):
                e, a, b = F.batch_of_step(t, len(shards[r]), run["B"])
                idx = shards[r][F.epoch_order(seeds[r], e, len(shards[r]))[a:b]]
                losses[r].append(float(TR.train_step(m, opt, *ts.batch(idx))))
            if F.sync_due(t, run["every"], run["validate_every"], 6):
                with torch.no_grad():
                    for p, q in zip(clients[0].parameters(), clients[1].parameters()):
                        mean = (p.numpy() + q.numpy()) / np.float32(2)
                        p.copy_(torch.from_numpy(mean))
                        q.copy_(torch.from_numpy(mean))
    assert np.array_equal(C.flat_params(clients[0]), got[0]["params"])
    for r in range(2):
        assert np.array_equal(np.asarray(losses[r], np.float32), got[r]["losses"])
    # sharded validation: every rank the same AUCs; the last one is the unsharded validator's on that model
    assert rec[0]["aucs"] == rec[1]["aucs"] and [t for t, _ in rec[0]["aucs"]] == [3, 6]
    np.testing.assert_allclose(rec[0]["aucs"][-1][1], rec[0]["unsharded_auc"], rtol=1e-12, atol=0)
    assert rec[0]["unsharded_auc"] == rec[1]["unsharded_auc"] and 0 < rec[0]["unsharded_auc"] < 1


def test_two_ranks_resume(two_ranks):
    out, res = two_ranks
    first, second = (res[0]["halves"][k] for k in range(2))
    assert first["files"] == ["ckpt-4.pth", "ckpt-4.rank1.pth"]
    assert set(second["files"]) >= {"ckpt-4.pth", "ckpt-4.rank1.pth"}
    newest = "ckpt-8.pth" if "ckpt-8.pth" in second["files"] else "ckpt-4.pth"      # step 8's AUC may not improve
    assert CK.latest_checkpoint(os.path.join(str(out), "ck_halves")) == os.path.join(str(out), "ck_halves", newest)
    assert second["files"] == res[0]["whole"][0]["files"]
    ck1 = CK.load(os.path.join(str(out), "ck_halves", "ckpt-4.rank1.pth"))
    assert sorted(ck1) == ["optimizer_state_dict", "step"] and ck1["step"] == 4
    for r in range(2):
        a, b = res[r]["halves"]
        w = res[r]["whole"][0]
        assert (a["start_step"], a["step"], b["start_step"], b["step"], b["steps"]) == (0, 4, 4, 8, 4)
        assert a["syncs"] == 2 and b["syncs"] == 2 and w["syncs"] == 4          # t = 3, 4 | 6, 8
        assert not any("optimizer state" in ln for ln in b["lines"])
        half, whole = _load(out, "halves", 1, r), _load(out, "whole", 0, r)
        for k in ("params", "exp_avg", "exp_avg_sq"):
            assert np.array_equal(half[k], whole[k]), (r, k)
        assert np.array_equal(half["losses"], whole["losses"][4:])
        assert np.array_equal(_load(out, "halves", 0, r)["losses"], whole["losses"][:4])
    assert np.array_equal(_load(out, "whole", 0, 0)["params"], _load(out, "whole", 0, 1)["params"])
    # rank 1's file gone: it resumes on rank 0's moments and says so
    lost = [res[r]["lost"][1] for r in range(2)]
    assert all((x["start_step"], x["step"], x["steps"]) == (4, 6, 2) for x in lost)
    assert lost[1]["lines"] == ["rank 1: no ckpt-4.rank1.pth, taking rank 0's optimizer state"]
    assert not any("optimizer state" in ln for ln in lost[0]["lines"])
    assert np.array_equal(_load(out, "lost", 1, 0)["params"], _load(out, "lost", 1, 1)["params"])
