"""The fit loop (newsrecommendationsystem_amd/fit.py) on the CPU: TrainSet
against the reference's own BaseDataset batches, the epoch order, the
reference's early stopping / checkpoint / resume rules (src/train.py:27-51,
144-149,260-279), and fit() against a hand loop of train.train_step."""
import copy
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from newsrecommendationsystem_amd import checkpoint as CK
from newsrecommendationsystem_amd import data as Dt
from newsrecommendationsystem_amd import train as TR
from tests import fit_cases as FC
from tests.test_flow_cpu import _small_cfg

F = FC.F


def _model(flow, seed=0, **cfg_fields):
    from newsrecommendationsystem_amd import NRMS
    torch.manual_seed(seed)
    return NRMS(FC.with_cfg(_small_cfg(int(flow["V_train"])), **cfg_fields))


def test_package_exports_fit_and_trainset():
    import newsrecommendationsystem_amd as P
    assert P.fit is F.fit and P.TrainSet is F.TrainSet


def test_trainset_batches_match_reference_basedataset(flow, tmp_path):
    ts = FC.flow_train_set(flow)
    assert ts.titles.dtype == torch.int64 and ts.rows.dtype == torch.int32
    assert tuple(ts.rows.shape) == (12, 53) and ts.titles.shape[1] == 20
    assert not ts.titles[-1].any()                                   # the padding title
    cand, clk = ts.batch(torch.arange(12))
    assert cand.dtype == torch.int64 and clk.dtype == torch.int64
    assert np.array_equal(cand.numpy(), flow["batch_cand"])
    assert np.array_equal(clk.numpy(), flow["batch_clicked"])
    idx = np.array([7, 0, 11, 7, 3, 3, 0])
    cand, clk = ts.batch(idx)
    assert np.array_equal(cand.numpy(), flow["batch_cand"][idx])
    assert np.array_equal(clk.numpy(), flow["batch_clicked"][idx])
    # one line with another number of candidates / an unknown id
    src = os.path.join(flow["dir"], "train", "behaviors_parsed.tsv")
    corpus = Dt.read_news_parsed(os.path.join(flow["dir"], "train", "news_parsed.tsv"))
    for name, line in (("ragged.tsv", "U99\t \tT1 T2\t1 0\n"), ("unknown.tsv", "U99\tT1\tT1 T2 Tnone\t1 0 0\n")):
        bad = tmp_path / name
        shutil.copy(src, bad)
        with open(bad, "a") as f:
            f.write(line)
        with pytest.raises(ValueError):
            F.TrainSet(str(bad), corpus)


def test_epoch_order_and_batch_slicing():
    S = 12
    o = F.epoch_order(5, 0, S)
    assert o.dtype == torch.int64 and sorted(o.tolist()) == list(range(S))
    assert torch.equal(o, F.epoch_order(5, 0, S))
    assert not torch.equal(o, F.epoch_order(5, 1, S))
    assert not torch.equal(F.epoch_order(5, 0, 64), F.epoch_order(6, 0, 64))
    # S = 12, B = 5: two steps per epoch (drop_last); step 3 is batch 0 of epoch 1
    assert [F.batch_of_step(t, S, 5) for t in (1, 2, 3, 4, 5)] == \
        [(0, 0, 5), (0, 5, 10), (1, 0, 5), (1, 5, 10), (2, 0, 5)]
    assert F.dropout_seed(3, 7) == F.dropout_seed(3, 7) != F.dropout_seed(3, 8)
    assert F.dropout_seed(3, 7) != F.dropout_seed(4, 7) and 2 * F.dropout_seed(2 ** 40, 2 ** 31 - 1) + 1 < 2 ** 63


def test_early_stopping_and_checkpoints(flow, tmp_path):
    aucs = [0.60, 0.70, 0.70, 0.65, 0.69, 0.66, 0.60, 0.60, 0.60]
    ts = FC.flow_train_set(flow)
    m = _model(flow, num_batches_validate=1)
    ck = str(tmp_path / "ck")
    lines = []
    r = F.fit(m, ts, checkpoint_dir=ck, steps=20, batch_size=4, validate=FC.scripted(aucs), log=lines.append)
    # improvements at steps 1 and 2 only: step 3's equal AUC is not one (strict <)
    assert sorted(os.listdir(ck)) == ["ckpt-1.pth", "ckpt-2.pth"]
    # five non-improvements (steps 3..7) end the loop
    assert r.early_stopped and r.step == 7 and r.steps == 7 and len(r.losses) == 7
    assert [a for _, a in r.aucs] == aucs[:7] and r.best_auc == 0.70 and r.last_auc == 0.60
    assert r.checkpoint.endswith("ckpt-2.pth") and "Early stop." in lines
    assert m.training
    esv = CK.load(os.path.join(ck, "ckpt-2.pth"))["early_stop_value"]
    assert isinstance(esv, np.float64) and esv == np.float64(-0.70)
    # a new fit over that directory resumes at step 2 with EarlyStopping seeded
    r2 = F.fit(_model(flow, seed=9, num_batches_validate=1), ts, checkpoint_dir=ck, steps=0, batch_size=4,
               validate=FC.scripted([0.1]), log=lines.append)
    assert r2.start_step == 2 and r2.step == 2 and r2.steps == 0
    assert r2.best_loss == np.float64(-0.70) and r2.checkpoint.endswith("ckpt-2.pth")


def test_fit_equals_hand_loop_of_train_step(flow):
    ts = FC.flow_train_set(flow)
    m1 = _model(flow, num_batches_show_loss=3)
    m2 = copy.deepcopy(m1)
    lines = []
    r = F.fit(m1, ts, steps=4, batch_size=4, seed=3, log=lines.append)
    opt = TR.make_optimizer(m2)
    losses = []
    for t in range(1, 5):
        e, a, b = F.batch_of_step(t, len(ts), 4)
        cand, clk = ts.batch(F.epoch_order(3, e, len(ts))[a:b])
        losses.append(TR.train_step(m2, opt, cand, clk))
    assert r.steps == 4 and r.step == 4 and r.start_step == 0
    assert r.losses.dtype == torch.float32 and torch.equal(r.losses, torch.stack(losses))
    FC.assert_same_training_state(m1, r.optimizer, m2, opt)
    # the reference's three numbers (src/train.py:241-244) at step 3
    want = (f"batches 3, current loss {float(losses[2]):.4f}, average loss: "
            f"{np.mean([float(x) for x in losses[:3]]):.4f}, latest average loss: "
            f"{np.mean([float(x) for x in losses[:3]]):.4f}")
    assert lines == [want]


def test_resume_continues_the_uninterrupted_run(flow, tmp_path):
    ts = FC.flow_train_set(flow)
    rising = [0.51, 0.52, 0.53]
    base = _model(flow, num_batches_validate=3)
    quiet = lambda *_: None
    ma = copy.deepcopy(base)
    ra = F.fit(ma, ts, checkpoint_dir=str(tmp_path / "a"), seed=1, steps=6, batch_size=4,
               validate=FC.scripted(rising), log=quiet)
    assert sorted(os.listdir(tmp_path / "a")) == ["ckpt-3.pth", "ckpt-6.pth"]
    mb = copy.deepcopy(base)
    F.fit(mb, ts, checkpoint_dir=str(tmp_path / "b"), seed=1, steps=3, batch_size=4,
          validate=FC.scripted(rising), log=quiet)
    fresh = _model(flow, seed=77, num_batches_validate=3)      # other weights: the checkpoint replaces them
    # default step count: up to num_epochs * S // B = 6 in total, so 3 more
    rb = F.fit(fresh, ts, checkpoint_dir=str(tmp_path / "b"), seed=1, batch_size=4,
               validate=FC.scripted(rising[1:]), log=quiet)
    assert rb.start_step == 3 and rb.steps == 3 and rb.step == 6
    assert torch.equal(ra.losses[3:], rb.losses)
    FC.assert_same_training_state(ma, ra.optimizer, fresh, rb.optimizer)


def test_cli_trains_on_a_directory(tmp_path):
    d = tmp_path / "mind"
    Dt.synthetic_train_split(str(d / "train"), seed=2, n_samples=10, n_news=30, V=50, K=2)
    Dt.synthetic_split(str(d / "val"), seed=3, n_news=30, n_users=5, n_impressions=6, V=64)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")    # on the CPU
    p = subprocess.run([sys.executable, "-m", "newsrecommendationsystem_amd.train", str(d), "--max-steps", "2",
                        "--batch", "4", "--checkpoint-dir", str(tmp_path / "ck")], cwd=FC.ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["steps"] == 2 and out["step"] == 2 and out["steps_per_s"] > 0
    assert out["last_auc"] is None and out["checkpoint"] is None and np.isfinite(out["final_loss"])


def test_load_model_rebuilds_the_checkpoints_model(tmp_path):
    """checkpoint.load_model: the config's vocabulary and embedding width are
    the saved table's, every tensor comes back equal, eval mode."""
    from newsrecommendationsystem_amd import NRMS, NRMSConfig
    torch.manual_seed(3)
    m = NRMS(type("Cfg37", (NRMSConfig,), dict(num_words=37, word_embedding_dim=300)))
    path = str(tmp_path / "ckpt-5.pth")
    CK.save(path, m, torch.optim.Adam(m.parameters(), lr=1e-4), 5, -0.5)
    got = CK.load_model(path, "cpu")
    assert got.config.num_words == 37 and got.config.word_embedding_dim == 300 and not got.training
    want, have = m.state_dict(), got.state_dict()
    assert list(want) == list(have)
    for k, v in want.items():
        assert torch.equal(have[k], v), k
