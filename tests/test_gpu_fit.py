"""The fit loop on the GPU (newsrecommendationsystem_amd/fit.py, csrc/fit.hip):
nrms_train_batch_gather bitwise against the host assembly, nrms_xent_class0
against fp64 (margin: 4 x the error of fp32 ATen on the same inputs), the first
fit step against the existing training path, bitwise determinism and resume
with dropout on, and learning on a planted-teacher split."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from newsrecommendationsystem_amd import checkpoint as CK
from newsrecommendationsystem_amd import data as Dt
from newsrecommendationsystem_amd import train as TR
from oracle import weights as W
from tests import fit_cases as FC
from tests.test_gpu_train import _compare

pytestmark = pytest.mark.gpu
F = FC.F
quiet = lambda *_: None   # noqa: E731


# ------------------------------------------------------------------ batch assembly
def _check_gather(ts, idx, valid=None):
    want_c, want_k = ts.host_batch(idx)
    cand, clk = ts.batch(torch.as_tensor(idx))
    assert cand.is_cuda and cand.dtype == torch.int64 and tuple(cand.shape) == tuple(want_c.shape)
    assert torch.equal(cand.cpu(), want_c) and torch.equal(clk.cpu(), want_k)
    if valid is not None:
        for b, ok in enumerate(valid):
            if not ok:
                assert not cand[b].any() and not clk[b].any()
    return cand, clk


@pytest.mark.parametrize("idx", [[4], list(range(12)), [3, 3, 0, 11, 3]], ids=["B1", "B12", "B5-repeats"])
def test_batch_gather_flow_fixture(device, flow, idx):
    ts = FC.flow_train_set(flow, device)
    cand, clk = _check_gather(ts, idx)
    assert np.array_equal(cand.cpu().numpy(), flow["batch_cand"][idx])
    assert np.array_equal(clk.cpu().numpy(), flow["batch_clicked"][idx])
    again = ts.batch(torch.as_tensor(idx, device=device))
    assert again[0].data_ptr() == cand.data_ptr() and again[1].data_ptr() == clk.data_ptr()   # the set's own buffers


@pytest.mark.parametrize("S,C,N,L,B", [(3, 1, 1, 7, 3), (70, 5, 50, 20, 65)], ids=["odd-L7", "ragged-last-workgroup"])
def test_batch_gather_generated(device, tmp_path, S, C, N, L, B):
    ts = FC.generated_train_set(tmp_path, device, S=S, C=C, N=N, L=L)
    # the host assembly itself against the reference-pinned reader
    corpus = Dt.read_news_parsed(str(tmp_path / "news_parsed.tsv"), num_words_title=L)
    rc, rk, _ = Dt.read_behaviors_parsed(str(tmp_path / "behaviors_parsed.tsv"), corpus, num_clicked=N)
    hc, hk = ts.host_batch(np.arange(S))
    assert np.array_equal(hc.numpy(), rc) and np.array_equal(hk.numpy(), rk)
    _check_gather(ts, F.epoch_order(1, 0, S)[:B])


def test_batch_gather_out_of_range_index_gives_zero_titles(device, flow):
    """An input check, not a fault: the kernel never reads at an index outside
    the set; that sample's titles are zeros and the others stay correct."""
    ts = FC.flow_train_set(flow, device)
    S = len(ts)
    idx = [2, -1, 0, S, 1]
    cand, clk = _check_gather(ts, idx, valid=[True, False, True, False, True])
    for b, s in ((0, 2), (2, 0), (4, 1)):
        assert np.array_equal(cand[b].cpu().numpy(), flow["batch_cand"][s])
        assert np.array_equal(clk[b].cpu().numpy(), flow["batch_clicked"][s])


# ------------------------------------------------------------------ fused loss
def _fp64(z):
    z64 = z.double()
    B = z.shape[0]
    loss = -torch.log_softmax(z64, 1)[:, 0].mean()
    d = torch.softmax(z64, 1)
    d[:, 0] -= 1.0
    return loss, d / B


def _aten_fp32_error(z, loss64, d64):
    """Error of fp32 F.cross_entropy and its autograd on the CPU vs fp64."""
    z32 = z.clone().requires_grad_(True)
    loss = Fn.cross_entropy(z32, torch.zeros(z.shape[0], dtype=torch.long))
    loss.backward()
    return abs(float(loss.detach().double() - loss64)), float((z32.grad.double() - d64).abs().max())


def _check_xent(z, device, tag):
    """The kernel against fp64 at 4 x the measured ATen fp32 error, floored at
    4 ulp of the loss (for dlogits: 4 ulp of 1 / B, the scale of an entry
    (softmax - onehot) / B). Returns (kernel errors, ATen errors)."""
    loss64, d64 = _fp64(z)
    a_loss, a_d = _aten_fp32_error(z, loss64, d64)
    loss, d = F.xent_class0(z.to(device))
    k_loss = abs(float(loss.cpu().double()[0] - loss64))
    k_d = float((d.cpu().double() - d64).abs().max())
    tol_loss = max(4 * a_loss, 4 * float(np.spacing(np.float32(abs(float(loss64))))))
    tol_d = max(4 * a_d, 4 * float(np.spacing(np.float32(1.0 / z.shape[0]))))
    print(f"xent {tag}: loss err kernel {k_loss:.3e} aten {a_loss:.3e} tol {tol_loss:.3e}; "
          f"dlogits err kernel {k_d:.3e} aten {a_d:.3e} tol {tol_d:.3e}")
    assert k_loss <= tol_loss, (tag, k_loss, tol_loss)
    assert k_d <= tol_d, (tag, k_d, tol_d)
    return (k_loss, k_d), (a_loss, a_d)


def test_xent_flow_fixture(device, flow):
    z = torch.from_numpy(flow["grad_logits"]).float()
    loss, _ = F.xent_class0(z.to(device))
    assert abs(float(loss.cpu()[0]) - float(flow["grad_loss"])) <= 1e-6
    _check_xent(z, device, "flow")


@pytest.mark.parametrize("C", [1, 3, 5, 65])
@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 257])
def test_xent_random_logits(device, B, C):
    g = torch.Generator().manual_seed(1000 * B + C)
    z = torch.randn(B, C, generator=g) * 3.0
    _check_xent(z, device, f"B{B}-C{C}")
    zd = z.to(device)
    l1, d1 = F.xent_class0(zd)
    l2, d2 = F.xent_class0(zd)
    assert torch.equal(l1, l2) and torch.equal(d1, d2)          # fixed summation order
    if C == 1:
        assert float(l1.cpu()[0]) == 0.0 and not d1.any()


def test_xent_wide_logits_inf_and_loss_slot(device):
    g = torch.Generator().manual_seed(7)
    z = (torch.rand(9, 5, generator=g) * 160.0 - 80.0)
    z[0, 0], z[0, 1] = -80.0, 80.0                              # exp(z) alone would overflow / underflow
    _check_xent(z, device, "spread +-80")
    loss, d = F.xent_class0(z.to(device))
    assert torch.isfinite(loss).all() and torch.isfinite(d).all()
    zi = z.clone()
    zi[3, 2] = float("inf")
    assert torch.isnan(Fn.cross_entropy(zi, torch.zeros(9, dtype=torch.long)))      # as torch does
    loss, _ = F.xent_class0(zi.to(device))
    assert torch.isnan(loss).all()
    # the loss goes where the caller points (a slot of the fit loop's device log)
    log = torch.full((4,), -1.0, device=device)
    F.xent_class0(z.to(device), loss_out=log[2:3])
    want, _ = F.xent_class0(z.to(device))
    assert log.cpu().tolist() == [-1.0, -1.0, float(want.cpu()[0]), -1.0]


# ------------------------------------------------------------------ the loop
V_FIT = 512


@pytest.fixture(scope="module")
def small_set(device, tmp_path_factory):
    """S = 16, C = 3, N = 50, L = 20 over V = 512."""
    return FC.generated_train_set(tmp_path_factory.mktemp("fit_small"), device, S=16, C=3, N=50, L=20,
                                  n_news=60, V=V_FIT, seed=4)


def _gpu_model(device, p, seed=51, **fields):
    from newsrecommendationsystem_amd import NRMS, NRMSConfig
    m = NRMS(FC.with_cfg(NRMSConfig, num_words=V_FIT, dropout_probability=p, **fields))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.nrms_state(seed, V_FIT).items()})
    return m.to(device).train()


@pytest.mark.parametrize("host_batches", [False, True], ids=["device", "host_batches"])
def test_first_fit_step_matches_existing_path(device, small_set, host_batches):
    B = 8
    m = _gpu_model(device, 0.0)
    ref = copy.deepcopy(m)
    got = {}
    for n, p in m.named_parameters():
        p.register_hook(lambda g, n=n: got.__setitem__(n, g.detach().clone()))
    r = F.fit(m, small_set, steps=1, batch_size=B, seed=0, log=quiet, host_batches=host_batches)
    cand, clk = small_set.host_batch(F.epoch_order(0, 0, len(small_set))[:B])
    loss = TR.loss_fn(ref.forward_ids(cand.to(device), clk.to(device)))
    loss.backward()
    want = {n: p.grad for n, p in ref.named_parameters()}
    assert set(got) == set(want)
    _compare(got, want)
    assert abs(float(r.losses[0]) - float(loss.detach())) <= 1e-6
    assert type(r.optimizer).__name__ == "HipAdam"
    assert not torch.equal(m.news_encoder.additive_attention.linear.weight,
                           ref.news_encoder.additive_attention.linear.weight)      # the update ran


def test_fit_is_bitwise_deterministic_with_dropout(device, small_set):
    base = _gpu_model(device, 0.2)
    runs = []
    for seed in (5, 5, 6):
        m = copy.deepcopy(base)
        runs.append((m, F.fit(m, small_set, steps=4, batch_size=4, seed=seed, log=quiet)))
    (ma, ra), (mb, rb), (mc, rc) = runs
    assert torch.equal(ra.losses, rb.losses) and torch.isfinite(ra.losses).all()
    FC.assert_same_training_state(ma, ra.optimizer, mb, rb.optimizer)
    assert not torch.equal(ra.losses, rc.losses)
    assert any(not torch.equal(p, q) for p, q in zip(ma.parameters(), mc.parameters()))


def test_fit_resume_is_bitwise_with_dropout(device, small_set, tmp_path):
    """Holds only if the order and the dropout seeds are functions of
    (seed, step), not of how many steps this process has run."""
    rising = [0.51, 0.52, 0.53]
    base = _gpu_model(device, 0.2, num_batches_validate=3)
    ma = copy.deepcopy(base)
    ra = F.fit(ma, small_set, checkpoint_dir=str(tmp_path / "a"), seed=1, steps=6, batch_size=4,
               validate=FC.scripted(rising), log=quiet)
    mb = copy.deepcopy(base)
    F.fit(mb, small_set, checkpoint_dir=str(tmp_path / "b"), seed=1, steps=3, batch_size=4,
          validate=FC.scripted(rising), log=quiet)
    assert sorted(os.listdir(tmp_path / "b")) == ["ckpt-3.pth"]
    fresh = _gpu_model(device, 0.2, seed=52, num_batches_validate=3)
    rb = F.fit(fresh, small_set, checkpoint_dir=str(tmp_path / "b"), seed=1, steps=3, batch_size=4,
               validate=FC.scripted(rising[1:]), log=quiet)
    assert rb.start_step == 3 and rb.step == 6
    assert torch.equal(ra.losses[3:], rb.losses)
    FC.assert_same_training_state(ma, ra.optimizer, fresh, rb.optimizer)


def test_fit_learns_a_planted_teacher_and_its_checkpoint_scores(device, tmp_path):
    from newsrecommendationsystem_amd import NRMS, quality as Q
    from newsrecommendationsystem_amd.evaluate import evaluate
    d = str(tmp_path / "val")
    cfg, teacher, corpus, titles, student = Q.setup(d, V=600, n_news=300, n_users=100, n_impressions=120)
    N, B, steps = cfg.num_clicked_news_a_user, 16, 30

    def positive(cands, hists):            # the teacher's top-scored candidate goes first (class 0)
        clk = np.zeros((len(hists), N, titles.shape[1]), np.int64)
        for k, h in enumerate(hists):
            h = h[:N]
            if len(h):
                clk[k, N - len(h):] = titles[h]
        with torch.no_grad():
            y = teacher.forward_ids(torch.from_numpy(titles[cands]), torch.from_numpy(clk))
        return y.argmax(1).cpu().numpy()
    tr = str(tmp_path / "train")
    Dt.synthetic_train_split(tr, seed=1, n_samples=B * steps, titles=titles, K=2, positive=positive)
    ts = F.TrainSet(os.path.join(tr, "behaviors_parsed.tsv"), corpus, device=device)
    student = student.to(device)
    student.config = FC.with_cfg(cfg, num_batches_validate=10, num_batches_show_loss=10)
    ck = str(tmp_path / "ck")
    r = F.fit(student, ts, d, checkpoint_dir=ck, steps=steps, batch_size=B, log=quiet)
    losses = r.losses.numpy()
    print("planted-teacher fit losses:", np.round(losses, 4).tolist(), "aucs:", r.aucs)
    assert r.steps == steps and np.isfinite(losses).all()
    assert losses[-5:].mean() < losses[:5].mean(), losses
    assert [s for s, _ in r.aucs] == [10, 20, 30] and os.path.exists(os.path.join(ck, "ckpt-10.pth"))
    # the checkpoint the run wrote resumes and scores through evaluate()
    m = NRMS(cfg).to(device)
    step, esv = CK.resume(r.checkpoint, m, TR.make_optimizer(m))
    assert isinstance(esv, np.float64) and r.checkpoint == CK.latest_checkpoint(ck)
    auc = evaluate(m.eval(), d)[0]
    assert 0.0 <= auc <= 1.0 and auc == pytest.approx(dict(r.aucs)[step], abs=1e-9) and -esv == dict(r.aucs)[step]
